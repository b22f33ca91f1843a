"""Population rollouts (brov_rollout_pop / engine.rollout_pop), ensemble statistics (brov_ensemble_stats_dev) and
simulate_population on the GPU, against oracle/fossen_params.py at the vehicles of tests/fossen_vehicles.py.

Inputs are the recipe of tests/test_fossen_params_gpu.py: rollout_inputs (same seeds, DT = 0.02), the error is that file's mixed
error and the bound its TOL_ROLL = 1e-10.  Every oracle comparison also runs the oracle in np.longdouble on the same inputs and
asserts, as that file's report() does, that fp64 and long double stay within a tenth of the bound."""
import ctypes
import functools

import numpy as np
import pytest

import fossen_vehicles as fv
from oracle import fossen_params as fp

pytestmark = pytest.mark.gpu

TOL_ROLL = 1e-10
L = np.longdouble
B, T, DT = 300, 24, 0.02                  # one full 256-lane block plus a ragged one
INTEG = {"euler": fp.EULER, "rk4": fp.RK4}
THRUSTER_POP = ("V0", "V5", "V6", "V8", "V7")
WRENCH_POP = ("V0", "V1", "V4", "V5", "V7")


def err(a, b):
    """max |a-b| / max(1, |b|), formed in long double"""
    a, b = np.asarray(a, dtype=L), np.asarray(b, dtype=L)
    return float(np.max(np.abs(a - b) / np.maximum(L(1), np.abs(b)))) if a.size else 0.0


def report(what, kernel_err, gap, bound):
    print(f"{what}: kernel err {kernel_err:.2e}  oracle fp64-vs-long-double gap {gap:.2e}  bound {bound:.0e}")
    assert gap < 0.1 * bound, (what, "inputs too hard for fp64", gap)
    assert kernel_err < bound, (what, kernel_err)


@pytest.fixture(scope="module")
def eng():
    from bluerov2_dynamics_amd import engine
    return engine


@pytest.fixture(scope="module")
def ctx():
    from bluerov2_dynamics_amd import _lib
    c = _lib.Context(0)
    yield c
    c.close()


def _bytes(p):
    return ctypes.string_at(ctypes.byref(p), ctypes.sizeof(p))


def _params(names):
    return [fv.params(n) for n in names]


# ------------------------------------------------------------------------------------------ shared inputs and oracle results
@functools.lru_cache(maxsize=None)
def rollout_inputs(model, T=T):
    """tests/test_fossen_params_gpu.py: rollout_inputs"""
    rng = np.random.default_rng(400 + model + T)
    X0 = rng.uniform(-0.5, 0.5, (B, fp.NX[model]))
    if model == 2:
        X0[:, 3:7] /= np.linalg.norm(X0[:, 3:7], axis=1, keepdims=True)
    U = rng.uniform(-1, 1, (B, T, fp.NU[model])) * (1.0 if model == 0 else 15.0)
    return X0, U, rng.uniform(-1, 1, (B, 8, 3))


@functools.lru_cache(maxsize=None)
def oracle(name, model, integ, lag_mode, ld=False, T=T, rows=B, steps=None, sub=1, zero_lag=False):
    """the oracle for vehicle `name` on the first `rows` trajectories and `steps` steps (default T) of rollout_inputs(model, T)"""
    X0, U, lag0 = rollout_inputs(model, T)
    steps = T if steps is None else steps
    return fp.rollout(model, INTEG[integ], lag_mode, fv.vehicle(name), X0[:rows], U[:rows, :steps], DT,
                      lag=None if (zero_lag or model != 0) else lag0[:rows], sub=sub, dtype=L if ld else np.float64)


def _check(what, r, names, model, integ, lag_mode, lag=True, **kw):
    """every candidate of a population result against the oracle of its vehicle"""
    e = gap = 0.0
    for j, n in enumerate(names):
        o, ol = oracle(n, model, integ, lag_mode, **kw), oracle(n, model, integ, lag_mode, ld=True, **kw)
        e, gap = max(e, err(r["xT"][j], o["xT"])), max(gap, err(o["xT"], ol["xT"]))
        if r["traj"] is not None:
            e, gap = max(e, err(r["traj"][j], o["traj"])), max(gap, err(o["traj"], ol["traj"]))
        if lag:
            e, gap = max(e, err(r["lag"][j], o["lag"])), max(gap, err(o["lag"], ol["lag"]))
    report(what, e, gap, TOL_ROLL)


# ------------------------------------------------------------------------------------------ 1, 2, 3: mixed populations
@pytest.mark.parametrize("integ,lag_mode", [("euler", 0), ("rk4", 0), ("rk4", 1)])
def test_mixed_population_thruster(eng, ctx, integ, lag_mode):
    """[V0, V5 (current), V6 (dense allocation), V8 (no observer form), V7 (everything)] in one launch, B = 300 (a full block and a
    ragged one), T = 24, start lag given: traj, xT and the end lag of every candidate."""
    X0, U, lag0 = rollout_inputs(0)
    r = eng.rollout_pop(0, integ, _params(THRUSTER_POP), X0, U, DT, lag=np.broadcast_to(lag0, (5,) + lag0.shape), lag_mode=lag_mode, ctx=ctx)
    assert r["traj"].shape == (5, B, T + 1, 12) and r["xT"].shape == (5, B, 12) and r["lag"].shape == (5, B, 8, 3)
    _check(f"pop thruster {integ} lag_mode {lag_mode}", r, THRUSTER_POP, 0, integ, lag_mode)


@pytest.mark.parametrize("model", [1, 2])
def test_mixed_population_wrench(eng, ctx, model):
    """WRENCH_EULER and WRENCH_QUAT, [V0, V1, V4 (xb, yb), V5 (current), V7], RK4, same shape."""
    X0, U, _ = rollout_inputs(model)
    r = eng.rollout_pop(model, "rk4", _params(WRENCH_POP), X0, U, DT, ctx=ctx)
    assert r["traj"].shape == (5, B, T + 1, fp.NX[model]) and r["lag"] is None
    _check(f"pop wrench model {model} rk4", r, WRENCH_POP, model, "rk4", 0, lag=False)


def test_candidate_index_matters():
    """On the oracle alone: the end states of any two distinct vehicles of the two tests above are more than 1e3 x the bound
    apart, so a kernel that ignored blockIdx.y (every candidate under one vehicle) cannot pass them."""
    for model, names, cases in ((0, THRUSTER_POP, (("euler", 0), ("rk4", 0), ("rk4", 1))), (1, WRENCH_POP, (("rk4", 0),)),
                                (2, WRENCH_POP, (("rk4", 0),))):
        for integ, lag_mode in cases:
            for i, a in enumerate(names):
                for b in names[i + 1:]:
                    d = err(oracle(a, model, integ, lag_mode)["xT"], oracle(b, model, integ, lag_mode)["xT"])
                    assert d > 1e3 * TOL_ROLL, (model, integ, lag_mode, a, b, d)


# ------------------------------------------------------------------------------------------ 4: small batches and strides
def test_one_trajectory_per_vehicle(eng, ctx):
    """B = 1, P = 70: the 64-lane block path, per-candidate inputs (70 scenarios, vehicles cycling V0..V8), start lag given."""
    X0, U, lag0 = rollout_inputs(0)
    P = 70
    names = [fv.NAMES[j % len(fv.NAMES)] for j in range(P)]
    r = eng.rollout_pop(0, "rk4", _params(names), X0[:P, None], U[:P, None], DT, lag=lag0[:P, None], per_candidate=True, ctx=ctx)
    assert r["traj"].shape == (P, 1, T + 1, 12)
    e = gap = 0.0
    for n in fv.NAMES:                                                  # one oracle run per vehicle, over all 70 scenarios
        o, ol = oracle(n, 0, "rk4", 0, rows=P), oracle(n, 0, "rk4", 0, ld=True, rows=P)
        js = [j for j in range(P) if names[j] == n]
        for k in ("traj", "xT", "lag"):
            e, gap = max(e, err(r[k][js, 0], o[k][js])), max(gap, err(o[k], ol[k]))
    report("pop B=1 P=70 per-candidate", e, gap, TOL_ROLL)


def test_small_batch_strides_and_empty_horizon(eng, ctx):
    """B = 65, P = 2 (the smallest batch that takes the 256-lane blocks); stride = 5 with T = 24 (T no multiple of the stride:
    5 rows); store=False (xT alone); T = 0 (xT == x0, one trajectory row, lag unchanged)."""
    X0, U, lag0 = rollout_inputs(0)
    names, n = ("V0", "V7"), 65
    lag = np.broadcast_to(lag0[:n], (2, n, 8, 3))
    r = eng.rollout_pop(0, "rk4", _params(names), X0[:n], U[:n], DT, lag=lag, ctx=ctx)
    _check("pop B=65 P=2", r, names, 0, "rk4", 0, rows=n)
    r = eng.rollout_pop(0, "rk4", _params(names), X0[:n], U[:n], DT, lag=lag, stride=5, ctx=ctx)
    assert r["traj"].shape == (2, n, 5, 12)
    _check("pop stride 5", r, names, 0, "rk4", 0, rows=n, sub=5)
    r = eng.rollout_pop(0, "rk4", _params(names), X0[:n], U[:n], DT, lag=lag, store=False, ctx=ctx)
    assert r["traj"] is None
    _check("pop store=False", r, names, 0, "rk4", 0, rows=n)
    r = eng.rollout_pop(0, "rk4", _params(names), X0[:n], U[:n, :0], DT, lag=lag, ctx=ctx)
    assert r["traj"].shape == (2, n, 1, 12)
    for j in range(2):
        assert np.array_equal(r["xT"][j], X0[:n]) and np.array_equal(r["traj"][j, :, 0], X0[:n]) and np.array_equal(r["lag"][j], lag0[:n])


# ------------------------------------------------------------------------------------------ 5: long horizon
def test_long_horizon_across_trig_refreshes(eng, ctx):
    """T = 130, B = 70, [V0, V7], thruster RK4: past two multiples of the rollout kernels' TRIG_REFRESH = 64.  (The long-double
    guard holds for these inputs at T = 130: checked on the CPU, gap printed below.)"""
    X0, U, lag0 = rollout_inputs(0, 130)
    names, n = ("V0", "V7"), 70
    r = eng.rollout_pop(0, "rk4", _params(names), X0[:n], U[:n], DT, lag=np.broadcast_to(lag0[:n], (2, n, 8, 3)), ctx=ctx)
    _check("pop T=130", r, names, 0, "rk4", 0, T=130, rows=n)


# ------------------------------------------------------------------------------------------ 6, 7: exact identities
def _same(a, b):
    return all((a[k] is None and b[k] is None) or np.array_equal(np.asarray(a[k]), np.asarray(b[k])) for k in ("traj", "xT", "lag"))


def test_exact_identities(eng, ctx):
    """P copies of one vehicle give P identical blocks; shared inputs == the same inputs replicated per candidate; device-array
    and host-array paths agree; two runs agree; the ctx's own parameters are the same bytes before and after."""
    X0, U, lag0 = rollout_inputs(0)
    before = _bytes(ctx.get_params())
    same = eng.rollout_pop(0, "rk4", _params(("V7",) * 3), X0, U, DT, lag=np.broadcast_to(lag0, (3,) + lag0.shape), ctx=ctx)
    for k in ("traj", "xT", "lag"):
        assert np.array_equal(same[k][0], same[k][1]) and np.array_equal(same[k][0], same[k][2]), k
    names = ("V0", "V5", "V7")
    lag = np.ascontiguousarray(np.broadcast_to(lag0, (3,) + lag0.shape))
    shared = eng.rollout_pop(0, "rk4", _params(names), X0, U, DT, lag=lag, ctx=ctx)
    again = eng.rollout_pop(0, "rk4", _params(names), X0, U, DT, lag=lag, ctx=ctx)
    assert _same(shared, again)
    rep = eng.rollout_pop(0, "rk4", _params(names), np.broadcast_to(X0, (3,) + X0.shape), np.broadcast_to(U, (3,) + U.shape), DT,
                          lag=lag, per_candidate=True, ctx=ctx)
    assert _same(shared, rep)
    up = lambda a: eng.DevArray.from_host(ctx, a)
    dev = eng.rollout_pop(0, "rk4", _params(names), up(X0), up(U), DT, lag=up(lag), ctx=ctx)
    assert isinstance(dev["traj"], eng.DevArray)
    assert _same(shared, {k: v.numpy() for k, v in dev.items()})
    assert np.array_equal(shared["xT"][2], same["xT"][0])          # V7 as candidate 2 of 3 vehicles == V7 as candidate 0 of 3 copies
    assert _bytes(ctx.get_params()) == before


@pytest.mark.parametrize("integ,lag_mode", [("euler", 0), ("rk4", 0), ("rk4", 1)])
def test_resume_is_bit_exact(eng, ctx, integ, lag_mode):
    """Thruster model with lag_io: T = 12 followed by T = 12 from the returned xT and lag equals one T = 24 call bit for bit, per
    candidate (the body state and the per-thruster lag state are the whole checkpoint)."""
    X0, U, lag0 = rollout_inputs(0)
    ps = _params(THRUSTER_POP)
    lag = np.broadcast_to(lag0, (5,) + lag0.shape)
    full = eng.rollout_pop(0, integ, ps, X0, U, DT, lag=lag, lag_mode=lag_mode, ctx=ctx)
    a = eng.rollout_pop(0, integ, ps, X0, U[:, :12], DT, lag=lag, lag_mode=lag_mode, ctx=ctx)
    b = eng.rollout_pop(0, integ, ps, a["xT"], np.broadcast_to(U[:, 12:], (5, B, 12, 8)), DT, lag=a["lag"], lag_mode=lag_mode,
                        per_candidate=True, ctx=ctx)
    assert np.array_equal(b["xT"], full["xT"]) and np.array_equal(b["lag"], full["lag"])
    assert np.array_equal(np.concatenate([a["traj"], b["traj"][:, :, 1:]], axis=2), full["traj"])


# ------------------------------------------------------------------------------------------ 8: errors
def test_refused_arguments(eng, ctx):
    """BROV_ERR_ARG with a message, checked on the host before anything is launched."""
    from bluerov2_dynamics_amd import _lib
    X0, U, _ = rollout_inputs(0)
    x0, u = X0[:1], U[:1]
    singular = fv.params("V0")
    singular.m = singular.added_mass[0]
    cases = [("a double-integrator model", dict(model=_lib.DI_THRUSTER_EULER, params=_params(("V0",))),
              "brov_rollout_pop: the double-integrator gains are not brov_params"),
             ("P = 65536", dict(params=[fv.params("V0")] * 65536), "brov_rollout_pop: P must be <= 65535"),
             ("a singular mass matrix", dict(params=[fv.params("V0"), singular]), "candidate 1: singular mass matrix"),
             ("stride = 0 with traj", dict(params=_params(("V0",)), stride=0), "brov_rollout_pop: traj_stride must be >= 1")]
    for what, kw, text in cases:
        with pytest.raises(_lib.BrovError, match=r"BROV_ERR_ARG: \S") as ei:
            eng.rollout_pop(kw.get("model", 0), "rk4", kw["params"], x0, u, DT, stride=kw.get("stride", 1), ctx=ctx)
        print(what, "->", ei.value)
        assert text in str(ei.value), (what, ei.value)
    r = eng.rollout_pop(0, "rk4", [], x0, u, DT, ctx=ctx)              # P = 0: nothing to do
    assert r["xT"].shape == (0, 1, 12)


# ------------------------------------------------------------------------------------------ 9: ensemble statistics
def _stats_ref(v):
    v = np.asarray(v, dtype=L)
    P = v.shape[0]
    mean = v.sum(0) / P
    std = np.sqrt(((v - mean) ** 2).sum(0) / (P - 1)) if P > 1 else np.zeros_like(mean)
    return mean, std


@pytest.mark.parametrize("shape", [(5, 1000), (1, 7)])
def test_ensemble_stats(eng, ctx, shape):
    """mean, sample standard deviation, minimum, maximum over the candidates against a long-double computation: min and max
    exact, mean within P 2^-52 mean_j|v|, std within 4 P 2^-52 max_j|v| (the bound of a sequential sum, not a measured figure)."""
    rng = np.random.default_rng(9)
    v = rng.normal(0, 1, shape) * 10.0 ** rng.uniform(-3, 3, shape[1])
    P = shape[0]
    s = eng.ensemble_stats(v, ctx=ctx)
    mean, std = _stats_ref(v)
    assert all(s[k].shape == (shape[1],) for k in ("mean", "std", "min", "max"))
    assert np.array_equal(s["min"], v.min(0)) and np.array_equal(s["max"], v.max(0))
    em = np.abs(s["mean"].astype(L) - mean) - P * L(2.0) ** -52 * np.abs(v).astype(L).mean(0)
    es = np.abs(s["std"].astype(L) - std) - 4 * P * L(2.0) ** -52 * np.abs(v).max(0).astype(L)
    print(f"ensemble_stats {shape}: mean err - bound max {float(em.max()):.2e}, std err - bound max {float(es.max()):.2e}")
    assert np.all(em <= 0) and np.all(es <= 0)
    if P == 1:
        assert np.array_equal(s["std"], np.zeros(shape[1])) and np.array_equal(s["mean"], v[0])
    # two runs: the same bits; a device array in gives device arrays out with the same bits
    d = eng.ensemble_stats(eng.DevArray.from_host(ctx, v), ctx=ctx)
    assert all(np.array_equal(d[k].numpy(), s[k]) for k in s)


def test_ensemble_stats_non_finite(eng, ctx):
    """one inf and one NaN make exactly their columns NaN in all four rows"""
    rng = np.random.default_rng(10)
    v = rng.normal(0, 1, (5, 1000))
    clean = eng.ensemble_stats(v, ctx=ctx)
    v[3, 17], v[0, 900] = np.inf, np.nan
    s = eng.ensemble_stats(v, ctx=ctx)
    bad = np.zeros(1000, dtype=bool)
    bad[[17, 900]] = True
    for k in ("mean", "std", "min", "max"):
        assert np.array_equal(np.isnan(s[k]), bad), k
        assert np.array_equal(s[k][~bad], clean[k][~bad]), k


# ------------------------------------------------------------------------------------------ 10: the vehicle class
def test_simulate_population():
    """rov.simulate_population for [V0, V2] equals simulate on vehicles that were given those parameters, and leaves rov's own
    parameters and lag as they were."""
    from bluerov2_dynamics_amd.fossen.BlueROV2 import BlueROV2
    from bluerov2_dynamics_amd.fossen import identify
    X0, U, _ = rollout_inputs(0)
    x0, u = X0[0], U[0]
    rov = BlueROV2()
    rov.simulate(x0, u[:5], DT, integrator="rk4")                       # a non-zero lag state of its own
    lag_before, params_before = np.array(rov._lag), _bytes(identify.params_of(rov))
    ps = _params(("V0", "V2"))
    pop = rov.simulate_population(x0, u, DT, ps, integrator="rk4")
    assert pop.shape == (2, T + 1, 12)
    assert np.array_equal(rov._lag, lag_before) and _bytes(identify.params_of(rov)) == params_before
    for j, p in enumerate(ps):
        other = BlueROV2()
        for name in identify.FREE_NAMES:
            if name not in identify._CURRENT:
                setattr(other, name, identify.get_param(p, name))
        ref = other.simulate(x0, u, DT, integrator="rk4")
        e = err(pop[j], ref)
        print(f"simulate_population candidate {j}: err {e:.2e}")
        assert e < TOL_ROLL
    assert err(pop[0], pop[1]) > 1e3 * TOL_ROLL


# ------------------------------------------------------------------------------------------ the covariance on the device path
def test_fit_covariance_device_path(eng, ctx):
    """fit_parameters(covariance=True) with the engine as evaluator (end states stay on the device, J^T J from
    brov_fd_normal_eq_dev, one download for r^T r) against the same call with the end states handed back as NumPy arrays
    (normal_eq_numpy).  iters=0, so both evaluate the covariance at the same point and differ only in the order in which the
    R = W nx products of every entry of J^T J are added.  Either order is within R u (u = 2^-53) of the exact sum relative to
    sum_r |J_ri J_rj| <= sqrt(A_ii A_jj) (A = J^T J), so the two are within 2 R u entrywise once A is scaled to a unit diagonal.
    The inverse amplifies a relative perturbation by the condition number; in the scaled form that is the condition of the
    parameters' correlation matrix (within a factor m of the best diagonal scaling, van der Sluis), and a factor m lies between
    the entrywise and the spectral norm: |C_dev - C_host|_ij / sqrt(C_ii C_jj) <= 2 m^2 R u cond(corr); s^2 adds one more R u,
    covered by rounding the factor up to 4."""
    from bluerov2_dynamics_amd.fossen import identify
    rng = np.random.default_rng(12)
    N, Hw = 300, 5
    U = 0.5 * np.sin(np.cumsum(rng.normal(0, 0.05, (N, 6)), 0)) * np.array([20.0, 20.0, 20.0, 2.0, 2.0, 2.0])
    truth = fv.params("V2")
    X = eng.rollout_pop(1, "euler", [truth], np.zeros((1, 12)), U[None, :N - 1], DT, ctx=ctx)["traj"][0, 0] + rng.normal(0, 1e-4, (N, 12))

    def host_evaluator(model, integrator, params_list, X_, U_, H_, dt, carry_lag=True, endpoints=False):
        out = eng.window_pop(model, integrator, params_list, X_, U_, H_, dt, carry_lag=carry_lag, endpoints=endpoints, ctx=ctx)
        return (out[0], out[1].numpy()) if endpoints else out
    free = ("Xu", "Yv", "Zw_abs")
    kw = dict(H=Hw, free=free, iters=0, model=1, covariance=True)
    base = fv.params("V0")
    base._ctx = ctx
    dev = identify.fit_parameters(base, X, U, DT, **kw)
    host = identify.fit_parameters(fv.params("V0"), X, U, DT, evaluator=host_evaluator, **kw)
    assert dev.params == host.params and dev.n_evals == host.n_evals == len(free) + 1
    assert dev.covariance.shape == (3, 3) and np.all(np.isfinite(dev.covariance)) and np.all(np.diag(dev.covariance) > 0)
    sd = np.sqrt(np.diag(host.covariance))
    R, m = (N - Hw) * 12, len(free)
    cond = np.linalg.cond(host.covariance / np.outer(sd, sd))
    bound = 4 * m * m * R * 2.0 ** -53 * cond
    e = np.max(np.abs(dev.covariance - host.covariance) / np.outer(sd, sd))
    print(f"covariance device vs host path: {e:.2e}, cond of the correlation matrix {cond:.1e}, bound {bound:.1e}")
    assert bound < 1e-6, "the problem is too ill-conditioned for this comparison to say anything"
    assert e < bound
