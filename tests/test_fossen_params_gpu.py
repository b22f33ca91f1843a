"""GPU parity at NON-nominal vehicles: brov_rhs, brov_thruster_forces, the rollout kernels (every layout, both thruster-model
implementations, both BTU staging modes, tracked and untracked lag), the window evaluator and its population form, against
oracle/fossen_params.py -- an fp64 NumPy restatement of the reference's formulas that takes the vehicle as an argument and
shares none of the constants csrc/capi.hip folds (md, E[12], G, XY, Tm = Minv T, the lag powers, the observer basis).  That
oracle is pinned on the CPU against the reference itself (tests/test_oracle_golden.py, tests/golden/fossen_vehicles.npz).

The vehicles are tests/fossen_vehicles.py's V0..V8; between them they reach every structural switch of derive_fast()
(has_xy, has_current, tm_dense, obs_bad) and the default kernels at non-default constants.

Bounds are the project's existing ones (conftest.rel_err, the mixed error): 1e-11 per call, 1e-10 on rollouts, 1e-9 per window
and 1e-8 on a window total.  Every test also evaluates the oracle in np.longdouble on the same inputs, prints that gap beside
the kernel's error and asserts that the gap stays below a tenth of the bound: the inputs are then not too hard for fp64 itself."""
import ctypes
import functools

import numpy as np
import pytest

import fossen_vehicles as fv
from oracle import fossen_params as fp

pytestmark = pytest.mark.gpu

TOL_CALL = 1e-11
TOL_ROLL = 1e-10
TOL_WIN = 1e-9
TOL_SE = 1e-8
L = np.longdouble
B, T, DT = 300, 24, 0.02                  # one full 256-lane block plus a ragged one
NWIN, H_MAX = 257, 10
INTEG = {"euler": fp.EULER, "rk4": fp.RK4}


def err(a, b):
    """conftest.rel_err's mixed error max |a-b| / max(1, |b|), formed in long double"""
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


# ------------------------------------------------------------------------------------------ shared inputs and oracle results
@functools.lru_cache(maxsize=None)
def rhs_inputs(model):
    rng = np.random.default_rng(300 + model)
    X = rng.uniform(-1.2, 1.2, (B, fp.NX[model]))
    U = rng.uniform(-1, 1, (B, fp.NU[model])) * (1.0 if model == 0 else 20.0)
    return X, U, rng.uniform(-2, 2, (B, 8, 3))


@functools.lru_cache(maxsize=None)
def oracle_rhs(name, model, ld=False):
    X, U, lag0 = rhs_inputs(model)
    return fp.rhs(model, fv.vehicle(name), X, U, DT, lag=lag0, dtype=L if ld else np.float64)


@functools.lru_cache(maxsize=None)
def rollout_inputs(model, T=T):
    rng = np.random.default_rng(400 + model + T)
    X0 = rng.uniform(-0.5, 0.5, (B, fp.NX[model]))
    if model == 2:
        X0[:, 3:7] /= np.linalg.norm(X0[:, 3:7], axis=1, keepdims=True)
    U = rng.uniform(-1, 1, (B, T, fp.NU[model])) * (1.0 if model == 0 else 15.0)
    return X0, U, rng.uniform(-1, 1, (B, 8, 3))


@functools.lru_cache(maxsize=None)
def oracle_rollout(name, model, integ, lag_mode, zero_lag, ld=False, dt=DT, T=T):
    X0, U, lag0 = rollout_inputs(model, T)
    return fp.rollout(model, INTEG[integ], lag_mode, fv.vehicle(name), X0, U, dt, lag=None if (zero_lag or model != 0) else lag0,
                      dtype=L if ld else np.float64)


def _smooth(rng, N, nu):
    U = 0.5 * np.sin(np.cumsum(rng.normal(0, 0.05, (N, nu)), 0))            # smooth, bounded commands
    return U if nu == 8 else U * np.array([20.0, 20.0, 20.0, 2.0, 2.0, 2.0])


@functools.lru_cache(maxsize=None)
def recording(name, model, N=NWIN + H_MAX):
    """the recipe of test_window_se_vs_oracle_chunk_edges: smooth commands, states = an oracle rollout of that vehicle + 1e-3 noise.
    The rollout restarts from rest every 256 rows: left running for 4100 steps, V1 (heavier than the water it displaces) tumbles
    through theta = -pi/2, where two windows are too ill-conditioned for fp64 itself (fp64 and long double 5e-9 apart)."""
    rng = np.random.default_rng(500 + model + N)
    U = _smooth(rng, N, fp.NU[model])
    x0 = np.zeros((1, fp.NX[model]))
    if model == 2:
        x0[0, 3] = 1.0
    X = np.concatenate([fp.rollout(model, fp.EULER, 0, fv.vehicle(name), x0, U[None, a:a + 256], DT)["traj"][0][1:] for a in range(0, N, 256)])
    return np.ascontiguousarray(X + rng.normal(0, 1e-3, (N, fp.NX[model]))), np.ascontiguousarray(U)


@functools.lru_cache(maxsize=None)
def oracle_windows(name, rec_name, model, integ, carry, H, ld=False, N=NWIN + H_MAX):
    """(se, per_window, endpoints) of vehicle `name` over ALL windows of rec_name's recording.  Window k depends on X[k], on
    U[k:k+H] and, through the carried lag, on U[:k+H-1] only: the first n windows of the full run are the windows of the
    recording cut to n + H rows, so the shorter cases below slice this result."""
    X, U = recording(rec_name, model, N)
    return fp.window_endpoints(model, INTEG[integ], fv.vehicle(name), X, U, H, DT, carry_lag=carry, dtype=L if ld else np.float64)


# ------------------------------------------------------------------------------------------ RHS and thruster forces
@pytest.mark.parametrize("name", fv.NAMES)
def test_rhs_and_thruster_forces(eng, ctx, name):
    """brov_rhs for models 0, 1, 2 and brov_thruster_forces, random lag state, lag included."""
    ctx.set_params(fv.params(name))
    for model in (0, 1, 2):
        X, U, lag0 = rhs_inputs(model)
        (o, lo), (ol, lol) = oracle_rhs(name, model), oracle_rhs(name, model, True)
        xd, lag = eng.rhs(model, X, U, DT, lag=lag0 if model == 0 else None, ctx=ctx)
        report(f"{name} rhs model {model}", err(xd, o), err(o, ol), TOL_CALL)
        if model == 0:
            report(f"{name} rhs lag", err(lag, lo), err(lo, lol), TOL_CALL)
    X, U, lag0 = rhs_inputs(0)
    v = fv.vehicle(name)
    (to, lo), (tl, ll) = fp.thruster_forces(v, U, DT, lag=lag0), fp.thruster_forces(v, U, DT, lag=lag0, dtype=L)
    tau, lag = eng.thruster_forces(U, DT, lag=lag0, ctx=ctx)
    report(f"{name} thruster_forces", max(err(tau, to), err(lag, lo)), max(err(to, tl), err(lo, ll)), TOL_CALL)


# ------------------------------------------------------------------------------------------ rollouts
def _to_layout(U, layout):
    b, t, nu = U.shape
    if layout == "btu":
        return U
    if layout == "tub":
        return np.ascontiguousarray(U.transpose(1, 2, 0))
    return np.ascontiguousarray(U.reshape(b, t, nu // 2, 2).transpose(1, 2, 0, 3))


def _from_layout(traj, layout, nx):
    if layout == "btu":
        return traj
    if layout == "tub":
        return traj.transpose(2, 0, 1)
    rows, pairs, b, _ = traj.shape
    return traj.transpose(2, 0, 1, 3).reshape(b, rows, 2 * pairs)[:, :, :nx]


def _check_rollout(what, r, o, ol, layout, nx, stride=1, lag=True):
    e = max(err(_from_layout(r["traj"], layout, nx), o["traj"][:, ::stride]), err(r["xT"], o["xT"]))
    gap = max(err(o["traj"], ol["traj"]), err(o["xT"], ol["xT"]))
    if lag:
        e, gap = max(e, err(r["lag"], o["lag"])), max(gap, err(o["lag"], ol["lag"]))
    report(what, e, gap, TOL_ROLL)
    return e


@pytest.mark.parametrize("name", fv.NAMES)
def test_thruster_rollouts_every_kernel_family(eng, ctx, name):
    """Thruster model, Euler and RK4 (lag per call and per step), layouts btu / tub / tpb, the two-wave and the one-lane kernel,
    BTU tiles staged through LDS and not, a random initial lag with the lag returned and a zero start without lag bookkeeping
    (the untracked kernels); stride 4 on one combination.  traj, xT and lag to 1e-10."""
    ctx.set_params(fv.params(name))
    X0, U, lag0 = rollout_inputs(0)
    worst = 0.0
    try:
        for integ, lag_mode in (("euler", 0), ("rk4", 0), ("rk4", 1)):
            o, ol = oracle_rollout(name, 0, integ, lag_mode, False), oracle_rollout(name, 0, integ, lag_mode, False, True)
            oz = oracle_rollout(name, 0, integ, lag_mode, True)
            for variant in (0, 1):
                ctx.set_rollout_variant(variant)
                for layout, staging in (("btu", 1), ("btu", 2), ("tub", 0), ("tpb", 0)):
                    ctx.set_btu_staging(staging)
                    what = f"{name} {integ} lag_mode {lag_mode} variant {variant} {layout} staging {staging}"
                    r = eng.rollout(0, integ, X0, _to_layout(U, layout), DT, lag=lag0, lag_mode=lag_mode, layout=layout, ctx=ctx)
                    worst = max(worst, _check_rollout(what, r, o, ol, layout, 12))
                    r = eng.rollout(0, integ, X0, _to_layout(U, layout), DT, lag_mode=lag_mode, layout=layout, return_lag=False, ctx=ctx)
                    assert r["lag"] is None
                    worst = max(worst, _check_rollout(what + " zero start untracked", r, oz, oz, layout, 12, lag=False))
        ctx.set_rollout_variant(0)
        ctx.set_btu_staging(0)
        o, ol = oracle_rollout(name, 0, "rk4", 0, False), oracle_rollout(name, 0, "rk4", 0, False, True)
        r = eng.rollout(0, "rk4", X0, U, DT, lag=lag0, stride=4, ctx=ctx)
        assert r["traj"].shape == (B, T // 4 + 1, 12)
        _check_rollout(f"{name} rk4 stride 4", r, o, ol, "btu", 12, stride=4)
    finally:
        ctx.set_rollout_variant(0)
        ctx.set_btu_staging(0)
    print(f"{name}: worst thruster-rollout error {worst:.2e}")


@pytest.mark.parametrize("name", fv.WRENCH_NAMES)
def test_wrench_rollouts(eng, ctx, name):
    """Wrench models 1 (Euler angles) and 2 (quaternion), Euler and RK4, layouts btu and tpb."""
    ctx.set_params(fv.params(name))
    for model in (1, 2):
        X0, U, _ = rollout_inputs(model)
        for integ in ("euler", "rk4"):
            o, ol = oracle_rollout(name, model, integ, 0, True), oracle_rollout(name, model, integ, 0, True, True)
            for layout in ("btu", "tpb"):
                r = eng.rollout(model, integ, X0, _to_layout(U, layout), DT, layout=layout, ctx=ctx)
                _check_rollout(f"{name} model {model} {integ} {layout}", r, o, ol, layout, fp.NX[model], lag=False)


@pytest.mark.parametrize("name", ["V0", "V3"])
def test_observer_form_conditioning_edge(eng, ctx, name):
    """derive_fast() accepts the observer-basis lag up to Frobenius cond(O) < 1e4.  With the nominal lag that is dt = 0.001
    (cond 5.8e3: the worst conditioning the host still accepts) and no longer dt = 0.0005 (2.2e4: the GENERIC kernels); every other
    test runs at cond ~ 10.  Both sides of the edge must meet the rollout bound: RK4, 64 steps, random initial lag, both
    thruster-model kernels."""
    v = fv.vehicle(name)
    c_in, c_out = fp.observer_cond(v, 0.001), fp.observer_cond(v, 0.0005)
    print(f"{name}: cond(O) {c_in:.4g} at dt 0.001, {c_out:.4g} at dt 0.0005")
    assert fp.observer_cond(v, DT) < 1e4 and c_in < 1e4 < c_out
    ctx.set_params(fv.params(name))
    X0, U, lag0 = rollout_inputs(0, 64)
    try:
        for dt in (0.001, 0.0005):
            o, ol = oracle_rollout(name, 0, "rk4", 0, False, False, dt, 64), oracle_rollout(name, 0, "rk4", 0, False, True, dt, 64)
            for variant in (0, 1):
                ctx.set_rollout_variant(variant)
                r = eng.rollout(0, "rk4", X0, U, dt, lag=lag0, ctx=ctx)
                _check_rollout(f"{name} dt {dt} variant {variant}", r, o, ol, "btu", 12)
    finally:
        ctx.set_rollout_variant(0)


# ------------------------------------------------------------------------------------------ windows, one parameter set
@pytest.mark.parametrize("name,model", [(n, 0) for n in fv.NAMES] + [(n, m) for m in (1, 2) for n in fv.WRENCH_NAMES])
def test_window_evaluator_single_set(eng, ctx, name, model):
    """brov_set_params + brov_window_endpoint_se against window_endpoints: Euler and RK4, carried and fresh lag, H = 1 and 10,
    1 / 64 / 65 / 257 windows (one window, a full scan chunk, a chunk plus one, more than one 256-lane block)."""
    ctx.set_params(fv.params(name))
    X, U = recording(name, model)
    for integ in ("euler", "rk4"):
        for carry in (True, False):
            for H in (1, H_MAX):
                (_, per_o, _), (_, per_l, _) = (oracle_windows(name, name, model, integ, carry, H, ld) for ld in (False, True))
                e_per = e_se = g_per = g_se = 0.0
                for nwin in (1, 64, 65, NWIN):
                    n = nwin + H
                    se_g, per_g = eng.window_endpoint_se(model, integ, X[:n], U[:n], H, DT, carry_lag=carry, ctx=ctx)
                    assert per_g.shape == (nwin,)
                    se_o, se_l = per_o[:nwin].sum(), per_l[:nwin].sum()
                    e_per, g_per = max(e_per, err(per_g, per_o[:nwin])), max(g_per, err(per_o[:nwin], per_l[:nwin]))
                    e_se, g_se = max(e_se, abs(se_g - se_o) / se_o), max(g_se, float(abs(se_o - se_l) / se_l))
                report(f"{name} model {model} {integ} carry {int(carry)} H {H} per window", e_per, g_per, TOL_WIN)
                report(f"{name} model {model} {integ} carry {int(carry)} H {H} total", e_se, g_se, TOL_SE)


@pytest.mark.parametrize("integ", ["euler", "rk4"])
def test_window_evaluator_chunk_of_chunks(eng, ctx, integ):
    """64 * 64 + 1 windows (the scan over chunk totals takes a second level), H = 3, thruster model, V1, carried lag."""
    N, H = 64 * 64 + 1 + 3, 3
    ctx.set_params(fv.params("V1"))
    X, U = recording("V1", 0, N)
    (se_o, per_o, _), (se_l, per_l, _) = (oracle_windows("V1", "V1", 0, integ, True, H, ld, N) for ld in (False, True))
    se_g, per_g = eng.window_endpoint_se(0, integ, X, U, H, DT, carry_lag=True, ctx=ctx)
    report(f"V1 {integ} 4097 windows per window", err(per_g, per_o), err(per_o, per_l), TOL_WIN)
    report(f"V1 {integ} 4097 windows total", abs(se_g - se_o) / se_o, float(abs(se_o - se_l) / se_l), TOL_SE)


# ------------------------------------------------------------------------------------------ windows, population
def _pop(eng, ctx, model, integ, plist, Xd, Ud, N, H):
    """raw brov_window_endpoint_pop_dev, carried lag: (se [P], E [P, N-H, nx])"""
    from bluerov2_dynamics_amd import _lib
    P = len(plist)
    pa = (_lib.BrovParams * P)(*plist)
    d_se, d_E = eng.DevArray(ctx, (P,)), eng.DevArray(ctx, (P, N - H, fp.NX[model]))
    ctx.use_null_stream()
    ctx.check(ctx.lib.brov_window_endpoint_pop_dev(ctx.h, model, eng.INTEGRATORS[integ], P, pa, N, H, DT, Xd.ptr, Ud.ptr, 1,
                                                   d_se.ptr, d_E.ptr), "brov_window_endpoint_pop_dev")
    return d_se.numpy(), d_E.numpy()


@pytest.mark.parametrize("model,integ", [(0, "euler"), (0, "rk4"), (1, "rk4"), (2, "rk4")])
def test_window_population_against_oracle(eng, ctx, model, integ):
    """One brov_window_endpoint_pop_dev call with every vehicle as a candidate (thruster model: all nine; wrench models: the six
    that differ there), on V0's recording, and again with the list reversed, so that a nominal candidate sits at both ends of the
    grid's y-dimension.  se[j] and endpoints[j] against the oracle per candidate; the two orders bit-equal per vehicle; the ctx's
    own parameters untouched.  Since the single-set evaluator became the P = 1 case of these kernels
    (test_population_equals_one_at_a_time compares the family with itself), this is their independent check."""
    from bluerov2_dynamics_amd import _lib
    names = list(fv.NAMES if model == 0 else fv.WRENCH_NAMES)
    ctx.set_params(_lib.default_params())
    before = _bytes(ctx.get_params())
    X, U = recording("V0", model)
    N, H = X.shape[0], H_MAX
    Xd, Ud = eng.DevArray.from_host(ctx, X), eng.DevArray.from_host(ctx, U)
    se_f, E_f = _pop(eng, ctx, model, integ, [fv.params(n) for n in names], Xd, Ud, N, H)
    se_r, E_r = _pop(eng, ctx, model, integ, [fv.params(n) for n in names[::-1]], Xd, Ud, N, H)
    assert _bytes(ctx.get_params()) == before
    for j, name in enumerate(names):
        k = len(names) - 1 - j
        assert se_f[j].tobytes() == se_r[k].tobytes() and E_f[j].tobytes() == E_r[k].tobytes(), name
        (se_o, per_o, E_o), (se_l, per_l, E_l) = (oracle_windows(name, "V0", model, integ, True, H, ld) for ld in (False, True))
        report(f"pop model {model} {integ} {name} endpoints", err(E_f[j], E_o), err(E_o, E_l), TOL_WIN)
        report(f"pop model {model} {integ} {name} per window", err(np.sum((E_f[j] - X[H:]) ** 2, axis=1), per_o), err(per_o, per_l), TOL_WIN)
        report(f"pop model {model} {integ} {name} total", abs(se_f[j] - se_o) / se_o, float(abs(se_o - se_l) / se_l), TOL_SE)


# ------------------------------------------------------------------------------------------ the edits are not too small to see
@pytest.mark.parametrize("name", fv.NAMES[1:])
def test_each_edit_matters(name):
    """On the inputs of the parity tests above, the oracle's RHS and window score of V1..V8 differ from V0's by more than 1e3 x the
    bound used there: a kernel that ignored an edited field would fail the parity tests rather than pass unnoticed."""
    d_rhs = err(oracle_rhs(name, 0)[0], oracle_rhs("V0", 0)[0])
    se, _, E = oracle_windows(name, "V0", 0, "rk4", True, H_MAX)
    se0, _, E0 = oracle_windows("V0", "V0", 0, "rk4", True, H_MAX)
    d_se, d_E = abs(se - se0) / se0, err(E, E0)
    print(f"{name}: RHS differs from V0's by {d_rhs:.2e}, window total by {d_se:.2e}, endpoints by {d_E:.2e}")
    assert d_rhs > 1e3 * TOL_CALL and d_se > 1e3 * TOL_SE and d_E > 1e3 * TOL_WIN
    if name in fv.WRENCH_NAMES:
        for model in (1, 2):
            d = err(oracle_rhs(name, model)[0], oracle_rhs("V0", model)[0])
            dw = abs(oracle_windows(name, "V0", model, "rk4", True, H_MAX)[0] / oracle_windows("V0", "V0", model, "rk4", True, H_MAX)[0] - 1)
            print(f"{name} model {model}: RHS differs by {d:.2e}, window total by {dw:.2e}")
            assert d > 1e3 * TOL_CALL and dw > 1e3 * TOL_SE
