"""Closed-loop rollouts (brov_rollout_feedback / engine.rollout_feedback / simulate_closed_loop) on the GPU against
tests/feedback_ref.py, the NumPy restatement of the law of include/brov2.h around the parameterised oracle, at the vehicles of
tests/fossen_vehicles.py.

Shapes and recipe as tests/test_rollout_pop_gpu.py: B = 300 (one full 256-lane block and a ragged one), T = 24, DT = 0.02, seeded
x0 and references in +-0.5, the mixed error max |a-b| / max(1,|b|) formed in long double against TOL_ROLL = 1e-10.  Every
comparison also runs the reference in np.longdouble and asserts that fp64 and long double stay within a tenth of the bound, and that
both margins of feedback_ref (distance of an attitude difference to the wrap, distance of a raw command to a limit) exceed 1e-6:
with such inputs the wrap branch and the saturated-step count are well-posed, and the count must match exactly.  The gains are
scaled so that some, not all, commands saturate (asserted on the reference)."""
import ctypes
import functools

import numpy as np
import pytest

import feedback_ref as fr
import fossen_vehicles as fv
from oracle import fossen_params as fp

pytestmark = pytest.mark.gpu

TOL_ROLL = 1e-10
MARGIN = 1e-6
L = np.longdouble
B, T, DT = 300, 24, 0.02
INTEG = {"euler": fp.EULER, "rk4": fp.RK4}
THRUSTER_POP = ("V0", "V5", "V6", "V8", "V7")
WRENCH_POP = ("V0", "V1", "V4", "V5", "V7")
KEYS = ("traj", "xT", "lag", "z", "u", "metrics")
SEED_X, SEED_K = 700, 900                 # chosen so that the margins below hold for every case of this file (checked on the CPU)


def chan_scale(model):
    """size of a command channel: thruster commands ~1, forces ~10 N, moments ~0.5 N m"""
    return np.ones(8) if model == 0 else np.array([10.0, 10.0, 10.0, 0.5, 0.5, 0.5])


def err(a, b):
    """max |a-b| / max(1, |b|), formed in long double"""
    a, b = np.asarray(a, dtype=L), np.asarray(b, dtype=L)
    return float(np.max(np.abs(a - b) / np.maximum(L(1), np.abs(b)))) if a.size else 0.0


def report(what, kernel_err, gap, bound):
    print(f"{what}: kernel err {kernel_err:.2e}  reference fp64-vs-long-double gap {gap:.2e}  bound {bound:.0e}")
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


# ------------------------------------------------------------------------------------------ shared inputs, laws, reference results
@functools.lru_cache(maxsize=None)
def inputs(model):
    """x0 [B,nx] and ref [B,T,nx] in +-0.5 (unit quaternions for model 2), u_ff [B,T,nu], start lag [B,8,3], start z [B,6]"""
    rng = np.random.default_rng(SEED_X + model)
    nx, nu = fp.NX[model], fp.NU[model]
    X0, REF = rng.uniform(-0.5, 0.5, (B, nx)), rng.uniform(-0.5, 0.5, (B, T, nx))
    if model == 2:
        X0[:, 3:7] /= np.linalg.norm(X0[:, 3:7], axis=1, keepdims=True)
        REF[:, :, 3:7] /= np.linalg.norm(REF[:, :, 3:7], axis=2, keepdims=True)
    UFF = rng.uniform(-0.2, 0.2, (B, T, nu)) * chan_scale(model)
    return X0, REF, UFF, rng.uniform(-1, 1, (B, 8, 3)), rng.uniform(-0.01, 0.01, (B, 6))


@functools.lru_cache(maxsize=None)
def gains(model, seed=0, hold=1):
    """random dense gains; per-channel limits 0.6 .. 1 x chan_scale, which lie in the tails of the raw commands (a few per cent of
    the commands reach them); an integral clamp that part of the integral states reach"""
    rng = np.random.default_rng(SEED_K + 10 * seed + model)
    nu, s = fp.NU[model], chan_scale(model)
    return fr.law(nu, K=rng.uniform(-1, 1, (nu, 12)) * 0.3 * s[:, None], Ki=rng.uniform(-1, 1, (nu, 6)) * 1.0 * s[:, None],
                  u_min=-np.linspace(1.0, 0.6, nu) * s, u_max=np.linspace(0.6, 1.0, nu) * s, z_max=np.linspace(0.01, 0.03, 6), hold=hold)


@functools.lru_cache(maxsize=None)
def reference(name, model, integ, lag_mode, ld=False, seed=0, hold=1, full=True):
    """feedback_ref for vehicle `name` on inputs(model).  full: ref_rows = T, u_ff, start lag and z given; otherwise a set-point
    (the first reference row), no u_ff, zero lag and z."""
    X0, REF, UFF, lag0, z0 = inputs(model)
    kw = dict(u_ff=UFF, lag=lag0 if model == 0 else None, z=z0) if full else dict(T=T)
    return fr.rollout(model, INTEG[integ], lag_mode, fv.vehicle(name), gains(model, seed, hold), X0, REF if full else REF[:, :1], DT,
                      dtype=L if ld else np.float64, **kw)


def _compare(got, o, ol, keys, sub=1):
    """(kernel error, fp64-vs-long-double gap) of one candidate's results; margins and the saturated-step count asserted"""
    e = gap = 0.0
    assert min(o["wrap_margin"], ol["wrap_margin"]) > MARGIN and min(o["sat_margin"], ol["sat_margin"]) > MARGIN, \
        (o["wrap_margin"], o["sat_margin"])
    for k in keys:
        a, b, c = got[k], o[k], ol[k]
        if k == "traj":
            b, c = b[:, ::sub], c[:, ::sub]
        if k == "metrics":
            assert np.array_equal(a[:, 3], b[:, 3]) and np.array_equal(b[:, 3], c[:, 3].astype(np.float64)), "saturated-step count"
            a, b, c = a[:, :3], b[:, :3], c[:, :3]
        assert a.shape == b.shape, (k, a.shape, b.shape)
        e, gap = max(e, err(a, b)), max(gap, err(b, c))
    return e, gap


def _check(what, r, names, model, integ, lag_mode, keys=KEYS, sub=1, seeds=None, **kw):
    """every candidate of a population result against the reference of its vehicle (and of its gain set, with seeds)"""
    e = gap = 0.0
    keys = [k for k in keys if r[k] is not None]
    for j, n in enumerate(names):
        s = 0 if seeds is None else seeds[j]
        o, ol = reference(n, model, integ, lag_mode, seed=s, **kw), reference(n, model, integ, lag_mode, ld=True, seed=s, **kw)
        ej, gj = _compare({k: r[k][j] for k in keys}, o, ol, keys, sub)
        e, gap = max(e, ej), max(gap, gj)
        onlim = (o["u"] == gains(model, s).u_min) | (o["u"] == gains(model, s).u_max)
        assert 0.003 < onlim.mean() < 0.5 and 0.02 < onlim.any(axis=2).mean() < 0.9, "gains must saturate some, not all, commands"
    report(what, e, gap, TOL_ROLL)


def _run(eng, ctx, names, model, integ, lag_mode=0, seed=0, hold=1, full=True, **kw):
    X0, REF, UFF, lag0, z0 = inputs(model)
    P = len(names)
    fb = fr.to_struct(gains(model, seed, hold))
    if not full:
        return eng.rollout_feedback(model, integ, _params(names), fb, X0, REF[:, :1], DT, T=T, lag_mode=lag_mode, want_u=True, ctx=ctx, **kw)
    return eng.rollout_feedback(model, integ, _params(names), fb, X0, REF, DT, u_ff=UFF,
                                lag=np.broadcast_to(lag0, (P,) + lag0.shape) if model == 0 else None,
                                z=np.broadcast_to(z0, (P,) + z0.shape), lag_mode=lag_mode, want_u=True, ctx=ctx, **kw)


# ------------------------------------------------------------------------------------------ parity
@pytest.mark.parametrize("integ", ["euler", "rk4"])
@pytest.mark.parametrize("model", [0, 1, 2])
def test_parity_three_models(eng, ctx, model, integ):
    """hold = 1, shared inputs, one controller for five vehicles, a reference row per step, u_ff, start lag and z given: traj, xT,
    lag, z, u and metrics of every candidate."""
    names = THRUSTER_POP if model == 0 else WRENCH_POP
    r = _run(eng, ctx, names, model, integ)
    nx, nu = fp.NX[model], fp.NU[model]
    assert r["traj"].shape == (5, B, T + 1, nx) and r["xT"].shape == (5, B, nx) and r["u"].shape == (5, B, T, nu)
    assert r["z"].shape == (5, B, 6) and r["metrics"].shape == (5, B, 4)
    assert (r["lag"].shape == (5, B, 8, 3)) if model == 0 else (r["lag"] is None)
    _check(f"feedback model {model} {integ}", r, names, model, integ, 0)


def test_parity_hold_setpoint_no_state(eng, ctx):
    """thruster model, RK4, hold = 5 (ticks at 0, 5, .., 20 of T = 24), a set-point, no u_ff, lag and z NULL"""
    r = _run(eng, ctx, THRUSTER_POP, 0, "rk4", hold=5, full=False)
    assert r["lag"] is None and r["z"] is None
    u = r["u"]
    for t in range(T):
        assert np.array_equal(u[:, :, t], u[:, :, t - t % 5]), "the command is held between ticks"
    assert not np.array_equal(u[:, :, 4], u[:, :, 5])
    _check("feedback hold 5, set-point", r, THRUSTER_POP, 0, "rk4", 0, hold=5, full=False)


def test_parity_lag_per_step(eng, ctx):
    r = _run(eng, ctx, THRUSTER_POP, 0, "rk4", lag_mode=1)
    _check("feedback LAG_PER_STEP", r, THRUSTER_POP, 0, "rk4", 1)


def test_parity_per_candidate_inputs(eng, ctx):
    """per_candidate=True: candidate j sees the shared scenarios rotated by 7 j rows, so its results are the reference's rotated"""
    X0, REF, UFF, lag0, z0 = inputs(0)
    P = 5
    rot = lambda a: np.stack([np.roll(a, 7 * j, axis=0) for j in range(P)])
    r = eng.rollout_feedback(0, "rk4", _params(THRUSTER_POP), fr.to_struct(gains(0)), rot(X0), rot(REF), DT, u_ff=rot(UFF), lag=rot(lag0),
                             z=rot(z0), want_u=True, per_candidate=True, ctx=ctx)
    back = {k: np.stack([np.roll(r[k][j], -7 * j, axis=0) for j in range(P)]) for k in KEYS}
    _check("feedback per-candidate inputs", back, THRUSTER_POP, 0, "rk4", 0)


def test_parity_gain_set_per_candidate(eng, ctx):
    """nfb = P: five gain sets on five copies of V7"""
    X0, REF, UFF, lag0, z0 = inputs(0)
    names, seeds = ("V7",) * 5, (0, 1, 2, 3, 4)
    fbs = [fr.to_struct(gains(0, s)) for s in seeds]
    r = eng.rollout_feedback(0, "rk4", _params(names), fbs, X0, REF, DT, u_ff=UFF, lag=np.broadcast_to(lag0, (5,) + lag0.shape),
                             z=np.broadcast_to(z0, (5,) + z0.shape), want_u=True, ctx=ctx)
    _check("feedback nfb = P", r, names, 0, "rk4", 0, seeds=seeds)
    assert err(r["xT"][0], r["xT"][1]) > 1e3 * TOL_ROLL, "the gain sets must matter"


def test_parity_stride_and_no_store(eng, ctx):
    names = ("V0", "V7")
    r = _run(eng, ctx, names, 0, "rk4", stride=4)
    assert r["traj"].shape == (2, B, 7, 12)
    _check("feedback stride 4", r, names, 0, "rk4", 0, sub=4)
    r = _run(eng, ctx, names, 0, "rk4", store=False)
    assert r["traj"] is None
    _check("feedback store=False", r, names, 0, "rk4", 0)


# ------------------------------------------------------------------------------------------ wrap and sign
@pytest.mark.parametrize("model", [0, 1, 2])
def test_wrap_and_short_way_round(eng, ctx, model):
    """Euler models: yaw -3.0 against a yaw reference of 3.0 (raw difference 6.0, wrapped -0.283) and the mirror image; quaternion
    model: yaw -0.2 against a reference at yaw +0.3 written in the opposite hemisphere (q_e.w < 0).  A positive yaw gain alone:
    parity with the reference, and the first command turns the short way round."""
    rng = np.random.default_rng(40 + model)
    n, nx, nu = 40, fp.NX[model], fp.NU[model]
    x0, ref = rng.uniform(-0.5, 0.5, (n, nx)), rng.uniform(-0.5, 0.5, (n, 1, nx))
    sign = np.where(np.arange(n) % 2 == 0, 1.0, -1.0)          # every other row is the mirror image
    if model == 2:
        x0[:, 3:7], ref[:, 0, 3:7] = 0.0, 0.0
        x0[:, 3], x0[:, 6] = np.cos(0.1), -sign * np.sin(0.1)                   # yaw -0.2 sign
        ref[:, 0, 3], ref[:, 0, 6] = -np.cos(0.15), -sign * np.sin(0.15)        # yaw +0.3 sign, written as -q
        assert np.all(np.sum(x0[:, 3:7] * ref[:, 0, 3:7], axis=1) < 0)           # q_e.w < 0
        want_dir = sign                                                          # the rotation left to do is +0.5 sign about z
    else:
        noise = rng.uniform(-0.05, 0.05, (2, n))
        x0[:, 5], ref[:, 0, 5] = -3.0 * sign + noise[0], 3.0 * sign + noise[1]
        want_dir = -sign                                                         # 6.0 sign wraps to -0.283 sign
    Kw = np.zeros((6, 12))
    Kw[5, 5] = 4.0
    T_alloc = fp.derived(fv.vehicle("V0"))[1]
    K = Kw if model != 0 else np.linalg.pinv(T_alloc) @ Kw / 8.9
    law = fr.law(nu, K=K, u_min=-0.9 * chan_scale(model), u_max=0.9 * chan_scale(model))
    names = ("V0", "V7")
    r = eng.rollout_feedback(model, "rk4", _params(names), fr.to_struct(law), x0, ref, DT, T=T, want_u=True, ctx=ctx)
    u0 = r["u"][0, :, 0]
    yaw_moment = u0[:, 5] if model != 0 else (T_alloc @ u0.T)[5]
    assert np.array_equal(np.sign(yaw_moment), want_dir), "the first command must turn the short way round"
    e = gap = 0.0
    for j, nme in enumerate(names):
        o = fr.rollout(model, fp.RK4, 0, fv.vehicle(nme), law, x0, ref, DT, T=T)
        ol = fr.rollout(model, fp.RK4, 0, fv.vehicle(nme), law, x0, ref, DT, T=T, dtype=L)
        keys = ("traj", "xT", "u", "metrics")
        ej, gj = _compare({k: r[k][j] for k in keys}, o, ol, keys)
        e, gap = max(e, ej), max(gap, gj)
    report(f"feedback wrap / sign, model {model}", e, gap, TOL_ROLL)


# ------------------------------------------------------------------------------------------ identities
@pytest.mark.parametrize("model", [0, 2])
def test_zero_gains_against_rollout_pop(eng, ctx, model):
    """K = Ki = 0, infinite limits: the applied command is u_ff, and traj, xT, lag agree with engine.rollout_pop on U = u_ff within
    TOL_ROLL (whether they are bit-equal is printed, not asserted)."""
    X0, REF, UFF, lag0, _ = inputs(model)
    names = THRUSTER_POP if model == 0 else WRENCH_POP
    lag = np.broadcast_to(lag0, (5,) + lag0.shape) if model == 0 else None
    r = eng.rollout_feedback(model, "rk4", _params(names), fr.to_struct(fr.law(fp.NU[model])), X0, REF, DT, u_ff=UFF, lag=lag, want_u=True,
                             ctx=ctx)
    p = eng.rollout_pop(model, "rk4", _params(names), X0, UFF, DT, lag=lag, ctx=ctx)
    assert np.array_equal(r["u"], np.broadcast_to(UFF, r["u"].shape)) and not r["metrics"][:, :, 3].any()
    keys = [k for k in ("traj", "xT", "lag") if p[k] is not None]
    e = max(err(r[k], p[k]) for k in keys)
    print(f"zero gains vs rollout_pop, model {model}: err {e:.2e}, bit-equal: {all(np.array_equal(r[k], p[k]) for k in keys)}")
    assert e < TOL_ROLL


def test_resume_is_bit_exact(eng, ctx):
    """T = 20, hold = 5: one call against 10 + 10 from the returned (xT, lag, z) with the remaining rows of u_ff and ref: the same bits
    in traj, xT, lag, z and u; the metrics add up to 1e-12 relative."""
    X0, REF, UFF, lag0, z0 = inputs(0)
    ps, fb = _params(THRUSTER_POP), fr.to_struct(gains(0, hold=5))
    lag, z = np.broadcast_to(lag0, (5,) + lag0.shape), np.broadcast_to(z0, (5,) + z0.shape)
    kw = dict(want_u=True, ctx=ctx)
    full = eng.rollout_feedback(0, "rk4", ps, fb, X0, REF[:, :20], DT, u_ff=UFF[:, :20], lag=lag, z=z, **kw)
    a = eng.rollout_feedback(0, "rk4", ps, fb, X0, REF[:, :10], DT, u_ff=UFF[:, :10], lag=lag, z=z, **kw)
    rest = lambda v: np.broadcast_to(v[:, 10:20], (5,) + v[:, 10:20].shape)
    b = eng.rollout_feedback(0, "rk4", ps, fb, a["xT"], rest(REF), DT, u_ff=rest(UFF), lag=a["lag"], z=a["z"], per_candidate=True, **kw)
    for k in ("xT", "lag", "z"):
        assert np.array_equal(b[k], full[k]), k
    assert np.array_equal(np.concatenate([a["traj"], b["traj"][:, :, 1:]], axis=2), full["traj"])
    assert np.array_equal(np.concatenate([a["u"], b["u"]], axis=2), full["u"])
    s = a["metrics"] + b["metrics"]
    assert np.array_equal(s[:, :, 3], full["metrics"][:, :, 3])
    assert np.max(np.abs(s - full["metrics"]) / np.maximum(np.abs(full["metrics"]), 1e-300)) < 1e-12
    assert full["metrics"][:, :, 3].any() and not np.array_equal(a["z"], z)


def test_two_calls_same_bits_and_ctx_parameters_untouched(eng, ctx):
    before = _bytes(ctx.get_params())
    a, b = _run(eng, ctx, THRUSTER_POP, 0, "rk4"), _run(eng, ctx, THRUSTER_POP, 0, "rk4")
    for k in KEYS:
        assert np.array_equal(a[k], b[k]), k
    up = lambda v: eng.DevArray.from_host(ctx, v)
    X0, REF, UFF, lag0, z0 = inputs(0)
    d = eng.rollout_feedback(0, "rk4", _params(THRUSTER_POP), fr.to_struct(gains(0)), up(X0), up(REF), DT, u_ff=up(UFF),
                             lag=up(np.broadcast_to(lag0, (5,) + lag0.shape)), z=up(np.broadcast_to(z0, (5,) + z0.shape)), want_u=True, ctx=ctx)
    assert isinstance(d["traj"], eng.DevArray)
    for k in KEYS:
        assert np.array_equal(d[k].numpy(), a[k]), k
    assert _bytes(ctx.get_params()) == before


# ------------------------------------------------------------------------------------------ the host contract
def test_host_contract(eng, ctx):
    """every rule of the header returns BROV_ERR_ARG with a brov_last_error text, and no output buffer is written"""
    from bluerov2_dynamics_amd import _lib
    X0, REF, UFF, _, _ = inputs(0)
    n, P = 3, 2
    x0, ref = np.ascontiguousarray(X0[:n]), np.ascontiguousarray(REF[:n])
    pa = (_lib.BrovParams * P)(*_params(("V0", "V7")))
    good = gains(0)

    def edited(*edits, hold=None):
        l = fr.Law(good.K.copy(), good.Ki.copy(), good.u_min.copy(), good.u_max.copy(), good.z_max.copy(), good.hold if hold is None else hold)
        for field, i, v in edits:
            getattr(l, field)[i] = v
        return l
    cases = [("hold < 1", dict(fb=[edited(hold=0)])),
             ("nfb not in {1, P}", dict(fb=[good] * 3)),
             ("ref_rows not in {1, T}", dict(ref_rows=T - 1)),
             ("u_min > u_max", dict(fb=[edited(("u_min", 2, 0.7), ("u_max", 2, 0.6))])),
             ("negative z_max", dict(fb=[good, edited(("z_max", 5, -1e-3))])),
             ("NaN in K", dict(fb=[edited(("K", (7, 11), np.nan))])),
             ("NaN in u_max", dict(fb=[edited(("u_max", 0, np.nan))])),
             ("traj_stride < 1", dict(stride=0))]
    sentinel = 7.25
    for what, kw in cases:
        fbs = [fr.to_struct(l) for l in kw.get("fb", [good])]
        fa = (_lib.BrovFeedback * len(fbs))(*fbs)
        outs = dict(traj=np.full((P, n, T + 1, 12), sentinel), xT=np.full((P, n, 12), sentinel), u=np.full((P, n, T, 8), sentinel),
                    metrics=np.full((P, n, 4), sentinel), lag=np.full((P, n, 8, 3), sentinel), z=np.full((P, n, 6), sentinel))
        rc = ctx.lib.brov_rollout_feedback(ctx.h, 0, _lib.RK4, 0, P, pa, len(fbs), fa, 0, n, T, DT, x0.ctypes.data, None, ref.ctypes.data,
                                           kw.get("ref_rows", T), outs["lag"].ctypes.data, outs["z"].ctypes.data, outs["traj"].ctypes.data,
                                           kw.get("stride", 1), outs["xT"].ctypes.data, outs["u"].ctypes.data, outs["metrics"].ctypes.data)
        msg = ctx.lib.brov_last_error(ctx.h)
        print(what, "->", rc, msg)
        assert rc == -1 and msg and len(msg.strip()) > 0, what
        assert all(np.all(v == sentinel) for v in outs.values()), what
    with pytest.raises(_lib.BrovError, match=r"BROV_ERR_ARG: \S"):
        eng.rollout_feedback(_lib.DI_THRUSTER_EULER, "rk4", _params(("V0",)), fr.to_struct(good), x0, ref, DT, ctx=ctx)
    r = eng.rollout_feedback(0, "rk4", [], fr.to_struct(good), x0, ref, DT, ctx=ctx)             # P = 0: nothing to do
    assert r["xT"].shape == (0, n, 12)


# ------------------------------------------------------------------------------------------ the vehicle class, ensemble statistics
def test_simulate_closed_loop(eng):
    """rov.simulate_closed_loop, one vehicle and with params_list, equals engine.rollout_feedback on the same arguments, and leaves
    the object's lag state and parameters as they were"""
    from bluerov2_dynamics_amd.fossen.BlueROV2 import BlueROV2
    from bluerov2_dynamics_amd.fossen import control, identify
    X0, REF, _, _, _ = inputs(0)
    x0, ref = X0[0], REF[0]
    rov = BlueROV2()
    rov.simulate(x0, np.full((5, 8), 0.1), DT, integrator="rk4")            # a non-zero lag state of its own
    lag_before, params_before = np.array(rov._lag), _bytes(identify.params_of(rov))
    fb = control.pid_thrusters(rov, [4.0, 4.0, 6.0, 0.5, 0.5, 1.0], [2.0, 2.0, 3.0, 0.2, 0.2, 0.4], 0.5, z_max=0.2)
    traj, u, m = rov.simulate_closed_loop(x0, ref, DT, fb, integrator="rk4", hold=2)
    assert traj.shape == (T + 1, 12) and u.shape == (T, 8) and m.shape == (4,)
    fb2 = control.pid_thrusters(rov, [4.0, 4.0, 6.0, 0.5, 0.5, 1.0], [2.0, 2.0, 3.0, 0.2, 0.2, 0.4], 0.5, z_max=0.2, hold=2)
    want = eng.rollout_feedback(0, "rk4", [identify.params_of(rov)], fb2, x0[None], ref[None], DT, want_u=True, ctx=rov._ctx)
    assert np.array_equal(traj, want["traj"][0, 0]) and np.array_equal(u, want["u"][0, 0]) and np.array_equal(m, want["metrics"][0, 0])
    assert np.array_equal(u[0], u[1]) and not np.array_equal(u[1], u[2]) and fb.hold == 1
    ps = _params(("V0", "V2", "V7"))
    trajP, uP, mP = rov.simulate_closed_loop(x0, ref[0], DT, fb, T=T, params_list=ps, integrator="rk4")
    want = eng.rollout_feedback(0, "rk4", ps, fb, x0[None], ref[None, :1], DT, T=T, want_u=True, ctx=rov._ctx)
    assert trajP.shape == (3, T + 1, 12) and uP.shape == (3, T, 8) and mP.shape == (3, 4)
    assert np.array_equal(trajP, want["traj"][:, 0]) and np.array_equal(uP, want["u"][:, 0]) and np.array_equal(mP, want["metrics"][:, 0])
    assert err(trajP[0], trajP[1]) > 1e3 * TOL_ROLL
    assert np.array_equal(rov._lag, lag_before) and _bytes(identify.params_of(rov)) == params_before


def test_ensemble_stats_over_metrics(eng, ctx):
    """engine.ensemble_stats reduces the metrics of a population: min and max exact, mean within P 2^-52 mean_j|v|, std within
    4 P 2^-52 max_j|v| of a long-double computation (the bounds of tests/test_rollout_pop_gpu.py)"""
    r = _run(eng, ctx, THRUSTER_POP, 0, "rk4")
    v, P = r["metrics"], 5
    s = eng.ensemble_stats(v, ctx=ctx)
    assert all(s[k].shape == (B, 4) for k in ("mean", "std", "min", "max"))
    assert np.array_equal(s["min"], v.min(0)) and np.array_equal(s["max"], v.max(0))
    vl = v.astype(L)
    mean = vl.sum(0) / P
    std = np.sqrt(((vl - mean) ** 2).sum(0) / (P - 1))
    assert np.all(np.abs(s["mean"].astype(L) - mean) <= P * L(2.0) ** -52 * np.abs(vl).mean(0))
    assert np.all(np.abs(s["std"].astype(L) - std) <= 4 * P * L(2.0) ** -52 * np.abs(vl).max(0))


def test_example_runs_small():
    """examples/closed_loop_ensemble.py without a CSV: eight vehicles from the +-10 % box, one second of simulated time"""
    import importlib.util
    import os
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "closed_loop_ensemble.py")
    spec = importlib.util.spec_from_file_location("closed_loop_ensemble", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    out = mod.run(ensemble=8, seconds=1.0, hold=5, integrator="rk4", verbose=False)
    assert out["traj"].shape == (51, 12) and out["u"].shape == (50, 8) and out["settle"].shape == (8, 2)
    assert np.all(np.isfinite(out["settle"])) and np.all(out["band"]["min"] <= out["band"]["max"]) and 0.0 <= out["saturating"] <= 1.0
    assert np.all(out["traj"][-1, 2] > 5.0), "the vehicle must have started towards the deeper set-point"
