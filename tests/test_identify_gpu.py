"""Parameter identification on the device: the population window evaluator against the reference fixture and against the
one-parameter-set-at-a-time path, the finite-difference normal equations against NumPy in long double, the end-to-end fit,
and the argument rules.  rel_err is conftest's mixed error (absolute below 1, relative above)."""
import ctypes

import numpy as np
import pytest

from conftest import load_golden, rel_err

pytestmark = pytest.mark.gpu

THR, WE, WQ = 0, 1, 2


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


@pytest.fixture(scope="module")
def seq_ctx():
    """the context of the one-at-a-time path: its parameters are set per candidate"""
    from bluerov2_dynamics_amd import _lib
    c = _lib.Context(0)
    yield c
    c.close()


def _bytes(p):
    return ctypes.string_at(ctypes.byref(p), ctypes.sizeof(p))


def _candidates(P):
    """Parameter sets that differ where the population path could go wrong: added mass (per-candidate Minv T, so per-candidate
    pre-scan matrices), a tilted thruster (dense allocation: one candidate needs the generic kernels), thrust curve and lag
    dynamics, a current, and the nominal vehicle."""
    from bluerov2_dynamics_amd import _lib
    out = []
    p = _lib.default_params()
    p.added_mass[0] *= 1.2; p.added_mass[2] *= 0.7; p.added_mass[5] *= 0.8
    out.append(p)
    p = _lib.default_params()
    d = np.array([p.thr_dir[0][j] for j in range(3)]) + np.array([0.05, -0.1, 0.15])
    d /= np.linalg.norm(d)
    for j in range(3):
        p.thr_dir[0][j] = d[j]
    out.append(p)
    p = _lib.default_params()
    for j in range(5):
        p.thrust_poly[j] *= 1.1
    for j in range(9):
        p.lag_Ac[j] *= 0.9
    out.append(p)
    p = _lib.default_params()
    for j in range(3):
        p.current[j] = (0.2, -0.1, 0.05)[j]
    p.xb = 0.01
    out.append(p)
    out.append(_lib.default_params())
    return out[:P]


def _recording(model, N, seed):
    rng = np.random.default_rng(seed)
    ang = rng.uniform(-0.5, 0.5, (N, 3))
    pos, nu = rng.uniform(-1, 1, (N, 3)), rng.uniform(-0.5, 0.5, (N, 6))
    if model == WQ:
        q = rng.normal(0, 1, (N, 4))
        X = np.concatenate([pos, q / np.linalg.norm(q, axis=1, keepdims=True), nu], 1)
    else:
        X = np.concatenate([pos, ang, nu], 1)
    U = rng.uniform(-1, 1, (N, 8)) if model == THR else rng.uniform(-1, 1, (N, 6)) * np.array([20, 20, 20, 2, 2, 2.0])
    return np.ascontiguousarray(X), np.ascontiguousarray(U)


def _pop(eng, ctx, model, integ, plist, Xd, Ud, N, H, dt, carry, want_E=True):
    """raw brov_window_endpoint_pop_dev: (se [P], E [P, N-H, nx] | None)"""
    from bluerov2_dynamics_amd import _lib
    P, nx, nwin = len(plist), _lib.NX[model], N - H
    pa = (_lib.BrovParams * P)(*plist)
    d_se = eng.DevArray(ctx, (P,))
    d_E = eng.DevArray(ctx, (P, nwin, nx)) if want_E else None
    ctx.use_null_stream()
    ctx.check(ctx.lib.brov_window_endpoint_pop_dev(ctx.h, model, eng.INTEGRATORS[integ], P, pa, N, H, dt, Xd.ptr, Ud.ptr, int(carry),
                                                   d_se.ptr, d_E.ptr if want_E else None), "pop")
    return d_se.numpy(), (d_E.numpy() if want_E else None)


# ------------------------------------------------------------------------------------------ 1. reference fixture
def test_window_pop_matches_reference_fixture(eng, ctx):
    """Four vehicles (nominal; quadratic damping x 1.3; linear damping x 0.7 with zb doubled; a current) scored by the
    reference's window loop (tools/gen_golden.py: gen_fossen_pop), all four in one population call per H."""
    from bluerov2_dynamics_amd import _lib
    g = load_golden("fossen_pop.npz")
    X, U, dt = g["X"], g["U"], float(g["dt"])
    plist = []
    for j in range(4):
        p = _lib.default_params()
        for i in range(6):
            p.lin_damp[i] = g[f"lin_damp_{j}"][i]
            p.quad_damp[i] = g[f"quad_damp_{j}"][i]
        p.zb = float(g[f"zb_{j}"])
        for i in range(3):
            p.current[i] = g[f"current_{j}"][i]
        plist.append(p)
    for i, H in enumerate(g["H"]):
        rmse = eng.window_pop(_lib.THRUSTER_EULER, "euler", plist, X, U, int(H), dt, ctx=ctx)
        print("H", int(H), "rmse", rmse, "diff", rmse - g["rmse"][i])
        assert rmse.shape == (4,) and np.max(np.abs(rmse - g["rmse"][i])) < 1e-10, (H, rmse - g["rmse"][i])
    assert len(set(np.round(g["rmse"][1], 6))) == 4          # the four vehicles do score differently


# ------------------------------------------------------------------------------------------ 2. one call == P calls
@pytest.mark.parametrize("model", [THR, WE, WQ])
@pytest.mark.parametrize("P,nwin,H", [(1, 1, 1), (3, 65, 10), (5, 257, 10), (2, 64 * 64 + 1, 3)])
def test_population_equals_one_at_a_time(eng, ctx, seq_ctx, model, P, nwin, H):
    """Candidate j of one population call == brov_set_params(params[j]) + brov_window_endpoint_se_dev: end states (through the
    per-window squared errors) and totals to 1e-12, the bound between two paths of the same arithmetic.  The shapes cross the
    256-lane block, the 64-window scan chunk and the chunk-of-chunks scan, and include a single window.  The first candidate
    has another added mass: a pre-scan shared across candidates would hand it the wrong initial lag states.

    Since the window evaluator was unified, the single-set entry point is the P = 1 case of the population kernels: both sides of
    this comparison are one kernel family, so it checks that a candidate's result does not depend on its neighbours or on P, and
    that runs repeat bit for bit -- not that the numbers are right.  The independent check of these candidates' kind (added mass,
    tilted thruster, thrust curve and lag, current) is tests/test_fossen_params_gpu.py: test_window_population_against_oracle and
    test_window_evaluator_single_set, against oracle/fossen_params.py."""
    from bluerov2_dynamics_amd import _lib
    N, dt, nx = nwin + H, 0.02, _lib.NX[model]
    X, U = _recording(model, N, seed=100 * model + P)
    Xd, Ud = eng.DevArray.from_host(ctx, X), eng.DevArray.from_host(ctx, U)
    Xs, Us = eng.DevArray.from_host(seq_ctx, X), eng.DevArray.from_host(seq_ctx, U)
    d_tot, d_per = eng.DevArray(seq_ctx, (1,)), eng.DevArray(seq_ctx, (nwin,))
    plist = _candidates(P)
    before = _bytes(ctx.get_params())
    for integ in ("euler", "rk4"):
        for carry in (0, 1):
            se, E = _pop(eng, ctx, model, integ, plist, Xd, Ud, N, H, dt, carry)
            se2, _ = _pop(eng, ctx, model, integ, plist, Xd, Ud, N, H, dt, carry, want_E=False)
            assert se.tobytes() == se2.tobytes(), (integ, carry)                    # same bits from run to run
            assert _bytes(ctx.get_params()) == before                                # the ctx's own parameters: untouched
            per_pop = np.sum((E - X[None, H:]) ** 2, axis=2)
            for j, p in enumerate(plist):
                seq_ctx.set_params(p)
                eng.window_endpoint_se_dev(model, integ, Xs, Us, H, dt, d_tot, d_per, carry_lag=bool(carry), ctx=seq_ctx)
                per, tot = d_per.numpy(), float(d_tot.numpy()[0])
                e_per = rel_err(per_pop[j], per)
                e_tot = abs(se[j] - tot) / max(1.0, abs(tot))
                assert e_per < 1e-12 and e_tot < 1e-12, (integ, carry, j, e_per, e_tot)
    if model == THR and nwin > 1:
        # the candidates are not interchangeable: the added-mass candidate (rk4, carried lag: the last pass) differs from the nominal vehicle
        se_n, _ = _pop(eng, ctx, model, "rk4", [_lib.default_params()], Xd, Ud, N, H, dt, 1, want_E=False)
        assert abs(se[0] - se_n[0]) > 1e-6 * abs(se_n[0])


# ------------------------------------------------------------------------------------------ 3. normal equations
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("W", [1, 257])
@pytest.mark.parametrize("m", [1, 7, 48])
def test_fd_normal_equations_against_longdouble(eng, ctx, m, W, weighted):
    """JtJ and Jtr from the device against the formulas in np.longdouble on the same (downloaded) end states.  Bound per entry:
    1e-13 * sum |terms| + 1e-300 -- a fixed-order sum of up to 2^20 rows errs by about depth * eps ~ 30 eps of that sum (and each
    term carries ~6 eps from forming the two J entries in fp64); 1e-13 is roughly 15x that."""
    nx = 13
    rng = np.random.default_rng(1000 * m + W + weighted)
    E0 = rng.normal(0, 1, (W, nx))
    delta = rng.choice([-1.0, 1.0], m) * rng.uniform(1e-5, 1e-2, m)
    E = np.concatenate([E0[None], E0[None] + delta[:, None, None] * rng.normal(0, 1, (m, W, nx))])
    tgt = E0 + rng.normal(0, 0.1, (W, nx))
    w = rng.uniform(0.2, 3.0, nx) if weighted else None
    dE = eng.DevArray.from_host(ctx, E)
    dT = eng.DevArray.from_host(ctx, tgt)
    JtJ, Jtr = eng.fd_normal_eq(dE, dT, delta, w, ctx=ctx)
    JtJ2, Jtr2 = eng.fd_normal_eq(dE, dT, delta, w, ctx=ctx)
    assert JtJ.tobytes() == JtJ2.tobytes() and Jtr.tobytes() == Jtr2.tobytes()
    L = np.longdouble
    Eh = dE.numpy().astype(L)
    wl = np.ones(nx, dtype=L) if w is None else w.astype(L)
    J = ((Eh[1:] - Eh[0]) * wl).reshape(m, -1).T / delta.astype(L)
    r = ((Eh[0] - tgt.astype(L)) * wl).reshape(-1)
    ref_JtJ, ref_Jtr = J.T @ J, J.T @ r
    mag_JtJ, mag_Jtr = np.abs(J).T @ np.abs(J), np.abs(J).T @ np.abs(r)
    e1 = np.max(np.abs(JtJ.astype(L) - ref_JtJ) / (mag_JtJ + L(1e-300)))
    e2 = np.max(np.abs(Jtr.astype(L) - ref_Jtr) / (mag_Jtr + L(1e-300)))
    print(f"m {m} W {W} weighted {weighted}: worst |err| / sum|terms|  JtJ {float(e1):.2e}  Jtr {float(e2):.2e}")
    assert np.all(np.abs(JtJ.astype(L) - ref_JtJ) <= L(1e-13) * mag_JtJ + L(1e-300))
    assert np.all(np.abs(Jtr.astype(L) - ref_Jtr) <= L(1e-13) * mag_Jtr + L(1e-300))
    assert np.array_equal(JtJ, JtJ.T)


# ------------------------------------------------------------------------------------------ 4. end to end
def _fit_case(make_rov, x0, U, H, dt, N=600):
    """truth: quadratic damping x 1.3, linear damping x 0.8 on surge, sway, heave, yaw; recording from the rollout kernel, started
    at x0; fit from the nominal vehicle.  Returns (FitResult, relative parameter error, window RMSE of the generating vehicle)."""
    from bluerov2_dynamics_amd.fossen import identify
    names = identify.DEFAULT_FREE
    truth = make_rov()
    for n in ("Xu", "Yv", "Zw", "Nr"):
        setattr(truth, n, getattr(truth, n) * 0.8)
        setattr(truth, n + "_abs", getattr(truth, n + "_abs") * 1.3)
    X = truth.rollout(np.asarray(x0, float)[None], U[None], dt, "euler")["traj"][0][:N]
    want = np.array([getattr(truth, n) for n in names])
    at_truth = truth.multistep_rmse_endpoint(X, U, H, dt, "euler")
    rov = make_rov()
    res = rov.fit_parameters(X, U, dt, H=H, integrator="euler", free=names, iters=20)
    got = np.array([res.params[n] for n in names])
    err = float(np.linalg.norm(got - want) / np.linalg.norm(want))
    print(f"rmse history {res.rmse_history}\naccepted {res.accepted} n_evals {res.n_evals}\nfitted {got}\nwanted {want}\n"
          f"rel param err {err:.3e}  final rmse {res.rmse_history[-1]:.3e}  rmse of the generating vehicle {at_truth:.3e}")
    assert np.all(np.diff(res.rmse_history) <= 0.0)
    assert [getattr(rov, n) for n in names] == [res.params[n] for n in names]      # assign=True
    assert res.rmse_history[-1] <= at_truth * (1 + 1e-9) + 1e-12                   # never worse than the vehicle that made the data
    return res, err, at_truth


# free decay: the vehicle is released with way on in surge, sway, heave and yaw and coasts for 12 s.  Speeds fall by more than
# a decade, which is what separates a linear from a quadratic coefficient on the same axis.
X0_COASTING = np.array([0, 0, 0, 0, 0, 0, 0.8, -0.6, 0.5, 0, 0, 0.9], float)


def test_fit_recovers_perturbed_damping():
    """A 600-row noise-free recording from the rollout kernel (not under test) of a thruster-model vehicle whose quadratic
    damping is x 1.3 and linear damping x 0.8 on surge, sway, heave and yaw; the fit starts from the nominal vehicle (H = 10,
    Euler, 8 free parameters, 20 iterations at most).

    Yardstick (tests/test_identify_cpu.py: test_recoverability_with_the_c_oracle): the CPU loop reached relative parameter error
    0.0 and final RMSE 0.0, so the bounds here are 4 x 0 + 1e-9 on both.

    The recording is a free-decay run: thrusters at rest, vehicle released at X0_COASTING.  Those bounds presuppose a residual
    that can reach zero, i.e. that the generating vehicle reproduces its own recording window by window.  With the thruster model
    that holds only while the lag filters are at rest: window k starts from the lag state window k-1 ended with (quirk Q2), which
    is the recording's lag state H-1 samples LATER than sample k, and without the carry it starts from zero lag; either differs
    from the recording's state wherever the thrusters have been driven (the next test measures by how much).  Free decay is the
    classic damping-identification experiment and the one excitation under which the evaluator's windows are exact.  The kernel
    under test is still the thruster one, carried-lag pre-scan included.

    The same loop on the host, with a NumPy statement of the dynamics as evaluator, takes this recording from RMSE 3.299e-3 to
    5.6e-18 in 7 accepted steps with relative parameter error 2.5e-16 (speeds fall from 0.8/0.6/0.5 m/s and 0.9 rad/s to below
    0.03), so the eight coefficients are identifiable from it."""
    from bluerov2_dynamics_amd.fossen.BlueROV2 import BlueROV2
    from test_identify_cpu import CPU_FINAL_RMSE, CPU_REL_PARAM_ERR
    dt = 0.02
    res, err, at_truth = _fit_case(lambda: BlueROV2(dt=dt), X0_COASTING, np.zeros((600, 8)), 10, dt)
    assert res.rmse_history[-1] <= 4 * CPU_FINAL_RMSE + 1e-9
    assert err <= 4 * CPU_REL_PARAM_ERR + 1e-9


def test_fit_on_a_driven_thruster_recording_ends_below_the_generating_vehicle():
    """The same vehicle and fit on a recording driven by AR(1) thruster inputs (oracle/controls.py), from rest.  Here the carried
    lag (quirk Q2) makes window k start from a lag state the recording did not have at sample k, so the vehicle that generated
    the noise-free data scores well above zero on it and no parameter set reaches zero.  What a least-squares fit of that
    residual owes is: a non-increasing history, an end no worse than the generating vehicle's own score, and an improvement on
    the start (all but the last asserted in _fit_case).  It does not owe the generating parameters: a residual that cannot reach
    zero biases them, which is why the fitted Fossen row is reported by its RMSE.

    Measured on the MI355X: RMSE 6.112e-3 -> 3.721e-3 in 5 accepted steps (120 window evaluations); the generating vehicle scores
    3.743e-3 (3.77e-3 from the C oracle on the same inputs with nominal constants; 6.1e-3 without the carry); relative parameter
    error 6.7e-2."""
    from bluerov2_dynamics_amd.fossen.BlueROV2 import BlueROV2
    from oracle import controls
    dt = 0.02
    res, err, at_truth = _fit_case(lambda: BlueROV2(dt=dt), np.zeros(12), controls.controls_ar1(33, 0, 1, 600)[0], 10, dt)
    assert at_truth > 1e-4                                   # the premise: the generating vehicle does not reproduce its recording
    assert res.rmse_history[-1] < res.rmse_history[0]


def test_fit_recovers_perturbed_damping_wrench_model():
    """The end-to-end case on the wrench Euler model, driven by AR(1) wrenches from rest.  Its windows carry no hidden state, so
    the generating vehicle scores (nearly) zero on a driven recording too, and the same bounds apply -- 4 x the CPU figures (both
    0.0) + 1e-9 on the final RMSE and on the relative parameter error.  Measured on the MI355X: RMSE 1.066e-3 -> 1.4e-17 in 5
    accepted steps, relative parameter error 2.4e-15."""
    from bluerov2_dynamics_amd.fossen.BlueROV2_thrust import BlueROV2 as BlueROV2Wrench
    from oracle import controls
    from test_identify_cpu import CPU_FINAL_RMSE, CPU_REL_PARAM_ERR
    U = controls.controls_ar1(33, 0, 1, 600, nu=6)[0] * np.array([20.0, 20.0, 20.0, 2.0, 2.0, 2.0])
    res, err, _ = _fit_case(BlueROV2Wrench, np.zeros(12), U, 10, 0.02)
    assert res.rmse_history[-1] <= 4 * CPU_FINAL_RMSE + 1e-9
    assert err <= 4 * CPU_REL_PARAM_ERR + 1e-9


# ------------------------------------------------------------------------------------------ 5. argument rules
def test_argument_rules(eng, ctx):
    from bluerov2_dynamics_amd import _lib
    lib, h = ctx.lib, ctx.h
    X, U = _recording(THR, 30, seed=1)
    Xd, Ud = eng.DevArray.from_host(ctx, X), eng.DevArray.from_host(ctx, U)
    pa = (_lib.BrovParams * 2)(_lib.default_params(), _lib.default_params())
    d_se = eng.DevArray(ctx, (2,))
    call = lambda model, P: lib.brov_window_endpoint_pop_dev(h, model, 0, P, pa, 30, 5, 0.02, Xd.ptr, Ud.ptr, 1, d_se.ptr, None)
    assert call(THR, 2) == 0
    for di in (_lib.DI_THRUSTER_EULER, _lib.DI_WRENCH_EULER, _lib.DI_WRENCH_QUAT):
        assert call(di, 2) == -1 and b"brov_window_endpoint_pop_dev: bad argument" in lib.brov_last_error(h)     # gains are not brov_params
    assert call(THR, 0) == -1 and b"brov_window_endpoint_pop_dev: bad argument" in lib.brov_last_error(h)
    assert lib.brov_window_endpoint_pop_dev(h, THR, 0, 2, pa, 30, 5, 0.02, None, Ud.ptr, 1, d_se.ptr, None) == -1
    assert b"brov_window_endpoint_pop_dev: NULL array" in lib.brov_last_error(h)
    se_h = np.zeros(2)
    assert lib.brov_window_endpoint_pop(h, _lib.DI_THRUSTER_EULER, 0, 2, pa, 30, 5, 0.02, X.ctypes.data, U.ctypes.data, 1, se_h.ctypes.data, None) == -1
    assert b"brov_window_endpoint_pop: bad argument" in lib.brov_last_error(h)
    assert lib.brov_window_endpoint_pop(h, THR, 0, 0, pa, 30, 5, 0.02, X.ctypes.data, U.ctypes.data, 1, se_h.ctypes.data, None) == -1
    assert b"brov_window_endpoint_pop: bad argument" in lib.brov_last_error(h)
    assert lib.brov_window_endpoint_pop(h, THR, 0, 2, pa, 30, 5, 0.02, X.ctypes.data, None, 1, se_h.ctypes.data, None) == -1
    assert b"brov_window_endpoint_pop: NULL array" in lib.brov_last_error(h)
    # the host form gives what the device form gives
    assert lib.brov_window_endpoint_pop(h, THR, 0, 2, pa, 30, 5, 0.02, X.ctypes.data, U.ctypes.data, 1, se_h.ctypes.data, None) == 0
    assert se_h.tobytes() == d_se.numpy().tobytes() and se_h[0] > 0
    # normal equations: 1 <= m <= 48
    E = eng.DevArray(ctx, (50, 4, 12)).zero_()
    T = eng.DevArray(ctx, (4, 12)).zero_()
    delta = np.full(49, 1e-3)
    out = np.zeros(49 * 49 + 49)
    fd = lambda m: lib.brov_fd_normal_eq_dev(h, 12, m, 4, E.ptr, T.ptr, delta.ctypes.data, None, out.ctypes.data, out[49 * 49:].ctypes.data)
    assert fd(0) == -1 and fd(49) == -1 and fd(48) == 0 and fd(1) == 0
    with pytest.raises(_lib.BrovError):
        eng.fd_normal_eq(eng.DevArray(ctx, (1, 4, 12)).zero_(), T, np.zeros(0), ctx=ctx)
    # N <= H: NaN like the existing evaluator
    r = eng.window_pop(THR, "euler", [_lib.default_params()] * 3, X[:5], U[:5], 10, 0.02, ctx=ctx)
    assert r.shape == (3,) and np.all(np.isnan(r))
    assert np.isnan(eng.window_rmse(THR, "euler", X[:5], U[:5], 10, 0.02, ctx=ctx))
    # the context is still usable
    assert np.all(np.isfinite(eng.window_pop(THR, "rk4", [_lib.default_params()], X, U, 5, 0.02, ctx=ctx)))
