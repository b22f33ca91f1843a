"""The window evaluator and the parameter fit over several recordings ("bags") on the device: the ragged entry points against
one plain call per bag, against the plain call when there is one bag, against the independent oracle (oracle/fossen_params.py),
the single-set form, the argument rules and the end-to-end fit.  rel_err is conftest's mixed error (absolute below 1, relative
above); report / err and the oracle bounds are tests/test_fossen_params_gpu.py's."""
import ctypes

import numpy as np
import pytest

from conftest import rel_err

pytestmark = pytest.mark.gpu

THR, WE, WQ = 0, 1, 2
DT = 0.02
# H = 3: 64, 0, 0, 1, 5, 58, 200, 2 and 130 windows -> an empty bag, a bag of exactly H rows, a bag with one window, bag openings
# at windows 64, 65 and 70 (three in the scan chunk 64..127, the first on its boundary), one at 128 (the next boundary), bags of
# 200 and 130 windows that span chunks, and W = 460 > one 256-lane block
LENS = (67, 0, 3, 4, 8, 61, 203, 5, 133)
H3 = 3


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
    """the context of the single-set form: its parameters are set per candidate"""
    from bluerov2_dynamics_amd import _lib
    c = _lib.Context(0)
    yield c
    c.close()


def _offsets(lens):
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)


def _rows(off, H):
    """first row of every window, bag after bag -- written out here, not taken from the package"""
    return np.array([a + k for a, b in zip(off[:-1], off[1:]) for k in range(max(int(b - a) - H, 0))], dtype=np.int64)


def _pop_ragged(eng, ctx, model, integ, plist, Xd, Ud, off, H, dt, carry, want=True):
    """raw brov_window_endpoint_pop_ragged_dev: (se [P], E [P, W, nx], target [W, nx], per_window [P, W]); the arrays only if want"""
    from bluerov2_dynamics_amd import _lib
    P, nx, W = len(plist), _lib.NX[model], len(_rows(off, H))
    pa = (_lib.BrovParams * P)(*plist)
    d_se = eng.DevArray(ctx, (P,))
    d_E, d_T, d_per = (eng.DevArray(ctx, (P, W, nx)), eng.DevArray(ctx, (W, nx)), eng.DevArray(ctx, (P, W))) if want else (None, None, None)
    ctx.use_null_stream()
    ctx.check(ctx.lib.brov_window_endpoint_pop_ragged_dev(ctx.h, model, eng.INTEGRATORS[integ], P, pa, len(off) - 1, off.ctypes.data, H, dt,
                                                          Xd.ptr, Ud.ptr, int(carry), d_se.ptr, d_E.ptr if want else None,
                                                          d_T.ptr if want else None, d_per.ptr if want else None), "pop_ragged")
    return (d_se.numpy(),) + ((d_E.numpy(), d_T.numpy(), d_per.numpy()) if want else (None, None, None))


# ------------------------------------------------------------------------------------------ 1. ragged == one plain call per bag
@pytest.mark.parametrize("model", [THR, WE, WQ])
def test_ragged_equals_the_per_bag_calls(eng, ctx, model):
    """Euler and RK4, fresh and carried lag, P = 3 candidates of test_identify_gpu._candidates' kind (a non-nominal added mass
    first: a pre-scan shared across candidates would hand it the wrong start states), over LENS.  Every bag with a window is also
    scored alone by brov_window_endpoint_pop_dev on its rows; the ragged call's end states and per-window errors on that bag's
    window range agree with it to 1e-12 (the bound of test_population_equals_one_at_a_time between two paths of the same
    arithmetic: where a bag starts inside a scan chunk the blocked scan associates differently), se[j] to 1e-12 relative of the sum
    of the bags' totals, the target equals the gathered rows exactly, two runs give the same bits, and the ctx's own parameters
    are untouched."""
    from bluerov2_dynamics_amd import _lib
    from test_identify_gpu import _bytes, _candidates, _pop, _recording
    off, H = _offsets(LENS), H3
    rows = _rows(off, H)
    assert len(rows) == 460 and np.cumsum(np.maximum(np.diff(off) - H, 0)).tolist() == [64, 64, 64, 65, 70, 128, 328, 330, 460]
    X, U = _recording(model, int(off[-1]), seed=900 + model)
    Xd, Ud = eng.DevArray.from_host(ctx, X), eng.DevArray.from_host(ctx, U)
    plist = _candidates(3)
    before = _bytes(ctx.get_params())
    worst = 0.0
    for integ in ("euler", "rk4"):
        for carry in (0, 1):
            se, E, T, per = _pop_ragged(eng, ctx, model, integ, plist, Xd, Ud, off, H, DT, carry)
            se2, E2, T2, per2 = _pop_ragged(eng, ctx, model, integ, plist, Xd, Ud, off, H, DT, carry)
            se3 = _pop_ragged(eng, ctx, model, integ, plist, Xd, Ud, off, H, DT, carry, want=False)[0]
            assert se.tobytes() == se2.tobytes() == se3.tobytes() and E.tobytes() == E2.tobytes() and per.tobytes() == per2.tobytes()
            assert _bytes(ctx.get_params()) == before
            assert np.array_equal(T, X[rows + H]) and np.array_equal(T2, T)
            total, w0 = np.zeros(3), 0
            for a, b in zip(off[:-1], off[1:]):
                L = int(b - a)
                if L <= H:
                    continue
                se_b, E_b = _pop(eng, ctx, model, integ, plist, Xd.rows(a, b), Ud.rows(a, b), L, H, DT, carry)
                w1 = w0 + L - H
                e_E = rel_err(E[:, w0:w1], E_b)
                e_per = rel_err(per[:, w0:w1], np.sum((E_b - X[None, a + H:b]) ** 2, axis=2))
                worst = max(worst, e_E, e_per)
                assert e_E < 1e-12 and e_per < 1e-12, (integ, carry, int(a), e_E, e_per)
                total, w0 = total + se_b, w1
            assert w0 == len(rows)
            e_se = np.max(np.abs(se - total) / np.abs(total))
            print(f"model {model} {integ} carry {carry}: se vs the bags' sum {e_se:.2e}")
            assert e_se < 1e-12, (integ, carry, e_se)
    print(f"model {model}: worst end-state / per-window error against the per-bag calls {worst:.2e}")
    if model == THR:
        # the bags are not interchangeable with one recording: the last pass (rk4, carried lag) against the plain call on the same rows
        se_p, _ = _pop(eng, ctx, model, "rk4", plist, Xd, Ud, int(off[-1]), H, DT, 1, want_E=False)
        assert np.all(np.abs(se_p - se) > 1e-6 * se)


# ------------------------------------------------------------------------------------------ 2. one bag == the plain call
@pytest.mark.parametrize("model", [THR, WQ])
def test_one_bag_equals_the_plain_call(eng, ctx, model):
    from test_identify_gpu import _candidates, _pop, _recording
    N, H = 463, H3
    X, U = _recording(model, N, seed=950 + model)
    Xd, Ud = eng.DevArray.from_host(ctx, X), eng.DevArray.from_host(ctx, U)
    plist, off = _candidates(3), np.array([0, N], dtype=np.int64)
    for integ in ("euler", "rk4"):
        for carry in (0, 1):
            se, E, T, per = _pop_ragged(eng, ctx, model, integ, plist, Xd, Ud, off, H, DT, carry)
            se_p, E_p = _pop(eng, ctx, model, integ, plist, Xd, Ud, N, H, DT, carry)
            e_E, e_se = rel_err(E, E_p), float(np.max(np.abs(se - se_p) / np.abs(se_p)))
            print(f"model {model} {integ} carry {carry}: end states {e_E:.2e}  totals {e_se:.2e}  "
                  f"same bits: end states {E.tobytes() == E_p.tobytes()}, totals {se.tobytes() == se_p.tobytes()}")
            assert e_E < 1e-12 and e_se < 1e-12
            assert np.array_equal(T, X[H:])


# ------------------------------------------------------------------------------------------ 3. against the independent oracle
ORACLE_LENS, ORACLE_H = (47, 90, 63), 10


def _oracle_case():
    """Three recordings of vehicle V1 (mass, volume, inertias, added mass: another Minv T, so other pre-scan matrices), each an
    oracle rollout from rest at its own position under its own smooth commands, + 1e-3 noise (test_fossen_params_gpu.recording's
    recipe).  The positions are metres apart, so a window across a join is scored against a jump."""
    import fossen_vehicles as fv
    from oracle import fossen_params as fp
    from test_fossen_params_gpu import _smooth
    rng = np.random.default_rng(77)
    Xs, Us = [], []
    for b, L in enumerate(ORACLE_LENS):
        U = _smooth(rng, L, 8)
        x0 = np.zeros((1, 12))
        x0[0, :3] = (2.0 * b, -1.5 * b, 0.5 * b)
        X = fp.rollout(0, fp.EULER, 0, fv.vehicle("V1"), x0, U[None], DT)["traj"][0][:L]
        Xs.append(X + rng.normal(0, 1e-3, X.shape))
        Us.append(U)
    return Xs, Us


@pytest.mark.parametrize("integ", ["euler", "rk4"])
def test_ragged_against_the_oracle(eng, ctx, integ):
    """Thruster model, carried lag, vehicle V1, three bags of 47, 90 and 63 rows at H = 10: oracle/fossen_params.window_endpoints
    per bag (a fresh lag state each), joined on the host, in fp64 and in long double.  End states and per-window errors to
    TOL_WIN = 1e-9, the total to TOL_SE = 1e-8; the oracle's own fp64-to-long-double gap below a tenth of each (report).  The plain
    call on the concatenated rows must differ from the ragged total by more than 1e3 x TOL_SE: what the bags are for."""
    import fossen_vehicles as fv
    from oracle import fossen_params as fp
    from test_fossen_params_gpu import INTEG, L, TOL_SE, TOL_WIN, err, report
    from test_identify_gpu import _pop
    Xs, Us = _oracle_case()
    H, off = ORACLE_H, _offsets(ORACLE_LENS)
    res = {}
    for ld in (False, True):
        parts = [fp.window_endpoints(0, INTEG[integ], fv.vehicle("V1"), X, U, H, DT, carry_lag=True, dtype=L if ld else np.float64)
                 for X, U in zip(Xs, Us)]
        res[ld] = (sum(p[0] for p in parts), np.concatenate([p[1] for p in parts]), np.concatenate([p[2] for p in parts]))
    (se_o, per_o, E_o), (se_l, per_l, E_l) = res[False], res[True]
    X, U = np.concatenate(Xs), np.concatenate(Us)
    Xd, Ud = eng.DevArray.from_host(ctx, X), eng.DevArray.from_host(ctx, U)
    se, E, T, per = _pop_ragged(eng, ctx, 0, integ, [fv.params("V1")], Xd, Ud, off, H, DT, 1)
    assert E.shape == (1, sum(ORACLE_LENS) - 3 * H, 12)
    report(f"ragged {integ} V1 endpoints", err(E[0], E_o), err(E_o, E_l), TOL_WIN)
    report(f"ragged {integ} V1 per window", err(per[0], per_o), err(per_o, per_l), TOL_WIN)
    report(f"ragged {integ} V1 total", abs(se[0] - se_o) / se_o, float(abs(se_o - se_l) / se_l), TOL_SE)
    se_p, _ = _pop(eng, ctx, 0, integ, [fv.params("V1")], Xd, Ud, X.shape[0], H, DT, 1, want_E=False)
    d = abs(se_p[0] - se[0]) / se[0]
    print(f"the concatenated rows as one recording: total {se_p[0]:.4e} against {se[0]:.4e} over bags, relative difference {d:.2e}")
    assert d > 1e3 * TOL_SE


# ------------------------------------------------------------------------------------------ 4. the single-set form
def test_single_set_form(eng, ctx, seq_ctx):
    """brov_window_endpoint_se_ragged_dev after set_params(p) == candidate p of the population call (total and per window, 1e-12),
    thruster model, both integrators, carried lag, over LENS.  One double-integrator model (gains are not brov_params: the
    single-set form only) against the sum of brov_window_endpoint_se_dev over the bags."""
    from bluerov2_dynamics_amd import _lib
    from test_identify_gpu import _candidates, _recording
    off, H = _offsets(LENS), H3
    W = len(_rows(off, H))
    X, U = _recording(THR, int(off[-1]), seed=970)
    Xd, Ud = eng.DevArray.from_host(ctx, X), eng.DevArray.from_host(ctx, U)
    Xs, Us = eng.DevArray.from_host(seq_ctx, X), eng.DevArray.from_host(seq_ctx, U)
    d_tot, d_per = eng.DevArray(seq_ctx, (1,)), eng.DevArray(seq_ctx, (W,))
    plist = _candidates(3)
    seq_ctx.use_null_stream()

    def single(model, integ, carry):
        seq_ctx.check(seq_ctx.lib.brov_window_endpoint_se_ragged_dev(seq_ctx.h, model, eng.INTEGRATORS[integ], len(off) - 1, off.ctypes.data, H, DT,
                                                                     Xs.ptr, Us.ptr, carry, d_tot.ptr, d_per.ptr), "se_ragged_dev")
        return float(d_tot.numpy()[0]), d_per.numpy()

    try:
        for integ in ("euler", "rk4"):
            se, _, _, per = _pop_ragged(eng, ctx, THR, integ, plist, Xd, Ud, off, H, DT, 1)
            for j, p in enumerate(plist):
                seq_ctx.set_params(p)
                tot, pw = single(THR, integ, 1)
                e_per, e_tot = rel_err(pw, per[j]), abs(tot - se[j]) / max(1.0, abs(se[j]))
                assert e_per < 1e-12 and e_tot < 1e-12, (integ, j, e_per, e_tot)
    finally:
        seq_ctx.set_params(_lib.default_params())
    # a double-integrator model: gains from a seeded draw, per-bag sums from the plain single-set entry point
    rng = np.random.default_rng(5)
    seq_ctx.set_di_gains(rng.normal(0, 0.05, (8, 3)), rng.normal(0, 0.05, (8, 3)))
    di = _lib.DI_THRUSTER_EULER
    tot, pw = single(di, "rk4", 1)
    want_tot, want_pw = 0.0, []
    for a, b in zip(off[:-1], off[1:]):
        L = int(b - a)
        if L > H:
            d_t, d_p = eng.DevArray(seq_ctx, (1,)), eng.DevArray(seq_ctx, (L - H,))
            eng.window_endpoint_se_dev(di, "rk4", Xs.rows(a, b), Us.rows(a, b), H, DT, d_t, d_p, carry_lag=True, ctx=seq_ctx)
            want_tot += float(d_t.numpy()[0])
            want_pw.append(d_p.numpy())
    e_per, e_tot = rel_err(pw, np.concatenate(want_pw)), abs(tot - want_tot) / max(1.0, abs(want_tot))
    print(f"double integrator: per window {e_per:.2e}  total {e_tot:.2e}")
    assert e_per < 1e-12 and e_tot < 1e-12 and want_tot > 0


# ------------------------------------------------------------------------------------------ 5. argument rules
def test_argument_rules(eng, ctx):
    from bluerov2_dynamics_amd import _lib
    from test_identify_gpu import _recording
    lib, h = ctx.lib, ctx.h
    X, U = _recording(THR, 30, seed=1)
    Xd, Ud = eng.DevArray.from_host(ctx, X), eng.DevArray.from_host(ctx, U)
    pa = (_lib.BrovParams * 2)(_lib.default_params(), _lib.default_params())
    d_se = eng.DevArray(ctx, (2,))
    ctx.use_null_stream()

    def call(off, model=THR, nbags=None, H=5):
        off = np.asarray(off, dtype=np.int64)
        return lib.brov_window_endpoint_pop_ragged_dev(h, model, 0, 2, pa, len(off) - 1 if nbags is None else nbags, off.ctypes.data, H, DT,
                                                       Xd.ptr, Ud.ptr, 1, d_se.ptr, None, None, None)
    assert call([0, 12, 30]) == 0
    good = d_se.numpy()
    assert good[0] > 0
    assert call([1, 12, 30]) == -1 and b"bag_offsets[0] must be 0" in lib.brov_last_error(h)
    assert call([0, 20, 12, 30]) == -1 and b"must not decrease" in lib.brov_last_error(h)
    assert call([0, 30], nbags=-1) == -1 and b"nbags" in lib.brov_last_error(h)
    d_tot, d_per = eng.DevArray(ctx, (1,)), eng.DevArray(ctx, (20,))
    off2 = np.array([0, 12, 30], dtype=np.int64)
    se_dev = lambda off, nb: lib.brov_window_endpoint_se_ragged_dev(h, THR, 0, nb, off.ctypes.data, 5, DT, Xd.ptr, Ud.ptr, 1, d_tot.ptr, d_per.ptr)
    assert se_dev(off2 + 1, 2) == -1 and b"brov_window_endpoint_se_ragged_dev: bag_offsets[0] must be 0" in lib.brov_last_error(h)
    assert se_dev(off2[::-1].copy(), 2) == -1 and b"brov_window_endpoint_se_ragged_dev: bag_offsets[0] must be 0" in lib.brov_last_error(h)
    assert se_dev(np.array([0, 30, 12], dtype=np.int64), 2) == -1
    assert b"brov_window_endpoint_se_ragged_dev: bag_offsets must not decrease" in lib.brov_last_error(h)
    assert se_dev(off2, -1) == -1 and b"brov_window_endpoint_se_ragged_dev: bad bag list" in lib.brov_last_error(h)
    assert lib.brov_window_endpoint_se_ragged_dev(h, THR, 0, 2, off2.ctypes.data, 5, DT, Xd.ptr, Ud.ptr, 1, d_tot.ptr, None) == -1
    assert b"brov_window_endpoint_se_ragged_dev: NULL array" in lib.brov_last_error(h)
    assert lib.brov_window_endpoint_se_ragged_dev(h, THR, 0, 2, off2.ctypes.data, 5, DT, Xd.ptr, Ud.ptr, 1, None, d_per.ptr) == -1
    assert b"brov_window_endpoint_se_ragged_dev: bad argument" in lib.brov_last_error(h)
    assert se_dev(off2, 2) == 0
    for di in (_lib.DI_THRUSTER_EULER, _lib.DI_WRENCH_EULER, _lib.DI_WRENCH_QUAT):
        assert call([0, 12, 30], model=di) == -1                              # gains are not brov_params
        assert b"brov_window_endpoint_pop_ragged_dev: bad argument" in lib.brov_last_error(h)
    # W = 0: se = 0, nothing else written; NaN from the engine
    d_se.copy_from_host(np.array([7.0, 7.0]))
    assert call([0, 5, 5, 9], H=5) == 0 and d_se.numpy().tolist() == [0.0, 0.0]
    assert call([0], nbags=0) == 0
    r = eng.window_pop(THR, "euler", [_lib.default_params()] * 3, X[:9], U[:9], 5, DT, ctx=ctx, bag_offsets=[0, 5, 5, 9])
    assert r.shape == (3,) and np.all(np.isnan(r))
    assert np.isnan(eng.window_rmse(THR, "euler", X[:9], U[:9], 5, DT, ctx=ctx, bag_offsets=[0, 5, 5, 9]))
    # the host forms give the device forms' bits
    se_h, off = np.zeros(2), off2
    assert lib.brov_window_endpoint_pop_ragged(h, THR, 0, 2, pa, 2, off.ctypes.data, 5, DT, X.ctypes.data, U.ctypes.data, 1, se_h.ctypes.data,
                                               None, None) == 0
    assert se_h.tobytes() == good.tobytes()
    tot = ctypes.c_double(0.0)
    assert lib.brov_window_endpoint_se_ragged(h, THR, 0, 2, off.ctypes.data, 5, DT, X.ctypes.data, U.ctypes.data, 1, ctypes.addressof(tot), None) == 0
    assert np.float64(tot.value).tobytes() == d_tot.numpy()[0].tobytes() and tot.value > 0
    assert lib.brov_window_endpoint_pop_ragged(h, THR, 0, 2, pa, 2, (off + 1).ctypes.data, 5, DT, X.ctypes.data, U.ctypes.data, 1, se_h.ctypes.data,
                                               None, None) == -1
    assert b"brov_window_endpoint_pop_ragged: bag_offsets[0] must be 0" in lib.brov_last_error(h)
    assert lib.brov_window_endpoint_pop_ragged(h, THR, 0, 2, pa, 2, off.ctypes.data, 5, DT, None, U.ctypes.data, 1, se_h.ctypes.data, None, None) == -1
    assert b"brov_window_endpoint_pop_ragged: NULL array" in lib.brov_last_error(h)
    assert lib.brov_window_endpoint_se_ragged(h, THR, 0, 2, off.ctypes.data, 5, DT, X.ctypes.data, None, 1, ctypes.addressof(tot), None) == -1
    assert b"brov_window_endpoint_se_ragged: NULL array" in lib.brov_last_error(h)
    assert lib.brov_window_endpoint_se_ragged(h, THR, 2, 2, off.ctypes.data, 5, DT, X.ctypes.data, U.ctypes.data, 1, ctypes.addressof(tot), None) == -1
    assert b"brov_window_endpoint_se_ragged: bad argument" in lib.brov_last_error(h)
    # the engine's forms of the same: window_pop / window_rmse over bags, and the target alone
    rm = eng.window_pop(THR, "euler", [_lib.default_params()] * 2, X, U, 5, DT, ctx=ctx, bag_offsets=off)
    assert np.allclose(rm, np.sqrt(good / (20 * 12)), rtol=1e-15, atol=0)
    assert abs(eng.window_rmse(THR, "euler", X, U, 5, DT, ctx=ctx, bag_offsets=off) - np.sqrt(tot.value / (20 * 12))) < 1e-15
    T = eng.window_target(Xd, 5, off, ctx=ctx)
    assert np.array_equal(T.numpy(), X[_rows(off, 5) + 5])
    # the context is still usable
    assert np.all(np.isfinite(eng.window_pop(THR, "rk4", [_lib.default_params()], X, U, 5, DT, ctx=ctx)))


# ------------------------------------------------------------------------------------------ 6. end to end
def test_fit_over_three_free_decay_recordings():
    """Three free-decay recordings of 200 rows (test_identify_bags_cpu.RELEASES: three releases with way on, thrusters at rest) from
    the rollout kernel of a thruster-model vehicle with quadratic damping x 1.3 and linear damping x 0.8 on surge, sway, heave and
    yaw (test_identify_gpu._fit_case's recipe).  fit_parameters_multi from the nominal vehicle (H = 10, Euler, the default free
    set): a non-increasing history, an end no worse than the generating vehicle, and 4 x the CPU figures
    (tests/test_identify_bags_cpu.py: both 0.0) + 1e-9 on the final RMSE and on the relative parameter error.  fit_parameters on the
    concatenated rows ends with a LARGER RMSE: 2 x H of its windows are scored across a join."""
    from bluerov2_dynamics_amd.fossen import identify
    from bluerov2_dynamics_amd.fossen.BlueROV2 import BlueROV2
    from test_identify_bags_cpu import CPU_BAGS_FINAL_RMSE, CPU_BAGS_REL_PARAM_ERR, H_FIT, RELEASES, ROWS
    names = identify.DEFAULT_FREE
    truth = BlueROV2(dt=DT)
    for n in ("Xu", "Yv", "Zw", "Nr"):
        setattr(truth, n, getattr(truth, n) * 0.8)
        setattr(truth, n + "_abs", getattr(truth, n + "_abs") * 1.3)
    X_all = truth.rollout(RELEASES, np.zeros((3, ROWS - 1, 8)), DT, "euler")["traj"]
    X_list, U_list = [np.ascontiguousarray(X_all[b]) for b in range(3)], [np.zeros((ROWS, 8)) for _ in range(3)]
    assert X_list[0].shape == (ROWS, 12)
    want = np.array([getattr(truth, n) for n in names])
    at_truth = truth.multistep_rmse_endpoint_multi(X_list, U_list, H_FIT, DT, "euler")
    rov = BlueROV2(dt=DT)
    res = rov.fit_parameters_multi(X_list, U_list, DT, H=H_FIT, integrator="euler", free=names, iters=20)
    got = np.array([res.params[n] for n in names])
    err = float(np.linalg.norm(got - want) / np.linalg.norm(want))
    print(f"rmse history {res.rmse_history}\naccepted {res.accepted} n_evals {res.n_evals} windows {res.n_windows}\nfitted {got}\nwanted {want}\n"
          f"rel param err {err:.3e}  final rmse {res.rmse_history[-1]:.3e}  rmse of the generating vehicle {at_truth:.3e}")
    assert res.n_windows == 3 * (ROWS - H_FIT)
    assert np.all(np.diff(res.rmse_history) <= 0.0)
    assert [getattr(rov, n) for n in names] == [res.params[n] for n in names]      # assign=True
    assert res.rmse_history[-1] <= at_truth * (1 + 1e-9) + 1e-12                   # never worse than the vehicle that made the data
    assert res.rmse_history[-1] <= 4 * CPU_BAGS_FINAL_RMSE + 1e-9
    assert err <= 4 * CPU_BAGS_REL_PARAM_ERR + 1e-9
    # the same rows as one recording
    rov2 = BlueROV2(dt=DT)
    res2 = rov2.fit_parameters(np.concatenate(X_list), np.concatenate(U_list), DT, H=H_FIT, integrator="euler", free=names, iters=20)
    print(f"final rmse over bags {res.rmse_history[-1]:.3e}, of the concatenation {res2.rmse_history[-1]:.3e}")
    assert res2.rmse_history[-1] > res.rmse_history[-1]
