"""Parameter identification over several recordings ("bags"), the parts that need no GPU: the bindings of the ragged window
evaluator, the window numbering and the host target gather, the `evaluator` seam with and without bags, the argument checks of
fit_parameters_multi, and the Levenberg-Marquardt loop over three free-decay recordings with the C oracle as evaluator."""
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

from conftest import REPO

from bluerov2_dynamics_amd import _lib
from bluerov2_dynamics_amd.fossen import identify

RAGGED = ("brov_window_endpoint_pop_ragged", "brov_window_endpoint_pop_ragged_dev", "brov_window_endpoint_se_ragged",
          "brov_window_endpoint_se_ragged_dev")


def test_ragged_declarations_are_bound():
    txt = open(os.path.join(REPO, "include", "brov2.h")).read()
    for name in RAGGED:
        assert re.search(r"BROV_API\s+int\s+" + name + r"\s*\(", txt), name
        assert name in _lib.SIGNATURES, name
    lib = _lib.load_library()
    assert lib.brov_window_endpoint_pop_ragged_dev.argtypes[4] == _lib.ctypes.POINTER(_lib.BrovParams)
    assert len(lib.brov_window_endpoint_pop_ragged_dev.argtypes) == 16 and len(lib.brov_window_endpoint_pop_ragged.argtypes) == 15
    assert len(lib.brov_window_endpoint_se_ragged_dev.argtypes) == 12 and len(lib.brov_window_endpoint_se_ragged.argtypes) == 12
    # without a ctx every one of them refuses before touching a device
    off = np.array([0, 5], dtype=np.int64)
    assert lib.brov_window_endpoint_pop_ragged(None, 0, 0, 1, None, 1, off.ctypes.data, 2, 0.02, None, None, 1, None, None, None) == -1
    assert lib.brov_window_endpoint_pop_ragged_dev(None, 0, 0, 1, None, 1, off.ctypes.data, 2, 0.02, None, None, 1, None, None, None, None) == -1
    assert lib.brov_window_endpoint_se_ragged(None, 0, 0, 1, off.ctypes.data, 2, 0.02, None, None, 1, None, None) == -1
    assert lib.brov_window_endpoint_se_ragged_dev(None, 0, 0, 1, off.ctypes.data, 2, 0.02, None, None, 1, None, None) == -1


def test_window_rows_hand_built():
    """Bags of 3, 0, 5, 2 and 2 rows at H = 2: 1, 0, 3, 0, 0 windows.  Window k of bag b starts at row offsets[b] + k."""
    off = [0, 3, 3, 8, 10, 12]
    assert identify.window_rows(off, 2).tolist() == [0, 3, 4, 5]
    assert identify.window_rows(off, 0).tolist() == list(range(12))
    assert identify.window_rows(off, 5).tolist() == [] and identify.window_rows([0], 1).tolist() == []
    assert identify.window_rows(off, 4).tolist() == [3]
    for bad in ([1, 3], [0, 4, 3], []):
        with pytest.raises(ValueError):
            identify.window_rows(bad, 2)


# ---- a model that is linear in (Xu, Zw_abs, zb), over bags: end state of window w = X[row_w] + sum_j theta_j F_j[w] ----------
_NAMES = ("Xu", "Zw_abs", "zb")
_TRUE = np.array([-9.5, -150.0, -0.03])
_LENS = (9, 0, 4, 5, 17)                                   # with H = 4: 5, 0, 0, 1 and 13 windows


def _linear_bag_problem(H=4, seed=7):
    rng = np.random.default_rng(seed)
    off = np.concatenate([[0], np.cumsum(_LENS)]).astype(np.int64)
    X = rng.normal(0, 1, (int(off[-1]), 12))
    rows = np.concatenate([np.arange(o, o + max(L - H, 0)) for o, L in zip(off[:-1], _LENS)]).astype(np.int64)   # written out, not window_rows
    F = rng.normal(0, 1, (3, rows.size, 12)) * np.array([0.1, 0.01, 10.0])[:, None, None]
    for w, r in enumerate(rows):                           # noise-free inside every bag; the rows across a join are unrelated noise
        X[r + H] = X[r] + np.tensordot(_TRUE, F[:, w], 1)
    seen = []

    def evaluator(model, integrator, params_list, X_, U_, H_, dt, carry_lag=True, endpoints=False, bag_offsets=None):
        seen.append(None if bag_offsets is None else np.asarray(bag_offsets).tolist())
        th = np.array([[identify.get_param(p, n) for n in _NAMES] for p in params_list])
        E = X_[None, rows] + np.tensordot(th, F, 1)
        rmse = np.sqrt(np.mean((E - X_[None, rows + H_]) ** 2, axis=(1, 2)))
        return (rmse, E) if endpoints else rmse
    return X, np.zeros((int(off[-1]), 6)), off, H, rows, F, evaluator, seen


def _rov(**kw):
    return SimpleNamespace(MODEL=_lib.WRENCH_EULER, **{"Xu": -13.7, "Zw_abs": -190.0, "zb": -0.01, **kw})


def test_host_target_gather_one_gauss_newton_step_is_exact():
    """The evaluator returns NumPy end states in window order; the loop must gather its target with the same numbering.  The
    problem is linear, so ONE Gauss-Newton step lands on the generating values -- if the residual is formed against X[row + H] of
    the right rows.  Against X[H:] (the one-recording target) the shapes do not even match; against any other rows the step is off."""
    X, U, off, H, rows, F, evaluator, seen = _linear_bag_problem()
    res = identify.fit_parameters(_rov(), X, U, 0.02, H=H, free=_NAMES, iters=1, evaluator=evaluator, bag_offsets=off)
    got = np.array([res.params[n] for n in _NAMES])
    assert np.max(np.abs(got - _TRUE)) < 1e-10, got - _TRUE
    assert res.accepted == [True] and res.rmse_history[1] < 1e-10 < res.rmse_history[0]
    assert res.n_windows == rows.size == 19
    assert len(seen) == 2 and all(s == off.tolist() for s in seen)          # both population calls carry the bags
    # the list form stacks the same rows and builds the same offsets
    Xl = [X[a:b] for a, b in zip(off[:-1], off[1:])]
    Ul = [U[a:b] for a, b in zip(off[:-1], off[1:])]
    res2 = identify.fit_parameters_multi(_rov(), Xl, Ul, 0.02, H=H, free=_NAMES, iters=1, evaluator=evaluator)
    assert res2.params == res.params and res2.rmse_history == res.rmse_history and seen[-1] == off.tolist()
    # the same rows as ONE recording: the windows across the joins are scored against unrelated rows, and the fit is biased
    def joined(model, integrator, params_list, X_, U_, H_, dt, carry_lag=True, endpoints=False):
        n = X_.shape[0] - H_
        Fj = np.zeros((3, n, 12))
        Fj[:, rows] = F
        th = np.array([[identify.get_param(p, k) for k in _NAMES] for p in params_list])
        E = X_[None, :n] + np.tensordot(th, Fj, 1)
        rmse = np.sqrt(np.mean((E - X_[None, H_:]) ** 2, axis=(1, 2)))
        return (rmse, E) if endpoints else rmse
    res3 = identify.fit_parameters(_rov(), X, U, 0.02, H=H, free=_NAMES, iters=3, evaluator=joined)
    assert res3.n_windows == X.shape[0] - H and res3.rmse_history[-1] > 0.1          # cannot reach zero: jumps at the joins


def test_legacy_evaluator_without_the_keyword_still_works():
    """An evaluator written before bags existed (no bag_offsets keyword, tests/test_identify_cpu.py's kind) is called exactly as
    before when no bags are given -- and told plainly (TypeError from the call) when bags are given to it."""
    from test_identify_cpu import _linear_problem, _NAMES as names, _TRUE as true, _rov as rov
    X, U, H, evaluator, calls = _linear_problem()
    res = identify.fit_parameters(rov(), X, U, 0.02, H=H, free=names, iters=1, evaluator=evaluator)
    assert np.max(np.abs(np.array([res.params[n] for n in names]) - true)) < 1e-10
    assert res.n_windows == X.shape[0] - H and calls[0] == 4
    with pytest.raises(TypeError):
        identify.fit_parameters(rov(), X, U, 0.02, H=H, free=names, iters=1, evaluator=evaluator, bag_offsets=[0, X.shape[0]])


def test_fit_parameters_multi_argument_checks():
    X, U, off, H, rows, F, evaluator, seen = _linear_bag_problem()
    Xl = [X[a:b] for a, b in zip(off[:-1], off[1:])]
    Ul = [U[a:b] for a, b in zip(off[:-1], off[1:])]
    with pytest.raises(ValueError, match="recordings"):
        identify.fit_parameters_multi(_rov(), Xl, Ul[:-1], 0.02, H=H, free=_NAMES, evaluator=evaluator)
    with pytest.raises(ValueError, match="recording 4: U has 16 rows, X has 17"):
        identify.fit_parameters_multi(_rov(), Xl, Ul[:-1] + [Ul[-1][:-1]], 0.02, H=H, free=_NAMES, evaluator=evaluator)
    with pytest.raises(ValueError):
        identify.fit_parameters_multi(_rov(), [], [], 0.02, H=H, free=_NAMES, evaluator=evaluator)
    with pytest.raises(ValueError, match="no window"):
        identify.fit_parameters_multi(_rov(), Xl[1:4], Ul[1:4], 0.02, H=5, free=_NAMES, evaluator=evaluator)
    with pytest.raises(ValueError, match="bag_offsets ends at row"):
        identify.fit_parameters(_rov(), X, U, 0.02, H=H, free=_NAMES, evaluator=evaluator, bag_offsets=off[:-1])
    with pytest.raises(ValueError, match="must start at 0"):
        identify.fit_parameters(_rov(), X, U, 0.02, H=H, free=_NAMES, evaluator=evaluator, bag_offsets=off + 1)
    assert seen == []
    # a U longer than its X is cut to X's rows (row-aligned), as the one-recording form accepts it
    Xs, Us, o = identify.stack_recordings(Xl, [np.concatenate([u, np.ones((2, 6))]) for u in Ul], _lib.WRENCH_EULER)
    assert np.array_equal(Xs, X) and np.array_equal(Us, U) and o.tolist() == off.tolist() and o.dtype == np.int64


# ---- three free-decay recordings, the C oracle as evaluator ---------------------------------------------------------------
# The recordings of the GPU end-to-end test (tests/test_window_bags_gpu.py): three releases with way on, thrusters at rest, 200 rows
# each, dt = 0.02, H = 10, Euler.
RELEASES = np.array([[0, 0, 0, 0, 0, 0, 0.8, -0.6, 0.5, 0, 0, 0.9],
                     [0, 0, 0, 0, 0, 0, -0.5, 0.7, -0.4, 0, 0, -0.6],
                     [0, 0, 0, 0, 0, 0, 0.3, 0.4, 0.9, 0, 0, 0.5]], float)
ROWS, H_FIT, DT = 200, 10, 0.02

# figures of test_bags_recoverability_with_the_c_oracle as measured on the CPU (see its docstring).  They are the yardstick of the
# GPU end-to-end test, which may use at most 4x these plus 1e-9.
CPU_BAGS_FINAL_RMSE = 0.0
CPU_BAGS_REL_PARAM_ERR = 0.0


def test_bags_recoverability_with_the_c_oracle():
    """fit_parameters_multi's loop with the C oracle as evaluator, one oracle rollout per bag: thruster Euler model, three
    free-decay recordings (RELEASES, 200 rows each, thrusters at rest so the lag stays zero), H = 10.  The oracle's vehicle
    constants are compiled in; as in tests/test_identify_cpu.py the only brov_params quantity it can vary is the current, so the
    generating vehicle carries a current and its three components are the free parameters (start: no current).

    First the oracle alone: the generating current scores exactly 0 on every bag's windows (the oracle that made the recordings also
    scores them), and the nominal vehicle scores above 1e-4 -- so the figures below are reachable and there is something to fit.
    The same rows as ONE recording score the generating current above 1e-2: the 2 x H windows across the joins end metres away
    from the rows they are compared with.

    Measured here: relative parameter error 0.0, final RMSE 0.0 (initial RMSE 1.057e-2, 10 accepted steps, 570 windows; the rows as one
    recording score the generating current 8.5e-2).  The asserts allow another host's arithmetic 1e-9 on
    both, as tests/test_identify_cpu.py does."""
    from oracle import fossen_c as fc
    true = np.array([0.10, -0.05, 0.02])
    U0 = np.zeros((ROWS - 1, 8))
    X_list = [fc.rollout(fc.MODEL_THRUSTER_EULER, fc.INTEG_EULER, x0[None], U0[None], DT, current=true)["traj"][0] for x0 in RELEASES]
    U_list = [np.zeros((ROWS, 8)) for _ in RELEASES]
    assert all(X.shape == (ROWS, 12) for X in X_list)

    def evaluator(model, integrator, params_list, X_, U_, H_, dt_, carry_lag=True, endpoints=False, bag_offsets=None):
        assert model == _lib.THRUSTER_EULER and integrator == "euler" and H_ == H_FIT and bag_offsets is not None
        E = []
        for p in params_list:
            ends = []
            for a, b in zip(bag_offsets[:-1], bag_offsets[1:]):
                n = max(int(b - a) - H_, 0)
                if n:
                    Uw = np.stack([U_[a + k:a + k + H_] for k in range(n)])
                    ends.append(fc.rollout(fc.MODEL_THRUSTER_EULER, fc.INTEG_EULER, X_[a:a + n], Uw, dt_, current=np.array(p.current[:]),
                                           store=False)["xT"])
            E.append(np.concatenate(ends))
        E = np.stack(E)
        rows = identify.window_rows(bag_offsets, H_)
        rmse = np.sqrt(np.mean((E - X_[None, rows + H_]) ** 2, axis=(1, 2)))
        return (rmse, E) if endpoints else rmse

    Xs, Us, off = identify.stack_recordings(X_list, U_list, _lib.THRUSTER_EULER)
    at = lambda cur: _lib.BrovParams(current=(ctypes_arr(cur)))
    r_true, r_nom = (float(evaluator(_lib.THRUSTER_EULER, "euler", [at(c)], Xs, Us, H_FIT, DT, bag_offsets=off)[0]) for c in (true, np.zeros(3)))
    joined = fc.window_rmse(fc.MODEL_THRUSTER_EULER, fc.INTEG_EULER, Xs, Us, H_FIT, DT, current=true)
    print(f"oracle alone: generating current {r_true:.3e}, nominal {r_nom:.3e}; the rows as one recording, generating current {joined:.3e}")
    assert r_true == 0.0 and r_nom > 1e-4 and joined > 1e-2

    rov = SimpleNamespace(MODEL=_lib.THRUSTER_EULER, current_speed=np.zeros(3))
    names = ("current_x", "current_y", "current_z")
    res = identify.fit_parameters_multi(rov, X_list, U_list, DT, H=H_FIT, free=names, iters=20, evaluator=evaluator)
    got = np.array([res.params[n] for n in names])
    err = float(np.linalg.norm(got - true) / np.linalg.norm(true))
    print(f"rel param err {err:.3e}  final rmse {res.rmse_history[-1]:.3e}  rmse0 {res.rmse_history[0]:.3e}  accepted {sum(res.accepted)}  "
          f"windows {res.n_windows}")
    assert res.n_windows == 3 * (ROWS - H_FIT)
    assert np.all(np.diff(res.rmse_history) <= 0.0)
    assert res.rmse_history[0] == r_nom
    assert err <= CPU_BAGS_REL_PARAM_ERR + 1e-9 and res.rmse_history[-1] <= CPU_BAGS_FINAL_RMSE + 1e-9


def ctypes_arr(v):
    return (_lib.ctypes.c_double * 3)(*[float(x) for x in v])
