"""Parameter identification, the parts that need no GPU: the bindings, the NumPy statement of the finite-difference normal
equations, and fit_parameters' Levenberg-Marquardt loop driven through its `evaluator` seam by NumPy / C-oracle models."""
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

from conftest import REPO

from bluerov2_dynamics_amd import _lib
from bluerov2_dynamics_amd.fossen import identify


def test_new_declarations_are_bound():
    txt = open(os.path.join(REPO, "include", "brov2.h")).read()
    for name in ("brov_window_endpoint_pop", "brov_window_endpoint_pop_dev", "brov_fd_normal_eq_dev"):
        assert re.search(r"BROV_API\s+int\s+" + name + r"\s*\(", txt), name
        assert name in _lib.SIGNATURES, name
    lib = _lib.load_library()
    assert lib.brov_window_endpoint_pop_dev.argtypes[4] == _lib.ctypes.POINTER(_lib.BrovParams)
    # without a ctx every one of them refuses before touching a device
    assert lib.brov_window_endpoint_pop(None, 0, 0, 1, None, 0, 0, 0.02, None, None, 1, None, None) == -1
    assert lib.brov_fd_normal_eq_dev(None, 12, 1, 1, None, None, None, None, None, None) == -1


def test_normal_equations_numpy_hand_built():
    """Three parameters, two windows of two coordinates: J, r written out by hand from the formulas of include/brov2.h."""
    E0 = np.array([[1.0, 2.0], [3.0, 5.0]])
    tgt = np.array([[0.5, 2.5], [3.0, 4.0]])
    delta = np.array([0.5, -0.25, 2.0])
    w = np.array([2.0, 0.5])
    D = [np.array([[1.0, 0.0], [2.0, -1.0]]), np.array([[0.5, 0.5], [0.0, 1.0]]), np.array([[-2.0, 4.0], [6.0, 0.0]])]
    E = np.stack([E0] + [E0 + d for d in D])
    # rows (k, i) = (0,0), (0,1), (1,0), (1,1); column j = w_i * D_j[k, i] / delta_j
    J = np.array([[2 * 1.0 / 0.5, 2 * 0.5 / -0.25, 2 * -2.0 / 2.0],
                  [0.5 * 0.0 / 0.5, 0.5 * 0.5 / -0.25, 0.5 * 4.0 / 2.0],
                  [2 * 2.0 / 0.5, 2 * 0.0 / -0.25, 2 * 6.0 / 2.0],
                  [0.5 * -1.0 / 0.5, 0.5 * 1.0 / -0.25, 0.5 * 0.0 / 2.0]])
    r = np.array([2 * 0.5, 0.5 * -0.5, 2 * 0.0, 0.5 * 1.0])
    JtJ, Jtr = identify.normal_eq_numpy(E, tgt, delta, w)
    assert np.allclose(JtJ, J.T @ J, rtol=0, atol=1e-14) and np.allclose(Jtr, J.T @ r, rtol=0, atol=1e-14)
    JtJ1, Jtr1 = identify.normal_eq_numpy(E, tgt, delta)
    J1 = J / np.array([2.0, 0.5, 2.0, 0.5])[:, None]
    assert np.allclose(JtJ1, J1.T @ J1, atol=1e-14) and np.allclose(Jtr1, J1.T @ (r / np.array([2.0, 0.5, 2.0, 0.5])), atol=1e-14)


# ---- a model that is linear in (Xu, Zw_abs, zb): end state = X[k] + sum_j theta_j F_j[k] -------------------------------
_NAMES = ("Xu", "Zw_abs", "zb")
_TRUE = np.array([-9.5, -150.0, -0.03])


def _linear_problem(N=60, H=4, seed=5):
    rng = np.random.default_rng(seed)
    X = rng.normal(0, 1, (N, 12))
    F = rng.normal(0, 1, (3, N - H, 12)) * np.array([0.1, 0.01, 10.0])[:, None, None]
    for k in range(N - H):                                 # noise-free: the generating parameters score (almost) exactly 0
        X[k + H] = X[k] + np.tensordot(_TRUE, F[:, k], 1)
    calls = []

    def evaluator(model, integrator, params_list, X_, U_, H_, dt, carry_lag=True, endpoints=False):
        calls.append(len(params_list))
        th = np.array([[identify.get_param(p, n) for n in _NAMES] for p in params_list])
        E = X_[None, :N - H_] + np.tensordot(th, F, 1)
        rmse = np.sqrt(np.mean((E - X_[None, H_:]) ** 2, axis=(1, 2)))
        return (rmse, E) if endpoints else rmse
    return X, np.zeros((N, 6)), H, evaluator, calls


def _rov(**kw):
    return SimpleNamespace(MODEL=_lib.WRENCH_EULER, **{"Xu": -13.7, "Zw_abs": -190.0, "zb": -0.01, **kw})


def test_fit_linear_model_one_gauss_newton_step_is_exact():
    X, U, H, evaluator, calls = _linear_problem()
    res = identify.fit_parameters(_rov(), X, U, 0.02, H=H, free=_NAMES, iters=1, evaluator=evaluator)
    got = np.array([res.params[n] for n in _NAMES])
    assert np.max(np.abs(got - _TRUE)) < 1e-10, got - _TRUE
    assert res.accepted == [True] and len(res.rmse_history) == 2 and res.rmse_history[1] < 1e-10 < res.rmse_history[0]
    # one population call with m + 1 candidates, one with the lambda trials
    assert calls[0] == 4 and len(calls) == 2 and res.n_evals == sum(calls)
    assert [identify.get_param(res.brov_params, n) for n in _NAMES] == [res.params[n] for n in _NAMES]


def test_fit_history_non_increasing_and_bounds_respected():
    X, U, H, evaluator, _ = _linear_problem()
    bounds = {"Xu": (-12.0, -11.0), "zb": (-0.02, 0.0)}          # the generating values lie outside both boxes
    res = identify.fit_parameters(_rov(), X, U, 0.02, H=H, free=_NAMES, iters=8, bounds=bounds, evaluator=evaluator,
                                  weights=np.linspace(0.5, 1.5, 12))
    h = np.array(res.rmse_history)
    assert len(h) >= 2 and np.all(np.diff(h) <= 0.0) and h[-1] < h[0]
    assert -12.0 <= res.params["Xu"] <= -11.0 and -0.02 <= res.params["zb"] <= 0.0
    assert len(res.accepted) == len(h) - 1
    # a start point outside its box is moved inside before the first evaluation
    res2 = identify.fit_parameters(_rov(Xu=-20.0), X, U, 0.02, H=H, free=("Xu",), iters=2, bounds={"Xu": (-12.0, -11.0)},
                                   evaluator=evaluator)
    assert -12.0 <= res2.params["Xu"] <= -11.0


def test_fit_rejects_unknown_names():
    X, U, H, evaluator, calls = _linear_problem()
    with pytest.raises(ValueError):
        identify.fit_parameters(_rov(), X, U, 0.02, H=H, free=("Xu", "no_such_attribute"), evaluator=evaluator)
    with pytest.raises(ValueError):
        identify.fit_parameters(_rov(), X, U, 0.02, H=H, free=(), evaluator=evaluator)
    with pytest.raises(ValueError):
        identify.fit_parameters(_rov(), X, U, 0.02, H=H, free=("Xu",), bounds={"Yv": (0, 1)}, evaluator=evaluator)
    assert calls == []
    assert set(("m", "volume", "zb", "Ix", "Iy", "Iz", "Xu_dot", "Nr_dot", "Kp", "Mq_abs")) <= set(identify.FREE_NAMES)


# figures of test_recoverability_with_the_c_oracle as measured: the loop lands on the generating values bit for bit (the oracle
# that made the recording also scores it, so their residual is exactly 0 and the loop stops there).  They are also the yardstick
# of the GPU end-to-end test (tests/test_identify_gpu.py), which may use at most 4x these plus 1e-9.
CPU_REL_PARAM_ERR = 0.0
CPU_RMSE_RATIO = 0.0
CPU_FINAL_RMSE = 0.0


def test_recoverability_with_the_c_oracle():
    """The same loop with the C oracle's rollout as evaluator: wrench Euler model, H = 10, a noise-free 600-row recording driven by
    AR(1) inputs (oracle/controls.py).  The oracle's vehicle constants are compiled in; the only brov_params quantity it can
    vary is the current, so the three components of `current` are the free parameters (start: no current).

    Measured here: relative parameter error |theta - theta*| / |theta*| = 0.0, final / initial window RMSE = 0.0 (initial RMSE
    8.805e-3, 7 accepted steps): the generating values are reached exactly.  The asserts do not demand that of another host's
    arithmetic: 1e-9 on both figures -- a forward-difference Jacobian costs convergence rate, not accuracy, on a residual that can
    reach zero, so what remains is rounding in the 3 x 3 solve (condition ~1e2) on steps that are already below 1e-6."""
    from oracle import controls, fossen_c as fc
    N, H, dt = 600, 10, 0.02
    true = np.array([0.10, -0.05, 0.02])
    U = controls.controls_ar1(21, 0, 1, N, nu=6)[0] * np.array([20.0, 20.0, 20.0, 2.0, 2.0, 2.0])
    X = fc.rollout(fc.MODEL_WRENCH_EULER, fc.INTEG_EULER, np.zeros((1, 12)), U[None], dt, current=true)["traj"][0][:N]
    nwin = N - H
    Uw = np.stack([U[k:k + H] for k in range(nwin)])

    def evaluator(model, integrator, params_list, X_, U_, H_, dt_, carry_lag=True, endpoints=False):
        assert model == _lib.WRENCH_EULER and integrator == "euler" and H_ == H
        E = np.stack([fc.rollout(fc.MODEL_WRENCH_EULER, fc.INTEG_EULER, X_[:nwin], Uw, dt_, current=np.array(p.current[:]),
                                 store=False)["xT"] for p in params_list])
        rmse = np.sqrt(np.mean((E - X_[None, H:]) ** 2, axis=(1, 2)))
        return (rmse, E) if endpoints else rmse

    rov = SimpleNamespace(MODEL=_lib.WRENCH_EULER, current_speed=np.zeros(3))
    res = identify.fit_parameters(rov, X, U, dt, H=H, free=("current_x", "current_y", "current_z"), iters=20, evaluator=evaluator)
    got = np.array([res.params[n] for n in ("current_x", "current_y", "current_z")])
    err = float(np.linalg.norm(got - true) / np.linalg.norm(true))
    ratio = res.rmse_history[-1] / res.rmse_history[0]
    print(f"rel param err {err:.3e}  rmse ratio {ratio:.3e}  rmse0 {res.rmse_history[0]:.3e}  accepted {sum(res.accepted)}")
    assert np.all(np.diff(res.rmse_history) <= 0.0)
    assert err < 1e-9 and ratio < 1e-9
