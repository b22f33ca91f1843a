"""The covariance of a parameter fit and the draws made from it (fossen/identify.py: fit_parameters(covariance=True),
sample_parameters), the parts that need no GPU: the Levenberg-Marquardt loop is driven by a NumPy evaluator, as in
tests/test_identify_bags_cpu.py."""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest

from bluerov2_dynamics_amd import _lib
from bluerov2_dynamics_amd.fossen import identify

_NAMES = ("Xu", "Zw_abs")
_TRUE = np.array([-9.5, -150.0])
SIGMA, H, NWIN, NX = 1e-3, 4, 200, 12


def _linear_problem(seed=11):
    """End state of window w = S[w] + sum_j theta_j F_j[w], linear in the two free parameters; the recording's scored rows are
    the end states at the generating values plus Gaussian noise of standard deviation SIGMA."""
    rng = np.random.default_rng(seed)
    S = rng.normal(0, 1, (NWIN, NX))
    F = rng.normal(0, 1, (2, NWIN, NX)) * np.array([0.1, 0.01])[:, None, None]
    X = np.zeros((NWIN + H, NX))
    X[H:] = S + np.tensordot(_TRUE, F, 1) + rng.normal(0, SIGMA, (NWIN, NX))
    calls = []

    def evaluator(model, integrator, params_list, X_, U_, H_, dt, carry_lag=True, endpoints=False):
        calls.append(len(params_list))
        th = np.array([[identify.get_param(p, n) for n in _NAMES] for p in params_list])
        E = S[None] + np.tensordot(th, F, 1)
        rmse = np.sqrt(np.mean((E - X_[None, H_:]) ** 2, axis=(1, 2)))
        return (rmse, E) if endpoints else rmse
    return X, np.zeros((NWIN + H, 6)), S, F, evaluator, calls


def _rov():
    return SimpleNamespace(MODEL=_lib.WRENCH_EULER, Xu=-13.7, Zw_abs=-190.0)


def test_covariance_on_a_linear_model():
    X, U, S, F, evaluator, calls = _linear_problem()
    weights = np.linspace(0.5, 2.0, NX)
    res = identify.fit_parameters(_rov(), X, U, 0.02, H=H, free=_NAMES, iters=6, evaluator=evaluator, covariance=True, weights=weights)
    theta = np.array([res.params[n] for n in _NAMES])
    assert res.covariance.shape == (2, 2) and np.array_equal(res.covariance, res.covariance.T)
    assert calls[-1] == 3 and res.n_evals == sum(calls)                 # the last population call: the base and two neighbours
    # s^2 (J^T J)^-1 written out: forward differences with the loop's step rule at the fitted point, weighted residual
    delta = 1e-4 * np.maximum(np.abs(theta), 1.0)
    E0 = S + np.tensordot(theta, F, 1)
    J = np.stack([((S + np.tensordot(theta + delta[j] * np.eye(2)[j], F, 1)) - E0) * weights / delta[j] for j in range(2)], -1).reshape(-1, 2)
    r = ((E0 - X[H:]) * weights).reshape(-1)
    s2 = r @ r / (NWIN * NX - 2)
    want = s2 * np.linalg.inv(J.T @ J)
    assert np.max(np.abs(res.covariance - want)) <= 1e-10 * np.max(np.abs(want)), (res.covariance, want)
    # the fit itself: within 4 standard deviations of the generating values
    sd = np.sqrt(np.diag(res.covariance))
    print("fitted - true in standard deviations:", (theta - _TRUE) / sd)
    assert np.all(np.abs(theta - _TRUE) < 4 * sd)


def test_residual_variance_matches_the_noise():
    """Unweighted, s^2 estimates SIGMA^2 from W nx - m = 2398 residuals: relative standard error sqrt(2 / 2398) = 2.9 %, so 15 % is
    five of them."""
    X, U, S, F, evaluator, _ = _linear_problem()
    res = identify.fit_parameters(_rov(), X, U, 0.02, H=H, free=_NAMES, iters=6, evaluator=evaluator, covariance=True)
    J = F.reshape(2, -1).T
    s2 = res.covariance[0, 0] / np.linalg.inv(J.T @ J)[0, 0]
    assert abs(s2 / SIGMA ** 2 - 1.0) < 0.15, s2


def test_default_path_is_unchanged():
    X, U, _, _, evaluator, calls = _linear_problem()
    kw = dict(H=H, free=_NAMES, iters=6, evaluator=evaluator)
    default = identify.fit_parameters(_rov(), X, U, 0.02, **kw)
    n_default_calls = len(calls)
    off = identify.fit_parameters(_rov(), X, U, 0.02, covariance=False, **kw)
    assert len(calls) == 2 * n_default_calls
    on = identify.fit_parameters(_rov(), X, U, 0.02, covariance=True, **kw)
    assert default.covariance is None and off.covariance is None and on.covariance is not None
    for other in (off, on):
        assert other.params == default.params and other.rmse_history == default.rmse_history and other.accepted == default.accepted
        assert other.n_windows == default.n_windows
        assert ctypes.string_at(ctypes.byref(other.brov_params), ctypes.sizeof(other.brov_params)) == \
            ctypes.string_at(ctypes.byref(default.brov_params), ctypes.sizeof(default.brov_params))
    assert off.n_evals == default.n_evals and on.n_evals == default.n_evals + 3


# ------------------------------------------------------------------------------------------ sample_parameters
def _result(cov):
    base = _lib.default_params()
    base.m, base.current[1] = 12.5, 0.3                    # not free: must reach every draw
    for n, v in zip(_NAMES, _TRUE):
        identify.set_param(base, n, v)
    return identify.FitResult(params=dict(zip(_NAMES, _TRUE.tolist())), rmse_history=[0.0], accepted=[], n_evals=0, brov_params=base,
                              covariance=cov)


def _theta(ps):
    return np.array([[identify.get_param(p, n) for n in _NAMES] for p in ps])


_COV = np.array([[0.04, 0.3], [0.3, 9.0]])                # standard deviations 0.2 and 3, correlation 0.5


def test_sample_parameters_moments_and_determinism():
    res = _result(_COV)
    n = 20000
    a, b, c = (_theta(identify.sample_parameters(res, n, seed=s)) for s in (3, 3, 4))
    assert np.array_equal(a, b) and not np.array_equal(a, c)
    sd_max = np.sqrt(_COV.diagonal().max())
    # standard errors: sd / sqrt(n) = 0.7 % of sd for the mean, sd^2 sqrt(2 / n) = 1 % of sd^2 for a variance
    assert np.max(np.abs(a.mean(0) - _TRUE)) < 0.05 * sd_max
    assert np.max(np.abs(np.cov(a.T) - _COV)) < 0.05 * sd_max ** 2
    small = np.abs(np.cov(a.T)[0, 0] - _COV[0, 0])        # the small variance on its own scale as well
    assert small < 0.05 * _COV[0, 0]


def test_sample_parameters_bounds_fixed_fields_and_errors():
    res = _result(_COV)
    bounds = {"Xu": (-9.6, -9.45), "Zw_abs": (-151.0, np.inf)}
    ps = identify.sample_parameters(res, 500, seed=1, bounds=bounds)
    th = _theta(ps)
    assert len(ps) == 500 and all(isinstance(p, _lib.BrovParams) for p in ps)
    assert th[:, 0].min() == -9.6 and th[:, 0].max() == -9.45 and th[:, 1].min() == -151.0 and th[:, 1].max() > -150.0
    free = _theta(identify.sample_parameters(res, 500, seed=1))
    inside = (free[:, 0] > -9.6) & (free[:, 0] < -9.45) & (free[:, 1] > -151.0)
    assert inside.any() and np.array_equal(th[inside], free[inside])    # clipping moves only what lies outside
    # every field that is not free is the fit's
    want = identify.copy_params(res.brov_params)
    for p in ps[:20]:
        q = identify.copy_params(p)
        for n, v in zip(_NAMES, _TRUE):
            identify.set_param(q, n, v)
        assert ctypes.string_at(ctypes.byref(q), ctypes.sizeof(q)) == ctypes.string_at(ctypes.byref(want), ctypes.sizeof(want))
        assert p.m == 12.5 and p.current[1] == 0.3
    with pytest.raises(ValueError, match="covariance"):
        identify.sample_parameters(_result(None), 3)
    with pytest.raises(ValueError, match="not free"):
        identify.sample_parameters(res, 3, bounds={"zb": (0, 1)})


def test_sample_parameters_clips_negative_eigenvalues():
    """A rank-one covariance whose second eigenvalue has rounded to a small negative number: the draws lie on the line."""
    v = np.array([0.2, 3.0])
    cov = np.outer(v, v) - 1e-15 * np.eye(2)
    assert np.linalg.eigvalsh(cov).min() < 0
    d = _theta(identify.sample_parameters(_result(cov), 200, seed=2)) - _TRUE
    assert np.all(np.isfinite(d)) and np.std(d[:, 0]) > 0.1
    assert np.max(np.abs(d[:, 0] * v[1] - d[:, 1] * v[0])) < 1e-6
