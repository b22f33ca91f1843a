"""Fit the Fossen model's parameters to a recording: Levenberg-Marquardt on the sliding-window endpoint error.

The residual is what multistep_rmse_endpoint_physics scores (training/train_tank_brov2_full_comparison.py:469-487): the end
state of every H-step window minus the recorded state.  One iteration is

  1. ONE population call (engine.window_pop) with the current parameters and one forward-difference neighbour per free
     parameter: m + 1 candidates, their window end states stay on the device;
  2. ONE normal-equation call (engine.fd_normal_eq): J^T J and J^T r from those end states;
  3. a host solve of (J^T J + lambda diag(J^T J)) step = -J^T r for several lambda at once (lambda = 0, Gauss-Newton, among them);
  4. ONE more population call that scores all those trial points together; the best one is taken
  5. only if its window RMSE is below the current one, so `rmse_history` never increases.

`evaluator` is the seam: any callable with window_pop's contract can stand in for the engine -- tests drive the same loop with
NumPy models, and a derivative-free optimiser can call the engine's evaluator directly.  When the evaluator hands back its end
states as a NumPy array the normal equations are formed on the host (normal_eq_numpy, the same formulas).

Several recordings ("bags": free decay on each axis, a driven run, ...) are fitted together with fit_parameters_multi, or with
fit_parameters(..., bag_offsets=...) on rows that are already stacked.  No window then starts in one recording and is scored against
a row of the next, and every recording is a fresh vehicle (zero thruster lag at its first window): what concatenating the
recordings cannot give.  The evaluator is then called with bag_offsets=...; without bags it never sees that keyword."""
import ctypes
from dataclasses import dataclass, field

import numpy as np

from .. import _lib

_ATTR6 = ("Xu_dot", "Yv_dot", "Zw_dot", "Kp_dot", "Mq_dot", "Nr_dot")
_LIN6 = ("Xu", "Yv", "Zw", "Kp", "Mq", "Nr")
_CURRENT = ("current_x", "current_y", "current_z")


def _fields():
    f = {n: (n, None) for n in ("m", "volume", "zb", "Ix", "Iy", "Iz")}
    for i, (a, l) in enumerate(zip(_ATTR6, _LIN6)):
        f[a], f[l], f[l + "_abs"] = ("added_mass", i), ("lin_damp", i), ("quad_damp", i)
    for i, n in enumerate(_CURRENT):
        f[n] = ("current", i)
    return f


# name of a free parameter -> (field of struct brov_params, index or None).  The vehicle attributes of fossen/_vehicle.py
# (_ATTR6, _LIN6, *_abs, m, volume, zb, Ix..Iz) and the three components of current_speed.
FREE_NAMES = _fields()
DEFAULT_FREE = ("Xu", "Yv", "Zw", "Nr", "Xu_abs", "Yv_abs", "Zw_abs", "Nr_abs")
_FIXED = {n: (n, None) for n in ("rho", "g", "xb", "yb")}


def get_param(p, name):
    fld, i = FREE_NAMES[name]
    return float(getattr(p, fld)) if i is None else float(getattr(p, fld)[i])


def set_param(p, name, value):
    fld, i = FREE_NAMES[name]
    if i is None:
        setattr(p, fld, float(value))
    else:
        getattr(p, fld)[i] = float(value)


def copy_params(p):
    q = _lib.BrovParams()
    ctypes.memmove(ctypes.byref(q), ctypes.byref(p), ctypes.sizeof(q))
    return q


def params_of(rov):
    """struct brov_params of a vehicle: a BrovParams (copied), a drop-in vehicle object (its attributes, synchronised), or any
    object carrying some of the attribute names (the rest of the struct is zero: enough for an evaluator that reads only those)."""
    if isinstance(rov, _lib.BrovParams):
        return copy_params(rov)
    if hasattr(rov, "_sync_params") and hasattr(rov, "_params"):
        rov._sync_params()
        return copy_params(rov._params)
    p = _lib.BrovParams()
    for name, (fld, i) in list(FREE_NAMES.items()) + list(_FIXED.items()):
        if name not in _CURRENT and hasattr(rov, name):
            if i is None:
                setattr(p, fld, float(getattr(rov, name)))
            else:
                getattr(p, fld)[i] = float(getattr(rov, name))
    cs = getattr(rov, "current_speed", None)
    if cs is not None:
        for i, v in enumerate(np.asarray(cs, dtype=float).reshape(3)):
            p.current[i] = v
    return p


def normal_eq_numpy(endpoints, target, delta, weights=None):
    """J^T J and J^T r of include/brov2.h: brov_fd_normal_eq_dev, stated in NumPy.  endpoints [m+1, W, nx] (block 0 = base,
    block j+1 = base + delta[j] e_j), target [W, nx]:  J[(k,i), j] = w_i (E_j[k,i] - E_0[k,i]) / delta_j,
    r[(k,i)] = w_i (E_0[k,i] - target[k,i])."""
    E = np.asarray(endpoints)
    target = np.asarray(target)
    delta = np.asarray(delta).reshape(-1)
    w = np.ones(E.shape[2], dtype=E.dtype) if weights is None else np.asarray(weights).reshape(E.shape[2])
    J = ((E[1:] - E[0]) * w).reshape(len(delta), -1).T / delta
    r = ((E[0] - target) * w).reshape(-1)
    return J.T @ J, J.T @ r


@dataclass
class FitResult:
    params: dict                       # name -> fitted value, in the order of `free`
    rmse_history: list                 # window RMSE before the first iteration and after each one: non-increasing
    accepted: list                     # per iteration: was a step taken
    n_evals: int                       # candidates scored (window evaluations of one parameter set)
    n_windows: int = 0                 # windows scored per candidate (over all bags)
    brov_params: object = field(default=None, repr=False)   # the fitted struct brov_params
    covariance: object = field(default=None, repr=False)    # [m, m] in the order of `free` (fit_parameters(covariance=True)), or None


def _engine_evaluator(ctx):
    from .. import engine

    def evaluate(model, integrator, params_list, X, U, H, dt, carry_lag=True, endpoints=False, bag_offsets=None):
        return engine.window_pop(model, integrator, params_list, X, U, H, dt, carry_lag=carry_lag, endpoints=endpoints, ctx=ctx,
                                 bag_offsets=bag_offsets)
    return evaluate


def window_rows(bag_offsets, H):
    """First row of every window of a bag list, int64 [W]: bag b (rows bag_offsets[b] .. bag_offsets[b+1]-1, L_b of them) has
    max(L_b - H, 0) windows, numbered bag after bag; window k of bag b starts at row bag_offsets[b] + k and is scored against row
    bag_offsets[b] + k + H.  The numbering of include/brov2.h: brov_window_endpoint_pop_ragged."""
    off = np.asarray(bag_offsets, dtype=np.int64).reshape(-1)
    if off.size < 1 or off[0] != 0 or np.any(np.diff(off) < 0):
        raise ValueError("bag_offsets must start at 0 and must not decrease")
    w = np.maximum(np.diff(off) - int(H), 0)
    return np.repeat(off[:-1] - (np.cumsum(w) - w), w) + np.arange(int(w.sum()), dtype=np.int64)


_LAMBDA_TRIALS = (0.0, 1e-2, 1e-1, 1.0, 1e1, 1e2)     # times the running lambda; 0 = the Gauss-Newton step


def fit_parameters(rov, X, U, dt, H=10, integrator="euler", free=DEFAULT_FREE, iters=20, weights=None, bounds=None, carry_lag=True,
                   rel_step=1e-4, evaluator=None, model=None, bag_offsets=None, covariance=False):
    """Fit the parameters named in `free` to the recording X [N,nx], U [N,nu] (see the module docstring).

    bag_offsets: int64 [nbags + 1], first 0, non-decreasing: X and U hold several recordings one after the other, recording b = rows
              bag_offsets[b] .. bag_offsets[b+1]-1 (fit_parameters_multi builds this from a list).  The evaluator is then called
              with bag_offsets=... and scores the windows of window_rows(bag_offsets, H).

    free    : names from FREE_NAMES; an unknown name raises ValueError.
    weights : [nx] weights of the state coordinates in the least-squares objective (None = 1).  Steps are still accepted on the
              unweighted window RMSE, the figure the comparison tables print.
    bounds  : {name: (lo, hi)}; start point, difference neighbours and trial points stay inside.
    rel_step: forward-difference step delta_j = rel_step * max(|theta_j|, 1) (backwards at an upper bound).
    evaluator: callable(model, integrator, params_list, X, U, H, dt, carry_lag=..., endpoints=...) -> rmse [P] or (rmse, E [P, N-H, nx]);
              default: the engine on the vehicle's device context.  With bags it also takes bag_offsets=... and its end states are
              [P, W, nx] in window_rows' order.
    covariance: True = after the loop, one more population call at the fitted point (the base and one forward-difference neighbour
              per free parameter, the loop's delta and bounds rule; counted in n_evals) gives the Gauss-Newton covariance
              FitResult.covariance = s^2 pinv(J^T J), s^2 = r^T r / (W nx - m) with r the weighted residual at the fitted point:
              what sample_parameters draws from.  NaN-filled when W nx <= m.
    Returns a FitResult."""
    names = tuple(free)
    unknown = [n for n in names if n not in FREE_NAMES]
    if unknown:
        raise ValueError(f"unknown parameter name(s) {unknown}: choose from {sorted(FREE_NAMES)}")
    if not names or len(set(names)) != len(names):
        raise ValueError("free must name at least one parameter, each once")
    if len(names) > 48:
        raise ValueError("at most 48 free parameters")
    bounds = dict(bounds or {})
    stray = [n for n in bounds if n not in names]
    if stray:
        raise ValueError(f"bounds given for parameters that are not free: {stray}")
    model = getattr(rov, "MODEL", _lib.THRUSTER_EULER) if model is None else model
    m = len(names)
    base = params_of(rov)
    lo = np.array([bounds.get(n, (-np.inf, np.inf))[0] for n in names], dtype=float)
    hi = np.array([bounds.get(n, (-np.inf, np.inf))[1] for n in names], dtype=float)
    theta = np.clip(np.array([get_param(base, n) for n in names]), lo, hi)

    device = evaluator is None
    if device:
        from .. import engine
        ctx = getattr(rov, "_ctx", None) or getattr(X, "ctx", None) or _lib.default_context()
        evaluator = _engine_evaluator(ctx)
        if isinstance(X, np.ndarray) or isinstance(X, (list, tuple)):      # one upload for the whole fit
            arr = engine._NativeArrays(ctx)
            X = arr.upload(_lib.as_f64(X).reshape(-1, _lib.NX[model]))
            U = arr.upload(_lib.as_f64(U).reshape(-1, _lib.NU[model]))
    N = int(X.shape[0])
    bag_kw = {}
    if bag_offsets is None:
        if N - H <= 0:
            raise ValueError(f"the recording has {N} rows: no window of H = {H} steps fits")
        target = X.rows(H, N) if hasattr(X, "rows") else X[H:]
        n_windows = N - H
    else:
        rows = window_rows(bag_offsets, H)
        off = np.ascontiguousarray(bag_offsets, dtype=np.int64).reshape(-1)
        if int(off[-1]) != N:
            raise ValueError(f"bag_offsets ends at row {int(off[-1])}, the recordings have {N} rows")
        n_windows = int(rows.size)
        if n_windows == 0:
            raise ValueError(f"none of the {off.size - 1} recordings has more than H = {H} rows: no window fits")
        bag_kw = dict(bag_offsets=off)
        if device:
            target = engine.window_target(X, H, off, ctx=ctx)
        else:
            target = np.asarray(X)[rows + H]         # the evaluator's NumPy end states are scored against the same rows

    def candidate(th):
        p = copy_params(base)
        for n, v in zip(names, th):
            set_param(p, n, v)
        return p

    def normal_eq(E, delta):
        if isinstance(E, np.ndarray):
            return normal_eq_numpy(E, np.asarray(target), delta, weights)
        from .. import engine
        return engine.fd_normal_eq(E, target, delta, weights)

    def difference_population(th):
        """the base and its m forward-difference neighbours (backwards at an upper bound), scored with their end states"""
        delta = rel_step * np.maximum(np.abs(th), 1.0)
        delta = np.where(th + delta > hi, -delta, delta)
        pop = [candidate(th)] + [candidate(th + delta[j] * np.eye(m)[j]) for j in range(m)]
        rmse, E = evaluator(model, integrator, pop, X, U, H, dt, carry_lag=carry_lag, endpoints=True, **bag_kw)
        return delta, rmse, E

    history, accepted, n_evals, lam, stalled = [], [], 0, 1e-3, 0
    for _ in range(int(iters)):
        delta, rmse, E = difference_population(theta)
        n_evals += m + 1
        cur = float(rmse[0])
        if not history:
            history.append(cur)
        JtJ, Jtr = normal_eq(E, delta)
        d = np.diag(JtJ).copy()
        d[d <= 0.0] = 1.0
        trials = []
        for f in _LAMBDA_TRIALS:
            A = JtJ + (lam * f) * np.diag(d)
            try:
                step = np.linalg.solve(A, -Jtr)
            except np.linalg.LinAlgError:
                continue
            if np.all(np.isfinite(step)):
                trials.append(np.clip(theta + step, lo, hi))
        took = False
        if trials:
            score = np.asarray(evaluator(model, integrator, [candidate(t) for t in trials], X, U, H, dt, carry_lag=carry_lag,
                                         endpoints=False, **bag_kw), dtype=float)
            n_evals += len(trials)
            score = np.where(np.isfinite(score), score, np.inf)
            b = int(np.argmin(score))
            if score[b] < cur:
                theta, cur, took = trials[b], float(score[b]), True
        lam = max(lam / 3.0, 1e-12) if took else min(lam * 10.0, 1e12)
        accepted.append(took)
        history.append(cur)
        stalled = 0 if took else stalled + 1
        if cur == 0.0 or stalled >= 3:
            break
    cov = None
    if covariance:
        delta, _, E = difference_population(theta)
        n_evals += m + 1
        JtJ, _ = normal_eq(E, delta)
        # r^T r of the weighted residual at the fitted point: block 0 of the end states against the target (one download each)
        E0 = E[0] if isinstance(E, np.ndarray) else _to_host(E.rows(0, 1) if hasattr(E, "rows") else E[0])
        nx = int(E.shape[2])
        w = np.ones(nx) if weights is None else np.asarray(weights, dtype=float).reshape(nx)
        r = (np.asarray(E0, dtype=float).reshape(-1, nx) - np.asarray(_to_host(target), dtype=float).reshape(-1, nx)) * w
        dof = n_windows * nx - m
        s2 = float(np.sum(r * r)) / dof if dof > 0 else np.nan
        cov = s2 * np.linalg.pinv(np.asarray(JtJ, dtype=float), hermitian=True)
    fitted = candidate(theta)
    return FitResult(params={n: float(v) for n, v in zip(names, theta)}, rmse_history=history, accepted=accepted, n_evals=n_evals,
                     brov_params=fitted, n_windows=n_windows, covariance=cov)


def _to_host(a):
    """NumPy copy of a host array, a DevArray or a torch tensor"""
    if isinstance(a, np.ndarray):
        return a
    return a.numpy() if hasattr(a, "ptr") else a.cpu().numpy()


def sample_parameters(result, n, seed=0, bounds=None):
    """n vehicles drawn around a fit: a list of BrovParams whose free parameters are theta_hat + L z, z standard normal from
    np.random.default_rng(seed), L L^T = result.covariance (symmetric eigendecomposition, negative eigenvalues clipped to 0), each
    clipped to bounds {name: (lo, hi)}; every other field is copied from result.brov_params.  Feed the list to engine.rollout_pop
    or rov.simulate_population; rov.log_likelihood_population ranks the draws against a noisy recording (the innovation
    likelihood of an unscented Kalman filter under each draw).  ValueError when the fit was made without covariance=True."""
    if result.covariance is None:
        raise ValueError("the fit carries no covariance: call fit_parameters(..., covariance=True)")
    names = tuple(result.params)
    bounds = dict(bounds or {})
    stray = [k for k in bounds if k not in names]
    if stray:
        raise ValueError(f"bounds given for parameters that are not free: {stray}")
    C = np.asarray(result.covariance, dtype=float)
    if C.shape != (len(names), len(names)) or not np.all(np.isfinite(C)):
        raise ValueError("the covariance must be a finite [m, m] array in the order of the fitted parameters")
    lam, V = np.linalg.eigh(0.5 * (C + C.T))
    L = V * np.sqrt(np.clip(lam, 0.0, None))
    theta = np.array([result.params[k] for k in names], dtype=float)
    lo = np.array([bounds.get(k, (-np.inf, np.inf))[0] for k in names], dtype=float)
    hi = np.array([bounds.get(k, (-np.inf, np.inf))[1] for k in names], dtype=float)
    z = np.random.default_rng(seed).standard_normal((int(n), len(names)))
    draws = np.clip(theta + z @ L.T, lo, hi)
    out = []
    for row in draws:
        p = copy_params(result.brov_params)
        for k, v in zip(names, row):
            set_param(p, k, v)
        out.append(p)
    return out


def _check_recordings(X_list, U_list, model):
    """the lists as fp64 [L_b, nx] / [L_b, nu] arrays, U cut to X's rows; ValueError where they do not pair up"""
    X_list, U_list = list(X_list), list(U_list)
    if len(X_list) != len(U_list):
        raise ValueError(f"{len(X_list)} state recordings but {len(U_list)} input recordings")
    if not X_list:
        raise ValueError("need at least one recording")
    nx, nu = _lib.NX[model], _lib.NU[model]
    X_list = [_lib.as_f64(X).reshape(-1, nx) for X in X_list]
    U_list = [_lib.as_f64(U).reshape(-1, nu) for U in U_list]
    for b, (X, U) in enumerate(zip(X_list, U_list)):
        if U.shape[0] < X.shape[0]:
            raise ValueError(f"recording {b}: U has {U.shape[0]} rows, X has {X.shape[0]}: U must be row-aligned with X")
    return X_list, [U[:X.shape[0]] for X, U in zip(X_list, U_list)]


def stack_recordings(X_list, U_list, model):
    """(X [rows, nx], U [rows, nu], bag_offsets int64 [nbags + 1]) of a list of recordings, stacked on the host"""
    X_list, U_list = _check_recordings(X_list, U_list, model)
    off = np.zeros(len(X_list) + 1, dtype=np.int64)
    np.cumsum([X.shape[0] for X in X_list], out=off[1:])
    return np.concatenate(X_list), np.concatenate(U_list), off


def fit_parameters_multi(rov, X_list, U_list, dt, H=10, evaluator=None, model=None, **kwargs):
    """fit_parameters over several recordings (KoopmanEDMDc.fit_multi's X_list / U_list): recording b is X_list[b] [L_b, nx] with
    U_list[b] [>= L_b, nu] row-aligned.  No window crosses from one recording into the next and every recording starts from zero
    thruster lag.  Recordings of H rows or fewer (empty ones included) contribute no window.  On the device path the list is
    uploaded once, bag by bag (engine.upload_bags); with an `evaluator` the rows are stacked on the host.  The other arguments
    are fit_parameters'."""
    model = getattr(rov, "MODEL", _lib.THRUSTER_EULER) if model is None else model
    X_list, U_list = _check_recordings(X_list, U_list, model)
    if evaluator is None:
        from .. import engine
        ctx = getattr(rov, "_ctx", None) or _lib.default_context()
        X, U, off = engine.upload_bags(X_list, U_list, _lib.NX[model], _lib.NU[model], ctx=ctx)
    else:
        X, U, off = stack_recordings(X_list, U_list, model)
    return fit_parameters(rov, X, U, dt, H=H, evaluator=evaluator, model=model, bag_offsets=off, **kwargs)
