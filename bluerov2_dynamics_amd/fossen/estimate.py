"""State estimation on the Fossen model: the record of the unscented Kalman filter (engine.ukf_filter, VehicleBase.filter_states,
VehicleBase.log_likelihood_population).  include/brov2.h (brov_ukf_filter) is the specification of the law: per row a sequence of
scalar Kalman updates with the measured components of the state (a NaN = not measured), then an unscented prediction through the
vehicle's own step with 2 n + 1 = 25 sigma points.

Nothing here runs on the device; the struct goes to the kernel through engine.ukf_filter."""
import numpy as np

from .. import _lib
from .control import _vec

P0_STAND_IN = 1.0       # default start variance of a component that is never measured (r = +inf): 1 (m, rad, m/s, rad/s) squared


def ukf(q, r, alpha=1.0, beta=2.0, kappa=1.0, n=12):
    """struct brov_ukf (include/brov2.h: brov_ukf_filter) from the per-step process variances q and the measurement variances r
    (scalar or [n]; r = +inf: the component is never measured), and the sigma-point settings alpha, beta, kappa.  n is the state
    size: 12, the Euler models.  ValueError where the library would refuse the record: n != 12, a NaN, a negative q or r, an infinite
    q, alpha not finite or <= 0, n + lambda <= 0 with lambda = alpha^2 (n + kappa) - n.  A small alpha costs digits (alpha = 1e-3:
    a centre weight of -1.2e7); alpha in [0.5, 1] is the tested range."""
    n = int(n)
    if n != 12:
        raise ValueError(f"n must be 12 (the Euler models), got {n}")
    q, r = _vec(q, n, 0.0, "q"), _vec(r, n, 0.0, "r")
    alpha, beta, kappa = float(alpha), float(beta), float(kappa)
    if np.isnan(q).any() or np.isnan(r).any() or np.isnan(beta) or np.isnan(kappa):
        raise ValueError("NaN in the UKF record")
    if np.any(q < 0) or np.any(r < 0):
        raise ValueError("the variances q and r must be >= 0")
    if np.any(np.isinf(q)):
        raise ValueError("q must be finite")
    if not np.isfinite(alpha) or not alpha > 0:
        raise ValueError("alpha must be finite and > 0")
    nl = alpha * alpha * (n + kappa)
    if not nl > 0 or not np.isfinite(nl) or not np.isfinite(beta):
        raise ValueError("n + lambda = alpha^2 (n + kappa) must be finite and > 0, and beta finite")
    cfg = _lib.BrovUkf()
    for i in range(n):
        cfg.q[i], cfg.r[i] = q[i], r[i]
    cfg.alpha, cfg.beta, cfg.kappa = alpha, beta, kappa
    return cfg


def default_start(Y, cfg):
    """(x0 [B,12], P0 [B,12,12]) of filter_states when none is given.  x0: the first row of each recording in Y [B,T,12] in which
    every component with a finite r is present, taken as the guess for row 0 (components that are never measured start at 0;
    ValueError when a recording has no such row).  P0 = diag(4 r), with P0_STAND_IN where r is infinite.  A component with r = 0
    gives a singular P0, which the filter reports as a failure at step 0: give P0 then."""
    Y = np.asarray(Y, dtype=float)
    r = np.array(list(cfg.r), dtype=float)
    need = np.isfinite(r)
    x0 = np.zeros((Y.shape[0], 12))
    for b in range(Y.shape[0]):
        full = np.flatnonzero(~np.isnan(Y[b][:, need]).any(axis=1))
        if full.size == 0:
            raise ValueError(f"recording {b} has no row with every measured component present: give x0")
        x0[b] = np.where(need, Y[b, full[0]], 0.0)
    d = np.where(need, 4.0 * np.where(need, r, 0.0), P0_STAND_IN)
    return x0, np.repeat(np.diag(d)[None], Y.shape[0], axis=0)
