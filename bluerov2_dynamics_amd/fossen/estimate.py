"""State estimation on the Fossen model: the record of the unscented Kalman filter (engine.ukf_filter, VehicleBase.filter_states,
VehicleBase.log_likelihood_population), the EM fit of its q and r (em_update, fit_noise; VehicleBase.fit_noise), and the draw of the
measurement noise that the output-feedback closed loop takes (measurement_noise).  include/brov2.h (brov_ukf_filter) is the specification of the law: per row a sequence of
scalar Kalman updates with the measured components of the state (a NaN = not measured), then an unscented prediction through the
vehicle's own step with 2 n + 1 = 25 sigma points.  The quaternion vehicle has the multiplicative form of the same filter
(engine.ukf_filter_quat; brov_ukf_filter_quat) and its smoother (engine.ukf_smooth_quat, VehicleBase.smooth_states_quat;
brov_ukf_smooth_quat) but no EM fit; quat_boxplus, quat_boxminus and default_start_quat are the chart and the default start of both.

Nothing here runs on the device: the struct goes to the kernel through engine.ukf_filter, and fit_noise sums nothing itself (the
statistics of an EM iteration come from engine.ukf_smooth)."""
import numpy as np

from .. import _lib
from .control import _vec

P0_STAND_IN = 1.0       # default start variance of a component that is never measured (r = +inf): 1 (m, rad, m/s, rad/s) squared


def ukf(q, r, alpha=1.0, beta=2.0, kappa=1.0, n=12):
    """struct brov_ukf (include/brov2.h: brov_ukf_filter) from the per-step process variances q and the measurement variances r
    (scalar or [n]; r = +inf: the component is never measured), and the sigma-point settings alpha, beta, kappa.  n is the state
    size: 12, the Euler models -- and the quaternion model too, whose record lives in its 12-component error state (q[3..5] and
    r[3..5] in the units of quat_boxminus, rad^2 at small angles).  ValueError where the library would refuse the record: n != 12, a NaN, a negative q or r, an infinite
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


# ---- the quaternion model: the chart of the multiplicative filter (include/brov2.h: brov_ukf_filter_quat holds the law) ------------
def _qmul(a, b):
    """Hamilton product over leading dimensions, w first"""
    aw, ax, ay, az = (a[..., i] for i in range(4))
    bw, bx, by, bz = (b[..., i] for i in range(4))
    return np.stack([aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
                     aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw], -1)


def quat_boxplus(X, D):
    """X [+] D of the quaternion model's filter: X [...,13] = (p, q with w first, nu), D [...,12] = (dp, g, dnu) with g twice the
    Gibbs vector of a rotation in the body frame.  Returns (p + dp, q (x) dq(g), nu + dnu) with dq(g) = (1, g / 2) / sqrt(1 +
    |g|^2 / 4).  No branch: negating q negates the result's quaternion; the norm of q is kept."""
    X, D = np.asarray(X), np.asarray(D)
    h = D[..., 3:6] / 2
    dq = np.concatenate([np.ones_like(h[..., :1]), h], -1) / np.sqrt(1 + np.sum(h * h, -1, keepdims=True))
    return np.concatenate([X[..., :3] + D[..., :3], _qmul(X[..., 3:7], dq), X[..., 7:] + D[..., 6:]], -1)


def quat_boxminus(A, B):
    """A [-] B, the inverse of quat_boxplus in its second argument: (p_a - p_b, 2 e_v / e_w, nu_a - nu_b) [...,12] with
    e = conj(q_b) (x) q_a.  Invariant to the sign and the norm of either quaternion; not finite at exactly half a turn (e_w = 0).
    The attitude part is 2 tan(angle / 2) along the axis: the angle in rad when it is small."""
    A, B = np.asarray(A), np.asarray(B)
    qb = B[..., 3:7] * np.array([1.0, -1.0, -1.0, -1.0], dtype=B.dtype)
    e = _qmul(qb, A[..., 3:7])
    with np.errstate(divide="ignore", invalid="ignore"):
        g = 2 * e[..., 1:] / e[..., :1]
    return np.concatenate([A[..., :3] - B[..., :3], g, A[..., 7:] - B[..., 7:]], -1)


def default_start_quat(Y, cfg):
    """(x0 [B,13], P0 [B,12,12]) of the quaternion vehicle's filter_states when none is given.  x0: the first row of each recording
    in Y [B,T,13] in which every component with a finite r is present (r[3..5] stand for the four numbers of the quaternion), taken as
    the guess for row 0 with its quaternion normalised; components that are never measured start at 0, the attitude at the identity.
    ValueError when a recording has no such row, or when that row's quaternion is zero.  P0 = diag(4 r), with P0_STAND_IN where r
    is infinite."""
    Y = np.asarray(Y, dtype=float)
    r = np.array(list(cfg.r), dtype=float)
    need = np.isfinite(r)
    att = bool(need[3:6].any())
    need13 = np.concatenate([need[:3], [att] * 4, need[6:]])
    x0 = np.zeros((Y.shape[0], 13))
    for b in range(Y.shape[0]):
        full = np.flatnonzero(~np.isnan(Y[b][:, need13]).any(axis=1))
        if full.size == 0:
            raise ValueError(f"recording {b} has no row with every measured component present: give x0")
        x0[b] = np.where(need13, Y[b, full[0]], 0.0)
        if att:
            n = np.linalg.norm(x0[b, 3:7])
            if not n > 0:
                raise ValueError(f"recording {b}: the quaternion of its first complete row is zero: give x0")
            x0[b, 3:7] /= n
        else:
            x0[b, 3:7] = (1.0, 0.0, 0.0, 0.0)
    d = np.where(need, 4.0 * np.where(need, r, 0.0), P0_STAND_IN)
    return x0, np.repeat(np.diag(d)[None], Y.shape[0], axis=0)


def measurement_noise(cfg, shape, dropout=0.0, never=(), seed=0):
    """The noise rows V [..., 12] of the output-feedback closed loop (engine.output_feedback, VehicleBase.simulate_output_feedback;
    include/brov2.h: brov_output_feedback): component i is drawn from N(0, cfg.r[i]), seeded; every entry is then dropped (NaN =
    "not measured at this row") with probability `dropout`.  The components in `never` and those with r = +inf are never measured:
    their whole column is NaN.  shape: the leading dimensions, (T,) or (B, T).  Runs on the host: the kernel has no random
    generator of its own.  The draw depends on (seed, shape) alone, not on dropout or never: two calls that differ in those keep the
    same numbers where both measure."""
    shape = (int(shape),) if np.isscalar(shape) else tuple(int(s) for s in shape)
    dropout = float(dropout)
    if not 0.0 <= dropout <= 1.0:
        raise ValueError("dropout must lie in [0, 1]")
    never = [int(i) for i in never]
    if any(i < 0 or i >= 12 for i in never):
        raise ValueError("never: components 0 .. 11")
    r = np.array(list(cfg.r), dtype=float)
    rng = np.random.default_rng(seed)
    V = rng.standard_normal(shape + (12,)) * np.sqrt(np.where(np.isfinite(r), r, 0.0))
    V[rng.random(shape + (12,)) < dropout] = np.nan
    V[..., [i for i in range(12) if i in never or not np.isfinite(r[i])]] = np.nan
    return V


# ---- fitting q and r by expectation-maximisation (include/brov2.h: brov_ukf_rts_em_dev holds the law of the statistics) -------------
def _records(cfgs, P):
    out = [cfgs] * P if isinstance(cfgs, _lib.BrovUkf) else list(cfgs)
    if len(out) == 1 and P > 1:
        out = out * P
    if len(out) != P:
        raise ValueError(f"{len(out)} records for {P} candidates: one or P")
    return out


def em_update(em, info, sinfo, cfgs, fit_q=True, fit_r=True, q_floor=0.0, r_floor=0.0):
    """The M-step of the EM fit of q and r, on the host.  em [P,B,37] = Sq [12] | Sr [12] | nr [12] | nq, info [P,B,4] and sinfo
    [P,B,2] are those of engine.ukf_smooth(..., want=("info", "sinfo", "em")); cfgs is the record (or the P records) that call ran
    under.  Per candidate, pooled over its recordings whose filter (info[2] = -1) and backward pass (sinfo[0] = -1) both completed:
        q_i <- max(sum Sq_i / sum nq, q_floor),     r_i <- max(sum Sr_i / sum nr_i, r_floor) where sum nr_i > 0,
    otherwise r_i stays, so +inf stays +inf.  fit_q / fit_r: a bool or bool[12], the components to update.  q_i = 0 stays 0 (the
    statistic is 0 there: EM cannot leave a zero).  x0 and P0 are not re-estimated.  Returns (the P new records, the number of
    (candidate, recording) problems left out); ValueError when every recording of a candidate failed."""
    em, info, sinfo = np.asarray(em, float), np.asarray(info, float), np.asarray(sinfo, float)
    P = em.shape[0]
    cfgs = _records(cfgs, P)
    fq, fr = np.broadcast_to(np.asarray(fit_q, bool), (12,)), np.broadcast_to(np.asarray(fit_r, bool), (12,))
    out, left = [], 0
    for j in range(P):
        ok = (info[j, :, 2] == -1) & (sinfo[j, :, 0] == -1)
        left += int((~ok).sum())
        if not ok.any():
            raise ValueError(f"every recording of candidate {j} failed: no statistics to fit its noise model from")
        e = em[j][ok]
        q, r = np.array(list(cfgs[j].q)), np.array(list(cfgs[j].r))
        nq, nr = e[:, 36].sum(), e[:, 24:36].sum(axis=0)
        if nq > 0:
            q = np.where(fq, np.maximum(e[:, :12].sum(axis=0) / nq, q_floor), q)
        with np.errstate(invalid="ignore", divide="ignore"):
            r = np.where(fr & (nr > 0), np.maximum(e[:, 12:24].sum(axis=0) / nr, r_floor), r)
        out.append(ukf(q, r, cfgs[j].alpha, cfgs[j].beta, cfgs[j].kappa))
    return out, left


def fit_noise(model, integrator, params_list, cfg, x0, P0, U, Y, dt, iters=20, tol=1e-4, fit_q=True, fit_r=True, q_floor=0.0, r_floor=0.0,
              lag=None, lag_mode=0, tape_bytes=0, ctx=None):
    """EM fit of the filter's q and r to recordings, one noise model per candidate of params_list, all candidates in the same
    launches.  cfg: the start, one record or P; x0 [B,12], P0 [B,12,12], U [B,T,nu], Y [B,T,12] as engine.ukf_smooth takes them
    (host arrays; they are uploaded once).  An iteration is one engine.ukf_smooth(want=("info", "sinfo", "em")), which stores no
    rows, and em_update on the host.  The loop stops after `iters` updates, or before an update when the rise of the summed
    log-likelihood over the last update is below tol times its magnitude; an update that lowered it (the E-step is approximate, so
    EM's monotonicity is not guaranteed) is taken back.  ValueError when every recording of a candidate failed.
    Returns dict(cfg: the P fitted records, q, r [P,12], loglik [its + 1, P] the log-likelihood of each candidate summed over its
    completed recordings, row k under the noise model after k updates, q_hist, r_hist [its + 1, P, 12], n_excluded: the
    (candidate, recording) problems left out of the last update, converged)."""
    from .. import engine
    P = len(params_list)
    cfgs = _records(cfg, P)
    ctx = ctx or engine.default_context()
    D = engine.DevArray.from_host
    dev = [D(ctx, np.asarray(v, float)) for v in (x0, P0, U, Y)]
    lag_d = None if lag is None else D(ctx, np.asarray(lag, float))
    hist = lambda: (np.array([list(c.q) for c in cfgs]), np.array([list(c.r) for c in cfgs]))

    def loglik(info, sinfo=None):
        ok = info[:, :, 2] == -1
        if sinfo is not None:
            ok &= sinfo[:, :, 0] == -1
        return np.where(ok, info[:, :, 0], 0.0).sum(axis=1)
    ll, qh, rh, left, converged = [], [], [], 0, False
    for it in range(int(iters) + 1):
        q, r = hist()
        qh.append(q)
        rh.append(r)
        if it == iters:
            o = engine.ukf_filter(model, integrator, list(params_list), cfgs, *dev, dt, lag=lag_d, lag_mode=lag_mode, want=("info",), ctx=ctx)
            ll.append(loglik(o["info"].numpy()))
            break
        o = engine.ukf_smooth(model, integrator, list(params_list), cfgs, *dev, dt, lag=lag_d, lag_mode=lag_mode, want=("info", "sinfo", "em"),
                              tape_bytes=tape_bytes, ctx=ctx)
        info, sinfo = o["info"].numpy(), o["sinfo"].numpy()
        ll.append(loglik(info, sinfo))
        if it >= 1 and ll[-1].sum() - ll[-2].sum() < tol * abs(ll[-2].sum()):
            converged = True
            if ll[-1].sum() < ll[-2].sum():      # the E-step is approximate: an update may lose likelihood; then the one before stands
                cfgs = before
                del ll[-1], qh[-1], rh[-1]
            break
        before = cfgs
        cfgs, left = em_update(o["em"].numpy(), info, sinfo, cfgs, fit_q, fit_r, q_floor, r_floor)
    return dict(cfg=cfgs, q=qh[-1], r=rh[-1], loglik=np.array(ll), q_hist=np.array(qh), r_hist=np.array(rh), n_excluded=left, converged=converged)
