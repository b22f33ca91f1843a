"""NumPy restatement of the unscented Kalman filter of include/brov2.h (brov_ukf_filter) around the parameterised oracle
(oracle.fossen_params._Prep / _step).  Dtype-generic (np.float64 / np.longdouble); not collected by pytest, shares no code with the
product.  Plain loops: the law is short and the test shapes are small.

filter() returns the outputs of the entry point plus, per (candidate, recording):
  wrap_margin  the smallest distance from pi of |innovation or deviation before wrapping| mod 2 pi (attitude components): a value
               near 0 means that rounding could send a wrap the other way, and the comparison would be ill-posed
  pivot_min    the smallest Cholesky pivot L[j][j] seen (info[3] of the entry point)
  shifted      how many attitude innovations the wrap moved by a multiple of 2 pi
"""
import dataclasses

import numpy as np

from oracle import fossen_params as fp

N = 12


@dataclasses.dataclass(frozen=True, eq=False)
class Cfg:
    q: np.ndarray
    r: np.ndarray
    alpha: float = 1.0
    beta: float = 2.0
    kappa: float = 1.0


def cfg(q, r, alpha=1.0, beta=2.0, kappa=1.0):
    return Cfg(np.broadcast_to(np.asarray(q, float), (N,)).copy(), np.broadcast_to(np.asarray(r, float), (N,)).copy(),
               float(alpha), float(beta), float(kappa))


def to_struct(c):
    from bluerov2_dynamics_amd import _lib
    s = _lib.BrovUkf()
    for i in range(N):
        s.q[i], s.r[i] = c.q[i], c.r[i]
    s.alpha, s.beta, s.kappa = c.alpha, c.beta, c.kappa
    return s


def _pi(dtype):
    return np.arccos(dtype(-1))


def weights(c, dtype):
    """(c, Wc0, Wi) of the law"""
    a, n = dtype(c.alpha), dtype(N)
    lam = a * a * (n + dtype(c.kappa)) - n
    wm0 = lam / (n + lam)
    return np.sqrt(n + lam), wm0 + dtype(1) - a * a + dtype(c.beta), dtype(1) / (dtype(2) * (n + lam))


def _wrap(d, dtype):
    """(d - 2 pi rint(d / 2 pi), distance of |d| mod 2 pi from pi)"""
    two_pi = dtype(2) * _pi(dtype)
    return d - two_pi * np.rint(d / two_pi), np.abs(np.mod(np.abs(d), two_pi) - _pi(dtype))


def cholesky(Pm, dtype):
    """(L, failed, pivots): lower factor by rows of columns, stopping at a pivot argument that is <= 0 or not finite"""
    L = np.zeros((N, N), dtype=dtype)
    piv = []
    for j in range(N):
        s = Pm[j, j]
        for k in range(j):
            s = s - L[j, k] * L[j, k]
        if not (s > 0) or not np.isfinite(s):
            return L, True, piv
        L[j, j] = np.sqrt(s)
        piv.append(L[j, j])
        for i in range(j + 1, N):
            s = Pm[i, j]
            for k in range(j):
                s = s - L[i, k] * L[j, k]
            L[i, j] = s / L[j, j]
    return L, False, piv


def update_row(x, Pm, y, r, dtype):
    """stage 1 of the law on one row.  Returns (x, P, innov [12], dl, n_applied, margin, shifted, failed)"""
    innov = np.full(N, np.nan, dtype=dtype)
    two_pi = dtype(2) * _pi(dtype)
    dl, napp, margin, shifted = dtype(0), 0, np.inf, 0
    for i in range(N):
        if np.isnan(y[i]) or np.isposinf(r[i]):
            continue
        v = y[i] - x[i]
        if 3 <= i < 6:
            w, mg = _wrap(v, dtype)
            margin = min(margin, float(mg))
            shifted += int(abs(w - v) > 1)
            v = w
        s = Pm[i, i] + r[i]
        if not (s > 0) or not np.isfinite(s):
            return x, Pm, innov, dl, napp, margin, shifted, True
        k = Pm[:, i] / s
        x = x + k * v
        Pm = Pm - np.outer(k, k) * s
        dl = dl - (np.log(two_pi * s) + v * v / s) / dtype(2)
        innov[i] = v / np.sqrt(s)
        napp += 1
    return x, Pm, innov, dl, napp, margin, shifted, False


def predict(c, model, integ, lag_mode, dt, x, Pm, u, lag, w, q, dtype):
    """stage 2 of the law.  Returns (x, P, lag, pivots, margin, failed)"""
    cw, wc0, wi = w
    L, bad, piv = cholesky(Pm, dtype)
    if bad:
        return x, Pm, lag, piv, np.inf, True
    chi = np.stack([x] + [x + cw * L[:, i] for i in range(N)] + [x - cw * L[:, i] for i in range(N)])
    ns = chi.shape[0]
    Xn, lagn = fp._step(c, model, integ, lag_mode, dt, chi, np.tile(u[None], (ns, 1)), np.tile(lag[None], (ns, 1, 1)))
    d = Xn - Xn[0]
    wr, mg = _wrap(d[:, 3:6], dtype)
    margin = float(np.min(mg[1:])) if np.all(np.isfinite(mg)) else 0.0
    d = d.copy()
    d[:, 3:6] = wr
    m = np.zeros(N, dtype=dtype)
    for i in range(1, ns):
        m = m + wi * d[i]
    xn = Xn[0] + m
    if not np.all(np.isfinite(xn)):
        return xn, Pm, lagn[0], piv, margin, True
    Pn = wc0 * np.outer(m, m)
    for i in range(1, ns):
        e = d[i] - m
        Pn = Pn + wi * np.outer(e, e)
    Pn = Pn + np.diag(q)
    return xn, Pn, lagn[0], piv, margin, False


def filter_one(c, model, integ, lag_mode, dt, k, x0, P0, U, Y, lag, dtype):
    """one candidate (prepared vehicle c), one recording"""
    T = U.shape[0]
    w = weights(k, dtype)
    q, r = np.asarray(k.q, dtype=dtype), np.asarray(k.r, dtype=dtype)
    x = np.asarray(x0, dtype=dtype).copy()
    Pm = np.tril(np.asarray(P0, dtype=dtype))
    Pm = Pm + np.tril(Pm, -1).T
    lag0 = lag
    xf, pstd, innov = (np.full((T, N), np.nan, dtype=dtype) for _ in range(3))
    ell, nupd, failed, pivmin, margin, shifted = dtype(0), 0, -1, np.inf, np.inf, 0
    for t in range(T):
        x, Pm, inn, dl, napp, mg, sh, bad = update_row(x, Pm, Y[t], r, dtype)
        nupd, margin, shifted = nupd + napp, min(margin, mg), shifted + sh
        ell = ell + dl
        if bad:
            failed = t
            break
        xf[t], innov[t] = x, inn
        with np.errstate(invalid="ignore"):
            pstd[t] = np.sqrt(np.diagonal(Pm))
        x, Pm, lag, piv, mg, bad = predict(c, model, integ, lag_mode, dt, x, Pm, U[t], lag, w, q, dtype)
        pivmin = min([pivmin] + [float(v) for v in piv])
        margin = min(margin, mg)
        if bad:
            failed = t
            break
    if failed >= 0:
        x, Pm, ell, lag = np.full(N, np.nan, dtype=dtype), np.full((N, N), np.nan, dtype=dtype), dtype(-np.inf), lag0
    return dict(xf=xf, pstd=pstd, innov=innov, xT=x, PT=Pm, info=np.array([ell, nupd, failed, pivmin], dtype=dtype), lag=lag,
                wrap_margin=margin, pivot_min=pivmin, shifted=shifted)


def filter(model, integ, lag_mode, vehicles, cfgs, x0, P0, U, Y, dt, lag=None, dtype=np.float64):
    """brov_ukf_filter: vehicles [P] (oracle Vehicles), cfgs one Cfg or [P]; x0 [B,12], P0 [B,12,12], U [B,T,nu], Y [B,T,12];
    lag [P,B,8,3] or None.  Returns dict(xf, pstd, innov [P,B,T,12], xT [P,B,12], PT [P,B,12,12], info [P,B,4], lag [P,B,8,3],
    wrap_margin, pivot_min, shifted [P,B])."""
    assert model in (fp.THRUSTER_EULER, fp.WRENCH_EULER)
    cfgs = [cfgs] * len(vehicles) if isinstance(cfgs, Cfg) else list(cfgs)
    U, Y = np.asarray(U, dtype=dtype), np.asarray(Y, dtype=dtype)
    P, B = len(vehicles), U.shape[0]
    keys = ("xf", "pstd", "innov", "xT", "PT", "info", "lag", "wrap_margin", "pivot_min", "shifted")
    out = {k: [] for k in keys}
    for j, v in enumerate(vehicles):
        c = fp._Prep(v, dt, dtype)
        rows = []
        for b in range(B):
            l0 = np.zeros((8, 3), dtype=dtype) if lag is None else np.asarray(lag, dtype=dtype).reshape(P, B, 8, 3)[j, b]
            rows.append(filter_one(c, model, integ, lag_mode, dt, cfgs[j], x0[b], P0[b], U[b], Y[b], l0, dtype))
        for k in keys:
            out[k].append(np.stack([np.asarray(r[k]) for r in rows]))
    return {k: np.stack(v) for k, v in out.items()}
