"""NumPy restatement of the multiplicative unscented Kalman filter of include/brov2.h (brov_ukf_filter_quat) around the parameterised
oracle (oracle.fossen_params._Prep / _step with WRENCH_QUAT).  Dtype-generic (np.float64 / np.longdouble); not collected by pytest,
shares no code with the product.  Plain loops: the law is short and the test shapes are small.  cholesky, weights and the record
(Cfg, cfg, to_struct) are those of tests/ukf_ref.py: the record is the same struct.

filter() returns the outputs of the entry point plus, per (candidate, recording):
  ew_min     the smallest |e_w| / (|q_a| |q_b|) over every [-] taken (innovations and propagated points): 1 at no rotation, 0 at half
             a turn, where the chart leaves the finite numbers and a comparison would be ill-posed
  pivot_min  the smallest Cholesky pivot L[j][j] seen (info[3] of the entry point)

variant: None is the law.  The other values are its neighbours, each one edit away, which tests/test_ukf_quat_cpu.py uses to show
that the test cases can tell them from the law: "plus_left" (the deviation applied on the left, dq (x) q), "minus_left" (e = q_a (x)
conj(q_b)), "no_d" (v = z[i] without - d[i]), "no_mean" (x = chi_0' without [+] m), "no_wc0" (no Wc_0 m m^T term)."""
import numpy as np

import ukf_ref as ur
from oracle import fossen_params as fp

N, NX = 12, 13
VARIANTS = ("plus_left", "minus_left", "no_d", "no_mean", "no_wc0")


def qmul(a, b):
    """Hamilton product, w first"""
    return np.array([a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3], a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2],
                     a[0] * b[2] - a[1] * b[3] + a[2] * b[0] + a[3] * b[1], a[0] * b[3] + a[1] * b[2] - a[2] * b[1] + a[3] * b[0]])


def conj(q):
    return np.array([q[0], -q[1], -q[2], -q[3]])


def boxplus(x, d, variant=None):
    """x [+] d: (p + dp, q (x) dq(g), nu + dnu), dq(g) = (1, g / 2) / sqrt(1 + |g|^2 / 4)"""
    dtype = x.dtype.type
    h = d[3:6] / dtype(2)
    dq = np.concatenate([[dtype(1)], h]) / np.sqrt(dtype(1) + h[0] * h[0] + h[1] * h[1] + h[2] * h[2])
    q = qmul(dq, x[3:7]) if variant == "plus_left" else qmul(x[3:7], dq)
    return np.concatenate([x[:3] + d[:3], q, x[7:] + d[6:]])


def att_minus(qa, qb, variant=None):
    """(2 e_v / e_w, |e_w| / (|q_a| |q_b|)) with e = conj(q_b) (x) q_a"""
    dtype = qa.dtype.type
    e = qmul(qa, conj(qb)) if variant == "minus_left" else qmul(conj(qb), qa)
    with np.errstate(all="ignore"):
        g = dtype(2) * e[1:] / e[0]
        ew = np.abs(e[0]) / (np.sqrt(np.sum(qa * qa)) * np.sqrt(np.sum(qb * qb)))
    return g, (float(ew) if np.isfinite(ew) else 0.0)


def boxminus(a, b, variant=None):
    """(a [-] b [12], the normalised |e_w|)"""
    g, ew = att_minus(a[3:7], b[3:7], variant)
    return np.concatenate([a[:3] - b[:3], g, a[7:] - b[7:]]), ew


def update_row(x, Pm, y, r, dtype, variant=None):
    """stage 1 of the law on one row.  Returns (x, P, innov [12], dl, n_applied, ew, failed)"""
    innov = np.full(N, np.nan, dtype=dtype)
    two_pi = dtype(2) * np.arccos(dtype(-1))
    z = np.full(N, np.nan, dtype=dtype)
    z[:3] = y[:3] - x[:3]
    z[6:] = y[7:] - x[7:]
    ew = np.inf
    if not np.isnan(y[3:7]).any():
        z[3:6], ew = att_minus(y[3:7], x[3:7], variant)
        if not np.all(np.isfinite(z[3:6])):
            return x, Pm, innov, dtype(0), 0, ew, True
    d = np.zeros(N, dtype=dtype)
    dl, napp = dtype(0), 0
    for i in range(N):
        if np.isnan(z[i]) or np.isposinf(r[i]):
            continue
        v = z[i] if variant == "no_d" else z[i] - d[i]
        s = Pm[i, i] + r[i]
        if not (s > 0) or not np.isfinite(s):
            return x, Pm, innov, dl, napp, ew, True
        k = Pm[:, i] / s
        d = d + k * v
        Pm = Pm - np.outer(k, k) * s
        dl = dl - (np.log(two_pi * s) + v * v / s) / dtype(2)
        innov[i] = v / np.sqrt(s)
        napp += 1
    return boxplus(x, d, variant), Pm, innov, dl, napp, ew, False


def predict(c, integ, dt, x, Pm, u, w, q, dtype, variant=None):
    """stage 2 of the law.  Returns (x, P, pivots, ew, failed)"""
    cw, wc0, wi = w
    L, bad, piv = ur.cholesky(Pm, dtype)
    if bad:
        return x, Pm, piv, np.inf, True
    chi = np.stack([x] + [boxplus(x, cw * L[:, i], variant) for i in range(N)] + [boxplus(x, -cw * L[:, i], variant) for i in range(N)])
    ns = chi.shape[0]
    with np.errstate(all="ignore"):
        Xn, _ = fp._step(c, fp.WRENCH_QUAT, integ, 0, dt, chi, np.tile(u[None], (ns, 1)), np.zeros((ns, 8, 3), dtype=dtype))
        pairs = [boxminus(Xn[i], Xn[0], variant) for i in range(ns)]
    d = np.stack([p[0] for p in pairs])
    ew = min(p[1] for p in pairs[1:])
    m = np.zeros(N, dtype=dtype)
    with np.errstate(all="ignore"):
        for i in range(1, ns):
            m = m + wi * d[i]
        xn = Xn[0] if variant == "no_mean" else boxplus(Xn[0], m, variant)
    if not np.all(np.isfinite(m)) or not np.all(np.isfinite(xn)):
        return xn, Pm, piv, ew, True
    Pn = np.zeros((N, N), dtype=dtype) if variant == "no_wc0" else wc0 * np.outer(m, m)
    for i in range(1, ns):
        e = d[i] - m
        Pn = Pn + wi * np.outer(e, e)
    Pn = Pn + np.diag(q)
    return xn, Pn, piv, ew, False


def filter_one(c, integ, dt, k, x0, P0, U, Y, dtype, variant=None):
    """one candidate (prepared vehicle c), one recording"""
    T = U.shape[0]
    w = ur.weights(k, dtype)
    q, r = np.asarray(k.q, dtype=dtype), np.asarray(k.r, dtype=dtype)
    x = np.asarray(x0, dtype=dtype).copy()
    Pm = np.tril(np.asarray(P0, dtype=dtype))
    Pm = Pm + np.tril(Pm, -1).T
    xf = np.full((T, NX), np.nan, dtype=dtype)
    pstd, innov = (np.full((T, N), np.nan, dtype=dtype) for _ in range(2))
    ell, nupd, failed, pivmin, ewmin = dtype(0), 0, -1, np.inf, np.inf
    for t in range(T):
        x, Pm, inn, dl, napp, ew, bad = update_row(x, Pm, Y[t], r, dtype, variant)
        nupd, ewmin = nupd + napp, min(ewmin, ew)
        ell = ell + dl
        if bad:
            failed = t
            break
        xf[t], innov[t] = x, inn
        with np.errstate(invalid="ignore"):
            pstd[t] = np.sqrt(np.diagonal(Pm))
        x, Pm, piv, ew, bad = predict(c, integ, dt, x, Pm, U[t], w, q, dtype, variant)
        pivmin = min([pivmin] + [float(v) for v in piv])
        ewmin = min(ewmin, ew)
        if bad:
            failed = t
            break
    if failed >= 0:
        x, Pm, ell = np.full(NX, np.nan, dtype=dtype), np.full((N, N), np.nan, dtype=dtype), dtype(-np.inf)
    return dict(xf=xf, pstd=pstd, innov=innov, xT=x, PT=Pm, info=np.array([ell, nupd, failed, pivmin], dtype=dtype), ew_min=ewmin,
                pivot_min=pivmin)


def filter(integ, vehicles, cfgs, x0, P0, U, Y, dt, dtype=np.float64, variant=None):
    """brov_ukf_filter_quat: vehicles [P] (oracle Vehicles), cfgs one ukf_ref.Cfg or [P]; x0 [B,13], P0 [B,12,12], U [B,T,6], Y [B,T,13].
    Returns dict(xf [P,B,T,13], pstd, innov [P,B,T,12], xT [P,B,13], PT [P,B,12,12], info [P,B,4], ew_min, pivot_min [P,B])."""
    assert variant is None or variant in VARIANTS
    cfgs = [cfgs] * len(vehicles) if isinstance(cfgs, ur.Cfg) else list(cfgs)
    U, Y = np.asarray(U, dtype=dtype), np.asarray(Y, dtype=dtype)
    B = U.shape[0]
    keys = ("xf", "pstd", "innov", "xT", "PT", "info", "ew_min", "pivot_min")
    out = {k: [] for k in keys}
    for j, v in enumerate(vehicles):
        c = fp._Prep(v, dt, dtype)
        rows = [filter_one(c, integ, dt, cfgs[j], x0[b], P0[b], U[b], Y[b], dtype, variant) for b in range(B)]
        for k in keys:
            out[k].append(np.stack([np.asarray(r[k]) for r in rows]))
    return {k: np.stack(v) for k, v in out.items()}
