"""NumPy restatement of the unscented Rauch-Tung-Striebel smoother of include/brov2.h (brov_ukf_filter_tape_dev, brov_ukf_rts_dev,
brov_ukf_smooth) on top of tests/ukf_ref.py, whose scalar updates, Cholesky factorisation and oracle step it uses.  Dtype-generic
(np.float64 / np.longdouble); not collected by pytest, shares no code with the product.  Plain loops: the law is short and the test
shapes are small.

smooth() returns, stacked over [P, B]: the filter's outputs (xf, pstd, innov, xT, PT, info, lag), the tape [T, 312] and nrows, the
smoother's xs, pstd_s [T, 12], Ps [T, 12, 12], Ps0, sinfo [2], the margins of ukf_ref (wrap_margin, pivot_min, shifted), Pf
[T, 12, 12] (the tape's first block, unpacked) and c_form, the largest relative difference between the compact form of C that the
tape holds and the textbook sum over the sigma points."""
import numpy as np

import ukf_ref as ur
from oracle import fossen_params as fp

N = ur.N
TAPE = 312
PF, XP, PP, CC = slice(0, 78), slice(78, 90), slice(90, 168), slice(168, 312)
TRIL = np.tril_indices(N)              # row by row: entry e = a (a + 1) / 2 + b


def pack(Pm):
    return Pm[TRIL]


def unpack(v, dtype):
    Pm = np.zeros((N, N), dtype=dtype)
    Pm[TRIL] = v
    return Pm + np.tril(Pm, -1).T


def predict_tape(c, model, integ, lag_mode, dt, x, Pm, u, lag, w, q, dtype):
    """stage 2 of the filter's law with the cross covariance.  Returns (x, P, lag, pivots, margin, failed, C, C_textbook)"""
    cw, wc0, wi = w
    L, bad, piv = ur.cholesky(Pm, dtype)
    if bad:
        return x, Pm, lag, piv, np.inf, True, None, None
    chi = np.stack([x] + [x + cw * L[:, i] for i in range(N)] + [x - cw * L[:, i] for i in range(N)])
    ns = chi.shape[0]
    Xn, lagn = fp._step(c, model, integ, lag_mode, dt, chi, np.tile(u[None], (ns, 1)), np.tile(lag[None], (ns, 1, 1)))
    d = Xn - Xn[0]
    wr, mg = ur._wrap(d[:, 3:6], dtype)
    margin = float(np.min(mg[1:])) if np.all(np.isfinite(mg)) else 0.0
    d = d.copy()
    d[:, 3:6] = wr
    m = np.zeros(N, dtype=dtype)
    for i in range(1, ns):
        m = m + wi * d[i]
    xn = Xn[0] + m
    if not np.all(np.isfinite(xn)):
        return xn, Pm, lagn[0], piv, margin, True, None, None
    Pn = wc0 * np.outer(m, m)
    for i in range(1, ns):
        e = d[i] - m
        Pn = Pn + wi * np.outer(e, e)
    Pn = Pn + np.diag(q)
    g = cw * wi
    C = np.zeros((N, N), dtype=dtype)
    for j in range(N):
        C = C + np.outer(L[:, j], g * (d[j + 1] - d[j + 1 + N]))
    Ct = np.zeros((N, N), dtype=dtype)
    for i in range(1, ns):
        Ct = Ct + wi * np.outer(chi[i] - x, d[i] - m)
    return xn, Pn, lagn[0], piv, margin, False, C, Ct


def forward_one(c, model, integ, lag_mode, dt, k, x0, P0, U, Y, lag, dtype):
    """ukf_ref.filter_one with the tape"""
    T = U.shape[0]
    w = ur.weights(k, dtype)
    q, r = np.asarray(k.q, dtype=dtype), np.asarray(k.r, dtype=dtype)
    x = np.asarray(x0, dtype=dtype).copy()
    Pm = np.tril(np.asarray(P0, dtype=dtype))
    Pm = Pm + np.tril(Pm, -1).T
    lag0 = lag
    xf, pstd, innov = (np.full((T, N), np.nan, dtype=dtype) for _ in range(3))
    tape = np.full((T, TAPE), np.nan, dtype=dtype)
    ell, nupd, failed, pivmin, margin, shifted, n, c_form = dtype(0), 0, -1, np.inf, np.inf, 0, T, 0.0
    for t in range(T):
        x, Pm, inn, dl, napp, mg, sh, bad = ur.update_row(x, Pm, Y[t], r, dtype)
        nupd, margin, shifted = nupd + napp, min(margin, mg), shifted + sh
        ell = ell + dl
        if bad:
            failed, n = t, t
            break
        xf[t], innov[t] = x, inn
        with np.errstate(invalid="ignore"):
            pstd[t] = np.sqrt(np.diagonal(Pm))
        tape[t, PF] = pack(Pm)
        x, Pm, lag, piv, mg, bad, C, Ct = predict_tape(c, model, integ, lag_mode, dt, x, Pm, U[t], lag, w, q, dtype)
        pivmin = min([pivmin] + [float(v) for v in piv])
        margin = min(margin, mg)
        if bad:
            failed, n = t, t + 1
            break
        tape[t, XP], tape[t, PP], tape[t, CC] = x, pack(Pm), C.reshape(-1)
        c_form = max(c_form, float(np.max(np.abs(C - Ct)) / np.max(np.abs(Ct))))
    if failed >= 0:
        x, Pm, ell, lag = np.full(N, np.nan, dtype=dtype), np.full((N, N), np.nan, dtype=dtype), dtype(-np.inf), lag0
    return dict(xf=xf, pstd=pstd, innov=innov, xT=x, PT=Pm, info=np.array([ell, nupd, failed, pivmin], dtype=dtype), lag=lag,
                wrap_margin=margin, pivot_min=pivmin, shifted=shifted, tape=tape, nrows=dtype(n), c_form=c_form)


def gain(C, L, dtype):
    """G = C (L L^T)^-1 by two triangular solves per row of C"""
    W = np.zeros((N, N), dtype=dtype)
    for j in range(N):
        W[:, j] = (C[:, j] - W[:, :j] @ L[j, :j]) / L[j, j]
    G = np.zeros((N, N), dtype=dtype)
    for j in range(N - 1, -1, -1):
        G[:, j] = (W[:, j] - G[:, j + 1:] @ L[j + 1:, j]) / L[j, j]
    return G


def rts_one(xf, tape, n, dtype, terminal=None):
    """the backward pass of one problem.  Returns dict(xs, pstd_s, Ps, Ps0, sinfo, Pf, rts_pivot_min)"""
    T = xf.shape[0]
    xf, tape = np.asarray(xf, dtype=dtype), np.asarray(tape, dtype=dtype)
    xs = np.full((T, N), np.nan, dtype=dtype)
    Ps = np.full((T, N, N), np.nan, dtype=dtype)
    Pf = np.stack([unpack(tape[t, PF], dtype) for t in range(T)])
    nan2 = np.full((N, N), np.nan, dtype=dtype)
    n = float(n)
    n = 0 if np.isnan(n) else int(min(max(n, 0.0), float(T)))       # the clamp of the header: the fraction dropped, NaN counts as 0, +inf as T
    if n == 0:
        return dict(xs=xs, pstd_s=xs.copy(), Ps=Ps, Ps0=nan2, sinfo=np.full(2, np.nan, dtype=dtype), Pf=Pf, rts_pivot_min=np.inf)
    if terminal is not None and n == T:
        x = np.asarray(terminal[0], dtype=dtype)
        Pm = np.tril(np.asarray(terminal[1], dtype=dtype))
        Pm = Pm + np.tril(Pm, -1).T
        first = T - 1
    else:
        x, Pm = xf[n - 1], Pf[n - 1]
        xs[n - 1], Ps[n - 1] = x, Pm
        first = n - 2
    failed, pivmin = -1, np.inf
    for t in range(first, -1, -1):
        xp, Pp, C = tape[t, XP], unpack(tape[t, PP], dtype), tape[t, CC].reshape(N, N)
        L, bad, piv = ur.cholesky(Pp, dtype)
        pivmin = min([pivmin] + [float(v) for v in piv])
        if bad:
            failed = t
            break
        G = gain(C, L, dtype)
        x = xf[t] + G @ (x - xp)                       # not wrapped: the filter's continuous attitude branch
        Pm = np.tril(Pf[t] + G @ (Pm - Pp) @ G.T)     # one expression serves both triangles
        Pm = Pm + np.tril(Pm, -1).T
        xs[t], Ps[t] = x, Pm
    if failed >= 0:
        xs[:failed + 1], Ps[:failed + 1] = np.nan, np.nan
    with np.errstate(invalid="ignore"):
        pstd_s = np.sqrt(np.diagonal(Ps, axis1=-2, axis2=-1))
    return dict(xs=xs, pstd_s=pstd_s, Ps=Ps, Ps0=Ps[0].copy() if failed < 0 else nan2, sinfo=np.array([failed, pivmin], dtype=dtype), Pf=Pf,
                rts_pivot_min=pivmin)


def smooth(model, integ, lag_mode, vehicles, cfgs, x0, P0, U, Y, dt, lag=None, dtype=np.float64, terminal=None):
    """brov_ukf_smooth, with an optional terminal pair (xs_T [P,B,12], Ps_T [P,B,12,12]) for the backward pass.  Arguments as
    ukf_ref.filter; x0 [B,12] / P0 [B,12,12] shared by the candidates, or [P,B,..] per candidate (a span resumed from xT, PT)."""
    assert model in (fp.THRUSTER_EULER, fp.WRENCH_EULER)
    cfgs = [cfgs] * len(vehicles) if isinstance(cfgs, ur.Cfg) else list(cfgs)
    U, Y = np.asarray(U, dtype=dtype), np.asarray(Y, dtype=dtype)
    P, B = len(vehicles), U.shape[0]
    x0, P0 = np.asarray(x0), np.asarray(P0)
    per_cand = x0.ndim == 3
    out = {}
    for j, v in enumerate(vehicles):
        c = fp._Prep(v, dt, dtype)
        rows = []
        for b in range(B):
            l0 = np.zeros((8, 3), dtype=dtype) if lag is None else np.asarray(lag, dtype=dtype).reshape(P, B, 8, 3)[j, b]
            f = forward_one(c, model, integ, lag_mode, dt, cfgs[j], x0[j, b] if per_cand else x0[b], P0[j, b] if per_cand else P0[b], U[b], Y[b],
                            l0, dtype)
            f.update(rts_one(f["xf"], f["tape"], f["nrows"], dtype, None if terminal is None else (terminal[0][j, b], terminal[1][j, b])))
            rows.append(f)
        for k in rows[0]:
            out.setdefault(k, []).append(np.stack([np.asarray(r[k]) for r in rows]))
    return {k: np.stack(v) for k, v in out.items()}
