"""NumPy restatement of the smoother of the quaternion model of include/brov2.h (brov_ukf_filter_tape_quat_dev, brov_ukf_rts_quat_dev,
brov_ukf_smooth_quat) around tests/ukf_quat_ref.py, whose update_row, chart (boxplus, boxminus) and oracle step it uses, with the
Cholesky factorisation and the gain of tests/ukf_ref.py / tests/ukf_smooth_ref.py.  Dtype-generic (np.float64 / np.longdouble); not
collected by pytest, shares no code with the product.  Plain loops: the law is short and the test shapes are small.

smooth() returns, stacked over [P, B]: the filter's outputs (xf [T,13], pstd, innov, xT [13], PT, info), the tape [T, 313] and nrows,
the smoother's xs [T,13], pstd_s [T,12], Ps [T,12,12], Ps0, sinfo [2], and the margins
  f_ew_min, f_pivot_min   those of ukf_quat_ref.filter (every [-] and every pivot of the forward pass)
  ew_min                  the smallest |e_w| / (|q_a| |q_b|) over the deltas xs_{t+1} [-] xp_{t+1} of the backward pass (+inf: none)
  pivot_min               the smallest pivot over the factorisations of Pp in the backward pass (sinfo[1])
  c_form                  the largest relative difference between the compact form of C that the tape holds and the sum over the
                          sigma points with chi_i [-] x formed through the chart

variant: None is the law.  The others are its neighbours in the backward pass, each one edit away, which
tests/test_ukf_quat_smooth_cpu.py uses to show that the test cases can tell them from the law: "minus_left" (delta through e = q_a (x)
conj(q_b)), "dx_linear" (the attitude part of delta as the difference of the quaternions' vector parts), "plus_left" (xs_t = xf_t [+]
G delta applied on the left), "C_T" (C transposed), "no_Pp" (Ps_{t+1} - Pf_{t+1} in place of Ps_{t+1} - Pp_{t+1}), "dx_from_xf" (delta
against xf_{t+1} in place of xp_{t+1}).  The forward pass is the law under every variant."""
import functools

import numpy as np

import fossen_vehicles as fv
import ukf_quat_cases as qc
import ukf_quat_ref as uq
import ukf_ref as ur
import ukf_smooth_ref as usr
from oracle import fossen_params as fp

N, NX = uq.N, uq.NX
TAPE = 313
PF, XP, PP, CC = slice(0, 78), slice(78, 91), slice(91, 169), slice(169, 313)
VARIANTS = ("minus_left", "dx_linear", "plus_left", "C_T", "no_Pp", "dx_from_xf")
pack, unpack, gain = usr.pack, usr.unpack, usr.gain


def predict_tape(c, integ, dt, x, Pm, u, w, q, dtype):
    """stage 2 of ukf_quat_ref.predict with the cross covariance.  Returns (x, P, pivots, ew, failed, C, C_chart)"""
    cw, wc0, wi = w
    L, bad, piv = ur.cholesky(Pm, dtype)
    if bad:
        return x, Pm, piv, np.inf, True, None, None
    chi = np.stack([x] + [uq.boxplus(x, cw * L[:, i]) for i in range(N)] + [uq.boxplus(x, -cw * L[:, i]) for i in range(N)])
    ns = chi.shape[0]
    with np.errstate(all="ignore"):
        Xn, _ = fp._step(c, fp.WRENCH_QUAT, integ, 0, dt, chi, np.tile(u[None], (ns, 1)), np.zeros((ns, 8, 3), dtype=dtype))
        pairs = [uq.boxminus(Xn[i], Xn[0]) for i in range(ns)]
    d = np.stack([p[0] for p in pairs])
    ew = min(p[1] for p in pairs[1:])
    m = np.zeros(N, dtype=dtype)
    with np.errstate(all="ignore"):
        for i in range(1, ns):
            m = m + wi * d[i]
        xn = uq.boxplus(Xn[0], m)
    if not np.all(np.isfinite(m)) or not np.all(np.isfinite(xn)):
        return xn, Pm, piv, ew, True, None, None
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
        Ct = Ct + wi * np.outer(uq.boxminus(chi[i], x)[0], d[i] - m)
    return xn, Pn, piv, ew, False, C, Ct


def forward_one(c, integ, dt, k, x0, P0, U, Y, dtype):
    """ukf_quat_ref.filter_one with the tape"""
    T = U.shape[0]
    w = ur.weights(k, dtype)
    q, r = np.asarray(k.q, dtype=dtype), np.asarray(k.r, dtype=dtype)
    x = np.asarray(x0, dtype=dtype).copy()
    Pm = np.tril(np.asarray(P0, dtype=dtype))
    Pm = Pm + np.tril(Pm, -1).T
    xf = np.full((T, NX), np.nan, dtype=dtype)
    pstd, innov = (np.full((T, N), np.nan, dtype=dtype) for _ in range(2))
    tape = np.full((T, TAPE), np.nan, dtype=dtype)
    ell, nupd, failed, pivmin, ewmin, n, c_form = dtype(0), 0, -1, np.inf, np.inf, T, 0.0
    for t in range(T):
        x, Pm, inn, dl, napp, ew, bad = uq.update_row(x, Pm, Y[t], r, dtype)
        nupd, ewmin = nupd + napp, min(ewmin, ew)
        ell = ell + dl
        if bad:
            failed, n = t, t
            break
        xf[t], innov[t] = x, inn
        with np.errstate(invalid="ignore"):
            pstd[t] = np.sqrt(np.diagonal(Pm))
        tape[t, PF] = pack(Pm)
        x, Pm, piv, ew, bad, C, Ct = predict_tape(c, integ, dt, x, Pm, U[t], w, q, dtype)
        pivmin = min([pivmin] + [float(v) for v in piv])
        ewmin = min(ewmin, ew)
        if bad:
            failed, n = t, t + 1
            break
        tape[t, XP], tape[t, PP], tape[t, CC] = x, pack(Pm), C.reshape(-1)
        c_form = max(c_form, float(np.max(np.abs(C - Ct)) / np.max(np.abs(Ct))))
    if failed >= 0:
        x, Pm, ell = np.full(NX, np.nan, dtype=dtype), np.full((N, N), np.nan, dtype=dtype), dtype(-np.inf)
    return dict(xf=xf, pstd=pstd, innov=innov, xT=x, PT=Pm, info=np.array([ell, nupd, failed, pivmin], dtype=dtype), f_ew_min=ewmin,
                f_pivot_min=pivmin, tape=tape, nrows=dtype(n), c_form=c_form)


def delta(xs, xp, dtype, variant=None):
    """(xs [-] xp [12], the normalised |e_w|)"""
    if variant == "dx_linear":
        return np.concatenate([xs[:3] - xp[:3], xs[4:7] - xp[4:7], xs[7:] - xp[7:]]), 1.0
    return uq.boxminus(xs, xp, "minus_left" if variant == "minus_left" else None)


def rts_one(xf, tape, n, dtype, terminal=None, variant=None):
    """the backward pass of one problem.  Returns dict(xs, pstd_s, Ps, Ps0, sinfo, ew_min, pivot_min)"""
    T = xf.shape[0]
    xf, tape = np.asarray(xf, dtype=dtype), np.asarray(tape, dtype=dtype)
    xs = np.full((T, NX), np.nan, dtype=dtype)
    Ps = np.full((T, N, N), np.nan, dtype=dtype)
    Pf = np.stack([unpack(tape[t, PF], dtype) for t in range(T)])
    nan2 = np.full((N, N), np.nan, dtype=dtype)
    n = float(n)
    n = 0 if np.isnan(n) else int(min(max(n, 0.0), float(T)))       # the clamp of the header: the fraction dropped, NaN counts as 0, +inf as T
    if n == 0:
        return dict(xs=xs, pstd_s=np.full((T, N), np.nan, dtype=dtype), Ps=Ps, Ps0=nan2, sinfo=np.full(2, np.nan, dtype=dtype), ew_min=np.inf,
                    pivot_min=np.inf)
    if terminal is not None and n == T:
        x = np.asarray(terminal[0], dtype=dtype)
        Pm = np.tril(np.asarray(terminal[1], dtype=dtype))
        Pm = Pm + np.tril(Pm, -1).T
        first = T - 1
    else:
        x, Pm = xf[n - 1], Pf[n - 1]
        xs[n - 1], Ps[n - 1] = x, Pm
        first = n - 2
    failed, pivmin, ewmin = -1, np.inf, np.inf
    for t in range(first, -1, -1):
        xp, Pp, C = tape[t, XP], unpack(tape[t, PP], dtype), tape[t, CC].reshape(N, N)
        L, bad, piv = ur.cholesky(Pp, dtype)
        pivmin = min([pivmin] + [float(v) for v in piv])
        if bad:
            failed = t
            break
        with np.errstate(all="ignore"):
            d, ew = delta(x, xf[t + 1] if variant == "dx_from_xf" and t + 1 < T else xp, dtype, variant)
        ewmin = min(ewmin, ew)
        if not np.all(np.isfinite(d)):
            failed = t
            break
        G = gain(C.T if variant == "C_T" else C, L, dtype)
        x = uq.boxplus(xf[t], G @ d, "plus_left" if variant == "plus_left" else None)
        Pm = np.tril(Pf[t] + G @ (Pm - (Pf[t + 1] if variant == "no_Pp" and t + 1 < T else Pp)) @ G.T)     # one expression serves both triangles
        Pm = Pm + np.tril(Pm, -1).T
        xs[t], Ps[t] = x, Pm
    if failed >= 0:
        xs[:failed + 1], Ps[:failed + 1] = np.nan, np.nan
    with np.errstate(invalid="ignore"):
        pstd_s = np.sqrt(np.diagonal(Ps, axis1=-2, axis2=-1))
    return dict(xs=xs, pstd_s=pstd_s, Ps=Ps, Ps0=Ps[0].copy() if failed < 0 else nan2, sinfo=np.array([failed, pivmin], dtype=dtype), ew_min=ewmin,
                pivot_min=pivmin)


def smooth(integ, vehicles, cfgs, x0, P0, U, Y, dt, dtype=np.float64, terminal=None, variant=None):
    """brov_ukf_smooth_quat, with an optional terminal pair (xs_T [P,B,13], Ps_T [P,B,12,12]) for the backward pass.  Arguments as
    ukf_quat_ref.filter; x0 [B,13] / P0 [B,12,12] shared by the candidates."""
    assert variant is None or variant in VARIANTS
    cfgs = [cfgs] * len(vehicles) if isinstance(cfgs, ur.Cfg) else list(cfgs)
    U, Y = np.asarray(U, dtype=dtype), np.asarray(Y, dtype=dtype)
    B = U.shape[0]
    out = {}
    for j, v in enumerate(vehicles):
        c = fp._Prep(v, dt, dtype)
        rows = []
        for b in range(B):
            f = forward_one(c, integ, dt, cfgs[j], x0[b], P0[b], U[b], Y[b], dtype)
            f.update(rts_one(f["xf"], f["tape"], f["nrows"], dtype, None if terminal is None else (terminal[0][j, b], terminal[1][j, b]), variant))
            rows.append(f)
        for k in rows[0]:
            out.setdefault(k, []).append(np.stack([np.asarray(r[k]) for r in rows]))
    return {k: np.stack(v) for k, v in out.items()}


# ---- on the cases of tests/ukf_quat_cases.py: computed once, shared by the CPU and the GPU tests, read-only ------------------------------
NAMES = tuple(sorted(qc.CASES))
TOL = 1e-10                 # the bound of tests/test_ukf_quat_gpu.py and tests/test_ukf_smooth_gpu.py
EW = 0.5
PIVOT = 1e-4


def vehicles():
    return [fv.vehicle(n) for n in qc.NAMES]


def smooth_case(name, ld=False, variant=None, **kw):
    """smooth() on ukf_quat_cases.inputs(name) with the entries of kw replaced"""
    i = qc.inputs(name)
    a = dict(x0=i["x0"], P0=i["P0"], U=i["U"], Y=i["Y"], terminal=None, cfgs=i["cfgs"])
    a.update(kw)
    return smooth(qc.INTEG[i["integ"]], vehicles(), a["cfgs"], a["x0"], a["P0"], a["U"], a["Y"], qc.DT, dtype=qc.L if ld else np.float64,
                  terminal=a["terminal"], variant=variant)


@functools.lru_cache(maxsize=None)
def reference(name, ld=False, variant=None):
    return smooth_case(name, ld, variant)


def tape_fields(tape):
    """the four fields of a tape [..., 313]: Pf and Pp unpacked to [..., 12, 12], xp [..., 13], C [..., 12, 12]"""
    tape = np.asarray(tape)

    def sym(v):
        Pm = np.zeros(v.shape[:-1] + (12, 12), dtype=v.dtype)
        Pm[..., usr.TRIL[0], usr.TRIL[1]] = v
        Pm[..., usr.TRIL[1], usr.TRIL[0]] = v
        return Pm
    return dict(Pf=sym(tape[..., PF]), xp=tape[..., XP], Pp=sym(tape[..., PP]), C=tape[..., CC].reshape(tape.shape[:-1] + (12, 12)))


def cross_err(tape, ref):
    """max |dC_ab| / sqrt(Pf_aa Pp_bb) over a tape"""
    a, b = tape_fields(tape), tape_fields(ref)
    if np.any(np.isnan(a["C"]) != np.isnan(b["C"])):
        return np.inf
    sa = np.sqrt(np.diagonal(b["Pf"], axis1=-2, axis2=-1)).astype(qc.L)
    sb = np.sqrt(np.diagonal(b["Pp"], axis1=-2, axis2=-1)).astype(qc.L)
    rel = np.abs(a["C"].astype(qc.L) - b["C"].astype(qc.L)) / (sa[..., :, None] * sb[..., None, :])
    ok = ~np.isnan(rel)
    return float(np.max(rel[ok])) if ok.any() else 0.0


def gaps(o, ol):
    """{output: error of o against ol} for the smoother's outputs and the four tape fields: the mixed error of ukf_cases.err, covariances
    as |dP_ij| / sqrt(P_ii P_jj), C as |dC_ab| / sqrt(Pf_aa Pp_bb)"""
    g = {k: qc.err(o[k], ol[k]) for k in ("xs", "pstd_s")}
    g["Ps"], g["Ps0"] = qc.cov_err(o["Ps"], ol["Ps"]), qc.cov_err(o["Ps0"], ol["Ps0"])
    a, b = tape_fields(o["tape"]), tape_fields(ol["tape"])
    g["tape Pf"], g["tape Pp"] = qc.cov_err(a["Pf"], b["Pf"]), qc.cov_err(a["Pp"], b["Pp"])
    g["tape xp"] = qc.err(a["xp"], b["xp"])
    g["tape C"] = cross_err(o["tape"], ol["tape"])
    g["sinfo[1]"] = qc.err(np.asarray(o["sinfo"])[..., 1], np.asarray(ol["sinfo"])[..., 1])
    return g
