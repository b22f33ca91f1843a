"""NumPy restatement of the EM statistics of include/brov2.h (brov_ukf_rts_em_dev, brov_ukf_smooth_em) on top of
tests/ukf_smooth_ref.py, whose filter, tape and backward pass it uses, and of the M-step and the loop of fossen/estimate.py
(em_update, fit_noise).  Dtype-generic (np.float64 / np.longdouble); not collected by pytest, shares no code with the product.

term()    the process term of one transition: q + q^2 (u_i^T M u_i + (u_i . dx)^2) per component, u_i = Pp^-1 e_i by two
          triangular solves, no inverse
stats()   ukf_smooth_ref.smooth plus em [P, B, 37] = Sq | Sr | nr | nq
m_step()  the pooled update of q and r
em()      the loop"""
import numpy as np

import ukf_ref as ur
import ukf_smooth_ref as usr

N = ur.N
EM = 37
SQ, SR, NR, NQ = slice(0, 12), slice(12, 24), slice(24, 36), 36


def term(q, L, M, dx, dtype):
    """[12]: q_i + q_i^2 (u_i^T M u_i + (u_i . dx)^2), u_i = (L L^T)^-1 e_i, the inner sums in index order"""
    n = len(q)                                              # (12; the identity test runs a smaller linear model through it)
    out = np.zeros(n, dtype=dtype)
    for i in range(n):
        w = np.zeros(n, dtype=dtype)
        for j in range(n):                                  # L w = e_i
            w[j] = ((dtype(1) if i == j else dtype(0)) - w[:j] @ L[j, :j]) / L[j, j]
        u = np.zeros(n, dtype=dtype)
        for j in range(n - 1, -1, -1):                      # L^T u = w
            u[j] = (w[j] - u[j + 1:] @ L[j + 1:, j]) / L[j, j]
        umu, udx = dtype(0), dtype(0)
        for c in range(n):
            mu = dtype(0)
            for k in range(n):
                mu = mu + M[c, k] * u[k]
            umu = umu + u[c] * mu
            udx = udx + u[c] * dx[c]
        out[i] = q[i] + q[i] * q[i] * (umu + udx * udx)
    return out


def stats_one(s, Y, q, r, dtype, terminal=None):
    """em [37] of one problem from its smoothed dict s (ukf_smooth_ref: xf, tape, nrows, xs, Ps, Pf, sinfo), its rows Y [T,12] and
    the variances of its candidate"""
    T = s["xf"].shape[0]
    n = float(s["nrows"])
    n = 0 if np.isnan(n) else int(min(max(n, 0.0), float(T)))
    nan = np.full(EM, np.nan, dtype=dtype)
    if n == 0 or s["sinfo"][0] >= 0:
        return nan
    q, r = np.asarray(q, dtype=dtype), np.asarray(r, dtype=dtype)
    Y = np.asarray(Y, dtype=dtype)
    tape, xs, Ps = np.asarray(s["tape"], dtype=dtype), s["xs"], s["Ps"]
    em = np.zeros(EM, dtype=dtype)
    with_pair = terminal is not None and n == T
    if with_pair:
        xT = np.asarray(terminal[0], dtype=dtype)
        PT = np.tril(np.asarray(terminal[1], dtype=dtype))
        PT = PT + np.tril(PT, -1).T

    def row(t):
        for i in range(N):
            if np.isnan(Y[t, i]) or np.isposinf(r[i]):
                continue
            v = Y[t, i] - xs[t, i]
            if 3 <= i < 6:
                v = ur._wrap(v, dtype)[0]
            em[12 + i] += v * v + Ps[t, i, i]
            em[24 + i] += 1
    if not with_pair:
        row(n - 1)
    for t in range(n - 1 if with_pair else n - 2, -1, -1):
        nxt = (xT, PT) if t == T - 1 else (xs[t + 1], Ps[t + 1])
        Pp = usr.unpack(tape[t, usr.PP], dtype)
        L, bad, _ = ur.cholesky(Pp, dtype)
        assert not bad
        em[SQ] += term(q, L, nxt[1] - Pp, nxt[0] - tape[t, usr.XP], dtype)
        em[NQ] += 1
        row(t)
    return em


def stats(model, integ, lag_mode, vehicles, cfgs, x0, P0, U, Y, dt, lag=None, dtype=np.float64, terminal=None):
    """ukf_smooth_ref.smooth with em [P,B,37] added"""
    o = usr.smooth(model, integ, lag_mode, vehicles, cfgs, x0, P0, U, Y, dt, lag=lag, dtype=dtype, terminal=terminal)
    cl = [cfgs] * len(vehicles) if isinstance(cfgs, ur.Cfg) else list(cfgs)
    P, B = o["xs"].shape[:2]
    em = np.zeros((P, B, EM), dtype=dtype)
    for j in range(P):
        for b in range(B):
            s = {k: o[k][j, b] for k in ("xf", "tape", "nrows", "xs", "Ps", "sinfo")}
            em[j, b] = stats_one(s, Y[b], cl[j].q, cl[j].r, dtype, None if terminal is None else (terminal[0][j, b], terminal[1][j, b]))
    o["em"] = em
    return o


def m_step(em, info, sinfo, cfgs, fit_q=True, fit_r=True, q_floor=0.0, r_floor=0.0):
    """(new Cfg per candidate, number of problems left out).  Per candidate, pooled over its recordings whose filter (info[2] = -1)
    and backward pass (sinfo[0] = -1) completed; ValueError when a candidate has none."""
    dtype = em.dtype.type
    P = em.shape[0]
    fq, fr = np.broadcast_to(np.asarray(fit_q, bool), (N,)), np.broadcast_to(np.asarray(fit_r, bool), (N,))
    out, left = [], 0
    for j in range(P):
        ok = (info[j, :, 2] == -1) & (sinfo[j, :, 0] == -1)
        left += int((~ok).sum())
        if not ok.any():
            raise ValueError(f"every recording of candidate {j} failed")
        e = em[j][ok]
        q, r = np.asarray(cfgs[j].q, dtype=dtype).copy(), np.asarray(cfgs[j].r, dtype=dtype).copy()
        nq = e[:, NQ].sum()
        for i in range(N):
            if fq[i] and nq > 0:
                q[i] = max(e[:, i].sum() / nq, dtype(q_floor))
            nr = e[:, 24 + i].sum()
            if fr[i] and nr > 0:
                r[i] = max(e[:, 12 + i].sum() / nr, dtype(r_floor))
        out.append((q, r))
    return out, left


def em(model, integ, lag_mode, vehicles, cfgs, x0, P0, U, Y, dt, iters, lag=None, dtype=np.float64, **kw):
    """`iters` EM iterations from cfgs (one Cfg or P).  Returns dict(q, r [P,12] after the last M-step, loglik [iters + 1, P] =
    the sum over the recordings of info[0] under the noise model of each iteration, the last row under the fitted one, q_hist,
    r_hist [iters + 1, P, 12]).  q and r are carried in `dtype`; the Cfg of an iteration holds them in that dtype as well."""
    cl = [cfgs] * len(vehicles) if isinstance(cfgs, ur.Cfg) else list(cfgs)
    ll, qh, rh = [], [], []
    for it in range(iters + 1):
        qh.append(np.stack([np.asarray(c.q, dtype=dtype) for c in cl]))
        rh.append(np.stack([np.asarray(c.r, dtype=dtype) for c in cl]))
        if it == iters:
            o = usr.smooth(model, integ, lag_mode, vehicles, cl, x0, P0, U, Y, dt, lag=lag, dtype=dtype)
            ll.append(o["info"][:, :, 0].sum(axis=1))
            break
        o = stats(model, integ, lag_mode, vehicles, cl, x0, P0, U, Y, dt, lag=lag, dtype=dtype)
        ll.append(o["info"][:, :, 0].sum(axis=1))
        new, _ = m_step(o["em"], o["info"], o["sinfo"], cl, **kw)
        cl = [ur.Cfg(q=q, r=r, alpha=c.alpha, beta=c.beta, kappa=c.kappa) for (q, r), c in zip(new, cl)]
    return dict(q=qh[-1], r=rh[-1], loglik=np.stack(ll), q_hist=np.stack(qh), r_hist=np.stack(rh))


# ---- the lag-one form on a linear-Gaussian model (tests/test_ukf_em_cpu.py: the identity) -------------------------------------
def linear_identity(seed=11, n=5, T=30):
    """Kalman filter and RTS smoother of x' = A x + w, y = x + v (diagonal Q with one zero, dropped measurements) in float64.
    Returns (lag, loc) [T-1, n]: the diagonal of E[w w^T | Y] per transition by the lag-one (Shumway-Stoffer) form
    Ps_{t+1} - Ps_{t+1,t} A^T - A Ps_{t,t+1} + A Ps_t A^T + e e^T, e = xs_{t+1} - A xs_t, Ps_{t+1,t} = Ps_{t+1} G_t^T, and by the
    local form Q + Q Pp^-1 (Ps_{t+1} - Pp + d d^T) Pp^-1 Q."""
    rng = np.random.default_rng(seed)
    A = 0.9 * np.eye(n) + 0.2 * rng.normal(size=(n, n))
    q = rng.uniform(0.01, 0.1, n)
    q[2] = 0.0
    r = rng.uniform(0.02, 0.2, n)
    Q = np.diag(q)
    x = rng.normal(size=n)
    Ys = []
    for _ in range(T):
        y = x + rng.normal(size=n) * np.sqrt(r)
        y[rng.uniform(size=n) < 0.3] = np.nan
        Ys.append(y)
        x = A @ x + rng.normal(size=n) * np.sqrt(q)
    m, Pm = np.zeros(n), np.eye(n)
    mf, Pf, mp, Pp = [], [], [], []
    for t in range(T):
        for i in range(n):
            if np.isnan(Ys[t][i]):
                continue
            s = Pm[i, i] + r[i]
            k = Pm[:, i] / s
            m = m + k * (Ys[t][i] - m[i])
            Pm = Pm - np.outer(k, k) * s
        mf.append(m)
        Pf.append(Pm)
        m, Pm = A @ m, A @ Pm @ A.T + Q
        mp.append(m)
        Pp.append(Pm)
    ms, Ps, G = [None] * T, [None] * T, [None] * T
    ms[T - 1], Ps[T - 1] = mf[T - 1], Pf[T - 1]
    for t in range(T - 2, -1, -1):
        G[t] = np.linalg.solve(Pp[t], A @ Pf[t]).T
        ms[t] = mf[t] + G[t] @ (ms[t + 1] - mp[t])
        Ps[t] = Pf[t] + G[t] @ (Ps[t + 1] - Pp[t]) @ G[t].T
    lag, loc = [], []
    for t in range(T - 1):
        cross = Ps[t + 1] @ G[t].T
        e = ms[t + 1] - A @ ms[t]
        lag.append(np.diagonal(Ps[t + 1] - cross @ A.T - A @ cross.T + A @ Ps[t] @ A.T + np.outer(e, e)))
        L = np.linalg.cholesky(Pp[t])
        loc.append(term(q, L, Ps[t + 1] - Pp[t], ms[t + 1] - mp[t], np.float64))
    return np.array(lag), np.array(loc)
