"""NumPy restatement of linear model-predictive control with an EDMDc model (include/brov2.h: edmdc_lmpc_step), for the tests.
Not collected.

dtype-generic (np.float64 / np.longdouble).  The coefficients P and Gc are formed here in `dtype` (markov), the gradient g and the
constant c from them; the ADMM loop restates the iteration with its stop rule and keeps the residuals of every iteration; the
predicted states under the result and the cost J come from the ITERATED recursion z <- A z + B v (koopman_mppi_ref.predict), never
from the linear form the kernel evaluates.  W is an argument, as it is for the library."""
import types

import numpy as np

import koopman_mppi_ref as kr


def two_pi(dtype):
    return dtype(8) * np.arctan(dtype(1))


def rec(n, nu, q, qf=None, r=0.0, u_min=-np.inf, u_max=np.inf, hold=1, iters=200, tol=0.0, rho=1.0):
    """the record as plain float64 arrays"""
    vec = lambda v, m: np.full(m, float(v)) if np.ndim(v) == 0 else np.asarray(v, dtype=float).copy()
    q = vec(q, n)
    return types.SimpleNamespace(n=n, nu=nu, q=q, qf=q.copy() if qf is None else vec(qf, n), r=vec(r, nu), u_min=vec(u_min, nu),
                                 u_max=vec(u_max, nu), hold=int(hold), iters=int(iters), tol=float(tol), rho=float(rho))


def with_(c, **kw):
    d = dict(vars(c))
    d.update(kw)
    return types.SimpleNamespace(**d)


def to_struct(c):
    """the _lib.BrovLmpc of a record, through the public builder"""
    from bluerov2_dynamics_amd.fossen import control
    return control.lmpc(c.q, c.qf, c.r, c.u_min, c.u_max, hold=c.hold, iters=c.iters, tol=c.tol, rho=c.rho, nu=c.nu, n=c.n)


def synth_model(n, r, k, seed):
    """(C [k,n] | None, gamma, A, B): the seeded synthetic model of tests/test_koopman_mppi_gpu.py restated -- A = 0.98 A0 / rho(A0)
    with A0 = I + 0.3 G / sqrt(d), B and the centres of the size of the states"""
    rng = np.random.default_rng(seed + 10 * n + r + k)
    d = n + k
    A0 = np.eye(d) + 0.3 * rng.normal(size=(d, d)) / np.sqrt(d)
    A = 0.98 * A0 / np.max(np.abs(np.linalg.eigvals(A0)))
    return (rng.uniform(-0.5, 0.5, (k, n)) if k else None), 0.5, A, 0.1 * rng.normal(size=(d, r))


def knots(H, hold):
    return (H + hold - 1) // hold


def markov(A, B, n, H, hold, dtype=np.float64):
    """(P [H+1,n,d], Gc [H+1,M,n,r]) as include/brov2.h defines them, in `dtype`"""
    A, B = np.asarray(A, dtype=dtype), np.asarray(B, dtype=dtype)
    d, r = A.shape[0], B.shape[1]
    M = knots(H, hold)
    P = np.zeros((H + 1, n, d), dtype=dtype)
    P[0, :, :n] = np.eye(n, dtype=dtype)
    G = np.zeros((H, n, r), dtype=dtype)
    for t in range(H):
        G[t] = P[t] @ B
        P[t + 1] = P[t] @ A
    Gc = np.zeros((H + 1, M, n, r), dtype=dtype)
    for t in range(1, H + 1):
        for s in range(t):
            Gc[t, s // hold] += G[t - 1 - s]
    return P, Gc


def adjust(rows, x, dtype=np.float64):
    """the reference rows [H+1,n] adjusted once against the measured state x [n]"""
    rt = np.asarray(rows, dtype=dtype).copy()
    x = np.asarray(x, dtype=dtype)
    if rt.shape[1] == 12:
        tp = two_pi(dtype)
        rt[:, 3:6] = rt[:, 3:6] - tp * np.rint((rt[:, 3:6] - x[3:6]) / tp)
    else:
        flip = (rt[:, 3:7] @ x[3:7]) < 0
        rt[flip, 3:7] = -rt[flip, 3:7]
    return rt


def window(ref_b, ref_row0, H):
    """the H + 1 reference rows of one problem: ref_b [rows,n]"""
    return np.repeat(ref_b[:1], H + 1, axis=0) if ref_b.shape[0] == 1 else ref_b[ref_row0:ref_row0 + H + 1]


def stage_weights(c, dt, H, dtype=np.float64):
    """wq [H+1,n] = w_t Q_t"""
    wq = np.repeat((dtype(dt) * c.q.astype(dtype))[None], H + 1, axis=0)
    wq[H] = c.qf.astype(dtype)
    return wq


def condense(Gc, c, dt, H, dtype=np.float64):
    """(Hq [Nv,Nv], steps [M])"""
    Gc = np.asarray(Gc, dtype=dtype)
    M, n, r = Gc.shape[1:]
    G = Gc.transpose(0, 2, 1, 3).reshape(H + 1, n, M * r)
    wq = stage_weights(c, dt, H, dtype)
    steps = np.minimum(c.hold, H - c.hold * np.arange(M))
    Hq = dtype(2) * np.einsum("tia,ti,tib->ab", G, wq, G) + dtype(2) * np.diag((dtype(dt) * np.outer(steps.astype(dtype), c.r.astype(dtype))).ravel())
    return Hq, steps


def gradient(c, F, Gc, rt, dt, H, dtype=np.float64):
    """(g [Nv], c0) from the free response F [H+1,n], Gc and the adjusted reference rows rt [H+1,n]"""
    Gc = np.asarray(Gc, dtype=dtype)
    M, n, r = Gc.shape[1:]
    G = Gc.transpose(0, 2, 1, 3).reshape(H + 1, n, M * r)
    wq = stage_weights(c, dt, H, dtype)
    e0 = np.asarray(F, dtype=dtype) - rt
    return dtype(2) * np.einsum("tia,ti->a", G, wq * e0), np.sum(wq * e0 * e0)


def cost(c, pred, rt, v, dt, H, dtype=np.float64):
    """J of the knots v [M,r] whose predicted states are pred [H+1,n]"""
    e = rt - np.asarray(pred, dtype=dtype)
    q, qf, r = c.q.astype(dtype), c.qf.astype(dtype), c.r.astype(dtype)
    v = np.asarray(v, dtype=dtype)
    J = dtype(0)
    for t in range(H):
        u = v[t // c.hold]
        J = J + dtype(dt) * (np.sum(q * e[t] * e[t]) + np.sum(r * u * u))
    return J + np.sum(qf * e[H] * e[H])


def admm(c, W, g, z0, y0, dtype=np.float64, iters=None, tol=None):
    """(z, y, r_prim, r_dual, iterations, history [iterations,2]) of the iteration from (z0, y0); z0 is clipped here"""
    iters = c.iters if iters is None else iters
    tol = dtype(c.tol if tol is None else tol)
    W, g = np.asarray(W, dtype=dtype), np.asarray(g, dtype=dtype)
    nv = g.shape[0]
    lo, hi = np.tile(c.u_min.astype(dtype), nv // c.nu), np.tile(c.u_max.astype(dtype), nv // c.nu)
    rho = dtype(c.rho)
    z = np.minimum(np.maximum(np.asarray(z0, dtype=dtype).ravel(), lo), hi)
    y = np.asarray(y0, dtype=dtype).ravel().copy()
    rp = rd = dtype(np.inf)
    hist = []
    it = 0
    while it < iters:
        v = W @ (rho * (z - y) - g)
        t = v + y
        zn = np.minimum(np.maximum(t, lo), hi)
        y = t - zn
        rp, rd = np.max(np.abs(v - zn)), rho * np.max(np.abs(zn - z))
        z = zn
        it += 1
        hist.append((rp, rd))
        if tol > 0 and rp <= tol and rd <= tol:
            break
    return z, y, rp, rd, it, np.array(hist, dtype=dtype).reshape(-1, 2)


def projected_gradient_residual(Hq, g, z, lo, hi):
    """|z - clip(z - (Hq z + g) / lambda_max)|_inf: zero exactly at the minimiser of the box-constrained QP"""
    step = 1.0 / np.linalg.eigvalsh(Hq)[-1]
    return float(np.max(np.abs(z - np.minimum(np.maximum(z - step * (Hq @ z + g), lo), hi))))


def step(C, gamma, A, B, c, W, x, ref, U_nom, dt, H, y=None, ref_row0=0, shift=False, dtype=np.float64):
    """One call for nb problems: x [nb,n], ref [nb,rows,n], U_nom [nb,M,r], y [nb,M,r] | None -> dict(U_nom, y (after the shift), z, u_apply
    [nb,hold,r], pred [nb,H+1,n], info [nb,6], g [nb,Nv], c0 [nb], hist (list of [iterations,2]))"""
    x, ref, U_nom = np.asarray(x), np.asarray(ref), np.asarray(U_nom)
    nb, M, r = U_nom.shape
    n = x.shape[1]
    assert M == knots(H, c.hold) and r == np.shape(B)[1] == c.nu and n == c.n
    P, Gc = markov(A, B, n, H, c.hold, dtype)
    lo, hi = np.tile(c.u_min.astype(dtype), M), np.tile(c.u_max.astype(dtype), M)
    out = dict(U_nom=[], y=[], z=[], u_apply=[], pred=[], info=[], g=[], c0=[], hist=[])
    for b in range(nb):
        rt = adjust(window(ref[b], ref_row0, H), x[b], dtype)
        F = P @ kr.lift(x[b], C, gamma, dtype)
        g, c0 = gradient(c, F, Gc, rt, dt, H, dtype)
        z0 = np.minimum(np.maximum(np.asarray(U_nom[b], dtype=dtype).ravel(), lo), hi)
        y0 = np.zeros(M * r, dtype=dtype) if y is None else np.asarray(y[b], dtype=dtype).ravel()
        if not (np.all(np.isfinite(g)) and np.isfinite(c0)):
            inf = dtype(np.inf)
            vals = dict(U_nom=np.asarray(U_nom[b], dtype=dtype), y=y0.reshape(M, r), z=z0.reshape(M, r),
                        u_apply=np.repeat(z0[None, :r], c.hold, axis=0), pred=np.full((H + 1, n), np.nan, dtype=dtype),
                        info=np.array([inf, inf, inf, inf, 0, 0], dtype=dtype), g=g, c0=c0, hist=np.zeros((0, 2), dtype=dtype))
        else:
            z, yy, rp, rd, it, hist = admm(c, W, g, z0, y0, dtype)
            z, yy = z.reshape(M, r), yy.reshape(M, r)
            pred = kr.predict(C, gamma, A, B, x[b], z[None], H, c.hold, dtype)[0]
            pred0 = kr.predict(C, gamma, A, B, x[b], z0.reshape(1, M, r), H, c.hold, dtype)[0]
            nbound = int(np.sum((z == lo.reshape(M, r)) | (z == hi.reshape(M, r))))
            info = np.array([cost(c, pred, rt, z, dt, H, dtype), cost(c, pred0, rt, z0.reshape(M, r), dt, H, dtype), rp, rd, it, nbound], dtype=dtype)
            sh = (lambda a: np.concatenate([a[1:], a[-1:]], axis=0)) if shift else (lambda a: a)
            vals = dict(U_nom=sh(z), y=sh(yy), z=z, u_apply=np.repeat(z[:1], c.hold, axis=0), pred=pred, info=info, g=g, c0=c0, hist=hist)
        for key, val in vals.items():
            out[key].append(val)
    return {key: (val if key == "hist" else np.stack(val)) for key, val in out.items()}


# ------------------------------------------------------------------------------------------ the cases the CPU and GPU tests share
SEED = 4210
DT = 0.05
REF_TOTAL, ROW0 = 4, 2      # rows beyond the window of a trajectory case, and its first row
# name -> n, r, k, H, hold, nb, iters, tol, trajectory reference, y given, special
CASES = {
    "nv6": dict(n=13, r=6, k=5, H=3, hold=3, nb=1, iters=40, tol=0.0, traj=False, y=False, special="quat_flip"),       # M = 1
    "nv8": dict(n=12, r=8, k=0, H=1, hold=1, nb=3, iters=2, tol=0.0, traj=True, y=True, special=None),                 # M = 1, a linear model
    "it0": dict(n=12, r=8, k=0, H=1, hold=1, nb=3, iters=0, tol=0.0, traj=True, y=True, special=None),
    "nv24": dict(n=12, r=8, k=5, H=7, hold=3, nb=5, iters=40, tol=0.0, traj=True, y=True, special="angle_wrap"),       # short last knot, two blocks
    "nv64": dict(n=12, r=8, k=70, H=8, hold=1, nb=3, iters=1, tol=0.0, traj=False, y=False, special=None),             # d crosses 64
    "nv72": dict(n=13, r=6, k=70, H=12, hold=1, nb=3, iters=40, tol=0.0, traj=True, y=True, special="quat_flip"),      # a second row per lane
    "nv90": dict(n=12, r=6, k=5, H=15, hold=1, nb=5, iters=40, tol=0.0, traj=False, y=False, special=None),            # W in LDS, the last such size
    "nv96": dict(n=12, r=8, k=5, H=12, hold=1, nb=5, iters=40, tol=0.0, traj=True, y=False, special=None),             # W from global memory
    "nv312": dict(n=12, r=8, k=0, H=39, hold=1, nb=3, iters=40, tol=0.0, traj=False, y=False, special=None),           # five rows per lane
    "nb65": dict(n=12, r=8, k=5, H=7, hold=3, nb=65, iters=40, tol=0.0, traj=False, y=True, special=None),             # seventeen blocks, the last with one wave
    # stop by the residuals.  With limits that are reached, the rows at a limit converge at the rate Hq / (Hq + rho) and the free rows at
    # rho / (Hq + rho): one of the two is >= 1/2, and no residual can fall from 10 tol to tol / 10 in one iteration, which is what an
    # exactly comparable iteration count needs (stop_well_posed).  So this case has limits that stay out of reach (+-5) and
    # rho = lambda_min / 10 000: every mode contracts by <= 1e-4 per iteration.  Every other problem starts 10 000 times nearer to its
    # minimiser (a warm start), so the problems of the first block stop at iterations 3, 2, 3, 2.
    "tol": dict(n=12, r=8, k=5, H=7, hold=3, nb=5, iters=60, tol=1e-12, traj=True, y=False, special="warm"),
}


def stop_well_posed(hist, tol):
    """The iteration count of a problem that stopped by its residuals can be compared exactly when the deciding residual,
    max(r_prim, r_dual), is a factor 10 away from tol at the stop iteration (<= tol / 10) and at the one before it (>= 10 tol).
    hist [iterations,2] of admm; False for a problem that made no iteration."""
    worst = np.max(np.asarray(hist, dtype=np.longdouble), axis=1)
    it = worst.shape[0]
    return bool(it >= 1 and worst[-1] <= tol / 10 and (it == 1 or worst[-2] >= 10 * tol))


def case_model(name):
    s = CASES[name]
    return synth_model(s["n"], s["r"], s["k"], SEED)


def case_record(name):
    """random weights; limits +-(0.2 .. 0.35) per channel, with channel 1 fixed (u_min = u_max) and channel 2 free (+-inf).  rho is
    filled by case_solver."""
    s = CASES[name]
    n, r = s["n"], s["r"]
    rng = np.random.default_rng(SEED + 90 + r + n)
    lo, hi = -np.linspace(0.35, 0.2, r), np.linspace(0.2, 0.35, r)
    lo[1] = hi[1] = 0.1
    if s["special"] == "warm":
        lo, hi = np.full(r, -5.0), np.full(r, 5.0)
    lo[2], hi[2] = -np.inf, np.inf
    return rec(n, r, rng.uniform(0.5, 2.0, n), rng.uniform(2.0, 8.0, n), rng.uniform(0.05, 0.2, r), lo, hi, hold=s["hold"], iters=s["iters"],
               tol=s["tol"])


def case_solver(name):
    """(record with rho = sqrt(lambda_min lambda_max) of Hq, Hq, W = (Hq + rho I)^-1): float64, what a caller would pass"""
    s = CASES[name]
    _, _, A, B = case_model(name)
    c = case_record(name)
    Hq = condense(markov(A, B, s["n"], s["H"], s["hold"])[1], c, DT, s["H"])[0]
    Hq = 0.5 * (Hq + Hq.T)
    ev = np.linalg.eigvalsh(Hq)
    c = with_(c, rho=float(ev[0] / 1e4 if s["special"] == "warm" else np.sqrt(ev[0] * ev[-1])))
    W = np.linalg.inv(Hq + c.rho * np.eye(Hq.shape[0]))
    return c, Hq, np.ascontiguousarray(0.5 * (W + W.T))


def case_inputs(name):
    """x [nb,n], ref [nb,rows,n], U [nb,M,r] (a part outside the limits), y [nb,M,r] | None, ref_row0"""
    s = CASES[name]
    n, r, nb, H = s["n"], s["r"], s["nb"], s["H"]
    M = knots(H, s["hold"])
    rng = np.random.default_rng(SEED + 7 * H + nb + len(name))
    rows = H + 1 + REF_TOTAL if s["traj"] else 1
    x, ref = rng.uniform(-0.5, 0.5, (nb, n)), rng.uniform(-0.5, 0.5, (nb, rows, n))
    if n == 13:
        x[:, 3:7] /= np.linalg.norm(x[:, 3:7], axis=1, keepdims=True)
        ref[:, :, 3:7] = x[:, None, 3:7] + 0.2 * ref[:, :, 3:7]
        ref[:, :, 3:7] /= np.linalg.norm(ref[:, :, 3:7], axis=2, keepdims=True)
    if s["special"] == "quat_flip":                     # every other problem's reference on the far hemisphere
        ref[::2, :, 3:7] = -ref[::2, :, 3:7]
    if s["special"] == "angle_wrap":                    # yaw reference 2 pi + 0.1 beyond the state, roll reference 2 pi - 0.2 below it
        ref[:, :, 5] = x[:, None, 5] + 2 * np.pi + 0.1 + 0.01 * ref[:, :, 5]
        ref[:, :, 3] = x[:, None, 3] - 2 * np.pi + 0.2 + 0.01 * ref[:, :, 3]
    U = rng.uniform(-0.4, 0.4, (nb, M, r))
    if s["special"] == "warm":                          # every other problem 10 000 times nearer to its unconstrained minimiser
        C, gamma, A, B = case_model(name)
        c, Hq, _ = case_solver(name)
        P, Gc = markov(A, B, n, H, s["hold"])
        for b in range(1, nb, 2):
            rt = adjust(window(ref[b], ROW0 if s["traj"] else 0, H), x[b])
            zs = -np.linalg.solve(Hq, gradient(c, P @ kr.lift(x[b], C, gamma), Gc, rt, DT, H)[0]).reshape(M, r)
            U[b] = zs + 1e-4 * (U[b] - zs)
    y = rng.uniform(-0.05, 0.05, (nb, M, r)) if s["y"] else None
    return np.ascontiguousarray(x), np.ascontiguousarray(ref), U, y, (ROW0 if s["traj"] else 0)


def case_reference(name, dtype=np.float64, **kw):
    """step() on the case; kw overrides fields of the record (iters, tol) or gives x / U_nom / y / shift"""
    s = CASES[name]
    C, gamma, A, B = case_model(name)
    c, _, W = case_solver(name)
    x, ref, U, y, row0 = case_inputs(name)
    c = with_(c, **{k: kw.pop(k) for k in ("iters", "tol") if k in kw})
    return step(C, gamma, A, B, c, W, kw.pop("x", x), ref, kw.pop("U_nom", U), DT, s["H"], y=kw.pop("y", y), ref_row0=row0, dtype=dtype, **kw)
