"""NumPy restatement of the model-predictive update with an EDMDc planning model (include/brov2.h: edmdc_mppi_step), for the tests.
Not collected.

The predicted states come from the ITERATED recursion z <- A z + B v of KoopmanEDMDc.simulate with oracle.edmdc_numpy's RBF matrix
(the expanded form) -- never from the linear form the kernel and engine.koopman_markov use --, dtype-generic (np.float64 /
np.longdouble) and vectorised over the samples.  The commands, the normals and the soft-min are mppi_ref's (commands / normals /
softmin), the tracking error is feedback_ref.error with its wrap margin: n = 12 takes the Euler-angle error, n = 13 the quaternion
error."""
import numpy as np

import feedback_ref as fr
import mppi_ref as mr
from oracle import edmdc_numpy as en
from oracle import fossen_params as fp

ERROR_MODEL = {12: fp.WRENCH_EULER, 13: fp.WRENCH_QUAT}      # whose tracking error a state of n entries takes


def lift(x, C, gamma, dtype=np.float64):
    """phi(x) = [x, rbf(x)] of one state, in `dtype`"""
    x = np.asarray(x, dtype=dtype)
    if C is None or len(C) == 0:
        return x.copy()
    return np.hstack([x, en.rbf_mat(x[None, :], np.asarray(C, dtype=dtype), dtype(gamma)).ravel()])


def predict(C, gamma, A, B, x, cmd, H, hold, dtype=np.float64):
    """pred [K,H+1,n]: the states of K command sequences cmd [K,M,r] from one state x [n]; step t applies knot t // hold"""
    A, B, cmd = np.asarray(A, dtype=dtype), np.asarray(B, dtype=dtype), np.asarray(cmd, dtype=dtype)
    n, K = len(x), cmd.shape[0]
    Z = np.repeat(lift(x, C, gamma, dtype)[None], K, axis=0)
    out = np.zeros((K, H + 1, n), dtype=dtype)
    out[:, 0] = Z[:, :n]
    for t in range(H):
        Z = Z @ A.T + cmd[:, t // hold] @ B.T
        out[:, t + 1] = Z[:, :n]
    return out


def costs(c, pred, ref_rows, U, cmd, delta, dt, H, dtype=np.float64):
    """(S [K], wrap margin) of one problem from its predicted states pred [K,H+1,n], reference rows [H+1,n], knots U [M,r] and
    commands cmd / delta [K,M,r]: mppi_ref.costs with the plant replaced by the prediction"""
    S, lanes = costs_lanes(c, pred, ref_rows, U, cmd, delta, dt, H, dtype)
    return S, min(np.inf, float(np.min(lanes)))


def costs_lanes(c, pred, ref_rows, U, cmd, delta, dt, H, dtype=np.float64):
    """costs() with the wrap margin of every sample [K]"""
    K, n = pred.shape[0], pred.shape[2]
    model = ERROR_MODEL[n]
    q, qf, r, sg = c.q.astype(dtype), c.qf.astype(dtype), c.r.astype(dtype), c.sigma.astype(dtype)
    h = dtype(dt)
    S = np.zeros(K, dtype=dtype)
    margin = np.full(K, np.inf, dtype=dtype)
    ref_rows = np.asarray(ref_rows, dtype=dtype)
    for t in range(H):
        e, m = fr.error_lanes(model, pred[:, t], np.repeat(ref_rows[t][None], K, axis=0), dtype)
        margin = np.minimum(margin, m)
        u = cmd[:, t // c.hold]
        S = S + h * (np.sum(q * e * e, axis=1) + np.sum(r * u * u, axis=1))
    e, m = fr.error_lanes(model, pred[:, H], np.repeat(ref_rows[H][None], K, axis=0), dtype)
    margin = np.minimum(margin, m)
    S = S + np.sum(qf * e * e, axis=1)
    on = c.sigma > 0
    Ud = np.asarray(U, dtype=dtype)
    imp = np.sum((Ud[None, :, on] * delta[:, :, on]) / (sg[on] * sg[on]), axis=(1, 2))
    return S + dtype(c.gamma) * imp, margin


def step(C, gamma, A, B, c, x, ref, U_nom, dt, K, H, seed=0, eps=None, ref_row0=0, shift=False, dtype=np.float64):
    """One update for nb problems: x [nb,n], ref [nb,rows,n], U_nom [nb,M,r], eps [nb,K,M,r] | None -> dict(cost [nb,K], pred
    [nb,K,H+1,n], U_new, U_nom (after the shift), u_apply [nb,hold,r], info [nb,4], xi, v, delta [nb,K,M,r], w [nb,K], wrap_margin, wrap_margin_lane [nb,K])"""
    x, ref, U_nom = np.asarray(x), np.asarray(ref), np.asarray(U_nom)
    nb, M, r = U_nom.shape
    assert M == mr.knots(H, c.hold) and r == np.shape(B)[1]
    rows = ref.shape[1]
    assert (rows == 1 and ref_row0 == 0) or (ref_row0 >= 0 and ref_row0 + H <= rows - 1)
    xi = mr.normals(seed, nb, K, M, r) if eps is None else np.asarray(eps, dtype=np.float64)
    out = dict(cost=[], pred=[], U_new=[], U_nom=[], u_apply=[], info=[], v=[], delta=[], w=[], wrap_margin_lane=[], xi=xi, wrap_margin=np.inf)
    lo, hi = c.u_min.astype(dtype), c.u_max.astype(dtype)
    for b in range(nb):
        v, d = mr.commands(c, U_nom[b], xi[b], dtype)
        rr = np.repeat(ref[b, :1], H + 1, axis=0) if rows == 1 else ref[b, ref_row0:ref_row0 + H + 1]
        pred = predict(C, gamma, A, B, x[b], v, H, c.hold, dtype)
        S, lanes = costs_lanes(c, pred, rr, U_nom[b], v, d, dt, H, dtype)
        margin = min(np.inf, float(np.min(lanes)))
        U_new, info, w = mr.softmin(c, S, d, U_nom[b], dtype)
        if w is None:               # no finite sample: the plan stays, the command is the clamped first knot
            Un = np.asarray(U_nom[b], dtype=dtype).copy()
            first = np.minimum(np.maximum(Un[0], lo), hi)
            w = np.zeros(K, dtype=dtype)
        else:
            Un = np.concatenate([U_new[1:], U_new[-1:]], axis=0) if shift else U_new
            first = U_new[0]
        out["wrap_margin"] = min(out["wrap_margin"], margin)
        for key, val in (("cost", S), ("pred", pred), ("U_new", U_new), ("U_nom", Un), ("u_apply", np.repeat(first[None], c.hold, axis=0)),
                         ("info", info), ("v", v), ("delta", d), ("w", w), ("wrap_margin_lane", lanes)):
            out[key].append(val)
    return {k: (np.stack(val) if isinstance(val, list) else val) for k, val in out.items()}
