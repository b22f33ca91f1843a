"""NumPy restatement of the model-predictive update of include/brov2.h (brov_mppi_step), for the tests.  Not collected.

Built like tests/feedback_ref.py: a loop over t around oracle.fossen_params._Prep / _step (the pinned parameterised oracle is the
whole plant) and feedback_ref.error (the tracking error, pinned by tests/test_feedback_cpu.py), dtype-generic (np.float64 /
np.longdouble), a loop over the problems b and vectorised over the samples k.  It shares no code with
bluerov2_dynamics_amd/fossen/control.py or the engine: the samples, the clamp, the cost, the soft-min and the shift are written out
again from the header comment.  The noise comes from oracle.controls.uniform01_at and the Box-Muller formula of
oracle.controls.controls_ar1, as float64 values (a normal IS its float64 value; the long-double runs take the same numbers)."""
import dataclasses

import numpy as np

import feedback_ref as fr
from oracle import controls as oc
from oracle import fossen_params as fp


@dataclasses.dataclass
class Cfg:
    """the fields of struct brov_mppi as arrays: q, qf [12], r, sigma, u_min, u_max [nu], lam, gamma, hold"""
    q: np.ndarray
    qf: np.ndarray
    r: np.ndarray
    sigma: np.ndarray
    u_min: np.ndarray
    u_max: np.ndarray
    lam: float = 1.0
    gamma: float = 1.0
    hold: int = 1


def cfg(nu, q=1.0, qf=None, r=0.0, sigma=0.1, lam=1.0, gamma=None, u_min=-np.inf, u_max=np.inf, hold=1):
    full = lambda v, n: np.broadcast_to(np.asarray(v, dtype=np.float64), (n,)).copy()
    return Cfg(full(q, 12), full(q if qf is None else qf, 12), full(r, nu), full(sigma, nu), full(u_min, nu), full(u_max, nu),
               float(lam), float(lam if gamma is None else gamma), int(hold))


def to_struct(c):
    """_lib.BrovMppi of a Cfg, filled field by field"""
    from bluerov2_dynamics_amd import _lib
    s = _lib.BrovMppi()
    for i in range(12):
        s.q[i], s.qf[i] = c.q[i], c.qf[i]
    for j in range(c.r.shape[0]):
        s.r[j], s.sigma[j], s.u_min[j], s.u_max[j] = c.r[j], c.sigma[j], c.u_min[j], c.u_max[j]
    s.lam, s.gamma, s.hold = c.lam, c.gamma, c.hold
    return s


def knots(H, hold):
    return (H + hold - 1) // hold


def normals(seed, B, K, M, nu):
    """xi [B,K,M,nu] of the library's stream: counter c = ((b K + k) M + m) nu + j, second stream seed ^ 0xA5.., Box-Muller on the
    uniforms number 2c and 2c + 1 (oracle.controls.controls_ar1's formula)"""
    c = np.arange(B * K * M * nu, dtype=np.uint64).reshape(B, K, M, nu)
    s2 = (seed & 0xFFFFFFFFFFFFFFFF) ^ oc.AR1_STREAM_XOR
    u1 = oc.uniform01_at(s2, np.uint64(2) * c)
    u2 = oc.uniform01_at(s2, np.uint64(2) * c + np.uint64(1))
    return np.sqrt(-2.0 * np.log1p(-u1)) * np.cos(2.0 * np.pi * u2)


def commands(c, U, xi, dtype=np.float64):
    """(v, delta) [K,M,nu] of one problem from its knots U [M,nu] and normals xi [K,M,nu]: sample 0 and the channels with sigma = 0
    are not perturbed (their xi is never looked at); the clamp lets a NaN through"""
    U, xi = np.asarray(U, dtype=dtype), np.array(xi, dtype=dtype)
    sg, lo, hi = c.sigma.astype(dtype), c.u_min.astype(dtype), c.u_max.astype(dtype)
    xi[0] = 0
    xi[:, :, c.sigma == 0] = 0
    v = np.minimum(np.maximum(U[None] + sg * xi, lo), hi)
    return v, v - U[None]


def softmin(c, S, delta, U, dtype=np.float64):
    """(U_new [M,nu], info [4]) of one problem from its costs S [K], perturbations delta [K,M,nu] and knots U [M,nu]"""
    S, U = np.asarray(S, dtype=dtype), np.asarray(U, dtype=dtype)
    lo, hi = c.u_min.astype(dtype), c.u_max.astype(dtype)
    fin = np.isfinite(S)
    nbad = int(S.size - fin.sum())
    if not fin.any():
        return U.copy(), np.array([S[0], np.inf, 0.0, nbad], dtype=dtype), None
    beta = S[fin].min()
    w = np.zeros_like(S)
    w[fin] = np.exp(-(S[fin] - beta) / dtype(c.lam))
    eta = w.sum()
    step = np.tensordot(w[fin], np.asarray(delta, dtype=dtype)[fin], axes=(0, 0)) / eta
    U_new = np.minimum(np.maximum(U + step, lo), hi)
    return U_new, np.array([S[0], beta, eta * eta / np.sum(w * w), nbad], dtype=dtype), w


def costs(model, integ, lag_mode, v, c, x, ref_rows, U, cmd, delta, dt, H, lag=None, dtype=np.float64):
    """S [K] of one problem: vehicle v, state x [nx], reference rows ref_rows [H+1,nx] (a set-point: the row repeated), commands
    cmd / delta [K,M,nu].  Also returns the smallest wrap margin of feedback_ref.error over the steps."""
    S, lanes = costs_lanes(model, integ, lag_mode, v, c, x, ref_rows, U, cmd, delta, dt, H, lag, dtype)
    return S, min(np.inf, float(np.min(lanes)))


def costs_lanes(model, integ, lag_mode, v, c, x, ref_rows, U, cmd, delta, dt, H, lag=None, dtype=np.float64):
    """costs() with the wrap margin of every sample [K]"""
    pc = fp._Prep(v, dt, dtype)
    K = cmd.shape[0]
    nu = fp.NU[model]
    xs, _, lg = fp._inputs(model, np.repeat(np.asarray(x, dtype=dtype)[None], K, axis=0), np.zeros((K, nu)),
                           None if lag is None else np.repeat(np.asarray(lag, dtype=dtype).reshape(1, 8, 3), K, axis=0), dtype)
    q, qf, r, sg = c.q.astype(dtype), c.qf.astype(dtype), c.r.astype(dtype), c.sigma.astype(dtype)
    h = dtype(dt)
    S = np.zeros(K, dtype=dtype)
    margin = np.full(K, np.inf, dtype=dtype)
    ref_rows = np.asarray(ref_rows, dtype=dtype)
    for t in range(H):
        e, m = fr.error_lanes(model, xs, np.repeat(ref_rows[t][None], K, axis=0), dtype)
        margin = np.minimum(margin, m)
        u = cmd[:, t // c.hold]
        S = S + h * (np.sum(q * e * e, axis=1) + np.sum(r * u * u, axis=1))
        xs, lg = fp._step(pc, model, integ, lag_mode, dt, xs, u, lg)
    e, m = fr.error_lanes(model, xs, np.repeat(ref_rows[H][None], K, axis=0), dtype)
    margin = np.minimum(margin, m)
    S = S + np.sum(qf * e * e, axis=1)
    on = c.sigma > 0
    Ud = np.asarray(U, dtype=dtype)
    imp = np.sum((Ud[None, :, on] * delta[:, :, on]) / (sg[on] * sg[on]), axis=(1, 2))
    return S + dtype(c.gamma) * imp, margin


def step(model, integ, lag_mode, vehicles, c, x, ref, U_nom, dt, K, H, lag=None, seed=0, eps=None, ref_row0=0, shift=False,
         dtype=np.float64):
    """One update for B problems: vehicles (1 or B oracle Vehicles), x [B,nx], ref [B,rows,nx], U_nom [B,M,nu], lag [B,8,3] | None,
    eps [B,K,M,nu] | None -> dict(cost [B,K], U_new, U_nom (after the shift), u_apply [B,hold,nu], info [B,4], xi, v, delta
    [B,K,M,nu], w [B,K], wrap_margin, wrap_margin_lane [B,K]: the margin of every sample)"""
    x, ref, U_nom = np.asarray(x), np.asarray(ref), np.asarray(U_nom)
    B, M, nu = U_nom.shape
    assert M == knots(H, c.hold) and nu == fp.NU[model]
    rows = ref.shape[1]
    assert (rows == 1 and ref_row0 == 0) or (ref_row0 >= 0 and ref_row0 + H <= rows - 1)
    xi = normals(seed, B, K, M, nu) if eps is None else np.asarray(eps, dtype=np.float64)
    out = dict(cost=[], U_new=[], U_nom=[], u_apply=[], info=[], v=[], delta=[], w=[], wrap_margin_lane=[], xi=xi, wrap_margin=np.inf)
    lo, hi = c.u_min.astype(dtype), c.u_max.astype(dtype)
    for b in range(B):
        veh = vehicles[b if len(vehicles) > 1 else 0]
        v, d = commands(c, U_nom[b], xi[b], dtype)
        rr = np.repeat(ref[b, :1], H + 1, axis=0) if rows == 1 else ref[b, ref_row0:ref_row0 + H + 1]
        S, lanes = costs_lanes(model, integ, lag_mode, veh, c, x[b], rr, U_nom[b], v, d, dt, H, None if lag is None else lag[b], dtype)
        margin = min(np.inf, float(np.min(lanes)))
        U_new, info, w = softmin(c, S, d, U_nom[b], dtype)
        if w is None:               # no finite sample: the plan stays, the command is the clamped first knot
            Un = np.asarray(U_nom[b], dtype=dtype).copy()
            first = np.minimum(np.maximum(Un[0], lo), hi)
            w = np.zeros(K, dtype=dtype)
        else:
            Un = np.concatenate([U_new[1:], U_new[-1:]], axis=0) if shift else U_new
            first = U_new[0]
        out["wrap_margin"] = min(out["wrap_margin"], margin)
        for key, val in (("cost", S), ("U_new", U_new), ("U_nom", Un), ("u_apply", np.repeat(first[None], c.hold, axis=0)), ("info", info),
                         ("v", v), ("delta", d), ("w", w), ("wrap_margin_lane", lanes)):
            out[key].append(val)
    return {k: (np.stack(val) if isinstance(val, list) else val) for k, val in out.items()}
