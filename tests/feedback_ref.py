"""NumPy restatement of the closed-loop law of include/brov2.h (brov_rollout_feedback), for the tests.  Not collected.

A loop over t around oracle.fossen_params._Prep / _step (the pinned parameterised oracle: its private step is the whole plant
here), dtype-generic (np.float64 / np.longdouble), vectorised over the batch.  It shares no code with
bluerov2_dynamics_amd/fossen/control.py: the error, the law, the hold, the clamp and the metrics are written out again from the
header comment, with the oracle's own rotation matrices.

Besides the results, rollout() returns two margins that say whether its discontinuous branches are well-posed for the inputs:
  wrap_margin  the smallest | |att_ref - att| - pi | before wrapping over all steps (Euler models; the distance to the nearest
               odd multiple of pi), and for the quaternion model the smallest |q_e.w| (the sign of the short way round);
  sat_margin   the smallest |u_raw - limit| over channels, finite limits and ticks (u_raw: the command before the clamp).
wrap_margin_lane / sat_margin_lane [B] hold the same per trajectory, so that a sweep over many shapes can leave out the one
trajectory that sits on a branch; the two scalars are their minima."""
import dataclasses

import numpy as np

from oracle import fossen_params as fp


@dataclasses.dataclass
class Law:
    """the fields of struct brov_feedback as arrays: K [nu,12], Ki [nu,6], u_min / u_max [nu], z_max [6], hold"""
    K: np.ndarray
    Ki: np.ndarray
    u_min: np.ndarray
    u_max: np.ndarray
    z_max: np.ndarray
    hold: int = 1


def law(nu, K=None, Ki=None, u_min=-np.inf, u_max=np.inf, z_max=np.inf, hold=1):
    full = lambda v, n: np.broadcast_to(np.asarray(v, dtype=np.float64), (n,)).copy()
    return Law(np.zeros((nu, 12)) if K is None else np.array(K, dtype=np.float64).reshape(nu, 12),
               np.zeros((nu, 6)) if Ki is None else np.array(Ki, dtype=np.float64).reshape(nu, 6),
               full(u_min, nu), full(u_max, nu), full(z_max, 6), int(hold))


def to_struct(l):
    """_lib.BrovFeedback of a Law, filled field by field"""
    from bluerov2_dynamics_amd import _lib
    s = _lib.BrovFeedback()
    for i in range(l.K.shape[0]):
        for j in range(12):
            s.K[i][j] = l.K[i, j]
        for j in range(6):
            s.Ki[i][j] = l.Ki[i, j]
        s.u_min[i], s.u_max[i] = l.u_min[i], l.u_max[i]
    for j in range(6):
        s.z_max[j] = l.z_max[j]
    s.hold = l.hold
    return s


def _pi(dtype):
    return np.arccos(dtype(-1))


def error(model, x, r, dtype=np.float64):
    """(e [B,12], margin): the tracking error of states x [B,nx] against reference rows r [B,nx]"""
    e, lanes = error_lanes(model, x, r, dtype)
    return e, (float(np.min(lanes)) if lanes.size else np.inf)


def error_lanes(model, x, r, dtype=np.float64):
    """(e [B,12], margin [B]): error() with the wrap margin of every row"""
    x, r = np.asarray(x, dtype=dtype), np.asarray(r, dtype=dtype)
    nx = fp.NX[model]
    e = np.zeros((x.shape[0], 12), dtype=dtype)
    if model == fp.WRENCH_QUAT:
        R = fp._quat_R(x[:, 3:7])
        qw, qx, qy, qz = (x[:, 3 + i] for i in range(4))
        rw, rx, ry, rz = (r[:, 3 + i] for i in range(4))
        # conj(q) (x) q_ref, Hamilton product with conj(q) = (qw, -qx, -qy, -qz)
        we = qw * rw + qx * rx + qy * ry + qz * rz
        ve = np.stack([qw * rx - qx * rw - qy * rz + qz * ry,
                       qw * ry + qx * rz - qy * rw - qz * rx,
                       qw * rz - qx * ry + qy * rx - qz * rw], -1)
        s = np.where(we >= 0, dtype(1), dtype(-1))
        e[:, 3:6] = dtype(2) * s[:, None] * ve
        margin = np.abs(we)
    else:
        R = fp._rotation(x[:, 3], x[:, 4], x[:, 5])
        d = r[:, 3:6] - x[:, 3:6]
        two_pi = dtype(2) * _pi(dtype)
        e[:, 3:6] = d - two_pi * np.rint(d / two_pi)
        margin = np.min(np.abs(np.mod(np.abs(d), two_pi) - _pi(dtype)), axis=1)
    dp = r[:, 0:3] - x[:, 0:3]
    for i in range(3):
        e[:, i] = R[:, 0, i] * dp[:, 0] + R[:, 1, i] * dp[:, 1] + R[:, 2, i] * dp[:, 2]
    e[:, 6:12] = r[:, nx - 6:] - x[:, nx - 6:]
    return e, margin


def rollout(model, integ, lag_mode, v, l, x0, ref, dt, T=None, u_ff=None, lag=None, z=None, sub=1, dtype=np.float64):
    """x0 [B,nx], ref [B,rows,nx] (rows 1 or T), u_ff [B,T,nu] | None, lag [B,8,3] | None, z [B,6] | None ->
    dict(traj [B,T//sub+1,nx], xT, lag, z, u [B,T,nu], metrics [B,4], wrap_margin, sat_margin, wrap_margin_lane [B], sat_margin_lane [B])"""
    c = fp._Prep(v, dt, dtype)
    nu = fp.NU[model]
    ref = np.asarray(ref, dtype=dtype)
    B, rows = ref.shape[0], ref.shape[1]
    T = rows if T is None else T
    assert rows in (1, T)
    x, _, lag = fp._inputs(model, x0, np.zeros((B, nu)), lag, dtype)
    z = np.zeros((B, 6), dtype=dtype) if z is None else np.array(z, dtype=dtype).reshape(B, 6)
    K, Ki = l.K.astype(dtype), l.Ki.astype(dtype)
    lo, hi, zm = l.u_min.astype(dtype), l.u_max.astype(dtype), l.z_max.astype(dtype)
    h = dtype(dt)
    traj, us = [x.copy()], []
    metrics = np.zeros((B, 4), dtype=dtype)
    wrap_margin = sat_margin = np.inf
    wrap_lane, sat_lane = np.full(B, np.inf, dtype=dtype), np.full(B, np.inf, dtype=dtype)
    u = np.zeros((B, nu), dtype=dtype)
    for t in range(T):
        e, ml = error_lanes(model, x, ref[:, t if rows > 1 else 0], dtype)
        wrap_lane = np.minimum(wrap_lane, ml)
        wrap_margin = min(wrap_margin, float(np.min(ml)) if ml.size else np.inf)
        if t % l.hold == 0:
            raw = np.zeros((B, nu), dtype=dtype) if u_ff is None else np.asarray(u_ff, dtype=dtype)[:, t].copy()
            for j in range(12):
                raw = raw + K[:, j] * e[:, j, None]
            for j in range(6):
                raw = raw + Ki[:, j] * z[:, j, None]
            for lim in (lo, hi):
                fin = np.isfinite(lim)
                if fin.any():
                    sat_margin = min(sat_margin, float(np.min(np.abs(raw[:, fin] - lim[fin]))))
                    sat_lane = np.minimum(sat_lane, np.min(np.abs(raw[:, fin] - lim[fin]), axis=1))
            u = np.minimum(np.maximum(raw, lo), hi)
            z = np.minimum(np.maximum(z + (dtype(l.hold) * h) * e[:, 0:6], -zm), zm)
        metrics[:, 0] += h * np.sum(e[:, 0:3] ** 2, axis=1)
        metrics[:, 1] += h * np.sum(e[:, 3:6] ** 2, axis=1)
        metrics[:, 2] += h * np.sum(u ** 2, axis=1)
        metrics[:, 3] += np.any((u == lo) | (u == hi), axis=1)
        us.append(u.copy())
        x, lag = fp._step(c, model, integ, lag_mode, dt, x, u, lag)
        if (t + 1) % sub == 0:
            traj.append(x.copy())
    return dict(traj=np.stack(traj, axis=1), xT=x, lag=lag, z=z, u=np.stack(us, axis=1) if us else np.zeros((B, 0, nu), dtype=dtype),
                metrics=metrics, wrap_margin=wrap_margin, sat_margin=sat_margin, wrap_margin_lane=wrap_lane, sat_margin_lane=sat_lane)
