"""NumPy restatement of the PINc inference path (training/train_tank_brov2_full_comparison.py:601-721, 838-890): PINcNet.forward,
simulate_pinc for a batch and multistep_rmse_endpoint_pinc's per-window errors.  TEST INFRASTRUCTURE ONLY (oracle/__init__.py).

fp64 by default (the fp32 parameters widened exactly); fp32=True runs the network in fp32 instead, the precision the reference and
the kernels run it in, so that a test can measure how far fp32 arithmetic itself lands from fp64 on the same inputs.  The thruster
map between network steps is the fp64 C oracle (oracle/fossen_c.py).  Pinned by tests/golden/pinc_kat.npz, pinc_rand_kat.npz and
cfg5_pinc.npz (tests/test_pinc_cpu.py)."""
import numpy as np

from . import fossen_c

N_IN, N_OUT = 14, 9
U4 = [0, 1, 2, 5]                  # thrusters_to_body_wrenches: tau[0, 1, 2, 5]


def _softplus(y, thr):
    """F.softplus (beta 1, threshold 20): y above the threshold, log1p(exp(y)) below."""
    return np.where(y > thr, y, np.log1p(np.exp(np.minimum(y, thr))))


def forward(sd, z, fp32=False):
    """PINcNet.forward: z [B,14] -> x_next [B,9] (float64, or float32 with fp32=True).  sd: the 22 state-dict arrays."""
    f = np.float32 if fp32 else np.float64
    z = np.asarray(z, dtype=f).reshape(-1, N_IN)
    h = z
    for idx in (0, 3, 6, 9):
        a = h @ np.asarray(sd[f"net.{idx}.weight"], f).T + np.asarray(sd[f"net.{idx}.bias"], f)
        beta = f(sd[f"net.{idx + 1}.beta"])
        s = _softplus(beta * a, f(20)) / (beta + f(1e-12))                     # AdaptiveSoftplus
        mean = s.mean(axis=1, keepdims=True, dtype=f)
        d = s - mean
        var = (d * d).mean(axis=1, keepdims=True, dtype=f)                      # LayerNorm: biased variance, eps 1e-5
        h = d / np.sqrt(var + f(1e-5)) * np.asarray(sd[f"net.{idx + 2}.weight"], f) + np.asarray(sd[f"net.{idx + 2}.bias"], f)
    dx = h @ np.asarray(sd["net.12.weight"], f).T + np.asarray(sd["net.12.bias"], f)
    c, s = z[:, 3], z[:, 4]
    out = z[:, :9] + dx
    out[:, 0] = c * dx[:, 0] - s * dx[:, 1] + z[:, 0]                          # x/y residual rotated body -> world by the input yaw
    out[:, 1] = s * dx[:, 0] + c * dx[:, 1] + z[:, 1]
    nrm = np.maximum(np.sqrt(out[:, 3] * out[:, 3] + out[:, 4] * out[:, 4]), f(1e-6))
    out[:, 3] /= nrm
    out[:, 4] /= nrm
    return out


def to9(x12):
    """dataset12_to_9 for rows [B,12] (fp64)."""
    x12 = np.asarray(x12, dtype=np.float64)
    return np.stack([x12[:, 0], x12[:, 1], x12[:, 2], np.cos(x12[:, 5]), np.sin(x12[:, 5]),
                     x12[:, 6], x12[:, 7], x12[:, 8], x12[:, 11]], axis=1)


def to12(x9):
    """state9_to_12 for rows [B,9] (fp64): phi, theta, p, q = 0, psi = atan2(sin, cos)."""
    x9 = np.asarray(x9, dtype=np.float64)
    out = np.zeros((x9.shape[0], 12))
    out[:, 0:3] = x9[:, 0:3]
    out[:, 5] = np.arctan2(x9[:, 4], x9[:, 3])
    out[:, 6:9] = x9[:, 5:8]
    out[:, 11] = x9[:, 8]
    return out


def rollout(sd, x0, U, dt, lag=None, stride=1, store=True, fp32=False):
    """simulate_pinc for a batch: x0 [B,12], U [B,T,8], lag [B,8,3] (None = fresh vehicles) -> dict(traj [B,T//stride+1,12] (None
    with store=False), xT [B,12], lag [B,8,3] after the last step).  Per step: the thruster map with each row's own lag, u4 =
    tau[0, 1, 2, 5], z = [x9, u4, dt] rounded to fp32 (the reference's .float()), x9 <- forward(z)."""
    U = np.asarray(U, dtype=np.float64)
    B, T = U.shape[0], U.shape[1]
    x12 = np.asarray(x0, dtype=np.float64).reshape(B, 12).copy()
    lag = np.zeros((B, 8, 3)) if lag is None else np.asarray(lag, dtype=np.float64).reshape(B, 8, 3).copy()
    traj = np.empty((B, T // stride + 1, 12)) if store else None
    if store:
        traj[:, 0] = x12
    x9 = to9(x12)
    for t in range(T):
        tau, lag = fossen_c.thruster_forces(U[:, t], dt, lag=lag)
        z = np.hstack([x9, tau[:, U4], np.full((B, 1), dt)]).astype(np.float32)
        x9 = forward(sd, z, fp32=fp32)
        if (store and (t + 1) % stride == 0) or t + 1 == T:
            x12 = to12(x9)
            if store and (t + 1) % stride == 0:
                traj[:, (t + 1) // stride] = x12
    return dict(traj=traj, xT=x12, lag=lag)


def _lag_step(x, F, Ad, Bd):
    """One sample of the eight thruster-lag filters, x [8,3] <- Ad x + Bd F, in the operation order of the C oracle's lag_step
    (bit for bit: both round every product and sum)."""
    return ((x[:, 0, None] * Ad[:, 0] + x[:, 1, None] * Ad[:, 1]) + x[:, 2, None] * Ad[:, 2]) + F[:, None] * Bd


def thruster_stream(U, dt, lag=None):
    """One map vehicle fed the commands U [n,8] in order (thrusters_to_body_wrenches once per row) -> (u4 [n,4], lag [8,3] after)."""
    U = np.asarray(U, dtype=np.float64).reshape(-1, 8)
    Ad, Bd = fossen_c.discretise_lag(dt)
    cst = fossen_c.constants()
    Cc = np.array([0.0, 5.992, 3.317])                  # ThrusterLag C (fossen/BlueROV2.py:476-480)
    Fc = fossen_c.thrust_poly(U)
    x = np.zeros((8, 3)) if lag is None else np.asarray(lag, dtype=np.float64).reshape(8, 3).copy()
    F = np.empty((len(U), 8))
    for r in range(len(U)):
        x = _lag_step(x, Fc[r], Ad, Bd)
        F[r] = x @ Cc
    return F @ cst["alloc"][U4].T, x


def lag_starts(U, H, dt, nwin, lag=None):
    """The map vehicle's lag at the start of each of nwin windows of H samples (window k reads U[k .. k+H-1] and window k+1 starts
    where window k's H samples left the vehicle), by the literal sequential map -> (starts [nwin,8,3], lag [8,3] after the last)."""
    U = np.asarray(U, dtype=np.float64).reshape(-1, 8)
    Ad, Bd = fossen_c.discretise_lag(dt)
    Fc = fossen_c.thrust_poly(U[:nwin + H - 1]) if nwin and H else np.zeros((0, 8))
    x = np.zeros((8, 3)) if lag is None else np.asarray(lag, dtype=np.float64).reshape(8, 3).copy()
    starts = np.empty((nwin, 8, 3))
    for k in range(nwin):
        starts[k] = x
        for t in range(H):
            x = _lag_step(x, Fc[k + t], Ad, Bd)
    return starts, x


def window_endpoint_se(sd, X, U, H, dt, lag=None, carry_lag=True, windows=None, fp32=False):
    """multistep_rmse_endpoint_pinc's terms: window k = 0..N-H-1 runs H steps from X[k] under U[k .. k+H-1]; per_window[k] =
    |x_end - X[k+H]|^2 (12-D).  lag [8,3]: the map vehicle's lag before the first window (None = zero); carry_lag: window k starts
    from the lag window k-1 left (the reference), else every window starts from `lag`.  windows: indices of the windows to evaluate
    (None = all), each from its true start.  -> dict(per_window [len(windows)], se (their sum), x_end [len(windows),12], lag [8,3]
    after the last window (carry_lag) or the given one, lag_starts [nwin,8,3] (carry_lag) or None)."""
    X = np.asarray(X, dtype=np.float64).reshape(-1, 12)
    U = np.asarray(U, dtype=np.float64).reshape(-1, 8)
    N, H = X.shape[0], int(H)
    nwin = max(N - H, 0)
    lag0 = np.zeros((8, 3)) if lag is None else np.asarray(lag, dtype=np.float64).reshape(8, 3)
    ks = np.arange(nwin) if windows is None else np.asarray(windows, dtype=np.int64)
    if carry_lag:
        starts, lag_end = lag_starts(U, H, dt, nwin, lag0)
        l0 = starts[ks]
    else:
        starts, lag_end = None, lag0.copy()
        l0 = np.broadcast_to(lag0, (len(ks), 8, 3))
    Uw = U[ks[:, None] + np.arange(H)[None, :]] if H else np.zeros((len(ks), 0, 8))
    r = rollout(sd, X[ks], Uw, dt, lag=l0, store=False, fp32=fp32)
    e = r["xT"] - X[ks + H]
    per = np.sum(e * e, axis=1)
    return dict(per_window=per, se=float(per.sum()), x_end=r["xT"], lag=lag_end, lag_starts=starts)
