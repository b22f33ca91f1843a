"""PINc residual network inference on the engine -- drop-in for the reference's simulate_pinc / multistep_rmse_endpoint_pinc
(training/train_tank_brov2_full_comparison.py:838-890) with the architecture of its shipped checkpoint (PINcNet, :648-721:
14 -> 64 x 4 -> 9, fp32).  The arithmetic runs in csrc/pinc.hip; training (train_pinc, physics_loss, rollout_loss) stays the
reference's torch code.

    w = PINcWeights("pinc_best.pt")            # or a .npz of the state-dict arrays, a dict, PINcNet itself
    net = PINc(w)
    net.forward(z)                             # PINcNet.forward: z [B,14] -> x_next [B,9] (fp32)
    net.rollout(x0, U, dt, lag=None)           # simulate_pinc for a batch -> dict(traj, xT, lag)
    net.multistep_rmse_endpoint(X, U, H, dt, vehicle=rov)

    simulate_pinc(x0_12, U_seq_8, dt, model, old_model_for_map)             # the reference's signatures; `model` is a PINcNet,
    multistep_rmse_endpoint_pinc(X, U, H, dt, model, old_model_for_map)     # a state dict or PINcWeights

The map vehicle (`old_model_for_map`, this package's fossen.BlueROV2) is stateful as in the reference: its thruster lag is read
before a call and written back after it, so it carries from window to window and from call to call.  This module does not import
torch; only loading a .pt checkpoint does (lazily)."""
import ctypes
import os

import numpy as np

from . import _lib, engine

__all__ = ["PINcWeights", "PINc", "simulate_pinc", "multistep_rmse_endpoint_pinc", "NPARAMS", "KEYS"]

HIDDEN, N_IN, N_OUT = 64, 14, 9
# state-dict keys and shapes of PINcNet(hidden_sizes=(64, 64, 64, 64)) in state-dict order (= the packed blob's order)
SHAPES = {}
for _l, _idx in enumerate((0, 3, 6, 9)):
    SHAPES[f"net.{_idx}.weight"] = (HIDDEN, N_IN if _l == 0 else HIDDEN)
    SHAPES[f"net.{_idx}.bias"] = (HIDDEN,)
    SHAPES[f"net.{_idx + 1}.beta"] = ()
    SHAPES[f"net.{_idx + 2}.weight"] = (HIDDEN,)
    SHAPES[f"net.{_idx + 2}.bias"] = (HIDDEN,)
SHAPES["net.12.weight"] = (N_OUT, HIDDEN)
SHAPES["net.12.bias"] = (N_OUT,)
KEYS = tuple(SHAPES)
NPARAMS = sum(int(np.prod(s, dtype=np.int64)) for s in SHAPES.values())      # 14 541


def _to_numpy(v):
    if hasattr(v, "detach"):                       # a torch tensor, read by duck typing (no torch import here)
        v = v.detach().cpu().numpy()
    return np.asarray(v)


def _state_dict_of(src):
    if isinstance(src, (str, os.PathLike)):
        path = os.fspath(src)
        if path.endswith(".npz"):
            with np.load(path, allow_pickle=False) as f:
                return {k: f[k] for k in f.files}
        # a torch checkpoint (the reference's models/pinc_best.pt).  Import torch before this package creates its first context:
        # importing it after the HIP runtime is initialised costs ~10 s ("One HIP runtime").
        import torch
        return torch.load(path, map_location="cpu")
    if hasattr(src, "state_dict") and callable(src.state_dict):
        return src.state_dict()
    if isinstance(src, dict):
        return src
    raise TypeError(f"PINc weights: cannot read parameters from {type(src).__name__} (want a .npz / .pt path, a dict or an object "
                    "with .state_dict())")


class PINcWeights:
    """The 22 parameter arrays of the network, validated, and their packed fp32 blob (`blob`, NPARAMS floats, state-dict order).

    src: a .npz of the state-dict arrays, a .pt checkpoint, a dict of arrays / tensors, an object with .state_dict() (the
    reference's PINcNet), or another PINcWeights.  A missing or unexpected key, or a wrong shape, raises ValueError naming it."""

    def __init__(self, src):
        if isinstance(src, PINcWeights):
            self.arrays, self.blob = dict(src.arrays), src.blob
            return
        sd = _state_dict_of(src)
        extra = [k for k in sd if k not in SHAPES]
        if extra:
            raise ValueError(f"PINc weights: unexpected key {extra[0]!r} (the network is 14 -> 64 x 4 -> 9)")
        arrays = {}
        for k, shape in SHAPES.items():
            if k not in sd:
                raise ValueError(f"PINc weights: missing key {k!r}")
            a = _to_numpy(sd[k])
            if tuple(a.shape) != shape:
                raise ValueError(f"PINc weights: {k!r} has shape {tuple(a.shape)}, expected {shape}")
            arrays[k] = np.ascontiguousarray(a, dtype=np.float32)
        self.arrays = arrays
        self.blob = np.concatenate([arrays[k].ravel() for k in KEYS]).astype(np.float32)
        assert self.blob.size == NPARAMS

    def state_dict(self):
        return dict(self.arrays)

    def save(self, path):
        np.savez(path, **self.arrays)


def set_weights(ctx, weights):
    """Upload the packed blob to `ctx` unless the ctx already holds these bytes (brov_pinc_set_weights)."""
    blob = weights.blob
    key = blob.tobytes()
    if getattr(ctx, "_pinc_blob", None) == key:
        return
    ctx.check(ctx.lib.brov_pinc_set_weights(ctx.h, blob.ctypes.data, int(blob.size)), "brov_pinc_set_weights")
    ctx._pinc_blob = key


class PINc:
    """The network on one device context (default: the process's default context)."""

    def __init__(self, weights, ctx=None):
        self.weights = weights if isinstance(weights, PINcWeights) else PINcWeights(weights)
        self.ctx = ctx or _lib.default_context()

    def _ready(self):
        ctx = self.ctx
        ctx.use_null_stream()
        set_weights(ctx, self.weights)
        return ctx

    def forward(self, z):
        """PINcNet.forward: z [B,14] (any float dtype; rounded to fp32 as the reference's .float()) -> x_next [B,9] float32."""
        z = np.ascontiguousarray(z, dtype=np.float32).reshape(-1, N_IN)
        ctx = self._ready()
        dz = engine.DevArray.from_host(ctx, z, np.float32)
        dx = engine.DevArray(ctx, (z.shape[0], N_OUT), np.float32)
        try:
            engine.pinc_forward_dev(dz, dx, ctx=ctx)
            return dx.numpy()
        finally:
            dz.free()
            dx.free()

    def rollout(self, x0, U, dt, lag=None, stride=1, store=True):
        """simulate_pinc for a batch: x0 [B,12], U [B,T,8], lag [B,8,3] (None = fresh vehicles) -> dict(traj [B,T//stride+1,12]
        (None with store=False), xT [B,12], lag [B,8,3] after the last step)."""
        ctx = self._ready()
        U = _lib.as_f64(U)
        if U.ndim == 2:
            U = U[None]
        B, T = U.shape[0], U.shape[1]
        assert U.shape[2] == 8, "U must be [B, T, 8] thruster commands"
        x0 = _lib.as_f64(x0).reshape(B, 12)
        lag_io = np.zeros((B, 8, 3)) if lag is None else _lib.as_f64(lag).reshape(B, 8, 3).copy()
        traj = np.empty((B, T // stride + 1, 12)) if store else None
        xT = np.empty((B, 12))
        ctx.check(ctx.lib.brov_pinc_rollout(ctx.h, B, T, float(dt), _lib._hptr(x0), _lib._hptr(U), _lib._hptr(lag_io), _lib._hptr(traj),
                                            int(stride), _lib._hptr(xT)), "brov_pinc_rollout")
        return dict(traj=traj, xT=xT, lag=lag_io)

    def window_endpoint_se(self, X, U, H, dt, lag=None, carry_lag=True, want_lag_starts=False):
        """Sum of the squared 12-D endpoint errors over the windows k = 0..N-H-1 (X [N,12], U [>= N-1, 8]).  lag [8,3]: the map
        vehicle's lag before the first window (None = zero).  Returns dict(se, per_window [N-H], lag [8,3] after the last window (carry_lag) or the given one,
        lag_starts [N-H,8,3] (want_lag_starts and carry_lag, else None))."""
        ctx = self._ready()
        X = _lib.as_f64(X).reshape(-1, 12)
        U = _lib.as_f64(U).reshape(-1, 8)
        N, H = X.shape[0], int(H)
        # window k reads U[k .. k+H-1], so rows up to N-2: the reference accepts len(U) == len(X) - 1
        assert U.shape[0] >= (N - 1 if H > 0 else 0), "U must be aligned with X (at least len(X) - 1 rows)"
        nwin = max(N - H, 0)
        lag_io = np.zeros((8, 3)) if lag is None else _lib.as_f64(lag).reshape(8, 3).copy()
        per = np.zeros(nwin)
        starts = np.zeros((nwin, 8, 3)) if want_lag_starts and carry_lag and nwin else None
        se = ctypes.c_double(0.0)
        ctx.check(ctx.lib.brov_pinc_window_endpoint_se(ctx.h, N, H, float(dt), _lib._hptr(X), _lib._hptr(U), int(bool(carry_lag)),
                                                       _lib._hptr(lag_io), ctypes.addressof(se), _lib._hptr(per) if nwin else None,
                                                       _lib._hptr(starts)), "brov_pinc_window_endpoint_se")
        return dict(se=se.value, per_window=per, lag=lag_io, lag_starts=starts)

    def multistep_rmse_endpoint(self, X, U, H, dt, vehicle=None, carry_lag=True):
        """multistep_rmse_endpoint_pinc: sqrt(se / (n_start * 12)); NaN when n_start <= 0 (the vehicle is then not touched).
        vehicle: the map vehicle (fossen.BlueROV2) whose lag the evaluation starts from and advances; None = a fresh one."""
        n_start = len(X) - int(H)
        if n_start <= 0:
            return float("nan")
        r = self.window_endpoint_se(X, U, H, dt, lag=None if vehicle is None else vehicle._lag, carry_lag=carry_lag)
        if vehicle is not None and carry_lag:
            vehicle._lag[...] = r["lag"]
        return float(np.sqrt(r["se"] / (n_start * 12)))


def _bound(model, vehicle):
    """A PINc on the vehicle's own context (its parameters synced, as BlueROV2.simulate does), or on the default one."""
    w = model if isinstance(model, PINcWeights) else PINcWeights(model)
    if vehicle is None:
        return PINc(w)
    vehicle._sync_params()
    return PINc(w, ctx=vehicle._ctx)


def simulate_pinc(x0_12, U_seq_8, dt, model, old_model_for_map, device=None):
    """Rollout of the PINc model from x0_12 under U_seq_8; returns the (H+1, 12) trajectory (row 0 = x0_12).
    Advances old_model_for_map's thruster lag by H samples, as the reference does.  `device` is accepted and ignored."""
    net = _bound(model, old_model_for_map)
    lag = None if old_model_for_map is None else old_model_for_map._lag[None]
    r = net.rollout(np.asarray(x0_12, float)[None], np.asarray(U_seq_8, float).reshape(1, -1, 8), dt, lag=lag)
    if old_model_for_map is not None:
        old_model_for_map._lag[...] = r["lag"][0]
    return r["traj"][0]


def multistep_rmse_endpoint_pinc(X_test, U_test, H, dt, model, old_model_for_map, device=None):
    """Endpoint RMSE of the PINc model over every window of length H (12-D, one map vehicle for all windows: the lag carries from
    window to window and into the next call).  `device` is accepted and ignored."""
    if len(X_test) - int(H) <= 0:
        return float("nan")
    return _bound(model, old_model_for_map).multistep_rmse_endpoint(X_test, U_test, H, dt, vehicle=old_model_for_map)
