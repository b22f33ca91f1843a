"""PINc residual network inference on the engine -- drop-in for the reference's simulate_pinc / multistep_rmse_endpoint_pinc
(training/train_tank_brov2_full_comparison.py:838-890) with the architecture of its shipped checkpoint (PINcNet, :648-721:
14 -> 64 x 4 -> 9, fp32) -- and for its make_pinc_dataset / train_pinc (:724-835).  The arithmetic runs in csrc/pinc.hip
(inference) and csrc/pinc_train.hip (loss, gradient, clip + AdamW).

    w = PINcWeights("pinc_best.pt")            # or a .npz of the state-dict arrays, a dict, PINcNet itself
    net = PINc(w)
    net.forward(z)                             # PINcNet.forward: z [B,14] -> x_next [B,9] (fp32)
    net.rollout(x0, U, dt, lag=None)           # simulate_pinc for a batch -> dict(traj, xT, lag)
    net.multistep_rmse_endpoint(X, U, H, dt, vehicle=rov)

    simulate_pinc(x0_12, U_seq_8, dt, model, old_model_for_map)             # the reference's signatures; `model` is a PINcNet,
    multistep_rmse_endpoint_pinc(X, U, H, dt, model, old_model_for_map)     # a state dict or PINcWeights

    z, y, U4 = make_pinc_dataset(X12, U8, dt, rov)                           # the reference's arrays (fp64)
    w = train_pinc(z, y, U4, dt, epochs=100, seed=0)                         # -> PINcWeights (w.save("pinc.npz"))
    tr = PINcTrainer(PINcWeights.init(0)); tr.epoch(Z, Y, U4, perm); tr.weights()

The map vehicle (`old_model_for_map`, this package's fossen.BlueROV2) is stateful as in the reference: its thruster lag is read
before a call and written back after it, so it carries from window to window and from call to call.  This module does not import
torch; only loading a .pt checkpoint does (lazily)."""
import ctypes
import os

import numpy as np

from . import _lib, engine

__all__ = ["PINcWeights", "PINc", "PINcTrainer", "simulate_pinc", "multistep_rmse_endpoint_pinc", "make_pinc_dataset", "train_pinc",
           "NPARAMS", "KEYS"]

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

    @classmethod
    def from_blob(cls, blob):
        """The weights of a packed blob (NPARAMS fp32 values in state-dict order)."""
        blob = np.asarray(blob, dtype=np.float32).ravel()
        if blob.size != NPARAMS:
            raise ValueError(f"PINc weights: a blob has {NPARAMS} values, got {blob.size}")
        sd, o = {}, 0
        for k, shape in SHAPES.items():
            n = int(np.prod(shape, dtype=np.int64))
            sd[k] = blob[o:o + n].reshape(shape)
            o += n
        return cls(sd)

    @classmethod
    def init(cls, seed=0):
        """A freshly initialised network with the distributions of torch's defaults for PINcNet(): Linear weights and biases
        U(-1/sqrt(fan_in), 1/sqrt(fan_in)), beta = 1, LayerNorm weight 1 and bias 0.  Equal to torch in distribution, not in
        bits (the generator is numpy's, seeded with `seed`)."""
        rng = np.random.default_rng(seed)
        sd = {}
        for k, shape in SHAPES.items():
            idx = int(k.split(".")[1])
            if idx in (0, 3, 6, 9, 12):                                # Linear
                bound = 1.0 / np.sqrt(N_IN if idx == 0 else HIDDEN)
                sd[k] = rng.uniform(-bound, bound, size=shape).astype(np.float32)
            elif k.endswith("beta"):
                sd[k] = np.float32(1.0)
            else:                                                      # LayerNorm
                sd[k] = (np.ones if k.endswith("weight") else np.zeros)(shape, dtype=np.float32)
        return cls(sd)

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


# ------------------------------------------------------------------------------------------ training
def _to9(X12):
    """dataset12_to_9 for rows [N,12] (fp64)."""
    X12 = _lib.as_f64(X12).reshape(-1, 12)
    return np.stack([X12[:, 0], X12[:, 1], X12[:, 2], np.cos(X12[:, 5]), np.sin(X12[:, 5]), X12[:, 6], X12[:, 7], X12[:, 8], X12[:, 11]],
                    axis=1)


def make_pinc_dataset(X12, U8, dt, old6=None):
    """(x9_k, u4_k, dt) -> x9_{k+1} pairs: z_in [N-1,14], y [N-1,9], U4 [N,4] (fp64, the reference's shapes).  old6: the map vehicle
    (this package's fossen.BlueROV2); its thruster lag advances by N samples, as in the reference.  None = a fresh vehicle."""
    X9 = _to9(X12)
    U8 = _lib.as_f64(U8).reshape(-1, 8)
    if old6 is None:
        tau, _ = engine.thruster_stream(U8, dt)
    else:
        old6._sync_params()
        tau, lag = engine.thruster_stream(U8, dt, lag=old6._lag, ctx=old6._ctx)
        old6._lag[...] = lag
    U4 = np.ascontiguousarray(tau[:, [0, 1, 2, 5]])
    xk = X9[:-1]
    z_in = np.hstack([xk, U4[:-1], np.full((len(xk), 1), float(dt))])
    return z_in, X9[1:], U4


class PINcTrainer:
    """train_pinc's loop body on one device context: mse + 0.5 physics_loss (a value only) + rollout_loss, clip_grad_norm_(max_norm),
    torch.optim.AdamW at its defaults.  A ctx holds one training session at a time; it does not touch the inference weights a PINc
    object put on the same ctx.  A second PINcTrainer on the same ctx takes the session over: the first one then raises
    RuntimeError on use and its close() leaves the new session alone.  Usable as a context manager.  Loss rows are (mse, physics mean square, rollout); the reference's loss is l[0] + 0.5 l[1] + l[2]."""

    def __init__(self, weights, ctx=None, lr=3e-3, batch=256, rollout_steps=10, use_physics=True, use_rollout=True, betas=(0.9, 0.999),
                 eps=1e-8, weight_decay=0.01, max_norm=5.0):
        self.ctx = ctx or _lib.default_context()
        w = weights if isinstance(weights, PINcWeights) else PINcWeights(weights)
        if int(batch) < 1:
            raise ValueError("PINcTrainer: batch must be >= 1")
        if not 0 <= int(rollout_steps) <= 16:
            raise ValueError("PINcTrainer: rollout_steps must be in 0..16")
        self.hyper = _lib.PincHyper(float(lr), float(betas[0]), float(betas[1]), float(eps), float(weight_decay), float(max_norm),
                                    int(batch), int(rollout_steps), int(bool(use_physics)), int(bool(use_rollout)))
        self.ctx.use_null_stream()
        blob = np.ascontiguousarray(w.blob, dtype=np.float32)
        self.ctx.check(self.ctx.lib.brov_pinc_train_begin(self.ctx.h, blob.ctypes.data, int(blob.size), ctypes.byref(self.hyper)),
                       "brov_pinc_train_begin")
        self._open = True
        self.ctx._pinc_trainer = self              # the ctx's one session belongs to this object now

    def _own(self):
        """The ctx with this object's session current on it; RuntimeError when the session was closed or taken over."""
        if not self._open or getattr(self.ctx, "_pinc_trainer", None) is not self:
            raise RuntimeError("PINcTrainer: this trainer's session is closed or was replaced by another PINcTrainer on the same context")
        self.ctx.use_null_stream()
        return self.ctx

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _k(self, B):
        return min(self.hyper.rollout_steps, B - 1) if self.hyper.use_rollout else 0

    def _get(self):
        blob, m, v = (np.empty(NPARAMS, dtype=np.float32) for _ in range(3))
        step = ctypes.c_int64(0)
        self._own()
        self.ctx.check(self.ctx.lib.brov_pinc_train_get(self.ctx.h, blob.ctypes.data, m.ctypes.data, v.ctypes.data, ctypes.byref(step)),
                       "brov_pinc_train_get")
        return blob, m, v, int(step.value)

    def loss_and_grad(self, z, y, u4):
        """The loss terms [3] and the unclipped gradient [NPARAMS] (blob order) of one minibatch z [B,14], y [B,9], u4 [B,4] at the
        session's current weights; nothing is updated."""
        ctx = self._own()
        z = np.ascontiguousarray(z, dtype=np.float32).reshape(-1, N_IN)
        B = z.shape[0]
        y = np.ascontiguousarray(y, dtype=np.float32).reshape(B, N_OUT)
        u4 = np.ascontiguousarray(u4, dtype=np.float32).reshape(B, 4)
        arrs = [engine.DevArray.from_host(ctx, a, np.float32) for a in (self._get()[0], z, y, u4)]
        arrs += [engine.DevArray(ctx, (NPARAMS,), np.float32), engine.DevArray(ctx, (3,), np.float32)]
        try:
            engine.pinc_loss_grad_dev(arrs[0], arrs[1], arrs[2], arrs[3], self._k(B), self.hyper.use_physics, arrs[4], arrs[5], ctx=ctx)
            return arrs[5].numpy(), arrs[4].numpy()
        finally:
            for a in arrs:
                a.free()

    def epoch(self, Z, Y, U4, perm):
        """One pass over Z [N,14], Y [N,9], U4 [N,4] in the order `perm` (a permutation of range(N)), in minibatches of `batch` rows
        (the last one short).  Returns the loss terms of every iteration, [ceil(N / batch), 3] float32."""
        self._own()
        Z = np.ascontiguousarray(Z, dtype=np.float32).reshape(-1, N_IN)
        N = Z.shape[0]
        perm = np.ascontiguousarray(perm, dtype=np.int32).ravel()
        if perm.size != N or N < 1 or not np.array_equal(np.sort(perm), np.arange(N, dtype=np.int32)):
            raise ValueError("PINcTrainer.epoch: perm must be a permutation of range(len(Z))")
        return self._epoch_dev(self.upload(Z, Y, U4), perm, free=True)

    def upload(self, Z, Y, U4):
        """The dataset on the device (fp32), for epochs that reuse it (`epoch_on`)."""
        ctx = self._own()
        Z = np.ascontiguousarray(Z, dtype=np.float32).reshape(-1, N_IN)
        N = Z.shape[0]
        Y = np.ascontiguousarray(Y, dtype=np.float32).reshape(N, N_OUT)
        U4 = np.ascontiguousarray(U4, dtype=np.float32).reshape(N, 4)
        out = []
        try:
            for a in (Z, Y, U4):
                out.append(engine.DevArray.from_host(ctx, a, np.float32))
        except Exception:
            for a in out:
                a.free()
            raise
        return tuple(out)

    def epoch_on(self, data, perm):
        """`epoch` on a dataset from `upload`."""
        perm = np.ascontiguousarray(perm, dtype=np.int32).ravel()
        N = data[0].shape[0]
        if perm.size != N or not np.array_equal(np.sort(perm), np.arange(N, dtype=np.int32)):
            raise ValueError("PINcTrainer.epoch_on: perm must be a permutation of range(len(Z))")
        return self._epoch_dev(data, perm, free=False)

    def _epoch_dev(self, data, perm, free):
        ctx = self._own()
        N = data[0].shape[0]
        iters = -(-N // self.hyper.batch)
        dperm = dlog = None
        try:
            dperm = engine.DevArray.from_host(ctx, perm, np.int32)
            dlog = engine.DevArray(ctx, (iters, 3), np.float32)
            ctx.check(ctx.lib.brov_pinc_train_epoch_dev(ctx.h, N, data[0].ptr, data[1].ptr, data[2].ptr, dperm.ptr, dlog.ptr),
                      "brov_pinc_train_epoch_dev")
            return dlog.numpy()                    # a copy on the ctx stream: it waits for the epoch
        finally:
            for a in (dperm, dlog):
                if a is not None:
                    a.free()
            if free:
                for a in data:
                    a.free()

    def weights(self):
        return PINcWeights.from_blob(self._get()[0])

    def state(self):
        """dict(blob, m, v, step): everything a resumed run needs (load_state)."""
        blob, m, v, step = self._get()
        return dict(blob=blob, m=m, v=v, step=step)

    def load_state(self, st):
        ctx = self._own()
        blob, m, v = (np.ascontiguousarray(st[k], dtype=np.float32).ravel() for k in ("blob", "m", "v"))
        if not (blob.size == m.size == v.size == NPARAMS):
            raise ValueError(f"PINcTrainer.load_state: blob, m and v have {NPARAMS} values each")
        ctx.check(ctx.lib.brov_pinc_train_begin(ctx.h, blob.ctypes.data, NPARAMS, ctypes.byref(self.hyper)), "brov_pinc_train_begin")
        ctx.check(ctx.lib.brov_pinc_train_set_state(ctx.h, m.ctypes.data, v.ctypes.data, int(st["step"])), "brov_pinc_train_set_state")

    def close(self):
        """Ends this trainer's session (idempotent; a session another trainer took over is left alone)."""
        if not getattr(self, "_open", False):
            return
        self._open = False
        if getattr(self.ctx, "_pinc_trainer", None) is self:
            self.ctx._pinc_trainer = None
            if self.ctx.h:
                self.ctx.lib.brov_pinc_train_end(self.ctx.h)


def train_pinc(z_train, y_train, u4_train, dt, device=None, epochs=100, batch=256, lr=3e-3, use_physics=True, use_rollout=True,
               rollout_steps=10, *, init=None, seed=0, perms=None, verbose=True):
    """The reference's train_pinc on the engine -> PINcWeights (.state_dict(), .save(); every inference entry point takes it).
    z_train [N,14], y_train [N,9], u4_train [N+1,4] as make_pinc_dataset returns them (u4_train[:-1] is aligned with the rows, as
    in the reference).  `device` is accepted and ignored; `dt` is already a column of z_train.  init: starting weights (default
    PINcWeights.init(seed)); perms: the row order of every epoch, [epochs, N] (default: drawn from numpy's default_rng(seed), a
    fresh permutation per epoch, so a run is replayable from its seed)."""
    z = np.asarray(z_train)
    y = np.asarray(y_train)
    u4 = np.asarray(u4_train)
    if z.ndim != 2 or z.shape[1] != N_IN or z.shape[0] < 1:
        raise ValueError(f"train_pinc: z_train must be [N, {N_IN}] with N >= 1, got {z.shape}")
    N = z.shape[0]
    if y.shape != (N, N_OUT):
        raise ValueError(f"train_pinc: y_train must be [{N}, {N_OUT}], got {y.shape}")
    if u4.ndim != 2 or u4.shape[1] != 4 or u4.shape[0] - 1 != N:
        raise ValueError(f"train_pinc: u4_train must be [{N + 1}, 4] (make_pinc_dataset's U4), got {u4.shape}")
    epochs = int(epochs)
    if epochs < 0 or int(batch) < 1:
        raise ValueError("train_pinc: epochs must be >= 0 and batch >= 1")
    if perms is not None:
        perms = np.asarray(perms)
        if perms.shape != (epochs, N):
            raise ValueError(f"train_pinc: perms must be [{epochs}, {N}], got {perms.shape}")
    rng = np.random.default_rng(seed)
    w0 = PINcWeights.init(seed) if init is None else (init if isinstance(init, PINcWeights) else PINcWeights(init))
    tr = PINcTrainer(w0, lr=lr, batch=batch, rollout_steps=rollout_steps, use_physics=use_physics, use_rollout=use_rollout)
    data = ()
    try:
        data = tr.upload(z, y, u4[:-1])
        for ep in range(epochs):
            perm = rng.permutation(N) if perms is None else perms[ep]
            log = tr.epoch_on(data, perm).astype(np.float64)
            if verbose and (ep + 1) % 10 == 0:
                ep_loss = float(np.sum(log[:, 0] + 0.5 * log[:, 1] + log[:, 2]))
                print(f"[PINc] epoch {ep + 1:4d}/{epochs} | loss ~ {ep_loss / len(log):.6f}")
        return tr.weights()
    finally:
        for a in data:
            a.free()
        tr.close()
