#!/usr/bin/env python3
"""One epoch of PINc training at the recorded size (36 658 rows = 80 % of 45 823, batch 256, K = 10, physics on): the engine
(PINcTrainer, csrc/pinc_train.hip) against a torch restatement of the same loop body on the same ROCm device and on the CPU.

Every leg: one warm-up epoch, then `--repeats` timed epochs (default 5), host to host, fenced with brov_sync (engine) or
torch.cuda.synchronize() (torch); the engine also reports the HIP-event time of the epoch's launches.  Median, min and max per leg
go to `--out` (default profiles/pinc_train_time.json).  The data are synthetic (timing does not depend on the values).

    python tools/time_pinc_train.py [--repeats 5] [--rows 36658] [--skip-cpu]
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from bluerov2_dynamics_amd import _lib  # noqa: E402
from bluerov2_dynamics_amd.fossen.bluerov_torch import bluerov_compute  # noqa: E402
from bluerov2_dynamics_amd.pinc import PINcTrainer, PINcWeights  # noqa: E402


class Softplus(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.beta = torch.nn.Parameter(torch.tensor(1.0))

    def forward(self, x):
        return F.softplus(self.beta * x) / (self.beta + 1e-12)


class Net(torch.nn.Module):
    """14 -> 64 x 4 -> 9 residual network with the state dict of the engine's PINcWeights."""

    def __init__(self):
        super().__init__()
        layers, n = [], 14
        for _ in range(4):
            layers += [torch.nn.Linear(n, 64), Softplus(), torch.nn.LayerNorm(64)]
            n = 64
        self.net = torch.nn.Sequential(*layers, torch.nn.Linear(64, 9))

    def forward(self, z):
        dx = self.net(z)
        c, s = z[:, 3], z[:, 4]
        base = z[:, :9] + dx
        cb, sb = base[:, 3], base[:, 4]
        nrm = torch.clamp(torch.sqrt(cb * cb + sb * sb), min=1e-6)
        return torch.stack([c * dx[:, 0] - s * dx[:, 1] + z[:, 0], s * dx[:, 0] + c * dx[:, 1] + z[:, 1], base[:, 2], cb / nrm, sb / nrm,
                            base[:, 5], base[:, 6], base[:, 7], base[:, 8]], dim=1)


def torch_epoch(net, opt, Z, Y, U, perm, batch, K0):
    for r0 in range(0, len(perm), batch):
        idx = perm[r0:r0 + batch]
        z, y, u = Z[idx], Y[idx], U[idx]
        x = net(z)
        loss = F.mse_loss(x, y)
        with torch.no_grad():
            loss = loss + 0.5 * (bluerov_compute(0.0, x, u) ** 2).mean()
        K = min(K0, z.shape[0] - 1)
        if K > 0:
            xc, roll = z[0:1, :9], 0.0
            for i in range(K):
                xc = net(torch.cat([xc, z[i:i + 1, 9:13], z[0:1, 13:14]], dim=1))
                roll = roll + F.mse_loss(xc, z[i + 1:i + 2, :9])
            loss = loss + roll / K
        opt.zero_grad()
        loss.backward()
        torch.nn.utils.clip_grad_norm_(net.parameters(), 5.0)
        opt.step()
    return float(loss.item())


def stats(v):
    return dict(median=float(np.median(v)), min=float(np.min(v)), max=float(np.max(v)), samples=[float(x) for x in v])


def time_torch(dev, w0, Z, Y, U, perms, batch, K):
    net = Net()
    net.load_state_dict({k: torch.from_numpy(np.asarray(v, dtype=np.float32).reshape(net.state_dict()[k].shape)) for k, v in w0.arrays.items()})
    net = net.to(dev).train()
    opt = torch.optim.AdamW(net.parameters(), lr=3e-3)
    Zt, Yt, Ut = (torch.from_numpy(a).to(dev) for a in (Z, Y, U))
    sync = torch.cuda.synchronize if dev.type == "cuda" else (lambda: None)
    out = []
    for i, p in enumerate(perms):
        pt = torch.from_numpy(p.astype(np.int64)).to(dev)
        sync()
        t0 = time.perf_counter()
        torch_epoch(net, opt, Zt, Yt, Ut, pt, batch, K)
        sync()
        if i:
            out.append(time.perf_counter() - t0)
    return out


def time_engine(w0, Z, Y, U, perms, batch, K):
    ctx = _lib.default_context()
    tr = PINcTrainer(w0, ctx=ctx, batch=batch, rollout_steps=K)
    data = tr.upload(Z, Y, U)
    host, dev = [], []
    ms = ctypes.c_float(0.0)
    try:
        for i, p in enumerate(perms):
            ctx.check(ctx.lib.brov_set_timing(ctx.h, 1 if i else 0), "brov_set_timing")
            ctx.check(ctx.lib.brov_sync(ctx.h), "brov_sync")
            t0 = time.perf_counter()
            log = tr.epoch_on(data, p)               # uploads the order, queues the epoch, reads the loss log back
            ctx.check(ctx.lib.brov_sync(ctx.h), "brov_sync")
            dt = time.perf_counter() - t0
            if i:
                ctx.check(ctx.lib.brov_last_kernel_ms(ctx.h, ctypes.byref(ms)), "brov_last_kernel_ms")
                host.append(dt)
                dev.append(ms.value * 1e-3)
            assert np.all(np.isfinite(log))
        ctx.check(ctx.lib.brov_set_timing(ctx.h, 0), "brov_set_timing")
    finally:
        for a in data:
            a.free()
        tr.close()
    return host, dev


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=36658)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--rollout-steps", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--skip-cpu", action="store_true")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "pinc_train_time.json"))
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    N = a.rows
    X = np.cumsum(rng.normal(0, 0.01, (N + 1, 9)), axis=0).astype(np.float32)
    psi = np.cumsum(rng.normal(0, 0.01, N + 1))
    X[:, 3], X[:, 4] = np.cos(psi), np.sin(psi)
    U = rng.normal(0, 5.0, (N, 4)).astype(np.float32)
    Z = np.hstack([X[:-1], U, np.full((N, 1), 0.02, np.float32)]).astype(np.float32)
    Y = X[1:].copy()
    perms = [rng.permutation(N).astype(np.int32) for _ in range(a.repeats + 1)]       # [0] is the warm-up epoch
    w0 = PINcWeights.init(0)
    res = dict(rows=N, batch=a.batch, rollout_steps=a.rollout_steps, use_physics=True, iterations=-(-N // a.batch), repeats=a.repeats,
               warmup_epochs=1, torch_version=torch.__version__, device=torch.cuda.get_device_name(0),
               reference_logged="737 s for 200 epochs (training/best_results.txt), 3.7 s per epoch")
    host, dev = time_engine(w0, Z, Y, U, perms, a.batch, a.rollout_steps)
    res["engine_host_s"], res["engine_hip_event_s"] = stats(host), stats(dev)
    print("engine", res["engine_host_s"]["median"], res["engine_hip_event_s"]["median"], flush=True)
    res["torch_rocm_s"] = stats(time_torch(torch.device("cuda"), w0, Z, Y, U, perms, a.batch, a.rollout_steps))
    print("torch rocm", res["torch_rocm_s"]["median"], flush=True)
    if not a.skip_cpu:
        res["torch_cpu_threads"] = torch.get_num_threads()
        res["torch_cpu_s"] = stats(time_torch(torch.device("cpu"), w0, Z, Y, U, perms, a.batch, a.rollout_steps))
        print("torch cpu", res["torch_cpu_s"]["median"], flush=True)
    best = min(res[k]["median"] for k in ("torch_rocm_s", "torch_cpu_s") if k in res)
    res["speedup_vs_faster_torch_baseline"] = best / res["engine_host_s"]["median"]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({k: (v["median"] if isinstance(v, dict) else v) for k, v in res.items()}))
