"""PINc inference at the reference's recorded size (training/best_results.txt:804-809: 45 823 test samples; Metrics H = 1 / 10 / 100
28.7 / 265 / 2 556 s, one 500-step rollout 0.279 s), plus a 65 536 x 500 batched rollout on device-resident arrays.  Synthetic
recording; prints one JSON line: per cell the host-to-host ms (median of 5 after a warm-up), the GPU event ms of the cell's kernels
(CallTimer) and the fp32 FLOP fraction of the 157.3 TF vector peak (27 520 FLOP per network step).

    GPU box: python3 tools/time_pinc.py [--out profiles/pinc_time.json]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np  # noqa: E402
from bluerov2_dynamics_amd import _lib, engine  # noqa: E402
from bluerov2_dynamics_amd.pinc import PINc, PINcWeights, set_weights  # noqa: E402

FLOP_STEP = 2 * (14 * 64 + 3 * 64 * 64 + 64 * 9)
PEAK = 157.3e12
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def timed(ctx, fn, reps=5):
    fn()
    ctx.sync()
    walls, gpus = [], []
    for _ in range(reps):
        ctx.set_timing(True)
        t0 = time.perf_counter()
        fn()
        ctx.sync()
        walls.append((time.perf_counter() - t0) * 1e3)
        gpus.append(ctx.last_kernel_ms())
        ctx.set_timing(False)
    return float(np.median(walls)), float(np.median(gpus))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--eval-only", action="store_true", help="the three evaluator cells only (profiler runs)")
    a = ap.parse_args()
    N, dt = 45823, 0.02
    rng = np.random.default_rng(0)
    X = np.zeros((N, 12))
    X[:, :3] = np.cumsum(rng.normal(0, 0.002, (N, 3)), 0)
    X[:, 5] = np.cumsum(rng.normal(0, 0.002, N))
    X[:, 6:9] = rng.normal(0, 0.05, (N, 3))
    X[:, 11] = rng.normal(0, 0.05, N)
    U = np.clip(rng.normal(0, 0.2, (N, 8)), -1, 1)
    net = PINc(PINcWeights(os.path.join(REPO, "tests", "golden", "pinc_weights.npz")))
    ctx = net.ctx
    res = dict(device=ctx.arch, N=N, flop_per_step=FLOP_STEP)
    for H in (1, 10, 100):
        nwin = N - H
        wall, gpu = timed(ctx, lambda: net.window_endpoint_se(X, U, H, dt))
        res[f"eval_H{H}"] = dict(windows=nwin, ms=wall, gpu_ms=gpu, flop_frac=nwin * H * FLOP_STEP / (gpu * 1e-3) / PEAK)
    if a.eval_only:
        print(json.dumps(res), flush=True)
        return
    wall, gpu = timed(ctx, lambda: net.rollout(X[1000][None], U[1000:1500][None], dt))
    res["rollout_1x500"] = dict(ms=wall, gpu_ms=gpu, flop_frac=500 * FLOP_STEP / (gpu * 1e-3) / PEAK)
    B, T = 65536, 500
    set_weights(ctx, net.weights)
    x0 = engine.DevArray.from_host(ctx, X[rng.integers(0, N, B)])
    dU = engine.DevArray(ctx, (B, T, 8))
    engine.fill_controls_dev(dU, "btu", ctx=ctx)
    xT = engine.DevArray(ctx, (B, 12))
    wall, gpu = timed(ctx, lambda: engine.pinc_rollout_dev(x0, dU, dt, xT=xT, ctx=ctx), reps=3)
    res["rollout_65536x500_dev"] = dict(ms=wall, gpu_ms=gpu, flop_frac=B * T * FLOP_STEP / (gpu * 1e-3) / PEAK)
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
