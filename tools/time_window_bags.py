"""What the bag list costs the window evaluator, at the reference's recorded size (45 823 rows, thruster model, Euler, H = 10,
carried lag, P = 9 candidates: one Levenberg-Marquardt population with the 8 default free parameters).  Synthetic recording.
  plain      engine.window_pop on the rows as one recording: the yardstick
  bags_3     the same rows cut into 3 bags
  bags_300   the same rows cut into 300 bags
Each leg: a warm-up, then 5 repeats, the three legs taking turns; HIP-event time of the call's kernels (brov_last_kernel_ms) and,
beside it, host-to-host time of the whole call (uploads of the candidates and the bag table, the download of se [P]); median and
min-max in ms.  Expectation: the ragged call sits within 10 % of the plain call plus the repeats' spread (one more launch, one map
load per lane per kernel).  Writes the record as JSON (default profiles/window_bags_time.json) and prints it.

    GPU box: python3 tools/time_window_bags.py [--out profiles/window_bags_time.json]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np  # noqa: E402
from bluerov2_dynamics_amd import _lib, engine  # noqa: E402
from bluerov2_dynamics_amd.fossen import identify  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def stats(v):
    return dict(median_ms=float(np.median(v)), min_ms=float(min(v)), max_ms=float(max(v)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "window_bags_time.json"))
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    N, H, dt = 45823, 10, 0.02
    rng = np.random.default_rng(0)
    X = np.zeros((N, 12))
    X[:, :3] = np.cumsum(rng.normal(0, 0.002, (N, 3)), 0)
    X[:, 5] = np.cumsum(rng.normal(0, 0.002, N))
    X[:, 6:9] = rng.normal(0, 0.05, (N, 3))
    X[:, 11] = rng.normal(0, 0.05, N)
    U = np.clip(rng.normal(0, 0.2, (N, 8)), -1, 1)
    ctx = _lib.Context(0)
    ctx.set_timing(True)
    Xd, Ud = engine.DevArray.from_host(ctx, X), engine.DevArray.from_host(ctx, U)
    base = ctx.get_params()
    cands = [identify.copy_params(base)]
    for n in identify.DEFAULT_FREE:
        p = identify.copy_params(base)
        identify.set_param(p, n, identify.get_param(p, n) + 1e-4 * max(abs(identify.get_param(p, n)), 1.0))
        cands.append(p)
    legs = {"plain": None}
    for nb in (3, 300):
        legs[f"bags_{nb}"] = np.linspace(0, N, nb + 1).astype(np.int64)

    def run(off):
        t0 = time.perf_counter()
        rm, E = engine.window_pop(_lib.THRUSTER_EULER, "euler", cands, Xd, Ud, H, dt, endpoints=True, ctx=ctx, bag_offsets=off)
        ctx.sync()
        return rm, (time.perf_counter() - t0) * 1e3, ctx.last_kernel_ms()

    res = dict(device=ctx.arch, N=N, H=H, P=len(cands), model="thruster", integrator="euler", carry_lag=1, reps=a.reps)
    kern, host = {k: [] for k in legs}, {k: [] for k in legs}
    for k, off in legs.items():
        rm, _, _ = run(off)                                 # warm-up; also the record of what each leg scores
        res[k] = dict(windows=N - H if off is None else engine.window_count(off, H), rmse_candidate_0=float(rm[0]))
    for _ in range(a.reps):
        for k, off in legs.items():
            _, h_ms, k_ms = run(off)
            kern[k].append(k_ms)
            host[k].append(h_ms)
    for k in legs:
        res[k].update(kernels=stats(kern[k]), host_to_host=stats(host[k]))
    spread = res["plain"]["kernels"]["max_ms"] - res["plain"]["kernels"]["min_ms"]
    for k in ("bags_3", "bags_300"):
        res[k]["kernels_over_plain"] = res[k]["kernels"]["median_ms"] / res["plain"]["kernels"]["median_ms"]
        res[k]["within_10_percent_plus_spread"] = bool(res[k]["kernels"]["median_ms"] <= 1.1 * res["plain"]["kernels"]["median_ms"] + spread)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
