"""Population rollouts: what one brov_rollout_pop_dev call buys over the loop it replaces.  Thruster model, RK4, B = 256
trajectories of T = 500 steps, every state stored, device-resident arrays; median and min-max of 5 repeats after a warm-up, host to
host (ms, stream synchronised) and by HIP events (the kernels alone), for
  (a) pop_P         one engine.rollout_pop call for P vehicles, P in {1, 16, 256}, shared inputs;
  (b) sequential_P  the same P vehicles through brov_set_params + brov_rollout_dev, one after the other: the way of doing it
                    before this entry point (P derivations, P uploads, P launches; brov_rollout_dev on its default path);
  (c) pop_B1_P4096  one trajectory for each of 4096 vehicles, per-candidate inputs (64-lane blocks);
  (d) ensemble_stats on the [256][256 x 501 x 12] result of (a).
Expectation: (a) takes less time than (b) from P = 16 up.  Writes the record as JSON (default profiles/rollout_pop_time.json) and
prints it; the ratios pop / sequential are part of the record.

    GPU box: python3 tools/time_rollout_pop.py [--out profiles/rollout_pop_time.json]"""
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


def _summary(v):
    return dict(median_ms=float(np.median(v)), min_ms=float(min(v)), max_ms=float(max(v)))


def timed(ctx, fn, reps=5):
    """fn(events): with events it returns the kernel milliseconds of its calls by HIP events (reading them waits for each call, so
    the host-to-host repeats run without)"""
    fn(False)
    ctx.sync()
    host = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn(False)
        ctx.sync()
        host.append((time.perf_counter() - t0) * 1e3)
    return dict(host=_summary(host), kernels=_summary([fn(True) for _ in range(reps)]))


def vehicles(base, P, rng):
    """P vehicles around the nominal one: the default free parameters of the fit, each moved by up to 5 %"""
    out = []
    for _ in range(P):
        p = identify.copy_params(base)
        for n in identify.DEFAULT_FREE:
            identify.set_param(p, n, identify.get_param(p, n) * (1.0 + rng.uniform(-0.05, 0.05)))
        out.append(p)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "rollout_pop_time.json"))
    a = ap.parse_args()
    B, T, dt, M = 256, 500, 0.02, _lib.THRUSTER_EULER
    rng = np.random.default_rng(0)
    ctx = _lib.Context(0)
    ctx.set_timing(True)
    base = ctx.get_params()
    x0 = np.zeros((B, 12))
    x0[:, 2] = 5.0
    x0d = engine.DevArray.from_host(ctx, x0)
    Ud = engine.DevArray.from_host(ctx, rng.uniform(-1, 1, (B, T, 8)))
    res = dict(device=ctx.arch, model="thruster", integrator="rk4", B=B, T=T, stride=1, reps=5)
    traj1, xT1 = engine.DevArray(ctx, (B, T + 1, 12)), engine.DevArray(ctx, (B, 12))
    last = None
    for P in (1, 16, 256):
        cands = vehicles(base, P, rng)

        def pop(events):
            nonlocal last
            last = engine.rollout_pop(M, "rk4", cands, x0d, Ud, dt, ctx=ctx)
            return ctx.last_kernel_ms() if events else None

        def sequential(events):
            ms = 0.0
            for p in cands:
                ctx.set_params(p)
                engine.rollout_dev(M, "rk4", x0d, Ud, dt, traj=traj1, xT=xT1, layout="btu", ctx=ctx)
                if events:
                    ms += ctx.last_kernel_ms()
            ctx.set_params(base)
            return ms

        pop(False)
        sequential(False)                                 # leaves the last vehicle's rollout in traj1
        diff = np.abs(last["traj"].rows(P - 1, P).numpy()[0] - traj1.numpy())
        res[f"max_abs_diff_pop_vs_sequential_{P}"] = float(diff.max())
        res[f"pop_{P}"] = timed(ctx, pop)
        res[f"sequential_{P}"] = timed(ctx, sequential)
        res[f"ratio_pop_over_sequential_{P}"] = dict(
            host=res[f"pop_{P}"]["host"]["median_ms"] / res[f"sequential_{P}"]["host"]["median_ms"],
            kernels=res[f"pop_{P}"]["kernels"]["median_ms"] / res[f"sequential_{P}"]["kernels"]["median_ms"])
    res["pop_faster_than_sequential_from_16"] = bool(all(res[f"ratio_pop_over_sequential_{P}"]["host"] < 1.0 for P in (16, 256)))

    vals = last["traj"]                                   # [256][256][501][12]

    def stats(events):
        engine.ensemble_stats(vals, ctx=ctx)
        return ctx.last_kernel_ms() if events else None
    res["ensemble_stats_256"] = dict(M=int(np.prod(vals.shape[1:])), **timed(ctx, stats))
    vals = last = None

    P1 = 4096
    cands = vehicles(base, P1, rng)
    x1 = engine.DevArray.from_host(ctx, np.tile(x0[:1], (P1, 1, 1)))
    U1 = engine.DevArray.from_host(ctx, rng.uniform(-1, 1, (P1, 1, T, 8)))

    def pop_b1(events):
        engine.rollout_pop(M, "rk4", cands, x1, U1, dt, per_candidate=True, ctx=ctx)
        return ctx.last_kernel_ms() if events else None
    res["pop_B1_P4096"] = timed(ctx, pop_b1)

    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
