"""Parameter identification at the reference's recorded size (45 823 test samples, H = 10, thruster model, Euler): what one
population call buys over the loop it replaces.  Synthetic recording; median and min-max of 5 repeats after a warm-up, host to host
(ms, stream synchronised), for
  (a) pop_33        one brov_window_endpoint_pop_dev call with P = 33 candidates (base + 32 one-parameter neighbours), end states kept;
  (b) sequential_33 the same 33 candidates through brov_set_params + brov_window_endpoint_se_dev, one after the other: the baseline;
  (c) lm_iteration  one full Levenberg-Marquardt iteration of fossen/identify.py with the 8 default free parameters
                    (9 + 6 candidates, the normal equations, the host solve).
Acceptance: (a) is not slower than (b).  Writes the record as JSON (default profiles/identify_time.json) and prints it.

    GPU box: python3 tools/time_identify.py [--out profiles/identify_time.json]"""
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


def timed(ctx, fn, reps=5):
    fn()
    ctx.sync()
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ctx.sync()
        ms.append((time.perf_counter() - t0) * 1e3)
    return dict(median_ms=float(np.median(ms)), min_ms=float(min(ms)), max_ms=float(max(ms)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "identify_time.json"))
    ap.add_argument("--pop-only", action="store_true", help="leg (a) alone, once after a warm-up (profiler runs)")
    a = ap.parse_args()
    N, H, dt, P = 45823, 10, 0.02, 33
    rng = np.random.default_rng(0)
    X = np.zeros((N, 12))
    X[:, :3] = np.cumsum(rng.normal(0, 0.002, (N, 3)), 0)
    X[:, 5] = np.cumsum(rng.normal(0, 0.002, N))
    X[:, 6:9] = rng.normal(0, 0.05, (N, 3))
    X[:, 11] = rng.normal(0, 0.05, N)
    U = np.clip(rng.normal(0, 0.2, (N, 8)), -1, 1)
    ctx = _lib.Context(0)
    Xd, Ud = engine.DevArray.from_host(ctx, X), engine.DevArray.from_host(ctx, U)
    base = ctx.get_params()
    names = list(identify.FREE_NAMES)                      # 27 names: the last candidates step some of them twice as far
    cands = [identify.copy_params(base)]
    for i in range(P - 1):
        p, n = identify.copy_params(base), names[i % len(names)]
        identify.set_param(p, n, identify.get_param(p, n) + (1 + i // len(names)) * 1e-4 * max(abs(identify.get_param(p, n)), 1.0))
        cands.append(p)
    d_tot, d_per = engine.DevArray(ctx, (1,)), engine.DevArray(ctx, (N - H,))

    def pop():
        return engine.window_pop(_lib.THRUSTER_EULER, "euler", cands, Xd, Ud, H, dt, endpoints=True, ctx=ctx)

    def sequential():
        out = []
        for p in cands:
            ctx.set_params(p)
            engine.window_endpoint_se_dev(_lib.THRUSTER_EULER, "euler", Xd, Ud, H, dt, d_tot, d_per, ctx=ctx)
            out.append(float(d_tot.numpy()[0]))
        ctx.set_params(base)
        return out

    if a.pop_only:
        pop()
        ctx.sync()
        pop()
        ctx.sync()
        return
    res = dict(device=ctx.arch, N=N, H=H, P=P, model="thruster", integrator="euler")
    rm, _ = pop()
    se_seq = np.array(sequential())
    res["max_rel_diff_pop_vs_sequential"] = float(np.max(np.abs(rm ** 2 * ((N - H) * 12) - se_seq) / se_seq))
    res["pop_33"] = timed(ctx, pop)
    res["sequential_33"] = timed(ctx, sequential)
    rov = identify.copy_params(base)
    res["lm_iteration"] = timed(ctx, lambda: identify.fit_parameters(rov, Xd, Ud, dt, H=H, iters=1, model=_lib.THRUSTER_EULER))
    res["pop_not_slower_than_sequential"] = bool(res["pop_33"]["median_ms"] <= res["sequential_33"]["median_ms"])
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
