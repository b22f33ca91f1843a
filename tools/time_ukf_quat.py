"""The multiplicative filter of the quaternion model (engine.ukf_filter_quat) against the Euler-wrench filter (engine.ukf_filter with
WRENCH_EULER) on the same commit and shapes: what the 13-state step and the chart cost.  RK4, T = 1000 rows at dt = 0.02, every
component measured, every output asked for; shapes (a) P = 1, B = 4096 and (b) P = 64, B = 64.  Both filters see the same motion:
the recordings are rollouts of the two models from the same start (the quaternion of the Euler angles) under the same smooth wrench,
with the same noise draw added (through [+] on the quaternion side).  An untimed first pass, one warm-up, 5 repeats, median and min-max, host to host (ms,
stream synchronised, device-resident arrays) and by HIP events (the kernel alone).
Writes the record as JSON (default profiles/ukf_quat_time.json) and prints it.

    GPU box: python3 tools/time_ukf_quat.py [--out profiles/ukf_quat_time.json]"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import numpy as np  # noqa: E402
from bluerov2_dynamics_amd import _lib, engine  # noqa: E402
from bluerov2_dynamics_amd.fossen import estimate  # noqa: E402
from bluerov2_dynamics_amd.fossen.BlueROV2_wrench import euler_to_quat  # noqa: E402
from time_rollout_pop import timed, vehicles  # noqa: E402

SIGMA = np.array([0.02] * 3 + [0.01] * 3 + [0.03] * 3 + [0.02] * 3)
SCALE = np.array([10.0, 10.0, 10.0, 0.5, 0.5, 0.5])


def measure(ctx, P, B, T, rng):
    dt = 0.02
    base = ctx.get_params()
    cands = vehicles(base, P, rng) if P > 1 else [base]
    t = np.arange(T) * dt
    U = (0.5 * np.sin(2 * np.pi * t[None, :, None] * np.linspace(0.3, 1.0, 6) + rng.uniform(0, 6, (B, 1, 6))) * SCALE)
    e0 = np.zeros((B, 12))
    e0[:, 2] = 5.0
    e0[:, 3:6] = rng.uniform(-0.3, 0.3, (B, 3))
    q0 = np.concatenate([e0[:, :3], np.stack([euler_to_quat(*a) for a in e0[:, 3:6]]), e0[:, 6:]], 1)
    noise = rng.standard_normal((B, T, 12)) * SIGMA
    start = rng.standard_normal((B, 12)) * SIGMA
    cfg = estimate.ukf(q=1e-6, r=SIGMA ** 2)
    P0 = np.repeat(np.diag(4.0 * SIGMA ** 2)[None], B, axis=0)
    D = engine.DevArray.from_host
    Ud, P0d = D(ctx, U), D(ctx, P0)
    Xe = engine.rollout_pop(_lib.WRENCH_EULER, "rk4", [base], e0, U, dt, ctx=ctx)["traj"][0][:, :T]
    Xq = engine.rollout_pop(_lib.WRENCH_QUAT, "rk4", [base], q0, U, dt, ctx=ctx)["traj"][0][:, :T]
    ye, yq = D(ctx, Xe + noise), D(ctx, estimate.quat_boxplus(Xq, noise))
    xe, xq = D(ctx, e0 + start), D(ctx, estimate.quat_boxplus(q0, start))
    del Xe, Xq, noise
    res = dict(P=P, B=B, T=T)
    calls = dict(ukf_quat=lambda: engine.ukf_filter_quat("rk4", cands, cfg, xq, P0d, Ud, yq, dt, ctx=ctx),
                 ukf_wrench_euler=lambda: engine.ukf_filter(_lib.WRENCH_EULER, "rk4", cands, cfg, xe, P0d, Ud, ye, dt, ctx=ctx))
    for name, call in calls.items():
        # a call's outputs (1.2 GB at these shapes) are dropped before the next call, so that every call finds the memory the one
        # before it gave back: the first pass below is there for that, and is not timed
        def fn(events):
            call()
            return ctx.last_kernel_ms() if events else None
        fn(False)
        ctx.sync()
        res[name] = timed(ctx, fn)
        last = call()
        info = last["info"].numpy()
        res[name]["failed_filters"] = int((info[..., 2] >= 0).sum())
        res[name]["mean_squared_normalised_innovation"] = float(np.nanmean(last["innov"].rows(0, 1).numpy() ** 2))
        del last
    med = lambda k, w: res[k][w]["median_ms"]
    res["ratio_quat_over_wrench_euler"] = dict(host=med("ukf_quat", "host") / med("ukf_wrench_euler", "host"),
                                               kernels=med("ukf_quat", "kernels") / med("ukf_wrench_euler", "kernels"))
    res["rows_per_second"] = dict(kernels=P * B * T / (med("ukf_quat", "kernels") * 1e-3))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "ukf_quat_time.json"))
    ap.add_argument("--rows", type=int, default=1000)
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    ctx = _lib.Context(0)
    ctx.set_timing(True)
    res = dict(device=ctx.arch, integrator="rk4", reps=5, runs=[])
    for P, B in ((1, 4096), (64, 64)):
        res["runs"].append(measure(ctx, P, B, a.rows, rng))
        print(json.dumps(res["runs"][-1]), flush=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
