"""The smoother of the quaternion model (engine.ukf_smooth_quat): what the tape costs the multiplicative filter, what the backward pass
costs, and the two together, beside the Euler-wrench smoother (engine.ukf_smooth with WRENCH_EULER) in the same run.  The setting of
tools/time_ukf_quat.py and tools/time_ukf_smooth.py: RK4, T = 1000 rows at dt = 0.02, every component measured, every output asked
for; shapes (a) P = 1, B = 4096 and (b) P = 64, B = 64; the recordings of tools/time_ukf_quat.py (rollouts of the two models from the
same start under the same smooth wrench, the same noise draw).  An untimed first pass, one warm-up, 5 repeats, median and min-max,
host to host (ms, stream synchronised, device-resident arrays) and by HIP events (the kernels alone), for
  (1) ukf_quat                    engine.ukf_filter_quat with every output, no tape (the figure of tools/time_ukf_quat.py);
  (2) ukf_quat_tape               the same with tape=True: 2 504 bytes per row, candidate and recording written besides (10.3 GB);
  (3) ukf_quat_rts                engine.ukf_rts_quat over that tape, every output (Ps included: 1.3 KB per row);
  (4) ukf_smooth_quat             engine.ukf_smooth_quat with every output and the default tape buffer of 2 GiB: chunks of 856
                                  (a) or 12 (b) recordings, a filter launch and a backward launch each;
  (5) ukf_smooth_quat_one_chunk   the same with tape_bytes = the whole tape: one filter launch and one backward launch;
  (6) ukf_smooth_wrench_euler     engine.ukf_smooth on the Euler-wrench model with the default buffer, and _one_chunk with the whole tape.
Writes the record as JSON (default profiles/ukf_quat_smooth_time.json) and prints it.

    GPU box: python3 tools/time_ukf_quat_smooth.py [--out profiles/ukf_quat_smooth_time.json]"""
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
    del Xe, noise
    res = dict(P=P, B=B, T=T, tape_bytes=P * B * T * engine.UKF_TAPE_QUAT * 8, tape_bytes_wrench_euler=P * B * T * engine.UKF_TAPE * 8)
    keep = {}

    def run(name, call, hold=False):
        # a call's outputs (gigabytes at these shapes) are dropped before the next call, so that every call finds the memory the
        # one before it gave back: the first pass is there for that, and is not timed
        def fn(events):
            keep.pop(name, None)
            out = call()
            if hold:
                keep[name] = out
            return ctx.last_kernel_ms() if events else None
        fn(False)
        ctx.sync()
        res[name] = timed(ctx, fn)

    run("ukf_quat", lambda: engine.ukf_filter_quat("rk4", cands, cfg, xq, P0d, Ud, yq, dt, ctx=ctx))
    run("ukf_quat_tape", lambda: engine.ukf_filter_quat("rk4", cands, cfg, xq, P0d, Ud, yq, dt, tape=True, ctx=ctx), hold=True)
    f = keep.pop("ukf_quat_tape")
    assert int((f["info"].numpy()[..., 2] >= 0).sum()) == 0 and np.all(f["nrows"].numpy() == T)
    run("ukf_quat_rts", lambda: engine.ukf_rts_quat(f["xf"], f["tape"], f["nrows"], ctx=ctx), hold=True)
    back = keep.pop("ukf_quat_rts")
    sinfo = back["sinfo"].numpy()
    res["failed_transitions"] = int((sinfo[..., 0] >= 0).sum())
    res["smallest_pivot_backward"] = float(sinfo[..., 1].min())
    xs, xf = back["xs"].rows(0, 1).numpy()[0], f["xf"].rows(0, 1).numpy()[0]
    rmse = lambda x: float(np.sqrt(np.mean(estimate.quat_boxminus(x, Xq) ** 2)))
    res["rmse_first_candidate"] = dict(filtered=rmse(xf), smoothed=rmse(xs))
    del f, back, xs, xf, Xq
    run("ukf_smooth_quat", lambda: engine.ukf_smooth_quat("rk4", cands, cfg, xq, P0d, Ud, yq, dt, ctx=ctx))
    run("ukf_smooth_quat_one_chunk", lambda: engine.ukf_smooth_quat("rk4", cands, cfg, xq, P0d, Ud, yq, dt, tape_bytes=res["tape_bytes"], ctx=ctx))
    run("ukf_smooth_wrench_euler", lambda: engine.ukf_smooth(_lib.WRENCH_EULER, "rk4", cands, cfg, xe, P0d, Ud, ye, dt, ctx=ctx))
    run("ukf_smooth_wrench_euler_one_chunk",
        lambda: engine.ukf_smooth(_lib.WRENCH_EULER, "rk4", cands, cfg, xe, P0d, Ud, ye, dt, tape_bytes=res["tape_bytes_wrench_euler"], ctx=ctx))
    med = lambda k, w: res[k][w]["median_ms"]
    both = lambda a, b: dict(host=med(a, "host") / med(b, "host"), kernels=med(a, "kernels") / med(b, "kernels"))
    res["ratio_tape_filter_over_filter"] = both("ukf_quat_tape", "ukf_quat")
    res["ratio_backward_over_filter"] = both("ukf_quat_rts", "ukf_quat")
    res["ratio_smooth_over_filter"] = both("ukf_smooth_quat", "ukf_quat")
    res["ratio_smooth_one_chunk_over_filter"] = both("ukf_smooth_quat_one_chunk", "ukf_quat")
    res["ratio_smooth_over_wrench_euler_smooth"] = both("ukf_smooth_quat", "ukf_smooth_wrench_euler")
    res["ratio_smooth_one_chunk_over_wrench_euler_smooth_one_chunk"] = both("ukf_smooth_quat_one_chunk", "ukf_smooth_wrench_euler_one_chunk")
    res["rows_per_second"] = dict(kernels=P * B * T / (med("ukf_smooth_quat", "kernels") * 1e-3))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "ukf_quat_smooth_time.json"))
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
