"""The output-feedback closed loop (engine.output_feedback): what closing the loop through the filter inside one kernel costs
against the filter alone, and against the tick assembled from one-step calls.  Thruster model, RK4, every component measured,
T = 1000 steps at dt = 0.02, hold 5, lag banks given; shapes (a) P = 1, B = 4096 and (b) P = 64, B = 64 (one plant, P filter models).
One warm-up, 5 repeats, median and min-max, host to host (ms, stream synchronised, device-resident arrays) and by HIP events (the
kernel alone), for
  (1) output_feedback   one engine.output_feedback call with every output;
  (2) ukf               engine.ukf_filter with every output on the rows (u, y) that (1) recorded, at the same shape: the filter alone,
                        without the plant's step, the law and the metrics;
  (3) assembled         the tick a caller can put together without the kernel: per step one engine.ukf_filter call of one row
                        (candidate by candidate: the filter's inputs are shared by its candidates, the estimates are not), the law in
                        NumPy (fossen/control.py: error_numpy) and one engine.rollout_pop call of one step, host arrays, on the first 50
                        steps, EXTRAPOLATED to T by T / 50 (a labelled estimate, not a measurement of the whole horizon).
Writes the record as JSON (default profiles/ukf_feedback_time.json) and prints it.

    GPU box: python3 tools/time_ukf_feedback.py [--out profiles/ukf_feedback_time.json]"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import numpy as np  # noqa: E402
from bluerov2_dynamics_amd import _lib, engine  # noqa: E402
from bluerov2_dynamics_amd.fossen import control, estimate  # noqa: E402
from time_rollout_pop import timed, vehicles  # noqa: E402

SIGMA = np.array([0.02] * 3 + [0.01] * 3 + [0.03] * 3 + [0.02] * 3)
ASSEMBLED_STEPS = 50
HOLD = 5


def assembled_ms(ctx, cands, plant, fb, cfg, x0, P0, V, ref, dt, steps):
    """milliseconds of `steps` ticks assembled from one-step calls, host arrays, all P candidates and B runs"""
    M_ = _lib.THRUSTER_EULER
    P, B = len(cands), x0.shape[0]
    K, Ki = np.ctypeslib.as_array(fb.K), np.ctypeslib.as_array(fb.Ki)
    lo, hi, zm = np.array(list(fb.u_min)), np.array(list(fb.u_max)), np.array(list(fb.z_max))
    xt = np.repeat(x0[None], P, axis=0)
    xh, Ph = xt.copy(), np.repeat(P0[None], P, axis=0)
    le, lp, z = np.zeros((P, B, 8, 3)), np.zeros((P, B, 8, 3)), np.zeros((P, B, 6))
    u = np.zeros((P, B, 8))
    t0 = time.perf_counter()
    for t in range(steps):
        y = xt + V[None, :, t]
        xf = np.empty_like(xh)
        for j in range(P):              # update: a filter call of one row; its prediction is redone below with the command
            xf[j] = engine.ukf_filter(M_, "rk4", cands[j:j + 1], cfg, xh[j], Ph[j], u[j][:, None], y[j][:, None], dt, lag=le[j:j + 1],
                                      want=("xf",), ctx=ctx)["xf"][0, :, 0]
        if t % HOLD == 0:
            e = control.error_numpy(M_, xf.reshape(-1, 12), np.repeat(ref[None], P, axis=0).reshape(-1, 12)).reshape(P, B, 12)
            u = np.clip(e @ K.T + z @ Ki.T, lo, hi)
            z = np.clip(z + HOLD * dt * e[..., :6], -zm, zm)
        r = engine.rollout_pop(M_, "rk4", [plant], xt.reshape(-1, 12), u.reshape(-1, 1, 8), dt, lag=lp.reshape(1, -1, 8, 3), store=False, ctx=ctx)
        xt, lp = r["xT"][0].reshape(P, B, 12), r["lag"][0].reshape(P, B, 8, 3)
        for j in range(P):              # update and predict with the command that was applied
            f = engine.ukf_filter(M_, "rk4", cands[j:j + 1], cfg, xh[j], Ph[j], u[j][:, None], y[j][:, None], dt, lag=le[j:j + 1],
                                  want=("xT", "PT"), ctx=ctx)
            xh[j], Ph[j], le[j] = f["xT"][0], f["PT"][0], f["lag"][0]
    return (time.perf_counter() - t0) * 1e3


def measure(ctx, P, B, T, rng):
    M_, dt = _lib.THRUSTER_EULER, 0.02
    base = ctx.get_params()
    cands = vehicles(base, P, rng) if P > 1 else [base]
    x0 = np.zeros((B, 12))
    x0[:, 2] = 5.0
    ref = x0.copy()
    ref[:, 2] += rng.uniform(0.2, 1.0, B)
    ref[:, 5] += rng.uniform(-0.5, 0.5, B)
    cfg = estimate.ukf(q=1e-6, r=SIGMA ** 2)
    V = estimate.measurement_noise(cfg, (B, T), seed=1)
    P0 = np.repeat(np.diag(4.0 * SIGMA ** 2)[None], B, axis=0)
    start = x0 + rng.standard_normal((B, 12)) * SIGMA
    fb = control.pid_thrusters(base, [40.0, 40.0, 60.0, 4.0, 4.0, 6.0], [20.0, 20.0, 30.0, 1.0, 1.0, 2.0], [4.0, 4.0, 6.0, 0.4, 0.4, 0.6],
                               z_max=2.0, hold=HOLD)
    D = engine.DevArray
    dev = {k: D.from_host(ctx, v) for k, v in dict(x0=x0, start=start, P0=P0, V=V, ref=ref[:, None]).items()}
    lag = (D.from_host(ctx, np.zeros((P, B, 8, 3))), D.from_host(ctx, np.zeros((P, B, 8, 3))))
    res = dict(P=P, B=B, T=T, hold=HOLD)
    last = None

    def loop(events):
        nonlocal last
        last = engine.output_feedback(M_, "rk4", cands, fb, cfg, dev["x0"], dev["start"], dev["P0"], dev["V"], dev["ref"], dt, plant_params=base,
                                      lag=lag, ctx=ctx)
        return ctx.last_kernel_ms() if events else None
    res["output_feedback"] = timed(ctx, loop)
    info, metrics = last["info"].numpy(), last["metrics"].numpy()
    res["failed_runs"] = int((info[..., 2] >= 0).sum())
    res["mean_final_depth_error"] = float(np.mean(np.abs(last["xT_true"].numpy()[..., 2] - ref[None, :, 2])))
    res["mean_position_estimation_error_sum"] = float(np.mean(metrics[..., 4]))
    # the filter alone on the recorded rows of candidate 0 (U and Y are shared by a filter call's candidates)
    Ud, Yd = last["u"].rows(0, 1).view(B, T, 8), last["y"].rows(0, 1).view(B, T, 12)
    last = None
    lag_f = D.from_host(ctx, np.zeros((P, B, 8, 3)))

    def ukf(events):
        engine.ukf_filter(M_, "rk4", cands, cfg, dev["start"], dev["P0"], Ud, Yd, dt, lag=lag_f, ctx=ctx)
        return ctx.last_kernel_ms() if events else None
    res["ukf"] = timed(ctx, ukf)
    ms = assembled_ms(ctx, cands, base, fb, cfg, x0, P0, V, ref, dt, ASSEMBLED_STEPS)
    res["assembled"] = dict(measured_ms=ms, measured_shape=dict(P=P, B=B, T=ASSEMBLED_STEPS),
                            extrapolated_ms=ms * T / ASSEMBLED_STEPS, note="extrapolated by T from the measured steps")
    med = lambda k, w: res[k][w]["median_ms"]
    res["ratio_output_feedback_over_ukf"] = dict(host=med("output_feedback", "host") / med("ukf", "host"),
                                                 kernels=med("output_feedback", "kernels") / med("ukf", "kernels"))
    res["ratio_assembled_extrapolated_over_output_feedback"] = dict(host=res["assembled"]["extrapolated_ms"] / med("output_feedback", "host"))
    res["steps_per_second"] = dict(kernels=P * B * T / (med("output_feedback", "kernels") * 1e-3))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "ukf_feedback_time.json"))
    ap.add_argument("--rows", type=int, default=1000)
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    ctx = _lib.Context(0)
    ctx.set_timing(True)
    res = dict(device=ctx.arch, model="thruster", integrator="rk4", reps=5, runs=[])
    for P, B in ((1, 4096), (64, 64)):
        res["runs"].append(measure(ctx, P, B, a.rows, rng))
        print(json.dumps(res["runs"][-1]), flush=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
