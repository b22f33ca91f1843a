"""Closed-loop rollouts: what evaluating the feedback law inside the rollout kernel costs and buys.  Thruster model, RK4, states
not stored, device-resident arrays, a depth-and-heading set-point under control.pid_thrusters gains; shapes P = 64, B = 1024,
T = 2000 (64 vehicles around the nominal one) and P = 1, B = 65536, T = 1000; hold 1 and 5.  One warm-up, 5 repeats, median and
min-max, host to host (ms, stream synchronised) and by HIP events (the kernels alone), for
  (a) feedback        one engine.rollout_feedback call (metrics only; `feedback_store_u` also writes the applied commands);
  (b) open_loop       engine.rollout_pop on the same x0 with U = the applied commands of (a): the same plant steps without the law,
                      the baseline (rollout_pop is not changed by this work);
  (c) per_step_route  what a user had before: T calls of rollout_pop with T = 1, host arrays, the law in NumPy in between
                      (control.error_numpy, two copies per step), timed over the first 50 steps and extrapolated to T.
Expectation (an instruction count, nothing measured before this tool): the law is a few hundred fp64 instructions per tick against
~800 of an RK4 step, so (a) / (b) should lie between 1 and 1.5 at hold = 1 and closer to 1 at hold = 5, and (c) / (a) is the launch
and copy overhead of T round trips.  (First measurement: 1.6 - 1.7 and 1.3; README quotes the record.)  Writes the record as JSON (default profiles/rollout_feedback_time.json) and prints it.

    GPU box: python3 tools/time_rollout_feedback.py [--out profiles/rollout_feedback_time.json]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np  # noqa: E402
from bluerov2_dynamics_amd import _lib, engine  # noqa: E402
from bluerov2_dynamics_amd.fossen import control  # noqa: E402
from time_rollout_pop import _summary, timed, vehicles  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROUTE_STEPS = 50


def per_step_route(ctx, cands, fb, x0, ref, dt, steps):
    """the law in NumPy around one-step rollout_pop calls on host arrays; returns the milliseconds of `steps` steps"""
    M, P, B = _lib.THRUSTER_EULER, len(cands), x0.shape[0]
    K, Ki = np.ctypeslib.as_array(fb.K), np.ctypeslib.as_array(fb.Ki)
    lo, hi, zm, hold = np.array(fb.u_min), np.array(fb.u_max), np.array(fb.z_max), fb.hold
    x, lag, z = np.broadcast_to(x0, (P, B, 12)).copy(), np.zeros((P, B, 8, 3)), np.zeros((P, B, 6))
    u = np.zeros((P, B, 8))
    t0 = time.perf_counter()
    for t in range(steps):
        if t % hold == 0:
            e = control.error_numpy(M, x, ref)
            u = np.clip(e @ K.T + z @ Ki.T, lo, hi)
            z = np.clip(z + hold * dt * e[..., :6], -zm, zm)
        r = engine.rollout_pop(M, "rk4", cands, x, u[:, :, None, :], dt, lag=lag, store=False, per_candidate=True, ctx=ctx)
        x, lag = r["xT"], r["lag"]
    return (time.perf_counter() - t0) * 1e3


def measure(ctx, P, B, T, hold, rng):
    M, dt = _lib.THRUSTER_EULER, 0.02
    base = ctx.get_params()
    cands = vehicles(base, P, rng) if P > 1 else [base]
    x0 = np.zeros((B, 12))
    x0[:, 2] = 5.0
    x0[:, :6] += rng.uniform(-0.05, 0.05, (B, 6))
    ref = np.zeros((B, 1, 12))
    ref[:, 0, 2], ref[:, 0, 5] = 6.0, 0.5                                   # one metre deeper, half a radian of heading
    fb = control.pid_thrusters(base, [40.0, 40.0, 60.0, 4.0, 4.0, 6.0], [20.0, 20.0, 30.0, 1.0, 1.0, 2.0], [4.0, 4.0, 6.0, 0.4, 0.4, 0.6],
                               z_max=2.0, hold=hold)
    x0d, refd = engine.DevArray.from_host(ctx, x0), engine.DevArray.from_host(ctx, ref)
    kw = dict(T=T, store=False, ctx=ctx)
    res = dict(P=P, B=B, T=T, hold=hold)

    def feedback(events):
        engine.rollout_feedback(M, "rk4", cands, fb, x0d, refd, dt, **kw)
        return ctx.last_kernel_ms() if events else None
    res["feedback"] = timed(ctx, feedback)
    last = None

    def feedback_u(events):
        nonlocal last
        last = None
        last = engine.rollout_feedback(M, "rk4", cands, fb, x0d, refd, dt, want_u=True, **kw)
        return ctx.last_kernel_ms() if events else None
    res["feedback_store_u"] = timed(ctx, feedback_u)
    U = last["u"]                                                           # [P][B][T][8], stays on the device
    met = last["metrics"].numpy()
    res["saturated_step_share"] = float(met[..., 3].mean() / T)
    xT_closed = last["xT"].numpy()
    last = None
    x0p = engine.DevArray.from_host(ctx, np.broadcast_to(x0, (P, B, 12)))
    open_last = None

    def open_loop(events):
        nonlocal open_last
        open_last = engine.rollout_pop(M, "rk4", cands, x0p, U, dt, store=False, per_candidate=True, ctx=ctx)
        return ctx.last_kernel_ms() if events else None
    res["open_loop"] = timed(ctx, open_loop)
    res["max_abs_diff_xT_feedback_vs_open_loop"] = float(np.abs(open_last["xT"].numpy() - xT_closed).max())
    U = open_last = None
    per_step_route(ctx, cands, fb, x0, ref[:, 0], dt, 5)                    # warm-up
    route = [per_step_route(ctx, cands, fb, x0, ref[:, 0], dt, ROUTE_STEPS) * T / ROUTE_STEPS for _ in range(5)]
    res["per_step_route_extrapolated"] = dict(steps_timed=ROUTE_STEPS, host=_summary(route))
    med = lambda k, w: res[k][w]["median_ms"]
    res["ratio_feedback_over_open_loop"] = dict(host=med("feedback", "host") / med("open_loop", "host"),
                                                kernels=med("feedback", "kernels") / med("open_loop", "kernels"))
    res["ratio_feedback_store_u_over_open_loop"] = dict(host=med("feedback_store_u", "host") / med("open_loop", "host"),
                                                        kernels=med("feedback_store_u", "kernels") / med("open_loop", "kernels"))
    res["ratio_per_step_route_over_feedback"] = dict(host=med("per_step_route_extrapolated", "host") / med("feedback", "host"))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "rollout_feedback_time.json"))
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    ctx = _lib.Context(0)
    ctx.set_timing(True)
    res = dict(device=ctx.arch, model="thruster", integrator="rk4", store=False, reps=5, runs=[])
    for P, B, T in ((64, 1024, 2000), (1, 65536, 1000)):
        for hold in (1, 5):
            res["runs"].append(measure(ctx, P, B, T, hold, rng))
            print(json.dumps(res["runs"][-1]), flush=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
