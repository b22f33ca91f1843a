"""One model-predictive (MPPI) update: what sampling, rolling out and scoring inside two kernels costs against the parts it is made
of.  Thruster model, RK4, hold 5, H = 50, a depth-and-heading set-point; shapes (a) B = 64 problems x K = 4096 samples (64 vehicles
around the nominal one, one planning model each) and (b) B = 1, K = 16384 (one real vehicle: the number that matters is whether a
tick fits far inside the 20 ms of the 50 Hz data).  One warm-up, 5 repeats, median and min-max, host to host (ms, stream
synchronised) and by HIP events (the kernels alone), for
  (1) mppi            one engine.mppi_step call on device-resident arrays, seeded stream (no eps array);
  (2) rollout_pop     engine.rollout_pop, endpoint only, on B K trajectories x H steps with precomputed commands in HBM: the same
                      plant steps without noise, error and cost terms -- the first baseline (rollout_pop is not changed by this work);
  (3) assembled       what a user had before: B K M nu normals in NumPy, held and uploaded as u_ff, engine.rollout_feedback at zero
                      gains for its three metric sums, download, soft-min on the host -- the second baseline, host to host only.
Expectation, not a gate: the cost kernel does rollout_pop's steps plus the error and cost terms per step and reads no command rows,
so (1) / (2) by kernels should not exceed the 1.7 the closed-loop kernel has at hold 1.  Writes the record as JSON (default
profiles/mppi_time.json) and prints it.

    GPU box: python3 tools/time_mppi.py [--out profiles/mppi_time.json]"""
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
Q = [40.0, 40.0, 60.0, 4.0, 4.0, 6.0, 2.0, 2.0, 3.0, 0.2, 0.2, 0.4]


def assembled(ctx, cands, cfg, x, ref, U_nom, dt, K, H, rng):
    """the update assembled from parts; returns (milliseconds, U_new)"""
    M_, B, (Mk, nu) = _lib.THRUSTER_EULER, x.shape[0], U_nom.shape[1:]
    hold, lam = cfg.hold, cfg.lam
    sg, lo, hi = np.array(cfg.sigma), np.array(cfg.u_min), np.array(cfg.u_max)
    q = np.array(cfg.q)
    t0 = time.perf_counter()
    xi = rng.standard_normal((B, K, Mk, nu))
    xi[:, 0] = 0.0
    v = np.clip(U_nom[:, None] + sg * xi, lo, hi)
    delta = v - U_nom[:, None]
    u_ff = np.repeat(v, hold, axis=2)[:, :, :H]
    fb = control.feedback(np.zeros((8, 12)), hold=hold)
    r = engine.rollout_feedback(M_, "rk4", cands, fb, np.repeat(x[:, None], K, axis=1), np.repeat(ref[:, None], K, axis=1), dt, T=H, u_ff=u_ff,
                                store=False, per_candidate=True, ctx=ctx)
    m = r["metrics"]                                               # three unweighted sums: position, attitude, command
    S = q[0] * m[..., 0] + q[3] * m[..., 1] + cfg.r[0] * m[..., 2] + lam * np.sum(U_nom[:, None] * delta / (sg * sg), axis=(2, 3))
    w = np.exp(-(S - S.min(axis=1, keepdims=True)) / lam)
    U_new = np.clip(U_nom + np.einsum("bk,bkmj->bmj", w, delta) / w.sum(axis=1)[:, None, None], lo, hi)
    return (time.perf_counter() - t0) * 1e3, U_new


def measure(ctx, B, K, H, hold, rng):
    M_, dt = _lib.THRUSTER_EULER, 0.02
    base = ctx.get_params()
    cands = vehicles(base, B, rng) if B > 1 else [base]
    Mk = (H + hold - 1) // hold
    x = np.zeros((B, 12))
    x[:, 2] = 5.0
    x[:, :6] += rng.uniform(-0.05, 0.05, (B, 6))
    ref = np.zeros((B, 1, 12))
    ref[:, 0, 2], ref[:, 0, 5] = 6.0, 0.5
    U_nom = rng.uniform(-0.1, 0.1, (B, Mk, 8))
    cfg = control.mppi(Q, r=0.05, sigma=0.15, lam=0.02, u_min=-1.0, u_max=1.0, hold=hold, nu=8)
    D = engine.DevArray
    xd, refd, Ud = D.from_host(ctx, x), D.from_host(ctx, ref), D.from_host(ctx, U_nom)
    res = dict(B=B, K=K, H=H, hold=hold, knots=Mk)
    last = None

    def mppi(events):
        nonlocal last
        last = engine.mppi_step(M_, "rk4", cands, cfg, xd, refd, Ud, dt, K, H=H, seed=1, ctx=ctx)
        return ctx.last_kernel_ms() if events else None
    res["mppi"] = timed(ctx, mppi)
    info = last["info"].numpy()
    res["effective_sample_size_mean"] = float(info[:, 2].mean())
    res["non_finite_samples"] = int(info[:, 3].sum())
    last = None
    # baseline 1: the same plant steps, commands precomputed in HBM, endpoints only
    x0p = D.from_host(ctx, np.repeat(x[:, None], K, axis=1))
    Up = D(ctx, (B, K, H, 8))
    engine.fill_controls_dev(Up.view(B * K, H, 8), "btu", dist="ar1", seed=3, ctx=ctx)

    def pop(events):
        engine.rollout_pop(M_, "rk4", cands, x0p, Up, dt, store=False, per_candidate=True, ctx=ctx)
        return ctx.last_kernel_ms() if events else None
    res["rollout_pop"] = timed(ctx, pop)
    x0p = Up = None
    # baseline 2: assembled from parts, host to host
    assembled(ctx, cands, cfg, x, ref, U_nom, dt, K, H, rng)
    res["assembled"] = dict(host=_summary([assembled(ctx, cands, cfg, x, ref, U_nom, dt, K, H, rng)[0] for _ in range(5)]))
    med = lambda k, w: res[k][w]["median_ms"]
    res["ratio_mppi_over_rollout_pop"] = dict(host=med("mppi", "host") / med("rollout_pop", "host"),
                                              kernels=med("mppi", "kernels") / med("rollout_pop", "kernels"))
    res["ratio_assembled_over_mppi"] = dict(host=med("assembled", "host") / med("mppi", "host"))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "mppi_time.json"))
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    ctx = _lib.Context(0)
    ctx.set_timing(True)
    res = dict(device=ctx.arch, model="thruster", integrator="rk4", reps=5, expectation_ratio_kernels_at_most=1.7, runs=[])
    for B, K in ((64, 4096), (1, 16384)):
        res["runs"].append(measure(ctx, B, K, 50, 5, rng))
        print(json.dumps(res["runs"][-1]), flush=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
