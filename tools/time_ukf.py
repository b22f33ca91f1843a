"""The unscented Kalman filter (engine.ukf_filter): what filtering P vehicles x B recordings of T rows in one launch costs against
the propagation work it contains.  Thruster model, RK4, every component measured, T = 1000 rows at dt = 0.02; shapes (a) P = 1,
B = 4096 (one fitted vehicle, many recordings) and (b) P = 64, B = 64 (the draws of a fit ranked on a set of recordings).  One
warm-up, 5 repeats, median and min-max, host to host (ms, stream synchronised, device-resident arrays) and by HIP events (the
kernel alone), for
  (1) ukf             one engine.ukf_filter call with every output;
  (2) ukf_loglik      the same asking for info alone (rov.log_likelihood_population: no per-row stores);
  (3) rollout_pop     engine.rollout_pop, endpoint only, on 25 P B trajectories x T steps under the same commands (25 P candidates
                      over the B command arrays): the 25 sigma-point propagations alone, one trajectory per lane instead of one
                      sigma point per lane of a 25-of-64 wave, and none of the update, Cholesky and moment phases;
  (4) numpy           tests/ukf_ref.py, the NumPy restatement, on P = 1, B = 1 and the first 50 rows, EXTRAPOLATED to the shape by the
                      ratio of P B T (a labelled estimate, not a measurement of the whole shape).
Writes the record as JSON (default profiles/ukf_time.json) and prints it.

    GPU box: python3 tools/time_ukf.py [--out profiles/ukf_time.json]"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import numpy as np  # noqa: E402
from bluerov2_dynamics_amd import _lib, engine  # noqa: E402
from bluerov2_dynamics_amd.fossen import estimate  # noqa: E402
from time_rollout_pop import timed, vehicles  # noqa: E402

SIGMA = np.array([0.02] * 3 + [0.01] * 3 + [0.03] * 3 + [0.02] * 3)
NUMPY_ROWS = 50


def numpy_reference_ms(base, cfg, x0, P0, U, Y, dt):
    """milliseconds of tests/ukf_ref.py on one recording and its first NUMPY_ROWS rows"""
    import ukf_ref as ur
    from oracle import fossen_params as fp
    k = ur.cfg(list(cfg.q), list(cfg.r), cfg.alpha, cfg.beta, cfg.kappa)
    t0 = time.perf_counter()
    o = ur.filter(0, fp.RK4, 0, [fp.from_brov_params(base)], k, x0[:1], P0[:1], U[:1, :NUMPY_ROWS], Y[:1, :NUMPY_ROWS], dt)
    assert o["info"][0, 0, 2] == -1
    return (time.perf_counter() - t0) * 1e3


def measure(ctx, P, B, T, rng):
    M_, dt = _lib.THRUSTER_EULER, 0.02
    base = ctx.get_params()
    cands = vehicles(base, P, rng) if P > 1 else [base]
    t = np.arange(T) * dt
    U = 0.5 * np.sin(2 * np.pi * t[None, :, None] * rng.uniform(0.3, 1.0, (B, 1, 8)) + rng.uniform(0, 6, (B, 1, 8)))
    x0 = np.zeros((B, 12))
    x0[:, 2] = 5.0
    X = engine.rollout_pop(M_, "rk4", [base], x0, U, dt, ctx=ctx)["traj"][0]
    Y = X[:, :T] + rng.standard_normal((B, T, 12)) * SIGMA
    X = None
    cfg = estimate.ukf(q=1e-6, r=SIGMA ** 2)
    P0 = np.repeat(np.diag(4.0 * SIGMA ** 2)[None], B, axis=0)
    start = x0 + rng.standard_normal((B, 12)) * SIGMA
    D = engine.DevArray
    x0d, P0d, Ud, Yd = D.from_host(ctx, start), D.from_host(ctx, P0), D.from_host(ctx, U), D.from_host(ctx, Y)
    res = dict(P=P, B=B, T=T, sigma_points=25)
    last = None

    def ukf(events, want=engine.UKF_OUTPUTS):
        nonlocal last
        last = engine.ukf_filter(M_, "rk4", cands, cfg, x0d, P0d, Ud, Yd, dt, want=want, ctx=ctx)
        return ctx.last_kernel_ms() if events else None
    res["ukf"] = timed(ctx, ukf)
    info = last["info"].numpy()
    res["failed_filters"] = int((info[..., 2] >= 0).sum())
    res["mean_squared_normalised_innovation"] = float(np.nanmean(last["innov"].rows(0, 1).numpy() ** 2))
    res["smallest_pivot"] = float(info[..., 3].min())
    last = None
    res["ukf_loglik"] = timed(ctx, lambda events: ukf(events, want=("info",)))
    last = None
    # baseline: the 25 propagations of every (candidate, recording, row) as plain rollouts, endpoints only
    many = [c for c in cands for _ in range(25)]

    def pop(events):
        engine.rollout_pop(M_, "rk4", many, x0d, Ud, dt, store=False, ctx=ctx)
        return ctx.last_kernel_ms() if events else None
    res["rollout_pop"] = timed(ctx, pop)
    ms = numpy_reference_ms(base, cfg, start, P0, U, Y, dt)
    res["numpy"] = dict(measured_ms=ms, measured_shape=dict(P=1, B=1, T=NUMPY_ROWS),
                        extrapolated_ms=ms * P * B * T / NUMPY_ROWS, note="extrapolated by P B T from the measured slice")
    med = lambda k, w: res[k][w]["median_ms"]
    res["ratio_ukf_over_rollout_pop"] = dict(host=med("ukf", "host") / med("rollout_pop", "host"),
                                             kernels=med("ukf", "kernels") / med("rollout_pop", "kernels"))
    res["ratio_numpy_extrapolated_over_ukf"] = dict(host=res["numpy"]["extrapolated_ms"] / med("ukf", "host"))
    res["rows_per_second"] = dict(kernels=P * B * T / (med("ukf", "kernels") * 1e-3))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "ukf_time.json"))
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
