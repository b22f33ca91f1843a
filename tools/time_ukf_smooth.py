"""The unscented RTS smoother (engine.ukf_smooth): what the tape costs the filter, what the backward pass costs, and the two
together.  The setting of tools/time_ukf.py: thruster model, RK4, every component measured, T = 1000 rows at dt = 0.02; shapes (a)
P = 1, B = 4096 and (b) P = 64, B = 64.  One warm-up, 5 repeats, median and min-max, host to host (ms, stream synchronised,
device-resident arrays) and by HIP events (the kernels alone), for
  (1) ukf             engine.ukf_filter with every output, no tape (the figure of tools/time_ukf.py);
  (2) ukf_tape        the same with tape=True: 2.5 KB per row, candidate and recording written besides (10.2 GB at either shape);
  (3) ukf_rts         engine.ukf_rts over that tape, every output (Ps included: 1.3 KB per row);
  (4) ukf_smooth      engine.ukf_smooth with every output: the tape in the library's buffer of 2 GiB by default, so the recordings go
                      through in chunks of 860 (a) or 12 (b), a filter launch and a backward launch each;
  (5) ukf_smooth_one_chunk   the same with tape_bytes = the whole tape: one filter launch and one backward launch;
  (6) numpy           tests/ukf_smooth_ref.py on P = 1, B = 1 and the first 50 rows, EXTRAPOLATED to the shape by the ratio of P B T (a
                      labelled estimate, not a measurement of the whole shape).
Writes the record as JSON (default profiles/ukf_smooth_time.json) and prints it.

    GPU box: python3 tools/time_ukf_smooth.py [--out profiles/ukf_smooth_time.json]"""
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
    """milliseconds of tests/ukf_smooth_ref.py on one recording and its first NUMPY_ROWS rows"""
    import ukf_ref as ur
    import ukf_smooth_ref as usr
    from oracle import fossen_params as fp
    k = ur.cfg(list(cfg.q), list(cfg.r), cfg.alpha, cfg.beta, cfg.kappa)
    t0 = time.perf_counter()
    o = usr.smooth(0, fp.RK4, 0, [fp.from_brov_params(base)], k, x0[:1], P0[:1], U[:1, :NUMPY_ROWS], Y[:1, :NUMPY_ROWS], dt)
    assert o["info"][0, 0, 2] == -1 and o["sinfo"][0, 0, 0] == -1
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
    cfg = estimate.ukf(q=1e-6, r=SIGMA ** 2)
    P0 = np.repeat(np.diag(4.0 * SIGMA ** 2)[None], B, axis=0)
    start = x0 + rng.standard_normal((B, 12)) * SIGMA
    D = engine.DevArray
    x0d, P0d, Ud, Yd = D.from_host(ctx, start), D.from_host(ctx, P0), D.from_host(ctx, U), D.from_host(ctx, Y)
    res = dict(P=P, B=B, T=T, tape_bytes=P * B * T * engine.UKF_TAPE * 8)
    last = None

    def ukf(events, tape=False):
        nonlocal last
        last = None
        last = engine.ukf_filter(M_, "rk4", cands, cfg, x0d, P0d, Ud, Yd, dt, tape=tape, ctx=ctx)
        return ctx.last_kernel_ms() if events else None
    res["ukf"] = timed(ctx, ukf)
    res["ukf_tape"] = timed(ctx, lambda events: ukf(events, tape=True))
    f = last
    assert int((f["info"].numpy()[..., 2] >= 0).sum()) == 0 and np.all(f["nrows"].numpy() == T)
    back = None

    def rts(events):
        nonlocal back
        back = None
        back = engine.ukf_rts(f["xf"], f["tape"], f["nrows"], ctx=ctx)
        return ctx.last_kernel_ms() if events else None
    res["ukf_rts"] = timed(ctx, rts)
    sinfo = back["sinfo"].numpy()
    res["failed_transitions"] = int((sinfo[..., 0] >= 0).sum())
    res["smallest_pivot_backward"] = float(sinfo[..., 1].min())
    xs, xf = back["xs"].rows(0, 1).numpy()[0], f["xf"].rows(0, 1).numpy()[0]
    lin = [0, 1, 2, 6, 7, 8, 9, 10, 11]          # the attitude is estimated up to multiples of 2 pi: left out
    rmse = lambda x: float(np.sqrt(np.mean((x - X[:, :T])[..., lin] ** 2)))
    res["rmse_first_candidate_without_attitude"] = dict(filtered=rmse(xf), smoothed=rmse(xs))
    last = f = back = X = None
    whole = None

    def smooth(events, tape_bytes=0):
        nonlocal whole
        whole = None
        whole = engine.ukf_smooth(M_, "rk4", cands, cfg, x0d, P0d, Ud, Yd, dt, tape_bytes=tape_bytes, ctx=ctx)
        return ctx.last_kernel_ms() if events else None
    res["ukf_smooth"] = timed(ctx, smooth)
    res["ukf_smooth_one_chunk"] = timed(ctx, lambda events: smooth(events, tape_bytes=res["tape_bytes"]))
    whole = None
    ms = numpy_reference_ms(base, cfg, start, P0, U, Y, dt)
    res["numpy"] = dict(measured_ms=ms, measured_shape=dict(P=1, B=1, T=NUMPY_ROWS),
                        extrapolated_ms=ms * P * B * T / NUMPY_ROWS, note="extrapolated by P B T from the measured slice")
    med = lambda k, w: res[k][w]["median_ms"]
    res["ratio_tape_filter_over_filter"] = dict(host=med("ukf_tape", "host") / med("ukf", "host"), kernels=med("ukf_tape", "kernels") / med("ukf", "kernels"))
    res["ratio_backward_over_filter"] = dict(host=med("ukf_rts", "host") / med("ukf", "host"), kernels=med("ukf_rts", "kernels") / med("ukf", "kernels"))
    res["ratio_smooth_over_filter"] = dict(host=med("ukf_smooth", "host") / med("ukf", "host"), kernels=med("ukf_smooth", "kernels") / med("ukf", "kernels"))
    res["ratio_numpy_extrapolated_over_smooth"] = dict(host=res["numpy"]["extrapolated_ms"] / med("ukf_smooth", "host"))
    res["rows_per_second"] = dict(kernels=P * B * T / (med("ukf_smooth", "kernels") * 1e-3))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "ukf_smooth_time.json"))
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
