"""The EM fit of the filter's q and r (engine.ukf_rts_em, engine.ukf_smooth(want=.."em"), estimate.fit_noise): what the statistics
cost the backward pass, what one EM iteration costs, and a whole fit.  The setting of tools/time_ukf_smooth.py: thruster model, RK4,
every component measured, T = 1000 rows at dt = 0.02; shapes (a) P = 1, B = 4096 and (b) P = 64, B = 64.  One warm-up, 5 repeats,
median and min-max, host to host (ms, stream synchronised, device-resident arrays) and by HIP events (the kernels alone), for
  (1) ukf             engine.ukf_filter with every output, no tape;
  (2) ukf_rts         the plain backward pass over a tape, every output;
  (3) ukf_rts_em      the EM backward pass over the same tape, every output and em;
  (4) ukf_rts_em_only the EM backward pass that stores no rows: sinfo and em alone;
  (5) ukf_smooth      engine.ukf_smooth with every output (the plain kernels, chunked by the default tape of 2 GiB);
  (6) em_iteration    engine.ukf_smooth(want=("info", "sinfo", "em")): one EM iteration, no per-row output;
  (7) fit_noise       estimate.fit_noise from q x 100 and sigma x 3, 20 updates (tol = 0; the record says how many ran), host to host,
                      the upload of the inputs included;
  (8) numpy           tests/ukf_em_ref.py on P = 1, B = 1 and the first 50 rows, EXTRAPOLATED to the shape by the ratio of P B T and to
                      20 iterations (a labelled estimate, not a measurement of the whole shape).
--parent FILE merges the record that tools/time_ukf_smooth.py wrote on the PARENT commit (its ukf, ukf_rts and ukf_smooth entries),
to show that the plain passes have not moved.  Writes the record as JSON (default profiles/ukf_em_time.json) and prints it.

    GPU box: python3 tools/time_ukf_em.py [--parent parent_ukf_smooth_time.json] [--out profiles/ukf_em_time.json]"""
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
from time_rollout_pop import _summary, timed, vehicles  # noqa: E402

SIGMA = np.array([0.02] * 3 + [0.01] * 3 + [0.03] * 3 + [0.02] * 3)
NUMPY_ROWS = 50
FIT_ITERS = 20


def numpy_reference_ms(base, cfg, x0, P0, U, Y, dt):
    """milliseconds of one EM iteration of tests/ukf_em_ref.py on one recording and its first NUMPY_ROWS rows"""
    import ukf_em_ref as uer
    import ukf_ref as ur
    from oracle import fossen_params as fp
    k = ur.cfg(list(cfg.q), list(cfg.r), cfg.alpha, cfg.beta, cfg.kappa)
    t0 = time.perf_counter()
    o = uer.stats(0, fp.RK4, 0, [fp.from_brov_params(base)], k, x0[:1], P0[:1], U[:1, :NUMPY_ROWS], Y[:1, :NUMPY_ROWS], dt)
    uer.m_step(o["em"], o["info"], o["sinfo"], [k])
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
    X = None
    cfg = estimate.ukf(q=1e-6, r=SIGMA ** 2)
    guess = estimate.ukf(q=1e-4, r=(3.0 * SIGMA) ** 2)
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
    ukf(False, tape=True)
    f = last
    assert int((f["info"].numpy()[..., 2] >= 0).sum()) == 0 and np.all(f["nrows"].numpy() == T)
    back = None

    def rts(events, em=False, want=None):
        nonlocal back
        back = None
        if em:
            back = engine.ukf_rts_em(f["xf"], f["tape"], f["nrows"], cfg, Yd, ctx=ctx, **({} if want is None else dict(want=want)))
        else:
            back = engine.ukf_rts(f["xf"], f["tape"], f["nrows"], ctx=ctx)
        return ctx.last_kernel_ms() if events else None
    res["ukf_rts"] = timed(ctx, rts)
    plain_xs = back["xs"].rows(0, 1).numpy()
    res["ukf_rts_em"] = timed(ctx, lambda events: rts(events, em=True))
    assert np.array_equal(back["xs"].rows(0, 1).numpy(), plain_xs), "the EM pass must leave xs as it is"
    em = back["em"].numpy()
    res["failed_transitions"] = int((back["sinfo"].numpy()[..., 0] >= 0).sum())
    res["fitted_over_true_sigma_after_one_update_first_candidate"] = np.sqrt(em[0, :, 12:24].sum(axis=0) / em[0, :, 24:36].sum(axis=0) / SIGMA ** 2).tolist()
    res["ukf_rts_em_only"] = timed(ctx, lambda events: rts(events, em=True, want=("sinfo",)))
    last = f = back = None
    whole = None

    def smooth(events, want=None):
        nonlocal whole
        whole = None
        whole = engine.ukf_smooth(M_, "rk4", cands, cfg, x0d, P0d, Ud, Yd, dt, ctx=ctx, **({} if want is None else dict(want=want)))
        return ctx.last_kernel_ms() if events else None
    res["ukf_smooth"] = timed(ctx, smooth)
    res["em_iteration"] = timed(ctx, lambda events: smooth(events, want=("info", "sinfo", "em")))
    whole = None
    fit = None

    def run_fit():
        nonlocal fit
        fit = estimate.fit_noise(M_, "rk4", cands, guess, start, P0, U, Y, dt, iters=FIT_ITERS, tol=0.0, ctx=ctx)
    run_fit()
    host = []
    for _ in range(5):
        t0 = time.perf_counter()
        run_fit()
        host.append((time.perf_counter() - t0) * 1e3)
    res["fit_noise"] = dict(host=_summary(host), updates=len(fit["loglik"]) - 1, converged=bool(fit["converged"]),
                            loglik_first_candidate=fit["loglik"][:, 0].tolist(), fitted_over_true_sigma_first_candidate=np.sqrt(fit["r"][0] / SIGMA ** 2).tolist(),
                            fitted_q_first_candidate=fit["q"][0].tolist(), n_excluded=int(fit["n_excluded"]))
    ms = numpy_reference_ms(base, cfg, start, P0, U, Y, dt)
    res["numpy"] = dict(measured_ms=ms, measured_shape=dict(P=1, B=1, T=NUMPY_ROWS), extrapolated_ms_one_iteration=ms * P * B * T / NUMPY_ROWS,
                        extrapolated_ms_fit=ms * P * B * T / NUMPY_ROWS * FIT_ITERS, note="extrapolated by P B T (and by 20 iterations) from the measured slice")
    med = lambda k, w: res[k][w]["median_ms"]
    res["ratio_em_backward_over_plain_backward"] = dict(host=med("ukf_rts_em", "host") / med("ukf_rts", "host"), kernels=med("ukf_rts_em", "kernels") / med("ukf_rts", "kernels"))
    res["ratio_em_iteration_over_smooth"] = dict(host=med("em_iteration", "host") / med("ukf_smooth", "host"), kernels=med("em_iteration", "kernels") / med("ukf_smooth", "kernels"))
    res["ratio_numpy_extrapolated_over_em_iteration"] = dict(host=res["numpy"]["extrapolated_ms_one_iteration"] / med("em_iteration", "host"))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "ukf_em_time.json"))
    ap.add_argument("--parent", default=None, help="the record of tools/time_ukf_smooth.py on the parent commit")
    ap.add_argument("--rows", type=int, default=1000)
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    ctx = _lib.Context(0)
    ctx.set_timing(True)
    res = dict(device=ctx.arch, model="thruster", integrator="rk4", reps=5, runs=[])
    for P, B in ((1, 4096), (64, 64)):
        res["runs"].append(measure(ctx, P, B, a.rows, rng))
        print(json.dumps(res["runs"][-1]), flush=True)
    if a.parent:
        with open(a.parent) as f:
            parent = json.load(f)
        res["parent_commit"] = dict(tool="tools/time_ukf_smooth.py", runs=[{k: r[k] for k in ("P", "B", "T", "ukf", "ukf_tape", "ukf_rts", "ukf_smooth")}
                                                                            for r in parent["runs"]])
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
