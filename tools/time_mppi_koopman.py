"""One model-predictive (MPPI) update planned with a Koopman EDMDc model (engine.koopman_mppi_step: free response, linear-form cost
kernel, soft-min -- three launches) against two baselines, at the two shapes of tools/time_mppi.py: (a) B = 64 problems x K = 4096
samples and (b) B = 1, K = 16384; H = 50 at hold 5 (M = 10 knots, so M nu = 80 and the cost kernel runs 64-lane blocks), a
depth-and-heading set-point.  The model has the recorded size, k = 500 centres and r = 8 (d = 512): a seeded synthetic one of
spectral radius 0.98, since the arithmetic does not depend on the entries.  One warm-up, 5 repeats, median and min-max, host to host
(ms, stream synchronised) and by HIP events (the kernels alone), for
  (1) koopman         one engine.koopman_mppi_step call on device-resident arrays, coefficients resident (a KoopmanPlanner), seeded stream;
  (2) fossen          engine.mppi_step with the thruster model, RK4, one planning vehicle, on the same B, K, H: the first baseline.  The
                      two kernels do different work (a block convolution against an RK4 rollout); no ratio is expected in advance;
  (3) assembled       the same update from what the engine offered before: normals in NumPy, held into B K command sequences,
                      engine.simulate_lifted on them (H lifted GEMM steps on the device, host arrays in and out), the tracking error, the
                      cost and the soft-min on the host -- the second baseline, host to host only.  The fused call has to beat it.
Writes the record as JSON (default profiles/mppi_koopman_time.json) and prints it.

    GPU box: python3 tools/time_mppi_koopman.py [--out profiles/mppi_koopman_time.json]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np  # noqa: E402
from bluerov2_dynamics_amd import _lib, engine  # noqa: E402
from bluerov2_dynamics_amd.fossen import control  # noqa: E402
from time_rollout_pop import _summary, timed  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Q = [40.0, 40.0, 60.0, 4.0, 4.0, 6.0, 2.0, 2.0, 3.0, 0.2, 0.2, 0.4]
N_STATE, N_INPUT, N_RBF = 12, 8, 500


def synthetic_model(rng):
    """(C, gamma, A, B) of the recorded size: A = 0.98 A0 / rho(A0), A0 = I + 0.3 G / sqrt(d)"""
    d = N_STATE + N_RBF
    A0 = np.eye(d) + 0.3 * rng.normal(size=(d, d)) / np.sqrt(d)
    A = 0.98 * A0 / np.max(np.abs(np.linalg.eigvals(A0)))
    C = rng.uniform(-1.0, 1.0, (N_RBF, N_STATE))
    C[:, 2] += 5.0
    return C, 0.5, A, 0.05 * rng.normal(size=(d, N_INPUT))


def assembled(ctx, mdl, cfg, x, ref, U_nom, dt, K, H, rng):
    """the update assembled from parts; returns (milliseconds, U_new, seconds per part)"""
    C, gamma, A, Bm = mdl
    B, (Mk, nu) = x.shape[0], U_nom.shape[1:]
    hold, lam = cfg.hold, cfg.lam
    sg, lo, hi = np.array(cfg.sigma), np.array(cfg.u_min), np.array(cfg.u_max)
    q, qf, rw = np.array(cfg.q), np.array(cfg.qf), np.array(cfg.r)
    t0 = time.perf_counter()
    xi = rng.standard_normal((B, K, Mk, nu))
    xi[:, 0] = 0.0
    v = np.clip(U_nom[:, None] + sg * xi, lo, hi)
    delta = v - U_nom[:, None]
    useq = np.repeat(v, hold, axis=2)[:, :, :H].reshape(B * K, H, nu)
    t1 = time.perf_counter()
    pred = engine.simulate_lifted(np.repeat(x, K, axis=0), useq, C, gamma, A, Bm, ctx=ctx).reshape(B, K, H + 1, N_STATE)
    t2 = time.perf_counter()
    e = control.error_numpy(_lib.THRUSTER_EULER, pred, ref[:, None])
    S = dt * (np.einsum("bkti,i->bk", e[:, :, :H] ** 2, q) + np.einsum("bktj,j->bk", useq.reshape(B, K, H, nu) ** 2, rw))
    S += np.einsum("bki,i->bk", e[:, :, H] ** 2, qf) + cfg.gamma * np.sum(U_nom[:, None] * delta / (sg * sg), axis=(2, 3))
    w = np.exp(-(S - S.min(axis=1, keepdims=True)) / lam)
    U_new = np.clip(U_nom + np.einsum("bk,bkmj->bmj", w, delta) / w.sum(axis=1)[:, None, None], lo, hi)
    t3 = time.perf_counter()
    return (t3 - t0) * 1e3, U_new, dict(noise_ms=(t1 - t0) * 1e3, simulate_lifted_ms=(t2 - t1) * 1e3, score_softmin_ms=(t3 - t2) * 1e3)


def measure(ctx, mdl, B, K, H, hold, rng):
    dt = 0.02
    C, gamma, A, Bm = mdl
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
    t0 = time.perf_counter()
    planner = engine.KoopmanPlanner(C, gamma, A, Bm, H, hold, ctx=ctx)
    res = dict(B=B, K=K, H=H, hold=hold, knots=Mk, k=N_RBF, d=N_STATE + N_RBF, planner_setup_ms=(time.perf_counter() - t0) * 1e3)
    last = None

    def koopman(events):
        nonlocal last
        last = planner.step(cfg, xd, refd, Ud, dt, K, seed=1)
        return ctx.last_kernel_ms() if events else None
    res["koopman"] = timed(ctx, koopman)
    info = last["info"].numpy()
    res["effective_sample_size_mean"] = float(info[:, 2].mean())
    res["non_finite_samples"] = int(info[:, 3].sum())
    U_fused = last["U_nom"].numpy()
    last = None
    base = ctx.get_params()

    def fossen(events):
        engine.mppi_step(_lib.THRUSTER_EULER, "rk4", [base], cfg, xd, refd, Ud, dt, K, H=H, seed=1, ctx=ctx)
        return ctx.last_kernel_ms() if events else None
    res["fossen"] = timed(ctx, fossen)
    assembled(ctx, mdl, cfg, x, ref, U_nom, dt, K, H, rng)
    runs = [assembled(ctx, mdl, cfg, x, ref, U_nom, dt, K, H, rng) for _ in range(5)]
    res["assembled"] = dict(host=_summary([r[0] for r in runs]), parts_of_the_median_run=sorted(runs, key=lambda r: r[0])[2][2])
    # recorded, not a check: other normals, and at this temperature weights that are nearly one-hot (see effective_sample_size_mean), so the
    # two plans differ by what their best samples differ
    res["plan_difference_fused_vs_assembled"] = float(np.max(np.abs(U_fused - runs[-1][1])))
    med = lambda k, w: res[k][w]["median_ms"]
    res["ratio_koopman_over_fossen"] = dict(host=med("koopman", "host") / med("fossen", "host"),
                                            kernels=med("koopman", "kernels") / med("fossen", "kernels"))
    res["ratio_assembled_over_koopman"] = dict(host=med("assembled", "host") / med("koopman", "host"))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "mppi_koopman_time.json"))
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    ctx = _lib.Context(0)
    ctx.set_timing(True)
    mdl = synthetic_model(rng)
    res = dict(device=ctx.arch, model=f"EDMDc n = {N_STATE}, r = {N_INPUT}, k = {N_RBF} (synthetic, spectral radius 0.98)", reps=5,
               condition="assembled / koopman (host) > 1 at both shapes", runs=[])
    for B, K in ((64, 4096), (1, 16384)):
        res["runs"].append(measure(ctx, mdl, B, K, 50, 5, rng))
        print(json.dumps(res["runs"][-1]), flush=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
