"""One tick of linear model-predictive control with a Koopman EDMDc model (engine.koopman_lmpc_step: free response, gradient, and the
whole ADMM loop in one launch -- three launches) against two baselines, with the model of the recorded size (n = 12, r = 8, k = 500,
a seeded synthetic one of spectral radius 0.98), H = 50 at hold 5 (Nv = 80: W lives in LDS), 200 iterations at tol = 0, coefficients resident (a KoopmanLmpc).  One warm-up, 5 repeats, median and min-max, host to host (ms, stream
synchronised) and by HIP events (the kernels alone), for
  (1) lmpc       one engine.koopman_lmpc_step call on device-resident arrays, at nb = 1, 64, 4 096, and at Nv = 312 (H = 39, hold 1:
                 W read from global memory) for nb = 64;
  (2) mppi       engine.koopman_mppi_step (unchanged) on the same box in the same run, at its recorded shapes nb = 64 x K = 4 096 and
                 nb = 1 x K = 16 384: what the sampling planner spends on the same model;
  (3) numpy      the same ADMM on the host in NumPy: g given, one W @ S product per iteration over the nb columns (the BLAS's threads,
                 16 on the measuring box), host to host only.  The one-launch solve has to beat it at nb = 64 and nb = 4 096.
The reference of a problem is a trajectory the model can reach: its own prediction from the problem's state under a random command
sequence within 0.85 of the limits (a set-point would not do: the free response of a random model leaves any set-point, and every
entry of z would end at a limit).  So the minimiser lies inside the limits, J falls by orders of magnitude, and the agreement of
the device's z with the host's is a check of the solve, recorded as plan_difference_lmpc_vs_numpy.
Also recorded: the realised closed-loop metrics of Fossen-MPPI, Koopman-MPPI and Koopman-QP from examples/mppi_tracking.py over one
scenario.  Writes the record as JSON (default profiles/lmpc_koopman_time.json) and prints it.

    GPU box: python3 tools/time_lmpc_koopman.py [--out profiles/lmpc_koopman_time.json]"""
import argparse
import importlib.util
import json
import os
import sys
import time

os.environ.setdefault("OMP_NUM_THREADS", "16")
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np  # noqa: E402
from bluerov2_dynamics_amd import _lib, engine  # noqa: E402
from bluerov2_dynamics_amd.fossen import control  # noqa: E402
from time_mppi_koopman import Q, synthetic_model  # noqa: E402
from time_rollout_pop import _summary, timed  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DT, ITERS = 0.02, 200


def problem(nb, M, rng):
    x = np.zeros((nb, 12))
    x[:, 2] = 5.0
    x[:, :6] += rng.uniform(-0.05, 0.05, (nb, 6))
    ref = np.zeros((nb, 1, 12))
    ref[:, 0, 2], ref[:, 0, 5] = 6.0, 0.5
    return x, ref, rng.uniform(-0.1, 0.1, (nb, M, 8))


def numpy_admm(W, g, z0, lo, hi, rho, iters):
    """the iteration of include/brov2.h over nb columns at once: W [Nv,Nv], g, z0 [Nv,nb]"""
    z, y = np.clip(z0, lo, hi), np.zeros_like(z0)
    for _ in range(iters):
        t = W @ (rho * (z - y) - g) + y
        z = np.clip(t, lo, hi)
        y = t - z
    return z


def blas_threads():
    """the threads the BLAS behind NumPy runs with, as it reports them (None when that cannot be asked)"""
    try:
        from threadpoolctl import threadpool_info
    except ImportError:
        return None
    return max((p.get("num_threads", 0) for p in threadpool_info() if p.get("user_api") == "blas"), default=None)


def measure_lmpc(ctx, planner, nb, rng):
    x, _, U = problem(nb, planner.M, rng)
    cfg = planner.cfg
    P, Gc = planner.P.numpy(), planner.Gc.numpy()
    C = planner.C.numpy()
    dist = (x * x).sum(1)[:, None] + (C * C).sum(1)[None] - 2.0 * x @ C.T
    phi = np.hstack([x, np.exp(-planner.gamma * dist)])
    F = np.einsum("tid,bd->bti", P, phi)
    G = Gc.transpose(0, 2, 1, 3).reshape(planner.H + 1, 12, -1)
    hi1 = np.tile(np.array(cfg.u_max), planner.M)
    ref = F + np.einsum("tia,ba->bti", G, rng.uniform(-0.85, 0.85, (nb, hi1.size)) * hi1)      # reachable: the prediction under these commands
    D = engine.DevArray
    xd, refd, Ud, yd = D.from_host(ctx, x), D.from_host(ctx, ref), D.from_host(ctx, U), D.from_host(ctx, np.zeros_like(U))
    last = None

    def lmpc(events):
        nonlocal last
        last = planner.step(xd, refd, Ud, yd)
        return ctx.last_kernel_ms() if events else None
    res = dict(nb=nb, H=planner.H, hold=planner.hold, Nv=planner.M * 8, iters=ITERS, rho=planner.rho,
               cond_Hq=float(np.linalg.cond(planner.Hq)), lmpc=timed(ctx, lmpc))
    info, z = last["info"].numpy(), last["U_nom"].numpy()
    res["J_mean"], res["J0_mean"] = float(info[:, 0].mean()), float(info[:, 1].mean())
    res["r_prim_max"], res["r_dual_max"], res["entries_at_a_limit_mean"] = float(info[:, 2].max()), float(info[:, 3].max()), float(info[:, 5].mean())
    # the host baseline starts from the g of the same problems (formed here once, not timed) and has to reproduce z
    wq = np.repeat((DT * np.array(cfg.q[:12]))[None], planner.H + 1, axis=0)
    wq[-1] = np.array(cfg.qf[:12])
    rt = ref.copy()                       # the reference adjusted against the state, as the law does
    rt[:, :, 3:6] -= 2.0 * np.pi * np.rint((rt[:, :, 3:6] - x[:, None, 3:6]) / (2.0 * np.pi))
    g = 2.0 * np.einsum("tia,bti->ab", G, wq[None] * (F - rt))
    W = planner.W.numpy()
    lo, hi = np.tile(np.array(cfg.u_min), planner.M)[:, None], np.tile(np.array(cfg.u_max), planner.M)[:, None]
    z0 = np.ascontiguousarray(U.reshape(nb, -1).T)
    numpy_admm(W, g, z0, lo, hi, planner.rho, ITERS)
    runs = []
    for _ in range(5):
        t0 = time.perf_counter()
        zh = numpy_admm(W, g, z0, lo, hi, planner.rho, ITERS)
        runs.append((time.perf_counter() - t0) * 1e3)
    res["numpy"] = dict(host=_summary(runs))
    res["plan_difference_lmpc_vs_numpy"] = float(np.max(np.abs(zh.T.reshape(z.shape) - z)))
    res["ratio_numpy_over_lmpc"] = dict(host=res["numpy"]["host"]["median_ms"] / res["lmpc"]["host"]["median_ms"])
    return res


def measure_mppi(ctx, mdl, nb, K, rng):
    C, gamma, A, Bm = mdl
    x, ref, U = problem(nb, 10, rng)
    cfg = control.mppi(Q, r=0.05, sigma=0.15, lam=0.02, u_min=-1.0, u_max=1.0, hold=5, nu=8)
    D = engine.DevArray
    xd, refd, Ud = D.from_host(ctx, x), D.from_host(ctx, ref), D.from_host(ctx, U)
    planner = engine.KoopmanPlanner(C, gamma, A, Bm, 50, 5, ctx=ctx)

    def mppi(events):
        planner.step(cfg, xd, refd, Ud, DT, K, seed=1)
        return ctx.last_kernel_ms() if events else None
    return dict(nb=nb, K=K, H=50, hold=5, mppi=timed(ctx, mppi))


def closed_loop():
    """the example's scenario under the three planners: mean over the plants of its four metrics"""
    spec = importlib.util.spec_from_file_location("mppi_tracking", os.path.join(REPO, "examples", "mppi_tracking.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    t0 = time.perf_counter()
    out = mod.run(plants=16, seconds=6.0, samples=4096, horizon=50, hold=5, planner="all", verbose=False)
    return dict(scenario="examples/mppi_tracking.py: 16 drawn plants, 6 s at dt = 0.02, H = 50, hold 5, K = 4096 samples, 200 ADMM iterations",
                metrics=list(mod.NAMES), seconds=time.perf_counter() - t0,
                mean_over_the_plants={mod.HEAD.get(k, "PID"): [float(v) for v in m.mean(axis=0)] for k, m in out.items()})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "lmpc_koopman_time.json"))
    ap.add_argument("--no-closed-loop", action="store_true")
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    ctx = _lib.Context(0)
    ctx.set_timing(True)
    mdl = synthetic_model(rng)
    C, gamma, A, Bm = mdl
    res = dict(device=ctx.arch, model="EDMDc n = 12, r = 8, k = 500 (synthetic, spectral radius 0.98)", reps=5, blas_threads=blas_threads(), omp_num_threads=os.environ.get("OMP_NUM_THREADS"),
               condition="numpy / lmpc (host) > 1 at nb = 64 and nb = 4096; lmpc (host) at nb = 1 below the 20 ms of a 50 Hz tick", runs=[], mppi=[])
    for H, hold, nbs in ((50, 5, (1, 64, 4096)), (39, 1, (64,))):
        cfg = control.lmpc(Q, qf=[5.0 * v for v in Q], r=0.05, u_min=-0.3, u_max=0.3, hold=hold, iters=ITERS, nu=8)
        t0 = time.perf_counter()
        planner = engine.KoopmanLmpc(C, gamma, A, Bm, H, cfg, DT, ctx=ctx)
        setup = (time.perf_counter() - t0) * 1e3
        for nb in nbs:
            res["runs"].append(dict(measure_lmpc(ctx, planner, nb, rng), planner_setup_ms=setup))
            print(json.dumps(res["runs"][-1]), flush=True)
    for nb, K in ((64, 4096), (1, 16384)):
        res["mppi"].append(measure_mppi(ctx, mdl, nb, K, rng))
        print(json.dumps(res["mppi"][-1]), flush=True)
    if not a.no_closed_loop:
        res["closed_loop"] = closed_loop()
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
