#!/usr/bin/env python3
"""Headline benchmark (BASELINE.json): RK4 rollout steps/s (batch x horizon) on MI355X, fp64, plus the EDMDc Gram build
samples/s and the sharded 2^20-rollout ensemble (config 4), each against its roofline, with the CPU baselines timed beside.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--dump-outputs DIR] [--full]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N --steps K --warmup W

`python bench.py --gpus N` with N > 1 and no torch.distributed environment starts its N ranks itself (a child
`torch.distributed.run`, before this process touches the GPU) or exits non-zero -- it never measures fewer GPUs than asked.

One "step" = one pass of the hot path over one batch = ONE launch of the rollout kernel over 65 536 trajectories x
5 000 RK4 steps (BASELINE config 2: thruster model, dt = 0.02, iid U(-1,1) commands from the counter-based stream, every
state stored).  Inputs are resident in HBM before the timed region.  With N GPUs every rank runs its own 65 536-trajectory
shard (weak scaling, no collective on the rollout path).

A plain run sets up, warms up, times the K steps, writes what the last timed step computed if --dump-outputs is given
(`dump_outputs`), and prints the one JSON line: the headline figure and the roofline of the timed launches.  With --full,
the legs after the timed headline loop run as well (all reported in the same JSON line, rank 0; the full record of every
leg goes to the --details file):
  verified     the trajectories the TIMED launches wrote, lanes 0..7, every 50th state, against the reference's own
               states (tests/golden/fossen_rollouts.npz: cfg2_rk4), plus random lanes against single-lane re-runs
  rollout_ar1  the same launch on the AR(1) command stream ("dist B", training/train_sim_brov2_koopmanEDMDc.py:161-164)
  edmdc        BASELINE config 3: 10^7 pairs per GPU, lift + G^T[G|Y] on device, RCCL all-reduce of the blocks
  config4      BASELINE config 4: 2^20 rollouts x 500 RK4 steps in total, sharded over the ranks (STRONG scaling), local
               Gram per rank, ONE RCCL all-reduce, fingerprint of the summed Gram (independent of the sharding)
  cpu_baseline the C/OpenMP port of the oracle on the host cores the box grants, and the reference-shaped scalar NumPy loop
"""
import argparse
import json
import os
import socket
import subprocess
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REPO)

# algorithmic work per unit
ROLLOUT_FLOP_PER_STEP = 3.1e3        # fp64 flop per RK4 step per trajectory (reference algebra)
# fp64 VALU instructions the shipped kernel (rollout_pair_kernel: body wave + thrust wave) executes per 64 trajectories and
# step: static count of the two time loops (tools/isa_loops.py) minus the rarely executed blocks;
# tests/test_cabi_cpu.py re-derives them from the compiler's listing, profiles/r02_rollout_pmc.txt has the counter view
ROLLOUT_EXEC_FP64_INSTR = {"rk4": 713, "euler": 248}      # (rk4: 725 before the half-step stages' shorter sin / cos kernels, round 5)
ROLLOUT_BYTES_PER_STEP = 160.0       # 64 B controls in + 96 B state out (store-all)
EDMDC_FLOP_PER_SAMPLE = 1.1236e6     # 2 p^2 + 2 p d, p = 532, d = 524
EDMDC_BYTES_PER_SAMPLE = 256.0
# /opt/skills/guides/MI355X_MICROARCH.md (HBM, clock) and gfx950 datasheet (fp64): SURVEY.md 8(d)
PEAK_HBM_GBS = 8000.0
PEAK_FP64_VALU_TFLOPS = 78.6
PEAK_FP64_MFMA_TFLOPS = 78.6
CLOCK_HZ = 2.4e9                     # nominal; the chip holds 1.9-2.1 GHz under this load, so issue-slot fractions are conservative
SIMDS = 1024


# ceilings measured on this pool with the committed microbenchmarks (profiles/r02_ubench_fp64.txt: v_fma_f64 streams at 2-4
# waves per SIMD 56.9-58.7 TFLOP/s under the board's power cap; MI355X_MICROARCH.md: ~6.3 TB/s achievable HBM)
MEASURED_FP64_VALU_TFLOPS = 57.0
MEASURED_HBM_GBS = 6300.0


def kernel_source_sha():
    """sha256 (16 hex) over the kernel sources with comments and blank space taken out: recorded next to a PMC summary
    (tools/pmc_summary.py) so that a traffic figure taken from an older build of the kernels is visible as stale -- and one that only
    predates an edited comment is not."""
    import hashlib
    import re
    h = hashlib.sha256()
    root = os.path.join(REPO, "bluerov2_dynamics_amd", "csrc")
    for f in sorted(os.listdir(root)):
        if f.endswith((".hip", ".h")):
            txt = open(os.path.join(root, f), encoding="utf-8", errors="replace").read()
            txt = re.sub(r"/\*.*?\*/", " ", txt, flags=re.S)          # block comments
            txt = re.sub(r"//[^\n]*", " ", txt)                         # line comments (no string of these sources holds "//")
            h.update(f.encode())
            h.update(" ".join(txt.split()).encode())
    return h.hexdigest()[:16]


def pmc_traffic(parts, files=("r06_pmc_summary.json", "r05_pmc_summary.json", "r04_pmc_summary.json", "r03_pmc_summary.json", "r02_pmc_summary.json", "r01_pmc_summary.json")):
    """HBM bytes from the committed PMC run (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes of this same command,
    FETCH_SIZE x2 per the gfx950 note of MI355X_MICROARCH.md).  parts: {kernel name in the summary: launches}; the figure is
    the sum over ALL of them (a fit = lift + tail + Gram per chunk).  PMC counters cannot be read from inside the timed
    process, so this is the recorded figure, not a live one: `kernel_source_sha` of the run it came from is printed beside
    the current one and `stale` says whether the kernels changed since."""
    for name in files:
        try:
            d = json.load(open(os.path.join(REPO, "profiles", name)))
            tot = sum(d[k]["hbm_total_GB_per_launch"] * 1e9 * n for k, n in parts.items())
            rec = d.get("_kernel_source_sha")
            cur = kernel_source_sha()
            return {"bytes": tot, "per_kernel_GB_per_launch": {k: d[k]["hbm_total_GB_per_launch"] for k in parts}, "launches": dict(parts),
                    "source": f"profiles/{name} (rocprofv3 --pmc, recorded run)", "recorded_kernel_source_sha": rec,
                    "current_kernel_source_sha": cur, "stale": (rec != cur) if rec else None}
        except Exception:
            continue
    return None


def lloyd_roofline(rows, kk, ms_per_step, iterations):
    """fp64 issue-slot roofline of the Lloyd E-step (csrc/kmeans.hip, candidate filter): VALU instructions one E-step executes
    (SQ_INSTS_VALU of a recorded counter run over the same data, profiles/r0N_lloyd_pmc_summary.json) x 64 lanes x 2 flop over
    the measured time per E + M step, against the fp64 vector peak -- the share of the chip's issue slots the kernel fills.
    The counters are a RECORDED run's (mean over its iterations): the summary's kernel-source hash and iteration count are printed
    beside the current ones, and `stale` says whether the kernels changed since (as pmc_traffic does)."""
    if rows != 10_020_000 or kk != 512 or not ms_per_step:
        return None
    cur = kernel_source_sha()
    for name in ("r06_lloyd_pmc_summary.json", "r05_lloyd_pmc_summary.json", "r04_lloyd_pmc_summary.json", "r03_lloyd_pmc_summary.json"):
        try:
            full = json.load(open(os.path.join(REPO, "profiles", name)))
            d = full.get("kmeans_assign") or full["kmeans_assign_lds_kernel<12>"]      # (all launches of the E-step kernel of the recorded loop)
        except Exception:
            continue
        rec = full.get("_kernel_source_sha")
        tf = d["SQ_INSTS_VALU"] * 128.0 / (ms_per_step * 1e-3) / 1e12
        lst = full.get("kmeans_assign_lds_kernel<12, true>") or {}
        return {"kernel": "kmeans_assign_lds_kernel<12, LIST> (+ bounds, M-step, centre distances, re-sorts)", "bound": "valu_fp64_issue", "achieved": tf,
                "list_form_launches_of_recorded_run": lst.get("launches_SQ_INSTS_VALU"), "list_form_valu_instr_per_e_step": lst.get("SQ_INSTS_VALU"),
                "peak": PEAK_FP64_VALU_TFLOPS, "unit": "TFLOP/s", "frac": tf / PEAK_FP64_VALU_TFLOPS, "valu_instr_per_e_step": d["SQ_INSTS_VALU"],
                "fma_f64_instr_per_e_step": d.get("SQ_INSTS_VALU_FMA_F64"), "ms_per_step": ms_per_step,
                "source": f"profiles/{name} (rocprofv3 --pmc, recorded run)", "recorded_kernel_source_sha": rec, "current_kernel_source_sha": cur,
                "stale": (rec != cur) if rec else None, "recorded_launches": d.get("launches"), "timed_iterations": iterations,
                "note": "every VALU slot priced as an FMA; instruction count = mean over the E-steps of the recorded run of the shipped loop "
                        "(sorted sample order; with the distance bounds most E-steps evaluate only the samples whose bounds fail: fewer "
                        "instructions AND less time than the plain loop -- the fraction says how full the issue slots are, not how much work was avoided), "
                        "time = this run's",
                "algorithmic": {"flop_per_sample": 2.0 * kk * 12, "unit": "TFLOP/s", "achieved": rows * 2.0 * kk * 12 / (ms_per_step * 1e-3) / 1e12,
                                "note": "the reference's E-step (scikit-learn: one N x k x n product per iteration) / this run's time per E + M step -- "
                                        "credit for the candidate filter, the packed-fp32 screening and the distance bounds, NOT a roofline "
                                        "fraction (exceeds the fp64 peak: most of that arithmetic is never done; labels are the full scan's)"},
                "traffic": ({"bytes_per_e_step": d["hbm_total_GB_per_launch"] * 1e9, "read_GB": d.get("hbm_read_GB_per_launch_corrected_x2"),
                             "write_GB": d.get("hbm_write_GB_per_launch"), "algorithmic_GB": rows * (12 * 8 + 4 + 4 + 4 + 4) / 1e9,
                             "note": "FETCH_SIZE (x 2: the gfx950 correction, profiles/r04_fetch_probe.txt) + WRITE_SIZE per E-step of the recorded run; "
                                     "algorithmic = one 96-byte row, its permutation index and old label in, label and sort key out per sample"}
                            if "hbm_total_GB_per_launch" in d else None)}
    return None


def cfg4_counter_terms(B, T, roll_ms, fill_ms):
    """Config 4's two caller-layout kernels against the ceilings that bind them, from the recorded counter run of exactly those kernels
    (tools/r06_cfg4_pmc.sh -> profiles/r06_cfg4_pmc_summary.json; times are this run's): the AR(1) fill is bound by fp64 VALU issue
    (216 instructions per value: two splitmix64, log, sqrt, cospi), the stored rollout by how HBM serves 2 x 65 536 interleaved
    192-byte streams (measured bytes, not algorithmic ones)."""
    try:
        d = json.load(open(os.path.join(REPO, "profiles", "r06_cfg4_pmc_summary.json")))
        if not (B == 1 << 20 and T == 500):
            return {}
        rb, fl = d["rollout_btu"], d["fill_ar1_btu"]
        slots = SIMDS * CLOCK_HZ / 4.0                       # fp64-rate wave-instructions per second, whole chip
        return {"fill_issue_frac": fl["SQ_INSTS_VALU"] / (fill_ms * 1e-3) / slots,
                "fill_valu_instr_per_value": fl["SQ_INSTS_VALU"] / (B * T * 8 / 64.0),
                "rollout_issue_frac": rb["SQ_INSTS_VALU"] / (roll_ms * 1e-3) / slots,
                "rollout_hbm_measured_bytes": rb["hbm_total_GB_per_launch"] * 1e9,
                "rollout_hbm_measured_frac": rb["hbm_total_GB_per_launch"] / (roll_ms * 1e-3) / PEAK_HBM_GBS,
                "counters_source": "profiles/r06_cfg4_pmc_summary.json", "counters_stale": d.get("_kernel_source_sha") != kernel_source_sha()}
    except Exception:
        return {}


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=65536, help="trajectories per GPU")
    ap.add_argument("--horizon", type=int, default=5000)
    ap.add_argument("--layout", default="tpb", choices=["tpb", "tub", "btu"])
    ap.add_argument("--no-store", action="store_true", help="endpoint only (64 B/step algorithmic)")
    ap.add_argument("--integrator", default="rk4", choices=["rk4", "euler"])
    ap.add_argument("--controls", default="iid", choices=["iid", "ar1"], help="command stream of the timed rollout leg")
    ap.add_argument("--no-ar1", action="store_true", help="skip the AR(1) (dist B) rollout variant")
    ap.add_argument("--no-variants", action="store_true", help="skip config 2's other runs (endpoint-only, Euler stored / endpoint-only)")
    ap.add_argument("--no-fit", action="store_true", help="skip the KoopmanEDMDc.fit() / fit_multi() end-to-end leg")
    ap.add_argument("--edmdc-samples", type=int, default=10_000_000, help="(x,u,x+) pairs per GPU for the Gram leg")
    ap.add_argument("--edmdc-steps", type=int, default=2)
    ap.add_argument("--kmeans-iters", type=int, default=300, help="cap on Lloyd iterations (scikit-learn's KMeans default: 300, tol 1e-4)")
    ap.add_argument("--no-edmdc", action="store_true")
    ap.add_argument("--no-cfg4", action="store_true", help="skip the config-4 ensemble leg")
    ap.add_argument("--cfg4-rollouts", type=int, default=1 << 20, help="TOTAL rollouts of the config-4 ensemble (all ranks together)")
    ap.add_argument("--cfg4-horizon", type=int, default=500)
    ap.add_argument("--no-recorded", action="store_true", help="skip the fresh-process KoopmanEDMDc.fit() leg at the reference's recorded size")
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--cpu-seconds", type=float, default=3.0, help="budget of EACH host baseline leg")
    ap.add_argument("--details", default=None, help="where the full record of every leg goes (default: bench_details.json in the repo root); "
                                                    "stdout carries ONE compact JSON line")
    ap.add_argument("--full", action="store_true", help="also run the legs after the headline loop: verification of the timed launches, "
                                                        "rollout variants, EDMDc Gram / fit, config 4, CPU baselines, and the --details file")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR", help="after the timed steps, write what the last step computed as DIR/<name>.npy "
                                                                         "(float64; rank 0's shard; see dump_outputs)")
    return ap.parse_args()


# ---------------------------------------------------------------------------------------------- self launch
def self_launch(a):
    """`python bench.py --gpus N` outside torch.distributed.run: become the launcher.  Runs before anything initialises
    the GPU in this process (device_count() does not on this image); the ranks are children, their exit code is ours."""
    import torch
    have = torch.cuda.device_count()
    share = os.environ.get("BROV2_BENCH_SHARE_GPU") == "1"
    if have < a.gpus and not share:
        sys.stderr.write(f"bench.py: --gpus {a.gpus} requested but {have} GPU(s) visible: refusing to measure fewer GPUs than asked\n")
        sys.exit(2)
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={a.gpus}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    sys.exit(subprocess.call(cmd, env=env))


def usable_cores():
    """Cores this process may actually use: the scheduler affinity, capped by the cgroup CPU quota (the GPU boxes of this
    pool show 256 logical CPUs and grant 16 of them: /sys/fs/cgroup/cpu.max = "1600000 100000")."""
    try:
        n = len(os.sched_getaffinity(0))
    except AttributeError:
        n = os.cpu_count() or 1
    for path in ("/sys/fs/cgroup/cpu.max",):
        try:
            quota, period = open(path).read().split()[:2]
            if quota != "max":
                n = min(n, max(1, int(float(quota) / float(period) + 0.5)))
        except (OSError, ValueError):
            pass
    try:
        q = int(open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us").read())
        per = int(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
        if q > 0 and per > 0:
            n = min(n, max(1, int(q / per + 0.5)))
    except (OSError, ValueError):
        pass
    return max(1, n)


# ---------------------------------------------------------------------------------------------- CPU baselines
def cpu_baseline_rollout(budget_s, integrator):
    """C oracle (oracle/brov2_oracle.c), one thread per usable host core, same stream / model / integrator."""
    from oracle import controls, fossen_c as fc
    cores = usable_cores()
    T = 5000
    integ = fc.INTEG_RK4 if integrator == "rk4" else fc.INTEG_EULER
    x0 = np.zeros((cores, 12))
    x0[:, 2] = 5.0
    U = controls.controls_iid(0x5EED, 0, cores, T)
    fc.rollout(fc.MODEL_THRUSTER_EULER, integ, x0, U, 0.02, store=False, nthreads=cores)      # warm (page faults, thread pool)
    t0 = time.perf_counter()
    fc.rollout(fc.MODEL_THRUSTER_EULER, integ, x0, U, 0.02, store=False, nthreads=cores)
    one = time.perf_counter() - t0
    reps = max(1, min(400, int(round(budget_s / max(one, 1e-3)))))
    t0 = time.perf_counter()
    for _ in range(reps):
        fc.rollout(fc.MODEL_THRUSTER_EULER, integ, x0, U, 0.02, store=False, nthreads=cores)
    el = time.perf_counter() - t0
    return {"value": reps * cores * T / el, "unit": "steps/s", "cores": cores, "kind": "port",
            "sample": f"{reps} x {cores} trajectories x {T} {integrator} steps of the config-2 stream, C oracle with {cores} OpenMP threads "
                      f"(usable cores of the box), {el:.1f} s"}


def cpu_baseline_reference_shape(budget_s, integrator):
    """The reference's way of computing, restated (oracle/fossen_scalar.py): one Python call per right-hand side, small
    ndarray temporaries, one lag update and one cross product per thruster -- sequential, one core.  The reference itself
    measured 775 RK4 steps/s in the build container; this restatement 755 there."""
    import warnings
    from oracle import controls, fossen_scalar as fs
    T = 4000
    U = controls.controls_iid(0x5EED, 0, 1, 5000)[0]
    x0 = np.zeros(12)
    x0[2] = 5.0
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        fs.simulate(x0, U[:20], 0.02, integrator)
        rov = fs.ScalarBlueROV2()
        x = x0.copy()
        n = 0
        t0 = time.perf_counter()
        while n < T and time.perf_counter() - t0 < budget_s:
            x = fs.simulate(x, U[n:n + 50], 0.02, integrator, rov=rov)[-1]
            n += 50
        el = time.perf_counter() - t0
    return {"value": n / el, "unit": "steps/s", "cores": 1, "kind": "port",
            "sample": f"{n} sequential {integrator} steps of trajectory 0 of the config-2 stream, scalar per-call NumPy loop in the reference's "
                      f"shape (oracle/fossen_scalar.py), {el:.1f} s; the reference itself: 775 RK4 steps/s on one core of the build container"}


def cpu_baseline_gram(C, gamma, budget_s):
    """NumPy restatement of the reference's lift + G^T G + G^T Y (BLAS threads as configured on the box)."""
    from oracle import edmdc_numpy as ek
    n_pairs = int(max(20_000, min(200_000, 1.3e5 * budget_s)))
    rng = np.random.default_rng(0)
    X = rng.normal(0, 0.5, (n_pairs + 1, 12))
    U = rng.uniform(-1, 1, (n_pairs + 1, 8))
    cores = usable_cores()
    try:
        from threadpoolctl import threadpool_limits
        limiter = threadpool_limits(limits=cores)          # BLAS would otherwise start one thread per logical CPU it sees
    except ImportError:
        limiter = None
    t0 = time.perf_counter()
    ek.gram([X], [U], C, gamma)
    el = time.perf_counter() - t0
    if limiter is not None:
        limiter.restore_original_limits()
    return {"value": n_pairs / el, "unit": "samples/s", "cores": cores, "kind": "port",
            "sample": f"{n_pairs} pairs, k={C.shape[0]}, NumPy/BLAS lift + Gram on {cores} threads, {el:.1f} s"}


# ---------------------------------------------------------------------------------------------- verification helpers
def recorded_shape_leg(engine, _lib, ctx, dev, dt, want_cpu):
    """KoopmanEDMDc.fit() where the reference's own log quotes it: N = 45 823 samples @ 50 Hz, n = 12, r = 8, 500 RBFs, gamma = 3,
    ridge = 0.1 (training/best_results.txt:3,761,798: 2.30 s on the authors' CPU; 5.34 s for the reference itself in the survey
    container) -- and on the 36 658 training rows the current script would hand it (80 % split,
    training/train_tank_brov2_full_comparison.py:40-44).  Host arrays in, public class, in a FRESH child process (first call = library load,
    context creation, code-object load, scratch arenas, BLAS pool start: what a script pays) and twice more (warm); the same for the
    quaternion variant (n = 13, r = 6: BlueROV2_wrench states, wrench inputs).  Beside it, at OMP_NUM_THREADS=4 (the reference's
    import-time default, Koopman/koopmanEDMDc.py:23-25), scikit-learn's KMeans + the NumPy restatement of fit() in the reference's
    shape (oracle/edmdc_numpy.py; kind "port")."""
    import tempfile
    import torch
    N, k, gamma, ridge = 45823, 500, 3.0, 0.1
    g = torch.Generator(device=dev)
    g.manual_seed(45823)
    # schema-true synthetic recording: one thruster-model trajectory under AR(1) commands + the sim script's sensor noise
    U1 = torch.empty((1, N, 8), dtype=torch.float64, device=dev)
    engine.fill_controls_dev(U1, "btu", "ar1", seed=0x7A2C, b0=0, T_total=N, ctx=ctx)
    X1 = torch.empty((1, N + 1, 12), dtype=torch.float64, device=dev)
    x0 = torch.zeros((1, 12), dtype=torch.float64, device=dev)
    x0[:, 2] = 5.0
    engine.rollout_dev(_lib.THRUSTER_EULER, "euler", x0, U1, dt, traj=X1, layout="btu", stride=1, ctx=ctx)
    sig = torch.tensor([5e-4] * 3 + [1e-3] * 3 + [5e-4] * 3 + [1e-3] * 3, dtype=torch.float64, device=dev)
    X = (X1[0, :N] + torch.randn((N, 12), generator=g, dtype=torch.float64, device=dev) * sig).cpu().numpy()
    U = U1[0].cpu().numpy()
    # quaternion variant: BlueROV2_wrench states [pos, q, nu], body wrench inputs
    Uq1 = torch.empty((1, N, 6), dtype=torch.float64, device=dev)
    engine.fill_controls_dev(Uq1, "btu", "ar1", seed=0x7A2D, b0=0, T_total=N, scale=[20.0, 20.0, 20.0, 1.5, 1.5, 1.5], ctx=ctx)
    Xq1 = torch.empty((1, N + 1, 13), dtype=torch.float64, device=dev)
    xq0 = torch.zeros((1, 13), dtype=torch.float64, device=dev)
    xq0[:, 2] = 5.0
    xq0[:, 3] = 1.0
    engine.rollout_dev(_lib.WRENCH_QUAT, "euler", xq0, Uq1, dt, traj=Xq1, layout="btu", stride=1, ctx=ctx)
    Xq = (Xq1[0, :N] + torch.randn((N, 13), generator=g, dtype=torch.float64, device=dev) * 5e-4).cpu().numpy()
    Uq = Uq1[0].cpu().numpy()
    ok = bool(np.isfinite(X).all() and np.isfinite(Xq).all())
    leg = {"rows_logged_by_the_reference": N, "k": k, "gamma": gamma, "ridge": ridge, "data_finite": ok,
           "reference_logged_fit_s": {"authors_cpu_unspecified": 2.302, "survey_container_8_cores_cold": 5.34,
                                      "source": "training/best_results.txt:761,798; BASELINE.md sections 1-2"}}
    child = os.path.join(REPO, "tools", "bench_fit_child.py")
    tmpd = tempfile.mkdtemp(prefix="brov2_bench_")
    # the three ways a process can hold the library (bluerov2_dynamics_amd/_lib.py: _one_hip_runtime): the default -- torch is not
    # imported, device memory through the C ABI --, the same on /opt/rocm's HIP runtime, and the torch-tensor path of rounds 1-5
    modes = (("torch_free", "auto", "native"), ("torch_free_rocm_runtime", "0", "native"), ("torch_tensors", "1", "torch"))
    try:
        runs = {}
        for tag, rows in (("N45823", N), ("train36658", int(0.8 * N))):
            path = os.path.join(tmpd, tag + ".npz")
            kw = dict(X=X[:rows], U=U[:rows], k=k, gamma=gamma, ridge=ridge)
            if tag == "N45823":
                kw.update(Xq=Xq[:rows], Uq=Uq[:rows])
            np.savez(path, **kw)
            for mode, env_torch, arrays in (modes if tag == "N45823" else modes[:1]):
                t0 = time.perf_counter()
                pr = subprocess.run([sys.executable, child, "gpu", path, "auto", arrays], capture_output=True, text=True, timeout=600,
                                    env=dict(os.environ, BROV2_TORCH=env_torch))
                wall = time.perf_counter() - t0
                if pr.returncode != 0:
                    runs[f"{tag}_{mode}"] = {"error": pr.stderr[-400:]}
                    continue
                r_ = json.loads(pr.stdout.strip().splitlines()[-1])
                r_["child_wall_s"] = wall
                for c_ in ("thruster_12_8", "quaternion_13_6"):
                    if c_ in r_:
                        f_ = r_[c_]["fit_calls_s"]
                        r_[c_]["first_call_s"] = f_[0]
                        r_[c_]["warm_call_s"] = min(f_[1:])
                        r_[c_]["warm_call_median_s"] = float(np.median(f_[1:]))
                        r_[c_]["samples_per_s_warm"] = (r_[c_]["rows"] - 1) / min(f_[1:])
                        r_[c_]["samples_per_s_first_call"] = (r_[c_]["rows"] - 1) / f_[0]
                runs[f"{tag}_{mode}"] = r_
            if want_cpu and tag == "N45823":
                env = dict(os.environ, OMP_NUM_THREADS="4", LOKY_MAX_CPU_COUNT="8")
                t0 = time.perf_counter()
                pr = subprocess.run([sys.executable, child, "cpu", path], capture_output=True, text=True, timeout=900, env=env)
                if pr.returncode == 0:
                    c_ = json.loads(pr.stdout.strip().splitlines()[-1])
                    f_ = c_["thruster_12_8"]["fit_calls_s"]
                    leg["cpu_baseline"] = {"value": (N - 1) / min(f_), "unit": "samples/s", "cores": 4, "kind": "port",
                                           "first_call_s": f_[0], "second_call_s": f_[1], "stages_second_call": c_["thruster_12_8"]["stages_second_call"],
                                           "multistep_rmse_H10_s": c_["thruster_12_8"]["multistep_rmse_H10_s"], "threadpools": c_.get("threadpools"),
                                           "sample": f"the whole call: sklearn KMeans({k}, n_init='auto', random_state=0) + NumPy lift / G^T G / pinv / "
                                                     f"(P G^T) Y in the reference's shape on the same {N} x 12 host arrays, OMP_NUM_THREADS=4, fresh process",
                                           "child_wall_s": time.perf_counter() - t0}
                else:
                    leg["cpu_baseline"] = {"error": pr.stderr[-400:]}
        # the start of the reference's tank scripts: parse the recording's CSV (pandas), then fit -- as it is, and with warm_up() after the
        # imports (the context is created while pandas parses)
        try:
            from bluerov2_dynamics_amd import data as bdata
            csv_path = os.path.join(tmpd, "recording.csv")
            bdata.write_dataset(csv_path, np.arange(N) * dt, X, U)
            script = {}
            for tag_, extra in (("plain", []), ("warm_up", ["warm_up"])):
                best = None
                for _ in range(2):                      # (the first child also pays the page cache of pandas)
                    pr = subprocess.run([sys.executable, child, "csv", csv_path, str(k), str(gamma), str(ridge)] + extra, capture_output=True,
                                        text=True, timeout=600, env=dict(os.environ, BROV2_TORCH="auto"))
                    if pr.returncode == 0:
                        r_ = json.loads(pr.stdout.strip().splitlines()[-1])
                        if best is None or r_["process_start_to_first_fit_done_s"] < best["process_start_to_first_fit_done_s"]:
                            best = r_
                script[tag_] = best if best is not None else {"error": pr.stderr[-300:]}
            leg["csv_script_start"] = script
        except Exception as exc:                        # (pandas missing on the box: the leg is informational)
            leg["csv_script_start"] = {"error": f"{type(exc).__name__}: {exc}"}
        leg["runs"] = runs
        first = {}
        for mode, _, _ in modes:
            run = runs.get(f"N45823_{mode}", {})
            h_ = run.get("thruster_12_8")
            if h_:
                first[mode] = {"first_call_s": h_["first_call_s"], "warm_call_s": h_["warm_call_s"], "warm_call_median_s": h_["warm_call_median_s"],
                               "process_start_to_first_fit_done_s": h_["process_start_to_first_fit_done_s"], "torch_imported": run.get("torch_imported"),
                               "hip_runtime": run.get("hip_runtime"), "first_fit_AB_sha256": run.get("first_fit_AB_sha256"),
                               "multistep_rmse_H1_10_100": h_["multistep_rmse_H1_10_100"]}
        leg["first_calls"] = first
        shas = {v["first_fit_AB_sha256"] for v in first.values()}
        leg["AB_bit_equal_across_modes"] = bool(len(first) == len(modes) and len(shas) == 1)
        h = runs.get("N45823_torch_free", {}).get("thruster_12_8")          # the shipped default
        if h:
            leg["value"] = h["samples_per_s_warm"]
            leg["unit"] = "samples/s"
            leg["metric"] = "KoopmanEDMDc.fit samples/s at the reference's logged size (host arrays, torch-free process, fastest of six warm calls; median and first call beside it)"
            leg["vs_reference_logs"] = {"first_call_vs_authors_2.302s": 2.302 / h["first_call_s"], "warm_call_vs_authors_2.302s": 2.302 / h["warm_call_s"],
                                        "first_call_vs_survey_container_5.34s": 5.34 / h["first_call_s"],
                                        "note": "other hardware: orientation only (BASELINE.json publishes no number for this metric)"}
    finally:
        import shutil
        shutil.rmtree(tmpd, ignore_errors=True)
    return leg


def lanes_from_traj(traj, lay, lanes, rows):
    """[len(lanes), len(rows), nx] host array out of a device trajectory buffer of any layout."""
    import torch
    li = torch.as_tensor(lanes, device=traj.device)
    ri = torch.as_tensor(rows, device=traj.device)
    if lay == "btu":
        out = traj.index_select(0, li).index_select(1, ri)
    elif lay == "tub":
        out = traj.index_select(0, ri).index_select(2, li).permute(2, 0, 1)
    else:
        t = traj.index_select(0, ri).index_select(2, li)               # [rows, nx/2, lanes, 2]
        out = t.permute(2, 0, 1, 3).reshape(len(lanes), len(rows), -1)
    return out.cpu().numpy()


def rel_err(a, b):
    return float(np.max(np.abs(a - b) / np.maximum(1.0, np.abs(b)))) if a.size else 0.0


# ---------------------------------------------------------------------------------------------- --dump-outputs
DUMP_XT_BYTES = 16_000_000           # end states: all of them up to this size (65 536 x 12 fp64 = 6.3 MB)
DUMP_TRAJ_BYTES = 40_000_000         # stored states: a fixed sample of lanes x rows up to this size (64 x 5 001 x 12 fp64 = 30.7 MB)
DUMP_TRAJ_LANES = 64


def dump_plan(B, T):
    """Which end states and which stored states `dump_outputs` writes for B trajectories x T steps: every lane of xT while they
    fit DUMP_XT_BYTES (else a seeded sample), and DUMP_TRAJ_LANES seeded lanes x every row of the trajectory buffer while they fit
    DUMP_TRAJ_BYTES (else evenly spaced rows, first and last included).  Depends on (B, T) only: two runs with the same arguments
    dump the same elements."""
    def lanes(n, k, seed):
        return np.arange(n) if n <= k else np.sort(np.random.default_rng(seed).choice(n, size=k, replace=False))
    end = lanes(B, DUMP_XT_BYTES // (12 * 8), 0x5EED)
    traj_lanes = lanes(B, DUMP_TRAJ_LANES, 0xD0)
    m = max(2, DUMP_TRAJ_BYTES // (12 * 8 * len(traj_lanes)))
    rows = np.arange(T + 1) if T + 1 <= m else np.unique(np.linspace(0, T, m).round().astype(np.int64))
    return end, traj_lanes, rows


def dump_outputs(path, xT, traj, lay, T):
    """What a caller of the timed path receives from its last step, as float64 .npy files under `path`:
    xT.npy           [len(end), 12] end states of the lanes dump_plan picks (all of them at the default sizes)
    traj_sample.npy  [lanes, rows, 12] stored states of dump_plan's lanes and rows (absent with --no-store)"""
    import torch
    os.makedirs(path, exist_ok=True)
    end, lanes, rows = dump_plan(xT.shape[0], T)
    np.save(os.path.join(path, "xT.npy"), xT.index_select(0, torch.as_tensor(end, device=xT.device)).cpu().numpy().astype(np.float64))
    if traj is not None:
        np.save(os.path.join(path, "traj_sample.npy"), lanes_from_traj(traj, lay, lanes, rows).astype(np.float64))


def main():
    a = parse()
    if "WORLD_SIZE" not in os.environ and a.gpus > 1:
        self_launch(a)                     # does not return
    # stdout carries ONE line, the JSON at the end: whatever a library prints meanwhile (gloo announces its ranks on fd 1, for one)
    # goes to stderr
    sys.stdout.flush()
    json_fd = os.dup(1)
    os.dup2(2, 1)
    import torch
    import torch.distributed as dist
    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if world != a.gpus:
        sys.stderr.write(f"bench.py: --gpus {a.gpus} but WORLD_SIZE={world}\n")
        sys.exit(2)
    # Rehearsal knobs for a box with fewer GPUs than ranks (never set by the driver): BROV2_BENCH_SHARE_GPU=1 maps every
    # rank to cuda:0 and BROV2_BENCH_BACKEND=gloo replaces RCCL (which refuses two ranks on one device).
    backend = os.environ.get("BROV2_BENCH_BACKEND", "nccl")
    if os.environ.get("BROV2_BENCH_SHARE_GPU") == "1":
        local = 0
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    if world > 1:
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=dev)
        else:
            dist.init_process_group(backend)

    from bluerov2_dynamics_amd import _lib, engine
    from bluerov2_dynamics_amd import dist as bdist
    ctx = _lib.default_context(local)

    def barrier():
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    def max_over_ranks(x):
        if world == 1:
            return x
        t = torch.tensor([x], dtype=torch.float64, device=dev if backend == "nccl" else "cpu")
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        return float(t.item())

    def gather_ranks(x):
        if world == 1:
            return [x]
        t = torch.tensor([x], dtype=torch.float64, device=dev if backend == "nccl" else "cpu")
        out = [torch.empty_like(t) for _ in range(world)]
        dist.all_gather(out, t)
        return [float(o.item()) for o in out]

    def allreduce_sum_(t):
        """the Gram exchange: RCCL over xGMI (gloo only in the shared-GPU rehearsal)"""
        if world == 1:
            return t
        if backend == "nccl":
            dist.all_reduce(t, op=dist.ReduceOp.SUM)
        else:
            h = t.cpu()
            dist.all_reduce(h, op=dist.ReduceOp.SUM)
            t.copy_(h)
        return t

    # ------------------------------------------------------------------ rollout leg (config 2)
    B, T, dt = a.batch, a.horizon, 0.02
    nu, nx = 8, 12
    lay = a.layout
    shape = {"tub": lambda r_, c_: (r_, c_, B), "btu": lambda r_, c_: (B, r_, c_), "tpb": lambda r_, c_: (r_, c_ // 2, B, 2)}[lay]
    U = torch.empty(shape(T, nu), dtype=torch.float64, device=dev)
    engine.fill_controls_dev(U, lay, a.controls, seed=0x5EED, b0=rank * B, T_total=T, ctx=ctx)
    x0 = torch.zeros((B, nx), dtype=torch.float64, device=dev)
    x0[:, 2] = 5.0
    traj = None
    if not a.no_store:
        traj = torch.empty(shape(T + 1, nx), dtype=torch.float64, device=dev)
    xT = torch.empty((B, nx), dtype=torch.float64, device=dev)

    def step():
        engine.rollout_dev(_lib.THRUSTER_EULER, a.integrator, x0, U, dt, traj=traj, xT=xT, layout=lay, stride=1, ctx=ctx)

    def timed_launches(nsteps):
        barrier()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(nsteps + 1)]
        t0 = time.perf_counter()
        ev[0].record()
        for i in range(nsteps):
            step()
            ev[i + 1].record()       # same stream as the kernel (ctx launches on torch's current stream)
        barrier()
        wall_ = max_over_ranks(time.perf_counter() - t0)
        return wall_, [ev[i].elapsed_time(ev[i + 1]) for i in range(nsteps)]

    for _ in range(a.warmup):
        step()
    wall, kern_ms = timed_launches(a.steps)
    kern_s = float(np.mean(kern_ms)) * 1e-3
    steps_total = world * B * T * a.steps
    value = steps_total / wall
    bytes_per_step = ROLLOUT_BYTES_PER_STEP if not a.no_store else 64.0
    flop_per_step = ROLLOUT_FLOP_PER_STEP if a.integrator == "rk4" else ROLLOUT_FLOP_PER_STEP * 0.76 / 3.1
    flop_rate = B * T * flop_per_step / kern_s / 1e12
    byte_rate = B * T * bytes_per_step / kern_s / 1e9
    # The bound of this kernel is the fp64 VALU issue rate: every fp64 vector instruction (FMA, mul or add alike) holds its
    # SIMD for 4 clocks, so the peak is SIMDS * clock / 4 wave-instructions per second, i.e. 78.6 TFLOP/s only if every slot
    # held an FMA.  achieved = the fp64 instructions the kernel really issues, priced as FMAs (2 flop x 64 lanes): the
    # fraction is the share of issue slots doing fp64 arithmetic and cannot exceed 1 whatever the algebra saves.
    instr = ROLLOUT_EXEC_FP64_INSTR[a.integrator]
    waves = -(-B // 64)
    issue_rate = waves * T * instr / kern_s                        # wave-instructions per second, whole chip
    issue_tflops = issue_rate * 64 * 2 / 1e12
    issue_frac = issue_tflops / PEAK_FP64_VALU_TFLOPS             # == issue_rate / (SIMDS * CLOCK_HZ / 4) up to the datasheet's rounding
    assert torch.isfinite(xT).all()

    # the binding term is max(issue, hbm).  After round 2's instruction trims the kernel sits across the ridge
    # (1 450 executed flop / 160 B = 9.1 < 9.8): both are printed, `bound` / `frac` name the larger one.
    hbm_frac = byte_rate / PEAK_HBM_GBS
    issue_term = {"bound": "valu_fp64_issue", "achieved": issue_tflops, "peak": PEAK_FP64_VALU_TFLOPS, "unit": "TFLOP/s", "frac": issue_frac,
                  "frac_of_measured_ceiling": issue_tflops / MEASURED_FP64_VALU_TFLOPS, "executed_fp64_instr_per_step": instr,
                  "note": "fp64 VALU instructions issued x 64 lanes x 2 flop (every slot priced as an FMA) / kernel time; frac = share "
                          "of the chip's fp64 issue slots (1024 SIMDs x 2.4 GHz / 4) the kernel fills"}
    hbm_term = {"bound": "hbm", "achieved": byte_rate, "peak": PEAK_HBM_GBS, "unit": "GB/s", "frac": hbm_frac,
                "frac_of_measured_ceiling": byte_rate / MEASURED_HBM_GBS, "bytes_per_step": bytes_per_step}
    binding = hbm_term if hbm_frac >= issue_frac else issue_term
    traffic = (pmc_traffic({"rollout": 1}) if (a.integrator == "rk4" and not a.no_store and lay != "btu" and B == 65536 and T == 5000) else None)
    out = {
        "metric": "rk4_rollout_steps_per_s" if a.integrator == "rk4" else "euler_rollout_steps_per_s",
        "value": value, "unit": "steps/s", "n_gpus": world, "steps": a.steps, "warmup": a.warmup,
        "ms_per_step": wall / a.steps * 1e3, "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
        "dtype": "f64", "data": "synthetic",
        "config": {"workload": f"BASELINE config 2: {B} trajectories/GPU x {T} {a.integrator.upper()} steps, thruster model, dt=0.02, "
                               + ("iid U(-1,1) commands" if a.controls == "iid" else "AR(1) commands (dist B)")
                               + f" (splitmix64 stream 0x5EED), layout {lay}, "
                               + ("all states stored" if traj is not None else "endpoint only"),
                   "trajectories_per_gpu": B, "horizon": T, "parallelism": f"{world} x independent shards, no collective"},
        "roofline": {"kernel": f"rollout_pair_kernel<{a.integrator.upper()},{lay.upper()}> (thruster model, two waves per SIMD)",
                     "bound": binding["bound"], "achieved": binding["achieved"], "peak": binding["peak"], "unit": binding["unit"],
                     "frac": binding["frac"], "frac_of_measured_ceiling": binding["frac_of_measured_ceiling"],
                     "measured_ceilings": {"fp64_valu_TFLOPs": MEASURED_FP64_VALU_TFLOPS, "hbm_GBs": MEASURED_HBM_GBS,
                                           "source": "profiles/r02_ubench_fp64.txt, MI355X_MICROARCH.md"},
                     "kernel_ms": kern_s * 1e3, "kernel_ms_each": kern_ms,
                     "algorithmic_bytes_per_launch": B * T * bytes_per_step,
                     "terms": {"valu_fp64_issue": issue_term, "hbm": hbm_term,
                               "note": "SURVEY 8(d): roofline.achieved = max(issue term, HBM term); both are fractions of datasheet peaks"},
                     "algorithmic": {"achieved": flop_rate, "flop_per_step": flop_per_step, "unit": "TFLOP/s",
                                     "note": "SURVEY 8(d) figure: the reference's dense 6x6 algebra per step / kernel time -- credit for "
                                             "algebra; NOT a roofline fraction (the kernel executes 1 450 flop per step, not 3 100)"},
                     "traffic": traffic},
    }

    if a.dump_outputs and rank == 0:
        dump_outputs(a.dump_outputs, xT, traj, lay, T)        # before any later leg overwrites traj / xT

    # ------------------------------------------------------------------ what did the timed launches write?
    if a.full and traj is not None and rank == 0:
        ver = {}
        gpath = os.path.join(REPO, "tests", "golden", "fossen_rollouts.npz")
        defaults = (a.integrator in ("rk4", "euler") and a.controls == "iid" and B >= 8 and os.path.exists(gpath))
        if defaults:
            g = np.load(gpath)
            sub, Tg = int(g["cfg2_sub"]), int(g["cfg2_T"])
            if T == Tg and float(g["cfg2_dt"]) == dt:
                got = lanes_from_traj(traj, lay, list(range(8)), list(range(0, T + 1, sub)))
                ref = g["cfg2_rk4" if a.integrator == "rk4" else "cfg2_euler"]
                ver["vs_reference_fixture"] = {"max_rel_err": rel_err(got, ref), "lanes": 8, "states_per_lane": int(ref.shape[1]),
                                               "fixture": "tests/golden/fossen_rollouts.npz (generated by importing the reference)"}
        # random lanes of the big launch against re-runs of those lanes alone (another grid, the BTU layout)
        rng = np.random.default_rng(7)
        lanes = sorted(set(int(v) for v in rng.integers(0, B, 6)) | {B - 1})
        rows = list(range(0, T + 1, max(1, T // 20)))
        got = lanes_from_traj(traj, lay, lanes, rows)
        Ul = torch.empty((len(lanes), T, nu), dtype=torch.float64, device=dev)
        for i, b in enumerate(lanes):
            engine.fill_controls_dev(Ul[i:i + 1], "btu", a.controls, seed=0x5EED, b0=rank * B + b, T_total=T, ctx=ctx)
        tl = torch.empty((len(lanes), T + 1, nx), dtype=torch.float64, device=dev)
        engine.rollout_dev(_lib.THRUSTER_EULER, a.integrator, x0[: len(lanes)].contiguous(), Ul, dt, traj=tl, layout="btu", stride=1, ctx=ctx)
        ver["random_lanes_vs_single_lane_runs"] = {"max_rel_err": rel_err(got, tl[:, rows].cpu().numpy()), "lanes": lanes}
        ver["max_rel_err"] = max(v["max_rel_err"] for v in ver.values())
        ver["tolerance"] = 1e-9
        ver["ok"] = bool(ver["max_rel_err"] <= 1e-9)
        out["verified"] = ver
        del Ul, tl

    # ------------------------------------------------------------------ AR(1) commands (dist B), same launch
    if a.full and not a.no_ar1 and a.controls == "iid":
        engine.fill_controls_dev(U, lay, "ar1", seed=0x5EED, b0=rank * B, T_total=T, ctx=ctx)
        step()
        w2, k2 = timed_launches(max(1, min(2, a.steps)))
        out["rollout_ar1"] = {"value": world * B * T * len(k2) / w2, "unit": "steps/s", "kernel_ms": float(np.mean(k2)),
                              "finite": bool(torch.isfinite(xT).all().item()),
                              "note": "same kernel and sizes on the AR(1) command stream u_t = clip(0.98 u_{t-1} + 0.02 xi_t) (dist B)"}

    # ------------------------------------------------------------------ config 2's other runs (SURVEY 8(d) cfg 2: "trajectories stored
    # in one run and endpoint-only in another"; the reference's comparison script integrates with Euler,
    # training/train_tank_brov2_full_comparison.py:453-466): same commands, same sizes, each verified
    if a.full and not a.no_variants and a.controls == "iid" and a.integrator == "rk4" and traj is not None:
        engine.fill_controls_dev(U, lay, "iid", seed=0x5EED, b0=rank * B, T_total=T, ctx=ctx)     # back to dist A
        xT_stored = {}
        variants = {}
        gpath = os.path.join(REPO, "tests", "golden", "fossen_rollouts.npz")
        for integ, store in (("rk4", True), ("rk4", False), ("euler", True), ("euler", False)):
            tr = traj if store else None

            def vstep():
                engine.rollout_dev(_lib.THRUSTER_EULER, integ, x0, U, dt, traj=tr, xT=xT, layout=lay, stride=1, ctx=ctx)

            vstep()
            if integ == "rk4" and store:               # the headline launch again: only its end states are needed (for the endpoint-only check)
                torch.cuda.synchronize()
                xT_stored[integ] = xT.clone()
                continue
            barrier()
            nrep = max(1, min(3, a.steps))
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(nrep + 1)]
            t0 = time.perf_counter()
            ev[0].record()
            for i in range(nrep):
                vstep()
                ev[i + 1].record()
            barrier()
            wv = max_over_ranks(time.perf_counter() - t0)
            kms = float(np.mean([ev[i].elapsed_time(ev[i + 1]) for i in range(nrep)]))
            bps = 160.0 if store else 64.0
            ninstr = ROLLOUT_EXEC_FP64_INSTR[integ]
            it = -(-B // 64) * T * ninstr * 128 / (kms * 1e-3) / 1e12
            hb = B * T * bps / (kms * 1e-3) / 1e9
            leg = {"value": world * B * T * nrep / wv, "unit": "steps/s", "kernel_ms": kms, "bytes_per_step": bps,
                   "roofline": {"bound": "hbm" if hb / PEAK_HBM_GBS >= it / PEAK_FP64_VALU_TFLOPS else "valu_fp64_issue",
                                "frac": max(hb / PEAK_HBM_GBS, it / PEAK_FP64_VALU_TFLOPS),
                                "hbm_GBs": hb, "hbm_frac": hb / PEAK_HBM_GBS, "issue_TFLOPs": it, "issue_frac": it / PEAK_FP64_VALU_TFLOPS,
                                "peak_hbm_GBs": PEAK_HBM_GBS, "peak_fp64_TFLOPs": PEAK_FP64_VALU_TFLOPS}}
            if rank == 0:
                ver = {}
                if store:
                    xT_stored[integ] = xT.clone()
                    if os.path.exists(gpath) and B >= 8:
                        g = np.load(gpath)
                        sub, Tg = int(g["cfg2_sub"]), int(g["cfg2_T"])
                        if T == Tg and float(g["cfg2_dt"]) == dt:
                            got = lanes_from_traj(traj, lay, list(range(8)), list(range(0, T + 1, sub)))
                            ver["vs_reference_fixture"] = rel_err(got, g["cfg2_" + integ])
                    rng = np.random.default_rng(11)
                    lanes = sorted(set(int(v) for v in rng.integers(0, B, 5)) | {B - 1})
                    rows = list(range(0, T + 1, max(1, T // 20)))
                    got = lanes_from_traj(traj, lay, lanes, rows)
                    Ul = torch.empty((len(lanes), T, nu), dtype=torch.float64, device=dev)
                    for i, b in enumerate(lanes):
                        engine.fill_controls_dev(Ul[i:i + 1], "btu", "iid", seed=0x5EED, b0=rank * B + b, T_total=T, ctx=ctx)
                    tl = torch.empty((len(lanes), T + 1, nx), dtype=torch.float64, device=dev)
                    engine.rollout_dev(_lib.THRUSTER_EULER, integ, x0[: len(lanes)].contiguous(), Ul, dt, traj=tl, layout="btu", stride=1, ctx=ctx)
                    ver["random_lanes_vs_single_lane_runs"] = rel_err(got, tl[:, rows].cpu().numpy())
                    del Ul, tl
                else:
                    # the endpoint-only launch against the end states of the stored launch of the same integrator
                    ver["xT_vs_stored_run"] = rel_err(xT.cpu().numpy(), xT_stored[integ].cpu().numpy())
                ver["max_rel_err"] = max(ver.values())
                ver["ok"] = bool(ver["max_rel_err"] <= 1e-9)
                leg["verified"] = ver
            variants[f"{integ}_{'stored' if store else 'endpoint_only'}"] = leg
        out["rollout_variants"] = variants
        del xT_stored

    # ------------------------------------------------------------------ EDMDc leg (config 3)
    del traj, U
    torch.cuda.empty_cache()
    n, r, k, gamma, ridge = 12, 8, 512, 1.0, 1e-3
    p, d = n + k + r, n + k
    Cc = None
    if a.full and not a.no_edmdc:
        L = 500
        nb = max(1, a.edmdc_samples // L)
        Ue = torch.empty((nb, L, r), dtype=torch.float64, device=dev)
        engine.fill_controls_dev(Ue, "btu", "ar1", seed=0xED3D, b0=rank * nb, T_total=L, ctx=ctx)
        Xe = torch.empty((nb, L + 1, n), dtype=torch.float64, device=dev)
        xe0 = torch.zeros((nb, n), dtype=torch.float64, device=dev)
        engine.rollout_dev(_lib.THRUSTER_EULER, "euler", xe0, Ue, dt, traj=Xe, layout="btu", stride=1, ctx=ctx)
        g = torch.Generator(device=dev)
        g.manual_seed(1234 + rank)
        sig = torch.tensor([5e-4] * 3 + [1e-3] * 3 + [5e-4] * 3 + [1e-3] * 3, dtype=torch.float64, device=dev)
        Xe += torch.randn(Xe.shape, generator=g, dtype=torch.float64, device=dev) * sig   # sensor noise of train_sim...:174-192
        torch.cuda.synchronize()
        # centres (outside the Gram timing, timed on its own): k-means++ seeding with scikit-learn's algorithm and random
        # stream, then Lloyd's E/M loop, both over ALL states in HBM (csrc/kmeans.hip); rank 0's result is broadcast
        Cc = torch.empty((k, n), dtype=torch.float64, device=dev)
        kmeans_info = None
        if rank == 0:
            torch.cuda.synchronize()
            ctx.set_timing(True)
            tk = time.perf_counter()
            ktim = {}
            Ck, inertia, n_iter = engine.kmeans_centers_dev(Xe.view(-1, n), k, random_state=0, max_iter=a.kmeans_iters, ctx=ctx, timings=ktim)
            torch.cuda.synchronize()
            lloyd_ms = ktim.get("lloyd_ms", float("nan"))
            ctx.set_timing(False)
            Cc.copy_(Ck)
            kmeans_info = {"rows": nb * (L + 1), "k": k, "lloyd_iterations": n_iter, "max_iter": a.kmeans_iters, "loop_info": ctx.kmeans_loop_info(),
                           "lloyd_ms_total": lloyd_ms, "lloyd_ms_per_iteration": lloyd_ms / max(n_iter, 1),
                           "kmeanspp_ms_device": ktim.get("kmeanspp_ms"), "wall_s_seeding_plus_lloyd": time.perf_counter() - tk,
                           "inertia": inertia,
                           "note": "k-means++ seeding (scikit-learn's algorithm and random stream) and Lloyd both on the GPU over all rows"}
        if world > 1:
            if backend == "nccl":
                dist.broadcast(Cc, 0)
            else:
                Ch = Cc.cpu()
                dist.broadcast(Ch, 0)
                Cc.copy_(Ch)
        GG = torch.zeros((p * p + p * d,), dtype=torch.float64, device=dev)   # one buffer -> one all-reduce
        GtG, GtY = GG[: p * p].view(p, p), GG[p * p:].view(p, d)

        def estep():
            engine.gram_dev(Xe.view(-1, n), Ue.view(-1, r), Cc, gamma, nb, L, L + 1, L, GtG, GtY, ctx=ctx)
            allreduce_sum_(GG)                 # RCCL over xGMI: 4.5 MB, the only collective of the fit

        estep()
        barrier()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        for _ in range(a.edmdc_steps):
            estep()
        e1.record()
        barrier()
        ewall = max_over_ranks(time.perf_counter() - t0)
        ekern_s = e0.elapsed_time(e1) * 1e-3 / a.edmdc_steps
        pairs = nb * L
        Gh_, Yh_ = GtG.cpu().numpy(), GtY.cpu().numpy()
        engine.solve_AB(Gh_, Yh_, ridge * 1.0, d)                  # the process's first LAPACK call starts the BLAS thread pool
        t1 = time.perf_counter()
        A_, B_ = engine.solve_AB(Gh_, Yh_, ridge * 1.0, d)
        solve_s = time.perf_counter() - t1
        eflops = pairs * EDMDC_FLOP_PER_SAMPLE / ekern_s / 1e12
        gram_tasks, gram_slabs = engine.gram_decomposition(n, r, k)
        xflops = pairs * gram_tasks * 12288.0 / ekern_s / 1e12          # MFMA flop the kernel issues / (lift + Gram) time
        chunks = -(-(pairs + nb) // (1 << 20))
        out["edmdc"] = {
            "metric": "edmdc_gram_samples_per_s", "value": world * pairs * a.edmdc_steps / ewall, "unit": "samples/s",
            "pairs_per_gpu": pairs, "ms_per_fit_gram": ewall / a.edmdc_steps * 1e3, "host_pinv_solve_s": solve_s,
            "gram_plus_host_solve_samples_per_s": world * pairs / (ewall / a.edmdc_steps + solve_s),
            "config": {"workload": f"BASELINE config 3: {pairs} (x,u,x+) pairs/GPU from {nb} Euler rollouts x {L} steps, "
                                   f"n=12 r=8 k=512 gamma={gamma}, lift + G^T[G|Y] on device, centres from GPU Lloyd k-means over all states"},
            "roofline": {"kernel": "lift_rows_kernel + gram_kernel (v_mfma_f64_16x16x4_f64)", "bound": "mfma", "achieved": xflops,
                         "peak": PEAK_FP64_MFMA_TFLOPS, "unit": "TFLOP/s", "frac": xflops / PEAK_FP64_MFMA_TFLOPS,
                         "kernel_ms": ekern_s * 1e3, "flop_per_sample": gram_tasks * 12288.0,
                         "tasks": gram_tasks, "slabs_per_chunk": gram_slabs,
                         "note": "achieved = MFMA flop the kernel EXECUTES (tasks x 24 tiles x 16 x 16 x 2 per sample; symmetry and the "
                                 "packing of the staircase make it less than the algorithmic figure) / (lift + Gram) time: a fraction of "
                                 "the pipe, <= 1",
                         "algorithmic": {"achieved": eflops, "flop_per_sample": EDMDC_FLOP_PER_SAMPLE, "unit": "TFLOP/s",
                                         "note": "SURVEY 8(d) figure 2p^2 + 2pd (the reference's full G.T@G + G.T@Y) / time -- credit for "
                                                 "symmetry, NOT a roofline fraction (can exceed the peak)"},
                         "traffic": pmc_traffic({"lift": chunks, "lift_tail": chunks, "gram": chunks}) if pairs == 10_000_000 else None},
            "A_finite": bool(np.isfinite(A_).all() and np.isfinite(B_).all()),
            "kmeans": kmeans_info,
        }
        # ---- the call the reference's scripts make: KoopmanEDMDc.fit() (Koopman/koopmanEDMDc.py:72-103; caller
        # training/train_tank_brov2_full_comparison.py:921-930): (a) the public call on host arrays, (b) its stages end to end on the
        # same data device-resident (engine.fit_dev) -- centres with
        # scikit-learn's stopping rule, G^T[G|Y], host solve, then fit()'s own product order (P G^T) Y as two MFMA passes
        # (edmdc_pinv_apply_dev: rows of W = G P^T, then W^T Y); and fit_multi() (:113-152: P (G^T Y), no apply pass)
        if not a.no_fit and world == 1:
            fit_legs = {}
            dec = engine.apply_decomposition(n, r, k)
            W_ = (k + 15) // 16 * 16 + (n + r + 15) // 16 * 16
            wrows_flop = dec["wrows_items_per_192_rows"] * 24 * 512.0 * W_ / 192.0          # executed MFMA flop per row of W
            wty_flop = dec["wty_tasks"] * 12288.0                                           # executed MFMA flop per pair of W^T Y
            # (a) What a user of the drop-in gets: KoopmanEDMDc(...).fit(X_host, U_host) itself -- host arrays in, upload included, the
            # default lift_cache=False -- as the first fit() of this process (its scratch arenas and task tables have not seen a fit yet;
            # the process itself is warm -- the cold first call of a fresh process is measured by the recorded_shape leg) and once more.  One trajectory of nb (L + 1) states (the class's fit() takes one; timing only).
            from bluerov2_dynamics_amd.Koopman.koopmanEDMDc import KoopmanEDMDc
            Xh_ = Xe.view(-1, n).cpu().numpy()
            Uh_ = np.zeros((Xh_.shape[0], r))
            Uh_[: nb * L] = Ue.view(-1, r).cpu().numpy()
            host_call = {}
            for tag in ("first_fit_of_this_process_s", "second_call_s"):
                mk = KoopmanEDMDc(state_dim=n, input_dim=r, n_rbfs=k, gamma=gamma, ridge=ridge)
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                mk.fit(Xh_, Uh_)
                host_call[tag] = time.perf_counter() - t0
            host_call.update(samples=int(Xh_.shape[0] - 1), samples_per_s_second_call=(Xh_.shape[0] - 1) / host_call["second_call_s"],
                             finite=bool(np.isfinite(mk.A_).all() and np.isfinite(mk.B_).all()),
                             note="KoopmanEDMDc.fit(X, U) with NumPy arrays: H2D upload of 1.6 GB, k-means with scikit-learn's stopping rule, "
                                  "G^T G, host solve (pinv='auto': numpy.linalg.pinv unless provably well conditioned), (P G^T) Y with a second lift (lift_cache off), "
                                  "download of A, B.  The process is warm by now (rollouts, Gram, k-means have run): a true first call in a fresh "
                                  "process is the recorded_shape leg's")
            # ... and fit_multi(X_list, U_list) on config 3 as the reference would hold it: a Python list of 20 000 separately allocated
            # (501, 12) / (501, 8) arrays (Koopman/koopmanEDMDc.py:113-152).  One upload (brov_upload_bags), one ragged Gram.
            X_list = [np.array(Xh_[b * (L + 1):(b + 1) * (L + 1)]) for b in range(nb)]
            Ue_h = Ue.cpu().numpy()
            U_list = [np.zeros((L + 1, r)) for b in range(nb)]             # aligned with X like the reference's U (its last row is never read)
            for b in range(nb):
                U_list[b][:L] = Ue_h[b]
            del Ue_h
            t0 = time.perf_counter()
            Xs_d, Us_d = torch.from_numpy(Xh_).to(dev), torch.from_numpy(Uh_).to(dev)
            torch.cuda.synchronize(dev)
            upload_s = time.perf_counter() - t0
            del Xs_d, Us_d
            fm = {}
            for tag in ("first_call_s", "second_call_s"):
                mk = KoopmanEDMDc(state_dim=n, input_dim=r, n_rbfs=k, gamma=gamma, ridge=ridge)
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                mk.fit_multi(X_list, U_list)
                fm[tag] = time.perf_counter() - t0
            fm.update(bags=nb, states_per_bag=L + 1, samples=nb * L, samples_per_s_second_call=nb * L / fm["second_call_s"],
                      plain_upload_of_the_stacked_arrays_s=upload_s, finite=bool(np.isfinite(mk.A_).all() and np.isfinite(mk.B_).all()),
                      note="KoopmanEDMDc.fit_multi(X_list, U_list) with a list of 20 000 separately allocated NumPy arrays per side: every bag goes "
                           "straight to its place in one device buffer (brov_upload_bags), k-means over all states, one ragged Gram call "
                           "(edmdc_gram_ragged_dev), host pinv, P (G^T Y)")
            host_call["fit_multi"] = fm
            del Xh_, Uh_, mk, X_list, U_list
            # (b) the same work on device-resident tensors (fit_dev), lifted rows kept in HBM between the two passes.  Warm-up (untimed,
            # like the warm-up launches of the headline): the 45.7 GB block that holds the lifted rows comes from torch's caching
            # allocator, whose first allocation of that size takes ~0.5 s
            engine.fit_dev(Xe.view(-1, n), Ue.view(-1, r), nb, L, k, gamma, ridge, order="fit", centers=Cc, ctx=ctx, lift_cache=True)
            for order in ("fit", "fit_multi"):
                tmf = {}
                ctx.set_timing(True)
                A_f, B_f, _ = engine.fit_dev(Xe.view(-1, n), Ue.view(-1, r), nb, L, k, gamma, ridge, order=order, max_iter=a.kmeans_iters,
                                             ctx=ctx, timings=tmf, lift_cache=True)
                apply_kernel_ms = ctx.last_kernel_ms() if order == "fit" else None
                ctx.set_timing(False)
                leg = {"fit_samples_per_s": pairs / tmf["total_s"], "wall_s": tmf["total_s"],
                       "stages_ms": {"centres_kmeanspp_plus_lloyd": tmf["centres_s"] * 1e3, "lift_plus_gram_plus_download": tmf["gram_s"] * 1e3,
                                     "host_pinv": tmf["pinv_s"] * 1e3,
                                     ("apply_lift_wrows_wty_plus_download" if order == "fit" else "host_P_times_GtY"): tmf["apply_s"] * 1e3},
                       "lloyd_iterations": tmf["lloyd_iterations"], "lloyd_max_iter": a.kmeans_iters, "lloyd_converged": tmf["lloyd_converged"],
                       "kmeanspp_ms_device": tmf.get("kmeanspp_ms"), "lloyd_ms_device": tmf.get("lloyd_ms"), "lloyd_loop_info": ctx.kmeans_loop_info(),
                       "lloyd_roofline": lloyd_roofline(nb * (L + 1), k, (tmf.get("lloyd_ms") or 0.0) / (tmf["lloyd_iterations"] + 1), tmf["lloyd_iterations"]),
                       "finite": bool(np.isfinite(A_f).all() and np.isfinite(B_f).all()),
                       "samples_per_s_excluding_centres": pairs / (tmf["total_s"] - tmf["centres_s"])}
                if order == "fit" and tmf.get("gram_kernel_ms"):
                    # fit()'s Gram pass is G^T G alone (the reference's fit never forms G^T Y): its own task table
                    t2, s2 = engine.gtg_decomposition(n, r, k)
                    gfl = pairs * t2 * 12288.0 / (tmf["gram_kernel_ms"] * 1e-3) / 1e12
                    leg["gram_pass_roofline"] = {"kernel": "lift_rows_kernel + gram_kernel (G^T G alone)", "bound": "mfma", "achieved": gfl,
                                                 "peak": PEAK_FP64_MFMA_TFLOPS, "unit": "TFLOP/s", "frac": gfl / PEAK_FP64_MFMA_TFLOPS,
                                                 "kernel_ms": tmf["gram_kernel_ms"], "tasks": t2, "slabs_per_chunk": s2,
                                                 "flop_per_sample": t2 * 12288.0, "traffic": None,
                                                 "note": "executed MFMA flop of the staircase over the G tiles / (lift + Gram) time"}
                if order == "fit":
                    aflops = pairs * (wrows_flop + wty_flop) / (apply_kernel_ms * 1e-3) / 1e12
                    leg["apply_kernel_ms"] = apply_kernel_ms
                    leg["roofline"] = {"kernel": "lift_rows_kernel + wrows_kernel + gram_kernel<W^T Y> (v_mfma_f64_16x16x4_f64)", "bound": "mfma",
                                       "achieved": aflops, "peak": PEAK_FP64_MFMA_TFLOPS, "unit": "TFLOP/s", "frac": aflops / PEAK_FP64_MFMA_TFLOPS,
                                       "kernel_ms": apply_kernel_ms, "flop_per_sample": wrows_flop + wty_flop,
                                       "wrows_flop_per_sample": wrows_flop, "wty_flop_per_sample": wty_flop, "decomposition": dec,
                                       "note": "executed MFMA flop of the two passes of (P G^T) Y / time of the whole apply pass (any re-lift included)",
                                       "traffic": pmc_traffic({"wrows": chunks, "wty_gram": chunks}, files=("r06_fit_pmc_summary.json", "r05_fit_pmc_summary.json", "r04_fit_pmc_summary.json", "r03_fit_pmc_summary.json")) if pairs == 10_000_000 else None,
                                       "algorithmic": {"flop_per_sample": 2.0 * p * p + 2.0 * p * d, "unit": "TFLOP/s",
                                                       "achieved": pairs * (2.0 * p * p + 2.0 * p * d) / (apply_kernel_ms * 1e-3) / 1e12}}
                    leg["ratio_to_full_gram_ms"] = (tmf["total_s"] - tmf["centres_s"]) * 1e3 / (ewall / a.edmdc_steps * 1e3)
                fit_legs[order] = leg
            if "fit_multi" in host_call:
                host_call["fit_multi"]["ratio_to_device_resident_leg_plus_upload"] = host_call["fit_multi"]["second_call_s"] / (
                    fit_legs["fit_multi"]["wall_s"] + host_call["fit_multi"]["plain_upload_of_the_stacked_arrays_s"])
            fit_legs["host_call"] = host_call
            fit_legs["config"] = {"workload": f"BASELINE config 3 data ({pairs} pairs in {nb} bags, n=12 r=8 k=512 gamma={gamma} ridge={ridge}); "
                                              f"'fit' / 'fit_multi' = engine.fit_dev on DEVICE-RESIDENT tensors with a warmed lift cache, 'host_call' = "
                                              f"KoopmanEDMDc.fit() on host arrays, cold and warm; KMeans stopping rule max_iter={a.kmeans_iters} "
                                              f"tol=1e-4; wall clock incl. host pinv and downloads"}
            out["edmdc_fit"] = fit_legs
        if not a.no_fit and not a.no_recorded and world == 1:
            out.setdefault("edmdc_fit", {})["recorded_shape"] = recorded_shape_leg(engine, _lib, ctx, dev, dt, not a.no_cpu)
        # ---- the same fit() sharded over the ranks (N > 1; weak scaling, 1e7 pairs per GPU): centres from rank 0's shard (already
        # broadcast above), local G^T G, all-reduce, the same host pinv on every rank, local (P G^T) Y, a second all-reduce of the
        # p x d block (dist.fit_sharded(order="fit")); identical A, B on every rank
        if not a.no_fit and world > 1:
            def ar2(x, y):
                allreduce_sum_(x)
                allreduce_sum_(y)
            Xs, Us = Xe.view(nb, L + 1, n), Ue.view(nb, L, r)
            bdist.fit_sharded(Xs, Us, Cc, gamma, ridge, order="fit", allreduce=ar2)       # warm-up (BLAS pool, task tables, code objects)
            barrier()
            # (round 4) the centres are part of it: KMeans over ALL ranks' states (Koopman/koopmanEDMDc.py:85 hands fit() every sample) --
            # k-means++ seeding with two small exchanges per centre, Lloyd with one integer all-reduce per iteration (dist.py)
            ktm = {}
            t0 = time.perf_counter()
            centres_error = None
            try:
                C_sh, inertia_sh, iters_sh = bdist.kmeans_centers_sharded(Xe.view(-1, n), k, max_iter=a.kmeans_iters, ctx=ctx, timings=ktm)
            except Exception as exc:          # (first run on >= 2 real GPUs happens at the driver: keep the other legs of the line alive)
                centres_error = f"{type(exc).__name__}: {exc}"
            torch.cuda.synchronize(dev)
            barrier()
            cwall = max_over_ranks(time.perf_counter() - t0)
            # every rank takes the same branch: one failed rank fails the centres for all (MAX of the flags), and a failed centres
            # stage can never produce a "centres included" throughput below
            centres_failed = max_over_ranks(1.0 if centres_error is not None else 0.0) > 0.0
            if centres_failed:
                C_sh, inertia_sh, iters_sh = Cc, None, None         # rank 0's centres, broadcast above: the same on every rank
                centres_error = centres_error or "another rank failed in kmeans_centers_sharded"
            t0 = time.perf_counter()
            A_s, B_s = bdist.fit_sharded(Xs, Us, C_sh, gamma, ridge, order="fit", allreduce=ar2)
            barrier()
            swall = max_over_ranks(time.perf_counter() - t0)
            chk = torch.tensor([float(np.abs(A_s).sum()), float(np.abs(B_s).sum())], dtype=torch.float64, device=dev)
            lo, hi = chk.clone(), chk.clone()
            if backend == "nccl":
                dist.all_reduce(lo, op=dist.ReduceOp.MIN); dist.all_reduce(hi, op=dist.ReduceOp.MAX)
            else:
                lo, hi = lo.cpu(), hi.cpu()
                dist.all_reduce(lo, op=dist.ReduceOp.MIN); dist.all_reduce(hi, op=dist.ReduceOp.MAX)
            if rank == 0:
                out["edmdc_fit_sharded"] = {
                    "metric": "fit_samples_per_s_given_centres" if centres_failed else "fit_samples_per_s_centres_included",
                    "value": world * pairs / swall if centres_failed else world * pairs / (cwall + swall), "unit": "samples/s",
                    "wall_s": None if centres_failed else cwall + swall, "centres_wall_s": None if centres_failed else cwall,
                    "centres_failed": centres_failed, "gram_pinv_apply_wall_s": swall,
                    "samples_per_s_given_centres": world * pairs / swall,
                    "kmeans": {"rows_total": world * nb * (L + 1), "k": k, "kmeanspp_s": ktm.get("kmeanspp_s"), "lloyd_s": ktm.get("lloyd_s"),
                               "lloyd_iterations": iters_sh, "max_iter": a.kmeans_iters, "inertia": inertia_sh,
                               "exchanges": "seeding: 2 small all-reduces per centre; Lloyd: 1 all-reduce of 2 k (n + 1) + 2 int64 words per iteration"},
                    "pairs_per_gpu": pairs, "ranks": world, "collectives_after_centres": 2,
                    "finite": bool(np.isfinite(A_s).all() and np.isfinite(B_s).all()),
                    "centres_error_rank0": centres_error,
                    "identical_on_all_ranks": bool(torch.equal(lo.cpu(), hi.cpu())),
                    "note": "KoopmanEDMDc.fit end to end on sharded data: KMeans over all ranks' states (sharded k-means++ and Lloyd, integer member "
                            "sums: the same centres on every rank), G^T G per rank + all-reduce + host pinv + (P G^T) Y per rank + all-reduce"}
        # f1: KoopmanEDMDc.multistep_rmse on the recorded-data size of the reference (45 823 samples, H = 100;
        # training/best_results.txt:801 logs 41.19 s for it on the authors' CPU) -- rank 0 only, host arrays in/out
        if rank == 0:
            Nm, Hm = min(45823, nb * L), 100              # the recorded size; smaller only when --edmdc-samples is
            Xm = Xe.view(-1, n)[: Nm].cpu().numpy()
            Um = Ue.view(-1, r)[: Nm].cpu().numpy()      # timing only: alignment across bag ends is irrelevant
            engine.multistep_se(Xm, Um, Cc.cpu().numpy(), gamma, A_, B_, Hm, ctx=ctx)     # warm-up: the same call (scratch size, streams, code objects)
            ctx.set_timing(True)
            t1 = time.perf_counter()
            se, _ = engine.multistep_se(Xm, Um, Cc.cpu().numpy(), gamma, A_, B_, Hm, ctx=ctx)
            wall_ms = (time.perf_counter() - t1) * 1e3
            kms = ctx.last_kernel_ms()
            ctx.set_timing(False)
            nw = Nm - Hm
            out["edmdc"]["multistep_rmse_H100"] = {
                "windows": nw, "H": Hm, "wall_ms_host_to_host": wall_ms, "kernel_ms": kms,
                "tflops": 2.0 * nw * d * p * Hm / (kms * 1e-3) / 1e12, "finite": bool(np.isfinite(se)),
                "note": "lift + 100 fp64 MFMA GEMM steps + endpoint error; reference CPU log: 41.19 s"}
            # the opt-in one-pass form (explicit powers of A: engine.multistep_se_linear), same data
            engine.multistep_se_linear(Xm, Um, Cc.cpu().numpy(), gamma, A_, B_, Hm, ctx=ctx)
            ctx.set_timing(True)
            t1 = time.perf_counter()
            se_l, _ = engine.multistep_se_linear(Xm, Um, Cc.cpu().numpy(), gamma, A_, B_, Hm, ctx=ctx)
            wall_l = (time.perf_counter() - t1) * 1e3
            kms_l = ctx.last_kernel_ms()
            ctx.set_timing(False)
            out["edmdc"]["multistep_rmse_H100"]["linear"] = {
                "wall_ms_host_to_host": wall_l, "kernel_ms": kms_l, "rel_diff_se": abs(se_l - se) / max(abs(se), 1e-300),
                "note": "method='linear' (opt-in): x_hat = (E A^H) phi(x) + sum_t (E A^(H-1-t) B) u in one pass; host forms the H coefficient blocks"}
            # K3: multistep_rmse_endpoint_physics (Fossen thruster model, carried lag) at the same size; the reference's own
            # log has 1247 s for H = 100 with the Euler integrator
            wt = {}
            for integ in ("euler", "rk4"):
                ctx.set_timing(True)
                t1 = time.perf_counter()
                rm = engine.window_rmse(_lib.THRUSTER_EULER, integ, Xm, Um, Hm, dt, ctx=ctx)
                wt[integ] = {"wall_ms_host_to_host": (time.perf_counter() - t1) * 1e3, "kernel_ms": ctx.last_kernel_ms(), "rmse_finite": bool(np.isfinite(rm))}
                ctx.set_timing(False)
            out["fossen_window_rmse_H100"] = {"windows": nw, "H": Hm, **wt, "note": "reference CPU log: 1247 s (Euler)"}
        if rank == 0 and not a.no_cpu and world == 1:
            out["edmdc"]["cpu_baseline"] = cpu_baseline_gram(Cc.cpu().numpy(), gamma, a.cpu_seconds / 2)
        del Xe, Ue, GG, GtG, GtY
        torch.cuda.empty_cache()

    # ------------------------------------------------------------------ config 4: the sharded ensemble (strong scaling)
    if a.full and not a.no_cfg4:
        Bt, T4 = a.cfg4_rollouts, a.cfg4_horizon
        b0, b1 = bdist.shard_range(Bt, rank, world)
        Bl = b1 - b0
        k4 = 512
        p4, d4 = n + k4 + r, n + k4
        U4 = torch.empty((Bl, T4, r), dtype=torch.float64, device=dev)
        X4 = torch.empty((Bl, T4 + 1, n), dtype=torch.float64, device=dev)
        x40 = torch.zeros((Bl, n), dtype=torch.float64, device=dev)
        x40[:, 2] = 5.0
        GG4 = torch.zeros((p4 * p4 + p4 * d4,), dtype=torch.float64, device=dev)
        G4, Y4 = GG4[: p4 * p4].view(p4, p4), GG4[p4 * p4:].view(p4, d4)
        engine.fill_controls_dev(U4, "btu", "ar1", seed=0xC0F4, b0=b0, T_total=T4, ctx=ctx)     # value depends on the GLOBAL trajectory index only
        fe = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        fe[0].record()
        engine.fill_controls_dev(U4, "btu", "ar1", seed=0xC0F4, b0=b0, T_total=T4, ctx=ctx)     # (the same values again: timed)
        fe[1].record()
        torch.cuda.synchronize()
        fill_ms = fe[0].elapsed_time(fe[1])

        def roll4():
            engine.rollout_dev(_lib.THRUSTER_EULER, "rk4", x40, U4, dt, traj=X4, layout="btu", stride=1, ctx=ctx)

        roll4()
        # centres: from the first 2048 trajectories of the ensemble, which rank 0 owns at every world size <= 512, so the
        # centres -- and with them the summed Gram -- do not depend on the sharding
        C4 = torch.empty((k4, n), dtype=torch.float64, device=dev)
        if rank == 0:
            nbc = min(2048, Bl)
            Ck, _, _ = engine.kmeans_centers_dev(X4[:nbc].reshape(-1, n), k4, random_state=0, max_iter=5, ctx=ctx)
            C4.copy_(Ck)
        if world > 1:
            if backend == "nccl":
                dist.broadcast(C4, 0)
            else:
                Ch = C4.cpu()
                dist.broadcast(Ch, 0)
                C4.copy_(Ch)
        barrier()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        t0 = time.perf_counter()
        ev[0].record()
        roll4()
        ev[1].record()
        engine.gram_dev(X4.view(-1, n), U4.view(-1, r), C4, gamma, Bl, T4, T4 + 1, T4, G4, Y4, ctx=ctx)
        ev[2].record()
        allreduce_sum_(GG4)
        ev[3].record()
        torch.cuda.synchronize()
        local_s = time.perf_counter() - t0
        barrier()
        wall4 = max_over_ranks(time.perf_counter() - t0)
        per_rank = gather_ranks(local_s * 1e3)
        roll_ms, gram_ms, ar_ms = ev[0].elapsed_time(ev[1]), ev[1].elapsed_time(ev[2]), ev[2].elapsed_time(ev[3])
        # independent check of the summed blocks: their x-x corners are plain sums over all pairs of the ensemble,
        # recomputed here with torch matmuls on every rank's shard and summed over the ranks
        chk = torch.zeros(2 * n * n, dtype=torch.float64, device=dev)
        for i0 in range(0, Bl, 32768):                     # in slices; one small product per trajectory (a single 12 x 12 x 16M
            Xa, Xb = X4[i0:i0 + 32768, :-1, :], X4[i0:i0 + 32768, 1:, :]        # product runs in one workgroup: 1.7 s each)
            chk[: n * n] += torch.bmm(Xa.transpose(1, 2), Xa).sum(0).reshape(-1)
            chk[n * n:] += torch.bmm(Xa.transpose(1, 2), Xb).sum(0).reshape(-1)
        allreduce_sum_(chk)
        cgg, cgy = chk[: n * n].view(n, n), chk[n * n:].view(n, n)
        e_gg = float(((G4[:n, :n] - cgg).norm() / cgg.norm()).item())
        e_gy = float(((Y4[:n, :n] - cgy).norm() / cgy.norm()).item())
        pairs4 = Bt * T4
        roll_max = max(gather_ranks(roll_ms))          # collectives: every rank, same order
        gram_max = max(gather_ranks(gram_ms))
        if rank == 0:
            Gh = G4.cpu().numpy()
            out["config4"] = {
                "metric": "ensemble_rollout_plus_gram", "scaling": "strong", "total_rollouts": Bt, "horizon": T4, "rollouts_this_rank": Bl,
                "rccl_ranks": dist.get_world_size() if world > 1 else 1, "backend": ("rccl (torch.distributed nccl)" if backend == "nccl" else backend) if world > 1 else "none (single rank)",
                "wall_ms": wall4 * 1e3, "per_rank_ms": per_rank,
                "rank0_ms": {"rollout_rk4_btu": roll_ms, "lift_plus_gram": gram_ms, "allreduce_4.5MB": ar_ms},
                "rollout_steps_per_s": Bt * T4 / (roll_max * 1e-3),
                # caller-layout ([B][T][c]) kernels of this leg against HBM: 64 B in + 96 B out per step; 64 B written per step by the fill
                "rollout_hbm_frac": Bl * T4 * 160.0 / (roll_ms * 1e-3) / 1e9 / PEAK_HBM_GBS,
                "fill_ar1_ms": fill_ms, "fill_hbm_frac": Bl * T4 * 64.0 / (fill_ms * 1e-3) / 1e9 / PEAK_HBM_GBS,
                **cfg4_counter_terms(Bl, T4, roll_ms, fill_ms),
                "gram_samples_per_s": pairs4 / (gram_max * 1e-3),
                "pairs_total": pairs4,
                "verified": {"GtG_xx_vs_torch_rel": e_gg, "GtY_xx_vs_torch_rel": e_gy, "ok": bool(e_gg < 1e-11 and e_gy < 1e-11),
                             "note": "x-x corners of the all-reduced blocks against X^T X / X^T X+ from torch matmuls summed over the ranks"},
                "gram_fingerprint": {"trace_GtG": float(np.trace(Gh)), "sum_GtY": float(Y4.sum().item()), "GtG_00": float(Gh[0, 0]),
                                     "GtG_rbf0_rbf0": float(Gh[n, n]), "frobenius_GtG": float(np.linalg.norm(Gh)),
                                     "note": "the ensemble, its command stream and the centres do not depend on the sharding: these numbers "
                                             "agree to ~1e-12 relative between runs at 1/2/4/8 GPUs (summed Gram == 1-GPU Gram)"},
                "config": {"workload": f"BASELINE config 4: {Bt} rollouts x {T4} RK4 steps in total (AR(1) commands, stream 0xC0F4), contiguous shards over the "
                                       f"ranks, trajectories stored [B][T+1][12], local lift + G^T[G|Y] (k=512) per rank, one all-reduce of {p4 * p4 + p4 * d4} doubles"},
            }
        del U4, X4, GG4, G4, Y4, Xa, Xb, chk
        torch.cuda.empty_cache()

    if a.full and rank == 0 and not a.no_cpu:
        # (N > 1: rank 0 times the same bounded host samples after every timed region; the other ranks have nothing left to do
        # but wait at the final barrier)
        out["cpu_baseline"] = cpu_baseline_rollout(a.cpu_seconds, a.integrator)
        out["cpu_baseline_reference_shape"] = cpu_baseline_reference_shape(a.cpu_seconds, a.integrator)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()
    if rank == 0:
        details = None
        if a.full:
            out["cpu_seconds_budget_per_leg"] = a.cpu_seconds
            details = write_details(out, a.details)
        line = json.dumps(compact_line(out, details), separators=(",", ":"))
        assert len(line) <= MAX_LINE_BYTES, len(line)
        sys.stdout.flush()
        os.write(json_fd, (line + "\n").encode())


MAX_LINE_BYTES = 4096        # the driver parses the ONE stdout line; round 5's 25 KB line came back unparsed (BENCH_r05.json: parsed null)


def write_details(out, path):
    """Everything the legs measured (per-launch times, child-process dumps, notes) as JSON in a file; the stdout line carries
    the contract fields and a flat summary only.  Returns the path written, relative to the repo when inside it."""
    path = path or os.path.join(REPO, "bench_details.json")
    try:
        with open(path, "w") as f:
            json.dump(out, f, indent=1)
        scratch = os.path.join(REPO, "gpurun_out")
        if os.path.isdir(scratch) and os.path.dirname(os.path.abspath(path)) == REPO:       # scratch dir of the GPU box: merged back to the builder
            with open(os.path.join(scratch, os.path.basename(path)), "w") as f:
                json.dump(out, f, indent=1)
    except OSError as exc:
        sys.stderr.write(f"bench.py: could not write {path}: {exc}\n")
        return None
    sys.stderr.write(f"bench.py: full record of every leg in {path}\n")
    return os.path.relpath(path, REPO) if os.path.abspath(path).startswith(REPO + os.sep) else path


def _sig(x, digits=6):
    """numbers of the stdout line: 6 significant digits (the full-precision values are in the details file)"""
    if isinstance(x, bool) or x is None or isinstance(x, (int, str)):
        return x
    if isinstance(x, float):
        return float(f"{x:.{digits}g}") if np.isfinite(x) else None
    if isinstance(x, (list, tuple)):
        return [_sig(v, digits) for v in x]
    if isinstance(x, dict):
        return {k: _sig(v, digits) for k, v in x.items()}
    return _sig(float(x), digits)


def _get(o, *path):
    for k in path:
        if not isinstance(o, dict) or k not in o:
            return None
        o = o[k]
    return o


def compact_line(out, details_path):
    """The ONE stdout line: the driver's contract fields, `config`, `roofline` of the dominant kernel, `cpu_baseline`, whether the timed
    launches were verified, and a flat `summary` of the other legs' headline numbers -- at most MAX_LINE_BYTES."""
    rf = out["roofline"]
    tr = rf.get("traffic")
    line = {k: out[k] for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
                                "vs_baseline", "dtype", "data")}
    cfg = out["config"]
    line["config"] = {"workload": cfg["workload"], "trajectories_per_gpu": cfg["trajectories_per_gpu"], "horizon": cfg["horizon"],
                      "parallelism": cfg["parallelism"]}
    line["roofline"] = {"kernel": rf["kernel"], "bound": rf["bound"], "achieved": rf["achieved"], "peak": rf["peak"], "unit": rf["unit"],
                        "frac": rf["frac"], "kernel_ms": rf["kernel_ms"],
                        "traffic": ({"bytes": tr["bytes"], "stale": tr["stale"], "source": tr["source"].split(" ")[0]} if tr else None),
                        "hbm_frac": _get(rf, "terms", "hbm", "frac"), "issue_frac": _get(rf, "terms", "valu_fp64_issue", "frac"),
                        "algorithmic_bytes_per_launch": rf.get("algorithmic_bytes_per_launch")}
    cb = out.get("cpu_baseline")
    if cb:
        line["cpu_baseline"] = {k: cb[k] for k in ("value", "unit", "cores", "kind", "sample")}
        line["cpu_baseline"]["budget_s"] = out.get("cpu_seconds_budget_per_leg")
    if "verified" in out:
        line["verified"] = {"ok": out["verified"]["ok"], "max_rel_err": out["verified"]["max_rel_err"], "tolerance": out["verified"]["tolerance"]}
    s = {}

    def put(key, *path, scale=1.0):
        v = _get(out, *path)
        if isinstance(v, (int, float)) and not isinstance(v, bool):
            s[key] = v * scale if scale != 1.0 else v
        elif v is not None:
            s[key] = v

    put("cpu_reference_shape_steps_per_s", "cpu_baseline_reference_shape", "value")
    put("rollout_ar1_steps_per_s", "rollout_ar1", "value")
    for name in ("rk4_endpoint_only", "euler_stored", "euler_endpoint_only"):
        put(f"{name}_steps_per_s", "rollout_variants", name, "value")
        put(f"{name}_frac", "rollout_variants", name, "roofline", "frac")
    rv = out.get("rollout_variants")
    if rv:
        s["rollout_variants_verified"] = all(_get(v, "verified", "ok") is True for v in rv.values())
    put("gram_samples_per_s", "edmdc", "value")
    put("gram_pairs_per_gpu", "edmdc", "pairs_per_gpu")
    put("gram_mfma_frac", "edmdc", "roofline", "frac")
    put("gram_kernel_ms", "edmdc", "roofline", "kernel_ms")
    put("gram_traffic_bytes", "edmdc", "roofline", "traffic", "bytes")
    put("gram_cpu_samples_per_s", "edmdc", "cpu_baseline", "value")
    put("gram_cpu_cores", "edmdc", "cpu_baseline", "cores")
    put("kmeans_lloyd_ms", "edmdc", "kmeans", "lloyd_ms_total")
    put("kmeans_lloyd_iterations", "edmdc", "kmeans", "lloyd_iterations")
    put("kmeanspp_ms", "edmdc", "kmeans", "kmeanspp_ms_device")
    put("multistep_H100_kernel_ms", "edmdc", "multistep_rmse_H100", "kernel_ms")
    put("multistep_H100_tflops", "edmdc", "multistep_rmse_H100", "tflops")
    put("multistep_H100_wall_ms", "edmdc", "multistep_rmse_H100", "wall_ms_host_to_host")
    put("multistep_H100_linear_wall_ms", "edmdc", "multistep_rmse_H100", "linear", "wall_ms_host_to_host")
    put("fossen_window_H100_euler_kernel_ms", "fossen_window_rmse_H100", "euler", "kernel_ms")
    put("fossen_window_H100_rk4_kernel_ms", "fossen_window_rmse_H100", "rk4", "kernel_ms")
    put("fit_samples_per_s", "edmdc_fit", "fit", "fit_samples_per_s")
    put("fit_wall_s", "edmdc_fit", "fit", "wall_s")
    put("fit_apply_mfma_frac", "edmdc_fit", "fit", "roofline", "frac")
    put("fit_gtg_mfma_frac", "edmdc_fit", "fit", "gram_pass_roofline", "frac")
    put("fit_multi_samples_per_s", "edmdc_fit", "fit_multi", "fit_samples_per_s")
    put("fit_host_arrays_second_call_s", "edmdc_fit", "host_call", "second_call_s")
    put("fit_multi_host_list_second_call_s", "edmdc_fit", "host_call", "fit_multi", "second_call_s")
    put("fit_multi_host_list_samples_per_s", "edmdc_fit", "host_call", "fit_multi", "samples_per_s_second_call")
    rs = _get(out, "edmdc_fit", "recorded_shape")
    if rs:
        put("recorded_rows", "edmdc_fit", "recorded_shape", "rows_logged_by_the_reference")
        put("recorded_samples_per_s_warm", "edmdc_fit", "recorded_shape", "value")
        for mode, run in (rs.get("first_calls") or {}).items():
            s[f"recorded_first_fit_s_{mode}"] = run.get("first_call_s")
            s[f"recorded_warm_fit_s_{mode}"] = run.get("warm_call_s")
            s[f"recorded_process_start_to_fit_done_s_{mode}"] = run.get("process_start_to_first_fit_done_s")
        put("recorded_AB_bit_equal_across_modes", "edmdc_fit", "recorded_shape", "AB_bit_equal_across_modes")
        put("recorded_csv_script_start_to_fit_done_s", "edmdc_fit", "recorded_shape", "csv_script_start", "plain", "process_start_to_first_fit_done_s")
        put("recorded_csv_script_start_to_fit_done_s_warm_up", "edmdc_fit", "recorded_shape", "csv_script_start", "warm_up", "process_start_to_first_fit_done_s")
        put("recorded_cpu_fit_s", "edmdc_fit", "recorded_shape", "cpu_baseline", "second_call_s")
        put("recorded_cpu_first_fit_s", "edmdc_fit", "recorded_shape", "cpu_baseline", "first_call_s")
        put("recorded_cpu_cores", "edmdc_fit", "recorded_shape", "cpu_baseline", "cores")
    put("fit_sharded_samples_per_s", "edmdc_fit_sharded", "value")
    put("fit_sharded_identical_on_all_ranks", "edmdc_fit_sharded", "identical_on_all_ranks")
    put("fit_sharded_centres_failed", "edmdc_fit_sharded", "centres_failed")
    c4 = out.get("config4")
    if c4:
        put("cfg4_total_rollouts", "config4", "total_rollouts")
        put("cfg4_horizon", "config4", "horizon")
        put("cfg4_rccl_ranks", "config4", "rccl_ranks")
        put("cfg4_backend", "config4", "backend")
        put("cfg4_wall_ms", "config4", "wall_ms")
        put("cfg4_per_rank_ms", "config4", "per_rank_ms")
        put("cfg4_rollout_ms", "config4", "rank0_ms", "rollout_rk4_btu")
        put("cfg4_gram_ms", "config4", "rank0_ms", "lift_plus_gram")
        put("cfg4_allreduce_ms", "config4", "rank0_ms", "allreduce_4.5MB")
        put("cfg4_rollout_steps_per_s", "config4", "rollout_steps_per_s")
        put("cfg4_rollout_hbm_frac", "config4", "rollout_hbm_frac")
        put("cfg4_fill_ms", "config4", "fill_ar1_ms")
        put("cfg4_fill_hbm_frac", "config4", "fill_hbm_frac")
        put("cfg4_fill_issue_frac", "config4", "fill_issue_frac")
        put("cfg4_rollout_issue_frac", "config4", "rollout_issue_frac")
        put("cfg4_rollout_hbm_measured_frac", "config4", "rollout_hbm_measured_frac")
        put("cfg4_gram_samples_per_s", "config4", "gram_samples_per_s")
        put("cfg4_verified", "config4", "verified", "ok")
        put("cfg4_gram_trace", "config4", "gram_fingerprint", "trace_GtG")
    for k in ("roofline", "cpu_baseline", "verified"):
        if k in line:
            line[k] = _sig(line[k])
    line["summary"] = _sig(s)
    line["details"] = details_path
    line["value"], line["ms_per_step"] = _sig(line["value"], 12), _sig(line["ms_per_step"], 12)
    # never over the limit: the summary gives way first (its numbers are in the details file), then the long strings
    while len(json.dumps(line, separators=(",", ":"))) > MAX_LINE_BYTES and line["summary"]:
        line["summary"].popitem()
    if len(json.dumps(line, separators=(",", ":"))) > MAX_LINE_BYTES:
        line["config"]["workload"] = line["config"]["workload"][:200]
        if "cpu_baseline" in line:
            line["cpu_baseline"]["sample"] = line["cpu_baseline"]["sample"][:160]
    return line


if __name__ == "__main__":
    main()
