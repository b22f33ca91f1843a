"""Case lists of the shape sweeps over the population-rollout, closed-loop, MPPI, Koopman-MPPI and population-window kernels, over
the EDMDc kernels (lift, Gram, pinv_apply, the two multistep evaluators, simulate), and over the UKF and Koopman-QP kernels.  Not
collected; pure NumPy; imports no GPU code.

One generator per family: NAME(seed) returns an ordered list of plain dicts (ints, bools, strings and lists of them), the
hand-written corner list first, then seeded random draws from the family's value sets.  The lists depend on the seed alone, never on
a clock: tests/test_sweep_cases_cpu.py pins a hash of each.  A case holds shapes, switches, vehicle names and the seed of its data;
tests/sweep_run.py turns it into arrays, runs the reference and compares.  draw_NAME(rng, names...) is one random case, which
tests/stress_parity.py calls with its own generator.

The value sets are the smallest shapes at which the kernels' grid rules, knot arithmetic, counter addressing and reductions can go
wrong: both sides of every block edge (64 lanes when B or K <= 64, 256 otherwise; 64 / 128 / 256 lanes by M nu in the Koopman cost
kernel), partial and full last knots, hold >= H, a set-point against a reference window, more than one trip of the 256-wide
strided loops (K = 513), the 64-window chunks of the lag scan.  The EDMDc families (second half of the file) add the 64-row / 256-centre
blocks of the lift, every tile count of the Gram's task packing, bags and chunk edges, the 192-row unit of the apply pass, window
blocks of 128 with the two-stream split from 16 blocks on, and both parities of the propagation's K-steps.  The last two families are
the unscented Kalman filter (ukf: the eight instantiations of csrc/ukf.hip, each with a full block of UKF_WAVES = 4 recordings and
with a ragged one, B = 1 .. 9, T = 1 .. 12, one noise record or one per candidate, rows with every component measured and recordings
with none, components with r = +inf, process variances of 0, the yaw through pi) and the QP of the Koopman linear MPC (lmpc: Nv on
both sides of every rows-per-lane step of csrc/koopman_qp.hip and of its LDS / global switch, a non-zero Nv % 8 at every step, H + 1
on both sides of the 64-lane trips of the epilogue, hold r on both sides of the 64-lane trip of the u_apply loop, short last knots,
iters 0 .. 40 and a residual stop at two, three and five rows per lane).  The k-means families (colstats, kmeanspp, lloyd; the end of
the file) walk csrc/colstats.hip, the seeding and Lloyd's loop of csrc/kmeans.hip: every operand form (host, device, strided rows, a
column block of a wider table on and off a 16-byte boundary), data scales 1e-13 .. 1e13, far column means, a constant column, the
block, chunk and row edges of the seeding, and for the loop every kernel its dispatch rules pick (csrc/capi.hip:
edmdc_kmeans_lloyd_dev), every stopping rule and every empty-cluster rule.  The last family is the unscented RTS smoother (smooth: the
eight TAPE = true instantiations of ukf_filter_kernel, each with a full and a ragged block, ukf_rts_kernel and the chunked
brov_ukf_smooth; the shapes of ukf plus B = 13, T = 1, 2, 3 with and without a terminal pair, a tape budget with room for 4, 8 or 5
recordings -- chunks 4 + 4 + 1, 8 + 5, 4 + 4 + 4 + 1, 5 rounded down to 4, nrec = P = 3 in chunks -- and strict subsets of the outputs).
The two families after it are the multiplicative filter and the smoother of the quaternion model (ukf_quat: the four instantiations of
ukf_quat_filter_kernel; smooth_quat: its TAPE forms, ukf_quat_rts_kernel and the chunked brov_ukf_smooth_quat with the 313-double
record): the shapes of ukf and smooth plus starts anywhere on the sphere, inverted with the yaw next to pi, near vertical, q_w < 0,
an attitude block of P0 wide enough for the sigma points to leave the chart's linear range, and r = +inf on an attitude component."""
import hashlib
import json

import numpy as np

NAMES = ("V0", "V1", "V2", "V3", "V4", "V5", "V6", "V7", "V8")      # tests/fossen_vehicles.py: NAMES
WRENCH_NAMES = ("V0", "V1", "V2", "V4", "V5", "V7")                 # tests/fossen_vehicles.py: WRENCH_NAMES
N_CASES = 48                                                        # per family: four slices of 12
N_CASES_EDMDC = 32                                                  # per EDMDc family: four slices of 8 (corner lists of 12 to 24)
N_CASES_FILTER = 32                                                 # ukf, lmpc, smooth, ukf_quat, smooth_quat: four slices of 8 (corners: 17, 26, 20, 16, 20)
N_CASES_KMEANS = 32                                                 # colstats, kmeanspp, lloyd: four slices of 8
SEED = 2024

SETS = dict(
    rollout_pop=dict(model=(0, 1, 2), integ=("euler", "rk4"), lag_mode=(0, 1), P=(1, 2, 5), B=(1, 2, 63, 64, 65, 255, 256, 257, 300),
                     T=(0, 1, 2, 3, 7, 65), stride=("1", "2", "T", "T+1"), store=(True, False), per_candidate=(True, False),
                     lag=(True, False)),
    feedback=dict(model=(0, 1, 2), integ=("euler", "rk4"), lag_mode=(0, 1), P=(1, 2, 5), B=(1, 2, 63, 64, 65, 255, 256, 257, 300),
                  T=(0, 1, 2, 3, 7, 24, 65, 130), hold=("1", "2", "3", "5", "T+1"), ref=("set", "T"), u_ff=(True, False), z=(True, False),
                  lag=(True, False), gain_sets=(True, False), stride=("1", "2", "T", "T+1"), store=(True, False)),
    mppi=dict(model=(0, 1, 2), integ=("euler", "rk4"), lag_mode=(0, 1), B=(1, 2, 3), nparams=("1", "B"),
              K=(1, 2, 63, 64, 65, 255, 256, 257, 300, 513), H=(1, 2, 5, 7, 12), hold=("1", "2", "3", "H", "H+2"), rows=("1", "H+1", "H+4"),
              shift=(True, False), eps=(True, False)),
    koopman_mppi=dict(n=(12, 13), r=(6, 8), k=(0, 5, 20), Mr=(6, 8, 36, 40, 42, 72, 78, 80, 84),
                      K=(1, 63, 64, 65, 127, 128, 129, 255, 256, 257, 300), B=(1, 2, 3), rows=("1", "H+1", "H+4"), shift=(True, False),
                      eps=(True, False)),
    window_pop=dict(model=(0, 1, 2), integ=("euler", "rk4"), carry=(True, False), P=(1, 2, 9), H=(1, 2, 5, 12),
                    nwin=(1, 2, 63, 64, 65, 127, 128, 129, 257), nbags=(1, 2, 3, 4, 5), short_u=(True, False)),
    lift=dict(N=(1, 63, 64, 65, 130), k=(1, 255, 256, 257, 513), n=(1, 5, 12, 13, 16), gamma=(0.3, 3.0), scale=(0.5, 3.0, 12.0)),
    gram=dict(nr=((12, 8), (13, 8), (12, 10), (13, 6), (9, 4), (5, 2), (12, 0), (12, 1)),
              k=(1, 15, 16, 17, 31, 32, 33, 48, 64, 80, 96, 112, 160, 257, 512, 513), gamma=(0.3, 1.0, 3.0),
              form=("host", "ragged_dev", "uniform_dev"), gty=(True, False), chunk=(64, 100, 257, 0), short_u=(True, False)),
    pinv_apply=dict(nr=((12, 8), (12, 6), (13, 6), (9, 4), (5, 2), (13, 8)), k=(1, 7, 16, 17, 48, 64, 80, 96, 100, 160, 257, 512, 530),
                    gamma=(0.3, 1.0, 3.0), form=("host", "ragged_dev", "uniform_dev"), chunk=(64, 192, 257)),
    multistep=dict(shape=((1, 1, 1), (2, 3, 3), (12, 35, 8), (12, 36, 9), (13, 36, 6), (12, 83, 8), (13, 84, 8), (12, 8, 0), (5, 8, 2), (9, 4, 6)),
                   nw=(0, 1, 127, 128, 129, 255, 256, 257, 1920, 1921, 2176), H=(0, 1, 2, 3, 7), short_u=(True, False)),
    simulate=dict(shape=((1, 1, 1), (2, 3, 3), (12, 35, 8), (12, 36, 9), (13, 36, 6), (12, 83, 8), (13, 84, 8), (12, 8, 0), (5, 8, 2), (9, 4, 6)),
                  nb=(1, 2, 127, 128, 129, 255, 256, 257, 300), T=(0, 1, 2, 3, 7, 50)),
    ukf=dict(model=(0, 1), integ=("euler", "rk4"), lag_mode=(0, 1), lag=(True, False), P=(1, 2, 3), nrec=("1", "P"), alpha=(0.5, 1.0),
             B=(1, 3, 4, 5, 8, 9), T=(1, 2, 3, 12), measured=("std", "all", "none"), r_inf=(0, 1, 3), q_zero=(True, False),
             wrap=(True, False)),
    lmpc=dict(n=(12, 13), r=(6, 8), k=(0, 5, 70),
              Nv=(6, 8, 64, 66, 88, 90, 96, 126, 128, 132, 136, 192, 198, 200, 256, 258, 264, 306, 312), hold=(1, 2, 3, 8, 9, 10, 11),
              H=(1, 3, 7, 12, 15, 25, 31, 33, 34, 39, 43, 48, 51, 63, 64, 65, 101, 121, 127, 128, 129), nb=(1, 3, 4, 5, 8, 9),
              iters=(0, 1, 2, 40), traj=(True, False), y=(True, False), shift=(True, False),
              special=(None, "quat_flip", "angle_wrap", "warm")),
    colstats=dict(N=(1, 2, 63, 64, 65, 255, 256, 257, 1023, 1025, 262401), n=(1, 2, 3, 12, 13, 16),
                  form=("host", "dev", "dev_stride", "block_odd", "block_even"), scale=(1e-4, 1.0, 50.0, 1e4), order=("walk", "shuffled", "blobs"),
                  offset=(True, False), const_col=(True, False), null=("none", "mean", "var")),
    kmeanspp=dict(N=(1, 15, 16, 17, 60, 4095, 4096, 4097, 8191, 8192, 8193, 12289, 70001), k=(1, 2, 3, 7, 8, 9, 20, 60, 64, 512),
                  trials=("1", "sk", "16"), n=(1, 2, 5, 12, 13, 16), mean=(True, False),
                  form=("host", "dev", "dev_stride", "block_odd", "block_even"), scale=(1e-4, 1.0, 1e4), order=("walk", "shuffled", "blobs"),
                  offset=(True, False), const_col=(True, False), first=("0", "N-1"), ind=(True, False)),
    lloyd=dict(N=(1, 63, 64, 65, 1023, 1024, 1025, 16385, 262143, 262144, 262145, 264193, 1048576), n=(1, 2, 5, 12, 13, 14, 15),
               k=(1, 2, 63, 64, 65, 128, 256, 512, 513, 600, 1024, 1200), stop=("max_iter", "strict", "shift"),
               init=("rows", "dup", "far2", "far3", "allzero"), form=("host", "dev", "dev_stride", "block_odd", "block_even"),
               scale=(1e-13, 1e-4, 1.0, 50.0, 1e4, 1e13), order=("walk", "shuffled", "blobs"), offset=(True, False), const_col=(True, False)),
    smooth=dict(model=(0, 1), integ=("euler", "rk4"), lag_mode=(0, 1), lag=(True, False), P=(1, 2, 3), nrec=("1", "P"), alpha=(0.5, 1.0),
                B=(1, 3, 4, 5, 8, 9, 13), T=(1, 2, 3, 12), measured=("std", "all", "none"), r_inf=(0, 1, 3), q_zero=(True, False),
                wrap=(True, False), chunk=("whole", 4, 8, 5), terminal=(True, False), want=("all", "xs+sinfo", "Ps0", "pstd_s+Ps")),
    ukf_quat=dict(integ=("euler", "rk4"), P=(1, 2, 3), nrec=("1", "P"), alpha=(0.5, 1.0), B=(1, 3, 4, 5, 8, 9, 13), T=(1, 2, 3, 12),
                  measured=("std", "all", "none"), r_inf=(0, 1, 3), q_zero=(True, False), attitude=("level", "vertical", "sphere", "inverted"),
                  spread=("std", "wide")),
    smooth_quat=dict(integ=("euler", "rk4"), P=(1, 2, 3), nrec=("1", "P"), alpha=(0.5, 1.0), B=(1, 3, 4, 5, 8, 9, 13), T=(1, 2, 3, 12),
                     measured=("std", "all", "none"), r_inf=(0, 1, 3), q_zero=(True, False), attitude=("level", "vertical", "sphere", "inverted"),
                     spread=("std", "wide"), chunk=(0, 1, 2, 1.5), terminal=(True, False), want=("all", "xs+sinfo", "Ps0", "pstd_s+Ps")),
)


def _sym(v, **names):
    """the number behind a symbolic value such as "T+1" or "H" """
    return int(eval(v, {"__builtins__": {}}, names)) if isinstance(v, str) else int(v)


def _pick(rng, values):
    return values[int(rng.integers(0, len(values)))]


def _vehicles(rng, model, P):
    pool = NAMES if model == 0 else WRENCH_NAMES
    return [pool[int(i)] for i in rng.integers(0, len(pool), P)]


def digest(cases):
    """hash of a case list: what tests/test_sweep_cases_cpu.py pins"""
    return hashlib.sha256(json.dumps(cases, sort_keys=True).encode()).hexdigest()[:16]


# ------------------------------------------------------------------------------------------ population rollouts
def _rollout_pop(rng, model, integ, lag_mode, P, B, T, stride, store, per_candidate, lag):
    """stride as a symbol of T; lag_mode 1 is the thruster model's under RK4 only, a lag the thruster model's only"""
    T = int(T)
    return dict(family="rollout_pop", model=model, integ=integ, lag_mode=lag_mode if (model == 0 and integ == "rk4") else 0, P=P, B=B, T=T,
                stride=max(_sym(stride, T=T), 1), stride_as=stride, store=bool(store), per_candidate=bool(per_candidate),
                lag=bool(lag and model == 0), names=_vehicles(rng, model, P), seed=int(rng.integers(0, 1 << 30)))


ROLLOUT_POP_CORNERS = (
    # model integ  lag_mode P  B    T   stride store  per_candidate lag
    (0, "rk4", 0, 5, 64, 7, "1", True, True, True),            # B = 64 (the 64-lane blocks) with P = 5 and per-candidate inputs
    (0, "rk4", 1, 2, 65, 7, "T+1", True, False, True),         # B = 65 (the 256-lane blocks) with a stride past the horizon
    (0, "euler", 0, 2, 63, 0, "1", True, False, True),         # an empty horizon with a start lag
    (1, "rk4", 0, 1, 1, 1, "1", True, False, False),
    (2, "euler", 0, 2, 2, 2, "T", True, True, False),
    (0, "euler", 0, 1, 255, 3, "2", False, False, False),
    (1, "euler", 0, 5, 256, 3, "T", True, False, False),
    (2, "rk4", 0, 2, 257, 2, "T+1", True, True, False),
    (0, "rk4", 0, 1, 300, 65, "2", True, False, True),
    (0, "rk4", 1, 2, 64, 65, "T", False, True, False),
    (1, "rk4", 0, 5, 1, 7, "T", True, True, False),
    (2, "rk4", 0, 1, 65, 1, "2", False, False, False),
)


def draw_rollout_pop(rng):
    s = SETS["rollout_pop"]
    T = _pick(rng, s["T"])
    return _rollout_pop(rng, _pick(rng, s["model"]), _pick(rng, s["integ"]), _pick(rng, s["lag_mode"]), _pick(rng, s["P"]), _pick(rng, s["B"]),
                        T, _pick(rng, s["stride"]) if T else "1", _pick(rng, s["store"]), _pick(rng, s["per_candidate"]), _pick(rng, s["lag"]))


# ------------------------------------------------------------------------------------------ closed-loop rollouts
def _feedback(rng, model, integ, lag_mode, P, B, T, hold, ref, u_ff, z, lag, gain_sets, stride, store):
    """hold and stride as symbols of T; T = 0 takes a set-point (ref_rows must be 1 or T)"""
    T = int(T)
    return dict(family="feedback", model=model, integ=integ, lag_mode=lag_mode if (model == 0 and integ == "rk4") else 0, P=P, B=B, T=T,
                hold=_sym(hold, T=T), hold_as=hold, ref="set" if T == 0 else ref, u_ff=bool(u_ff), z=bool(z), lag=bool(lag and model == 0),
                gain_sets=bool(gain_sets), stride=max(_sym(stride, T=T), 1), stride_as=stride, store=bool(store),
                names=_vehicles(rng, model, P), seed=int(rng.integers(0, 1 << 30)))


FEEDBACK_CORNERS = (
    # model integ lag_mode P  B    T    hold   ref    u_ff   z      lag    gain_sets stride store
    (0, "rk4", 0, 5, 64, 7, "5", "T", True, True, True, True, "1", True),
    (0, "rk4", 1, 2, 65, 24, "T+1", "set", False, False, False, False, "T+1", True),
    (0, "euler", 0, 2, 63, 0, "1", "set", False, True, True, False, "1", True),
    (1, "rk4", 0, 1, 1, 1, "1", "T", True, False, False, False, "1", True),
    (2, "euler", 0, 2, 2, 2, "2", "set", True, True, False, True, "T", True),
    (0, "euler", 0, 1, 255, 3, "3", "T", False, True, True, False, "2", False),
    (1, "euler", 0, 5, 256, 3, "T+1", "T", True, True, False, True, "T", True),
    (2, "rk4", 0, 2, 257, 65, "5", "T", True, False, False, False, "T+1", True),
    (0, "rk4", 0, 1, 300, 130, "3", "T", True, True, True, False, "2", True),
    (0, "rk4", 1, 2, 64, 65, "2", "set", True, True, False, True, "T", False),
    (1, "rk4", 0, 5, 1, 7, "T+1", "set", False, False, False, True, "T", True),
    (2, "rk4", 0, 1, 65, 24, "5", "T", True, True, False, False, "2", False),
)


def draw_feedback(rng):
    s = SETS["feedback"]
    T = _pick(rng, s["T"])
    return _feedback(rng, _pick(rng, s["model"]), _pick(rng, s["integ"]), _pick(rng, s["lag_mode"]), _pick(rng, s["P"]), _pick(rng, s["B"]), T,
                     _pick(rng, s["hold"]), _pick(rng, s["ref"]), _pick(rng, s["u_ff"]), _pick(rng, s["z"]), _pick(rng, s["lag"]),
                     _pick(rng, s["gain_sets"]), _pick(rng, s["stride"]) if T else "1", _pick(rng, s["store"]))


# ------------------------------------------------------------------------------------------ MPPI with the Fossen model
def _window(rng, rows, H):
    """(reference rows, ref_row0): a set-point, or a window drawn over its whole legal range 0 .. rows - 1 - H"""
    n = _sym(rows, H=H)
    return n, (0 if n == 1 else int(rng.integers(0, n - H)))


def _mppi(rng, model, integ, lag_mode, B, nparams, K, H, hold, rows, shift, eps):
    hold_n = _sym(hold, H=H)
    rows_n, row0 = _window(rng, rows, H)
    nu = 8 if model == 0 else 6
    return dict(family="mppi", model=model, integ=integ, lag_mode=lag_mode if (model == 0 and integ == "rk4") else 0, B=B,
                nparams=_sym(nparams, B=B), K=K, H=H, hold=hold_n, hold_as=hold, M=(H + hold_n - 1) // hold_n, rows=rows_n, rows_as=rows,
                row0=row0, shift=bool(shift), eps=bool(eps), stream_seed=int(rng.integers(0, 1 << 40)), sigma0=int(rng.integers(0, nu)),
                names=_vehicles(rng, model, _sym(nparams, B=B)), seed=int(rng.integers(0, 1 << 30)))


MPPI_CORNERS = (
    # model integ lag_mode B nparams K    H   hold   rows    shift  eps
    (0, "rk4", 0, 2, "B", 300, 7, "H", "H+4", True, True),       # M = 1 with the shift
    (0, "rk4", 1, 3, "B", 513, 5, "2", "H+1", False, False),     # three trips of the update's stride loop, the seeded stream, B = 3
    (0, "euler", 0, 3, "1", 64, 12, "3", "1", True, True),       # K = 64 and 65 under Euler: both block sizes
    (1, "euler", 0, 2, "B", 65, 12, "H+2", "H+4", True, False),
    (2, "rk4", 0, 1, "1", 1, 1, "1", "1", False, True),
    (1, "rk4", 0, 2, "1", 2, 2, "2", "H+1", True, True),
    (2, "euler", 0, 3, "B", 63, 2, "1", "H+4", False, False),
    (0, "rk4", 0, 1, "B", 255, 5, "3", "H+1", True, False),
    (1, "rk4", 0, 3, "B", 256, 7, "2", "1", False, True),
    (2, "rk4", 0, 2, "B", 257, 5, "H+2", "H+4", True, False),
    (0, "euler", 0, 2, "1", 513, 1, "H", "H+1", True, True),
    (0, "rk4", 1, 3, "B", 65, 7, "3", "H+4", False, True),
)


def draw_mppi(rng):
    s = SETS["mppi"]
    return _mppi(rng, _pick(rng, s["model"]), _pick(rng, s["integ"]), _pick(rng, s["lag_mode"]), _pick(rng, s["B"]), _pick(rng, s["nparams"]),
                 _pick(rng, s["K"]), _pick(rng, s["H"]), _pick(rng, s["hold"]), _pick(rng, s["rows"]), _pick(rng, s["shift"]), _pick(rng, s["eps"]))


# ------------------------------------------------------------------------------------------ MPPI with a Koopman model
# (H, hold) for every M: full last knots and partial ones
KOOPMAN_KNOTS = {1: ((1, 1), (3, 5)), 5: ((5, 1), (9, 2)), 6: ((6, 1), (11, 2)), 7: ((7, 1), (13, 2)), 9: ((9, 1), (17, 2)),
                 10: ((10, 1), (28, 3)), 12: ((12, 1), (23, 2)), 13: ((13, 1), (25, 2)), 14: ((14, 1), (27, 2))}


def _koopman_mppi(rng, n, r, k, Mr, K, B, rows, shift, eps, partial):
    """Mr = M r picks the number of knots; partial: the (H, hold) whose last knot is cut short"""
    assert Mr % r == 0, (Mr, r)
    M = Mr // r
    H, hold = KOOPMAN_KNOTS[M][1 if partial else 0]
    rows_n, row0 = _window(rng, rows, H)
    return dict(family="koopman_mppi", n=n, r=r, k=k, Mr=Mr, M=M, H=H, hold=hold, K=K, B=B, rows=rows_n, rows_as=rows, row0=row0,
                shift=bool(shift), eps=bool(eps), stream_seed=int(rng.integers(0, 1 << 40)), sigma0=int(rng.integers(0, r)),
                seed=int(rng.integers(0, 1 << 30)))


KOOPMAN_MPPI_CORNERS = (
    # n   r  k   Mr  K    B  rows    shift  eps    partial
    (12, 6, 0, 6, 1, 1, "1", True, True, False),                  # M = 1 with the shift, one sample
    (13, 8, 5, 8, 63, 2, "H+1", False, False, True),
    (12, 6, 20, 36, 300, 3, "H+4", True, False, False),           # 256 lanes, the seeded stream, B = 3
    (13, 8, 20, 40, 65, 2, "H+4", False, True, True),             # M r = 40: 128 lanes
    (13, 6, 5, 42, 127, 3, "H+1", True, True, False),
    (12, 8, 0, 72, 128, 1, "1", False, False, True),
    (13, 6, 20, 78, 129, 2, "H+4", True, True, True),             # M r = 78: the last of the 128-lane sizes
    (12, 8, 5, 80, 255, 3, "H+1", False, True, False),            # M r = 80: 64 lanes at K > 64, dynamic LDS
    (13, 6, 0, 84, 256, 2, "1", True, False, True),
    (12, 6, 5, 72, 257, 1, "H+4", False, True, False),
    (13, 8, 0, 80, 64, 3, "H+1", True, True, True),               # K = 64: 64 lanes whatever M r
    (12, 6, 20, 78, 300, 2, "H+1", False, False, False),
)


def draw_koopman_mppi(rng):
    s = SETS["koopman_mppi"]
    r = _pick(rng, s["r"])
    return _koopman_mppi(rng, _pick(rng, s["n"]), r, _pick(rng, s["k"]), _pick(rng, [v for v in s["Mr"] if v % r == 0]), _pick(rng, s["K"]),
                         _pick(rng, s["B"]), _pick(rng, s["rows"]), _pick(rng, s["shift"]), _pick(rng, s["eps"]), bool(rng.integers(0, 2)))


# ------------------------------------------------------------------------------------------ population window evaluator
def _window_pop(rng, model, integ, carry, P, H, lens, bags, short_u):
    """lens: rows per bag (symbols of H); bags False: one recording through the plain entry point.  The windows of a bag number
    max(L - H, 0), counted bag after bag."""
    L = [_sym(v, H=H) for v in lens]
    assert bags or len(L) == 1
    pool = NAMES if model == 0 else WRENCH_NAMES
    first = int(rng.integers(0, len(pool)))
    return dict(family="window_pop", model=model, integ=integ, carry=bool(carry), P=P, H=H, lens=L, nwin=sum(max(v - H, 0) for v in L),
                bags=bool(bags), short_u=bool(short_u), names=[pool[(first + j) % len(pool)] for j in range(P)],
                seed=int(rng.integers(0, 1 << 30)))


WINDOW_POP_CORNERS = (
    # model integ carry P  H   lens                                  bags   short_u
    (0, "rk4", True, 2, 5, ("H+64", "0", "H+1"), True, False),                 # a join on the edge of a scan chunk, an empty bag: 65 windows
    (0, "euler", True, 9, 1, ("H+1",), False, True),                           # one window
    (0, "rk4", False, 1, 2, ("H+2",), True, False),                            # one bag through the ragged entry point: 2 windows
    (1, "rk4", True, 2, 12, ("H+63",), False, False),
    (2, "euler", False, 9, 5, ("H+64",), False, True),
    (0, "rk4", True, 1, 12, ("1", "H", "H+65", "H+62", "0"), True, True),      # bags without a window first: 127 windows in five bags
    (0, "euler", True, 2, 2, ("H+128",), False, False),
    (0, "rk4", True, 2, 1, ("H+64", "H+65"), True, True),                      # 129 windows, the join on a chunk edge
    (0, "rk4", True, 2, 5, ("H+257",), False, False),
    (1, "euler", True, 1, 2, ("H+1", "H", "H+64", "H+63"), True, False),       # 128 windows in four bags
    (2, "rk4", True, 2, 12, ("H+65", "H+64", "H+128"), True, True),            # 257 windows, joins at 65 and 129
    (0, "rk4", True, 9, 5, ("H+63", "H+1"), True, False),                      # 64 windows, a join inside the first chunk
)

WINDOW_BAG_LENS = ("0", "1", "H", "H+1", "H+2", "H+63", "H+64", "H+65")


def draw_window_pop(rng):
    s = SETS["window_pop"]
    H = _pick(rng, s["H"])
    bags = bool(rng.integers(0, 2))
    if bags:
        lens = [_pick(rng, WINDOW_BAG_LENS) for _ in range(_pick(rng, s["nbags"]))]
        if all(_sym(v, H=H) <= H for v in lens):
            lens[int(rng.integers(0, len(lens)))] = "H+64"                     # a case keeps at least one window
    else:
        lens = ["H+%d" % _pick(rng, s["nwin"])]
    return _window_pop(rng, _pick(rng, s["model"]), _pick(rng, s["integ"]), _pick(rng, s["carry"]), _pick(rng, s["P"]), H, lens, bags,
                       _pick(rng, s["short_u"]))


# ------------------------------------------------------------------------------------------ EDMDc: lift
def _lift(rng, N, k, n, gamma, scale):
    """scale: the rows are uniform in +- scale; 12 puts every row far from every centre (|x_j| in 6 .. 12, the centres in +-0.5)"""
    return dict(family="lift", N=N, k=k, n=n, gamma=gamma, scale=scale, seed=int(rng.integers(0, 1 << 30)))


LIFT_CORNERS = (
    # N   k    n   gamma scale
    (1, 1, 1, 0.3, 0.5),
    (63, 255, 5, 3.0, 0.5),                # below both block edges; the runtime-n instantiation
    (64, 256, 12, 0.3, 0.5),               # one block each way, <12>
    (65, 257, 13, 3.0, 0.5),               # two blocks each way, <13>
    (130, 513, 16, 0.3, 0.5),              # three blocks each way, n = LIFT_NMAX
    (130, 257, 12, 3.0, 12.0),             # far from every centre: the clamped ldexp of exp_fast
    (65, 513, 13, 0.3, 3.0),               # values down to the denormals
    (1, 513, 12, 3.0, 0.5),
    (130, 1, 5, 0.3, 3.0),
    (64, 255, 16, 3.0, 3.0),
    (63, 256, 1, 3.0, 12.0),
    (65, 257, 12, 0.3, 0.5),
)


def draw_lift(rng):
    """one row against one centre is a single value, whose float64-to-long-double gap says nothing about the size of the error at its
    exponent (it can be 0 by chance) although the relative bound is a multiple of it: that draw takes 63 rows.  The corner list keeps
    N = k = n = 1 at scale 0.5, where the exponent is below 0.3 and the 2^-50 of the bound covers any rounding of it."""
    s = SETS["lift"]
    N, k = _pick(rng, s["N"]), _pick(rng, s["k"])
    return _lift(rng, 63 if N * k == 1 else N, k, _pick(rng, s["n"]), _pick(rng, s["gamma"]), _pick(rng, s["scale"]))


# ------------------------------------------------------------------------------------------ EDMDc: Gram and pinv_apply
def tiles(n, r, k):
    """(nt = lifted-row width / 16, xplus) of csrc/brov2_kernels.h: edmdc_shape -- what the task packing depends on"""
    tailp = (n + r + 15) // 16 * 16
    return ((k + 15) // 16 * 16 + tailp) // 16, int(n + r + n <= tailp)


def chunk_rows(chunk, lens, xpad=0):
    """the rows per lifted chunk that gram / apply (csrc/capi.hip) use: the setting rounded up to 4, at most the rows that can start a pair"""
    rows = sum(lens) + xpad * (len(lens) - 1)
    top = max((max(rows - 1, 0) + 3) // 4 * 4, 4)
    return min((chunk + 3) // 4 * 4, top) if chunk else top


def bag_ends(lens):
    """row index one past the last row of every bag that has a row"""
    return [e for e, m in zip(np.cumsum(lens).tolist(), lens) if m]


def _bags(rng, family, n, r, k, gamma, form, gty, lens, xpad, upad, chunk, short_u, split):
    """lens: state rows per bag (uniform_dev: all equal, L + 1); xpad / upad: rows between the bags of the uniform layout beyond L + 1 / L;
    chunk: edmdc_set_chunk_rows (0 = the default); short_u: the inputs of the last bag one row shorter than its states (list forms);
    split: bags in the first of two accumulate calls (device forms of the Gram; 0 = one call)"""
    lens = [int(v) for v in lens]
    uniform = form == "uniform_dev"
    assert not uniform or (len(set(lens)) == 1 and lens[0] >= 1), lens
    assert 0 <= split < max(len(lens), 1) and (split == 0 or (form != "host" and family == "gram"))
    nt, xplus = tiles(n, r, k)
    return dict(family=family, n=n, r=r, k=k, gamma=gamma, form=form, gty=bool(gty or form == "host" or family == "pinv_apply"), lens=lens,
                xpad=xpad if uniform else 0, upad=upad if uniform else 0, chunk=chunk, short_u=bool(short_u and not uniform and lens[-1] >= 1),
                split=split, pairs=sum(max(v - 1, 0) for v in lens), nt=nt, xplus=xplus, seed=int(rng.integers(0, 1 << 30)))


def _gram(rng, n, r, k, gamma, form, gty, lens, xpad, upad, chunk, short_u, split):
    return _bags(rng, "gram", n, r, k, gamma, form, gty, lens, xpad, upad, chunk, short_u, split)


GRAM_CORNERS = (
    # n   r   k    gamma form          gty    lens                             xpad upad chunk short_u split
    (12, 8, 1, 1.0, "host", True, (0, 5, 1, 2, 3), 0, 0, 0, False, 0),                  # bags of 0 .. 3 rows first, last, in the middle
    (13, 8, 15, 0.3, "host", True, (1, 4, 0, 3, 2), 0, 0, 64, True, 0),
    (12, 10, 16, 3.0, "ragged_dev", True, (2, 6, 3, 0, 1), 0, 0, 100, False, 2),
    (13, 6, 17, 1.0, "ragged_dev", False, (3, 2, 7, 1, 0), 0, 0, 257, False, 0),        # G^T G alone over a ragged list
    (9, 4, 31, 0.3, "uniform_dev", True, (9,) * 4, 0, 0, 0, False, 2),                  # strides L + 1 / L, two halves
    (5, 2, 32, 3.0, "uniform_dev", True, (9,) * 5, 3, 2, 64, False, 2),                 # larger strides, uneven halves
    (12, 0, 33, 1.0, "host", True, (20, 1, 13), 0, 0, 0, False, 0),                     # r = 0
    (12, 1, 48, 0.3, "uniform_dev", False, (17,) * 3, 2, 0, 64, False, 0),              # r = 1; G^T G alone over a uniform layout
    (12, 8, 64, 1.0, "host", True, (64, 63, 66, 5), 0, 0, 64, False, 0),                # bags ending on, one before, one after a chunk's last row
    (13, 8, 80, 3.0, "host", True, (5,) + (1,) * 130 + (7,), 0, 0, 64, False, 0),       # a chunk that holds no pair
    (12, 10, 96, 0.3, "ragged_dev", True, (65, 36), 0, 0, 64, True, 1),                 # a pair across the chunk edge; a short U
    (13, 6, 112, 1.0, "ragged_dev", False, (100, 1, 0, 99), 0, 0, 100, False, 0),       # bags of 1 and 0 rows behind a chunk edge
    (9, 4, 160, 3.0, "host", True, (40, 30), 0, 0, 0, True, 0),
    (5, 2, 257, 0.3, "host", True, (30, 25), 0, 0, 0, False, 0),
    (12, 8, 512, 1.0, "uniform_dev", True, (12,) * 2, 0, 0, 0, False, 1),
    (13, 8, 513, 3.0, "host", True, (14, 9), 0, 0, 64, False, 0),
    (12, 8, 16, 1.0, "host", True, (2,), 0, 0, 0, False, 0),                            # one pair: fewer rows than K-slabs
    (13, 6, 17, 0.3, "ragged_dev", True, (2, 0, 2), 0, 0, 64, False, 0),                # two pairs
    (9, 4, 1, 3.0, "uniform_dev", True, (2,) * 3, 1, 1, 0, False, 1),                   # three pairs
    (12, 10, 512, 0.3, "ragged_dev", False, (10, 11), 0, 0, 0, False, 0),
    (13, 8, 257, 1.0, "uniform_dev", False, (8,) * 3, 0, 3, 0, False, 0),
    (12, 8, 33, 1.0, "host", True, (63, 1, 0, 64, 0, 1, 66), 0, 0, 64, True, 0),        # bags of 0 and 1 rows on both sides of chunk edges
    (5, 2, 48, 1.0, "host", True, (260, 259, 262, 4), 0, 0, 257, False, 0),             # chunk 257 (260 rows): on, before, after
    (13, 6, 64, 0.3, "ragged_dev", True, (100, 99, 102, 4), 0, 0, 100, False, 3),       # chunk 100: on, before, after
)

GRAM_LENS = (0, 1, 2, 3, 5, 33, 63, 64, 65, 100)


def _draw_bags(rng, k, form, lens_set):
    """a bag list whose long-double reference stays cheap: few rows where k is large"""
    small = tuple(v for v in lens_set if v <= 12)
    if form == "uniform_dev":
        lens = [_pick(rng, [v for v in (small if k > 160 else lens_set) if v >= 2])] * int(rng.integers(1, 6))
    else:
        lens = [_pick(rng, small if k > 160 else lens_set) for _ in range(int(rng.integers(1, 6)))]
        if max(lens) < 2:
            lens[int(rng.integers(0, len(lens)))] = 5
    return lens


def draw_gram(rng):
    s = SETS["gram"]
    (n, r), k, form = _pick(rng, s["nr"]), _pick(rng, s["k"]), _pick(rng, s["form"])
    lens = _draw_bags(rng, k, form, GRAM_LENS)
    split = int(rng.integers(0, len(lens))) if form != "host" else 0
    return _gram(rng, n, r, k, _pick(rng, s["gamma"]), form, _pick(rng, s["gty"]), lens, int(rng.integers(0, 4)), int(rng.integers(0, 4)),
                 _pick(rng, s["chunk"]), _pick(rng, s["short_u"]), split)


def _pinv_apply(rng, n, r, k, gamma, form, lens, xpad, upad, chunk):
    return _bags(rng, "pinv_apply", n, r, k, gamma, form, True, lens, xpad, upad, chunk, False, 0)


PINV_APPLY_CORNERS = (
    # n   r  k    gamma form          lens              xpad upad chunk
    (12, 8, 1, 1.0, "host", (2, 3), 0, 0, 64),
    (12, 6, 7, 0.3, "host", (192,), 0, 0, 192),                    # one 192-row unit, one chunk
    (13, 6, 16, 3.0, "ragged_dev", (193, 2), 0, 0, 192),
    (9, 4, 17, 1.0, "uniform_dev", (193,) * 2, 0, 0, 64),
    (5, 2, 48, 0.3, "uniform_dev", (3,) * 3, 2, 1, 257),
    (13, 8, 64, 3.0, "host", (257, 3), 0, 0, 64),
    (12, 8, 80, 1.0, "ragged_dev", (192, 193), 0, 0, 257),
    (12, 6, 96, 0.3, "host", (3, 2, 12), 0, 0, 192),
    (13, 6, 100, 3.0, "uniform_dev", (12,) * 2, 0, 3, 64),
    (9, 4, 160, 1.0, "host", (2, 12, 3), 0, 0, 257),
    (5, 2, 257, 0.3, "ragged_dev", (12, 3), 0, 0, 64),
    (13, 8, 512, 3.0, "host", (12,), 0, 0, 192),
    (12, 8, 530, 1.0, "uniform_dev", (3,) * 4, 0, 0, 257),
    (12, 8, 17, 1.0, "host", (257, 192, 2), 0, 0, 192),
)

PINV_APPLY_LENS = (2, 3, 12, 192, 193, 257)


def draw_pinv_apply(rng):
    s = SETS["pinv_apply"]
    (n, r), k, form = _pick(rng, s["nr"]), _pick(rng, s["k"]), _pick(rng, s["form"])
    lens = _draw_bags(rng, k, form, PINV_APPLY_LENS)[:3]
    return _pinv_apply(rng, n, r, k, _pick(rng, s["gamma"]), form, lens, int(rng.integers(0, 4)), int(rng.integers(0, 4)), _pick(rng, s["chunk"]))


# ------------------------------------------------------------------------------------------ EDMDc: multistep evaluators and simulate
def _prop(n, k, r):
    """(d, K-steps of propagate_kernel = ceil((n + k + r) / 4))"""
    return n + k, (n + k + r + 3) // 4


def _multistep(rng, shape, nw, H, short_u):
    """nw windows of horizon H over N = nw + H rows; nw = 0: H >= N (three rows at most), where the evaluators return 0"""
    n, k, r = shape
    H = max(H, 1) if nw == 0 else H
    d, ksteps = _prop(n, k, r)
    return dict(family="multistep", n=n, k=k, r=r, d=d, ksteps=ksteps, nw=nw, H=H, N=nw + H if nw else min(H, 3), short_u=bool(short_u),
                seed=int(rng.integers(0, 1 << 30)))


MULTISTEP_CORNERS = (
    # (n, k, r)     nw    H  short_u
    ((1, 1, 1), 1, 0, False),              # one K-step, H = 0, one window
    ((2, 3, 3), 127, 1, True),             # two K-steps
    ((12, 35, 8), 128, 2, False),          # d = 47
    ((12, 36, 9), 129, 3, True),           # d = 48, 15 K-steps: the odd tail
    ((13, 36, 6), 255, 7, False),          # d = 49
    ((12, 83, 8), 256, 2, False),          # d = 95
    ((13, 84, 8), 257, 3, True),           # d = 97, 27 K-steps
    ((12, 8, 0), 129, 7, False),           # r = 0
    ((5, 8, 2), 1920, 7, False),           # 15 window blocks: one stream
    ((9, 4, 6), 1921, 2, True),            # 16 blocks: two streams; odd K-steps, even H
    ((5, 8, 2), 2176, 3, False),           # 17 blocks: 8 + 9; even K-steps, odd H
    ((9, 4, 6), 0, 7, False),              # H >= N
    ((1, 1, 1), 2176, 2, True),            # one K-step on two streams
    ((12, 8, 0), 1, 1, True),
)


def draw_multistep(rng):
    s = SETS["multistep"]
    shape, nw = _pick(rng, s["shape"]), _pick(rng, s["nw"])
    if nw > 257 and shape[0] + shape[1] > 20:                      # the long-double reference: many windows go with a small d
        shape = (5, 8, 2)
    return _multistep(rng, shape, nw, _pick(rng, s["H"]), _pick(rng, s["short_u"]))


def _simulate(rng, shape, nb, T):
    n, k, r = shape
    d, ksteps = _prop(n, k, r)
    return dict(family="simulate", n=n, k=k, r=r, d=d, ksteps=ksteps, nb=nb, T=T, seed=int(rng.integers(0, 1 << 30)))


SIMULATE_CORNERS = (
    # (n, k, r)     nb   T
    ((1, 1, 1), 1, 0),
    ((2, 3, 3), 2, 1),
    ((12, 35, 8), 127, 2),
    ((12, 36, 9), 128, 3),
    ((13, 36, 6), 129, 7),
    ((12, 83, 8), 255, 2),
    ((13, 84, 8), 256, 3),
    ((12, 8, 0), 257, 7),                  # r = 0, a third block
    ((5, 8, 2), 300, 50),
    ((9, 4, 6), 257, 50),
    ((12, 8, 0), 300, 1),
    ((1, 1, 1), 129, 50),
)


def draw_simulate(rng):
    s = SETS["simulate"]
    shape, T = _pick(rng, s["shape"]), _pick(rng, s["T"])
    if T == 50 and shape[0] + shape[1] > 20:                       # the long-double reference: a long horizon goes with a small d
        T = 7
    return _simulate(rng, shape, _pick(rng, s["nb"]), T)


# ------------------------------------------------------------------------------------------ unscented Kalman filter
UKF_ROWS = 200                                                      # P B T of a case at most: the reference is plain Python loops


def ukf_instance(c):
    """the instantiation of ukf_filter_kernel a case runs: (model, integ, lag_mode, TRACK)"""
    return (c["model"], c["integ"], c["lag_mode"], c["lag"])


def _ukf(rng, model, integ, lag_mode, lag, P, nrec, alpha, B, T, measured, r_inf, q_zero, wrap):
    """lag: the thruster model starts from a lag (TRACK; without one the kernel takes its other form); nrec: noise records, one or one
    per candidate; measured: "std" about 30 % of the entries dropped and one row dropped entirely (tests/ukf_cases.py), "all" every
    entry of every row, "none" no entry at all; r_inf: components with r = +inf whose Y columns still carry numbers; q_zero: three
    process variances exactly 0; wrap: the true yaw passes pi while Y reports it wrapped.  The recordings are simulated with the last
    candidate's vehicle."""
    assert P * B * T <= UKF_ROWS, (P, B, T)
    return dict(family="ukf", model=model, integ=integ, lag_mode=lag_mode if (model == 0 and integ == "rk4") else 0, lag=bool(lag and model == 0),
                P=P, nrec=_sym(nrec, P=P), nrec_as=nrec, alpha=alpha, B=B, T=T, measured=measured, r_inf=r_inf, q_zero=bool(q_zero),
                wrap=bool(wrap), names=_vehicles(rng, model, P), seed=int(rng.integers(0, 1 << 30)))


UKF_CORNERS = (
    # model integ lag_mode lag  P  nrec alpha B  T  measured r_inf q_zero wrap     -- every instantiation with a full and a ragged block
    (0, "euler", 0, True, 2, "1", 1.0, 4, 12, "std", 1, False, True),              # the yaw through pi, as thr_euler_wrap
    (0, "euler", 0, True, 1, "1", 0.5, 5, 12, "all", 0, True, False),              # 12 updates in every row; a full block and a lone wave
    (0, "euler", 0, False, 3, "P", 1.0, 8, 2, "std", 3, False, False),             # no start lag; a noise record per candidate at P = 3
    (0, "euler", 0, False, 2, "1", 0.5, 1, 12, "none", 1, True, False),            # pure prediction, one recording
    (0, "rk4", 0, True, 1, "1", 1.0, 8, 3, "std", 1, False, False),
    (0, "rk4", 0, True, 3, "P", 0.5, 3, 12, "std", 0, True, True),
    (0, "rk4", 0, False, 2, "P", 1.0, 4, 1, "all", 0, False, False),               # T = 1
    (0, "rk4", 0, False, 1, "1", 0.5, 9, 12, "std", 1, False, False),              # three blocks, the last with one wave
    (0, "rk4", 1, True, 2, "1", 1.0, 4, 12, "all", 3, False, False),
    (0, "rk4", 1, True, 1, "1", 0.5, 3, 2, "std", 1, True, False),
    (0, "rk4", 1, False, 1, "1", 1.0, 8, 12, "std", 0, False, True),
    (0, "rk4", 1, False, 3, "1", 0.5, 5, 1, "none", 1, False, False),
    (1, "euler", 0, False, 2, "P", 1.0, 8, 3, "all", 0, True, False),
    (1, "euler", 0, False, 1, "1", 0.5, 9, 2, "std", 3, False, True),
    (1, "rk4", 0, False, 3, "1", 1.0, 4, 12, "std", 1, False, False),
    (1, "rk4", 0, False, 2, "P", 0.5, 1, 1, "none", 0, False, False),
    (1, "rk4", 0, False, 3, "P", 1.0, 5, 12, "all", 0, True, False),               # 180 filter rows of 12 updates each
)


def draw_ukf(rng):
    s = SETS["ukf"]
    while True:
        P, B, T = _pick(rng, s["P"]), _pick(rng, s["B"]), _pick(rng, s["T"])
        if P * B * T <= UKF_ROWS:                                     # a draw beyond the row budget is drawn again
            break
    return _ukf(rng, _pick(rng, s["model"]), _pick(rng, s["integ"]), _pick(rng, s["lag_mode"]), _pick(rng, s["lag"]), P, _pick(rng, s["nrec"]),
                _pick(rng, s["alpha"]), B, T, _pick(rng, s["measured"]), _pick(rng, s["r_inf"]), _pick(rng, s["q_zero"]), _pick(rng, s["wrap"]))


# ------------------------------------------------------------------------------------------ Koopman linear MPC: the batched QP
LMPC_H_MAX = 129                                                    # H + 1 = 130: one step into the third trip of the epilogue
LMPC_H_EDGES = (63, 64, 65, 127, 128, 129)                          # H + 1 on both sides of 64 and 128
LMPC_REF_TOTAL, LMPC_ROW0 = 4, 2                                    # tests/koopman_lmpc_ref.py: REF_TOTAL, ROW0
LMPC_TOL, LMPC_LDS_NV = 1e-12, 95                                   # the tolerance of a "warm" case; W is staged in LDS up to this Nv


def lmpc_rows(c):
    """(rows per lane Q of qp_solve, W staged in LDS) of csrc/koopman_qp.hip: koopman_qp_solve_kernel"""
    lds = c["Nv"] <= LMPC_LDS_NV
    nq = (c["Nv"] + 63) // 64
    return (nq if lds else 5 if nq > 4 else max(nq, 2)), lds


def _lmpc(rng, n, r, k, Nv, hold, H, nb, iters, traj, y, shift, special):
    """Nv = M r picks the knots, H lies in (M - 1) hold + 1 .. M hold; traj: a reference trajectory (else a set-point); y: the dual
    variable given; special: references on the far hemisphere (n = 13) / a turn away (n = 12), or "warm": the residual stop of
    tests/koopman_lmpc_ref.py's `tol` case (limits out of reach, rho = lambda_min / 10 000, every other problem started 10 000
    times nearer to its minimiser, tol = 1e-12)"""
    assert Nv % r == 0 and (H + hold - 1) // hold == Nv // r and 1 <= H <= LMPC_H_MAX, (Nv, r, hold, H)
    assert special in (None, "warm") or (special == "quat_flip") == (n == 13), (special, n)
    return dict(family="lmpc", n=n, r=r, k=k, Nv=Nv, M=Nv // r, hold=hold, H=H, nb=nb, iters=iters, tol=LMPC_TOL if special == "warm" else 0.0,
                traj=bool(traj), y=bool(y), shift=bool(shift), special=special, seed=int(rng.integers(0, 1 << 30)))


LMPC_CORNERS = (
    # n   r  k   Nv   hold H    nb iters traj   y      shift  special
    (13, 6, 5, 6, 3, 3, 1, 40, False, False, False, "quat_flip"),                  # one knot
    (12, 8, 0, 8, 1, 1, 3, 2, True, True, False, None),                            # one knot, a linear model
    (12, 8, 5, 8, 9, 7, 4, 0, True, True, True, None),                             # hold r = 72: a second trip of the u_apply loop; hold > H
    (12, 8, 70, 64, 8, 64, 3, 1, False, False, False, None),                       # hold r = 64; H + 1 = 65; the last one-row size
    (12, 6, 5, 66, 10, 101, 5, 40, True, True, True, "angle_wrap"),                # hold r = 60; two rows per lane, W in LDS, Nv % 8 = 2
    (13, 6, 0, 66, 11, 121, 3, 2, False, True, False, "quat_flip"),                # hold r = 66
    (12, 8, 5, 88, 3, 31, 8, 40, True, False, False, None),                        # two full blocks
    (12, 6, 5, 90, 1, 15, 5, 40, False, False, True, None),                        # the last size with W in LDS
    (12, 8, 5, 96, 1, 12, 5, 40, True, False, False, None),                        # W from global memory
    (13, 6, 70, 96, 2, 31, 9, 1, True, True, True, None),                          # three blocks, the last with one wave
    (13, 6, 5, 126, 3, 63, 4, 40, True, True, False, "quat_flip"),                 # H + 1 = 64: one full trip; the scalar tail (Nv % 8 = 6) from global memory
    (12, 8, 0, 128, 8, 127, 3, 2, False, True, True, None),                        # H + 1 = 128; the last two-row size
    (12, 6, 5, 132, 3, 64, 5, 40, True, True, True, "angle_wrap"),                 # three rows per lane, H + 1 = 65, a short last knot, Nv % 8 = 4
    (12, 8, 70, 136, 8, 129, 3, 40, False, False, False, None),                    # H + 1 = 130: a third trip
    (12, 8, 5, 192, 2, 48, 4, 1, True, True, False, None),                         # the last three-row size
    (13, 6, 5, 198, 2, 65, 1, 40, True, False, True, None),                        # four rows per lane, H + 1 = 66, Nv % 8 = 6
    (12, 8, 0, 200, 1, 25, 8, 2, False, True, False, None),
    (12, 8, 5, 256, 2, 64, 3, 40, True, True, True, None),                         # the last four-row size, H + 1 = 65
    (12, 6, 5, 258, 3, 128, 3, 40, False, True, False, None),                      # five rows per lane, H + 1 = 129, a short last knot, Nv % 8 = 2
    (12, 8, 5, 264, 1, 33, 5, 0, True, True, True, None),
    (13, 6, 5, 306, 1, 51, 4, 40, True, False, True, "quat_flip"),
    (12, 8, 0, 312, 1, 39, 3, 40, False, False, False, None),                      # the largest problem
    (12, 8, 5, 96, 3, 34, 5, 40, True, False, False, "warm"),                      # the residual stop at two rows per lane from global memory,
    (12, 6, 5, 132, 2, 43, 5, 40, True, False, True, "warm"),                      # at three
    (12, 8, 5, 264, 2, 65, 4, 40, True, False, False, "warm"),                     # and at five
    (13, 6, 5, 258, 3, 127, 3, 2, True, False, True, "quat_flip"),                 # H + 1 = 128 at five rows per lane
)


def draw_lmpc(rng):
    """never "warm": whether a residual stop can be compared exactly is a property of the seed, which the corner list has checked"""
    s = SETS["lmpc"]
    n, r = _pick(rng, s["n"]), _pick(rng, s["r"])
    M = _pick(rng, [v for v in s["Nv"] if v % r == 0]) // r
    hold = _pick(rng, [h for h in s["hold"] if (h <= 3 or h in ((8, 9) if r == 8 else (10, 11))) and (M - 1) * h + 1 <= LMPC_H_MAX])
    lo, hi = (M - 1) * hold + 1, min(M * hold, LMPC_H_MAX)
    H = _pick(rng, sorted({lo, hi} | {v for v in LMPC_H_EDGES if lo <= v <= hi}))
    special = _pick(rng, (None, "quat_flip" if n == 13 else "angle_wrap"))
    return _lmpc(rng, n, r, _pick(rng, s["k"]), M * r, hold, H, _pick(rng, s["nb"]), _pick(rng, s["iters"]), _pick(rng, s["traj"]),
                 _pick(rng, s["y"]), _pick(rng, s["shift"]), special)



# ------------------------------------------------------------------------------------------ k-means: column statistics
# The data recipe of the three k-means families (tests/sweep_kmeans.py: data): a random walk cumsum(N(0, 0.05)) + 0.3 sin(i w_j); order:
# the walk, shuffled rows (more than KM_GMAX = 8 label groups per wave of the Lloyd filter: full scan) or four blobs; times scale; offset:
# column means 20 .. 100 scale from 0; const_col: one column constant.  form: "host" a host array (colstats, kmeanspp: a DevArray
# uploaded from it), "dev" a contiguous torch tensor, "dev_stride" rows n + 1 doubles apart, "block_odd" / "block_even" columns
# 3 .. / 4 .. of a 40-column tensor (the base 8 bytes off a 16-byte boundary / on one).
KM_BLOCK_WIDTH, KM_BLOCK_COL = 40, {"block_odd": 3, "block_even": 4}
CS_SATURATED = 1024 * 256                                           # csrc/colstats.hip: colstats_blocks stays at 1024 blocks of 256 rows beyond


def _colstats(rng, N, n, form, scale, order, offset, const_col, null):
    """null: the output pointer that is NULL ("none": both given), through the C ABI"""
    return dict(family="colstats", N=N, n=n, form=form, scale=scale, order=order, offset=bool(offset), const_col=bool(const_col), null=null,
                seed=int(rng.integers(0, 1 << 30)))


COLSTATS_CORNERS = (
    # N     n   form          scale order       offset const_col null
    (1, 1, "host", 1.0, "walk", False, False, "none"),                         # one row: variance exactly 0
    (2, 2, "dev", 1e-4, "walk", True, False, "none"),
    (63, 3, "dev_stride", 50.0, "shuffled", False, True, "none"),
    (64, 12, "dev_stride", 1.0, "walk", True, False, "mean"),                  # x_stride 13
    (65, 13, "block_odd", 1e4, "blobs", False, False, "var"),
    (255, 16, "block_even", 1.0, "walk", True, True, "none"),
    (256, 12, "block_odd", 1e-4, "shuffled", True, False, "none"),             # one full block
    (257, 13, "block_even", 50.0, "walk", False, False, "none"),               # two blocks
    (1023, 2, "host", 1e4, "blobs", True, False, "none"),
    (1025, 16, "dev", 1.0, "shuffled", False, True, "none"),                   # five blocks, the last with one row
    # beyond 1024 blocks x 256 rows, a second trip of the first 257 lanes.  Blobs about 0: NumPy's own mean over axis 0 adds the rows one
    # after the other, and on a walk of this length (column means of ~10) or far from 0 its error exceeds a tenth of the bound (0.22 .. 0.25)
    (262401, 12, "block_even", 1.0, "blobs", False, False, "none"),
    (262401, 3, "dev_stride", 50.0, "blobs", False, False, "var"),
)


def draw_colstats(rng):
    s = SETS["colstats"]
    N, order, offset = _pick(rng, s["N"]), _pick(rng, s["order"]), _pick(rng, s["offset"])
    if N > CS_SATURATED:                                              # (see the corner list)
        order, offset = "blobs", False
    return _colstats(rng, N, _pick(rng, s["n"]), _pick(rng, s["form"]), _pick(rng, s["scale"]), order, offset, _pick(rng, s["const_col"]),
                     _pick(rng, s["null"]))


# ------------------------------------------------------------------------------------------ k-means: k-means++ seeding
PP_CHUNK, PP_ROW, PP_SCREEN_FROM, PP_LMAX = 4096, 16, 8, 16             # csrc/kmeans.hip
PP_WORK = 2.0e8                                                     # (k - 1) trials N n of a case at most: the reference is long double (1 .. 2 s
                                                                    # at 1e8; the corner list spreads such cases over the four slices)


def pp_trials(c):
    return _sym(c["trials_as"].replace("sk", str(2 + int(np.log(c["k"])))))


def _kmeanspp(rng, N, k, trials, n, mean, form, scale, order, offset, const_col, first, ind):
    """trials: candidates per round: "1", scikit-learn's 2 + int(log k) ("sk") or PP_LMAX; mean: column means given (else NULL: the data
    are taken as they are, and offset is off); first: first_index as a symbol of N; ind: indices_host given.  The uniforms are the case's
    own (seeded), not a RandomState's: tests/sweep_kmeans.py feeds the same numbers to scikit-learn."""
    assert 1 <= k <= N, (N, k)
    c = dict(family="kmeanspp", N=N, k=k, trials_as=trials, n=n, mean=bool(mean), form=form, scale=scale, order=order,
             offset=bool(offset and mean), const_col=bool(const_col and n > 1), first=_sym(first, N=N), first_as=first, ind=bool(ind),
             seed=int(rng.integers(0, 1 << 30)))
    c["trials"] = pp_trials(c)
    assert (k - 1) * c["trials"] * N * n <= PP_WORK, c
    return c


KMEANSPP_CORNERS = (
    # N     k    trials n  mean   form          scale order       offset const_col first  ind
    (1, 1, "sk", 1, True, "host", 1.0, "walk", False, False, "0", True),
    (15, 2, "1", 2, False, "dev", 1e-4, "walk", False, False, "N-1", True),            # below one PP_ROW
    (16, 3, "16", 5, True, "dev_stride", 1e4, "shuffled", True, False, "0", True),     # one row of 16, PP_LMAX candidates
    (17, 7, "sk", 12, True, "dev_stride", 1.0, "walk", False, False, "N-1", False),    # x_stride 13; no indices
    # k = N: the last round has one row left.  One candidate per round: with more, two mutually nearest rows are drawn together in some
    # round of every seed, and their potentials tie in exact arithmetic (tests/stress_parity.py: kmeanspp)
    (60, 60, "1", 13, True, "block_odd", 1.0, "blobs", False, False, "0", True),
    (4097, 512, "sk", 5, True, "dev", 1.0, "walk", False, False, "0", True),           # two chunks, the second with one row; 8 trials
    (4096, 9, "16", 12, True, "block_odd", 1e4, "walk", True, True, "0", True),        # one full chunk; the first screened round
    (4095, 8, "sk", 16, False, "block_even", 1e-4, "walk", False, False, "N-1", True), # the last round before the screening
    (8191, 64, "sk", 12, True, "dev", 1.0, "walk", True, False, "0", False),
    (8192, 9, "sk", 1, False, "host", 1.0, "blobs", False, False, "N-1", True),
    (12289, 20, "16", 13, True, "block_even", 1e-4, "walk", False, True, "N-1", True), # four chunks, the last with one row
    (8193, 20, "1", 13, True, "block_even", 1.0, "shuffled", False, False, "N-1", True),
    (70001, 20, "sk", 12, True, "dev_stride", 1.0, "walk", False, False, "0", True),   # most rows screened out
    (60, 2, "16", 2, True, "host", 1e4, "walk", True, False, "N-1", True),
)


def draw_kmeanspp(rng):
    s = SETS["kmeanspp"]
    while True:
        N, n, trials = _pick(rng, s["N"]), _pick(rng, s["n"]), _pick(rng, s["trials"])
        k = _pick(rng, [v for v in s["k"] if v <= N])
        L = _sym(trials.replace("sk", str(2 + int(np.log(k)))))
        if (k - 1) * L * N * n <= PP_WORK:                             # a draw beyond the work budget is drawn again
            break
    return _kmeanspp(rng, N, k, trials, n, _pick(rng, s["mean"]), _pick(rng, s["form"]), _pick(rng, s["scale"]), _pick(rng, s["order"]),
                     _pick(rng, s["offset"]), _pick(rng, s["const_col"]), _pick(rng, s["first"]), _pick(rng, s["ind"]))


# ------------------------------------------------------------------------------------------ k-means: Lloyd's loop
KM_SORTED_FROM = 1 << 18                                            # csrc/capi.hip: the loop keeps a sorted sample order from here on
KM_LDS_BYTES = 150 * 1024                                           # k (n + 1) 8 at most
KM_ALLZERO = (12, 6)                                                # (N, k) of the integer-point set of init "allzero"


def lloyd_paths(c):
    """what csrc/capi.hip: edmdc_kmeans_lloyd_dev picks for a case at the default variant: (filter, sorting, packed-fp32 kernel,
    screening inside the LDS / DPP kernel, distance bounds)"""
    N, n, k = c["N"], c["n"], c["k"]
    filt = k >= 64
    lds = n <= 14 and k <= 512                                      # kmeans_lds_form: the kernel that reads through the permutation
    pk_ok = n in (12, 13) and 64 <= k <= 1024
    big = not lds and pk_ok
    sorting = filt and (lds or big) and N >= KM_SORTED_FROM
    pk = sorting and big
    pk_lds = sorting and not pk and pk_ok and lds
    return filt, sorting, pk, pk_lds, pk_lds


def _lloyd(rng, N, n, k, stop, max_iter, init, form, scale, order, offset, const_col):
    """stop: "max_iter" tol_abs = 0 and the loop runs max_iter iterations with labels still moving; "strict" tol_abs = 0 and the labels
    stop moving before max_iter; "shift" tol_abs = 1e-4 mean(var) (scikit-learn's) and the centre shift falls below it before max_iter.
    init: "rows" k distinct rows; "dup" rows with centres 1 and k - 1 copies of centre 0 (exact ties, empty clusters: a relocation);
    "far2" / "far3" rows with two / three centres far from all data; "allzero" the integer-point set whose distances are all zero.
    From 2^18 rows on the case runs with bounds_rate 1 and `expect` names what kmeans_loop_info must show."""
    if init == "allzero":
        N, k, n = KM_ALLZERO[0], KM_ALLZERO[1], max(n, 4)
    assert 1 <= k <= N and k * (n + 1) * 8 <= KM_LDS_BYTES and n <= 15, (N, n, k)
    c = dict(family="lloyd", N=N, n=n, k=k, stop=stop, max_iter=max_iter, init=init, form=form, scale=scale, order=order, offset=bool(offset),
             const_col=bool(const_col and n > 1), seed=int(rng.integers(0, 1 << 30)))
    _, sorting, _, _, bnd = lloyd_paths(c)
    c["rate1"] = bool(sorting)
    c["expect"] = (["resort"] if sorting else []) + (["list"] if bnd else [])
    return c


LLOYD_CORNERS = (
    # N       n   k     stop        max_iter init     form          scale  order       offset const_col
    (1, 1, 1, "max_iter", 1, "rows", "host", 1.0, "walk", False, False),
    (63, 2, 2, "max_iter", 3, "rows", "dev", 1e-4, "walk", True, False),
    (64, 5, 63, "max_iter", 1, "rows", "dev_stride", 50.0, "shuffled", False, False),          # the last k without the filter
    (65, 12, 64, "max_iter", 1, "rows", "dev_stride", 1.0, "walk", False, True),               # the first with it; x_stride 13: scalar loads
    (1023, 13, 65, "max_iter", 3, "rows", "block_odd", 1.0, "walk", True, False),              # two mask words
    (16385, 13, 65, "shift", 60, "rows", "block_odd", 1.0, "walk", True, False),               # stops on the shift (below ~1e4 rows the labels settle first)
    (1024, 14, 128, "max_iter", 3, "rows", "block_even", 1e4, "walk", False, False),           # vec loads with a stride other than n
    (1025, 15, 256, "max_iter", 3, "rows", "block_odd", 1.0, "shuffled", False, False),        # n = 15: beyond the LDS / DPP kernel
    (1024, 5, 2, "strict", 60, "rows", "dev", 1.0, "blobs", False, False),                     # to strict convergence
    (12, 5, 1, "strict", 5, "allzero", "host", 1.0, "walk", False, False),                     # _average_centers copies the SUM
    (1025, 12, 64, "max_iter", 6, "dup", "host", 1.0, "walk", False, False),                   # exact ties; a relocation
    (16385, 12, 64, "shift", 60, "far2", "dev", 1.0, "walk", True, False),                     # two empties, the library's selection rule
    (1025, 13, 65, "max_iter", 5, "far3", "block_even", 50.0, "walk", False, False),           # three
    (16385, 12, 512, "max_iter", 3, "rows", "block_even", 1.0, "walk", True, False),           # one past KM_THREADS KM_EPOCH_PASSES; the last k of the table
    (16385, 13, 513, "max_iter", 2, "rows", "dev", 50.0, "walk", False, False),                # the first beyond it
    (16385, 12, 1024, "max_iter", 2, "rows", "dev", 1e-4, "shuffled", False, True),
    (16385, 15, 1200, "max_iter", 2, "rows", "host", 1.0, "walk", False, False),               # k (n + 1) 8 = 150 KiB exactly
    # every sample (or all but two) its own centre: an inertia of 0, or tiny against sum |x|^2 -- what the expanded form
    # |x|^2 - 2 (x.c - |c|^2 / 2) of the E-step kernels cannot give to a relative bound (it returned 8.4e-15 and missed by 2.0e-10 here)
    (63, 1, 63, "max_iter", 1, "rows", "dev_stride", 50.0, "shuffled", True, False),
    (65, 1, 63, "max_iter", 1, "rows", "block_even", 50.0, "walk", True, False),
    # from 2^18 rows on: the sorted order; max_iter is the smallest at which kmeans_loop_info shows what `expect` names, found on an MI355X
    # with bounds_rate 1: the first re-sort falls into iteration 3 in all eight, the first list-form E-step into iteration 4
    (262143, 12, 64, "max_iter", 3, "rows", "dev", 1.0, "walk", False, False),                 # the last size in the caller's order
    (262144, 12, 64, "max_iter", 4, "rows", "dev", 1.0, "walk", False, False),                 # the first sorted one: screening, bounds
    (262145, 13, 128, "max_iter", 4, "rows", "block_odd", 50.0, "shuffled", False, False),
    (264193, 12, 256, "max_iter", 4, "rows", "block_even", 1.0, "walk", True, False),          # 2^18 + 2049: a bounds tile of one row
    (262144, 5, 128, "max_iter", 3, "rows", "host", 1.0, "walk", False, False),                # sorted, no screening, no bounds
    (262145, 13, 600, "max_iter", 3, "rows", "dev_stride", 1.0, "walk", False, False),         # the packed-fp32 kernel
    (264193, 13, 512, "max_iter", 4, "rows", "dev", 1e-13, "walk", False, False),              # M^2 below 1e-24: screening off by prm[5]
    (262144, 12, 512, "max_iter", 4, "rows", "dev", 1e13, "shuffled", False, False),           # M^2 above 1e24
    (262145, 13, 513, "max_iter", 3, "rows", "block_even", 1.0, "walk", False, True),          # the packed-fp32 kernel at its first k
    (1048576, 2, 2, "max_iter", 2, "rows", "dev", 1.0, "walk", False, False),                  # member sums beyond 2^64: the high word of km_to_double
)

LLOYD_DRAW_N = tuple(v for v in SETS["lloyd"]["N"] if v < KM_SORTED_FROM - 1)      # draws stay below the sorted loop: its cases are hand-tuned


def draw_lloyd(rng):
    s = SETS["lloyd"]
    N, n = _pick(rng, LLOYD_DRAW_N), _pick(rng, s["n"])
    k = _pick(rng, [v for v in s["k"] if v <= N and v * (n + 1) * 8 <= KM_LDS_BYTES])
    init = _pick(rng, [v for v in ("rows", "rows", "dup", "far2", "far3") if v == "rows" or (k >= 8 and 1000 <= N <= 1025)])
    stop = "shift" if (63 <= k <= 128 and N == 16385 and init == "rows" and rng.integers(0, 2)) else "max_iter"
    max_iter = 60 if stop == "shift" else 1 if (k * 2 > N or k <= 2) else int(_pick(rng, (1, 2, 3, 5)))      # few or single-row clusters settle at once
    return _lloyd(rng, N, n, k, stop, max_iter, init, _pick(rng, s["form"]), _pick(rng, [v for v in s["scale"] if 1e-12 < v < 1e12]),
                  _pick(rng, ("walk", "shuffled")), _pick(rng, s["offset"]), _pick(rng, s["const_col"]))


# ------------------------------------------------------------------------------------------ unscented RTS smoother
SMOOTH_OUTS = ("xs", "pstd_s", "Ps", "Ps0", "sinfo")                # bluerov2_dynamics_amd/engine.py: UKF_SMOOTH_OUTPUTS
SMOOTH_WANT = {"all": SMOOTH_OUTS, "xs+sinfo": ("xs", "sinfo"), "Ps0": ("Ps0",), "pstd_s+Ps": ("pstd_s", "Ps")}
SMOOTH_RECORD = 312 * 8                                             # bytes of a tape record: 2496
SMOOTH_T_DRAW = (1, 2, 2, 3, 3, 12, 12, 12)                         # the weights of a draw's T: one in eight is a single row


def smooth_tape_bytes(c):
    """the tape_bytes a case passes: room for `chunk` recordings ("whole": for all B, and never below the one block of UKF_WAVES = 4
    recordings that the host demands)"""
    return c["P"] * (max(c["B"], 4) if c["chunk"] == "whole" else c["chunk"]) * c["T"] * SMOOTH_RECORD


def smooth_chunks(c):
    """the recordings per launch pair of brov_ukf_smooth under smooth_tape_bytes(c), by the rule of csrc/capi.hip: ukf_filter -- what
    fits, rounded down to whole blocks of 4, unless all B fit"""
    fit = smooth_tape_bytes(c) // (c["P"] * c["T"] * SMOOTH_RECORD)
    step = c["B"] if fit >= c["B"] else fit // 4 * 4
    return [min(step, c["B"] - b0) for b0 in range(0, c["B"], step)]


def _smooth(rng, model, integ, lag_mode, lag, P, nrec, alpha, B, T, measured, r_inf, q_zero, wrap, chunk, terminal, want):
    """the fields of _ukf (tests/sweep_ukf_lmpc.py: ukf_inputs reads no other), then chunk: the recordings the tape budget of the
    chunked call has room for ("whole": all); terminal: the two-call path passes a terminal pair (tests/sweep_smooth.py:
    terminal_pair); want: the smoother outputs asked for, by the names of SMOOTH_WANT"""
    c = _ukf(rng, model, integ, lag_mode, lag, P, nrec, alpha, B, T, measured, r_inf, q_zero, wrap)
    c.update(family="smooth", chunk=chunk, terminal=bool(terminal), want=list(SMOOTH_WANT[want]), want_as=want)
    return c


SMOOTH_CORNERS = (
    # model integ lag_mode lag  P  nrec alpha B  T  measured r_inf q_zero wrap chunk terminal want  -- every tape instantiation with a full and a ragged block
    (0, "euler", 0, True, 2, "1", 1.0, 4, 12, "std", 1, False, True, "whole", True, "all"),           # the yaw through pi into a terminal pair
    (0, "euler", 0, True, 1, "1", 0.5, 5, 12, "all", 0, True, False, 4, False, "all"),                # chunks 4 + 1; 12 updates a row; q = 0 on three components
    (0, "euler", 0, False, 3, "P", 1.0, 8, 3, "std", 3, False, False, 4, True, "xs+sinfo"),           # no start lag; nrec = P = 3 in chunks 4 + 4; T = 3 with a pair
    (0, "euler", 0, False, 2, "1", 0.5, 1, 12, "none", 1, True, False, "whole", False, "all"),        # B = 1, pure prediction
    (0, "rk4", 0, True, 2, "1", 1.0, 8, 12, "std", 1, False, False, 5, False, "all"),                 # room for 5, rounded down to 4: chunks 4 + 4
    (0, "rk4", 0, True, 3, "P", 0.5, 3, 2, "std", 0, True, False, "whole", False, "Ps0"),             # T = 2 without a pair: one transition, no prefetch
    (0, "rk4", 0, False, 2, "P", 1.0, 4, 1, "all", 0, False, False, "whole", True, "all"),            # T = 1 with a pair: one transition from the pair
    (0, "rk4", 0, False, 1, "1", 0.5, 13, 12, "std", 1, False, False, 4, False, "all"),               # chunks 4 + 4 + 4 + 1
    (0, "rk4", 1, True, 2, "1", 1.0, 4, 12, "all", 3, False, False, "whole", False, "pstd_s+Ps"),
    (0, "rk4", 1, True, 1, "1", 0.5, 3, 2, "std", 1, True, False, 4, True, "all"),                    # T = 2 with a pair
    (0, "rk4", 1, False, 1, "1", 1.0, 8, 12, "std", 0, False, True, 8, True, "all"),
    (0, "rk4", 1, False, 3, "1", 0.5, 5, 1, "none", 1, False, False, 4, False, "all"),                # T = 1 without a pair: the loop and the fetch never run
    (1, "euler", 0, False, 2, "P", 1.0, 8, 3, "all", 0, True, False, 5, False, "all"),                # T = 3 without a pair; room for 5 at B = 8
    (1, "euler", 0, False, 1, "1", 0.5, 9, 12, "std", 3, False, True, 4, True, "all"),                # chunks 4 + 4 + 1
    (1, "rk4", 0, False, 3, "1", 1.0, 4, 12, "std", 1, False, False, "whole", False, "all"),
    (1, "rk4", 0, False, 2, "P", 0.5, 1, 1, "none", 0, False, False, "whole", True, "all"),           # B = 1, T = 1, a pair
    (1, "rk4", 0, False, 3, "P", 1.0, 9, 3, "std", 0, False, False, 4, False, "all"),                 # nrec = P = 3 in chunks 4 + 4 + 1
    (1, "rk4", 0, False, 1, "1", 1.0, 13, 12, "all", 0, True, False, 8, False, "all"),                # chunks 8 + 5: a ragged second chunk
    (0, "rk4", 0, False, 2, "1", 1.0, 8, 12, "std", 1, False, False, 8, False, "all"),                # two full blocks without a start lag, 12 rows
    (1, "euler", 0, False, 2, "1", 0.5, 8, 12, "std", 1, False, False, "whole", True, "xs+sinfo"),    # two full blocks of the wrench model, 12 rows
)


def draw_smooth(rng):
    s = SETS["smooth"]
    while True:
        P, B, T = _pick(rng, s["P"]), _pick(rng, s["B"]), _pick(rng, SMOOTH_T_DRAW)
        if P * B * T <= UKF_ROWS:                                     # a draw beyond the row budget is drawn again
            break
    return _smooth(rng, _pick(rng, s["model"]), _pick(rng, s["integ"]), _pick(rng, s["lag_mode"]), _pick(rng, s["lag"]), P, _pick(rng, s["nrec"]),
                   _pick(rng, s["alpha"]), B, T, _pick(rng, s["measured"]), _pick(rng, s["r_inf"]), _pick(rng, s["q_zero"]), _pick(rng, s["wrap"]),
                   _pick(rng, s["chunk"]), _pick(rng, s["terminal"]), _pick(rng, s["want"]))


# ------------------------------------------------------------------------------------------ quaternion-model UKF and RTS smoother
SMOOTH_QUAT_RECORD = 313 * 8                                        # bytes of a tape record of the quaternion model: 2504
QUAT_BLOCK = 4                                                      # UKF_WAVES: the recordings of a block, the unit of `chunk`


def _ukf_quat(rng, integ, P, nrec, alpha, B, T, measured, r_inf, q_zero, attitude, spread):
    """nrec, measured, r_inf, q_zero as in _ukf (r_inf in the error state: component 7, then 2, then the attitude component 4 while 3 and
    5 are updated).  attitude: the start of every recording -- "level" Euler angles in +-0.3, "vertical" the pitch within 0.1 rad of 90
    degrees, x0's quaternion negated and every third measured quaternion times -2, "sphere" a uniformly random unit quaternion with the
    sign as drawn, "inverted" the roll within 0.1 rad of pi and the yaw at +-(pi - 0.05).  spread: "wide" gives the attitude block of
    P0 a sigma of QUAT_WIDE_SIGMA in chart units (tests/sweep_quat.py).  The recordings are simulated with the last candidate's vehicle."""
    assert P * B * T <= UKF_ROWS, (P, B, T)
    return dict(family="ukf_quat", integ=integ, P=P, nrec=_sym(nrec, P=P), nrec_as=nrec, alpha=alpha, B=B, T=T, measured=measured, r_inf=r_inf,
                q_zero=bool(q_zero), attitude=attitude, spread=spread, names=_vehicles(rng, 2, P), seed=int(rng.integers(0, 1 << 30)))


UKF_QUAT_CORNERS = (
    # integ  P  nrec alpha B  T  measured r_inf q_zero attitude spread
    ("euler", 2, "P", 1.0, 4, 12, "std", 1, False, "level", "std"),                # a full block alone
    ("rk4", 3, "P", 0.5, 5, 12, "all", 0, True, "sphere", "wide"),                 # blockIdx.y = 2 reads its own record; 12 updates in every row
    ("euler", 3, "P", 1.0, 5, 12, "all", 3, False, "inverted", "wide"),            # r = +inf on attitude component 4, 3 and 5 updated, every row
    ("rk4", 1, "1", 1.0, 4, 12, "none", 1, False, "vertical", "std"),              # pure prediction over 12 rows
    ("euler", 1, "1", 0.5, 1, 1, "none", 0, False, "vertical", "std"),             # B = 1, T = 1, no measurement
    ("rk4", 2, "1", 0.5, 8, 12, "std", 1, True, "level", "std"),                   # two full blocks
    ("euler", 1, "1", 1.0, 9, 12, "std", 0, False, "sphere", "std"),               # three blocks, the last with one wave
    ("rk4", 1, "1", 1.0, 9, 2, "std", 3, False, "inverted", "std"),
    ("euler", 2, "1", 0.5, 3, 3, "std", 1, True, "inverted", "std"),
    ("rk4", 3, "P", 1.0, 3, 2, "all", 0, False, "level", "wide"),
    ("euler", 1, "1", 1.0, 8, 1, "all", 0, False, "sphere", "wide"),
    ("rk4", 2, "P", 0.5, 1, 12, "std", 1, False, "sphere", "std"),
    ("euler", 3, "1", 0.5, 4, 3, "std", 0, False, "vertical", "wide"),
    ("rk4", 2, "1", 1.0, 5, 1, "std", 1, False, "vertical", "std"),
    ("euler", 1, "1", 1.0, 13, 12, "all", 0, True, "level", "std"),                # four blocks, the last with one wave
    ("rk4", 3, "P", 1.0, 4, 3, "none", 3, False, "inverted", "wide"),
)


def _draw_quat_shape(rng, s, t_set):
    while True:
        P, B, T = _pick(rng, s["P"]), _pick(rng, s["B"]), _pick(rng, t_set)
        if P * B * T <= UKF_ROWS:                                     # a draw beyond the row budget is drawn again
            return P, B, T


def draw_ukf_quat(rng):
    s = SETS["ukf_quat"]
    P, B, T = _draw_quat_shape(rng, s, s["T"])
    return _ukf_quat(rng, _pick(rng, s["integ"]), P, _pick(rng, s["nrec"]), _pick(rng, s["alpha"]), B, T, _pick(rng, s["measured"]),
                     _pick(rng, s["r_inf"]), _pick(rng, s["q_zero"]), _pick(rng, s["attitude"]), _pick(rng, s["spread"]))


def smooth_quat_tape_bytes(c):
    """the tape_bytes a case passes: room for `chunk` blocks of QUAT_BLOCK recordings (1.5: six recordings, which the host rounds down
    to one block; 0: for all B, and never below the one block that the host demands)"""
    return c["P"] * (max(c["B"], QUAT_BLOCK) if c["chunk"] == 0 else int(c["chunk"] * QUAT_BLOCK)) * c["T"] * SMOOTH_QUAT_RECORD


def smooth_quat_chunks(c):
    """the recordings per launch pair of brov_ukf_smooth_quat under smooth_quat_tape_bytes(c), by the rule of csrc/capi.hip:
    ukf_filter_quat -- what fits, rounded down to whole blocks, unless all B fit"""
    fit = smooth_quat_tape_bytes(c) // (c["P"] * c["T"] * SMOOTH_QUAT_RECORD)
    step = c["B"] if fit >= c["B"] else fit // QUAT_BLOCK * QUAT_BLOCK
    return [min(step, c["B"] - b0) for b0 in range(0, c["B"], step)]


def _smooth_quat(rng, integ, P, nrec, alpha, B, T, measured, r_inf, q_zero, attitude, spread, chunk, terminal, want):
    """the fields of _ukf_quat, then chunk: the blocks of recordings the tape budget of the chunked call has room for (0: all B);
    terminal: the two-call path passes a terminal pair (tests/sweep_quat.py: terminal_pair); want as in _smooth"""
    c = _ukf_quat(rng, integ, P, nrec, alpha, B, T, measured, r_inf, q_zero, attitude, spread)
    c.update(family="smooth_quat", chunk=chunk, terminal=bool(terminal), want=list(SMOOTH_WANT[want]), want_as=want)
    return c


SMOOTH_QUAT_CORNERS = (
    # integ  P  nrec alpha B  T  measured r_inf q_zero attitude spread chunk terminal want
    ("euler", 2, "P", 1.0, 8, 12, "std", 1, False, "level", "std", 1, False, "all"),                # chunks 4 + 4 under Euler; two full blocks
    ("rk4", 2, "P", 0.5, 8, 12, "std", 1, False, "sphere", "std", 0, True, "all"),                  # a pair at T = 12 from anywhere on the sphere
    ("rk4", 3, "P", 1.0, 9, 3, "std", 0, False, "level", "std", 1, False, "all"),                   # nrec = P = 3 in chunks 4 + 4 + 1: loc != row at blockIdx.y = 2
    ("euler", 3, "P", 0.5, 5, 12, "all", 3, False, "inverted", "wide", 1, False, "xs+sinfo"),       # chunks 4 + 1, xf scratch; +inf on attitude component 4
    ("rk4", 3, "P", 1.0, 5, 12, "all", 0, True, "sphere", "wide", 0, False, "xs+sinfo"),            # xf scratch in one chunk; 12 updates a row
    ("rk4", 1, "1", 1.0, 13, 12, "std", 1, False, "level", "std", 2, False, "all"),                 # chunks 8 + 5: a ragged second chunk
    ("euler", 1, "1", 0.5, 1, 1, "none", 0, False, "vertical", "std", 0, False, "all"),             # B = 1, T = 1 without a pair: the loop never runs
    ("rk4", 1, "1", 1.0, 4, 1, "std", 1, False, "vertical", "std", 0, True, "all"),                 # T = 1 with a pair: the loop starts at t = n - 1 = 0
    ("euler", 2, "1", 1.0, 4, 2, "std", 1, False, "sphere", "std", 0, True, "Ps0"),                 # T = 2 with a pair
    ("rk4", 2, "1", 0.5, 3, 2, "all", 0, False, "inverted", "std", 0, False, "all"),                # T = 2 without: fetch(t - 1) never taken
    ("euler", 1, "1", 1.0, 9, 3, "std", 3, False, "inverted", "std", 1.5, True, "Ps0"),             # T = 3 with a pair; room for 6 rounded down: 4 + 4 + 1
    ("rk4", 3, "1", 0.5, 3, 3, "none", 1, False, "level", "wide", 0, False, "pstd_s+Ps"),           # T = 3 without a pair
    ("euler", 1, "1", 1.0, 8, 12, "none", 1, True, "level", "std", 1, False, "pstd_s+Ps"),          # pure prediction over 12 rows, in chunks
    ("rk4", 1, "1", 1.0, 5, 12, "all", 0, True, "vertical", "std", 1, True, "all"),                 # chunks 4 + 1 under RK4
    ("euler", 1, "1", 0.5, 13, 12, "std", 0, False, "vertical", "wide", 1, False, "all"),           # chunks 4 + 4 + 4 + 1: two middle chunks
    ("rk4", 1, "1", 1.0, 8, 12, "std", 1, False, "inverted", "wide", 1.5, False, "all"),            # room for 6 of 8: chunks 4 + 4
    ("euler", 2, "1", 0.5, 5, 12, "std", 1, False, "sphere", "wide", 0, True, "all"),
    ("rk4", 1, "1", 1.0, 1, 12, "std", 1, False, "sphere", "std", 0, False, "all"),                 # B = 1 over 12 rows
    ("euler", 3, "P", 1.0, 4, 12, "all", 0, False, "level", "std", 0, True, "all"),
    ("rk4", 2, "1", 1.0, 4, 12, "std", 1, False, "level", "std", 0, False, "all"),                  # the corner of the terminal-pair and short-prefix test
)


def draw_smooth_quat(rng):
    s = SETS["smooth_quat"]
    P, B, T = _draw_quat_shape(rng, s, SMOOTH_T_DRAW)
    return _smooth_quat(rng, _pick(rng, s["integ"]), P, _pick(rng, s["nrec"]), _pick(rng, s["alpha"]), B, T, _pick(rng, s["measured"]),
                        _pick(rng, s["r_inf"]), _pick(rng, s["q_zero"]), _pick(rng, s["attitude"]), _pick(rng, s["spread"]), _pick(rng, s["chunk"]),
                        _pick(rng, s["terminal"]), _pick(rng, s["want"]))


# ------------------------------------------------------------------------------------------ the lists
_MAKE = dict(rollout_pop=(_rollout_pop, ROLLOUT_POP_CORNERS, draw_rollout_pop), feedback=(_feedback, FEEDBACK_CORNERS, draw_feedback),
             mppi=(_mppi, MPPI_CORNERS, draw_mppi), koopman_mppi=(_koopman_mppi, KOOPMAN_MPPI_CORNERS, draw_koopman_mppi),
             window_pop=(_window_pop, WINDOW_POP_CORNERS, draw_window_pop),
             lift=(_lift, LIFT_CORNERS, draw_lift), gram=(_gram, GRAM_CORNERS, draw_gram),
             pinv_apply=(_pinv_apply, PINV_APPLY_CORNERS, draw_pinv_apply), multistep=(_multistep, MULTISTEP_CORNERS, draw_multistep),
             simulate=(_simulate, SIMULATE_CORNERS, draw_simulate), ukf=(_ukf, UKF_CORNERS, draw_ukf), lmpc=(_lmpc, LMPC_CORNERS, draw_lmpc),
             colstats=(_colstats, COLSTATS_CORNERS, draw_colstats), kmeanspp=(_kmeanspp, KMEANSPP_CORNERS, draw_kmeanspp),
             lloyd=(_lloyd, LLOYD_CORNERS, draw_lloyd), smooth=(_smooth, SMOOTH_CORNERS, draw_smooth),
             ukf_quat=(_ukf_quat, UKF_QUAT_CORNERS, draw_ukf_quat), smooth_quat=(_smooth_quat, SMOOTH_QUAT_CORNERS, draw_smooth_quat))
FAMILIES = tuple(_MAKE)                                             # the order is part of the seeds: new families go last
EDMDC_FAMILIES = ("lift", "gram", "pinv_apply", "multistep", "simulate")
N_CORNERS = {f: len(_MAKE[f][1]) for f in FAMILIES}                 # 12 for the five older families
FILTER_FAMILIES = ("ukf", "lmpc", "smooth", "ukf_quat", "smooth_quat")
KMEANS_FAMILIES = ("colstats", "kmeanspp", "lloyd")
N_CASES_OF = {f: N_CASES_EDMDC if f in EDMDC_FAMILIES else N_CASES_FILTER if f in FILTER_FAMILIES else N_CASES_KMEANS if f in KMEANS_FAMILIES
              else N_CASES for f in FAMILIES}
# a case whose reference is not decided (tests/sweep_kmeans.py) gets another data seed here: (family, index in the list) -> seed
KM_RESEED = {("colstats", 10): 6}        # NumPy's own axis-0 mean at N = 262 401, n = 12: 0.13 .. 0.25 of the bound on six seeds of eight, 0.065 on this one


def _reseeded(family, seed, out):
    """KM_RESEED applied to the first len(out) cases of the list at the pinned SEED (another seed gives another list altogether)"""
    if seed == SEED:
        for (f, i), data_seed in KM_RESEED.items():
            if f == family and i < len(out):
                out[i] = dict(out[i], seed=data_seed)
    return out


def corners(family, seed=SEED):
    make, rows, _ = _MAKE[family]
    rng = np.random.default_rng([seed, FAMILIES.index(family), 0])
    return _reseeded(family, seed, [make(rng, *row) for row in rows])


def cases(family, seed=SEED, n=None):
    """the corner list, then seeded draws up to n cases (N_CASES_OF[family] unless given)"""
    n = N_CASES_OF[family] if n is None else n
    out = corners(family, seed)
    rng = np.random.default_rng([seed, FAMILIES.index(family), 1])
    while len(out) < n:
        out.append(_MAKE[family][2](rng))
    return _reseeded(family, seed, out)


def rollout_pop(seed=SEED):
    return cases("rollout_pop", seed)


def feedback(seed=SEED):
    return cases("feedback", seed)


def mppi(seed=SEED):
    return cases("mppi", seed)


def koopman_mppi(seed=SEED):
    return cases("koopman_mppi", seed)


def window_pop(seed=SEED):
    return cases("window_pop", seed)


def lift(seed=SEED):
    return cases("lift", seed)


def gram(seed=SEED):
    return cases("gram", seed)


def pinv_apply(seed=SEED):
    return cases("pinv_apply", seed)


def multistep(seed=SEED):
    return cases("multistep", seed)


def simulate(seed=SEED):
    return cases("simulate", seed)


def ukf(seed=SEED):
    return cases("ukf", seed)


def lmpc(seed=SEED):
    return cases("lmpc", seed)


def colstats(seed=SEED):
    return cases("colstats", seed)


def kmeanspp(seed=SEED):
    return cases("kmeanspp", seed)


def lloyd(seed=SEED):
    return cases("lloyd", seed)


def smooth(seed=SEED):
    return cases("smooth", seed)


def ukf_quat(seed=SEED):
    return cases("ukf_quat", seed)


def smooth_quat(seed=SEED):
    return cases("smooth_quat", seed)
