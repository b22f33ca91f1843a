"""Start sets of test_rollout_rare_paths.py (and of tools/gen_rollout_rare_golden.py, which recorded the parent build's bits for them).

The body wave of rollout_pair_kernel has three kinds of code that a benchmark-like start hardly ever runs:
    the cos(theta) clamp of rhs_fast_euler, one copy per dynamics() call of a step (four for RK4), each behind a wave-level test;
    the range extension of trig_delta (halve the increment k times, double sin / cos - 1 back k times), two regions per call;
    NaN lanes, which take the range-extension path with a NaN scale.
Every set has B = 70 trajectories (one full wave and a partial one: 6 live lanes, 58 dead ones shadowing the last) and lane NAN_LANE
starts as NaN.  T = 130 crosses the 64-step sin/cos refresh twice and leaves an odd remainder.

bench   the benchmark's start: x0 = 0, iid controls of seed 0x5EED.
clamp   pitch within 1e-8 of +-pi/2 at a chosen dynamics() call of the first step (stage s = b % 4: RK4 calls 1..4; Euler has only the first).
        At the singularity the reference clamps cos(theta) to +-1e-7, so roll and yaw rate are +-1e7 (sin(phi) q + cos(phi) r): an O(1)
        roll angle or yaw rate there leaves the range in which a trajectory is a function of its start to 1e-11 within one step, a TINY one
        does not -- inside the clamp the reciprocal is exactly +-1e7 whatever the last bits of cos(theta) are, and a relative error eps in
        r becomes 1e7 eps r.  Four kinds of lane share every wave (kind = (b / 4 + 1) % 4), so that the clamped value, its sign and the
        lane mask it is written under all show in the result:
          0  in the pitch plane (phi = 0, v = p = r = 0, controls 0: the plane is invariant and the clamped reciprocal multiplies 0);
          1  the same with a yaw rate r0 of +-1e-8 .. 1e-6 rad/s: roll and yaw rate of 0.1 .. 10 rad/s in the clamped call (1e-4 of that for
             the lanes of RK4 calls 2..4, see clamp_set);
          2  the same with a roll angle phi0 of that size (sin(phi) q comparable);
          3  out of the plane (r0 = +-0.05) and 0.3 rad away from the singularity: never clamped, in a wave whose other lanes are.
        theta0 = +-pi/2 + delta - c h (pitch rate of the stage before) so that the call with stage offset c (0, 1/2, 1/2, 1) sees pitch
        +-pi/2 + delta, |delta| <= 1e-8; the neighbouring calls then sit at |cos(theta)| ~ h q ~ 1e-2.
fast    body rates of 8 to 150 rad/s about the roll or the yaw axis.  With the quadratic damping of the model the explicit integrators are
        unstable at dt = 0.02 above 36 rad/s (Euler) and 48 rad/s (RK4): the C oracle overflows within 9 and 3 steps, and before that
        its angle increments pass the 2^37 rad beyond which trig_delta returns NaN by design.  The set therefore runs at DT_FAST =
        0.004 s, where both integrators are stable over the whole range (limits 180 and 240 rad/s) and the oracle stays finite for all
        130 steps: angle increments per step up to 0.6 rad, i.e. beyond 1/8 (1/16 for the half-step stages) by one halving (k = 1) and
        by several (k = 2, 3) -- but only in the first two steps, so fast do the rates decay.
spin    the same at the benchmark's dt = 0.02 with rates of 8 to 34 rad/s, inside both stability limits: increments of 0.16 to 0.68 rad, and
        the range extension stays busy for eight or nine steps instead of two (profiles/rollout_hot_slots.md has the counts).
"""
import numpy as np

B, T, DT = 70, 130, 0.02
DT_FAST = 0.004
NAN_LANE = 66                   # in the partial wave: wave 0 of every set keeps its NaN-free common path
GOLD_LANES = (0, 63, 64, 69)    # first / last lane of the full wave, first / last live lane of the partial one
SETS = ("bench", "clamp", "fast", "spin")


def _with_nan(x0):
    x0 = x0.copy()
    x0[NAN_LANE, :] = np.nan
    return x0


def bench_set():
    from oracle import controls
    return _with_nan(np.zeros((B, 12))), controls.controls_iid(0x5EED, 0, B, T)


def clamp_kinds():
    """-> stage [B], kind [B] of the clamp set's lanes"""
    return np.arange(B) % 4, (np.arange(B) // 4 + 1) % 4


def clamp_set():
    """The pitch rate the s-th call integrates over is k_theta of the call before it (q0 for s = 1 up to the tiny out-of-plane terms), taken
    from the oracle's own right-hand side in a fixed-point sweep."""
    from oracle import fossen_c as fc
    rng = np.random.default_rng(0xC1A)
    x0 = np.zeros((B, 12))
    U = np.zeros((B, T, 8))
    stage, kind = clamp_kinds()
    sign = np.where(rng.integers(0, 2, B) == 0, -1.0, 1.0)
    delta = rng.uniform(-1e-8, 1e-8, B)
    q0 = -sign * rng.uniform(0.5, 2.0, B)           # pitching back towards level: one passage through the singularity, none on the way back
    q0[(stage == 0) & (kind == 0) & (np.arange(B) % 8 == 0)] = 0.0          # a start at rest, exactly at the singularity
    tiny = np.geomspace(1e-8, 1e-6, B)[rng.permutation(B)] * np.where(rng.integers(0, 2, B) == 0, -1.0, 1.0)
    # RK4 calls 2..4: the calls after the clamped one sit within h^2 qdot ~ 1e-4 of the singularity, unclamped (reciprocal ~ 1e4), and
    # multiply what the clamped call put into phi once more; 1e-12 .. 1e-10 keeps phi below 1e-3 there (roll rate 1e-5 .. 1e-3 in the clamp)
    tiny[stage > 0] *= 1e-4
    x0[:, 2] = 5.0
    x0[:, 5] = rng.uniform(-3.0, 3.0, B)            # yaw is free: the plane is the vertical plane of that heading
    x0[:, 6] = rng.uniform(-0.3, 0.3, B)            # surge and heave stay in the plane
    x0[:, 8] = rng.uniform(-0.3, 0.3, B)
    x0[:, 10] = q0
    x0[kind == 1, 11] = tiny[kind == 1]
    x0[kind == 2, 3] = tiny[kind == 2]
    x0[kind == 3, 11] = 0.05 * sign[kind == 3]
    target = sign * (np.pi / 2 - np.where(kind == 3, 0.3, 0.0)) + delta
    h = DT
    c = np.array([0.0, 0.5, 0.5, 1.0])[stage]
    th0 = target - c * h * q0
    for _ in range(3):
        x = x0.copy()
        x[:, 4] = th0
        k1, _ = fc.rhs(fc.MODEL_THRUSTER_EULER, x, np.zeros((B, 8)), dt=h)
        k2, _ = fc.rhs(fc.MODEL_THRUSTER_EULER, x + 0.5 * h * k1, np.zeros((B, 8)), dt=h)
        k3, _ = fc.rhs(fc.MODEL_THRUSTER_EULER, x + 0.5 * h * k2, np.zeros((B, 8)), dt=h)
        rate = np.stack([np.zeros(B), k1[:, 4], k2[:, 4], k3[:, 4]], axis=1)[np.arange(B), stage]
        th0 = target - c * h * rate
    x0[:, 4] = th0
    hit = np.abs(np.cos(th0 + c * h * rate))
    assert (hit[kind != 3] < 2e-8).all(), hit[kind != 3].max()     # inside the clamp's 1e-7 at its call, with room for the kernel's own rounding
    assert (hit[kind == 3] > 0.2).all()
    return _with_nan(x0), U


def fast_set(lo=8.0, hi=150.0, seed=0xFA57):
    rng = np.random.default_rng(seed)
    x0 = np.zeros((B, 12))
    x0[:, 2] = 5.0
    x0[:, 3:6] = rng.uniform(-0.1, 0.1, (B, 3))
    rate = np.geomspace(lo, hi, B)[rng.permutation(B)] * np.where(rng.integers(0, 2, B) == 0, -1.0, 1.0)
    x0[np.arange(B), 9 + 2 * (np.arange(B) % 2)] = rate      # roll or yaw: a pitch spin crosses theta = +-pi/2, where the trajectory stops being well-conditioned
    from oracle import controls
    return _with_nan(x0), controls.controls_iid(seed, 0, B, T)


def start_set(name):
    """-> x0 [B,12], U [B,T,8], dt"""
    x0, U = {"bench": bench_set, "clamp": clamp_set, "fast": fast_set, "spin": lambda: fast_set(8.0, 34.0, 0x5B1A)}[name]()
    return x0, U, (DT_FAST if name == "fast" else DT)


def layouts_of(U):
    """U [B,T,8] -> the three control layouts of engine.rollout"""
    b, t = U.shape[0], U.shape[1]
    return {"btu": U, "tub": np.ascontiguousarray(U.transpose(1, 2, 0)), "tpb": np.ascontiguousarray(U.reshape(b, t, 4, 2).transpose(1, 2, 0, 3))}


def to_btx(traj, lay, b):
    """stored states of any layout -> [B, rows, 12]"""
    if lay == "btu":
        return traj
    if lay == "tub":
        return traj.transpose(2, 0, 1)
    return traj.transpose(2, 0, 1, 3).reshape(b, -1, 12)


def canon(a):
    """NaNs to the one canonical quiet NaN: which operand's payload an instruction propagates is the compiler's choice"""
    a = np.array(a, dtype=np.float64)
    a[np.isnan(a)] = np.nan
    return a


def bits_equal(a, b):
    return np.array_equal(canon(a).view(np.uint64), canon(b).view(np.uint64))


def digest(a):
    import hashlib
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(canon(a)).tobytes()).digest(), dtype=np.uint8).copy()
