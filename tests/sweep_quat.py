"""What the shape sweeps do with a case of the families `ukf_quat` and `smooth_quat` of tests/sweep_cases.py: the multiplicative
unscented Kalman filter of the quaternion model (the four instantiations of ukf_quat_filter_kernel<INTEG, TAPE>, csrc/ukf_quat.hip) and
its Rauch-Tung-Striebel smoother (ukf_quat_rts_kernel and the chunked brov_ukf_smooth_quat, csrc/capi.hip: ukf_filter_quat).  prepare /
run / compare as in tests/sweep_run.py, which registers them, in the shape of tests/sweep_smooth.py.  Not collected.

Inputs (quat_inputs) by the recipe of tests/ukf_quat_cases.py: inputs, seeded by the case -- the oracle's WRENCH_QUAT rollout with the
last candidate's vehicle, commands of +-0.3 of the channel scale, noise of ukf_cases.SIGMA through [+], about 30 % of the measurements
dropped with a single missing quaternion number dropping the row's attitude, one row emptied where T > 1, numbers left in every
r = +inf column of Y, a dense positive-definite P0 whose upper triangle is NaN -- with what the case switches: the start attitude
(level; near vertical with x0's quaternion negated and every third measured quaternion times -2; anywhere on the sphere with the sign
as drawn; inverted with the yaw at +-(pi - 0.05)), the attitude block of P0 with a sigma of WIDE_SIGMA = 0.3 in chart units (c L moves
the sigma points' attitude by up to a radian), every entry measured or none, r = +inf on error components 7, 2 and 4 (the last one an
attitude component, while 3 and 5 are updated), three process variances of 0, a noise record per candidate.  WIDE_SIGMA = 0.3 is the
value the issue asked for; no lane of the two lists had to be left out at it, so it was never lowered.

The references are ukf_quat_ref.filter and ukf_quat_smooth_ref.smooth in float64 and in long double; for smooth_quat with the case's
terminal pair (terminal_pair: xT of the float64 reference moved through [+] by a normal draw of ukf_cases.SIGMA, a positive-definite
Ps_T between 0.3 and 0.8 of its PT, the upper triangle NaN) and, because the one-call smoother takes no pair, without it as well.  A
lane is one (candidate, recording) problem.  It is compared if its own float64-to-long-double gap in every measure is below a tenth
of TOL = 1e-10, the normalised |e_w| of every [-] taken, forward and backward, exceeds EW = 0.5, every forward and backward pivot
exceeds PIVOT = 1e-4, every row and transition completes, and both precisions count the same updates.  tests/test_sweep_cases_cpu.py
asserts that no lane of any case is left out.

The filter's measures: the mixed error of ukf_quat_cases.gaps on xf, pstd, innov, xT, info[0] and info[3], PT as |dP_ij| /
sqrt(P_ii P_jj), and the quaternion columns of xf and xT up to sign as min(|a - b|, |a + b|) (which the first measure bounds: the
kernel keeps the sign of x0's quaternion, as the reference does); info[1] and info[2] exactly.  The smoother's: those of
ukf_quat_smooth_ref.gaps (xs, pstd_s, Ps, Ps0, the tape's Pf, Pp, C and xp, sinfo[1]).

A smooth_quat case runs three ways: (a) engine.ukf_filter_quat(tape=True), then engine.ukf_rts_quat with the terminal pair; (b)
engine.ukf_smooth_quat in one chunk; (c) engine.ukf_smooth_quat with the case's tape_bytes and, where the case asks for a strict subset
of the smoother's outputs, for that subset alone (xf is then scratch inside the library), on the recordings in reversed order, so that
rows which a chunk failed to write cannot pass for written by holding what run (b) left in the same memory.  Compared: (a) against the reference with the
pair, (b) against the reference without it, filter outputs included; nrows = T and sinfo[0] = -1 exactly; Ps bit-symmetric, Ps0 =
Ps[:, :, 0], row T - 1 the filter's without a pair; the filter outputs of (a) the bits of the plain filter; (b) and (c) the same bits,
and those of (a) without a pair; with a pair xs of (a) and (b) apart by more than 1e3 TOL in every lane; what was not wanted None.

A recording without measurements (measured = "none").  For the Euler models the smoother then returns the filter bit for bit
(tests/sweep_smooth.py).  The quaternion law of include/brov2.h promises that only in part, and prediction_only asserts what it does
promise, of both references in prepare and of the kernel in the sweep:
  - pstd_s = pstd and Ps = Pf bit for bit.  Stage 1 applies no update, so Pf_{t+1} is Pp_{t+1} and, by induction from row T - 1,
    Ps_{t+1} - Pp_{t+1} is a difference of equal numbers, G 0 G^T is 0 and Pf_t + 0 is Pf_t.
  - row T - 1 of xs is xf's (the header says so of every call without a pair).
  - rows < T - 1 of xs equal xf to NONE_XS = 1e-13 in the mixed error, NOT bit for bit.  xf_{t+1} = xp_{t+1} [+] 0 does return
    xp_{t+1}'s bits (q (x) (1, 0, 0, 0) / sqrt(1) is exact), so xs_{t+1} and xp_{t+1} hold the same quaternion q.  But the vector part
    of e = conj(q) (x) q is q_0 q_i - q_i q_0 + q_j q_k - q_k q_j summed in the product's order, which is not pair by pair: the float64
    reference gives 1.8e-18 in one component of one problem of corner 11, and ukf_quat.hip forms each component as a chain of three
    fused multiply-adds on a rounded product, which leaves the rounding error of that product.  With four products and three sums of
    magnitude <= |q|^2, each rounded once or fused, |e_v| <= 7 x 2^-53 |q|^2, so |delta| = 2 |e_v| / e_w <= 1.6e-15 on the three
    attitude components and exactly 0 on the nine others, and |G delta| <= 3 max |G| x 1.6e-15 < 1e-13 for max |G| <= 20 (G = C Pp^-1
    is the inverse transition in units of the components' sigmas, whose ratios stay below 15 in these cases).  Making delta exactly
    0 would need a law that subtracts pair by pair; the header states none, and the kernel matches the reference to TOL either way."""
import numpy as np

import fossen_vehicles as fv
import sweep_cases as sc
import sweep_ukf_lmpc as su
import ukf_cases as uc
import ukf_quat_cases as qc
import ukf_quat_ref as uq
import ukf_quat_smooth_ref as qs
import ukf_ref as ur
from oracle import fossen_params as fp

L = np.longdouble
TOL, EW, PIVOT = qs.TOL, qs.EW, qs.PIVOT
DT = qc.DT
WIDE_SIGMA = 0.3
F_OUTS = su.UKF_OUTS
S_OUTS = sc.SMOOTH_OUTS
ROWS = ("xs", "pstd_s", "Ps")
TAPE_KEYS = ("tape", "nrows")
GAP_KEYS = S_OUTS + ("tape",)
TERMINAL_LO, TERMINAL_HI = 0.3, 0.8
NONE_XS = 1e-13                            # |xs - xf| on a recording without measurements (the module text)
YAW_INVERTED = np.pi - 0.05


# ------------------------------------------------------------------------------------------ the inputs
def start_states(rng, B, attitude):
    """[B,13]: positions and velocities in +-0.3 and the attitude of the case"""
    e = rng.uniform(-0.3, 0.3, (B, 12))
    if attitude == "sphere":
        q = rng.normal(size=(B, 4))
        q = q / np.linalg.norm(q, axis=1, keepdims=True)            # the sign stays as drawn: about half start with q_w < 0
    elif attitude == "vertical":
        q = qc.quat_of_euler(e[:, 3], np.pi / 2 + rng.uniform(-0.1, 0.1, B), e[:, 5])
    elif attitude == "inverted":
        q = qc.quat_of_euler(np.pi + rng.uniform(-0.1, 0.1, B), e[:, 4], rng.choice([-1.0, 1.0], B) * YAW_INVERTED)
    else:
        assert attitude == "level", attitude
        q = qc.quat_of_euler(e[:, 3], e[:, 4], e[:, 5])
    return np.concatenate([e[:, :3], q, e[:, 6:]], 1)


def y_column(i):
    """the column of Y that carries error component i alone, or None for an attitude component (the quaternion is measured as a group)"""
    return i if i < 3 else None if i < 6 else i + 1


def quat_inputs(case):
    """dict(cfgs, x0 [B,13], P0 [B,12,12], U [B,T,6], Y [B,T,13], X [B,T+1,13])"""
    c, rng = case, np.random.default_rng(case["seed"])
    B, T = c["B"], c["T"]
    xs = start_states(rng, B, c["attitude"])
    U = rng.uniform(-0.3, 0.3, (B, T, 6)) * uc.chan_scale(1)
    X = fp.rollout(fp.WRENCH_QUAT, su.INTEG[c["integ"]], 0, fv.vehicle(c["names"][-1]), xs, U, DT)["traj"]
    Y = qc.measure(rng, X[:, :T], drop=0.3 if c["measured"] == "std" else 0.0)
    if c["measured"] == "std" and T > 1:                           # one row without any measurement (a single row keeps its own)
        Y[:, min(qc.EMPTY_ROW, T - 1)] = np.nan
    if c["measured"] == "none":
        Y[:] = np.nan
    for i in su.UKF_NEVER[:c["r_inf"]]:
        if y_column(i) is not None:
            Y[:, :, y_column(i)] = X[:, :T, y_column(i)] + 5.0      # numbers the filter must not look at (the quaternion keeps its own)
    x0 = qc.boxplus(X[:, 0], rng.normal(size=(B, 12)) * qc.SIGMA)
    if c["attitude"] == "vertical":
        x0[:, 3:7] = -x0[:, 3:7]
        Y[:, ::3, 3:7] *= -2.0
    d = np.sqrt(4.0 * qc.SIGMA ** 2)
    if c["spread"] == "wide":
        d[3:6] = WIDE_SIGMA
    M = rng.normal(size=(B, 12, 12))
    C = 0.7 * np.eye(12) + 0.3 * (M @ M.transpose(0, 2, 1)) / 12.0
    P0 = d[None, :, None] * C * d[None, None, :]
    P0 = 0.5 * (P0 + P0.transpose(0, 2, 1))
    P0[:, np.triu_indices(12, 1)[0], np.triu_indices(12, 1)[1]] = np.nan
    return dict(cfgs=su.ukf_cfgs(c), x0=x0, P0=P0, U=U, Y=Y, X=X)


# ------------------------------------------------------------------------------------------ the references
def _ref_args(case, ins, cand, rec, rows):
    cand, rec, rows = (slice(None) if v is None else v for v in (cand, rec, rows))
    cfgs = ins["cfgs"] if isinstance(ins["cfgs"], ur.Cfg) else ins["cfgs"][cand]
    return (su.INTEG[case["integ"]], [fv.vehicle(n) for n in case["names"]][cand], cfgs, ins["x0"][rec], ins["P0"][rec], ins["U"][rec, rows],
            ins["Y"][rec, rows], DT)


def ref_filter(case, ins, dtype=np.float64, cand=None, rec=None, rows=None, variant=None):
    """ukf_quat_ref.filter on the arrays of ins, or on a slice of its candidates, recordings and rows"""
    return uq.filter(*_ref_args(case, ins, cand, rec, rows), dtype=dtype, variant=variant)


def ref_smooth(case, ins, dtype=np.float64, cand=None, rec=None, rows=None, terminal=None, variant=None):
    """ukf_quat_smooth_ref.smooth likewise"""
    return qs.smooth(*_ref_args(case, ins, cand, rec, rows), dtype=dtype, terminal=terminal, variant=variant)


def terminal_pair(case, o):
    """(xs_T [P,B,13], Ps_T [P,B,12,12]) for the backward pass over the outputs o of the float64 reference (or of the filter: xT, PT):
    xT [+] a normal draw of ukf_cases.SIGMA; Ps_T = Lc diag(s) Lc^T with PT = Lc Lc^T and s uniform in 0.3 .. 0.8, so that
    0.3 PT <= Ps_T <= 0.8 PT in the order of the positive-definite matrices; the upper triangle NaN.  Seeded by the case."""
    rng = np.random.default_rng([case["seed"], 1])
    xT, PT = np.asarray(o["xT"], dtype=np.float64), np.asarray(o["PT"], dtype=np.float64)
    xs_T = qc.boxplus(xT, rng.normal(size=xT.shape[:-1] + (12,)) * qc.SIGMA)
    Lc = np.linalg.cholesky(np.tril(PT) + np.tril(PT, -1).swapaxes(-1, -2))
    s = rng.uniform(TERMINAL_LO, TERMINAL_HI, PT.shape[:-1])
    Ps_T = (Lc * s[..., None, :]) @ Lc.swapaxes(-1, -2)
    Ps_T = 0.5 * (Ps_T + Ps_T.swapaxes(-1, -2))
    iu = np.triu_indices(12, 1)
    Ps_T[..., iu[0], iu[1]] = np.nan
    return xs_T, Ps_T


def with_terminal(o, terminal, dtype, variant=None):
    """the outputs o of ref_smooth with the backward pass of every problem run again from the terminal pair"""
    P, B = o["nrows"].shape
    out = dict(o)
    lanes = [[qs.rts_one(o["xf"][j, b], o["tape"][j, b], o["nrows"][j, b], dtype, (terminal[0][j, b], terminal[1][j, b]), variant) for b in range(B)]
             for j in range(P)]
    for k in lanes[0][0]:
        out[k] = np.stack([np.stack([np.asarray(lanes[j][b][k]) for b in range(B)]) for j in range(P)])
    return out


def _lane(o, keys, j, b):
    return {k: np.asarray(o[k])[j:j + 1, b:b + 1] for k in keys}


def sign_free(a, b):
    """the largest min(|a - b|, |a + b|) over quaternions [..., 4] (NaN rows of b skipped); inf where the NaN patterns differ"""
    a, b = np.asarray(a, dtype=L), np.asarray(b, dtype=L)
    if a.shape != b.shape or np.any(np.isnan(a) != np.isnan(b)):
        return np.inf
    ok = ~np.isnan(b).any(axis=-1)
    if not ok.any():
        return 0.0
    return float(np.max(np.minimum(np.abs(a[ok] - b[ok]).max(axis=-1), np.abs(a[ok] + b[ok]).max(axis=-1))))


def filter_gaps(a, o):
    """{measure: error of a against o} for the filter's outputs"""
    la, lo = dict(a), dict(o)
    la["info"], lo["info"] = np.asarray(a["info"])[..., [0, 3]], np.asarray(o["info"])[..., [0, 3]]       # the counts are compared exactly, elsewhere
    g = qc.gaps(la, lo)
    g["xf q"], g["xT q"] = sign_free(np.asarray(a["xf"])[..., 3:7], np.asarray(o["xf"])[..., 3:7]), sign_free(np.asarray(a["xT"])[..., 3:7], np.asarray(o["xT"])[..., 3:7])
    return g


def filter_lane_gaps(a, o):
    """[P,B] of the largest of filter_gaps per problem"""
    P, B = np.asarray(o["info"]).shape[:2]
    return np.array([[max(filter_gaps(_lane(a, F_OUTS, j, b), _lane(o, F_OUTS, j, b)).values()) for b in range(B)] for j in range(P)])


def smooth_lane_gaps(a, o):
    """[P,B] of the largest of ukf_quat_smooth_ref.gaps per problem"""
    P, B = np.asarray(o["nrows"]).shape
    return np.array([[max(qs.gaps(_lane(a, GAP_KEYS, j, b), _lane(o, GAP_KEYS, j, b)).values()) for b in range(B)] for j in range(P)])


def prepare_ukf_quat(case):
    c = case
    ref = quat_inputs(c)
    ref["o"], ref["ol"] = ref_filter(c, ref), ref_filter(c, ref, L)
    o, ol = ref["o"], ref["ol"]
    ok = (np.minimum(o["ew_min"], ol["ew_min"]) > EW) & (np.minimum(o["pivot_min"], ol["pivot_min"]) > PIVOT)
    ok &= (o["info"][..., 2] == -1) & (ol["info"][..., 2] == -1) & (o["info"][..., 1] == ol["info"][..., 1].astype(np.float64))
    return su._finish(ref, filter_lane_gaps(o, ol), ok)


def prediction_only(case, r, what):
    """a recording without measurements: the backward pass from the filter's last row changes no bit of the filter's covariance and
    moves the estimate by the rounding of conj(q) (x) q alone (the module text)"""
    Pf = qs.tape_fields(r["tape"])["Pf"]
    assert np.array_equal(r["pstd_s"], r["pstd"]) and np.array_equal(r["Ps"], Pf), (what, "pstd_s = pstd, Ps = Pf", case)
    assert np.array_equal(r["xs"][:, :, -1], r["xf"][:, :, -1]), (what, "row T - 1 is the filter's", case)
    e = uc.err(r["xs"], r["xf"])
    assert e < NONE_XS, (what, "xs = xf to the rounding of the chart", e, case)


def prepare_smooth_quat(case):
    c, T = case, case["T"]
    ref = quat_inputs(c)
    ref["o_plain"], ref["ol_plain"] = ref_smooth(c, ref), ref_smooth(c, ref, L)
    ref["terminal"] = terminal_pair(c, ref["o_plain"]) if c["terminal"] else None
    if c["terminal"]:
        ref["o"], ref["ol"] = with_terminal(ref["o_plain"], ref["terminal"], np.float64), with_terminal(ref["ol_plain"], ref["terminal"], L)
    else:
        ref["o"], ref["ol"] = ref["o_plain"], ref["ol_plain"]
    gaps = np.maximum(smooth_lane_gaps(ref["o"], ref["ol"]), filter_lane_gaps(ref["o"], ref["ol"]))
    ok = np.ones((c["P"], c["B"]), dtype=bool)
    for key in ("o", "ol", "o_plain", "ol_plain"):
        r = ref[key]
        ok &= (r["f_ew_min"] > EW) & (r["ew_min"] > EW) & (r["f_pivot_min"] > PIVOT) & (r["pivot_min"] > PIVOT)
        ok &= (r["info"][..., 2] == -1) & (r["nrows"] == T) & (r["sinfo"][..., 0] == -1)
    ok &= ref["o"]["info"][..., 1] == ref["ol"]["info"][..., 1].astype(np.float64)
    if c["terminal"]:
        gaps = np.maximum(gaps, smooth_lane_gaps(ref["o_plain"], ref["ol_plain"]))
    if c["measured"] == "none":
        prediction_only(c, ref["o_plain"], "the float64 reference")
        prediction_only(c, ref["ol_plain"], "the long-double reference")
    return su._finish(ref, gaps, ok)


# ------------------------------------------------------------------------------------------ the engine calls
def call(fn, ctx, case, ins, cand=None, rec=None, rows=None, extra=None, **kw):
    """fn = engine.ukf_filter_quat or engine.ukf_smooth_quat on the arrays of ins; cand / rec / rows: slices of the candidates, the
    recordings, the time rows; kw overrides cfgs, x0, P0, U, Y; extra: further keyword arguments of fn"""
    c = case
    cand, rec, rows = (slice(None) if v is None else v for v in (cand, rec, rows))
    cfgs = kw.pop("cfgs", ins["cfgs"])
    cfgs = cfgs if isinstance(cfgs, ur.Cfg) else cfgs[cand]
    a = dict(x0=ins["x0"][rec], P0=ins["P0"][rec], U=ins["U"][rec, rows], Y=ins["Y"][rec, rows])
    a.update(kw)
    return fn(c["integ"], [fv.params(n) for n in c["names"]][cand], su._structs(cfgs), a["x0"], a["P0"], a["U"], a["Y"], DT, ctx=ctx, **(extra or {}))


def two_step(eng, ctx, case, ins, terminal=None, want=S_OUTS, **kw):
    """the tape filter, then the backward pass over its tape: one dict with both calls' outputs"""
    f = call(eng.ukf_filter_quat, ctx, case, ins, extra=dict(tape=True), **kw)
    f.update(eng.ukf_rts_quat(f["xf"], f["tape"], f["nrows"], terminal=terminal, want=want, ctx=ctx))
    return f


def smooth(eng, ctx, case, ins, want=F_OUTS + S_OUTS, tape_bytes=0, **kw):
    return call(eng.ukf_smooth_quat, ctx, case, ins, extra=dict(want=want, tape_bytes=tape_bytes), **kw)


def same(a, b, keys, what, ia=(), ib=()):
    """a[k][ia] and b[k][ib] hold the same bits (NaN where NaN) for every key; None goes with None"""
    for k in keys:
        if a[k] is None or b[k] is None:
            assert a[k] is None and b[k] is None, (k, what)
        else:
            assert np.array_equal(a[k][ia], b[k][ib], equal_nan=True), (k, what)


def _filter_checked(case, what, got, o, keep):
    """the worst error of a run's filter outputs against the reference o over the compared lanes, and the exact properties"""
    c, T = case, case["T"]
    for k in F_OUTS:
        assert got[k].shape == np.asarray(o[k]).shape, (what, k, got[k].shape, case)
    worst = su._worst(case, what, filter_lane_gaps(got, o), keep)
    assert np.array_equal(got["info"][..., 1:3][keep], o["info"][..., 1:3][keep]), (what, "the number of updates and the failed step are exact", case)
    assert np.array_equal(got["PT"], got["PT"].swapaxes(-1, -2)), (what, "PT must be bit-symmetric", case)
    if c["measured"] == "none":
        assert np.isnan(got["innov"]).all() and not got["info"][..., 0].any() and not got["info"][..., 1].any(), (what, "pure prediction", case)
    if c["measured"] == "all":
        assert np.all(got["info"][..., 1] == T * (12 - c["r_inf"])), (what, "every measured component of every row is an update", case)
    return worst


def sweep_ukf_quat(eng, ctx, case, ref):
    return _filter_checked(case, "ukf_quat", call(eng.ukf_filter_quat, ctx, case, ref), ref["o"], ref["keep"])


def _checked(case, what, got, o, keep, with_tape):
    """the worst error of one run against the reference o over the compared lanes, and the exact properties of a clean run"""
    c, T = case, case["T"]
    have = dict(got)
    if not with_tape:
        have["tape"] = o["tape"]
    worst = max(su._worst(case, what, smooth_lane_gaps(have, o), keep), _filter_checked(case, what, got, o, keep))
    assert np.all(got["sinfo"][..., 0][keep] == -1), (what, "no failed transition", got["sinfo"][..., 0], case)
    if with_tape:
        assert np.all(got["nrows"][keep] == T), (what, "nrows", got["nrows"], case)
    assert np.array_equal(got["Ps"], got["Ps"].swapaxes(-1, -2)), (what, "Ps must be bit-symmetric", case)
    assert np.array_equal(got["Ps0"], got["Ps"][:, :, 0]), (what, "Ps0 is row 0 of Ps", case)
    return worst


def sweep_smooth_quat(eng, ctx, case, ref):
    """the three runs of a case and every assertion on them; the worst kernel error over the compared lanes"""
    c, keep, T = case, ref["keep"], case["T"]
    term, want = ref["terminal"], tuple(c["want"])
    plain = call(eng.ukf_filter_quat, ctx, c, ref)
    a = two_step(eng, ctx, c, ref, terminal=term)
    b = smooth(eng, ctx, c, ref)
    assert a["tape"].shape == (c["P"], c["B"], T, qs.TAPE) and a["nrows"].shape == (c["P"], c["B"]), case
    worst = max(_checked(c, "two calls", a, ref["o"], keep, True), _checked(c, "one call", b, ref["o_plain"], keep, False))
    same(a, plain, F_OUTS, ("the tape changes no filter output", case))
    if term is None:
        assert np.array_equal(a["xs"][:, :, T - 1], a["xf"][:, :, T - 1]) and np.array_equal(a["pstd_s"][:, :, T - 1], a["pstd"][:, :, T - 1]), \
            ("row T - 1 is the filter's", case)
        same(b, a, F_OUTS + S_OUTS, ("one call against two", case))
    else:
        same(b, a, F_OUTS, ("one call against two: the filter", case))
        moved = np.array([[uc.err(a["xs"][j, i], b["xs"][j, i]) for i in range(c["B"])] for j in range(c["P"])])
        assert np.all(moved > 1e3 * TOL), ("the terminal pair must move the estimate", moved, case)
    # (c) the chunked call, for the case's subset of the outputs
    sub = want != S_OUTS
    keys = want if sub else F_OUTS + S_OUTS
    # on the recordings in reversed order: an output row that a chunk never wrote is uninitialised memory, which the allocator may
    # hand back with the bits run (b) left there -- in the same order it would pass for written
    rev = slice(None, None, -1)
    ch = smooth(eng, ctx, c, ref, want=keys, tape_bytes=sc.smooth_quat_tape_bytes(c), rec=rev)
    for k in F_OUTS + S_OUTS:
        if k not in keys:
            assert ch[k] is None, (k, "not wanted", case)
    same(ch, b, keys, ("chunked against one chunk", sc.smooth_quat_chunks(c), case), (slice(None), rev))
    if sub:                                                          # the two-call path with the subset
        s = eng.ukf_rts_quat(a["xf"], a["tape"], a["nrows"], terminal=term, want=want, ctx=ctx)
        for k in S_OUTS:
            assert (s[k] is None) == (k not in want), (k, "not wanted", case)
        same(s, a, want, ("a subset of the outputs changes no bit", case))
    if c["measured"] == "none":
        prediction_only(c, dict(b, tape=a["tape"]), "one call")
        if term is None:
            prediction_only(c, a, "two calls")
    return worst


PREPARE = dict(ukf_quat=prepare_ukf_quat, smooth_quat=prepare_smooth_quat)


def sweep_one(eng, ctx, case, ref):
    """(worst kernel error, 0.0) of one case"""
    return (sweep_ukf_quat if case["family"] == "ukf_quat" else sweep_smooth_quat)(eng, ctx, case, ref), 0.0
