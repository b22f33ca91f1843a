"""What the shape sweeps do with a case of the family `smooth` of tests/sweep_cases.py: the unscented Rauch-Tung-Striebel smoother,
i.e. the TAPE = true instantiations of ukf_filter_kernel, ukf_rts_kernel (csrc/ukf.hip) and the chunked brov_ukf_smooth
(csrc/capi.hip: ukf_filter).  prepare / run / compare as in tests/sweep_run.py, which registers them.  Not collected.

Inputs by tests/sweep_ukf_lmpc.py: ukf_inputs (a smooth case holds every field of a ukf case).  The reference is
ukf_smooth_ref.smooth in float64 and in long double, with the case's terminal pair (terminal_pair below: xT of the float64 reference
moved by about one sigma, a positive-definite Ps_T between 0.3 and 0.8 of its PT, the upper triangle NaN) and, because the one-call
smoother takes no pair, without it as well.  A lane is one (candidate, recording) problem.  It is compared if its own
float64-to-long-double gap in the measures of ukf_smooth_cases.gaps (xs, pstd_s as the mixed error, Ps, Ps0 and the tape's Pf, Pp as
|dP_ij| / sqrt(P_ii P_jj), the tape's C as |dC_ab| / sqrt(Pf_aa Pp_bb), xp, sinfo[1]) and in those of the filter
(sweep_ukf_lmpc.ukf_lane_gaps) is below a tenth of TOL = 1e-10, both precisions give a wrap margin above 1e-6 and forward and
backward pivots above 1e-4, and both complete all T rows and every transition.  tests/test_sweep_cases_cpu.py asserts that no lane of
any case is left out.

Every case runs three ways: (a) engine.ukf_filter(tape=True), then engine.ukf_rts with the terminal pair; (b) engine.ukf_smooth in
one chunk; (c) engine.ukf_smooth with the case's tape_bytes and, where the case asks for a strict subset of the smoother's outputs,
for that subset alone (xf is then scratch inside the library).  Compared: (a) against the float64 reference at 1e-10 in the measures
above, filter outputs included, (b) against the reference without the pair; nrows = T and sinfo[0] = -1 exactly; Ps bit-symmetric,
Ps0 = Ps[:, :, 0], row T - 1 the filter's without a pair; the filter outputs of (a), lag_io included, the bits of the plain filter;
(b) and (c) the same bits, and those of (a) without a pair; what was not wanted None and what was wanted unchanged; on a recording
without measurements xs = xf, pstd_s = pstd and Ps = Pf bit for bit (a prediction is never corrected: xs_{t+1} - xp_{t+1} and
Ps_{t+1} - Pp_{t+1} are exactly 0), which prepare asserts of the reference too."""
import numpy as np

import fossen_vehicles as fv
import sweep_cases as sc
import sweep_ukf_lmpc as su
import ukf_cases as uc
import ukf_ref as ur
import ukf_smooth_cases as us
import ukf_smooth_ref as usr

L = np.longdouble
TOL, MARGIN, PIVOT = us.TOL, us.MARGIN, us.PIVOT
F_OUTS = su.UKF_OUTS
S_OUTS = sc.SMOOTH_OUTS
ROWS = ("xs", "pstd_s", "Ps")
TAPE_KEYS = ("tape", "nrows")
GAP_KEYS = S_OUTS + ("tape",)
TERMINAL_LO, TERMINAL_HI = 0.3, 0.8


# ------------------------------------------------------------------------------------------ the reference
def ref_smooth(case, ins, dtype=np.float64, cand=None, rec=None, rows=None, terminal=None):
    """ukf_smooth_ref.smooth on the arrays of ins (tests/sweep_ukf_lmpc.py: ukf_inputs), or on a slice of its candidates, recordings
    and rows"""
    c = case
    cand, rec, rows = (slice(None) if v is None else v for v in (cand, rec, rows))
    cfgs = ins["cfgs"] if isinstance(ins["cfgs"], ur.Cfg) else ins["cfgs"][cand]
    return usr.smooth(c["model"], su.INTEG[c["integ"]], c["lag_mode"], [fv.vehicle(n) for n in c["names"]][cand], cfgs, ins["x0"][rec], ins["P0"][rec],
                      ins["U"][rec, rows], ins["Y"][rec, rows], su.DT_UKF, lag=None if ins["lag"] is None else ins["lag"][cand, rec], dtype=dtype,
                      terminal=terminal)


def terminal_pair(case, o):
    """(xs_T [P,B,12], Ps_T [P,B,12,12]) for the backward pass over the outputs o of the float64 reference (or of the filter: xT, PT):
    xT moved by a normal draw of ukf_cases.SIGMA; Ps_T = Lc diag(s) Lc^T with PT = Lc Lc^T and s uniform in 0.3 .. 0.8, so that
    0.3 PT <= Ps_T <= 0.8 PT in the order of the positive-definite matrices; the upper triangle NaN.  Seeded by the case."""
    rng = np.random.default_rng([case["seed"], 1])
    xT, PT = np.asarray(o["xT"], dtype=np.float64), np.asarray(o["PT"], dtype=np.float64)
    xs_T = xT + rng.normal(size=xT.shape) * uc.SIGMA
    Lc = np.linalg.cholesky(np.tril(PT) + np.tril(PT, -1).swapaxes(-1, -2))
    s = rng.uniform(TERMINAL_LO, TERMINAL_HI, xT.shape)
    Ps_T = (Lc * s[..., None, :]) @ Lc.swapaxes(-1, -2)
    Ps_T = 0.5 * (Ps_T + Ps_T.swapaxes(-1, -2))
    iu = np.triu_indices(12, 1)
    Ps_T[..., iu[0], iu[1]] = np.nan
    return xs_T, Ps_T


def with_terminal(o, terminal, dtype):
    """the outputs o of ref_smooth with the backward pass of every problem run again from the terminal pair"""
    P, B = o["nrows"].shape
    out = dict(o)
    lanes = [[usr.rts_one(o["xf"][j, b], o["tape"][j, b], o["nrows"][j, b], dtype, (terminal[0][j, b], terminal[1][j, b])) for b in range(B)]
             for j in range(P)]
    for k in lanes[0][0]:
        out[k] = np.stack([np.stack([np.asarray(lanes[j][b][k]) for b in range(B)]) for j in range(P)])
    return out


def lane_gaps(a, o):
    """[P,B] of the largest of ukf_smooth_cases.gaps per problem"""
    P, B = np.asarray(o["nrows"]).shape
    g = np.zeros((P, B))
    for j in range(P):
        for b in range(B):
            g[j, b] = max(us.gaps({k: np.asarray(a[k])[j:j + 1, b:b + 1] for k in GAP_KEYS}, {k: np.asarray(o[k])[j:j + 1, b:b + 1] for k in GAP_KEYS}).values())
    return g


def prediction_only(case, r, what):
    """a recording without measurements: the backward pass from the filter's last row changes no bit of the filter's estimate"""
    Pf = us.tape_fields(r["tape"])["Pf"]
    assert np.array_equal(r["xs"], r["xf"]) and np.array_equal(r["pstd_s"], r["pstd"]) and np.array_equal(r["Ps"], Pf), (what, "xs = xf, Ps = Pf", case)


def prepare_smooth(case):
    c = case
    ref = su.ukf_inputs(c)
    T = c["T"]
    ref["o_plain"], ref["ol_plain"] = ref_smooth(c, ref), ref_smooth(c, ref, L)
    ref["terminal"] = terminal_pair(c, ref["o_plain"]) if c["terminal"] else None
    if c["terminal"]:
        ref["o"], ref["ol"] = with_terminal(ref["o_plain"], ref["terminal"], np.float64), with_terminal(ref["ol_plain"], ref["terminal"], L)
    else:
        ref["o"], ref["ol"] = ref["o_plain"], ref["ol_plain"]
    gaps = np.maximum(lane_gaps(ref["o"], ref["ol"]), su.ukf_lane_gaps(ref["o"], ref["ol"], c["model"] == 0))
    ok = np.ones((c["P"], c["B"]), dtype=bool)
    for key in ("o", "ol", "o_plain", "ol_plain"):
        r = ref[key]
        ok &= (r["wrap_margin"] > MARGIN) & (r["pivot_min"] > PIVOT) & (r["rts_pivot_min"] > PIVOT)
        ok &= (r["info"][..., 2] == -1) & (r["nrows"] == T) & (r["sinfo"][..., 0] == -1)
    ok &= ref["o"]["info"][..., 1] == ref["ol"]["info"][..., 1].astype(np.float64)
    if c["terminal"]:
        gaps = np.maximum(gaps, lane_gaps(ref["o_plain"], ref["ol_plain"]))
    if c["measured"] == "none":
        prediction_only(c, ref["o_plain"], "the float64 reference")
        prediction_only(c, ref["ol_plain"], "the long-double reference")
    return su._finish(ref, gaps, ok)


# ------------------------------------------------------------------------------------------ the engine calls
def call(fn, ctx, case, ins, cand=None, rec=None, rows=None, extra=None, **kw):
    """fn = engine.ukf_filter or engine.ukf_smooth on the arrays of ins; cand / rec / rows: slices of the candidates, the recordings,
    the time rows; kw overrides cfgs, x0, P0, U, Y, lag; extra: further keyword arguments of fn"""
    c = case
    cand, rec, rows = (slice(None) if v is None else v for v in (cand, rec, rows))
    cfgs = kw.pop("cfgs", ins["cfgs"])
    cfgs = cfgs if isinstance(cfgs, ur.Cfg) else cfgs[cand]
    a = dict(x0=ins["x0"][rec], P0=ins["P0"][rec], U=ins["U"][rec, rows], Y=ins["Y"][rec, rows], lag=None if ins["lag"] is None else ins["lag"][cand, rec])
    a.update(kw)
    return fn(c["model"], c["integ"], [fv.params(n) for n in c["names"]][cand], su._structs(cfgs), a["x0"], a["P0"], a["U"], a["Y"], su.DT_UKF,
              lag=a["lag"], lag_mode=c["lag_mode"], ctx=ctx, **(extra or {}))


def two_step(eng, ctx, case, ins, terminal=None, want=S_OUTS, **kw):
    """the tape filter, then the backward pass over its tape: one dict with both calls' outputs"""
    f = call(eng.ukf_filter, ctx, case, ins, extra=dict(tape=True), **kw)
    f.update(eng.ukf_rts(f["xf"], f["tape"], f["nrows"], terminal=terminal, want=want, ctx=ctx))
    return f


def smooth(eng, ctx, case, ins, want=F_OUTS + S_OUTS, tape_bytes=0, **kw):
    return call(eng.ukf_smooth, ctx, case, ins, extra=dict(want=want, tape_bytes=tape_bytes), **kw)


def same(a, b, keys, what, ia=(), ib=()):
    """a[k][ia] and b[k][ib] hold the same bits (NaN where NaN) for every key; None goes with None"""
    for k in keys:
        if a[k] is None or b[k] is None:
            assert a[k] is None and b[k] is None, (k, what)
        else:
            assert np.array_equal(a[k][ia], b[k][ib], equal_nan=True), (k, what)


def _checked(case, what, got, o, keep, with_tape):
    """the worst error of one run against the reference o over the compared lanes, and the exact properties of a clean run"""
    c, T = case, case["T"]
    have = dict(got)
    if not with_tape:
        have["tape"] = o["tape"]
    if have["lag"] is None:
        have["lag"] = o["lag"]
    e = np.maximum(lane_gaps(have, o), su.ukf_lane_gaps(have, o, c["lag"]))
    worst = su._worst(case, what, e, keep)
    assert np.array_equal(got["info"][..., 1:3][keep], o["info"][..., 1:3][keep]), (what, "updates and failed step are exact", case)
    assert np.all(got["sinfo"][..., 0][keep] == -1), (what, "no failed transition", got["sinfo"][..., 0], case)
    if with_tape:
        assert np.all(got["nrows"][keep] == T), (what, "nrows", got["nrows"], case)
    assert np.array_equal(got["Ps"], got["Ps"].swapaxes(-1, -2)), (what, "Ps must be bit-symmetric", case)
    assert np.array_equal(got["Ps0"], got["Ps"][:, :, 0]), (what, "Ps0 is row 0 of Ps", case)
    return worst


def sweep_smooth(eng, ctx, case, ref):
    """the three runs of a case and every assertion on them; the worst kernel error over the compared lanes"""
    c, keep, T = case, ref["keep"], case["T"]
    term, want = ref["terminal"], tuple(c["want"])
    plain = call(eng.ukf_filter, ctx, c, ref)
    a = two_step(eng, ctx, c, ref, terminal=term)
    b = smooth(eng, ctx, c, ref)
    assert (a["lag"] is None) == (not c["lag"]) and (b["lag"] is None) == (not c["lag"]), ("lag_io is None exactly without a start lag", case)
    assert a["tape"].shape == (c["P"], c["B"], T, usr.TAPE) and a["nrows"].shape == (c["P"], c["B"]), case
    worst = max(_checked(c, "two calls", a, ref["o"], keep, True), _checked(c, "one call", b, ref["o_plain"], keep, False))
    same(a, plain, F_OUTS + ("lag",), ("the tape changes no filter output", case))
    if term is None:
        assert np.array_equal(a["xs"][:, :, T - 1], a["xf"][:, :, T - 1]) and np.array_equal(a["pstd_s"][:, :, T - 1], a["pstd"][:, :, T - 1]), \
            ("row T - 1 is the filter's", case)
        same(b, a, F_OUTS + S_OUTS + ("lag",), ("one call against two", case))
    else:
        same(b, a, F_OUTS + ("lag",), ("one call against two: the filter", case))
        moved = np.array([[uc.err(a["xs"][j, i], b["xs"][j, i]) for i in range(c["B"])] for j in range(c["P"])])
        assert np.all(moved > 1e3 * TOL), ("the terminal pair must move the estimate", moved, case)
    # (c) the chunked call, for the case's subset of the outputs
    sub = want != S_OUTS
    keys = want if sub else F_OUTS + S_OUTS
    ch = smooth(eng, ctx, c, ref, want=keys, tape_bytes=sc.smooth_tape_bytes(c))
    for k in F_OUTS + S_OUTS:
        if k not in keys:
            assert ch[k] is None, (k, "not wanted", case)
    same(ch, b, keys + ("lag",), ("chunked against one chunk", sc.smooth_chunks(c), case))
    if sub:                                                          # the two-call path with the subset
        s = eng.ukf_rts(a["xf"], a["tape"], a["nrows"], terminal=term, want=want, ctx=ctx)
        for k in S_OUTS:
            assert (s[k] is None) == (k not in want), (k, "not wanted", case)
        same(s, a, want, ("a subset of the outputs changes no bit", case))
    if c["measured"] == "none":
        prediction_only(c, dict(b, tape=a["tape"]), "one call")
        if term is None:
            prediction_only(c, a, "two calls")
    return worst


PREPARE = dict(smooth=prepare_smooth)


def sweep_one(eng, ctx, case, ref):
    """(worst kernel error, 0.0) of one case"""
    return sweep_smooth(eng, ctx, case, ref), 0.0
