"""The smoother of the quaternion model (brov_ukf_filter_tape_quat_dev, brov_ukf_rts_quat_dev, brov_ukf_smooth_quat /
engine.ukf_filter_quat(tape=True), engine.ukf_rts_quat, engine.ukf_smooth_quat / rov.smooth_states_quat) on the GPU against
tests/ukf_quat_smooth_ref.py, the NumPy restatement of the law of include/brov2.h.

Recipe and bound of tests/test_ukf_smooth_gpu.py and tests/test_ukf_quat_gpu.py: 1e-10 on the mixed error (covariances as |dP_ij| /
sqrt(P_ii P_jj), the cross covariance C of the tape as |dC_ab| / sqrt(Pf_aa Pp_bb)), every comparison with the reference's own fp64
against long-double gap asserted below a tenth of it, no [-] near half a turn (|e_w| > 0.5), no pivot below 1e-4
(tests/test_ukf_quat_smooth_cpu.py checks all that without a GPU, and that the cases tell the law from six of its neighbours).
Shapes: the five cases of tests/ukf_quat_cases.py -- P = 2 candidates, T = 12 rows, B = 3 recordings (the fourth wave of the block
idle) and B = 5 in the ragged case (a full block and a block with one live wave), Euler and RK4, a noise record per candidate, the
start near vertical with a negated x0 and measured quaternions times -2.  The failures of section 3 are numerical conditions of the
input which the kernels handle and report."""
import ctypes

import numpy as np
import pytest

import fossen_vehicles as fv
import ukf_quat_cases as qc
import ukf_quat_ref as uq
import ukf_quat_smooth_ref as qs
import ukf_ref as ur

pytestmark = pytest.mark.gpu

P, T, DT = 2, qc.T, qc.DT
F_OUTS = ("xf", "pstd", "innov", "xT", "PT", "info")
S_OUTS = ("xs", "pstd_s", "Ps", "Ps0", "sinfo")
ROWS = ("xs", "pstd_s", "Ps")
ARGS = ("x0", "P0", "U", "Y")
TAPE = 313


def report(what, kernel_err, gap, bound):
    print(f"{what}: kernel err {kernel_err:.2e}  reference fp64-vs-long-double gap {gap:.2e}  bound {bound:.0e}")
    assert gap < 0.1 * bound, (what, "inputs too hard for fp64", gap)
    assert kernel_err < bound, (what, kernel_err)


@pytest.fixture(scope="module")
def eng():
    from bluerov2_dynamics_amd import engine
    return engine


@pytest.fixture(scope="module")
def ctx():
    from bluerov2_dynamics_amd import _lib
    c = _lib.Context(0)
    yield c
    c.close()


def _params(names=qc.NAMES):
    return [fv.params(n) for n in names]


def _structs(cfgs):
    return ur.to_struct(cfgs) if isinstance(cfgs, ur.Cfg) else [ur.to_struct(c) for c in cfgs]


def _call(fn, ctx, name, params=None, extra=None, **kw):
    """fn = engine.ukf_filter_quat or engine.ukf_smooth_quat on inputs(name), with x0 / P0 / U / Y / cfg replaced by kw"""
    i = qc.inputs(name)
    a = dict(cfg=_structs(i["cfgs"]), x0=i["x0"], P0=i["P0"], U=i["U"], Y=i["Y"])
    a.update(kw)
    return fn(i["integ"], _params() if params is None else params, a["cfg"], a["x0"], a["P0"], a["U"], a["Y"], DT, ctx=ctx, **(extra or {}))


def _two_step(eng, ctx, name, terminal=None, **kw):
    """the tape filter, then the backward pass over its tape: one dict with both calls' outputs"""
    f = _call(eng.ukf_filter_quat, ctx, name, extra=dict(tape=True), **kw)
    f.update(eng.ukf_rts_quat(f["xf"], f["tape"], f["nrows"], terminal=terminal, ctx=ctx))
    return f


def _same(a, b, keys, where=()):
    for k in keys:
        if a[k] is None or b[k] is None:
            assert a[k] is None and b[k] is None, k
        else:
            assert np.array_equal(a[k], b[k], equal_nan=True), (k,) + tuple(where)


def _negq(x):
    x = np.array(x)
    x[..., 3:7] = -x[..., 3:7]
    return x


# ------------------------------------------------------------------------------------------ 1. parity
@pytest.mark.parametrize("name", qs.NAMES)
def test_parity(eng, ctx, name):
    """xs, pstd_s, Ps, Ps0, the four fields of the tape and the smallest pivot against the reference; the tape filter's outputs are the
    plain filter's bit for bit; Ps bit-symmetric, nrows = T, no failed transition, row T-1 is the filter's; engine.ukf_smooth_quat gives
    the bits of the two calls"""
    got = _two_step(eng, ctx, name)
    _same(got, _call(eng.ukf_filter_quat, ctx, name), F_OUTS)                    # the tape changes no filter output
    o, ol = qs.reference(name), qs.reference(name, ld=True)
    assert min(o["ew_min"].min(), ol["ew_min"].min(), o["f_ew_min"].min(), ol["f_ew_min"].min()) > qs.EW
    assert min(o["pivot_min"].min(), ol["pivot_min"].min(), o["f_pivot_min"].min(), ol["f_pivot_min"].min()) > qs.PIVOT
    B = qc.inputs(name)["B"]
    assert got["tape"].shape == (P, B, T, TAPE) and got["xs"].shape == (P, B, T, 13) and got["pstd_s"].shape == (P, B, T, 12)
    e, g = qs.gaps(got, o), qs.gaps(o, ol)
    for k in e:
        report(f"{name} {k}", e[k], g[k], qs.TOL)
    assert np.array_equal(got["Ps"], got["Ps"].transpose(0, 1, 2, 4, 3)), "Ps must be bit-symmetric"
    assert np.array_equal(got["Ps0"], got["Ps"][:, :, 0])
    assert np.all(got["nrows"] == T) and np.all(got["sinfo"][..., 0] == -1)
    assert np.array_equal(got["xs"][:, :, T - 1], got["xf"][:, :, T - 1]) and np.array_equal(got["pstd_s"][:, :, T - 1], got["pstd"][:, :, T - 1])
    assert qc.err(got["xs"], got["xf"]) > 1e3 * qs.TOL, "smoothing must move the estimate"
    assert qc.err(got["xs"][0], got["xs"][1]) > 1e3 * qs.TOL, "the candidates must differ"
    _same(_call(eng.ukf_smooth_quat, ctx, name), got, F_OUTS + S_OUTS)


# ------------------------------------------------------------------------------------------ 2. exact identities
def test_calls_repeat_and_chunks_change_no_bit(eng, ctx):
    """B = 5: two calls give the same bits; engine.ukf_smooth_quat with the whole tape and with a tape_bytes of exactly one block of four
    recordings (two chunks, of 4 and of 1) equals the tape filter followed by the backward pass; xf is scratch inside the library when
    not wanted"""
    name = "q_rk4_ragged"
    a = _two_step(eng, ctx, name)
    _same(a, _two_step(eng, ctx, name), F_OUTS + S_OUTS + ("tape", "nrows"))
    whole = _call(eng.ukf_smooth_quat, ctx, name)
    chunked = _call(eng.ukf_smooth_quat, ctx, name, extra=dict(tape_bytes=P * 4 * T * TAPE * 8))
    _same(whole, a, F_OUTS + S_OUTS)
    _same(chunked, a, F_OUTS + S_OUTS)
    assert np.all(a["info"][..., 2] == -1) and np.all(a["sinfo"][..., 0] == -1)
    want = _call(eng.ukf_smooth_quat, ctx, name, extra=dict(want=("xs", "sinfo"), tape_bytes=P * 4 * T * TAPE * 8))
    assert want["xf"] is None and want["Ps"] is None and np.array_equal(want["xs"], a["xs"]) and np.array_equal(want["sinfo"], a["sinfo"])


def test_each_problem_alone_equals_its_slot(eng, ctx):
    """B = 5: candidate j alone and recording b alone carry the bits they have in the batch (every wave slot and the ragged block)"""
    name = "q_rk4_ragged"
    i, a = qc.inputs(name), _call(eng.ukf_smooth_quat, ctx, name)
    for j in range(P):
        s = _call(eng.ukf_smooth_quat, ctx, name, params=_params()[j:j + 1])
        for k in F_OUTS + S_OUTS:
            assert np.array_equal(s[k][0], a[k][j], equal_nan=True), (k, j)
    for b in range(i["B"]):
        s = _call(eng.ukf_smooth_quat, ctx, name, **{k: i[k][b:b + 1] for k in ARGS})
        for k in F_OUTS + S_OUTS:
            assert np.array_equal(s[k][:, 0], a[k][:, b], equal_nan=True), (k, b)


@pytest.mark.parametrize("name", ["q_rk4", "q_euler"])
def test_split_in_time(eng, ctx, name):
    """filter rows 0..s-1 with a tape, filter and smooth rows s..11 from (xT, PT), then the backward pass over the first span with the
    second's (xs[0], Ps0) as its terminal pair: the bits of the unbroken call in xs, pstd_s, Ps and Ps0; s = 1, 4 and 5 (around the
    empty row) and 11.  Negating or doubling the terminal quaternion changes no bit."""
    i, whole = qc.inputs(name), _call(eng.ukf_smooth_quat, ctx, name)
    for s in (1, 4, 5, 11):
        for j in range(P):                                      # x0 and P0 are shared by the candidates: resume one by one
            pj = _params()[j:j + 1]
            first = _call(eng.ukf_filter_quat, ctx, name, params=pj, extra=dict(tape=True), U=i["U"][:, :s], Y=i["Y"][:, :s])
            second = _call(eng.ukf_smooth_quat, ctx, name, params=pj, x0=first["xT"][0], P0=first["PT"][0], U=i["U"][:, s:], Y=i["Y"][:, s:])
            term = (second["xs"][:, :, 0], second["Ps0"])
            back = eng.ukf_rts_quat(first["xf"], first["tape"], first["nrows"], terminal=term, ctx=ctx)
            for k in ROWS:
                assert np.array_equal(np.concatenate([back[k], second[k]], axis=2), whole[k][j:j + 1]), (name, s, k, j)
            assert np.array_equal(back["Ps0"], whole["Ps0"][j:j + 1])
            if s == 5:
                for scale in (-1.0, 2.0):
                    t2 = term[0].copy()
                    t2[..., 3:7] *= scale
                    _same(eng.ukf_rts_quat(first["xf"], first["tape"], first["nrows"], terminal=(t2, term[1]), ctx=ctx), back, S_OUTS, where=(scale,))
                alone = eng.ukf_rts_quat(first["xf"], first["tape"], first["nrows"], ctx=ctx)   # without the pair the span ends at the filter
                assert np.array_equal(alone["xs"][:, :, s - 1], first["xf"][:, :, s - 1]) and qc.err(alone["xs"], back["xs"]) > 1e3 * qs.TOL


@pytest.mark.parametrize("name", ["q_rk4_vertical", "q_euler"])
def test_sign_of_x0(eng, ctx, name):
    """negating x0's quaternion negates the quaternion of every xf, xT and xs bit for bit and changes no other output"""
    i, a = qc.inputs(name), _call(eng.ukf_smooth_quat, ctx, name)
    n = _call(eng.ukf_smooth_quat, ctx, name, x0=_negq(i["x0"]))
    for k in F_OUTS + S_OUTS:
        assert np.array_equal(n[k], _negq(a[k]) if k in ("xf", "xT", "xs") else a[k], equal_nan=True), k


def test_host_form_equals_dev_form(eng, ctx):
    from bluerov2_dynamics_amd import _lib
    name = "q_rk4"
    i = qc.inputs(name)
    a = _call(eng.ukf_smooth_quat, ctx, name)                   # host arrays through the engine: uploads, then the _dev form
    n = i["B"]
    x0, P0, U, Y = (np.ascontiguousarray(i[k]) for k in ARGS)
    pa = (_lib.BrovParams * P)(*_params())
    ca = (_lib.BrovUkf * 1)(ur.to_struct(i["cfgs"]))
    shapes = eng._ukf_quat_shapes(P, n, T)
    outs = {k: np.empty(shapes[k]) for k in F_OUTS + S_OUTS}
    rc = ctx.lib.brov_ukf_smooth_quat(ctx.h, _lib.RK4, P, pa, 1, ca, n, T, DT, x0.ctypes.data, P0.ctypes.data, U.ctypes.data, Y.ctypes.data,
                                      *(outs[k].ctypes.data for k in F_OUTS + S_OUTS), 0)
    assert rc == 0, ctx.lib.brov_last_error(ctx.h)
    _same(a, outs, F_OUTS + S_OUTS)
    d = eng.ukf_smooth_quat("rk4", _params(), ur.to_struct(i["cfgs"]), *(eng.DevArray.from_host(ctx, i[k]) for k in ARGS), DT, ctx=ctx)
    assert isinstance(d["xs"], eng.DevArray)
    _same(a, {k: (None if v is None else v.numpy()) for k, v in d.items()}, F_OUTS + S_OUTS)


# ------------------------------------------------------------------------------------------ 3. failure paths
@pytest.mark.parametrize("b,s", [(0, 6), (3, 1), (4, 9), (2, 0)])
def test_zero_measured_quaternion_stops_one_filter(eng, ctx, b, s):
    """a measured quaternion of (0, 0, 0, 0) in row s of recording b (B = 5: wave slots of the full block and the lone wave of the
    ragged one): stage 1 of row s fails before any update, nrows = s, rows >= s and their tape records are NaN, record s-1 is
    complete, rows < s are smoothed and equal the call cut to T = s, the other recordings keep the bits of the clean call;
    engine.ukf_smooth_quat gives the bits of the two calls"""
    name = "q_rk4_ragged"
    i, clean = qc.inputs(name), _two_step(eng, ctx, name)
    Y = i["Y"].copy()
    Y[b, s, 3:7] = 0.0
    got = _two_step(eng, ctx, name, Y=Y)
    want_n = np.full((P, i["B"]), float(T))
    want_n[:, b] = s
    assert np.array_equal(got["nrows"], want_n), got["nrows"]
    assert np.all(got["info"][:, b, 2] == s)
    for k in ROWS:
        assert np.isnan(got[k][:, b, s:]).all(), k
    assert np.isnan(got["tape"][:, b, s:]).all() and np.isfinite(got["tape"][:, b, :s]).all()
    if s:
        short = _call(eng.ukf_smooth_quat, ctx, name, U=i["U"][:, :s], Y=Y[:, :s])
        for k in ROWS:
            assert np.isfinite(got[k][:, b, :s]).all() and np.array_equal(got[k][:, b, :s], short[k][:, b]), k
        assert np.array_equal(got["Ps0"][:, b], short["Ps0"][:, b]) and np.array_equal(got["sinfo"][:, b], short["sinfo"][:, b])
        assert np.all(got["sinfo"][:, b, 0] == -1)
    else:
        assert np.isnan(got["Ps0"][:, b]).all() and np.isnan(got["sinfo"][:, b]).all()
    for other in range(i["B"]):
        if other != b:
            for k in F_OUTS + S_OUTS + ("tape", "nrows"):
                assert np.array_equal(got[k][:, other], clean[k][:, other], equal_nan=True), (k, other, "with a failure in", b)
    _same(_call(eng.ukf_smooth_quat, ctx, name, Y=Y), got, F_OUTS + S_OUTS)


@pytest.mark.parametrize("name,j,b,ts", [("q_rk4_ragged", 1, 2, 6), ("q_rk4_ragged", 0, 4, 10), ("q_euler", 0, 0, 0)])
def test_backward_failure(eng, ctx, name, j, b, ts):
    """a Pp diagonal entry of transition ts of one problem of a clean tape is made negative on the host: sinfo[0] = ts, rows <= ts and
    Ps0 are NaN, rows > ts and every other problem keep their bits"""
    clean = _two_step(eng, ctx, name)
    tape = clean["tape"].copy()
    d = 91 + 3 * 4 // 2 + 3                                     # Pp[3][3]
    tape[j, b, ts, d] = -tape[j, b, ts, d]
    got = eng.ukf_rts_quat(clean["xf"], tape, clean["nrows"], ctx=ctx)
    assert got["sinfo"][j, b, 0] == ts and np.isnan(got["Ps0"][j, b]).all()
    assert 0.0 < got["sinfo"][j, b, 1] <= np.sqrt(tape[j, b, ts, 91]), "the pivots up to the failing one are still reported"
    for k in ROWS:
        assert np.isnan(got[k][j, b, :ts + 1]).all() and np.array_equal(got[k][j, b, ts + 1:], clean[k][j, b, ts + 1:]), k
    keep = np.ones(clean["nrows"].shape, dtype=bool)
    keep[j, b] = False
    for k in S_OUTS:
        assert np.array_equal(got[k][keep], clean[k][keep]), k


def test_half_a_turn_fails_the_transition(eng, ctx):
    """a terminal quaternion exactly half a turn from xp_T (xp_T's quaternion set to (0.5, 0.5, -0.5, 0.5) in the tape, the terminal one
    to that times a pure imaginary unit: every product is +-0.25 and the four terms of e_w cancel exactly): delta leaves the finite
    numbers and transition T-1 fails like a bad pivot -- sinfo[0] = T-1, every row and Ps0 NaN, the pivots of that transition's
    factorisation reported, the other problems untouched.  A zero terminal quaternion does the same."""
    name = "q_rk4"
    f = _call(eng.ukf_filter_quat, ctx, name, extra=dict(tape=True))
    clean = eng.ukf_rts_quat(f["xf"], f["tape"], f["nrows"], terminal=(f["xT"], f["PT"]), ctx=ctx)
    assert np.all(clean["sinfo"][..., 0] == -1) and np.isfinite(clean["xs"]).all()
    q = np.array([0.5, 0.5, -0.5, 0.5])
    tape = f["tape"].copy()
    tape[1, 2, T - 1, 81:85] = q
    ref = eng.ukf_rts_quat(f["xf"], tape, f["nrows"], terminal=(f["xT"], f["PT"]), ctx=ctx)
    assert np.all(ref["sinfo"][..., 0] == -1)
    for xq in (uq.qmul(q, np.array([0.0, 1.0, 0.0, 0.0])), np.zeros(4)):
        xT = f["xT"].copy()
        xT[1, 2, 3:7] = xq
        assert np.sum(xT[1, 2, 3:7] * q) == 0.0
        got = eng.ukf_rts_quat(f["xf"], tape, f["nrows"], terminal=(xT, f["PT"]), ctx=ctx)
        assert got["sinfo"][1, 2, 0] == T - 1 and clean["sinfo"][1, 2, 1] <= got["sinfo"][1, 2, 1] < np.inf
        assert all(np.isnan(got[k][1, 2]).all() for k in ROWS + ("Ps0",))
        keep = np.ones((P, 3), dtype=bool)
        keep[1, 2] = False
        for k in S_OUTS:
            assert np.array_equal(got[k][keep], clean[k][keep]), k


def test_edited_nrows(eng, ctx):
    """nrows is a plain array: 0, NaN, a fraction and +inf follow the clamp of the header (NaN and anything below 1 count as 0, the
    fraction is dropped, +inf counts as T)"""
    name = "q_rk4"
    f = _call(eng.ukf_filter_quat, ctx, name, extra=dict(tape=True))
    clean = eng.ukf_rts_quat(f["xf"], f["tape"], f["nrows"], ctx=ctx)
    nrows = f["nrows"].copy()
    nrows[0, 0], nrows[0, 1], nrows[0, 2], nrows[1, 0], nrows[1, 1] = 0.0, np.nan, 7.9, np.inf, 0.99
    got = eng.ukf_rts_quat(f["xf"], f["tape"], nrows, ctx=ctx)
    for jb in ((0, 0), (0, 1), (1, 1)):
        assert all(np.isnan(got[k][jb]).all() for k in S_OUTS), jb
    seven = eng.ukf_rts_quat(f["xf"][:, :, :7], f["tape"][:, :, :7], np.full((P, 3), 7.0), ctx=ctx)
    for k in ROWS:
        assert np.isnan(got[k][0, 2, 7:]).all() and np.array_equal(got[k][0, 2, :7], seven[k][0, 2]), k
    assert np.array_equal(got["xs"][0, 2, 6], f["xf"][0, 2, 6])
    for jb in ((1, 0), (1, 2)):
        for k in S_OUTS:
            assert np.array_equal(got[k][jb], clean[k][jb]), (k, jb)


# ------------------------------------------------------------------------------------------ 4. the host contract
def test_host_contract(eng, ctx):
    """every rule of the header returns BROV_ERR_ARG with a brov_last_error text naming the function called, and no output buffer is
    written; P = 0 and B = 0 return BROV_OK and touch nothing; brov_ukf_smooth keeps refusing the quaternion model in its own words"""
    from bluerov2_dynamics_amd import _lib
    i = qc.inputs("q_rk4")
    n = i["B"]
    x0, P0, U, Y = (np.ascontiguousarray(i[k]) for k in ARGS)
    pa = (_lib.BrovParams * P)(*_params())
    good = i["cfgs"]

    def edited(**kw):
        d = dict(q=good.q.copy(), r=good.r.copy(), alpha=good.alpha, beta=good.beta, kappa=good.kappa)
        for k, v in kw.items():
            if isinstance(v, tuple):
                d[k][v[0]] = v[1]
            else:
                d[k] = v
        return ur.to_struct(ur.Cfg(**d))
    heavy = _params()
    heavy[1].m = heavy[1].added_mass[0]              # m - added_mass[0] = 0: a singular mass matrix
    block = P * 4 * T * TAPE * 8
    assert block == P * 4 * T * 2504
    cases = [("bad integrator", dict(integ=7), "bad enum"),
             ("negative B", dict(B=-1), "negative size"),
             ("B > 2^31", dict(B=(1 << 31) + 1), "2^31"),
             ("nrec not in {1, P}", dict(cfgs=[edited()] * 3), "nrec"),
             ("alpha = 0", dict(cfgs=[edited(alpha=0.0)]), "alpha"),
             ("alpha NaN", dict(cfgs=[edited(), edited(alpha=np.nan)]), "alpha"),
             ("n + lambda <= 0", dict(cfgs=[edited(kappa=-12.0)]), "lambda"),
             ("negative q", dict(cfgs=[edited(q=(3, -1e-9))]), "q must"),
             ("infinite q", dict(cfgs=[edited(q=(11, np.inf))]), "q must"),
             ("NaN r", dict(cfgs=[edited(r=(5, np.nan))]), "r must"),
             ("T < 1", dict(T=0), "T must"),
             ("P > 65535", dict(P=65536), "65535"),
             ("NULL params", dict(null="params"), "NULL"),
             ("NULL ukf", dict(null="ukf"), "NULL"),
             ("NULL x0", dict(null="x0"), "NULL"),
             ("NULL P0", dict(null="P0"), "NULL"),
             ("NULL U", dict(null="U"), "NULL"),
             ("NULL Y", dict(null="Y"), "NULL"),
             ("dt = 0", dict(dt=0.0), "dt"),
             ("singular mass matrix", dict(params=heavy), "singular mass"),
             ("tape_bytes below one block of recordings", dict(tape_bytes=block - 1), "one block of recordings (P * 4 * T * 2504 bytes)"),
             ("negative tape_bytes", dict(tape_bytes=-1), "tape_bytes")]
    sentinel = 7.25
    shapes = eng._ukf_quat_shapes(P, n, T)
    order = F_OUTS + S_OUTS
    for what, kw, word in cases:
        cfgs = kw.get("cfgs", [edited()])
        ca = (_lib.BrovUkf * len(cfgs))(*cfgs)
        ps = (_lib.BrovParams * P)(*kw["params"]) if "params" in kw else pa
        outs = {k: np.full(shapes[k], sentinel) for k in order}
        ptr = dict(params=ps, ukf=ca, x0=x0.ctypes.data, P0=P0.ctypes.data, U=U.ctypes.data, Y=Y.ctypes.data)
        if "null" in kw:
            ptr[kw["null"]] = None
        rc = ctx.lib.brov_ukf_smooth_quat(ctx.h, kw.get("integ", _lib.RK4), kw.get("P", P), ptr["params"], len(cfgs), ptr["ukf"], kw.get("B", n),
                                          kw.get("T", T), kw.get("dt", DT), ptr["x0"], ptr["P0"], ptr["U"], ptr["Y"],
                                          *(outs[k].ctypes.data for k in order), kw.get("tape_bytes", 0))
        msg = (ctx.lib.brov_last_error(ctx.h) or b"").decode()
        print(what, "->", rc, msg)
        assert rc == -1 and word in msg, (what, msg)
        # (dt and the mass matrix are refused by the derivation of the candidates, whose texts name no function for any caller)
        assert msg.startswith("brov_ukf_smooth_quat: ") or word in ("dt", "singular mass"), ("the text names the function that was called", what, msg)
        assert all(np.all(v == sentinel) for v in outs.values()), what
    # exactly one block of recordings is enough
    ok = _call(eng.ukf_smooth_quat, ctx, "q_rk4", extra=dict(tape_bytes=block, want=("xs",)))
    assert np.isfinite(ok["xs"]).all()
    # B = 0 and P = 0: nothing to do, nothing touched
    r = eng.ukf_smooth_quat("rk4", [], ur.to_struct(good), x0, P0, U, Y, DT, ctx=ctx)
    assert r["xs"].shape == (0, n, T, 13) and r["sinfo"].shape == (0, n, 2)
    r = eng.ukf_smooth_quat("rk4", _params(), ur.to_struct(good), x0[:0], P0[:0], U[:0], Y[:0], DT, ctx=ctx)
    assert r["Ps0"].shape == (P, 0, 12, 12)
    sinfo = np.full((P, n, 2), sentinel)
    ca = (_lib.BrovUkf * 1)(edited())
    for kw in (dict(P=0), dict(B=0)):
        rc = ctx.lib.brov_ukf_smooth_quat(ctx.h, _lib.RK4, kw.get("P", P), pa, 1, ca, kw.get("B", n), T, DT, x0.ctypes.data, P0.ctypes.data,
                                          U.ctypes.data, Y.ctypes.data, *([None] * 10), sinfo.ctypes.data, 0)
        assert rc == 0 and np.all(sinfo == sentinel), kw
    # the Euler smoother still refuses model 2, in the words its own tests look for
    rc = ctx.lib.brov_ukf_smooth(ctx.h, _lib.WRENCH_QUAT, _lib.RK4, 0, P, pa, 1, ca, n, T, DT, x0.ctypes.data, P0.ctypes.data, U.ctypes.data,
                                 Y.ctypes.data, *([None] * 11), sinfo.ctypes.data, 0)
    assert rc == -1 and "Euler models" in (ctx.lib.brov_last_error(ctx.h) or b"").decode() and np.all(sinfo == sentinel)
    # the tape filter and the backward pass on device buffers
    f = _call(eng.ukf_filter_quat, ctx, "q_rk4", extra=dict(tape=True))
    D = eng.DevArray.from_host
    xf, tape, nrows, xsT, PsT = D(ctx, f["xf"]), D(ctx, f["tape"]), D(ctx, f["nrows"]), D(ctx, f["xT"]), D(ctx, f["PT"])
    xs = D(ctx, np.full((P, n, T, 13), sentinel))
    p = eng._dptr

    def rts(what, word, P_=P, B_=n, T_=T, xf_=xf, tape_=tape, nrows_=nrows, xsT_=None, PsT_=None, rc_want=-1):
        rc = ctx.lib.brov_ukf_rts_quat_dev(ctx.h, P_, B_, T_, p(xf_), p(tape_), p(nrows_), p(xsT_), p(PsT_), p(xs), None, None, None, None)
        msg = (ctx.lib.brov_last_error(ctx.h) or b"").decode()
        print(what, "->", rc, msg)
        assert rc == rc_want and (rc == 0 or (word in msg and msg.startswith("brov_ukf_rts_quat_dev: "))), (what, msg)
        assert np.all(xs.numpy() == sentinel), what
    rts("xs_T without Ps_T", "terminal pair", xsT_=xsT)
    rts("Ps_T without xs_T", "terminal pair", PsT_=PsT)
    rts("NULL xf", "NULL", xf_=None)
    rts("NULL tape", "NULL", tape_=None)
    rts("NULL nrows", "NULL", nrows_=None)
    rts("T < 1", "T must", T_=0)
    rts("P > 65535", "65535", P_=65536)
    rts("negative B", "negative", B_=-1)
    rts("P = 0", "", P_=0, rc_want=0)
    rts("B = 0", "", B_=0, rc_want=0)
    d = [D(ctx, v) for v in (x0, P0, U, Y)]
    for kw, word in ((dict(tape=tape), "go together"), (dict(nrows=nrows), "go together")):
        rc = ctx.lib.brov_ukf_filter_tape_quat_dev(ctx.h, _lib.RK4, P, pa, 1, ca, n, T, DT, *(p(v) for v in d), p(xs), None, None, None, None, None,
                                                   p(kw.get("tape")), p(kw.get("nrows")))
        msg = (ctx.lib.brov_last_error(ctx.h) or b"").decode()
        assert rc == -1 and word in msg and msg.startswith("brov_ukf_filter_tape_quat_dev: "), msg
        assert np.all(xs.numpy() == sentinel)
    # with both NULL it is the plain call
    rc = ctx.lib.brov_ukf_filter_tape_quat_dev(ctx.h, _lib.RK4, P, pa, 1, ca, n, T, DT, *(p(v) for v in d), p(xs), None, None, None, None, None,
                                               None, None)
    assert rc == 0 and np.array_equal(xs.numpy(), f["xf"])


# ------------------------------------------------------------------------------------------ 5. the vehicle class and the example
def test_vehicle_method(eng):
    """rov.smooth_states_quat equals engine.ukf_smooth_quat at P = 1 on the same arguments (x0's quaternion normalised on the host), with
    the default start of filter_states, and leaves the object's parameters as they were; it raises on an Euler vehicle, as
    smooth_states does on the quaternion one"""
    from bluerov2_dynamics_amd.fossen.BlueROV2_wrench import BlueROV2
    from bluerov2_dynamics_amd.fossen.BlueROV2_thrust import BlueROV2 as BlueROV2Wrench      # the Euler-angle wrench vehicle
    from bluerov2_dynamics_amd.fossen import estimate, identify
    name = "q_rk4_vertical"
    i = qc.inputs(name)
    cfg = ur.to_struct(i["cfgs"])
    rov = BlueROV2()
    own = identify.params_of(rov)
    before = ctypes.string_at(ctypes.byref(own), ctypes.sizeof(own))
    scaled = i["x0"].copy()
    scaled[:, 3:7] *= 3.0                                       # a given x0 need not be unit
    s = rov.smooth_states_quat(i["Y"], i["U"], DT, cfg, x0=scaled, P0=i["P0"], integrator="rk4", tape_bytes=4 * T * TAPE * 8)
    xn = scaled.copy()
    xn[:, 3:7] /= np.linalg.norm(xn[:, 3:7], axis=1, keepdims=True)
    want = eng.ukf_smooth_quat("rk4", [own], cfg, xn, i["P0"], i["U"], i["Y"], DT, ctx=rov._ctx)
    for mine, theirs in (("x", "xf"), ("std", "pstd"), ("innov", "innov"), ("xT", "xT"), ("PT", "PT"), ("xs", "xs"), ("std_s", "pstd_s"), ("Ps", "Ps"),
                         ("Ps0", "Ps0")):
        assert np.array_equal(s[mine], want[theirs][0], equal_nan=True), mine
    assert s["x"].shape == (i["B"], T, 13) and s["xs"].shape == (i["B"], T, 13) and s["xT"].shape == (i["B"], 13) and s["std_s"].shape == (i["B"], T, 12)
    assert np.all(s["failed_transition"] == -1) and np.all(s["failed_step"] == -1) and np.array_equal(s["loglik"], want["info"][0, :, 0])
    f = rov.filter_states(i["Y"], i["U"], DT, cfg, x0=scaled, P0=i["P0"], integrator="rk4")
    assert np.array_equal(f["x"], s["x"], equal_nan=True) and qc.err(s["xs"], s["x"]) > 1e3 * qs.TOL
    Y = i["Y"].copy()
    Y[:, 1] = np.where(np.isnan(Y[:, 1]), 0.1, Y[:, 1])            # row 1 is the first fully measured one
    dx0, dP0 = estimate.default_start_quat(Y, cfg)
    one = rov.smooth_states_quat(Y[0], i["U"][0], DT, cfg, params=fv.params("V5"), integrator="rk4")
    w1 = eng.ukf_smooth_quat("rk4", [fv.params("V5")], cfg, dx0[:1], dP0[:1], i["U"][:1], Y[:1], DT, ctx=rov._ctx)
    assert one["xs"].shape == (T, 13) and np.array_equal(one["xs"], w1["xs"][0, 0]) and np.array_equal(one["Ps"], w1["Ps"][0, 0])
    own = identify.params_of(rov)
    assert ctypes.string_at(ctypes.byref(own), ctypes.sizeof(own)) == before
    with pytest.raises(NotImplementedError, match="smooth_states_quat"):
        rov.smooth_states(i["Y"], i["U"], DT, cfg, x0=i["x0"], P0=i["P0"])
    with pytest.raises(NotImplementedError, match="smooth_states"):
        BlueROV2Wrench().smooth_states_quat(i["Y"], i["U"], DT, cfg)


def _example():
    import importlib.util
    import os
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "filter_recording.py")
    spec = importlib.util.spec_from_file_location("filter_recording", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_example_smooths_quat():
    """examples/filter_recording.py --quat --smooth: the smoothed RMSE does not exceed the filtered one in position, in attitude and
    over all measured entries together.  The velocity group is dropped: on this recording (150 rows, the second half scored) the NumPy
    reference itself (tests/ukf_quat_smooth_ref.py on the same rows, simulated by the oracle) gives position 0.00487 -> 0.00375,
    attitude 0.00364 -> 0.00308, total 0.00380 -> 0.00342, but velocity 0.00304 -> 0.00340 (filtered -> smoothed), so that group is a property of
    the recording and not of the kernels.
    --quat alone returns what it returned before, and --quat --fit-noise still exits with an error."""
    from bluerov2_dynamics_amd.fossen import estimate
    mod = _example()
    out = mod.main(["--quat", "--smooth"])
    print("RMSE filtered", out["rmse_filtered"], "smoothed", out["rmse_smoothed"])
    assert out["xs"].shape == (150, 13) and out["std_s"].shape == (150, 12) and np.all(np.isfinite(out["xs"]))
    for k in ("position", "attitude"):
        assert out["rmse_smoothed"][k] <= out["rmse_filtered"][k], k
    Y, X = out["Y"], out["X"][:150]
    att = ~np.isnan(Y[:, 3:7]).any(axis=1)
    seen = np.concatenate([~np.isnan(Y[:, :3]), np.repeat(att[:, None], 3, 1), ~np.isnan(Y[:, 7:])], 1)[75:]
    total = lambda x: float(np.sqrt(np.mean(estimate.quat_boxminus(x, X)[75:][seen] ** 2)))
    print("total filtered", total(out["x"]), "smoothed", total(out["xs"]))
    assert total(out["xs"]) <= total(out["x"])
    plain = mod.main(["--quat"])
    assert set(out) - set(plain) == {"xs", "std_s", "rmse_smoothed"}
    for k in plain:
        if isinstance(plain[k], np.ndarray):
            assert np.array_equal(plain[k], out[k], equal_nan=True), k
        else:
            assert plain[k] == out[k], k
    with pytest.raises(SystemExit):
        mod.main(["--quat", "--fit-noise"])
