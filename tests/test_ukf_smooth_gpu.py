"""The unscented Rauch-Tung-Striebel smoother (brov_ukf_filter_tape_dev, brov_ukf_rts_dev, brov_ukf_smooth / engine.ukf_filter(tape=True),
engine.ukf_rts, engine.ukf_smooth / rov.smooth_states) on the GPU against tests/ukf_smooth_ref.py, the NumPy restatement of the law
of include/brov2.h.

Recipe and shapes of tests/test_ukf_gpu.py: the bound 1e-10 on the mixed error (covariances as |dP_ij| / sqrt(P_ii P_jj), the cross
covariance C of the tape as |dC_ab| / sqrt(Pf_aa Pp_bb)), every comparison with the reference's own fp64 against long-double gap
asserted below a tenth of it (tests/test_ukf_smooth_cpu.py checks the gaps, the pivots and the wrap margins without a GPU); P = 2
candidates, T = 12 rows, B = 3 recordings (the fourth wave of the block idle) and B = 5 in the ragged case (a full block and a block
with one live wave).  The failures of sections 3 and 4 are numerical conditions of the input which the kernels handle and report."""
import ctypes

import numpy as np
import pytest

import fossen_vehicles as fv
import ukf_cases as uc
import ukf_ref as ur
import ukf_smooth_cases as us

pytestmark = pytest.mark.gpu

P, T, DT = 2, uc.T, uc.DT
F_OUTS = ("xf", "pstd", "innov", "xT", "PT", "info")
S_OUTS = ("xs", "pstd_s", "Ps", "Ps0", "sinfo")
ROWS = ("xs", "pstd_s", "Ps")
TAPE = 312


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


def _params():
    return [fv.params(n) for n in uc.NAMES]


def _structs(cfgs):
    return ur.to_struct(cfgs) if isinstance(cfgs, ur.Cfg) else [ur.to_struct(c) for c in cfgs]


def _call(fn, ctx, name, params=None, extra=None, **kw):
    """fn = engine.ukf_filter or engine.ukf_smooth on inputs(name), with x0 / P0 / U / Y / lag / cfg replaced by kw"""
    i = uc.inputs(name)
    a = dict(cfg=_structs(i["cfgs"]), x0=i["x0"], P0=i["P0"], U=i["U"], Y=i["Y"], lag=i["lag"])
    a.update(kw)
    return fn(i["model"], i["integ"], _params() if params is None else params, a["cfg"], a["x0"], a["P0"], a["U"], a["Y"], DT, lag=a["lag"],
              lag_mode=i["lag_mode"], ctx=ctx, **(extra or {}))


def _two_step(eng, ctx, name, terminal=None, **kw):
    """the tape filter, then the backward pass over its tape: one dict with both calls' outputs"""
    f = _call(eng.ukf_filter, ctx, name, extra=dict(tape=True), **kw)
    f.update(eng.ukf_rts(f["xf"], f["tape"], f["nrows"], terminal=terminal, ctx=ctx))
    return f


def _same(a, b, keys, where=()):
    for k in keys:
        if a[k] is None or b[k] is None:
            assert a[k] is None and b[k] is None, k
        else:
            assert np.array_equal(a[k], b[k], equal_nan=True), (k,) + tuple(where)


# ------------------------------------------------------------------------------------------ 1. parity
@pytest.mark.parametrize("name", us.NAMES)
def test_parity(eng, ctx, name):
    """xs, pstd_s, Ps, Ps0, the four fields of the tape and the smallest pivot against the reference; Ps bit-symmetric, nrows = T, no
    failed transition; engine.ukf_smooth gives the bits of the two calls"""
    got = _two_step(eng, ctx, name)
    o, ol = us.reference(name), us.reference(name, ld=True)
    assert min(o["wrap_margin"].min(), ol["wrap_margin"].min()) > us.MARGIN
    assert min(o["pivot_min"].min(), ol["pivot_min"].min(), o["rts_pivot_min"].min(), ol["rts_pivot_min"].min()) > us.PIVOT
    assert got["tape"].shape == (P, uc.inputs(name)["B"], T, TAPE)
    e, g = us.gaps(got, o), us.gaps(o, ol)
    for k in e:
        report(f"{name} {k}", e[k], g[k], us.TOL)
    assert np.array_equal(got["Ps"], got["Ps"].transpose(0, 1, 2, 4, 3)), "Ps must be bit-symmetric"
    assert np.array_equal(got["Ps0"], got["Ps"][:, :, 0])
    assert np.all(got["nrows"] == T) and np.all(got["sinfo"][..., 0] == -1)
    assert uc.err(got["xs"], got["xf"]) > 1e3 * us.TOL, "smoothing must move the estimate"
    if name == "thr_euler_wrap":
        assert np.nanmax(got["xs"][..., 5]) > np.pi + 0.02, "the smoothed yaw stays on the filter's continuous branch"
    _same(_call(eng.ukf_smooth, ctx, name), got, F_OUTS + S_OUTS + ("lag",))


# ------------------------------------------------------------------------------------------ 2. exact identities
def test_tape_filter_is_the_filter_and_calls_repeat(eng, ctx):
    for name in ("thr_rk4", "wr_euler"):
        a = _two_step(eng, ctx, name)
        _same(a, _call(eng.ukf_filter, ctx, name), F_OUTS + ("lag",))                # the tape changes no filter output, nor lag_io
        _same(a, _two_step(eng, ctx, name), F_OUTS + S_OUTS + ("lag", "tape", "nrows"))     # two calls give the same bits
        assert np.array_equal(a["xs"][:, :, T - 1], a["xf"][:, :, T - 1]) and np.array_equal(a["pstd_s"][:, :, T - 1], a["pstd"][:, :, T - 1])
        want = _call(eng.ukf_smooth, ctx, name, extra=dict(want=("xs", "sinfo")))   # xf is scratch inside the library when not wanted
        assert want["xf"] is None and want["Ps"] is None and np.array_equal(want["xs"], a["xs"]) and np.array_equal(want["sinfo"], a["sinfo"])


def test_chunked_tape_changes_no_bit(eng, ctx):
    """B = 5 with a tape_bytes of exactly one block of four recordings: two chunks, of 4 and of 1"""
    name = "thr_rk4_ragged"
    whole = _call(eng.ukf_smooth, ctx, name)
    chunked = _call(eng.ukf_smooth, ctx, name, extra=dict(tape_bytes=P * 4 * T * TAPE * 8))
    _same(chunked, whole, F_OUTS + S_OUTS + ("lag",))
    assert np.all(whole["info"][..., 2] == -1) and np.all(whole["sinfo"][..., 0] == -1)


def test_host_form_equals_dev_form(eng, ctx):
    from bluerov2_dynamics_amd import _lib
    name = "thr_rk4"
    i = uc.inputs(name)
    a = _call(eng.ukf_smooth, ctx, name)                        # host arrays through the engine: uploads, then the _dev form
    n = i["B"]
    x0, P0, U, Y = (np.ascontiguousarray(i[k]) for k in ("x0", "P0", "U", "Y"))
    pa = (_lib.BrovParams * P)(*_params())
    ca = (_lib.BrovUkf * 1)(ur.to_struct(i["cfgs"]))
    shapes = eng._ukf_shapes(P, n, T)
    outs = {k: np.empty(shapes[k]) for k in F_OUTS + S_OUTS}
    outs["lag"] = i["lag"].copy()
    rc = ctx.lib.brov_ukf_smooth(ctx.h, 0, _lib.RK4, 0, P, pa, 1, ca, n, T, DT, x0.ctypes.data, P0.ctypes.data, U.ctypes.data, Y.ctypes.data,
                                 *(outs[k].ctypes.data for k in ("lag",) + F_OUTS + S_OUTS), 0)
    assert rc == 0, ctx.lib.brov_last_error(ctx.h)
    _same(a, outs, F_OUTS + S_OUTS + ("lag",))
    d = eng.ukf_smooth(0, "rk4", _params(), ur.to_struct(i["cfgs"]), *(eng.DevArray.from_host(ctx, i[k]) for k in ("x0", "P0", "U", "Y")), DT,
                       lag=eng.DevArray.from_host(ctx, i["lag"]), ctx=ctx)
    assert isinstance(d["xs"], eng.DevArray)
    _same(a, {k: (None if v is None else v.numpy()) for k, v in d.items()}, F_OUTS + S_OUTS + ("lag",))


def test_a_recording_does_not_depend_on_the_batch(eng, ctx):
    """B = 1 against B = 5: every recording alone carries the bits it has in the batch"""
    name = "thr_rk4_ragged"
    i, a = uc.inputs(name), _call(eng.ukf_smooth, ctx, name)
    for b in range(i["B"]):
        s = _call(eng.ukf_smooth, ctx, name, x0=i["x0"][b:b + 1], P0=i["P0"][b:b + 1], U=i["U"][b:b + 1], Y=i["Y"][b:b + 1], lag=i["lag"][:, b:b + 1])
        for k in F_OUTS + S_OUTS + ("lag",):
            assert np.array_equal(s[k][:, 0], a[k][:, b], equal_nan=True), (k, b)


@pytest.mark.parametrize("name", ["thr_rk4", "wr_euler", "thr_euler_wrap"])
def test_split_in_time(eng, ctx, name):
    """filter rows 0..4 with a tape, filter and smooth rows 5..11 from (xT, PT, lag_io), then the backward pass over the first span
    with the second's (xs[0], Ps0) as its terminal pair: the bits of the unbroken call in xs, pstd_s and Ps"""
    i, whole = uc.inputs(name), _call(eng.ukf_smooth, ctx, name)
    t1 = us.T1
    for j in range(P):                                          # x0 and P0 are shared by the candidates: resume one by one
        pj = _params()[j:j + 1]
        lag = None if i["lag"] is None else i["lag"][j:j + 1]
        first = _call(eng.ukf_filter, ctx, name, params=pj, extra=dict(tape=True), U=i["U"][:, :t1], Y=i["Y"][:, :t1], lag=lag)
        second = _call(eng.ukf_smooth, ctx, name, params=pj, x0=first["xT"][0], P0=first["PT"][0], U=i["U"][:, t1:], Y=i["Y"][:, t1:], lag=first["lag"])
        back = eng.ukf_rts(first["xf"], first["tape"], first["nrows"], terminal=(second["xs"][:, :, 0], second["Ps0"]), ctx=ctx)
        for k in ROWS:
            assert np.array_equal(np.concatenate([back[k], second[k]], axis=2), whole[k][j:j + 1]), (name, k, j)
        assert np.array_equal(back["Ps0"], whole["Ps0"][j:j + 1])
        alone = eng.ukf_rts(first["xf"], first["tape"], first["nrows"], ctx=ctx)      # without the pair the first span ends at the filter
        assert np.array_equal(alone["xs"][:, :, t1 - 1], first["xf"][:, :, t1 - 1]) and uc.err(alone["xs"], back["xs"]) > 1e3 * us.TOL


# ------------------------------------------------------------------------------------------ 3. a filter that stops early
def _prefix(eng, ctx, name, clean, b, n, stage=2, **kw):
    """Filter b of the call with the inputs kw completes n rows: nrows says so, its rows < n carry the bits of the same problem cut
    to its first n rows, its rows >= n are NaN, the tape records of transitions that did not complete are NaN (stage 2 of row n - 1
    failed: its Pf stays, xp, Pp and C are NaN; stage 1 of row n failed: record n - 1 is complete), and every other problem carries
    the bits of the clean call.  engine.ukf_smooth gives the bits of the two calls."""
    i = uc.inputs(name)
    got = _two_step(eng, ctx, name, **kw)
    want_n = np.full((P, i["B"]), float(T))
    want_n[:, b] = n
    assert np.array_equal(got["nrows"], want_n), (b, got["nrows"])
    for k in ROWS:
        assert np.isnan(got[k][:, b, n:]).all(), (k, b)
    assert np.isnan(got["tape"][:, b, n:]).all() and np.isfinite(got["tape"][:, b, :max(n - 1, 0)]).all(), b
    if n:
        last = got["tape"][:, b, n - 1]
        assert np.isfinite(last[:, :78]).all() and (np.isfinite(last[:, 78:]).all() if stage == 1 else np.isnan(last[:, 78:]).all()), b
    assert np.array_equal(got["info"][:, b, 2], np.full(P, float(n if stage == 1 else n - 1))), (b, got["info"][:, b])
    if n:
        a = dict(U=i["U"], Y=i["Y"])
        a.update(kw)
        cut = dict(kw, U=a["U"][:, :n], Y=a["Y"][:, :n])
        short = _call(eng.ukf_smooth, ctx, name, **cut)
        for k in ROWS:
            assert np.isfinite(got[k][:, b, :n]).all() and np.array_equal(got[k][:, b, :n], short[k][:, b]), (k, b)
        assert np.array_equal(got["Ps0"][:, b], short["Ps0"][:, b]) and np.array_equal(got["sinfo"][:, b], short["sinfo"][:, b])
        assert np.all(got["sinfo"][:, b, 0] == -1)
    else:
        assert np.isnan(got["Ps0"][:, b]).all() and np.isnan(got["sinfo"][:, b]).all()
    for other in range(i["B"]):
        if other != b:
            for k in F_OUTS + S_OUTS + ("lag", "tape", "nrows"):
                assert np.array_equal(got[k][:, other], clean[k][:, other], equal_nan=True), (k, other, "with a failure in", b)
    _same(_call(eng.ukf_smooth, ctx, name, **kw), got, F_OUTS + S_OUTS + ("lag",), where=(b, n))


@pytest.mark.parametrize("b", range(5))
def test_valid_prefix_in_every_wave_slot(eng, ctx, b):
    """the three conditions under which a filter stops (include/brov2.h: brov_ukf_filter), by the mechanisms of tests/test_ukf_gpu.py, in
    each of the four wave slots of the full block and in the lone wave of the ragged one (B = 5):
    an indefinite P0 under a row 0 without measurements (stage 2 of row 0 fails: n = 1); an infinite command at row 6 (the predicted
    mean is not finite: n = 7); P0[i][i] = -2 r[i] on the last measured component of row 0 (stage 1 of row 0 fails: n = 0); and a
    stage-1 failure at a later row (n = 6), for which the variances must be out of range since the Cholesky factorisation of every
    row vouches for P: q[0] = 5e305 and r[0] = 1.797e308, both finite and so accepted.  Component 0, the x position, on which the
    dynamics do not depend, is measured in row 6 of recording b alone: P[0][0] grows by q[0] a row, stays far below the overflow of
    its sigma points (13 P[0][0] = 3.9e307 in row 6, 7.8e307 in row 11 of the other recordings), and s = P[0][0] + r[0] = 1.8e308
    overflows at the first update that looks at it.  The reference (tests/ukf_smooth_ref.py) says the same: stage 1 of row 6."""
    name = "thr_rk4_ragged"
    i = uc.inputs(name)
    Y0 = i["Y"].copy()
    Y0[:, 0] = np.nan
    P0 = i["P0"].copy()
    P0[b, 1, 0] = 2.0 * P0[b, 0, 0]                             # (the upper triangle is NaN: never read)
    _prefix(eng, ctx, name, _two_step(eng, ctx, name, Y=Y0), b, 1, P0=P0, Y=Y0)
    clean = _two_step(eng, ctx, name)
    U = i["U"].copy()
    U[b, 6, 0] = np.inf
    _prefix(eng, ctx, name, clean, b, 7, U=U)
    r = i["cfgs"].r
    comp = [k for k in range(12) if not np.isnan(i["Y"][b, 0, k]) and np.isfinite(r[k])][-1]
    P0 = i["P0"].copy()
    P0[b, comp, comp] = -2.0 * r[comp]
    _prefix(eng, ctx, name, clean, b, 0, stage=1, P0=P0)
    good = i["cfgs"]
    q, r = good.q.copy(), good.r.copy()
    q[0], r[0] = 5e305, 1.797e308
    wide = ur.Cfg(q=q, r=r, alpha=good.alpha, beta=good.beta, kappa=good.kappa)
    Y = i["Y"].copy()
    Y[:, :, 0] = np.nan
    clean = _two_step(eng, ctx, name, cfg=ur.to_struct(wide), Y=Y)
    assert np.all(clean["nrows"] == T) and np.isfinite(clean["xs"]).all()
    Yb = Y.copy()
    Yb[b, 6, 0] = i["X"][b, 6, 0]
    with np.errstate(over="ignore"):
        o = us.smooth(name, cfgs=wide, x0=i["x0"][b:b + 1], P0=i["P0"][b:b + 1], U=i["U"][b:b + 1], Y=Yb[b:b + 1], lag=i["lag"][:, b:b + 1])
    assert np.all(o["nrows"] == 6) and np.all(o["info"][..., 2] == 6) and np.isfinite(o["xs"][:, :, :6]).all(), "the reference fails in stage 1 of row 6"
    _prefix(eng, ctx, name, clean, b, 6, stage=1, cfg=ur.to_struct(wide), Y=Yb)


# ------------------------------------------------------------------------------------------ 4. a backward pass that stops
@pytest.mark.parametrize("name,j,b,ts", [("thr_rk4_ragged", 1, 2, 6), ("thr_rk4_ragged", 0, 4, 10), ("wr_euler", 0, 0, 0)])
def test_backward_failure(eng, ctx, name, j, b, ts):
    """the Pp block of transition ts of one problem of a clean tape is overwritten on the host by an indefinite matrix
    (Pp[1][0] = 2 Pp[0][0]): sinfo[0] = ts, rows <= ts and Ps0 are NaN, rows > ts and every other problem keep their bits"""
    clean = _two_step(eng, ctx, name)
    tape = clean["tape"].copy()
    tape[j, b, ts, 90 + 1] = 2.0 * tape[j, b, ts, 90]
    got = eng.ukf_rts(clean["xf"], tape, clean["nrows"], ctx=ctx)
    assert got["sinfo"][j, b, 0] == ts and np.isnan(got["Ps0"][j, b]).all()
    assert 0.0 < got["sinfo"][j, b, 1] <= np.sqrt(tape[j, b, ts, 90]), "the pivots up to the failing one are still reported"
    for k in ROWS:
        assert np.isnan(got[k][j, b, :ts + 1]).all() and np.array_equal(got[k][j, b, ts + 1:], clean[k][j, b, ts + 1:]), k
    keep = np.ones(clean["nrows"].shape, dtype=bool)
    keep[j, b] = False
    for k in S_OUTS:
        assert np.array_equal(got[k][keep], clean[k][keep]), k


# ------------------------------------------------------------------------------------------ 5. the host contract
def test_host_contract(eng, ctx):
    """every rule of the header returns BROV_ERR_ARG with a brov_last_error text naming it, and no output buffer is written"""
    from bluerov2_dynamics_amd import _lib
    i = uc.inputs("thr_rk4")
    n = i["B"]
    x0, P0, U, Y = (np.ascontiguousarray(i[k]) for k in ("x0", "P0", "U", "Y"))
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
    cases = [("quaternion model", dict(model=2), "Euler models"),
             ("double-integrator model", dict(model=3), "double-integrator"),
             ("nrec not in {1, P}", dict(cfgs=[edited()] * 3), "nrec"),
             ("alpha = 0", dict(cfgs=[edited(alpha=0.0)]), "alpha"),
             ("alpha = inf", dict(cfgs=[edited(alpha=np.inf)]), "alpha"),
             ("alpha NaN", dict(cfgs=[edited(), edited(alpha=np.nan)]), "alpha"),
             ("n + lambda <= 0", dict(cfgs=[edited(kappa=-12.0)]), "lambda"),
             ("negative q", dict(cfgs=[edited(q=(3, -1e-9))]), "q must"),
             ("NaN q", dict(cfgs=[edited(q=(0, np.nan))]), "q must"),
             ("infinite q", dict(cfgs=[edited(q=(11, np.inf))]), "q must"),
             ("negative r", dict(cfgs=[edited(r=(5, -1e-9))]), "r must"),
             ("NaN r", dict(cfgs=[edited(r=(5, np.nan))]), "r must"),
             ("T < 1", dict(T=0), "T must"),
             ("P > 65535", dict(P=65536), "65535"),
             ("NULL params", dict(null="params"), "NULL"),
             ("NULL x0", dict(null="x0"), "NULL"),
             ("NULL P0", dict(null="P0"), "NULL"),
             ("NULL U", dict(null="U"), "NULL"),
             ("NULL Y", dict(null="Y"), "NULL"),
             ("dt = 0", dict(dt=0.0), "dt"),
             ("dt NaN", dict(dt=np.nan), "dt"),
             ("singular mass matrix", dict(params=heavy), "singular mass"),
             ("tape_bytes below one block of recordings", dict(tape_bytes=block - 1), "one block of recordings"),
             ("negative tape_bytes", dict(tape_bytes=-1), "tape_bytes")]
    sentinel = 7.25
    shapes = dict(eng._ukf_shapes(P, n, T), lag=(P, n, 8, 3))
    order = ("lag",) + F_OUTS + S_OUTS
    for what, kw, word in cases:
        cfgs = kw.get("cfgs", [edited()])
        ca = (_lib.BrovUkf * len(cfgs))(*cfgs)
        ps = (_lib.BrovParams * P)(*kw["params"]) if "params" in kw else pa
        outs = {k: np.full(shapes[k], sentinel) for k in order}
        ptr = dict(params=ps, x0=x0.ctypes.data, P0=P0.ctypes.data, U=U.ctypes.data, Y=Y.ctypes.data)
        if "null" in kw:
            ptr[kw["null"]] = None
        rc = ctx.lib.brov_ukf_smooth(ctx.h, kw.get("model", 0), _lib.RK4, 0, kw.get("P", P), ptr["params"], len(cfgs), ca, n, kw.get("T", T),
                                     kw.get("dt", DT), ptr["x0"], ptr["P0"], ptr["U"], ptr["Y"], *(outs[k].ctypes.data for k in order),
                                     kw.get("tape_bytes", 0))
        msg = (ctx.lib.brov_last_error(ctx.h) or b"").decode()
        print(what, "->", rc, msg)
        assert rc == -1 and word in msg, (what, msg)
        # (dt and the mass matrix are refused by the derivation of the candidates, whose texts name no function for any caller)
        assert msg.startswith("brov_ukf_smooth: ") or word in ("dt", "singular mass"), ("the text names the function that was called", what, msg)
        assert all(np.all(v == sentinel) for v in outs.values()), what
    # exactly one block of recordings is enough
    ok = _call(eng.ukf_smooth, ctx, "thr_rk4", extra=dict(tape_bytes=block, want=("xs",)))
    assert np.isfinite(ok["xs"]).all()
    # B = 0 and P = 0: nothing to do, nothing touched
    r = eng.ukf_smooth(0, "rk4", [], ur.to_struct(good), x0, P0, U, Y, DT, ctx=ctx)
    assert r["xs"].shape == (0, n, T, 12) and r["sinfo"].shape == (0, n, 2)
    r = eng.ukf_smooth(0, "rk4", _params(), ur.to_struct(good), x0[:0], P0[:0], U[:0], Y[:0], DT, ctx=ctx)
    assert r["Ps0"].shape == (P, 0, 12, 12)
    sinfo = np.full((P, n, 2), sentinel)
    ca = (_lib.BrovUkf * 1)(edited())
    for kw in (dict(P=0), dict(B=0)):
        rc = ctx.lib.brov_ukf_smooth(ctx.h, 0, _lib.RK4, 0, kw.get("P", P), pa, 1, ca, kw.get("B", n), T, DT, x0.ctypes.data, P0.ctypes.data,
                                     U.ctypes.data, Y.ctypes.data, *([None] * 11), sinfo.ctypes.data, 0)
        assert rc == 0 and np.all(sinfo == sentinel), kw
    # the tape filter and the backward pass on device buffers
    f = _call(eng.ukf_filter, ctx, "thr_rk4", extra=dict(tape=True))
    D = eng.DevArray.from_host
    xf, tape, nrows, xsT, PsT = D(ctx, f["xf"]), D(ctx, f["tape"]), D(ctx, f["nrows"]), D(ctx, f["xT"]), D(ctx, f["PT"])
    xs = D(ctx, np.full((P, n, T, 12), sentinel))
    p = eng._dptr

    def rts(what, word, P_=P, B_=n, T_=T, xf_=xf, tape_=tape, nrows_=nrows, xsT_=None, PsT_=None, rc_want=-1):
        rc = ctx.lib.brov_ukf_rts_dev(ctx.h, P_, B_, T_, p(xf_), p(tape_), p(nrows_), p(xsT_), p(PsT_), p(xs), None, None, None, None)
        msg = (ctx.lib.brov_last_error(ctx.h) or b"").decode()
        print(what, "->", rc, msg)
        assert rc == rc_want and (rc == 0 or word in msg), (what, msg)
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
    ca = (_lib.BrovUkf * 1)(edited())
    d = [D(ctx, v) for v in (x0, P0, U, Y)]
    for kw, word in ((dict(tape=tape), "go together"), (dict(nrows=nrows), "go together")):
        rc = ctx.lib.brov_ukf_filter_tape_dev(ctx.h, 0, _lib.RK4, 0, P, pa, 1, ca, n, T, DT, *(p(v) for v in d), None, p(xs), None, None, None, None,
                                              None, p(kw.get("tape")), p(kw.get("nrows")))
        msg = (ctx.lib.brov_last_error(ctx.h) or b"").decode()
        assert rc == -1 and word in msg and msg.startswith("brov_ukf_filter_tape_dev: "), msg
        assert np.all(xs.numpy() == sentinel)


# ------------------------------------------------------------------------------------------ 6. the vehicle classes and the example
def test_vehicle_method(eng):
    """rov.smooth_states equals engine.ukf_smooth at P = 1 (thruster and Euler-wrench vehicles), with the default start of
    filter_states, and leaves the object's parameters as they were"""
    from bluerov2_dynamics_amd.fossen.BlueROV2 import BlueROV2
    from bluerov2_dynamics_amd.fossen.BlueROV2_thrust import BlueROV2 as BlueROV2Wrench      # the Euler-angle wrench vehicle
    from bluerov2_dynamics_amd.fossen import estimate, identify
    for cls, name in ((BlueROV2, "thr_rk4"), (BlueROV2Wrench, "wr_rk4")):
        i = uc.inputs(name)
        cfg = ur.to_struct(i["cfgs"])
        rov = cls()
        own = identify.params_of(rov)
        before = ctypes.string_at(ctypes.byref(own), ctypes.sizeof(own))
        s = rov.smooth_states(i["Y"], i["U"], DT, cfg, x0=i["x0"], P0=i["P0"], integrator="rk4")
        want = eng.ukf_smooth(i["model"], "rk4", [own], cfg, i["x0"], i["P0"], i["U"], i["Y"], DT, ctx=rov._ctx)
        for mine, theirs in (("x", "xf"), ("std", "pstd"), ("innov", "innov"), ("PT", "PT"), ("xs", "xs"), ("std_s", "pstd_s"), ("Ps", "Ps"), ("Ps0", "Ps0")):
            assert np.array_equal(s[mine], want[theirs][0], equal_nan=True), mine
        assert np.all(s["failed_transition"] == -1) and np.all(s["failed_step"] == -1) and np.array_equal(s["loglik"], want["info"][0, :, 0])
        f = rov.filter_states(i["Y"], i["U"], DT, cfg, x0=i["x0"], P0=i["P0"], integrator="rk4")
        assert np.array_equal(f["x"], s["x"], equal_nan=True) and uc.err(s["xs"], s["x"]) > 1e3 * us.TOL
        Y = i["Y"].copy()
        Y[:, 1] = np.where(np.isnan(Y[:, 1]), 0.1, Y[:, 1])            # row 1 is the first fully measured one
        dx0, dP0 = estimate.default_start(Y, cfg)
        one = rov.smooth_states(Y[0], i["U"][0], DT, cfg, params=fv.params("V5"), integrator="rk4")
        w1 = eng.ukf_smooth(i["model"], "rk4", [fv.params("V5")], cfg, dx0[:1], dP0[:1], i["U"][:1], Y[:1], DT, ctx=rov._ctx)
        assert one["xs"].shape == (T, 12) and np.array_equal(one["xs"], w1["xs"][0, 0]) and np.array_equal(one["Ps"], w1["Ps"][0, 0])
        own = identify.params_of(rov)
        assert ctypes.string_at(ctypes.byref(own), ctypes.sizeof(own)) == before


def test_example_smooths_small():
    """examples/filter_recording.py --smooth in its small mode: the smoothed RMSE is below the filtered one"""
    import importlib.util
    import os
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "filter_recording.py")
    spec = importlib.util.spec_from_file_location("filter_recording", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    out = mod.main(["--small", "--smooth"])
    print("RMSE raw", out["rmse_raw"], "filtered", out["rmse_filtered"], "smoothed", out["rmse_smoothed"])
    assert out["xs"].shape == (150, 12) and np.all(np.isfinite(out["xs"]))
    assert out["rmse_smoothed"] < out["rmse_filtered"] < out["rmse_raw"]
