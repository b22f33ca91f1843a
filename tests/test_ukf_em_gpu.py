"""The EM fit of the filter's q and r on the GPU (brov_ukf_rts_em_dev, brov_ukf_smooth_em[_dev] / engine.ukf_rts_em,
engine.ukf_smooth(want=.."em") / estimate.fit_noise / rov.fit_noise) against tests/ukf_em_ref.py, the NumPy restatement of the law
of include/brov2.h.

Recipe and shapes of tests/test_ukf_smooth_gpu.py: P = 2 candidates, T = 12 rows, B = 3 recordings (B = 5 in the ragged case: a full
block and a block with one live wave); em compared per entry, relative, under the bound 1e-10 of that file with the reference's own
fp64 against long-double gap asserted below a tenth of it (tests/test_ukf_em_cpu.py checks the gaps without a GPU); counts compare
exactly.  The failures of section 6 are numerical conditions of the input which the kernels handle and report."""
import ctypes

import numpy as np
import pytest

import fossen_vehicles as fv
import ukf_cases as uc
import ukf_em_cases as ue
import ukf_em_ref as uer
import ukf_ref as ur

pytestmark = pytest.mark.gpu

P, T, DT = 2, uc.T, uc.DT
F_OUTS = ("xf", "pstd", "innov", "xT", "PT", "info")
S_OUTS = ("xs", "pstd_s", "Ps", "Ps0", "sinfo")
ALL = F_OUTS + S_OUTS
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


def _args(name, **kw):
    i = ue.inputs(name)
    a = dict(cfg=_structs(i["cfgs"]), x0=i["x0"], P0=i["P0"], U=i["U"], Y=i["Y"], lag=i["lag"])
    a.update(kw)
    return i, a


def _call(fn, ctx, name, params=None, extra=None, **kw):
    """fn = engine.ukf_filter or engine.ukf_smooth on inputs(name), with x0 / P0 / U / Y / lag / cfg replaced by kw"""
    i, a = _args(name, **kw)
    return fn(i["model"], i["integ"], _params() if params is None else params, a["cfg"], a["x0"], a["P0"], a["U"], a["Y"], DT, lag=a["lag"],
              lag_mode=i["lag_mode"], ctx=ctx, **(extra or {}))


def _smooth_em(eng, ctx, name, want=ALL + ("em",), **kw):
    extra = dict(kw.pop("extra", {}), want=want)
    return _call(eng.ukf_smooth, ctx, name, extra=extra, **kw)


def _two_step(eng, ctx, name, terminal=None, plain=False, **kw):
    """the tape filter, then the backward pass over its tape (with the EM statistics unless plain): one dict with both calls' outputs"""
    _, a = _args(name, **kw)
    f = _call(eng.ukf_filter, ctx, name, extra=dict(tape=True), **kw)
    if plain:
        f.update(eng.ukf_rts(f["xf"], f["tape"], f["nrows"], terminal=terminal, ctx=ctx))
    else:
        f.update(eng.ukf_rts_em(f["xf"], f["tape"], f["nrows"], a["cfg"], a["Y"], terminal=terminal, ctx=ctx))
    return f


def _same(a, b, keys, where=()):
    for k in keys:
        if a[k] is None or b[k] is None:
            assert a[k] is None and b[k] is None, k
        else:
            assert np.array_equal(a[k], b[k], equal_nan=True), (k,) + tuple(where)


# ------------------------------------------------------------------------------------------ 1. parity
@pytest.mark.parametrize("pair", [False, True], ids=["last_row", "terminal_pair"])
@pytest.mark.parametrize("name", ue.NAMES)
def test_parity(eng, ctx, name, pair):
    got = _two_step(eng, ctx, name, terminal=ue.terminal(name) if pair else None)
    o, ol = ue.reference(name, pair=pair), ue.reference(name, ld=True, pair=pair)
    assert got["em"].shape == (P, ue.inputs(name)["B"], eng.UKF_EM) and eng.UKF_EM == 37
    assert np.array_equal(got["em"][..., 24:], ol["em"][..., 24:].astype(np.float64)), "the counts compare exactly"
    report(f"{name} em", ue.em_err(got["em"], ol["em"]), ue.em_err(o["em"], ol["em"]), ue.TOL)
    assert np.all(got["sinfo"][..., 0] == -1) and np.isfinite(got["em"]).all()


# ------------------------------------------------------------------------------------------ 2. nothing else moves
@pytest.mark.parametrize("name", ["thr_rk4_ragged", "wr_rk4_nrec2", "bigq"])
def test_every_other_output_keeps_its_bits(eng, ctx, name):
    for pair in (None, ue.terminal(name)):
        _same(_two_step(eng, ctx, name, terminal=pair), _two_step(eng, ctx, name, terminal=pair, plain=True), ALL + ("lag", "tape", "nrows"))
    plain = _call(eng.ukf_smooth, ctx, name)
    assert "em" not in plain, "the default want is unchanged"
    _same(_smooth_em(eng, ctx, name), plain, ALL + ("lag",))


# ------------------------------------------------------------------------------------------ 3. bit identities of em
def test_em_bit_identities(eng, ctx):
    from bluerov2_dynamics_amd import _lib
    for name in ("thr_rk4", "wr_rk4_nrec2"):
        two = _two_step(eng, ctx, name)
        one = _smooth_em(eng, ctx, name)
        assert np.array_equal(one["em"], two["em"]), "one call = two steps"
        assert np.array_equal(_smooth_em(eng, ctx, name)["em"], one["em"]), "a second call = the first"
        only = _smooth_em(eng, ctx, name, want=("em",))
        assert all(only[k] is None for k in ALL) and np.array_equal(only["em"], one["em"]), "em alone = every output wanted"
        it = _smooth_em(eng, ctx, name, want=("info", "sinfo", "em"))
        assert np.array_equal(it["em"], one["em"]) and np.array_equal(it["info"], one["info"]) and np.array_equal(it["sinfo"], one["sinfo"])
    # chunked: B = 5 with a tape_bytes of exactly one block of four recordings
    name = "thr_rk4_ragged"
    whole = _smooth_em(eng, ctx, name)
    chunked = _smooth_em(eng, ctx, name, extra=dict(tape_bytes=P * 4 * T * TAPE * 8))
    _same(chunked, whole, ALL + ("lag", "em"))
    # a recording alone = the same recording in the batch of 5: the four wave slots of the full block and the lone wave
    i = ue.inputs(name)
    for b in range(i["B"]):
        s = _smooth_em(eng, ctx, name, want=("em",), x0=i["x0"][b:b + 1], P0=i["P0"][b:b + 1], U=i["U"][b:b + 1], Y=i["Y"][b:b + 1], lag=i["lag"][:, b:b + 1])
        assert np.array_equal(s["em"][:, 0], whole["em"][:, b]), b
    # host form = device form
    name = "thr_rk4"
    i = ue.inputs(name)
    a = _smooth_em(eng, ctx, name)
    n = i["B"]
    x0, P0, U, Y = (np.ascontiguousarray(i[k]) for k in ("x0", "P0", "U", "Y"))
    pa = (_lib.BrovParams * P)(*_params())
    ca = (_lib.BrovUkf * 1)(ur.to_struct(i["cfgs"]))
    shapes = eng._ukf_shapes(P, n, T)
    outs = {k: np.empty(shapes[k]) for k in ALL + ("em",)}
    outs["lag"] = i["lag"].copy()
    rc = ctx.lib.brov_ukf_smooth_em(ctx.h, 0, _lib.RK4, 0, P, pa, 1, ca, n, T, DT, x0.ctypes.data, P0.ctypes.data, U.ctypes.data, Y.ctypes.data,
                                    *(outs[k].ctypes.data for k in ("lag",) + ALL), 0, outs["em"].ctypes.data)
    assert rc == 0, ctx.lib.brov_last_error(ctx.h)
    _same(a, outs, ALL + ("lag", "em"))
    em = np.empty(shapes["em"])                     # every per-row output NULL: one EM iteration of the host form
    info, sinfo, lag = np.empty(shapes["info"]), np.empty(shapes["sinfo"]), i["lag"].copy()
    rc = ctx.lib.brov_ukf_smooth_em(ctx.h, 0, _lib.RK4, 0, P, pa, 1, ca, n, T, DT, x0.ctypes.data, P0.ctypes.data, U.ctypes.data, Y.ctypes.data,
                                    lag.ctypes.data, None, None, None, None, None, info.ctypes.data, None, None, None, None, sinfo.ctypes.data, 0, em.ctypes.data)
    assert rc == 0 and np.array_equal(em, a["em"]) and np.array_equal(info, a["info"]) and np.array_equal(sinfo, a["sinfo"])
    d = eng.ukf_smooth(0, "rk4", _params(), ur.to_struct(i["cfgs"]), *(eng.DevArray.from_host(ctx, i[k]) for k in ("x0", "P0", "U", "Y")), DT,
                       lag=eng.DevArray.from_host(ctx, i["lag"]), want=ALL + ("em",), ctx=ctx)
    assert isinstance(d["em"], eng.DevArray) and np.array_equal(d["em"].numpy(), a["em"])


# ------------------------------------------------------------------------------------------ 4. exact values
def test_exact_values(eng, ctx):
    z = _two_step(eng, ctx, "zeroq")["em"]
    assert np.all(z[..., [2, 9]] == 0.0) and not np.signbit(z[..., [2, 9]]).any(), "Sq[i] == 0.0 where q_i = 0"
    assert np.all(z[..., [0, 1, 3, 4, 5, 6, 7, 8, 10, 11]] > 0)
    name = "thr_rk4_ragged"
    i = ue.inputs(name)
    Y = i["Y"].copy()
    Y[:, :, 2] = np.nan                                         # a column that no row carries
    for pair in (None, ue.terminal(name)):
        em = _two_step(eng, ctx, name, terminal=pair, Y=Y)["em"]
        for k in (uc.UNMEASURED, 2):
            assert np.all(em[..., 12 + k] == 0.0) and np.all(em[..., 24 + k] == 0.0), k
        seen = (~np.isnan(Y)).sum(axis=1).astype(float)
        seen[:, uc.UNMEASURED] = 0
        assert np.array_equal(em[..., 24:36], np.broadcast_to(seen, (P,) + seen.shape)), "nr is the count taken from Y"
        assert np.all(em[..., 36] == (T - 1 if pair is None else T)), "nq"


# ------------------------------------------------------------------------------------------ 5. split in time
@pytest.mark.parametrize("name", ["thr_rk4", "wr_euler", "bigq"])
def test_split_in_time(eng, ctx, name):
    """span 2 without a terminal pair plus span 1 with span 2's (xs[0], Ps0): the em of the unbroken call up to rounding"""
    i, whole = ue.inputs(name), _smooth_em(eng, ctx, name)
    t1 = 5
    cfg = _structs(i["cfgs"])
    gap = ue.em_err(ue.reference(name)["em"], ue.reference(name, ld=True)["em"])
    for j in range(P):                                          # x0 and P0 are shared by the candidates: resume one by one
        pj = _params()[j:j + 1]
        lag = None if i["lag"] is None else i["lag"][j:j + 1]
        first = _call(eng.ukf_filter, ctx, name, params=pj, extra=dict(tape=True), U=i["U"][:, :t1], Y=i["Y"][:, :t1], lag=lag)
        second = _smooth_em(eng, ctx, name, params=pj, x0=first["xT"][0], P0=first["PT"][0], U=i["U"][:, t1:], Y=i["Y"][:, t1:], lag=first["lag"])
        back = eng.ukf_rts_em(first["xf"], first["tape"], first["nrows"], cfg, i["Y"][:, :t1], terminal=(second["xs"][:, :, 0], second["Ps0"]), ctx=ctx)
        assert np.all(back["em"][..., 36] == t1) and np.all(second["em"][..., 36] == T - t1 - 1)
        report(f"{name} candidate {j} split", ue.em_err(back["em"] + second["em"], whole["em"][j:j + 1]), gap, ue.TOL)


# ------------------------------------------------------------------------------------------ 6. prefixes and failures
@pytest.mark.parametrize("b", range(5))
def test_valid_prefix_in_every_wave_slot(eng, ctx, b):
    """nrows of one problem edited to n on the host: its em carries the bits of the call on the first n rows, every other problem
    those of the undisturbed call.  n = 0 (also as NaN): 37 NaN."""
    name = "thr_rk4_ragged"
    i, a = _args(name)
    clean = _two_step(eng, ctx, name)
    for j, n in ((b % 2, 7), (1 - b % 2, 1), (b % 2, 0), (b % 2, np.nan)):
        nrows = clean["nrows"].copy()
        nrows[j, b] = n
        got = eng.ukf_rts_em(clean["xf"], clean["tape"], nrows, a["cfg"], a["Y"], ctx=ctx)
        keep = np.ones(nrows.shape, dtype=bool)
        keep[j, b] = False
        assert np.array_equal(got["em"][keep], clean["em"][keep]), (b, n)
        if n >= 1:
            short = _two_step(eng, ctx, name, U=i["U"][:, :n], Y=i["Y"][:, :n])
            assert np.array_equal(got["em"][j, b], short["em"][j, b]) and got["em"][j, b, 36] == n - 1, (b, n)
        else:
            assert np.isnan(got["em"][j, b]).all() and got["em"][j, b].shape == (37,), (b, n)


@pytest.mark.parametrize("name,j,b,ts", [("thr_rk4_ragged", 1, 2, 6), ("thr_rk4_ragged", 0, 4, 10), ("wr_euler", 0, 0, 0)])
def test_backward_failure(eng, ctx, name, j, b, ts):
    """the Pp block of transition ts of one problem of a clean tape is overwritten on the host by an indefinite matrix
    (Pp[1][0] = 2 Pp[0][0]): 37 NaN for that problem, every other problem keeps the bits of the undisturbed call"""
    _, a = _args(name)
    clean = _two_step(eng, ctx, name)
    tape = clean["tape"].copy()
    tape[j, b, ts, 90 + 1] = 2.0 * tape[j, b, ts, 90]
    got = eng.ukf_rts_em(clean["xf"], tape, clean["nrows"], a["cfg"], a["Y"], ctx=ctx)
    assert got["sinfo"][j, b, 0] == ts and np.isnan(got["em"][j, b]).all()
    keep = np.ones(clean["nrows"].shape, dtype=bool)
    keep[j, b] = False
    for k in S_OUTS + ("em",):
        assert np.array_equal(got[k][keep], clean[k][keep]), k
    _same(got, eng.ukf_rts(clean["xf"], tape, clean["nrows"], ctx=ctx), S_OUTS)


# ------------------------------------------------------------------------------------------ 7. EM on the device
EM_ITERS = 3


def _rel(a, b):
    a, b = np.asarray(a, dtype=uc.L), np.asarray(b, dtype=uc.L)
    if a.shape != b.shape or np.any(np.isposinf(a) != np.isposinf(b)) or np.any(np.isnan(a)) or np.any((b == 0) & (a != 0)):
        return np.inf
    ok = np.isfinite(b) & (b != 0)
    return float(np.max(np.abs(a[ok] - b[ok]) / np.abs(b[ok])))


@pytest.mark.parametrize("name", ["bigq", "thr_rk4"])
def test_fit_noise_follows_the_reference(ctx, name):
    """estimate.fit_noise, EM_ITERS = 3 updates, against ukf_em_ref.em in long double: q and r per entry, relative, and the
    log-likelihood per iteration by the mixed error of tests/ukf_cases.py, under the bound 1e-10; the log-likelihood of each
    candidate rises at every update.  (The fp64 reference's own gap after 3 updates, measured: at most 6e-16 on q, 4e-15 on r and
    2e-16 on the log-likelihood, far below a tenth of the bound, so the count of 3 stands.)"""
    from bluerov2_dynamics_amd.fossen import estimate
    i = ue.inputs(name)
    ref = {ld: uer.em(i["model"], uc.INTEG[i["integ"]], i["lag_mode"], ue.vehicles(), i["cfgs"], i["x0"], i["P0"], i["U"], i["Y"], DT, EM_ITERS,
                      lag=i["lag"], dtype=uc.L if ld else np.float64) for ld in (False, True)}
    got = estimate.fit_noise(i["model"], i["integ"], _params(), ur.to_struct(i["cfgs"]), i["x0"], i["P0"], i["U"], i["Y"], DT, iters=EM_ITERS, tol=0.0,
                             lag=i["lag"], lag_mode=i["lag_mode"], ctx=ctx)
    assert got["loglik"].shape == (EM_ITERS + 1, P) and got["q_hist"].shape == (EM_ITERS + 1, P, 12) and got["n_excluded"] == 0
    assert not got["converged"] and len(got["cfg"]) == P
    for k in ("q", "r", "q_hist", "r_hist"):
        report(f"{name} {k}", _rel(got[k], ref[True][k]), _rel(ref[False][k], ref[True][k]), ue.TOL)
    report(f"{name} loglik", uc.err(got["loglik"], ref[True]["loglik"]), uc.err(ref[False]["loglik"], ref[True]["loglik"]), ue.TOL)
    print(name, "loglik per update and candidate", got["loglik"])
    assert np.all(np.diff(got["loglik"], axis=0) > 0), "the log-likelihood rises at every update"
    assert np.all(np.isposinf(got["r"][:, uc.UNMEASURED]))
    assert np.array_equal(np.array(list(got["cfg"][1].q)), got["q"][1])


# ------------------------------------------------------------------------------------------ 8. the host contract
def test_host_contract(eng, ctx):
    """every refusal returns BROV_ERR_ARG with a text naming the function called, and no output buffer is written"""
    from bluerov2_dynamics_amd import _lib
    i = ue.inputs("thr_rk4")
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
    noise = [("nrec not in {1, P}", dict(cfgs=[edited()] * 3), "nrec"),
             ("negative q", dict(cfgs=[edited(q=(3, -1e-9))]), "q must"),
             ("NaN q", dict(cfgs=[edited(q=(0, np.nan))]), "q must"),
             ("infinite q", dict(cfgs=[edited(), edited(q=(11, np.inf))]), "q must"),
             ("negative r", dict(cfgs=[edited(r=(5, -1e-9))]), "r must"),
             ("NaN r", dict(cfgs=[edited(r=(5, np.nan))]), "r must"),
             ("NULL ukf", dict(null="ukf"), "NULL")]
    heavy = _params()
    heavy[1].m = heavy[1].added_mass[0]
    block = P * 4 * T * TAPE * 8
    cases = noise + [("quaternion model", dict(model=2), "Euler models"),
                     ("alpha = 0", dict(cfgs=[edited(alpha=0.0)]), "alpha"),
                     ("n + lambda <= 0", dict(cfgs=[edited(kappa=-12.0)]), "lambda"),
                     ("T < 1", dict(T=0), "T must"),
                     ("P > 65535", dict(P=65536), "65535"),
                     ("NULL params", dict(null="params"), "NULL"),
                     ("NULL x0", dict(null="x0"), "NULL"),
                     ("NULL Y", dict(null="Y"), "NULL"),
                     ("NULL em", dict(null="em"), "NULL em"),
                     ("dt = 0", dict(dt=0.0), "dt"),
                     ("singular mass matrix", dict(params=heavy), "singular mass"),
                     ("tape_bytes below one block of recordings", dict(tape_bytes=block - 1), "one block of recordings"),
                     ("negative tape_bytes", dict(tape_bytes=-1), "tape_bytes")]
    sentinel = 7.25
    shapes = dict(eng._ukf_shapes(P, n, T), lag=(P, n, 8, 3))
    order = ("lag",) + ALL
    for what, kw, word in cases:
        cfgs = kw.get("cfgs", [edited()])
        ca = (_lib.BrovUkf * len(cfgs))(*cfgs)
        ps = (_lib.BrovParams * P)(*kw["params"]) if "params" in kw else pa
        outs = {k: np.full(shapes[k], sentinel) for k in order + ("em",)}
        ptr = dict(params=ps, ukf=ca, x0=x0.ctypes.data, P0=P0.ctypes.data, U=U.ctypes.data, Y=Y.ctypes.data, em=outs["em"].ctypes.data)
        if "null" in kw:
            ptr[kw["null"]] = None
        rc = ctx.lib.brov_ukf_smooth_em(ctx.h, kw.get("model", 0), _lib.RK4, 0, kw.get("P", P), ptr["params"], len(cfgs), ptr["ukf"], n, kw.get("T", T),
                                        kw.get("dt", DT), ptr["x0"], ptr["P0"], ptr["U"], ptr["Y"], *(outs[k].ctypes.data for k in order),
                                        kw.get("tape_bytes", 0), ptr["em"])
        msg = (ctx.lib.brov_last_error(ctx.h) or b"").decode()
        print(what, "->", rc, msg)
        assert rc == -1 and word in msg, (what, msg)
        assert msg.startswith("brov_ukf_smooth_em: ") or word in ("dt", "singular mass"), ("the text names the function that was called", what, msg)
        assert all(np.all(v == sentinel) for v in outs.values()), what
    # P = 0 and B = 0: nothing to do, nothing touched
    em = np.full((P, n, 37), sentinel)
    ca = (_lib.BrovUkf * 1)(edited())
    for kw in (dict(P=0), dict(B=0)):
        rc = ctx.lib.brov_ukf_smooth_em(ctx.h, 0, _lib.RK4, 0, kw.get("P", P), pa, 1, ca, kw.get("B", n), T, DT, x0.ctypes.data, P0.ctypes.data,
                                        U.ctypes.data, Y.ctypes.data, *([None] * 12), 0, em.ctypes.data)
        assert rc == 0 and np.all(em == sentinel), kw
    r = eng.ukf_smooth(0, "rk4", _params(), ur.to_struct(good), x0[:0], P0[:0], U[:0], Y[:0], DT, want=("em",), ctx=ctx)
    assert r["em"].shape == (P, 0, 37)
    # the device forms
    f = _call(eng.ukf_filter, ctx, "thr_rk4", extra=dict(tape=True))
    D = eng.DevArray.from_host
    xf, tape, nrows, xsT, PsT, Yd = D(ctx, f["xf"]), D(ctx, f["tape"]), D(ctx, f["nrows"]), D(ctx, f["xT"]), D(ctx, f["PT"]), D(ctx, Y)
    emd, xs = D(ctx, np.full((P, n, 37), sentinel)), D(ctx, np.full((P, n, T, 12), sentinel))
    p = eng._dptr

    def rts(what, word, P_=P, B_=n, T_=T, xf_=xf, tape_=tape, nrows_=nrows, xsT_=None, PsT_=None, cfgs=None, ukf_null=False, Y_=Yd, em_=emd, rc_want=-1):
        cfgs = cfgs or [edited()]
        ca = None if ukf_null else (_lib.BrovUkf * len(cfgs))(*cfgs)
        rc = ctx.lib.brov_ukf_rts_em_dev(ctx.h, P_, B_, T_, p(xf_), p(tape_), p(nrows_), p(xsT_), p(PsT_), p(xs), None, None, None, None,
                                         len(cfgs), ca, p(Y_), p(em_))
        msg = (ctx.lib.brov_last_error(ctx.h) or b"").decode()
        print(what, "->", rc, msg)
        assert rc == rc_want and (rc == 0 or (word in msg and msg.startswith("brov_ukf_rts_em_dev: "))), (what, msg)
        assert np.all(xs.numpy() == sentinel) and np.all(emd.numpy() == sentinel), what
    for what, kw, word in noise:
        rts(what, word, cfgs=kw.get("cfgs"), ukf_null="null" in kw)
    rts("xs_T without Ps_T", "terminal pair", xsT_=xsT)
    rts("Ps_T without xs_T", "terminal pair", PsT_=PsT)
    rts("NULL xf", "NULL", xf_=None)
    rts("NULL tape", "NULL", tape_=None)
    rts("NULL nrows", "NULL", nrows_=None)
    rts("NULL Y", "NULL", Y_=None)
    rts("NULL em", "NULL", em_=None)
    rts("T < 1", "T must", T_=0)
    rts("P > 65535", "65535", P_=65536)
    rts("negative B", "negative", B_=-1)
    rts("P = 0", "", P_=0, rc_want=0)
    rts("B = 0", "", B_=0, rc_want=0)
    d = [D(ctx, v) for v in (x0, P0, U, Y)]
    for what, kw, word in noise + [("NULL em", dict(null="em"), "NULL em")]:
        cfgs = kw.get("cfgs", [edited()])
        ca = None if kw.get("null") == "ukf" else (_lib.BrovUkf * len(cfgs))(*cfgs)
        rc = ctx.lib.brov_ukf_smooth_em_dev(ctx.h, 0, _lib.RK4, 0, P, pa, len(cfgs), ca, n, T, DT, *(p(v) for v in d), None, None, None, None, None,
                                            None, None, p(xs), None, None, None, None, 0, None if kw.get("null") == "em" else p(emd))
        msg = (ctx.lib.brov_last_error(ctx.h) or b"").decode()
        assert rc == -1 and word in msg and msg.startswith("brov_ukf_smooth_em_dev: "), (what, msg)
        assert np.all(xs.numpy() == sentinel) and np.all(emd.numpy() == sentinel), what


# ------------------------------------------------------------------------------------------ 9. the vehicle classes and the example
def test_vehicle_methods(eng):
    """rov.fit_noise and rov.fit_noise_population are estimate.fit_noise at P = 1 and at P candidates, and leave the object's
    parameters as they were; the true vehicle explains the recordings better under its own fitted noise than the other candidate"""
    from bluerov2_dynamics_amd.fossen.BlueROV2 import BlueROV2
    from bluerov2_dynamics_amd.fossen import estimate, identify
    i = ue.inputs("bigq")
    from bluerov2_dynamics_amd.fossen.BlueROV2_thrust import BlueROV2 as BlueROV2Wrench      # the Euler-angle wrench vehicle
    rov = BlueROV2Wrench()
    cfg = ur.to_struct(i["cfgs"])
    own = identify.params_of(rov)
    before = ctypes.string_at(ctypes.byref(own), ctypes.sizeof(own))
    true = fv.params(uc.TRUE)
    one = rov.fit_noise(i["Y"], i["U"], DT, cfg, x0=i["x0"], P0=i["P0"], params=true, integrator="rk4", iters=4, tol=0.0)
    want = estimate.fit_noise(i["model"], "rk4", [true], cfg, i["x0"], i["P0"], i["U"], i["Y"], DT, iters=4, tol=0.0, ctx=rov._ctx)
    assert one["q"].shape == (12,) and one["loglik"].shape == (5,) and np.array_equal(one["q"], want["q"][0]) and np.array_equal(one["r"], want["r"][0])
    assert np.array_equal(one["loglik"], want["loglik"][:, 0]) and np.all(np.diff(one["loglik"]) > 0)
    m = np.arange(12) != uc.UNMEASURED
    start, fit = np.sqrt(np.array(list(cfg.r)))[m], np.sqrt(one["r"])[m]
    print("sigma true", uc.SIGMA[m], "start", start, "fitted", fit)
    assert np.all(np.abs(fit - uc.SIGMA[m]) < np.abs(start - uc.SIGMA[m])), "the fitted sigma is closer to the truth in every measured component"
    s = rov.smooth_states(i["Y"], i["U"], DT, one["cfg"], x0=i["x0"], P0=i["P0"], params=true, integrator="rk4")
    assert abs(s["loglik"].sum() - one["loglik"][-1]) < 1e-12 * abs(one["loglik"][-1]), "the last row is the log-likelihood under the fitted record"
    pop = rov.fit_noise_population(_params(), i["Y"], i["U"], DT, cfg, x0=i["x0"], P0=i["P0"], integrator="rk4", iters=4, tol=0.0)
    assert pop["q"].shape == (P, 12) and pop["loglik"].shape == (5, P) and np.array_equal(pop["loglik_fitted"], pop["loglik"][-1])
    assert np.array_equal(pop["q"][1], one["q"]) and np.array_equal(pop["loglik"][:, 1], one["loglik"]), "candidate 1 is the true vehicle"
    assert pop["loglik_fitted"][1] > pop["loglik_fitted"][0]
    own = identify.params_of(rov)
    assert ctypes.string_at(ctypes.byref(own), ctypes.sizeof(own)) == before
    thr = BlueROV2()
    j = ue.inputs("thr_rk4")
    t = thr.fit_noise(j["Y"][0], j["U"][0], DT, ur.to_struct(ue.start_cfg(0.5)), x0=j["x0"][0], P0=j["P0"][0], params=true, integrator="rk4", iters=2, tol=0.0)
    assert t["loglik"].shape == (3,) and np.all(np.diff(t["loglik"]) > 0)


def test_example_fits_noise_small():
    """examples/filter_recording.py --fit-noise in its small mode: the log-likelihood rises, the fitted sigma is closer to the truth
    than the start in every measured component"""
    import importlib.util
    import os
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "filter_recording.py")
    spec = importlib.util.spec_from_file_location("filter_recording", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    out = mod.main(["--small", "--fit-noise"])
    m = np.arange(12) != mod.UNMEASURED
    assert np.all(np.diff(out["loglik_fit"]) > 0)
    assert np.all(np.abs(out["sigma_fit"] - mod.SIGMA)[m] < np.abs(out["sigma_start"] - mod.SIGMA)[m])
    print("RMSE filtered", out["rmse_filtered_before"], "->", out["rmse_filtered_after"], "smoothed", out["rmse_smoothed_before"], "->", out["rmse_smoothed_after"])
    assert out["fit_converged"] and np.isfinite([out["rmse_filtered_after"], out["rmse_smoothed_after"]]).all()
