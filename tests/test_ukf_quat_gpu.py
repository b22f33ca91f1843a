"""The multiplicative unscented Kalman filter of the quaternion model (brov_ukf_filter_quat / engine.ukf_filter_quat /
rov.filter_states on the quaternion vehicle) on the GPU against tests/ukf_quat_ref.py, the NumPy restatement of the law of
include/brov2.h around the parameterised oracle, at the vehicles V0 and V5 of tests/fossen_vehicles.py.

Recipe of tests/test_ukf_gpu.py: the mixed error max |a-b| / max(1,|b|) formed in long double against TOL_ROLL = 1e-10; every
comparison also runs the reference in np.longdouble and asserts that fp64 and long double stay within a tenth of the bound, that no
[-] comes near half a turn (|e_w| > 0.5) and that no Cholesky pivot is below 1e-4.  Covariances are compared as |dP_ij| / sqrt(P_ii
P_jj) of the reference against the same 1e-10.  The seeds are chosen so that this holds (tests/test_ukf_quat_cpu.py checks it
without a GPU, and shows that the cases tell the law from five of its neighbours).

Shapes, the smallest that can still go wrong (tests/ukf_quat_cases.py): P = 2 candidates; T = 12 rows; B = 3 recordings, which
leaves the fourth wave of the one block idle, and B = 5 in the ragged case: a full block and a block with one live wave; both
instantiations (Euler, RK4); about 30 % NaNs in Y, rows with one number of the quaternion missing, row 4 without any measurement,
error component 7 with r = +inf while its Y column carries numbers, a NaN upper triangle in P0; alpha in {0.5, 1}; a start within
0.1 rad of pitch 90 degrees with x0's quaternion negated and every third measured quaternion multiplied by -2."""
import ctypes

import numpy as np
import pytest

import fossen_vehicles as fv
import ukf_quat_cases as qc
import ukf_quat_ref as uq
import ukf_ref as ur

pytestmark = pytest.mark.gpu

TOL_ROLL = 1e-10
EW = 0.5
PIVOT = 1e-4
P, T, DT = 2, qc.T, qc.DT
OUTS = ("xf", "pstd", "innov", "xT", "PT", "info")
ARGS = ("x0", "P0", "U", "Y")


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


def _run(eng, ctx, name, params=None, want=OUTS, **kw):
    i = qc.inputs(name)
    a = dict(cfg=_structs(i["cfgs"]), x0=i["x0"], P0=i["P0"], U=i["U"], Y=i["Y"])
    a.update(kw)
    return eng.ukf_filter_quat(i["integ"], _params() if params is None else params, a["cfg"], a["x0"], a["P0"], a["U"], a["Y"], DT, want=want,
                               ctx=ctx)


def _same(a, b, keys=OUTS):
    for k in keys:
        assert np.array_equal(a[k], b[k], equal_nan=True), k


def _negq(x):
    x = np.array(x)
    x[..., 3:7] = -x[..., 3:7]
    return x


# ------------------------------------------------------------------------------------------ 1. parity
@pytest.mark.parametrize("name", sorted(qc.CASES))
def test_parity(eng, ctx, name):
    """xf, pstd, innov (same NaN pattern), xT, PT and info against the reference: Euler and RK4, B = 3 and B = 5, a noise record per
    candidate, and the start near vertical with a negated x0 and scaled measured quaternions"""
    got = _run(eng, ctx, name)
    o, ol = qc.reference(name), qc.reference(name, ld=True)
    assert min(o["ew_min"].min(), ol["ew_min"].min()) > EW and min(o["pivot_min"].min(), ol["pivot_min"].min()) > PIVOT
    e, g = qc.gaps(got, o), qc.gaps(o, ol)
    for k in e:
        report(f"{name} {k}", e[k], g[k], TOL_ROLL)
    assert np.array_equal(got["info"][..., 1:3], o["info"][..., 1:3]), "the number of updates and the failed step are exact"
    for j in range(P):
        for b in range(got["PT"].shape[1]):
            assert np.array_equal(got["PT"][j, b], got["PT"][j, b].T), "PT must be bit-symmetric"
    assert qc.err(o["xf"][0], o["xf"][1]) > 1e3 * TOL_ROLL, "the candidates must differ"
    assert got["xf"].shape == (P, qc.inputs(name)["B"], T, 13) and got["xT"].shape[-1] == 13 and got["pstd"].shape[-1] == 12
    if name == "q_rk4_nrec2":
        one = _run(eng, ctx, name, cfg=ur.to_struct(qc.inputs(name)["cfgs"][0]))
        assert np.array_equal(one["xf"][0], got["xf"][0]) and qc.err(one["xf"][1], got["xf"][1]) > 1e3 * TOL_ROLL


# ------------------------------------------------------------------------------------------ 2. exact identities
def test_each_problem_alone_equals_its_slot(eng, ctx):
    """two calls give the same bits; candidate j and recording b alone are their slot of the batch (B = 5: every wave slot and the
    ragged block)"""
    name = "q_rk4_ragged"
    i = qc.inputs(name)
    a = _run(eng, ctx, name)
    _same(a, _run(eng, ctx, name))
    for j in range(P):
        s = _run(eng, ctx, name, params=_params()[j:j + 1])
        for k in OUTS:
            assert np.array_equal(s[k][0], a[k][j], equal_nan=True), (k, j)
    for b in range(i["B"]):
        s = _run(eng, ctx, name, **{k: i[k][b:b + 1] for k in ARGS})
        for k in OUTS:
            assert np.array_equal(s[k][:, 0], a[k][:, b], equal_nan=True), (k, b)


@pytest.mark.parametrize("name", ["q_rk4", "q_euler"])
def test_continuation(eng, ctx, name):
    """a call split at row s and resumed from (xT, PT) gives the unbroken per-row outputs, xT and PT, bit for bit; s = 1, s = 4 and 5
    (around the empty row) and s = 11"""
    i, a = qc.inputs(name), _run(eng, ctx, name)
    for s in (1, 4, 5, 11):
        h = _run(eng, ctx, name, U=i["U"][:, :s], Y=i["Y"][:, :s])
        parts = [_run(eng, ctx, name, params=_params()[j:j + 1], x0=h["xT"][j], P0=h["PT"][j], U=i["U"][:, s:], Y=i["Y"][:, s:]) for j in range(P)]
        for k in ("xf", "pstd", "innov"):
            both = np.concatenate([h[k], np.concatenate([p[k] for p in parts])], axis=2)
            assert np.array_equal(both, a[k], equal_nan=True), (name, s, k)
        for k in ("xT", "PT"):
            assert np.array_equal(np.concatenate([p[k] for p in parts]), a[k]), (name, s, k)
        n2 = h["info"][..., 1] + np.concatenate([p["info"] for p in parts])[..., 1]
        assert np.array_equal(n2, a["info"][..., 1])
        ll = h["info"][..., 0] + np.concatenate([p["info"] for p in parts])[..., 0]
        assert np.max(np.abs(ll - a["info"][..., 0]) / np.abs(a["info"][..., 0])) < 1e-12


@pytest.mark.parametrize("name", ["q_rk4_vertical", "q_euler"])
def test_sign_and_scale_of_the_quaternions(eng, ctx, name):
    """negating x0's quaternion negates the quaternion of xf and xT and leaves every other output as it is; replacing every measured
    quaternion by -2 times itself changes nothing: bit for bit"""
    i, a = qc.inputs(name), _run(eng, ctx, name)
    n = _run(eng, ctx, name, x0=_negq(i["x0"]))
    for k in OUTS:
        assert np.array_equal(n[k], _negq(a[k]) if k in ("xf", "xT") else a[k], equal_nan=True), k
    Y = i["Y"].copy()
    Y[:, :, 3:7] *= -2.0
    _same(a, _run(eng, ctx, name, Y=Y))


def test_host_form_equals_dev_form(eng, ctx):
    """brov_ukf_filter_quat on host arrays = engine.ukf_filter_quat on host arrays (which uploads and calls the _dev form) = the same on
    DevArrays; want=("info",) gives the same info"""
    from bluerov2_dynamics_amd import _lib
    name = "q_rk4"
    i = qc.inputs(name)
    a = _run(eng, ctx, name)
    n = i["B"]
    x0, P0, U, Y = (np.ascontiguousarray(i[k]) for k in ARGS)
    pa = (_lib.BrovParams * P)(*_params())
    ca = (_lib.BrovUkf * 1)(ur.to_struct(i["cfgs"]))
    outs = dict(xf=np.empty((P, n, T, 13)), pstd=np.empty((P, n, T, 12)), innov=np.empty((P, n, T, 12)), xT=np.empty((P, n, 13)),
                PT=np.empty((P, n, 12, 12)), info=np.empty((P, n, 4)))
    rc = ctx.lib.brov_ukf_filter_quat(ctx.h, _lib.RK4, P, pa, 1, ca, n, T, DT, x0.ctypes.data, P0.ctypes.data, U.ctypes.data, Y.ctypes.data,
                                      *(outs[k].ctypes.data for k in OUTS))
    assert rc == 0, ctx.lib.brov_last_error(ctx.h)
    _same(a, outs)
    d = eng.ukf_filter_quat("rk4", _params(), ur.to_struct(i["cfgs"]), *(eng.DevArray.from_host(ctx, i[k]) for k in ARGS), DT, ctx=ctx)
    assert isinstance(d["xf"], eng.DevArray)
    _same(a, {k: v.numpy() for k, v in d.items()})
    only = _run(eng, ctx, name, want=("info",))
    assert only["xf"] is None and only["PT"] is None and np.array_equal(only["info"], a["info"])


# ------------------------------------------------------------------------------------------ 3. a failing filter stops alone
def _failure(eng, ctx, name, clean, b, t_fail, row_kept, cfgs=None, **kw):
    """Filter b of the call with the inputs kw fails at row t_fail, and the reference says so too.  Against the reference: info (l =
    -inf, the updates counted up to the failure, the failed row, the smallest pivot), the NaN pattern of xf / pstd / innov with row
    t_fail kept or not as the header states and the kept rows to TOL_ROLL, xT and PT all NaN.  Every other filter of the call keeps
    the bits of the clean call."""
    i = qc.inputs(name)
    cfgs = i["cfgs"] if cfgs is None else cfgs
    a = {k: i[k] for k in ARGS}
    a.update(kw)
    got = _run(eng, ctx, name, cfg=_structs(cfgs), **kw)
    with np.errstate(all="ignore"):
        o = uq.filter(qc.INTEG[i["integ"]], [fv.vehicle(n) for n in qc.NAMES], cfgs, *(a[k][b:b + 1] for k in ARGS), DT)
    assert np.all(o["info"][:, 0, 2] == t_fail) and np.all(o["info"][:, 0, 0] == -np.inf), ("the reference must fail there", o["info"])
    first_nan = t_fail + 1 if row_kept else t_fail
    for j in range(P):
        assert got["info"][j, b, 0] == -np.inf and np.array_equal(got["info"][j, b, 1:3], o["info"][j, 0, 1:3]), (j, b, got["info"][j, b], o["info"][j, 0])
        assert qc.err(got["info"][j, b, 3], o["info"][j, 0, 3]) < TOL_ROLL, (j, b, got["info"][j, b], o["info"][j, 0])
        assert np.isnan(got["xT"][j, b]).all() and np.isnan(got["PT"][j, b]).all(), (j, b)
        for k in ("xf", "pstd", "innov"):
            assert np.isnan(got[k][j, b, first_nan:]).all() and np.isnan(o[k][j, 0, first_nan:]).all(), (k, j, b)
            if k != "innov" and first_nan:
                assert np.isfinite(got[k][j, b, :first_nan]).all(), (k, j, b)
            e = qc.err(got[k][j, b], o[k][j, 0])                    # inf where the NaN patterns differ
            assert e < TOL_ROLL, (k, j, b, e)
        for other in range(i["B"]):
            if other != b:
                for k in OUTS:
                    assert np.array_equal(got[k][j, other], clean[k][j, other], equal_nan=True), (k, j, other, "with a failure in", b)


def test_failures_stop_alone_in_every_wave_slot(eng, ctx):
    """B = 5, each recording in turn (the four wave slots of the full block and the lone wave of the ragged one):
    (a) an indefinite P0 (P0[1][0] = 2 P0[0][0]) with row 0 carrying no measurement, so that the matrix reaches the factorisation as
        it came: stage 2 at step 0, row 0 kept;
    (b) a measured quaternion of (0, 0, 0, 0) at row 6: stage 1 at t = 6 before any update of the row, rows >= 6 NaN, info[1] counts
        the rows before it only;
    (c) r[2] = 0 with row and column 2 of P0 zero and component 2 measured at row 0: s = 0, stage 1 at t = 0, nothing kept."""
    name = "q_rk4_ragged"
    i = qc.inputs(name)
    Ya = i["Y"].copy()
    Ya[:, 0] = np.nan
    clean_a, clean_b = _run(eng, ctx, name, Y=Ya), _run(eng, ctx, name)
    c0 = i["cfgs"]
    r = c0.r.copy()
    r[2] = 0.0
    cz = ur.cfg(c0.q, r, c0.alpha, c0.beta, c0.kappa)
    Yc = i["Y"].copy()
    Yc[:, :, 2] = np.nan
    clean_c = _run(eng, ctx, name, cfg=ur.to_struct(cz), Y=Yc)
    for clean in (clean_a, clean_b, clean_c):
        assert np.all(clean["info"][..., 2] == -1)
    for b in range(i["B"]):
        P0 = i["P0"].copy()
        P0[b, 1, 0] = 2.0 * P0[b, 0, 0]                             # (the upper triangle is NaN: never read)
        _failure(eng, ctx, name, clean_a, b, 0, True, P0=P0, Y=Ya)
        Y = i["Y"].copy()
        Y[b, 6, 3:7] = 0.0
        _failure(eng, ctx, name, clean_b, b, 6, False, Y=Y)
        P0 = i["P0"].copy()
        P0[b, 2, :3] = 0.0
        P0[b, 3:, 2] = 0.0
        Y = Yc.copy()
        Y[b, 0, :3] = i["X"][b, 0, :3]
        _failure(eng, ctx, name, clean_c, b, 0, False, cfgs=cz, P0=P0, Y=Y)


def test_half_a_turn_fails_stage_one(eng, ctx):
    """a measured attitude exactly half a turn from the estimate (the estimate's own quaternion times a pure imaginary unit, row 0):
    e_w = 0 exactly, the innovation leaves the finite numbers and stage 1 of row 0 fails before any update"""
    name = "q_rk4"
    i = qc.inputs(name)
    clean = _run(eng, ctx, name)
    x0 = i["x0"].copy()
    x0[1, 3:7] = (0.5, 0.5, -0.5, 0.5)
    Y = i["Y"].copy()
    Y[1, 0, 3:7] = uq.qmul(x0[1, 3:7], np.array([0.0, 1.0, 0.0, 0.0]))   # every product is +-0.25: the four terms of e_w cancel exactly
    assert np.sum(x0[1, 3:7] * Y[1, 0, 3:7]) == 0.0
    got = _run(eng, ctx, name, x0=x0, Y=Y)
    assert np.all(got["info"][:, 1, 2] == 0) and np.all(got["info"][:, 1, 1] == 0) and np.all(got["info"][:, 1, 0] == -np.inf)
    assert all(np.isnan(got[k][:, 1]).all() for k in ("xf", "pstd", "innov", "xT", "PT"))
    for b in (0, 2):
        for k in OUTS:
            assert np.array_equal(got[k][:, b], clean[k][:, b], equal_nan=True), (k, b)


# ------------------------------------------------------------------------------------------ 4. the host contract
def test_host_contract(eng, ctx):
    """every rule of the header returns BROV_ERR_ARG with a brov_last_error text naming it, in brov_ukf_filter's words, and no output
    buffer is written; P = 0 and B = 0 return 0 and touch nothing; brov_ukf_filter keeps refusing the quaternion model"""
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
    cases = [("bad integrator", dict(integ=7), "bad enum"),
             ("negative B", dict(B=-1), "negative size"),
             ("B > 2^31", dict(B=(1 << 31) + 1), "2^31"),
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
             ("NULL ukf", dict(null="ukf"), "NULL"),
             ("NULL x0", dict(null="x0"), "NULL"),
             ("NULL P0", dict(null="P0"), "NULL"),
             ("NULL U", dict(null="U"), "NULL"),
             ("NULL Y", dict(null="Y"), "NULL"),
             ("dt = 0", dict(dt=0.0), "dt"),
             ("dt NaN", dict(dt=np.nan), "dt"),
             ("singular mass matrix", dict(params=heavy), "singular mass")]
    sentinel = 7.25

    def fresh():
        return dict(xf=np.full((P, n, T, 13), sentinel), pstd=np.full((P, n, T, 12), sentinel), innov=np.full((P, n, T, 12), sentinel),
                    xT=np.full((P, n, 13), sentinel), PT=np.full((P, n, 12, 12), sentinel), info=np.full((P, n, 4), sentinel))
    for what, kw, word in cases:
        cfgs = kw.get("cfgs", [edited()])
        ca = (_lib.BrovUkf * len(cfgs))(*cfgs)
        ps = (_lib.BrovParams * P)(*kw["params"]) if "params" in kw else pa
        outs = fresh()
        ptr = dict(params=ps, ukf=ca, x0=x0.ctypes.data, P0=P0.ctypes.data, U=U.ctypes.data, Y=Y.ctypes.data)
        if "null" in kw:
            ptr[kw["null"]] = None
        rc = ctx.lib.brov_ukf_filter_quat(ctx.h, kw.get("integ", _lib.RK4), kw.get("P", P), ptr["params"], len(cfgs), ptr["ukf"], kw.get("B", n),
                                          kw.get("T", T), kw.get("dt", DT), ptr["x0"], ptr["P0"], ptr["U"], ptr["Y"],
                                          *(outs[k].ctypes.data for k in OUTS))
        msg = (ctx.lib.brov_last_error(ctx.h) or b"").decode()
        print(what, "->", rc, msg)
        assert rc == -1 and word in msg, (what, msg)
        assert "brov_ukf_filter_quat" in msg or word in ("dt", "singular mass"), ("the text names the function called", msg)
        assert all(np.all(v == sentinel) for v in outs.values()), what
    # B = 0 and P = 0: nothing to do, nothing touched
    r = eng.ukf_filter_quat("rk4", [], ur.to_struct(good), x0, P0, U, Y, DT, ctx=ctx)
    assert r["xf"].shape == (0, n, T, 13) and r["info"].shape == (0, n, 4)
    r = eng.ukf_filter_quat("rk4", _params(), ur.to_struct(good), x0[:0], P0[:0], U[:0], Y[:0], DT, ctx=ctx)
    assert r["xT"].shape == (P, 0, 13)
    for kw in (dict(P=0), dict(B=0)):
        ca = (_lib.BrovUkf * 1)(edited())
        outs = fresh()
        rc = ctx.lib.brov_ukf_filter_quat(ctx.h, _lib.RK4, kw.get("P", P), pa, 1, ca, kw.get("B", n), T, DT, x0.ctypes.data, P0.ctypes.data,
                                          U.ctypes.data, Y.ctypes.data, *(outs[k].ctypes.data for k in OUTS))
        assert rc == 0 and all(np.all(v == sentinel) for v in outs.values()), kw
    # the Euler filter still refuses model 2, in the words its own tests look for
    ca = (_lib.BrovUkf * 1)(edited())
    info = np.full((P, n, 4), sentinel)
    rc = ctx.lib.brov_ukf_filter(ctx.h, _lib.WRENCH_QUAT, _lib.RK4, 0, P, pa, 1, ca, n, T, DT, x0.ctypes.data, P0.ctypes.data, U.ctypes.data,
                                 Y.ctypes.data, None, None, None, None, None, None, info.ctypes.data)
    assert rc == -1 and "Euler models" in (ctx.lib.brov_last_error(ctx.h) or b"").decode() and np.all(info == sentinel)


# ------------------------------------------------------------------------------------------ 5. the vehicle class
def test_vehicle_methods(eng):
    """rov.filter_states and rov.log_likelihood_population of the quaternion vehicle equal engine.ukf_filter_quat on the same arguments
    (x0's quaternion normalised on the host), with the documented default start, and leave the object's parameters as they were;
    smooth_states, fit_noise and simulate_output_feedback raise"""
    from bluerov2_dynamics_amd.fossen.BlueROV2_wrench import BlueROV2
    from bluerov2_dynamics_amd.fossen import estimate, identify
    name = "q_rk4_vertical"
    i = qc.inputs(name)
    cfg = ur.to_struct(i["cfgs"])
    rov = BlueROV2()
    assert rov.MODEL == 2
    own = identify.params_of(rov)
    before = ctypes.string_at(ctypes.byref(own), ctypes.sizeof(own))
    f = rov.filter_states(i["Y"], i["U"], DT, cfg, x0=i["x0"], P0=i["P0"], integrator="rk4")
    xn = i["x0"].copy()
    xn[:, 3:7] /= np.linalg.norm(xn[:, 3:7], axis=1, keepdims=True)
    want = eng.ukf_filter_quat("rk4", [own], cfg, xn, i["P0"], i["U"], i["Y"], DT, ctx=rov._ctx)
    assert f["x"].shape == (i["B"], T, 13) and f["std"].shape == (i["B"], T, 12) and f["xT"].shape == (i["B"], 13)
    assert np.array_equal(f["x"], want["xf"][0], equal_nan=True) and np.array_equal(f["std"], want["pstd"][0], equal_nan=True)
    assert np.array_equal(f["innov"], want["innov"][0], equal_nan=True) and np.array_equal(f["PT"], want["PT"][0])
    assert np.array_equal(f["xT"], want["xT"][0]) and np.array_equal(f["loglik"], want["info"][0, :, 0])
    assert np.all(f["failed_step"] == -1) and f["n_updates"].dtype == np.int64
    scaled = i["x0"].copy()
    scaled[:, 3:7] *= 3.0
    f3 = rov.filter_states(i["Y"], i["U"], DT, cfg, x0=scaled, P0=i["P0"], integrator="rk4")
    # (normalising 3 q instead of q moves x0 by a rounding or two; the filter amplifies that no more than it amplifies its own
    # roundings, which tests/test_ukf_quat_cpu.py bounds by 1e-15 on xf against long double)
    assert qc.err(f3["x"], f["x"]) < 1e-13, "a given x0 need not be unit"
    Y = i["Y"].copy()
    Y[:, 1] = np.where(np.isnan(Y[:, 1]), 0.1, Y[:, 1])            # row 1 is the first fully measured one
    dx0, dP0 = estimate.default_start_quat(Y, cfg)
    one = rov.filter_states(Y[0], i["U"][0], DT, cfg, params=fv.params("V5"), integrator="rk4")
    w1 = eng.ukf_filter_quat("rk4", [fv.params("V5")], cfg, dx0[:1], dP0[:1], i["U"][:1], Y[:1], DT, ctx=rov._ctx)
    assert one["x"].shape == (T, 13) and np.array_equal(one["x"], w1["xf"][0, 0], equal_nan=True) and one["loglik"] == w1["info"][0, 0, 0]
    ll = rov.log_likelihood_population(_params(), i["Y"], i["U"], DT, cfg, x0=i["x0"], P0=i["P0"], integrator="rk4")
    w2 = eng.ukf_filter_quat("rk4", _params(), cfg, xn, i["P0"], i["U"], i["Y"], DT, ctx=rov._ctx)
    assert ll.shape == (P, i["B"]) and np.array_equal(ll, w2["info"][:, :, 0])
    own = identify.params_of(rov)
    assert ctypes.string_at(ctypes.byref(own), ctypes.sizeof(own)) == before
    with pytest.raises(NotImplementedError):
        rov.smooth_states(i["Y"], i["U"], DT, cfg, x0=i["x0"], P0=i["P0"])
    with pytest.raises(NotImplementedError):
        rov.fit_noise(i["Y"], i["U"], DT, cfg, x0=i["x0"], P0=i["P0"], iters=1)
    with pytest.raises(NotImplementedError):
        rov.simulate_output_feedback(i["x0"][0], i["x0"][0], DT, None, cfg, np.zeros((T, 12)))


# ------------------------------------------------------------------------------------------ 6. the example
def test_example_runs_quat():
    """examples/filter_recording.py --quat: from a start near vertical the filter beats the raw rows in position, attitude and
    velocity, the noise model fits and the true vehicle ranks near the top"""
    import importlib.util
    import os
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "filter_recording.py")
    spec = importlib.util.spec_from_file_location("filter_recording", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    out = mod.main(["--quat"])
    assert out["x"].shape == (150, 13) and out["loglik"].shape == (8,) and np.all(np.isfinite(out["loglik"]))
    q = out["X"][0, 3:7]
    assert abs(np.arcsin(2 * (q[0] * q[2] - q[3] * q[1])) - np.pi / 2) < 0.1
    for k in ("position", "attitude", "velocity"):
        assert out["rmse_filtered"][k] < out["rmse_raw"][k], k
    assert 0.7 < out["nis"] < 1.3
    # Three seconds of rows do not pin twelve hydrodynamic terms: the candidate that fits these rows best gains over the true vehicle
    # half a chi-square of at most twelve degrees of freedom, 6 on average, and a drawn vehicle may pick up part of that.  So the
    # true vehicle need not be first, but it is within that gain of the best and in the upper half.
    ll = out["loglik"]
    assert out["rank_true"] == int(np.flatnonzero(out["order"] == 0)[0]) and out["rank_true"] < 4
    assert ll[0] > ll.max() - 6.0 and ll[0] > np.median(ll[1:])
