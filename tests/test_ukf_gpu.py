"""The unscented Kalman filter (brov_ukf_filter / engine.ukf_filter / rov.filter_states) on the GPU against tests/ukf_ref.py, the
NumPy restatement of the law of include/brov2.h around the parameterised oracle, at the vehicles V0 and V5 of
tests/fossen_vehicles.py.

Recipe of tests/test_mppi_gpu.py: the mixed error max |a-b| / max(1,|b|) formed in long double against TOL_ROLL = 1e-10; every
comparison also runs the reference in np.longdouble and asserts that fp64 and long double stay within a tenth of the bound, that
no wrap sits within 1e-6 of its threshold and that no Cholesky pivot is below 1e-4.  Covariances are compared as
|dP_ij| / sqrt(P_ii P_jj) of the reference against the same 1e-10.  The seeds are chosen so that this holds (tests/test_ukf_cpu.py
checks it without a GPU).

Shapes, the smallest that can still go wrong (tests/ukf_cases.py): P = 2 candidates; T = 12 rows; B = 3 recordings, which leaves
the fourth wave of the one block idle (the kernel packs four recordings, one per wave, into a block), and B = 5 in the ragged case:
a full block and a block with one live wave; about 30 % NaNs in Y, row 4 without any measurement, component 7 with r = +inf while its
Y column carries numbers, a NaN upper triangle in P0, a start lag for the thruster model; alpha in {0.5, 1}.  The other shapes (no start lag, full
blocks, P = 1 and 3, T = 1 ..) run in the sweep of tests/test_family_sweeps_gpu.py; section 5 here takes the three failure
conditions of the header on corner cases of that sweep (tests/sweep_cases.py: UKF_CORNERS), in every wave slot."""
import ctypes

import numpy as np
import pytest

import fossen_vehicles as fv
import sweep_cases as sc
import sweep_ukf_lmpc as su
import ukf_cases as uc
import ukf_ref as ur

pytestmark = pytest.mark.gpu

TOL_ROLL = 1e-10
MARGIN = 1e-6
PIVOT = 1e-4
P, T, DT = 2, uc.T, uc.DT
OUTS = ("xf", "pstd", "innov", "xT", "PT", "info")


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


def _params(names=uc.NAMES):
    return [fv.params(n) for n in names]


def _structs(cfgs):
    return ur.to_struct(cfgs) if isinstance(cfgs, ur.Cfg) else [ur.to_struct(c) for c in cfgs]


def _run(eng, ctx, name, params=None, **kw):
    i = uc.inputs(name)
    a = dict(cfg=_structs(i["cfgs"]), x0=i["x0"], P0=i["P0"], U=i["U"], Y=i["Y"], lag=i["lag"], lag_mode=i["lag_mode"])
    a.update(kw)
    return eng.ukf_filter(i["model"], i["integ"], _params() if params is None else params, a["cfg"], a["x0"], a["P0"], a["U"], a["Y"], DT,
                          lag=a["lag"], lag_mode=a["lag_mode"], ctx=ctx)


def _check(name, got):
    o, ol = uc.reference(name), uc.reference(name, ld=True)
    assert min(o["wrap_margin"].min(), ol["wrap_margin"].min()) > MARGIN and min(o["pivot_min"].min(), ol["pivot_min"].min()) > PIVOT
    have = {k: got[k] for k in OUTS}
    have["lag"] = got["lag"] if got["lag"] is not None else o["lag"]
    assert (got["lag"] is None) == (uc.inputs(name)["lag"] is None)
    e, g = uc.gaps(have, o), uc.gaps(o, ol)
    for k in e:
        report(f"{name} {k}", e[k], g[k], TOL_ROLL)
    assert np.array_equal(got["info"][..., 1:3], o["info"][..., 1:3]), "the number of updates and the failed step are exact"
    for j in range(got["PT"].shape[0]):
        for b in range(got["PT"].shape[1]):
            assert np.array_equal(got["PT"][j, b], got["PT"][j, b].T), "PT must be bit-symmetric"
    return o


def _same(a, b, keys=OUTS + ("lag",)):
    for k in keys:
        if a[k] is None or b[k] is None:
            assert a[k] is None and b[k] is None, k
        else:
            assert np.array_equal(a[k], b[k], equal_nan=True), k


# ------------------------------------------------------------------------------------------ 1. - 3. parity
@pytest.mark.parametrize("name", ["thr_euler", "thr_rk4", "wr_euler", "wr_rk4", "thr_rk4_ragged"])
def test_parity(eng, ctx, name):
    """xf, pstd, innov (same NaN pattern), xT, PT, info and lag_io against the reference: models 0 and 1 x Euler / RK4, and B = 5
    (one full block of four waves and a block with one live wave)"""
    o = _check(name, _run(eng, ctx, name))
    assert uc.err(o["xf"][0], o["xf"][1]) > 1e3 * TOL_ROLL, "the candidates must differ"


def test_parity_lag_per_step(eng, ctx):
    """BROV_LAG_PER_STEP; on the reference the lag mode matters"""
    name = "thr_rk4_lagstep"
    o = _check(name, _run(eng, ctx, name))
    assert uc.err(o["xf"], uc.reference(name, lag_mode=0)["xf"]) > 1e3 * TOL_ROLL


def test_two_noise_records(eng, ctx):
    """nrec = P: candidate j under its own noise record (the second one with another alpha and 1.5 x the measurement sigma)"""
    name = "wr_rk4_nrec2"
    got = _run(eng, ctx, name)
    _check(name, got)
    one = _run(eng, ctx, name, cfg=ur.to_struct(uc.inputs(name)["cfgs"][0]))
    assert np.array_equal(one["xf"][0], got["xf"][0]) and uc.err(one["xf"][1], got["xf"][1]) > 1e3 * TOL_ROLL


def test_yaw_through_pi(eng, ctx):
    """the true yaw leaves [-pi, pi] while Y reports it wrapped: innovations are shifted by 2 pi (asserted on the reference) and the
    filtered yaw stays continuous"""
    name = "thr_euler_wrap"
    got = _run(eng, ctx, name)
    o = _check(name, got)
    assert o["shifted"].min() > 0
    assert np.nanmax(got["xf"][..., 5]) > np.pi + 0.02


# ------------------------------------------------------------------------------------------ 4. exact identities
def test_exact_identities(eng, ctx):
    name = "thr_rk4"
    i = uc.inputs(name)
    a = _run(eng, ctx, name)
    _same(a, _run(eng, ctx, name))                                                   # two calls give the same bits
    for j in range(P):                                                               # candidate j of P = 2 is the P = 1 call on params[j]
        s = _run(eng, ctx, name, params=_params()[j:j + 1], lag=i["lag"][j:j + 1])
        for k in OUTS + ("lag",):
            assert np.array_equal(s[k][0], a[k][j], equal_nan=True), (k, j)
    # r[i] = +inf equals NaN in column i of Y
    c = i["cfgs"]
    r2 = c.r.copy()
    r2[7], r2[2] = 1e-4, np.inf
    Y2 = i["Y"].copy()
    Y2[:, :, 7] = np.nan
    Y3 = Y2.copy()
    Y3[:, :, 2] = np.nan
    r3 = r2.copy()
    r3[2] = c.r[2]
    _same(_run(eng, ctx, name, cfg=ur.to_struct(ur.cfg(c.q, r2, c.alpha, c.beta, c.kappa)), Y=Y2),
          _run(eng, ctx, name, cfg=ur.to_struct(ur.cfg(c.q, r3, c.alpha, c.beta, c.kappa)), Y=Y3))
    # lag_io out is brov_rollout_pop's lag_io on the same commands and start lag
    xs = np.zeros((i["B"], 12))
    for lag_mode in (0, 1):
        f = _run(eng, ctx, name, lag_mode=lag_mode)
        pop = eng.rollout_pop(0, "rk4", _params(), xs, i["U"], DT, lag=i["lag"], lag_mode=lag_mode, store=False, ctx=ctx)
        assert np.array_equal(f["lag"], pop["lag"]), lag_mode
    # 12 rows = 5 + 7 rows resumed from (xT, PT, lag_io)
    for nm in (name, "wr_euler"):
        i, a = uc.inputs(nm), _run(eng, ctx, nm)
        h = _run(eng, ctx, nm, U=i["U"][:, :5], Y=i["Y"][:, :5])
        parts = []
        for j in range(P):                                                           # x0 and P0 are shared by the candidates: resume one by one
            parts.append(_run(eng, ctx, nm, params=_params()[j:j + 1], x0=h["xT"][j], P0=h["PT"][j], U=i["U"][:, 5:], Y=i["Y"][:, 5:],
                              lag=None if h["lag"] is None else h["lag"][j:j + 1]))
        for k in ("xf", "pstd", "innov"):
            both = np.concatenate([h[k], np.concatenate([p[k] for p in parts])], axis=2)
            assert np.array_equal(both, a[k], equal_nan=True), (nm, k)
        for k in ("xT", "PT") + (("lag",) if a["lag"] is not None else ()):
            assert np.array_equal(np.concatenate([p[k] for p in parts]), a[k]), (nm, k)
        ll = h["info"][..., 0] + np.concatenate([p["info"] for p in parts])[..., 0]
        assert np.max(np.abs(ll - a["info"][..., 0]) / np.abs(a["info"][..., 0])) < 1e-12
        n2 = h["info"][..., 1] + np.concatenate([p["info"] for p in parts])[..., 1]
        assert np.array_equal(n2, a["info"][..., 1])


# ------------------------------------------------------------------------------------------ 5. a failing filter
@pytest.mark.parametrize("name", ["thr_rk4", "wr_euler"])
def test_indefinite_P0_fails_alone(eng, ctx, name):
    """recording 1 starts from a P0 that is not positive definite (P0[0][1] = P0[1][0] = 2 P0[0][0]): a numerical condition handled in
    the kernel.  Its info reports step 0 and l = -inf, its outputs after the failing stage are NaN; the others keep their bits."""
    i = uc.inputs(name)
    a = _run(eng, ctx, name)
    P0 = i["P0"].copy()
    P0[1, 1, 0] = P0[1, 0, 1] = 2.0 * P0[1, 0, 0]
    got = _run(eng, ctx, name, P0=P0)
    o = ur.filter(i["model"], uc.INTEG[i["integ"]], i["lag_mode"], [fv.vehicle(n) for n in uc.NAMES], i["cfgs"], i["x0"], P0, i["U"], i["Y"], DT,
                  lag=i["lag"])
    assert np.all(o["info"][:, 1, 2] == 0)
    for j in range(P):
        assert got["info"][j, 1, 0] == -np.inf and got["info"][j, 1, 2] == 0 and got["info"][j, 1, 1] == o["info"][j, 1, 1]
        assert np.isnan(got["xT"][j, 1]).all() and np.isnan(got["PT"][j, 1]).all()
        for k in ("xf", "pstd", "innov"):
            assert np.isnan(got[k][j, 1, 1:]).all(), k
            assert np.array_equal(np.isnan(got[k][j, 1, 0]), np.isnan(o[k][j, 1, 0])), k      # row 0 is kept when its update was complete
        if got["lag"] is not None:
            assert np.array_equal(got["lag"][j, 1], i["lag"][j, 1])
        for b in (0, 2):
            for k in OUTS + (("lag",) if got["lag"] is not None else ()):
                assert np.array_equal(got[k][j, b], a[k][j, b], equal_nan=True), (k, j, b)



def _sweep_case(**want):
    """the first corner of the sweep's ukf list that holds `want`, with its inputs"""
    c = [c for c in sc.corners("ukf") if all(c[k] == v for k, v in want.items())][0]
    return c, su.ukf_inputs(c)


def _failure(eng, ctx, c, i, clean, b, t_fail, row_kept, **kw):
    """Filter b of the call with the inputs kw fails at row t_fail; ukf_ref says so too.  Against ukf_ref: info (l = -inf, the updates
    counted up to the failure, the failed row, the smallest pivot), the NaN pattern of xf / pstd / innov with row t_fail kept or not
    as the header states and the kept rows to TOL_ROLL, xT and PT all NaN.  lag_io of the failed filter is untouched, and every
    other filter of the call keeps the bits of the clean call."""
    got = su.run_ukf(eng, ctx, c, i, **kw)
    a = dict(x0=i["x0"], P0=i["P0"], U=i["U"], Y=i["Y"])
    a.update(kw)
    with np.errstate(all="ignore"):
        o = ur.filter(c["model"], su.INTEG[c["integ"]], c["lag_mode"], [fv.vehicle(n) for n in c["names"]], i["cfgs"], a["x0"][b:b + 1], a["P0"][b:b + 1],
                      a["U"][b:b + 1], a["Y"][b:b + 1], DT, lag=None if i["lag"] is None else i["lag"][:, b:b + 1])
    assert np.all(o["info"][:, 0, 2] == t_fail) and np.all(o["info"][:, 0, 0] == -np.inf), ("the reference must fail there", o["info"])
    first_nan = t_fail + 1 if row_kept else t_fail
    for j in range(c["P"]):
        assert got["info"][j, b, 0] == -np.inf and np.array_equal(got["info"][j, b, 1:3], o["info"][j, 0, 1:3]), (j, b, got["info"][j, b], o["info"][j, 0])
        assert uc.err(got["info"][j, b, 3], o["info"][j, 0, 3]) < TOL_ROLL, (j, b, got["info"][j, b], o["info"][j, 0])
        assert np.isnan(got["xT"][j, b]).all() and np.isnan(got["PT"][j, b]).all(), (j, b)
        for k in ("xf", "pstd", "innov"):
            assert np.isnan(got[k][j, b, first_nan:]).all() and np.isnan(o[k][j, 0, first_nan:]).all(), (k, j, b)
            if k != "innov" and first_nan:
                assert np.isfinite(got[k][j, b, :first_nan]).all(), (k, j, b)
            e = uc.err(got[k][j, b], o[k][j, 0])                    # inf where the NaN patterns differ
            assert e < TOL_ROLL, (k, j, b, e)
        if c["lag"]:
            assert np.array_equal(got["lag"][j, b], i["lag"][j, b]), ("lag_io of a failed filter", j, b)
        else:
            assert got["lag"] is None
        for other in range(c["B"]):
            if other != b:
                for k in OUTS + (("lag",) if c["lag"] else ()):
                    assert np.array_equal(got[k][j, other], clean[k][j, other], equal_nan=True), (k, j, other, "with a failure in", b)


@pytest.mark.parametrize("P,model", [(1, 0), (3, 1)])
def test_bad_pivot_in_every_wave_slot(eng, ctx, P, model):
    """the indefinite P0 of test_indefinite_P0_fails_alone, at P = 1 and P = 3 and B = 5, in each recording in turn: the four wave
    slots of the full block and the lone wave of the ragged last block.  Row 0 of every recording carries no measurement here, so
    that the indefinite matrix reaches the Cholesky factorisation whatever the noise (an update could meet s <= 0 first); the row's
    update is complete, so row 0 is kept."""
    c, i = _sweep_case(P=P, model=model, B=5, T=12, measured="all")
    Y = i["Y"].copy()
    Y[:, 0] = np.nan
    clean = su.run_ukf(eng, ctx, c, i, Y=Y)
    assert np.all(clean["info"][..., 2] == -1)
    for b in range(c["B"]):
        P0 = i["P0"].copy()
        P0[b, 1, 0] = 2.0 * P0[b, 0, 0]                             # (the upper triangle is NaN: never read)
        _failure(eng, ctx, c, i, clean, b, 0, True, P0=P0, Y=Y)


@pytest.mark.parametrize("want", [dict(model=0, lag=True, T=12, measured="std", P=2), dict(model=0, lag=False, T=12, measured="std", B=9),
                                  dict(model=1, T=12, measured="std", P=3)])
def test_stage_one_failure_and_a_non_finite_prediction(eng, ctx, want):
    """(a) s = P[i][i] + r[i] <= 0 at row 0: P0[i][i] = -2 r[i] on the last measured component of the row, so that the earlier
    updates of the row are applied and counted; the row is not kept: rows 0 .. are NaN.  (b) an infinite command at row t > 0 (the
    header does not validate U): the predicted mean is not finite, row t is kept, rows t + 1 .. are NaN.  Both in wave slot 1 of the
    first block and in the last recording; a thruster filter with and without a start lag and a wrench filter."""
    c, i = _sweep_case(**want)
    clean = su.run_ukf(eng, ctx, c, i)
    assert np.all(clean["info"][..., 2] == -1)
    r = (i["cfgs"] if isinstance(i["cfgs"], ur.Cfg) else i["cfgs"][0]).r
    for b in (1, c["B"] - 1):
        comp = [k for k in range(12) if not np.isnan(i["Y"][b, 0, k]) and np.isfinite(r[k])][-1]
        P0 = i["P0"].copy()
        P0[b, comp, comp] = -2.0 * r[comp]
        _failure(eng, ctx, c, i, clean, b, 0, False, P0=P0)
        for t in (3, c["T"] - 1):
            U = i["U"].copy()
            U[b, t, 0] = np.inf
            _failure(eng, ctx, c, i, clean, b, t, True, U=U)


# ------------------------------------------------------------------------------------------ 6. the host contract
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
             ("singular mass matrix", dict(params=heavy), "singular mass")]
    sentinel = 7.25
    for what, kw, word in cases:
        cfgs = kw.get("cfgs", [edited()])
        ca = (_lib.BrovUkf * len(cfgs))(*cfgs)
        ps = (_lib.BrovParams * P)(*kw["params"]) if "params" in kw else pa
        outs = dict(lag=np.full((P, n, 8, 3), sentinel), xf=np.full((P, n, T, 12), sentinel), pstd=np.full((P, n, T, 12), sentinel),
                    innov=np.full((P, n, T, 12), sentinel), xT=np.full((P, n, 12), sentinel), PT=np.full((P, n, 12, 12), sentinel),
                    info=np.full((P, n, 4), sentinel))
        ptr = dict(params=ps, x0=x0.ctypes.data, P0=P0.ctypes.data, U=U.ctypes.data, Y=Y.ctypes.data)
        if "null" in kw:
            ptr[kw["null"]] = None
        rc = ctx.lib.brov_ukf_filter(ctx.h, kw.get("model", 0), _lib.RK4, 0, kw.get("P", P), ptr["params"], len(cfgs), ca, n, kw.get("T", T),
                                     kw.get("dt", DT), ptr["x0"], ptr["P0"], ptr["U"], ptr["Y"], *(outs[k].ctypes.data for k in
                                                                                                   ("lag", "xf", "pstd", "innov", "xT", "PT", "info")))
        msg = (ctx.lib.brov_last_error(ctx.h) or b"").decode()
        print(what, "->", rc, msg)
        assert rc == -1 and word in msg, (what, msg)
        assert all(np.all(v == sentinel) for v in outs.values()), what
    # B = 0 and P = 0: nothing to do, nothing touched
    r = eng.ukf_filter(0, "rk4", [], ur.to_struct(good), x0, P0, U, Y, DT, ctx=ctx)
    assert r["xf"].shape == (0, n, T, 12) and r["info"].shape == (0, n, 4)
    r = eng.ukf_filter(0, "rk4", _params(), ur.to_struct(good), x0[:0], P0[:0], U[:0], Y[:0], DT, ctx=ctx)
    assert r["xT"].shape == (P, 0, 12)
    info = np.full((P, n, 4), sentinel)
    for kw in (dict(P=0), dict(B=0)):
        ca = (_lib.BrovUkf * 1)(edited())
        rc = ctx.lib.brov_ukf_filter(ctx.h, 0, _lib.RK4, 0, kw.get("P", P), pa, 1, ca, kw.get("B", n), T, DT, x0.ctypes.data, P0.ctypes.data,
                                     U.ctypes.data, Y.ctypes.data, None, None, None, None, None, None, info.ctypes.data)
        assert rc == 0 and np.all(info == sentinel), kw


# ------------------------------------------------------------------------------------------ 7. host form = _dev form
def test_host_form_equals_dev_form(eng, ctx):
    from bluerov2_dynamics_amd import _lib
    name = "thr_rk4"
    i = uc.inputs(name)
    a = _run(eng, ctx, name)                                    # engine.ukf_filter on host arrays: uploads, then the _dev form
    n = i["B"]
    x0, P0, U, Y = (np.ascontiguousarray(i[k]) for k in ("x0", "P0", "U", "Y"))
    pa = (_lib.BrovParams * P)(*_params())
    ca = (_lib.BrovUkf * 1)(ur.to_struct(i["cfgs"]))
    outs = dict(lag=i["lag"].copy(), xf=np.empty((P, n, T, 12)), pstd=np.empty((P, n, T, 12)), innov=np.empty((P, n, T, 12)),
                xT=np.empty((P, n, 12)), PT=np.empty((P, n, 12, 12)), info=np.empty((P, n, 4)))
    rc = ctx.lib.brov_ukf_filter(ctx.h, 0, _lib.RK4, 0, P, pa, 1, ca, n, T, DT, x0.ctypes.data, P0.ctypes.data, U.ctypes.data, Y.ctypes.data,
                                 *(outs[k].ctypes.data for k in ("lag", "xf", "pstd", "innov", "xT", "PT", "info")))
    assert rc == 0, ctx.lib.brov_last_error(ctx.h)
    _same(a, outs)
    d = eng.ukf_filter(0, "rk4", _params(), ur.to_struct(i["cfgs"]), *(eng.DevArray.from_host(ctx, i[k]) for k in ("x0", "P0", "U", "Y")), DT,
                       lag=eng.DevArray.from_host(ctx, i["lag"]), ctx=ctx)
    assert isinstance(d["xf"], eng.DevArray)
    _same(a, {k: (None if v is None else v.numpy()) for k, v in d.items()})
    only = eng.ukf_filter(0, "rk4", _params(), ur.to_struct(i["cfgs"]), i["x0"], i["P0"], i["U"], i["Y"], DT, lag=i["lag"], want=("info",), ctx=ctx)
    assert only["xf"] is None and only["PT"] is None and np.array_equal(only["info"], a["info"])


# ------------------------------------------------------------------------------------------ 8. the vehicle classes
def test_vehicle_methods(eng):
    """rov.filter_states and rov.log_likelihood_population equal engine.ukf_filter on the same arguments (thruster and Euler-wrench
    vehicles), with the documented default start, and leave the object's lag state and parameters as they were"""
    from bluerov2_dynamics_amd.fossen.BlueROV2 import BlueROV2
    from bluerov2_dynamics_amd.fossen.BlueROV2_thrust import BlueROV2 as BlueROV2Wrench      # the Euler-angle wrench vehicle
    from bluerov2_dynamics_amd.fossen import estimate, identify
    for cls, name in ((BlueROV2, "thr_rk4"), (BlueROV2Wrench, "wr_rk4")):
        i = uc.inputs(name)
        cfg = ur.to_struct(i["cfgs"])
        rov = cls()
        own = identify.params_of(rov)
        before = ctypes.string_at(ctypes.byref(own), ctypes.sizeof(own))
        f = rov.filter_states(i["Y"], i["U"], DT, cfg, x0=i["x0"], P0=i["P0"], integrator="rk4")
        want = eng.ukf_filter(i["model"], "rk4", [own], cfg, i["x0"], i["P0"], i["U"], i["Y"], DT, ctx=rov._ctx)
        assert np.array_equal(f["x"], want["xf"][0], equal_nan=True) and np.array_equal(f["std"], want["pstd"][0], equal_nan=True)
        assert np.array_equal(f["innov"], want["innov"][0], equal_nan=True) and np.array_equal(f["PT"], want["PT"][0])
        assert np.array_equal(f["loglik"], want["info"][0, :, 0]) and np.all(f["failed_step"] == -1) and f["n_updates"].dtype == np.int64
        Y = i["Y"].copy()
        Y[:, 1] = np.where(np.isnan(Y[:, 1]), 0.1, Y[:, 1])            # row 1 is the first fully measured one
        dx0, dP0 = estimate.default_start(Y, cfg)
        assert np.array_equal(dx0[:, :7], Y[:, 1, :7]) and np.all(dx0[:, 7] == 0.0) and dP0[0, 7, 7] == estimate.P0_STAND_IN
        one = rov.filter_states(Y[0], i["U"][0], DT, cfg, params=fv.params("V5"), integrator="rk4")
        w1 = eng.ukf_filter(i["model"], "rk4", [fv.params("V5")], cfg, dx0[:1], dP0[:1], i["U"][:1], Y[:1], DT, ctx=rov._ctx)
        assert one["x"].shape == (T, 12) and np.array_equal(one["x"], w1["xf"][0, 0], equal_nan=True) and one["loglik"] == w1["info"][0, 0, 0]
        ll = rov.log_likelihood_population(_params(), i["Y"], i["U"], DT, cfg, x0=i["x0"], P0=i["P0"], integrator="rk4")
        w2 = eng.ukf_filter(i["model"], "rk4", _params(), cfg, i["x0"], i["P0"], i["U"], i["Y"], DT, ctx=rov._ctx)
        assert ll.shape == (P, i["B"]) and np.array_equal(ll, w2["info"][:, :, 0])
        own = identify.params_of(rov)
        assert ctypes.string_at(ctypes.byref(own), ctypes.sizeof(own)) == before


# ------------------------------------------------------------------------------------------ 9. the example
def test_example_runs_small():
    """examples/filter_recording.py in its small mode: the filter beats the raw rows and the true vehicle ranks first"""
    import importlib.util
    import os
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "filter_recording.py")
    spec = importlib.util.spec_from_file_location("filter_recording", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    out = mod.main(["--small"])
    assert out["x"].shape == (150, 12) and out["loglik"].shape == (8,) and np.all(np.isfinite(out["loglik"]))
    assert out["rmse_filtered"] < out["rmse_raw"] and 0.7 < out["nis"] < 1.3
    assert out["order"][0] == 0, "the true vehicle must rank first"
