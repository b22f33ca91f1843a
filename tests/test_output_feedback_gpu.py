"""The output-feedback closed loop (brov_output_feedback / engine.output_feedback / rov.simulate_output_feedback) on the GPU: the
unscented Kalman filter inside the rollout kernel, the feedback law on its estimate.

1. Exact identities, no tolerance.  Together they pin the loop by induction over t: the estimator is engine.ukf_filter on the rows
   (u, y) the kernel recorded; the plant is engine.rollout_pop on u; y = traj + V; the command is held; a call resumed from the
   checkpoint, two calls, and every problem alone give the same bits; a failing run fails alone with the NaN pattern of the header.
2. The law and the metrics, open loop on the kernel's own rows against long double at TOL_UPDATE = 1e-12 of the sum of |terms|.
3. End-to-end parity with tests/ukf_feedback_ref.py by the lane rule of tests/sweep_run.py at TOL_ROLL = 1e-10
   (tests/test_output_feedback_cpu.py checks the reference side of it without a GPU).
4. The host contract, the host form, the vehicle method, the example.
The cases and their shapes: tests/ukf_feedback_ref.py."""
import ctypes
import importlib.util
import os

import numpy as np
import pytest

import feedback_ref as fr
import fossen_vehicles as fv
import ukf_feedback_ref as ofr
import ukf_ref as ur
from oracle import fossen_params as fp

pytestmark = pytest.mark.gpu

L = np.longdouble
DT, TOL_ROLL, TOL_UPDATE, MARGIN = ofr.DT, ofr.TOL_ROLL, ofr.TOL_UPDATE, ofr.MARGIN
ROWS = ("traj", "y", "u", "xf", "pstd", "innov")                           # per-row outputs
CHECKPOINT = ("xT_true", "xT", "PT", "lag_est", "lag_plant", "z")
ALL = ROWS + CHECKPOINT + ("metrics", "info")
NAMES = tuple(ofr.CASES)
RESUMABLE = tuple(n for n in NAMES if ofr.case(n)["model"] == 1 or ofr.case(n)["banks"])      # (x, lag) is the whole checkpoint


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


def _args(name, **kw):
    i = ofr.inputs(name)
    a = dict(params=[fv.params(n) for n in i["models"]], plants=[fv.params(n) for n in i["plants"]], fb=[fr.to_struct(l) for l in i["laws"]],
             cfg=[ur.to_struct(k) for k in i["cfgs"]], lag=None if i["lag_est"] is None else (i["lag_est"], i["lag_plant"]))
    a.update({k: i[k] for k in ("x0_true", "x0_est", "P0", "V", "W", "u_ff", "ref", "z")})
    a.update(kw)
    return a


def _call(eng, ctx, name, **kw):
    c, a = ofr.case(name), _args(name, **kw)
    return eng.output_feedback(c["model"], c["integ"], a["params"], a["fb"], a["cfg"], a["x0_true"], a["x0_est"], a["P0"], a["V"], a["ref"], DT,
                               plant_params=a["plants"], W=a["W"], u_ff=a["u_ff"], lag=a["lag"], z=a["z"], lag_mode=c["lag_mode"], ctx=ctx)


_GOT = {}


def _got(eng, ctx, name):
    """the kernel's outputs on a case, computed once and left unchanged"""
    if name not in _GOT:
        _GOT[name] = _call(eng, ctx, name)
    return _GOT[name]


def _same(a, b, keys=ALL, what=""):
    for k in keys:
        if a[k] is None or b[k] is None:
            assert a[k] is None and b[k] is None, (what, k)
        else:
            assert np.array_equal(a[k], b[k], equal_nan=True), (what, k)


def _one(seq, j):
    return seq[j:j + 1] if len(seq) > 1 else seq


def _candidate(name, j, **kw):
    """the arguments of candidate j alone (P = 1)"""
    a = _args(name)
    lag = None if a["lag"] is None else (a["lag"][0][j:j + 1], a["lag"][1][j:j + 1])
    out = dict(params=a["params"][j:j + 1], plants=_one(a["plants"], j), fb=_one(a["fb"], j), cfg=_one(a["cfg"], j), lag=lag,
               z=None if a["z"] is None else a["z"][j:j + 1])
    out.update(kw)
    return out


# ------------------------------------------------------------------------------------------ 1. exact identities
@pytest.mark.parametrize("name", NAMES)
def test_estimator_is_the_filter(eng, ctx, name):
    """engine.ukf_filter under params[j] on (u[j], y[j]) from the same start returns the bits of xf, pstd, innov, xT, PT, the
    estimator's lag and all four entries of info: the log-likelihood is accumulated in the filter's order"""
    c, a, got = ofr.case(name), _args(name), _got(eng, ctx, name)
    assert np.array_equal(got["info"][..., 2], np.full((c["P"], c["B"]), -1.0)), "no run of a case fails"
    for j in range(c["P"]):
        lag = None if a["lag"] is None else a["lag"][0][j:j + 1]
        f = eng.ukf_filter(c["model"], c["integ"], a["params"][j:j + 1], _one(a["cfg"], j), a["x0_est"], a["P0"], got["u"][j], got["y"][j], DT,
                           lag=lag, lag_mode=c["lag_mode"], ctx=ctx)
        for k in ("xf", "pstd", "innov", "xT", "PT", "info"):
            assert np.array_equal(f[k][0], got[k][j], equal_nan=True), (name, j, k)
        if lag is not None:
            assert np.array_equal(f["lag"][0], got["lag_est"][j]), (name, j)
    assert (got["lag_est"] is None) == (a["lag"] is None) and (got["lag_plant"] is None) == (a["lag"] is None)


@pytest.mark.parametrize("name", [n for n in NAMES if not ofr.case(n)["W"]])
def test_plant_is_the_rollout(eng, ctx, name):
    """without W, engine.rollout_pop under the plant's parameters from x0_true on u[j] returns the bits of traj, xT_true and the
    plant's lag"""
    c, a, got = ofr.case(name), _args(name), _got(eng, ctx, name)
    for j in range(c["P"]):
        lag = None if a["lag"] is None else a["lag"][1][j:j + 1]
        r = eng.rollout_pop(c["model"], c["integ"], _one(a["plants"], j), a["x0_true"], got["u"][j], DT, lag=lag, lag_mode=c["lag_mode"], ctx=ctx)
        assert np.array_equal(r["traj"][0], got["traj"][j]) and np.array_equal(r["xT"][0], got["xT_true"][j]), (name, j)
        if lag is not None:
            assert np.array_equal(r["lag"][0], got["lag_plant"][j]), (name, j)


@pytest.mark.parametrize("name", NAMES)
def test_measurement_and_hold(eng, ctx, name):
    """y = traj[t] + V[t] bit for bit, NaN exactly where V is NaN; u[t] = u[t - t % hold] bit for bit, and the command changes at ticks"""
    c, a, got = ofr.case(name), _args(name), _got(eng, ctx, name)
    T, hold = c["T"], c["hold"]
    assert np.array_equal(got["y"], got["traj"][:, :, :T] + a["V"][None], equal_nan=True)
    assert np.array_equal(np.isnan(got["y"]), np.broadcast_to(np.isnan(a["V"]), got["y"].shape))
    t = np.arange(T)
    assert np.array_equal(got["u"], got["u"][:, :, t - t % hold])
    if T > hold:
        assert not np.array_equal(got["u"][:, :, 0], got["u"][:, :, hold])
    assert np.array_equal(got["traj"][:, :, 0], np.broadcast_to(a["x0_true"], got["traj"][:, :, 0].shape))


@pytest.mark.parametrize("name", RESUMABLE)
def test_resume(eng, ctx, name):
    """a call of T1 steps continued from the checkpoint gives the bits of the unbroken call in every per-row output and in the
    checkpoint, split at the first tick after the start (T1 = hold) and at the last tick; the metrics and the log-likelihood add up
    within TOL_UPDATE relative, the number of updates exactly"""
    c, a, got = ofr.case(name), _args(name), _got(eng, ctx, name)
    T, hold = c["T"], c["hold"]
    cut = lambda v, s: None if v is None else v[:, s]
    z0 = a["z"]
    if z0 is None:                           # z is part of the checkpoint: a start from zeros is the start without z, and returns it
        z0 = np.zeros((c["P"], c["B"], 6))
        full = _call(eng, ctx, name, z=z0)
        _same(full, got, tuple(k for k in ALL if k != "z"), name)
        got = full
    for T1 in sorted({hold, (T - 1) // hold * hold}):
        assert 0 < T1 < T
        head, tail = slice(0, T1), slice(T1, T)
        rows = (lambda s: a["ref"][:, s]) if c["moving"] else (lambda s: a["ref"])
        h = _call(eng, ctx, name, z=z0, V=a["V"][:, head], W=cut(a["W"], head), u_ff=cut(a["u_ff"], head), ref=rows(head))
        parts = []
        for j in range(c["P"]):              # the start is shared by the candidates and the checkpoint is not: resume one by one
            lag = None if h["lag_est"] is None else (h["lag_est"][j:j + 1], h["lag_plant"][j:j + 1])
            parts.append(_call(eng, ctx, name, **_candidate(name, j, x0_true=h["xT_true"][j], x0_est=h["xT"][j], P0=h["PT"][j], lag=lag,
                                                              z=h["z"][j:j + 1], V=a["V"][:, tail], W=cut(a["W"], tail),
                                                              u_ff=cut(a["u_ff"], tail), ref=rows(tail))))
        second = {k: (None if parts[0][k] is None else np.concatenate([p[k] for p in parts])) for k in ALL}
        assert np.array_equal(second["traj"][:, :, 0], h["traj"][:, :, -1]), "the second call's row 0 repeats the first call's last"
        for k in ROWS:
            both = np.concatenate([h[k], second[k][:, :, 1:] if k == "traj" else second[k]], axis=2)
            assert np.array_equal(both, got[k], equal_nan=True), (name, T1, k)
        _same(second, got, CHECKPOINT, (name, T1))
        m = h["metrics"] + second["metrics"]
        assert np.max(np.abs(m - got["metrics"]) / np.maximum(np.abs(got["metrics"]), 1e-300)) < TOL_UPDATE, (name, T1)
        assert np.array_equal(m[..., 3], got["metrics"][..., 3])
        ll = h["info"][..., 0] + second["info"][..., 0]
        assert np.max(np.abs(ll - got["info"][..., 0]) / np.abs(got["info"][..., 0])) < TOL_UPDATE, (name, T1)
        assert np.array_equal(h["info"][..., 1] + second["info"][..., 1], got["info"][..., 1])


@pytest.mark.parametrize("name", ["thr_rk4", "wr_rk4"])
def test_determinism_and_problems_alone(eng, ctx, name):
    """two calls give the same bits; every (candidate, run) alone as P = B = 1 gives the bits it has in the batch"""
    c, a, got = ofr.case(name), _args(name), _got(eng, ctx, name)
    _same(_call(eng, ctx, name), got, what=name)
    cut = lambda v, b: None if v is None else v[b:b + 1]
    for j in range(c["P"]):
        for b in range(c["B"]):
            k1 = _candidate(name, j)
            lag = None if k1["lag"] is None else (k1["lag"][0][:, b:b + 1], k1["lag"][1][:, b:b + 1])
            one = _call(eng, ctx, name, **dict(k1, lag=lag, z=None if k1["z"] is None else k1["z"][:, b:b + 1],
                                               **{k: cut(a[k], b) for k in ("x0_true", "x0_est", "P0", "V", "W", "u_ff", "ref")}))
            for k in ALL:
                if got[k] is not None:
                    assert np.array_equal(one[k][0, 0], got[k][j, b], equal_nan=True), (name, j, b, k)


@pytest.mark.parametrize("stage", [1, 2])
@pytest.mark.parametrize("name", ["thr_rk4", "wr_euler"])
def test_failing_run_fails_alone(eng, ctx, name, stage):
    """run 1 starts from a covariance that is not positive definite: a numerical condition handled in the kernel.  Stage 1: P0[0][0] < 0
    with component 0 measured at row 0, so s <= 0 there.  Stage 2: P0[0][1] = P0[1][0] = 2 P0[0][0] with nothing measured at row 0, so
    the Cholesky factorisation of row 0 meets a negative pivot argument.  The run shows the NaN pattern of the header and leaves its
    lag banks and z as they came; every other run keeps the bits of the call without it."""
    c, a, got = ofr.case(name), _args(name), _got(eng, ctx, name)
    T = c["T"]
    P0, V = a["P0"].copy(), a["V"].copy()
    if stage == 1:
        P0[1, 0, 0] = -1.0
        V[1, 0, 0] = 0.01
    else:
        P0[1, 1, 0] = P0[1, 0, 1] = 2.0 * P0[1, 0, 0]
        V[1, 0, :] = np.nan
    f = _call(eng, ctx, name, P0=P0, V=V)
    o = ofr.run_reference(ofr.inputs(name), P0=P0, V=V)
    n = 0 if stage == 1 else 1                                # the first NaN row of xf, pstd, innov and u; traj from n + 1, y from 1
    for j in range(c["P"]):
        assert f["info"][j, 1, 0] == -np.inf and f["info"][j, 1, 2] == 0 and f["info"][j, 1, 1] == o["info"][j, 1, 1], (j, f["info"][j, 1])
        for k in ("xf", "pstd", "innov", "u"):
            assert np.isnan(f[k][j, 1, n:]).all(), k
        assert np.isnan(f["traj"][j, 1, n + 1:]).all() and np.isfinite(f["traj"][j, 1, :n + 1]).all()
        assert np.isnan(f["y"][j, 1, 1:]).all() and np.array_equal(np.isnan(f["y"][j, 1, 0]), np.isnan(V[1, 0]))
        if stage == 2:                                        # row 0 was complete: the estimate no measurement touched, a command, a plant step
            assert np.array_equal(f["xf"][j, 1, 0], a["x0_est"][1]) and np.isfinite(f["u"][j, 1, 0]).all()
            assert np.isnan(f["innov"][j, 1, 0]).all() and np.isfinite(f["pstd"][j, 1, 0]).all()
        for k in ("xT_true", "xT", "PT", "metrics"):
            assert np.isnan(f[k][j, 1]).all(), k
        for k, src in (("lag_est", None if a["lag"] is None else a["lag"][0]), ("lag_plant", None if a["lag"] is None else a["lag"][1]), ("z", a["z"])):
            if src is not None:
                assert np.array_equal(f[k][j, 1], src[j, 1]), k
        for k in ALL:                                         # the reference states the same pattern
            if f[k] is not None and k not in ("info",):
                assert np.array_equal(np.isnan(f[k][j, 1]), np.isnan(o[k][j, 1])), (k, j)
    others = [b for b in range(c["B"]) if b != 1]
    for k in ALL:
        if f[k] is not None:
            assert np.array_equal(f[k][:, others], got[k][:, others], equal_nan=True), k


# ------------------------------------------------------------------------------------------ 2. the law and the metrics
def _law_ld(name, j, xf, ref, u_ff, z0):
    """the law of the header in long double on rows xf [T,12] of candidate j: (u [T,nu], sum of |terms| [T,nu])"""
    i, c = ofr.inputs(name), ofr.case(name)
    law = i["laws"][j if len(i["laws"]) > 1 else 0]
    nu, T = fp.NU[c["model"]], xf.shape[0]
    K, Ki, lo, hi, zm = (np.asarray(v, dtype=L) for v in (law.K, law.Ki, law.u_min, law.u_max, law.z_max))
    z = np.asarray(z0, dtype=L).copy()
    u, size = np.zeros((T, nu), dtype=L), np.zeros((T, nu), dtype=L)
    for t in range(T):
        if t % law.hold == 0:
            e, _ = fr.error(c["model"], xf[t][None], ref[t if ref.shape[0] > 1 else 0][None], L)
            e = e[0]
            ff = np.zeros(nu, dtype=L) if u_ff is None else np.asarray(u_ff[t], dtype=L)
            raw = ff + K @ e + Ki @ z
            held = np.minimum(np.maximum(raw, lo), hi)
            scale = np.abs(ff) + np.abs(K) @ np.abs(e) + np.abs(Ki) @ np.abs(z)
            z = np.minimum(np.maximum(z + L(law.hold) * L(DT) * e[:6], -zm), zm)
        u[t], size[t] = held, scale
    return u, size


@pytest.mark.parametrize("name", NAMES)
def test_law_on_the_kernels_own_rows(eng, ctx, name):
    """u against the law in long double on the kernel's xf, the reference rows and z rebuilt by the recurrence from the same xf:
    |err| / sum |terms| < TOL_UPDATE.  Open loop: nothing amplifies.  (profiles/output_feedback_checks.md records the worst value.)"""
    c, a, got = ofr.case(name), _args(name), _got(eng, ctx, name)
    worst = 0.0
    for j in range(c["P"]):
        for b in range(c["B"]):
            z0 = np.zeros(6) if a["z"] is None else a["z"][j, b]
            u, size = _law_ld(name, j, got["xf"][j, b], a["ref"][b], None if a["u_ff"] is None else a["u_ff"][b], z0)
            worst = max(worst, float(np.max(np.abs(got["u"][j, b].astype(L) - u) / size)))
    print(f"{name}: law worst |err| / sum |terms| = {worst:.2e}  bound {TOL_UPDATE:.0e}")
    assert worst < TOL_UPDATE


@pytest.mark.parametrize("name", NAMES)
def test_metrics_and_saturation_count(eng, ctx, name):
    """entries 0 .. 6 rebuilt in long double from the kernel's traj, xf, u and the reference rows, relative to TOL_UPDATE; the count
    of saturated steps equals the count on the kernel's own u, and the reference's on the runs whose saturation margin exceeds MARGIN"""
    c, a, got = ofr.case(name), _args(name), _got(eng, ctx, name)
    i, o = ofr.inputs(name), ofr.reference(name)
    T, h = c["T"], L(DT)
    worst = 0.0
    for j in range(c["P"]):
        law = i["laws"][j if len(i["laws"]) > 1 else 0]
        for b in range(c["B"]):
            ref = a["ref"][b] if c["moving"] else np.repeat(a["ref"][b], T, axis=0)
            e, _ = fr.error(c["model"], got["traj"][j, b, :T], ref, L)
            u, d = got["u"][j, b].astype(L), got["xf"][j, b].astype(L) - got["traj"][j, b, :T].astype(L)
            d[:, 3:6] = ur._wrap(d[:, 3:6], L)[0]
            m = np.array([h * np.sum(e[:, 0:3] ** 2), h * np.sum(e[:, 3:6] ** 2), h * np.sum(u ** 2),
                          np.sum(np.any((got["u"][j, b] == law.u_min) | (got["u"][j, b] == law.u_max), axis=1)),
                          h * np.sum(d[:, 0:3] ** 2), h * np.sum(d[:, 3:6] ** 2), h * np.sum(d[:, 6:12] ** 2)], dtype=L)
            assert got["metrics"][j, b, 3] == m[3], (name, j, b)
            worst = max(worst, float(np.max(np.abs(got["metrics"][j, b].astype(L) - m) / np.abs(m)[[0, 1, 2, 0, 4, 5, 6]])))
    print(f"{name}: metrics worst relative error = {worst:.2e}  bound {TOL_UPDATE:.0e}")
    assert worst < TOL_UPDATE
    ok = o["sat_margin"] > MARGIN
    assert np.array_equal(got["metrics"][..., 3][ok], o["metrics"][..., 3][ok])


# ------------------------------------------------------------------------------------------ 3. end-to-end parity
@pytest.mark.parametrize("name", NAMES)
def test_parity(eng, ctx, name):
    """every output against tests/ukf_feedback_ref.py in float64 on the compared lanes: the mixed error against TOL_ROLL, the
    covariance measure for PT, the counts exact"""
    got, o = _got(eng, ctx, name), ofr.reference(name)
    keep, gaps = ofr.compared(name)
    assert keep.sum() >= 0.75 * keep.size and gaps[keep].max() < 0.1 * TOL_ROLL
    have = dict(got)
    for k in ("lag_est", "lag_plant", "z"):                   # what the call does not return, the reference carries from zero
        if have[k] is None:
            have[k] = o[k]
    e = ofr.lane_gaps(have, o)
    print(f"{name}: kernel err {e[keep].max():.2e}  reference fp64-vs-long-double gap {gaps[keep].max():.2e}  bound {TOL_ROLL:.0e}  "
          f"lanes compared {int(keep.sum())} of {keep.size}")
    assert e[keep].max() < TOL_ROLL
    assert np.array_equal(got["info"][..., 1:3][keep], o["info"][..., 1:3][keep])
    assert np.array_equal(got["metrics"][..., 3][keep], o["metrics"][..., 3][keep])
    for j in range(got["PT"].shape[0]):
        for b in range(got["PT"].shape[1]):
            assert np.array_equal(got["PT"][j, b], got["PT"][j, b].T), "PT must be bit-symmetric"


# ------------------------------------------------------------------------------------------ 4. the contract, the forms
def _host_call(ctx, name, a, P, B, T, outs, ref_rows=None, lag=True, nplant=None):
    """brov_output_feedback (the host form) on host arrays; outs: name -> array or None"""
    from bluerov2_dynamics_amd import _lib
    c = ofr.case(name)
    arr = lambda t, seq: (t * len(seq))(*seq)
    ptr = lambda v: None if v is None else v.ctypes.data
    pa, pl = arr(_lib.BrovParams, a["params"]), arr(_lib.BrovParams, a["plants"])
    fa, ca = arr(_lib.BrovFeedback, a["fb"]), arr(_lib.BrovUkf, a["cfg"])
    keep = [np.ascontiguousarray(a[k]) if a[k] is not None else None for k in ("x0_true", "x0_est", "P0", "V", "W", "u_ff", "ref")]
    rc = ctx.lib.brov_output_feedback(ctx.h, c["model"], ofr.INTEG[c["integ"]], c["lag_mode"], P, pa, len(a["plants"]) if nplant is None else nplant,
                                      pl, len(a["fb"]), fa, len(a["cfg"]), ca, B, T, DT, *(ptr(v) for v in keep),
                                      a["ref"].shape[1] if ref_rows is None else ref_rows,
                                      *(ptr(outs.get(k)) for k in ("lag_est", "lag_plant", "z", "traj", "y", "u", "xf", "pstd", "innov", "xT_true",
                                                                    "xT", "PT", "metrics", "info")))
    return rc, ctx.lib.brov_last_error(ctx.h)


def test_host_contract(eng, ctx):
    """every rule of the header returns BROV_ERR_ARG with a brov_last_error text that names the call, and no output is written"""
    from bluerov2_dynamics_amd import _lib
    name = "thr_rk4"
    c, good, i = ofr.case(name), _args(name), ofr.inputs(name)
    P, B, T = c["P"], c["B"], c["T"]
    law, k0 = i["laws"][0], i["cfgs"][0]

    def fb(hold=None, **edits):
        l = fr.Law(law.K.copy(), law.Ki.copy(), law.u_min.copy(), law.u_max.copy(), law.z_max.copy(), law.hold if hold is None else hold)
        for field, (idx, v) in edits.items():
            getattr(l, field)[idx] = v
        return fr.to_struct(l)

    def cfg(**kw):
        d = dict(q=k0.q.copy(), r=k0.r.copy(), alpha=k0.alpha, beta=k0.beta, kappa=k0.kappa)
        for key, v in kw.items():
            if isinstance(v, tuple):
                d[key][v[0]] = v[1]
            else:
                d[key] = v
        s = _lib.BrovUkf()
        for n in range(12):
            s.q[n], s.r[n] = d["q"][n], d["r"][n]
        s.alpha, s.beta, s.kappa = d["alpha"], d["beta"], d["kappa"]
        return s
    singular = fv.params("V0")
    singular.m = singular.added_mass[0]              # m - added_mass[0] = 0: a singular mass matrix
    cases = [("hold < 1", dict(fb=[fb(hold=0)]), {}),
             ("nfb not in {1, P}", dict(fb=[fb()] * 2), {}),
             ("ref_rows not in {1, T}", {}, dict(ref_rows=T - 1)),
             ("u_min > u_max", dict(fb=[fb(u_min=(2, 0.7), u_max=(2, 0.6))]), {}),
             ("negative z_max", dict(fb=[fb(z_max=(5, -1e-3))]), {}),
             ("NaN in K", dict(fb=[fb(K=((7, 11), np.nan))]), {}),
             ("nrec not in {1, P}", dict(cfg=[cfg()] * 2), {}),
             ("alpha <= 0", dict(cfg=[cfg(alpha=0.0)]), {}),
             ("alpha not finite", dict(cfg=[cfg(alpha=np.inf)]), {}),
             ("n + lambda <= 0", dict(cfg=[cfg(kappa=-12.0)]), {}),
             ("negative q", dict(cfg=[cfg(q=(3, -1e-9))]), {}),
             ("infinite q", dict(cfg=[cfg(q=(3, np.inf))]), {}),
             ("NaN r", dict(cfg=[cfg(r=(0, np.nan))]), {}),
             ("nplant not in {1, P}", dict(plants=good["plants"][:2]), {}),
             ("one lag bank without the other", {}, dict(lag=False)),
             ("T < 1", {}, dict(T=0)),
             ("P > 65535", {}, dict(P=65536)),
             ("the quaternion model", {}, dict(model=_lib.WRENCH_QUAT)),
             ("a double-integrator model", {}, dict(model=_lib.DI_THRUSTER_EULER)),
             ("dt not > 0", {}, dict(dt=0.0)),
             ("a singular plant", dict(plants=[singular] * P), {}),
             ("NULL V", dict(V=None), {})]
    sentinel = 7.25
    for what, kw, how in cases:
        a = dict(good, **kw)
        outs = dict(traj=np.full((P, B, T + 1, 12), sentinel), y=np.full((P, B, T, 12), sentinel), u=np.full((P, B, T, 8), sentinel),
                    xf=np.full((P, B, T, 12), sentinel), pstd=np.full((P, B, T, 12), sentinel), innov=np.full((P, B, T, 12), sentinel),
                    xT_true=np.full((P, B, 12), sentinel), xT=np.full((P, B, 12), sentinel), PT=np.full((P, B, 12, 12), sentinel),
                    metrics=np.full((P, B, 7), sentinel), info=np.full((P, B, 4), sentinel), lag_est=np.full((P, B, 8, 3), sentinel),
                    lag_plant=np.full((P, B, 8, 3), sentinel), z=np.full((P, B, 6), sentinel))
        passed = dict(outs)
        if how.get("lag") is False:
            passed["lag_plant"] = None
        if "model" in how or "dt" in how:
            arr = lambda t, seq: (t * len(seq))(*seq)
            ptr = lambda v: None if v is None else np.ascontiguousarray(v).ctypes.data
            ins = [np.ascontiguousarray(a[k]) for k in ("x0_true", "x0_est", "P0", "V")] + [None, np.ascontiguousarray(a["u_ff"]), np.ascontiguousarray(a["ref"])]
            rc = ctx.lib.brov_output_feedback(ctx.h, how.get("model", 0), _lib.RK4, 0, P, arr(_lib.BrovParams, a["params"]), len(a["plants"]),
                                              arr(_lib.BrovParams, a["plants"]), 1, arr(_lib.BrovFeedback, a["fb"]), 1, arr(_lib.BrovUkf, a["cfg"]),
                                              B, T, how.get("dt", DT), *(None if v is None else v.ctypes.data for v in ins), T,
                                              *(passed[k].ctypes.data for k in ("lag_est", "lag_plant", "z", "traj", "y", "u", "xf", "pstd", "innov",
                                                                                "xT_true", "xT", "PT", "metrics", "info")))
            msg = ctx.lib.brov_last_error(ctx.h)
        else:
            rc, msg = _host_call(ctx, name, a, how.get("P", P), B, how.get("T", T), passed, ref_rows=how.get("ref_rows"))
        print(what, "->", rc, msg)
        # the rules of the call itself name it; dt and the mass matrix are refused by the derivation every population call shares
        want = {"dt not > 0": b"dt must be finite and > 0", "a singular plant": b"singular mass matrix"}.get(what, b"brov_output_feedback: ")
        assert rc == -1 and want in msg and len(msg) > len(b"brov_output_feedback: "), what
        assert all(np.all(v == sentinel) for v in outs.values()), what
    with pytest.raises(_lib.BrovError, match=r"BROV_ERR_ARG: brov_output_feedback: fb\[0\]: hold must be >= 1"):
        _call(eng, ctx, name, fb=[fb(hold=0)])                                        # through the engine: the library's text in the exception
    with pytest.raises(AssertionError, match="plant_params must be one"):
        _call(eng, ctx, name, plants=good["plants"][:2])                              # what the engine can see itself it refuses itself
    r = _call(eng, ctx, name, params=[], plants=good["plants"][:1], lag=None, z=None)  # P = 0: nothing to do
    assert r["xT"].shape == (0, B, 12)


@pytest.mark.parametrize("name", ["thr_rk4", "wr_rk4"])
def test_host_form_equals_dev_form(eng, ctx, name):
    """brov_output_feedback on host arrays returns the bits of brov_output_feedback_dev through the engine, lag banks and z in place"""
    c, a, got = ofr.case(name), _args(name), _got(eng, ctx, name)
    P, B, T, nu = c["P"], c["B"], c["T"], fp.NU[c["model"]]
    shapes = dict(traj=(P, B, T + 1, 12), y=(P, B, T, 12), u=(P, B, T, nu), xf=(P, B, T, 12), pstd=(P, B, T, 12), innov=(P, B, T, 12),
                  xT_true=(P, B, 12), xT=(P, B, 12), PT=(P, B, 12, 12), metrics=(P, B, 7), info=(P, B, 4))
    outs = {k: np.zeros(s) for k, s in shapes.items()}
    outs["z"] = None if a["z"] is None else a["z"].copy()
    outs["lag_est"], outs["lag_plant"] = (None, None) if a["lag"] is None else (a["lag"][0].copy(), a["lag"][1].copy())
    rc, msg = _host_call(ctx, name, a, P, B, T, outs)
    assert rc == 0, msg
    _same(outs, got, what=name)


def test_dev_arrays_in_dev_arrays_out(eng, ctx):
    name = "wr_euler"
    a, got = _args(name), _got(eng, ctx, name)
    dev = {k: (None if a[k] is None else eng.DevArray.from_host(ctx, a[k])) for k in ("x0_true", "x0_est", "P0", "V", "W", "u_ff", "ref")}
    d = _call(eng, ctx, name, **dev)
    assert isinstance(d["traj"], eng.DevArray)
    for k in ALL:
        if got[k] is not None:
            assert np.array_equal(d[k].numpy(), got[k], equal_nan=True), k


def test_vehicle_method(eng):
    """rov.simulate_output_feedback, one vehicle and with params_list, equals engine.output_feedback on the same arguments and leaves
    the object's lag state as it was"""
    from bluerov2_dynamics_amd.fossen.BlueROV2 import BlueROV2
    from bluerov2_dynamics_amd.fossen import control, estimate, identify
    rov = BlueROV2()
    rov.simulate(np.zeros(12), np.full((5, 8), 0.1), DT, integrator="rk4")            # a non-zero lag state of its own
    lag_before = np.array(rov._lag)
    T = 12
    x0, ref = np.zeros(12), np.zeros(12)
    x0[2], ref[2], ref[5] = 5.0, 5.2, 0.3
    cfg = estimate.ukf(q=1e-6, r=ofr.SIGMA ** 2)
    V = estimate.measurement_noise(cfg, (T,), dropout=0.2, never=(7,), seed=3)
    fb = control.pid_thrusters(rov, [4.0, 4.0, 6.0, 0.5, 0.5, 1.0], [2.0, 2.0, 3.0, 0.2, 0.2, 0.4], 0.5, z_max=0.2, hold=2)
    got = rov.simulate_output_feedback(x0, ref, DT, fb, cfg, V, integrator="rk4")
    P0 = np.diag(4.0 * ofr.SIGMA ** 2)
    me = identify.params_of(rov)
    want = eng.output_feedback(0, "rk4", [me], fb, cfg, x0[None], x0[None], P0[None], V[None], ref[None, None], DT, plant_params=me, ctx=rov._ctx)
    assert got["traj"].shape == (T + 1, 12) and got["u"].shape == (T, 8) and got["metrics"].shape == (7,) and got["failed_step"] == -1
    for k, w in (("traj", "traj"), ("y", "y"), ("u", "u"), ("x", "xf"), ("std", "pstd"), ("innov", "innov"), ("metrics", "metrics")):
        assert np.array_equal(got[k], want[w][0, 0], equal_nan=True), k
    assert np.isnan(got["y"][:, 7]).all() and np.isfinite(got["x"]).all()
    ps = [fv.params(n) for n in ("V0", "V2", "V5")]
    gotP = rov.simulate_output_feedback(x0, ref, DT, fb, cfg, V, T=T, params_list=ps, integrator="rk4")
    wantP = eng.output_feedback(0, "rk4", ps, fb, cfg, x0[None], x0[None], P0[None], V[None], ref[None, None], DT, plant_params=me, ctx=rov._ctx)
    assert gotP["traj"].shape == (3, T + 1, 12) and np.array_equal(gotP["traj"], wantP["traj"][:, 0])
    assert np.array_equal(gotP["x"], wantP["xf"][:, 0]) and not np.array_equal(gotP["x"][0], gotP["x"][1])
    assert np.array_equal(rov._lag, lag_before)
    with pytest.raises(ValueError):
        rov.simulate_output_feedback(x0, ref, DT, fb, cfg, V, T=T + 1)


def test_example_runs_small():
    """examples/output_feedback_ensemble.py --small: the same gains with the true state and with the estimate fed back"""
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "output_feedback_ensemble.py")
    spec = importlib.util.spec_from_file_location("output_feedback_ensemble", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    out = mod.run(small=True, verbose=False)
    P, T = out["P"], out["T"]
    assert out["state_feedback"]["metrics"].shape == (P, 4) and out["output_feedback"]["metrics"].shape == (P, 7)
    assert out["output_feedback"]["traj"].shape == (P, T + 1, 12) and np.all(out["output_feedback"]["failed_step"] == -1)
    assert np.all(np.isfinite(out["output_feedback"]["metrics"])) and np.all(out["output_feedback"]["metrics"][:, 4:] > 0)
    assert np.isnan(out["output_feedback"]["y"][:, :, 2]).any(), "the depth channel must drop out"
    assert np.isnan(out["output_feedback"]["y"][:, :, 6:9]).all(), "the linear velocity is never measured"
