"""The model-predictive update planned with an EDMDc model (edmdc_mppi_step / engine.koopman_mppi_step / simulate_mppi(planner=))
on the GPU against tests/koopman_mppi_ref.py, the NumPy restatement of the law of include/brov2.h whose predictions come from the
ITERATED recursion z <- A z + B v (the kernel evaluates the linear form).

Recipe of tests/test_mppi_gpu.py: the mixed error max |a-b| / max(1,|b|) formed in long double against TOL_ROLL = 1e-10; every
comparison also runs the reference in np.longdouble and asserts that fp64 and long double stay within a tenth of the bound, and that
the wrap margin of feedback_ref.error exceeds 1e-6.  The seeds are chosen so that this holds (checked on the CPU).

Shapes, the smallest that can still go wrong: B = 3 problems; K = 96 samples (two waves, dead lanes in the second); H = 7 at hold = 3,
so M = 3 knots and the last covers one step; ref_total = 12 with ref_row0 = 2; limits that a few per cent of the sample commands
reach (asserted on the reference); one channel with sigma = 0.  Models: tests/golden/edmdc.npz (d = 60) and simscript.npz (d = 72)
with n = 12, r = 8; the ill-conditioned edmdc_fit.npz small_* (d = 212) at H = 20; seeded synthetic models for the other
instantiations of the kernel: (n, r, k) = (13, 6, 20), (12, 6, 0) -- a purely linear model -- and (13, 8, 5)."""
import ctypes
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import fossen_vehicles as fv
import koopman_mppi_ref as kr
import mppi_ref as mr
from conftest import REPO, load_golden

pytestmark = pytest.mark.gpu

TOL_ROLL = 1e-10
MARGIN = 1e-6
L = np.longdouble
B, K, H, HOLD, DT = 3, 96, 7, 3, 0.05
M, REF_TOTAL, ROW0 = 3, 12, 2
SEED_X = 7301                              # chosen so that the margins below hold for every case of this file (checked on the CPU)
SYNTH = {"quat": (13, 6, 20), "lin": (12, 6, 0), "quat8": (13, 8, 5)}


def err(a, b):
    """max |a-b| / max(1, |b|), formed in long double"""
    a, b = np.asarray(a, dtype=L), np.asarray(b, dtype=L)
    return float(np.max(np.abs(a - b) / np.maximum(L(1), np.abs(b)))) if a.size else 0.0


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


# ------------------------------------------------------------------------------------------ shared models, inputs, records, references
@functools.lru_cache(maxsize=None)
def model(name):
    """(C [k,n] | None, gamma, A, B, X | None): a fixture model with the recording its states come from, or a seeded synthetic one:
    A = 0.98 A0 / rho(A0) with A0 = I + 0.3 G / sqrt(d) (spectral radius 0.98, predictions that stay near the start state, so a
    predicted quaternion keeps a norm near 1), B and the centres of the size of the states"""
    if name == "edmdc":
        g = load_golden("edmdc.npz")
        return g["centers"], float(g["gamma"]), g["A"], g["B"], g["X"]
    if name == "simscript":
        g = load_golden("simscript.npz")
        return g["centers"], 1.0, g["A"], g["B"], g["X"]
    if name == "small":
        g = load_golden("edmdc_fit.npz")
        return g["small_centers"], 1.0, g["small_A"], g["small_B"], load_golden("edmdc.npz")["X"]
    n, r, k = SYNTH[name]
    rng = np.random.default_rng(SEED_X + 10 * n + r + k)
    d = n + k
    A0 = np.eye(d) + 0.3 * rng.normal(size=(d, d)) / np.sqrt(d)
    A = 0.98 * A0 / np.max(np.abs(np.linalg.eigvals(A0)))
    return (rng.uniform(-0.5, 0.5, (k, n)) if k else None), 0.5, A, 0.1 * rng.normal(size=(d, r)), None


def dims(name):
    C, _, A, Bm, _ = model(name)
    k = 0 if C is None else C.shape[0]
    return A.shape[0] - k, Bm.shape[1], k


@functools.lru_cache(maxsize=None)
def inputs(name, nb=B, h=H, hold=HOLD, ref_total=REF_TOTAL):
    """x [nb,n], ref [nb,ref_total,n] (rows of the recording, or +-0.5 with unit quaternions), knots U [nb,m,r], eps [nb,K,m,r]"""
    n, r, _ = dims(name)
    X = model(name)[4]
    rng = np.random.default_rng(SEED_X + len(name) + 7 * h)
    m = mr.knots(h, hold)
    if X is not None:
        x = X[rng.choice(len(X), nb, replace=False)]
        ref = np.stack([X[i:i + ref_total] for i in rng.choice(len(X) - ref_total, nb, replace=False)])
    else:
        x, ref = rng.uniform(-0.5, 0.5, (nb, n)), rng.uniform(-0.5, 0.5, (nb, ref_total, n))
        if n == 13:
            x[:, 3:7] /= np.linalg.norm(x[:, 3:7], axis=1, keepdims=True)
            ref[:, :, 3:7] /= np.linalg.norm(ref[:, :, 3:7], axis=2, keepdims=True)
    U = rng.uniform(-0.3, 0.3, (nb, m, r))
    eps = rng.normal(size=(nb, K, m, r))
    return np.ascontiguousarray(x), np.ascontiguousarray(ref), U, eps


@functools.lru_cache(maxsize=None)
def record(r, lam=1.0, plain=False, hold=HOLD):
    """random weights, gamma = 1 whatever the temperature; sigma 0.2 with channel 2 unperturbed; per-channel limits 0.5 .. 0.8, which lie in the tails of the sample
    commands.  plain: q = qf = 0, gamma = 0, no limits (the cost reads the noise out directly)."""
    rng = np.random.default_rng(SEED_X + 90 + r)
    sigma = np.full(r, 0.2)
    sigma[2] = 0.0
    q, qf, rr = rng.uniform(0.5, 2.0, 12), rng.uniform(2.0, 8.0, 12), rng.uniform(0.05, 0.2, r)
    if plain:
        return mr.cfg(r, q=0.0, qf=0.0, r=rr, sigma=sigma, lam=lam, gamma=0.0, hold=hold)
    return mr.cfg(r, q=q, qf=qf, r=rr, sigma=sigma, lam=lam, gamma=1.0, u_min=-np.linspace(0.8, 0.5, r), u_max=np.linspace(0.5, 0.8, r),
                  hold=hold)


def _case(name, setpoint, nb, h, hold):
    x, ref, U, eps = inputs(name, nb, h, hold, 1 if setpoint else REF_TOTAL)
    return x, ref, U, eps, 0 if setpoint else ROW0


@functools.lru_cache(maxsize=None)
def reference(name, ld=False, lam=1.0, setpoint=False, k=K, shift=False, seed=None, plain=False, nb=B, h=H, hold=HOLD):
    """koopman_mppi_ref.step on inputs(name); setpoint: ref_total = 1; seed: the seeded stream instead of the explicit eps"""
    C, gamma, A, Bm, _ = model(name)
    x, ref, U, eps, row0 = _case(name, setpoint, nb, h, hold)
    return kr.step(C, gamma, A, Bm, record(dims(name)[1], lam, plain, hold), x, ref, U, DT, k, h, seed=seed or 0,
                   eps=None if seed is not None else eps[:, :k], ref_row0=row0, shift=shift, dtype=L if ld else np.float64)


def _run(eng, ctx, name, lam=1.0, setpoint=False, k=K, shift=False, seed=None, plain=False, eps=None, x=None, nb=B, h=H, hold=HOLD, **kw):
    C, gamma, A, Bm, _ = model(name)
    X, ref, U, e, row0 = _case(name, setpoint, nb, h, hold)
    if seed is None and eps is None:
        eps = e[:, :k]
    kw.setdefault("want_pred", True)
    return eng.koopman_mppi_step(C, gamma, A, Bm, mr.to_struct(record(dims(name)[1], lam, plain, hold)), X if x is None else x, ref, U, DT, k,
                                 H=h, seed=seed or 0, eps=eps, ref_row0=row0, shift=shift, want_cost=True, ctx=ctx, **kw)


def _limits_reached(name, o):
    c = record(dims(name)[1])
    on = (o["v"] == c.u_min) | (o["v"] == c.u_max)
    frac = on[:, 1:][..., c.sigma > 0].mean()
    assert 0.01 < frac < 0.2, ("a few per cent of the sample commands must reach a limit", frac)


def _check(what, got, name, **kw):
    """pred and cost of a run against the reference in float64, with the reference's own gap to long double and its wrap margin"""
    o, ol = reference(name, **kw), reference(name, ld=True, **kw)
    assert min(o["wrap_margin"], ol["wrap_margin"]) > MARGIN, o["wrap_margin"]
    assert got["cost"].shape == o["cost"].shape and np.all(np.isfinite(got["cost"]))
    if got.get("pred") is not None:
        assert got["pred"].shape == o["pred"].shape
        report(what + ", pred", err(got["pred"], o["pred"]), err(o["pred"], ol["pred"]), TOL_ROLL)
    report(what + ", cost", err(got["cost"], o["cost"]), err(o["cost"], ol["cost"]), TOL_ROLL)
    return o


# ------------------------------------------------------------------------------------------ 1. pred and cost
@pytest.mark.parametrize("name", ["edmdc", "simscript"])
def test_pred_and_cost(eng, ctx, name):
    """the reference window at ROW0, explicit eps, limits reached: pred [B,K,H+1,n] and cost [B,K] against the iterated recursion"""
    r = _run(eng, ctx, name)
    assert r["cost"].shape == (B, K) and r["pred"].shape == (B, K, H + 1, 12) and r["U_nom"].shape == (B, M, 8)
    assert r["u_apply"].shape == (B, HOLD, 8) and r["info"].shape == (B, 4)
    o = _check(f"koopman mppi {name}", r, name)
    _limits_reached(name, o)
    assert np.array_equal(r["pred"][:, :, 0], np.repeat(inputs(name)[0][:, None], K, axis=1)), "row 0 of pred is the state itself"
    assert not np.array_equal(r["pred"][:, 1, 1], r["pred"][:, 2, 1]), "every sample has its own prediction"


def test_set_point(eng, ctx):
    """ref_total = 1: every step is scored against the one row"""
    r = _run(eng, ctx, "edmdc", setpoint=True)
    _check("koopman mppi, set-point", r, "edmdc", setpoint=True)
    assert err(reference("edmdc", setpoint=True)["cost"], reference("edmdc")["cost"]) > 1e-3, "other reference, other costs"


def test_ill_conditioned_model(eng, ctx):
    """small_* (d = 212, ridge 1e-8) at H = 20, hold = 5, two problems, a set-point: the linear form itself departs from the iterated recursion by
    rounding amplified by |E A^t|.  Bound: max(1e-10, 50 x the error of the NumPy linear form (engine.koopman_markov, float64) against
    the long-double iterated reference, computed here); the multiple allows for FMA contraction and the kernel's fixed summation
    order over a 212-term dot product."""
    h, hold, nb = 20, 5, 2
    C, gamma, A, Bm, _ = model("small")
    r = _run(eng, ctx, "small", nb=nb, h=h, hold=hold, setpoint=True)
    ol = reference("small", ld=True, nb=nb, h=h, hold=hold, setpoint=True)
    assert ol["wrap_margin"] > MARGIN
    P, Gc = eng.koopman_markov(A, Bm, 12, h, hold)
    x = inputs("small", nb, h, hold, 1)[0]
    v = np.asarray(ol["v"], dtype=np.float64)
    lin = np.stack([np.einsum("tid,d->ti", P, kr.lift(x[b], C, gamma))[None] + np.einsum("tmij,kmj->kti", Gc, v[b]) for b in range(nb)])
    e_lin = err(lin, ol["pred"])
    bound = max(TOL_ROLL, 50.0 * e_lin)
    e_pred, e_cost = err(r["pred"], ol["pred"]), err(r["cost"], ol["cost"])
    print(f"koopman mppi small_*: kernel pred err {e_pred:.2e}  cost err {e_cost:.2e}  NumPy linear form {e_lin:.2e}  bound {bound:.2e}")
    assert e_pred <= bound and e_cost <= bound


@pytest.mark.parametrize("name", ["quat", "lin", "quat8"])
def test_other_instantiations(eng, ctx, name):
    """(n, r, k) = (13, 6, 20): the quaternion error and the nu = 6 update; (12, 6, 0): a purely linear model, no centres; (13, 8, 5)"""
    n, r_, _ = dims(name)
    r = _run(eng, ctx, name)
    assert r["pred"].shape == (B, K, H + 1, n) and r["U_nom"].shape == (B, M, r_)
    o = _check(f"koopman mppi {name} {SYNTH[name]}", r, name)
    _limits_reached(name, o)
    ol = reference(name, ld=True)
    c = record(r_)
    for b in range(B):
        Un, info, _ = mr.softmin(c, r["cost"][b], ol["delta"][b], inputs(name)[2][b], dtype=L)
        assert err(r["U_nom"][b], Un) < 1e-12 and err(r["info"][b, 2], info[2]) < 1e-12


# ------------------------------------------------------------------------------------------ 2. update
@functools.lru_cache(maxsize=None)
def spread_lambda():
    """a sixth of the reference's cost spread (max - min of a problem's costs, the smallest over the problems)"""
    S = reference("edmdc")["cost"]
    return float(np.min(S.max(axis=1) - S.min(axis=1))) / 6.0


@pytest.mark.parametrize("shift", [False, True])
def test_update_from_the_kernels_own_costs(eng, ctx, shift):
    """U_new, u_apply and info against the soft-min recomputed in long double from the kernel's OWN returned costs and the reference's
    delta, at 1e-12 (a fixed-order fp64 sum of <= 96 terms errs by <= 96 x 2^-53 = 1e-14 of sum |terms|).  S_0, beta and the
    non-finite count are exact."""
    lam = spread_lambda()
    r = _run(eng, ctx, "edmdc", lam=lam, shift=shift)
    ol = reference("edmdc", ld=True, lam=lam)
    c = record(8, lam)
    e = 0.0
    for b in range(B):
        Un, info, w = mr.softmin(c, r["cost"][b], ol["delta"][b], inputs("edmdc")[2][b], dtype=L)
        plan = np.concatenate([Un[1:], Un[-1:]], axis=0) if shift else Un
        e = max(e, err(r["U_nom"][b], plan), err(r["u_apply"][b], np.repeat(Un[:1], HOLD, axis=0)), err(r["info"][b, 2], info[2]))
        assert r["info"][b, 0] == r["cost"][b, 0] and r["info"][b, 1] == r["cost"][b].min() and r["info"][b, 3] == 0
    print(f"koopman mppi update from the kernel's costs (shift {shift}): err {e:.2e}  bound 1e-12")
    assert e < 1e-12


def test_update_end_to_end(eng, ctx):
    """U_new against the reference at 1e-6.  lambda is a sixth of the reference's cost spread; asserted on the reference: the premise
    2 (1e-10 max|S|) max|delta| / lambda <= 1e-6, and an effective sample size between 2 and K / 2 (weights neither uniform nor
    one-hot).  The plan must move by more than 1e-3."""
    lam = spread_lambda()
    r = _run(eng, ctx, "edmdc", lam=lam)
    o, ol = reference("edmdc", lam=lam), reference("edmdc", ld=True, lam=lam)
    assert 2 * TOL_ROLL * max(1.0, np.max(np.abs(o["cost"]))) * np.max(np.abs(o["delta"])) / lam <= 1e-6
    assert np.all(o["info"][:, 2] >= 2) and np.all(o["info"][:, 2] <= K / 2), o["info"][:, 2]
    assert np.all(o["info"][:, 3] == 0)
    print("effective sample sizes", o["info"][:, 2], "kernel", r["info"][:, 2])
    report("koopman mppi U_new end to end", err(r["U_nom"], o["U_new"]), err(o["U_new"], ol["U_new"]), 1e-6)
    assert err(r["info"][:, 2], o["info"][:, 2]) < 1e-4
    assert err(o["U_new"], inputs("edmdc")[2]) > 1e-3, "the update must move the plan"


# ------------------------------------------------------------------------------------------ 3. seeded stream
def test_seeded_stream_equals_explicit_normals(eng, ctx):
    a = _run(eng, ctx, "edmdc", seed=77)
    b = _run(eng, ctx, "edmdc", eps=mr.normals(77, B, K, M, 8))
    e = max(err(a["cost"], b["cost"]), err(a["pred"], b["pred"]))
    print(f"seeded against explicit normals: {e:.2e}")
    assert e < TOL_ROLL
    _check("koopman mppi, seeded stream", a, "edmdc", seed=77)
    assert err(a["cost"], reference("edmdc")["cost"]) > 1e-3, "other normals, other costs"


def test_seeded_stream_read_out_and_equal_to_the_fossen_planner(eng, ctx):
    """q = qf = 0, gamma = 0, no limits: S_k = dt sum_t sum_j r_j (U + sigma xi)^2 reads the noise out of the kernel (1e-12: 7 x 8
    fused terms err by <= 56 x 2^-53 = 6e-15 of the sum and the normals by ~6e-15).  engine.mppi_step on the same seed and record
    forms the same commands with the same code and accumulates the same terms in the same order: the same costs, whatever the
    model predicts (its tracking error is finite and weighs nothing)."""
    r = _run(eng, ctx, "edmdc", seed=123, plain=True)
    c = record(8, plain=True)
    x, ref, U, _ = inputs("edmdc")
    xi = mr.normals(123, B, K, M, 8).astype(L)
    xi[:, 0] = 0
    xi[..., c.sigma == 0] = 0
    v = U[:, None].astype(L) + c.sigma.astype(L) * xi
    steps = np.array([min(HOLD, H - m * HOLD) for m in range(M)], dtype=L)
    want = L(DT) * np.sum(steps[None, None, :, None] * c.r.astype(L) * v * v, axis=(2, 3))
    e = err(r["cost"], want)
    print(f"noise read out through the cost: {e:.2e}")
    assert e < 1e-12
    assert len(np.unique(r["cost"][0])) == K, "every sample has its own noise"
    f = eng.mppi_step(0, "rk4", [fv.params("V0")], mr.to_struct(c), x, ref, U, DT, K, H=H, seed=123, ref_row0=ROW0, want_cost=True, ctx=ctx)
    assert np.all(np.isfinite(f["cost"])) and np.array_equal(f["cost"], r["cost"])


# ------------------------------------------------------------------------------------------ 4. edges
def test_one_sample(eng, ctx):
    """K = 1: the nominal alone.  U_new is the clamped nominal and the effective sample size is 1."""
    r = _run(eng, ctx, "edmdc", k=1)
    c, U = record(8), inputs("edmdc")[2]
    assert np.array_equal(r["U_nom"], np.clip(U, c.u_min, c.u_max)) and np.array_equal(r["info"][:, 2], np.ones(B))
    assert np.array_equal(r["info"][:, 0], r["cost"][:, 0]) and np.array_equal(r["info"][:, 1], r["cost"][:, 0])
    _check("koopman mppi K = 1", r, "edmdc", k=1)


def test_64_lane_launch(eng, ctx):
    r = _run(eng, ctx, "edmdc", k=64)
    _check("koopman mppi K = 64", r, "edmdc", k=64)
    for b in range(B):
        Un, info, _ = mr.softmin(record(8), r["cost"][b], reference("edmdc", ld=True, k=64)["delta"][b], inputs("edmdc")[2][b], dtype=L)
        assert err(r["U_nom"][b], Un) < 1e-12 and err(r["info"][b, 2], info[2]) < 1e-12


@pytest.mark.parametrize("h,lanes", [(4, 256), (5, 128), (9, 128), (10, 64), (39, 64)])
def test_block_size_follows_the_lds_need(eng, ctx, h, lanes):
    """hold = 1, nu = 8, a set-point.  A block holds M nu x 8 x lanes bytes of commands and 64 bytes of table, and the larger sizes are
    taken only while two blocks fit the 160 KB of a CU: M nu = 32 runs 256 lanes and 40 already 128; 72 runs 128 and 80 -- the knots
    of H = 50 at hold 5 -- already 64; 312 is the limit (156 KB)"""
    from bluerov2_dynamics_amd import _lib
    lds = lambda bs: h * 8 * 8 * bs + 64
    cu = 160 * 1024
    assert {256: 2 * lds(256) <= cu, 128: 2 * lds(256) > cu >= 2 * lds(128), 64: 2 * lds(128) > cu >= lds(64)}[lanes]
    r = _run(eng, ctx, "edmdc", nb=2, h=h, hold=1, setpoint=True, want_pred=h < 39)
    _check(f"koopman mppi H = {h}, hold 1 ({lanes} lanes)", r, "edmdc", nb=2, h=h, hold=1, setpoint=True)
    if h == 39:                             # one knot more is refused, with the limit in the text
        with pytest.raises(_lib.BrovError, match="M nu = 320 must be <= 312"):
            _run(eng, ctx, "edmdc", nb=2, h=40, hold=1, setpoint=True)


def test_shift_and_determinism(eng, ctx):
    a, s = _run(eng, ctx, "edmdc", seed=5), _run(eng, ctx, "edmdc", seed=5, shift=True)
    assert np.array_equal(s["U_nom"][:, :-1], a["U_nom"][:, 1:]) and np.array_equal(s["U_nom"][:, -1], a["U_nom"][:, -1])
    assert not np.array_equal(a["U_nom"][:, 0], a["U_nom"][:, 1])
    for r in (a, s):
        assert np.array_equal(r["u_apply"], np.repeat(a["U_nom"][:, :1], HOLD, axis=1))
    assert np.array_equal(a["cost"], s["cost"]) and np.array_equal(a["info"], s["info"])
    a2 = _run(eng, ctx, "edmdc", seed=5)
    for k in ("U_nom", "u_apply", "cost", "info", "pred"):
        assert a[k].tobytes() == a2[k].tobytes(), k


def test_nan_in_one_sample(eng, ctx):
    """one NaN in eps of sample 5 of problem 1: that sample has weight 0 and is counted, the other problems are unaffected"""
    eps = inputs("edmdc")[3].copy()
    eps[1, 5, 1, 0] = np.nan
    good, r = _run(eng, ctx, "edmdc"), _run(eng, ctx, "edmdc", eps=eps)
    assert np.isnan(r["cost"][1, 5]) and np.isfinite(np.delete(r["cost"][1], 5)).all()
    assert list(r["info"][:, 3]) == [0, 1, 0]
    for b in (0, 2):
        for k in ("U_nom", "u_apply", "cost", "info", "pred"):
            assert r[k][b].tobytes() == good[k][b].tobytes(), (k, b)
    Un, info, w = mr.softmin(record(8), r["cost"][1], reference("edmdc", ld=True)["delta"][1], inputs("edmdc")[2][1], dtype=L)
    assert w[5] == 0 and err(r["U_nom"][1], Un) < 1e-12 and err(r["info"][1, 2], info[2]) < 1e-12
    assert np.isfinite(r["U_nom"]).all() and not np.array_equal(r["U_nom"][1], good["U_nom"][1])


def test_no_finite_sample(eng, ctx):
    """a NaN state in problem 2: its plan comes back byte-identical, u_apply is the clamped first knot, info = (non-finite, inf, 0,
    K), the call succeeds and the other problems' bits are unchanged"""
    X, _, U, _ = inputs("edmdc")
    x = X.copy()
    x[2, 0] = np.nan
    good, r = _run(eng, ctx, "edmdc", shift=True), _run(eng, ctx, "edmdc", x=x, shift=True)
    c = record(8)
    assert r["U_nom"][2].tobytes() == U[2].tobytes()
    assert np.array_equal(r["u_apply"][2], np.repeat(np.clip(U[2, :1], c.u_min, c.u_max), HOLD, axis=0))
    assert not np.isfinite(r["info"][2, 0]) and r["info"][2, 1] == np.inf and r["info"][2, 2] == 0 and r["info"][2, 3] == K
    assert not np.isfinite(r["cost"][2]).any()
    for b in (0, 1):
        for k in ("U_nom", "u_apply", "cost", "info", "pred"):
            assert r[k][b].tobytes() == good[k][b].tobytes(), (k, b)


# ------------------------------------------------------------------------------------------ 5. the host form and its refusals
def _host_args(eng, name="edmdc"):
    C, gamma, A, Bm, _ = model(name)
    x, ref, U, eps = inputs(name)
    P, Gc = eng.koopman_markov(A, Bm, 12, H, HOLD)
    f = np.ascontiguousarray
    return f(C), gamma, f(A), f(Bm), P, Gc, x, ref, U, f(eps)


def test_host_form_equals_device_form(eng, ctx):
    """edmdc_mppi_step (host arrays staged by the library) gives the bytes of engine.koopman_mppi_step, which calls the _dev form; with
    eps = NULL, and with u_apply, cost, info and pred each NULL in turn, on a fresh context whose first call grows the arena"""
    from bluerov2_dynamics_amd import _lib
    C, gamma, A, Bm, P, Gc, x, ref, U, eps = _host_args(eng)
    s = mr.to_struct(record(8))
    p = lambda a: None if a is None else a.ctypes.data
    r = _run(eng, ctx, "edmdc", shift=True)
    out = dict(U_nom=U.copy(), u_apply=np.zeros((B, HOLD, 8)), cost=np.zeros((B, K)), info=np.zeros((B, 4)), pred=np.zeros((B, K, H + 1, 12)))
    rc = ctx.lib.edmdc_mppi_step(ctx.h, 12, 8, C.shape[0], gamma, p(C), p(A), p(Bm), p(P), p(Gc), B, ctypes.byref(s), K, H, DT, 0, p(x), p(ref),
                                 REF_TOTAL, ROW0, p(eps), p(out["U_nom"]), 1, p(out["u_apply"]), p(out["cost"]), p(out["info"]), p(out["pred"]))
    assert rc == 0, ctx.lib.brov_last_error(ctx.h)
    for k, got in out.items():
        assert got.tobytes() == r[k].tobytes(), k
    seeded = _run(eng, ctx, "edmdc", shift=True, seed=77)
    fresh = _lib.Context(0)
    try:
        for drop in (None, "u_apply", "cost", "info", "pred"):
            out = dict(U_nom=U.copy(), u_apply=np.full((B, HOLD, 8), -7.25), cost=np.full((B, K), -7.25), info=np.full((B, 4), -7.25),
                       pred=np.full((B, K, H + 1, 12), -7.25))
            ptr = {k: (None if k == drop else p(v)) for k, v in out.items()}
            rc = fresh.lib.edmdc_mppi_step(fresh.h, 12, 8, C.shape[0], gamma, p(C), p(A), p(Bm), p(P), p(Gc), B, ctypes.byref(s), K, H, DT, 77,
                                           p(x), p(ref), REF_TOTAL, ROW0, None, ptr["U_nom"], 1, ptr["u_apply"], ptr["cost"], ptr["info"],
                                           ptr["pred"])
            assert rc == 0, fresh.lib.brov_last_error(fresh.h)
            for k, got in out.items():
                assert np.all(got == -7.25) if k == drop else got.tobytes() == seeded[k].tobytes(), (drop, k)
    finally:
        fresh.close()


def test_host_contract(eng, ctx):
    """every rule of the header returns BROV_ERR_ARG with a brov_last_error text naming it, and no output buffer is written"""
    C, gamma, A, Bm, P, Gc, x, ref, U, eps = _host_args(eng)
    eps = np.ascontiguousarray(eps[:, :8])
    PAT = -7.25
    p = lambda a: None if a is None else a.ctypes.data

    def call(want, n=12, r=8, k=C.shape[0], g=gamma, nb=B, kk=8, h=H, dt=DT, ref_total=REF_TOTAL, row0=ROW0, edit=None, null=()):
        s = mr.to_struct(record(8))
        if edit:
            edit(s)
        Un = U.copy()
        ua, cost, info, pred = np.full((B, max(s.hold, 1), 8), PAT), np.full((B, 8), PAT), np.full((B, 4), PAT), np.full((B, 8, H + 1, 12), PAT)
        a = dict(C=p(C), A=p(A), B=p(Bm), P=p(P), Gc=p(Gc), x=p(x), ref=p(ref), U=p(Un), cfg=ctypes.byref(s))
        for name in null:
            a[name] = None
        rc = ctx.lib.edmdc_mppi_step(ctx.h, n, r, k, g, a["C"], a["A"], a["B"], a["P"], a["Gc"], nb, a["cfg"], kk, h, dt, 0, a["x"], a["ref"],
                                     ref_total, row0, p(eps), a["U"], 0, p(ua), p(cost), p(info), p(pred))
        msg = ctx.lib.brov_last_error(ctx.h)
        msg = msg.decode() if isinstance(msg, bytes) else msg
        assert rc == -1 and want in msg and msg.startswith("edmdc_mppi_step: "), (want, rc, msg)
        assert np.array_equal(Un, U) and all(np.all(v == PAT) for v in (ua, cost, info, pred)), want

    def setf(name, value, i=None):
        def edit(s):
            if i is None:
                setattr(s, name, value)
            else:
                getattr(s, name)[i] = value
        return edit

    # what brov_mppi_step refuses and still applies
    call("K must be >= 1", kk=0)
    call("H must be >= 1", h=0)
    call("K must be <= 2^31", kk=2 ** 31 + 1)
    call("H must be <= 2^31", h=2 ** 31 + 1, ref_total=1, row0=0)
    call("hold must be >= 1", edit=setf("hold", 0))
    call("lambda must be > 0", edit=setf("lam", 0.0))
    call("q and qf must be >= 0", edit=setf("q", -1.0, 3))
    call("q and qf must be >= 0", edit=setf("qf", -1.0, 11))
    call("r must be >= 0", edit=setf("r", -0.5, 0))
    call("sigma must be >= 0", edit=setf("sigma", -0.1, 1))
    call("gamma must be >= 0", edit=setf("gamma", -1.0))
    call("u_min must be <= u_max", edit=setf("u_min", 2.0, 7))
    call("NaN in the record", edit=setf("qf", np.nan, 2))
    call("NaN in the record", edit=setf("lam", np.nan))
    call("reference window", row0=REF_TOTAL - H)
    call("reference window", row0=-1)
    call("reference window", ref_total=1, row0=1)
    call("B must be <= 65535", nb=65536)
    call("negative size", nb=-1)
    call("dt must be finite and > 0", dt=0.0)
    call("dt must be finite and > 0", dt=np.inf)
    call("dt must be finite and > 0", dt=np.nan)
    for name in ("cfg", "x", "ref", "U"):
        call("NULL input", null=(name,))
    # the model
    for n in (11, 14, 0):
        call("n must be 12 (Euler angles) or 13 (quaternion)", n=n)
    for r in (7, 0, 9):
        call("r must be 6 or 8", r=r)
    call("k must be >= 0", k=-1)
    call("k must be <= 1024", k=1025)
    for name in ("A", "B", "P", "Gc"):
        call("NULL A, B, P or Gc", null=(name,))
    call("NULL C with k > 0", null=("C",))
    call("NaN gamma", g=np.nan)
    call("M nu = 320 must be <= 312", h=40, edit=setf("hold", 1), ref_total=1, row0=0)
    # nb = 0: BROV_OK, nothing touched
    s = mr.to_struct(record(8))
    Un, cost = U.copy(), np.full((B, 8), PAT)
    rc = ctx.lib.edmdc_mppi_step(ctx.h, 12, 8, C.shape[0], gamma, p(C), p(A), p(Bm), p(P), p(Gc), 0, ctypes.byref(s), 8, H, DT, 0, p(x), p(ref),
                                 REF_TOTAL, ROW0, None, p(Un), 0, None, p(cost), None, None)
    assert rc == 0 and np.array_equal(Un, U) and np.all(cost == PAT)


# ------------------------------------------------------------------------------------------ 6. the receding-horizon driver
def _bytes(p):
    return ctypes.string_at(ctypes.byref(p), ctypes.sizeof(p))


def test_simulate_mppi_with_a_koopman_planner(eng):
    """T = 6 at hold = 3 (two ticks), two plants of which one is mismatched (V5), K = 64, H = 6, planned with the edmdc.npz model while
    the plants are Fossen thruster vehicles.  Verified tick by tick from what the driver recorded: each tick's shifted plan and
    u_apply against koopman_mppi_ref fed the recorded (x, U_nom, seed + n) at 1e-6, under the premise 2 (1e-10 max|S|) max|delta| /
    lambda <= 1e-6 asserted on the reference at every tick; the plant states equal engine.rollout_pop on the applied commands;
    planner=None gives the bits of the call without the argument."""
    from bluerov2_dynamics_amd.fossen.BlueROV2 import BlueROV2
    from bluerov2_dynamics_amd.fossen import control, identify
    from bluerov2_dynamics_amd.Koopman.koopmanEDMDc import KoopmanEDMDc
    T, hold, nb, k, h, seed = 6, 3, 2, 64, 6, 900
    C, gamma, A, Bm, X = model("edmdc")
    rng = np.random.default_rng(SEED_X + 7)
    x0 = X[rng.choice(len(X), nb, replace=False)]
    ref = np.stack([X[i:i + T + h + 1] for i in rng.choice(len(X) - T - h - 1, nb, replace=False)])
    rov = BlueROV2()
    km = KoopmanEDMDc(state_dim=12, input_dim=8, n_rbfs=C.shape[0], gamma=gamma)
    km.centers_, km.A_, km.B_ = C, A, Bm
    planner = km.mppi_planner(h, hold)
    assert (planner.n, planner.r, planner.k, planner.M) == (12, 8, C.shape[0], 2)
    c = mr.cfg(8, q=np.linspace(1.0, 2.0, 12), qf=np.linspace(4.0, 6.0, 12), r=0.1, sigma=0.25, lam=1.0, u_min=-0.7, u_max=0.7, hold=hold)
    cfg = control.mppi(c.q, qf=c.qf, r=c.r, sigma=c.sigma, lam=c.lam, u_min=c.u_min, u_max=c.u_max, hold=hold)
    assert _bytes(cfg) == _bytes(mr.to_struct(c))
    plants = [identify.params_of(rov), fv.params("V5")]
    r = rov.simulate_mppi(x0, ref, DT, cfg, T, k, h, plant_params=plants, integrator="rk4", seed=seed, planner=planner)
    tk = r["ticks"]
    nt, m = T // hold, 2
    assert r["traj"].shape == (nb, T + 1, 12) and r["u"].shape == (nb, T, 8) and r["info"].shape == (nt, nb, 4)
    assert tk["x"].shape == (nt, nb, 12) and tk["U_nom"].shape == (nt, nb, m, 8)
    assert list(tk["seed"]) == [seed + n for n in range(nt)] and list(tk["ref_row0"]) == [n * hold for n in range(nt)]
    assert np.array_equal(tk["x"][0], x0) and not tk["U_nom"][0].any()
    e_plan = g_plan = 0.0
    for n in range(nt):
        kw = dict(seed=seed + n, ref_row0=n * hold, shift=True)
        o = kr.step(C, gamma, A, Bm, c, tk["x"][n], ref, tk["U_nom"][n], DT, k, h, **kw)
        ol = kr.step(C, gamma, A, Bm, c, tk["x"][n], ref, tk["U_nom"][n], DT, k, h, dtype=L, **kw)
        assert min(o["wrap_margin"], ol["wrap_margin"]) > MARGIN
        assert 2 * TOL_ROLL * max(1.0, np.max(np.abs(o["cost"]))) * np.max(np.abs(o["delta"])) / c.lam <= 1e-6
        seg = slice(n * hold, (n + 1) * hold)
        e_plan, g_plan = max(e_plan, err(r["u"][:, seg], o["u_apply"])), max(g_plan, err(o["u_apply"], ol["u_apply"]))
        if n + 1 < nt:
            e_plan, g_plan = max(e_plan, err(tk["U_nom"][n + 1], o["U_nom"])), max(g_plan, err(o["U_nom"], ol["U_nom"]))
            assert np.array_equal(tk["x"][n + 1], r["traj"][:, (n + 1) * hold])
        # the plants: the thruster vehicles under the applied commands, from the recorded state and lag
        p = eng.rollout_pop(0, "rk4", plants, tk["x"][n][:, None], r["u"][:, seg][:, None], DT, lag=tk["lag"][n][:, None], per_candidate=True,
                            ctx=rov._ctx)
        assert np.array_equal(p["traj"][:, 0], r["traj"][:, n * hold:(n + 1) * hold + 1])
    report("simulate_mppi(planner) plan per tick", e_plan, g_plan, 1e-6)
    assert np.max(np.abs(r["u"])) <= 0.7 and np.max(np.abs(r["u"])) > 0.01
    # planner=None is the call without the argument, bit for bit
    a = rov.simulate_mppi(x0, ref, DT, cfg, T, k, h, plant_params=plants, integrator="rk4", seed=seed)
    b = rov.simulate_mppi(x0, ref, DT, cfg, T, k, h, plant_params=plants, integrator="rk4", seed=seed, planner=None)
    assert all(a[key].tobytes() == b[key].tobytes() for key in ("traj", "u", "info")) and not np.array_equal(a["u"], r["u"])
    with pytest.raises(ValueError, match="the planner is for"):
        rov.simulate_mppi(x0, ref, DT, cfg, T, k, h - 1, planner=planner)


def test_example_runs_both_planners():
    """examples/mppi_tracking.py --planner both at a size of seconds: exit status 0 and a column per planner"""
    out = subprocess.run([sys.executable, os.path.join(REPO, "examples", "mppi_tracking.py"), "--planner", "both", "--plants", "2", "--seconds",
                          "0.5", "--samples", "64", "--fit-rollouts", "8", "--fit-steps", "100", "--rbfs", "16"],
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    head = next(l for l in out.stdout.splitlines() if "fossen" in l and "koopman" in l)
    assert head.index("fossen") < head.index("koopman"), out.stdout
