"""Linear model-predictive control with an EDMDc model (edmdc_lmpc_step / engine.koopman_lmpc_step / simulate_lmpc) on the GPU against
tests/koopman_lmpc_ref.py, the NumPy restatement of the law of include/brov2.h: its coefficients are formed in the precision of the
run, and its predicted states and costs come from the ITERATED recursion z <- A z + B v (the kernel evaluates the linear form).

Parity: the mixed error max |a-b| / max(1,|b|) formed in long double against 1e-10 on U_nom, y, u_apply, pred, J(z), J(z0) and the
residuals; the iteration count and the number of entries at a limit exactly.  Every comparison also runs the reference in
np.longdouble and asserts that float64 and long double stay within a tenth of the bound.  The cases (koopman_lmpc_ref.CASES) are the
smallest at which the kernel can go wrong: Nv = 6 (one knot) .. 312 (five rows per lane), 90 and 96 either side of the switch between
W in LDS and W in global memory (test_koopman_lmpc_cpu.py asserts the switch itself), a short last knot, k = 0, 5, 70, n = 13 with r = 6, nb = 1, 3, 5, 65, iters = 0, 1, 2, 40, a
reference trajectory and a set-point, references a turn away and on the far hemisphere, a channel with u_min = u_max and one without
limits, and a tolerance case whose problems stop at different iterations (test_koopman_lmpc_cpu.py asserts that its stop rule is
well posed)."""
import ctypes
import functools

import numpy as np
import pytest

import fossen_vehicles as fv
import koopman_lmpc_ref as lr
import mppi_ref as mr
from conftest import load_golden

pytestmark = pytest.mark.gpu

TOL = 1e-10
L = np.longdouble
DT = lr.DT
KEYS = ("U_nom", "y", "u_apply", "pred", "info")


def err(a, b):
    """max |a-b| / max(1, |b|), formed in long double; equal infinities agree"""
    a, b = np.asarray(a, dtype=L), np.asarray(b, dtype=L)
    same = (a == b) | (np.isnan(a) & np.isnan(b))
    with np.errstate(invalid="ignore"):
        e = np.where(same, L(0), np.abs(a - b) / np.maximum(L(1), np.abs(b)))
    return float(np.max(e)) if a.size else 0.0


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


@functools.lru_cache(maxsize=None)
def reference(name, ld=False, shift=False):
    return lr.case_reference(name, dtype=L if ld else np.float64, shift=shift)


@functools.lru_cache(maxsize=None)
def coeffs(name):
    """(P, Gc) of engine.koopman_markov and the W of the case: float64, what a caller passes"""
    from bluerov2_dynamics_amd import engine
    s = lr.CASES[name]
    _, _, A, B = lr.case_model(name)
    return engine.koopman_markov(A, B, s["n"], s["H"], s["hold"]) + (lr.case_solver(name)[2],)


def run(eng, ctx, name, x=None, U_nom=None, y="case", sel=None, **kw):
    """engine.koopman_lmpc_step on the case (host arrays); iters / tol override the record; sel: a subset of the problems"""
    C, gamma, A, B = lr.case_model(name)
    c = lr.case_solver(name)[0]
    X, ref, U, Y, row0 = lr.case_inputs(name)
    X, U, Y = (X if x is None else x), (U if U_nom is None else U_nom), (Y if isinstance(y, str) else y)
    if sel is not None:
        X, ref, U, Y = X[sel], ref[sel], U[sel], (None if Y is None else Y[sel])
    c = lr.with_(c, **{k: kw.pop(k) for k in ("iters", "tol") if k in kw})
    kw.setdefault("want_pred", True)
    return eng.koopman_lmpc_step(C, gamma, A, B, lr.to_struct(c), X, ref, U, DT, H=lr.CASES[name]["H"], y=Y, ref_row0=row0, coeffs=coeffs(name),
                                 ctx=ctx, **kw)


def same(a, b, keys=KEYS):
    return all((a[k] is None and b[k] is None) or a[k].tobytes() == b[k].tobytes() for k in keys)


def check(what, got, name, shift=False):
    o, ol = reference(name, shift=shift), reference(name, True, shift=shift)
    c = lr.case_solver(name)[0]
    for key in ("U_nom", "y", "u_apply", "pred"):
        if got[key] is None:
            assert key == "y" and not lr.CASES[name]["y"]
            continue
        assert got[key].shape == o[key].shape, (key, got[key].shape, o[key].shape)
        report(f"{what}, {key}", err(got[key], o[key]), err(o[key], ol[key]), TOL)
    assert got["info"].shape == o["info"].shape
    for i, key in enumerate(("J(z)", "J(z0)", "r_prim", "r_dual")):
        report(f"{what}, {key}", err(got["info"][:, i], o["info"][:, i]), err(o["info"][:, i], ol["info"][:, i]), TOL)
    assert np.array_equal(o["info"][:, 4:], ol["info"][:, 4:].astype(np.float64)), "the reference's own counts depend on the precision"
    cmp = np.ones(len(o["info"]), dtype=bool)
    if lr.CASES[name]["tol"] > 0:                             # a count that hangs on rounding is left out: at most 2 % of the problems
        cmp = np.array([lr.stop_well_posed(a, c.tol) and lr.stop_well_posed(b, c.tol) for a, b in zip(o["hist"], ol["hist"])])
        assert np.sum(~cmp) <= 0.02 * len(cmp), cmp
    assert np.array_equal(got["info"][cmp, 4], o["info"][cmp, 4]), ("iterations", got["info"][:, 4], o["info"][:, 4])
    assert np.array_equal(got["info"][:, 5], o["info"][:, 5]), ("entries at a limit", got["info"][:, 5], o["info"][:, 5])
    # feasibility always; descent from a feasible start once an iteration was made with the W of the record
    z = got["U_nom"] if not shift else None
    if z is not None:
        assert np.all((z >= c.u_min) & (z <= c.u_max))
        assert np.array_equal(got["u_apply"], np.repeat(z[:, :1], c.hold, axis=1))
    if lr.CASES[name]["iters"] >= 40:
        assert np.all(got["info"][:, 0] <= got["info"][:, 1]), (got["info"][:, 0], got["info"][:, 1])
    return o


# ------------------------------------------------------------------------------------------ 1. parity
@pytest.mark.parametrize("name", list(lr.CASES))
def test_parity(eng, ctx, name):
    o = check(name, run(eng, ctx, name), name)
    s = lr.CASES[name]
    nv = lr.knots(s["H"], s["hold"]) * s["r"]
    at = o["info"][:, 5]
    if s["iters"] >= 40 and s["special"] != "warm":
        assert np.all(at >= nv // s["r"]) and np.all(at < nv), "the fixed channel is at its limit, the free one never"
    if s["tol"] > 0:
        assert len(set(o["info"][:4, 4])) > 1 and np.all(o["info"][:, 4] < s["iters"]), "the problems of a block stop at different iterations"


def test_shift(eng, ctx):
    """shift = 1 moves z and y one knot forward with the last knot repeated; everything else is the call without it"""
    a, b = run(eng, ctx, "nv24"), run(eng, ctx, "nv24", shift=True)
    check("nv24 shifted", b, "nv24", shift=True)
    for key in ("U_nom", "y"):
        assert np.array_equal(b[key], np.concatenate([a[key][:, 1:], a[key][:, -1:]], axis=1))
    assert same(a, b, ("u_apply", "pred", "info"))
    one = run(eng, ctx, "nv6", shift=True)                    # a single knot stays where it is
    assert same(one, run(eng, ctx, "nv6"))


# ------------------------------------------------------------------------------------------ 2. identities, exact bits
@pytest.mark.parametrize("name", ["nv24", "nv72", "nv96"])
def test_host_form_equals_device_form_and_calls_repeat(eng, ctx, name):
    C, gamma, A, B = lr.case_model(name)
    c = lr.to_struct(lr.case_solver(name)[0])
    x, ref, U, y, row0 = lr.case_inputs(name)
    a = run(eng, ctx, name)
    assert same(a, run(eng, ctx, name))
    up = lambda v: None if v is None else eng.DevArray.from_host(ctx, v)
    d = eng.koopman_lmpc_step(C, gamma, A, B, c, up(x), up(ref), up(U), DT, H=lr.CASES[name]["H"], y=up(y), ref_row0=row0, want_pred=True,
                              coeffs=tuple(up(v) for v in coeffs(name)), ctx=ctx)
    assert all(v is None or isinstance(v, eng.DevArray) for v in d.values())
    assert same(a, {k: (None if v is None else v.numpy()) for k, v in d.items()})
    # the host entry point itself, with every optional array NULL: the same U_nom
    lib, P, Gc, W = ctx.lib, *coeffs(name)
    U2 = U.copy()
    p = lambda v: None if v is None else v.ctypes.data
    s = lr.CASES[name]
    ctx.check(lib.edmdc_lmpc_step(ctx.h, s["n"], s["r"], s["k"], gamma, p(C), p(A), p(B), p(P), p(Gc), p(W), s["nb"], ctypes.byref(c), s["H"], DT,
                                  p(x), p(ref), ref.shape[1], row0, p(U2), None, 0, None, None, None), "edmdc_lmpc_step")
    if y is None:
        assert np.array_equal(U2, a["U_nom"])
    else:                                                     # without y_io the iteration starts from y = 0
        assert np.array_equal(U2, run(eng, ctx, name, y=np.zeros_like(y))["U_nom"])


@pytest.mark.parametrize("name", ["nv24", "nv96"])
@pytest.mark.parametrize("a,b", [(1, 1), (17, 23)])
def test_resume(eng, ctx, name, a, b):
    """iters = a, then iters = b on the returned (U_nom, y), is one call with iters = a + b"""
    y0 = np.zeros_like(lr.case_inputs(name)[2])
    first = run(eng, ctx, name, y=y0, iters=a)
    second = run(eng, ctx, name, U_nom=first["U_nom"], y=first["y"], iters=b)
    whole = run(eng, ctx, name, y=y0, iters=a + b)
    assert same(second, whole, ("U_nom", "y", "u_apply", "pred"))
    assert np.array_equal(second["info"][:, [0, 2, 3, 5]], whole["info"][:, [0, 2, 3, 5]])
    assert np.all(second["info"][:, 4] == b) and np.all(whole["info"][:, 4] == a + b)


def test_no_iteration_returns_the_clipped_start(eng, ctx):
    x, ref, U, y, row0 = lr.case_inputs("it0")
    c = lr.case_solver("it0")[0]
    r = run(eng, ctx, "it0")
    assert np.array_equal(r["U_nom"], np.clip(U, c.u_min, c.u_max)) and np.array_equal(r["y"], y)
    assert np.all(np.isinf(r["info"][:, 2:4])) and not r["info"][:, 4].any() and np.array_equal(r["info"][:, 0], r["info"][:, 1])


@pytest.mark.parametrize("name", ["nv24", "tol"])
def test_problems_are_independent(eng, ctx, name):
    """nb problems in one call are nb calls of one problem"""
    whole = run(eng, ctx, name)
    for b in range(lr.CASES[name]["nb"]):
        one = run(eng, ctx, name, sel=slice(b, b + 1))
        assert all(whole[k] is None or np.array_equal(whole[k][b:b + 1], one[k]) for k in KEYS), b


# ------------------------------------------------------------------------------------------ 3. the existing planner's cost
def test_cost_is_the_sampling_planners(eng, ctx):
    """n = 12 with equal weights on the three position errors and the reference attitude within 1 rad of the state: J(z) is the cost
    edmdc_mppi_step gives sample 0 for U_nom = z, K = 1, sigma = 0, gamma = 0 (its body-frame rotation keeps the norm, its wrapped
    angle error is the plain difference)"""
    name = "nv24"
    s = lr.CASES[name]
    C, gamma, A, B = lr.case_model(name)
    P, Gc, _ = coeffs(name)
    c = lr.case_record(name)
    q, qf = c.q.copy(), c.qf.copy()
    q[:3], qf[:3] = q[0], qf[0]
    c = lr.with_(c, q=q, qf=qf, rho=1.0)
    Hq = lr.condense(Gc, c, DT, s["H"])[0]
    c = lr.with_(c, rho=float(np.sqrt(np.prod(np.linalg.eigvalsh(Hq)[[0, -1]]))))
    W = eng._qp_inverse(Hq, c.rho)
    rng = np.random.default_rng(lr.SEED + 5)
    x, ref = rng.uniform(-0.5, 0.5, (3, 12)), rng.uniform(-0.5, 0.5, (3, 1, 12))
    U = rng.uniform(-0.3, 0.3, (3, lr.knots(s["H"], s["hold"]), 8))
    r = eng.koopman_lmpc_step(C, gamma, A, B, lr.to_struct(c), x, ref, U, DT, H=s["H"], coeffs=(P, Gc, W), ctx=ctx)
    mc = mr.cfg(8, q=q, qf=qf, r=c.r, sigma=0.0, lam=1.0, gamma=0.0, u_min=c.u_min, u_max=c.u_max, hold=s["hold"])
    m = eng.koopman_mppi_step(C, gamma, A, B, mr.to_struct(mc), x, ref, r["U_nom"], DT, 1, H=s["H"], want_cost=True, coeffs=(P, Gc), ctx=ctx)
    e = err(r["info"][:, 0], m["cost"][:, 0])
    print(f"J(z) against edmdc_mppi_step's cost of sample 0: {e:.2e}  bound {TOL:.0e}")
    assert e < TOL and np.all(r["info"][:, 0] < r["info"][:, 1])
    # a W that belongs to another record shows as a J that does not fall
    bad = eng.koopman_lmpc_step(C, gamma, A, B, lr.to_struct(c), x, ref, U, DT, H=s["H"], coeffs=(P, Gc, 3.0 * W), ctx=ctx)
    assert np.any(bad["info"][:, 0] > bad["info"][:, 1])


# ------------------------------------------------------------------------------------------ 4. a problem that is not finite
def test_a_non_finite_problem_is_left_alone(eng, ctx):
    name = "nv24"
    x, ref, U, y, row0 = lr.case_inputs(name)
    c = lr.case_solver(name)[0]
    good = run(eng, ctx, name, shift=True)
    xb = x.copy()
    xb[1, 7] = np.nan
    r = run(eng, ctx, name, x=xb, shift=True)
    keep = [0, 2, 3, 4]
    assert all(np.array_equal(r[k][keep], good[k][keep]) for k in KEYS)
    assert np.array_equal(r["U_nom"][1], U[1]) and np.array_equal(r["y"][1], y[1])
    assert np.array_equal(r["u_apply"][1], np.repeat(np.clip(U[1, :1], c.u_min, c.u_max), c.hold, axis=0))
    assert np.array_equal(r["info"][1], [np.inf] * 4 + [0, 0]) and np.all(np.isnan(r["pred"][1]))


# ------------------------------------------------------------------------------------------ 5. what the library refuses
def test_refusals(ctx):
    """every rule of the header, on the host form and the device form: BROV_ERR_ARG, a text naming the rule, nothing written"""
    from bluerov2_dynamics_amd import _lib
    name = "nv24"
    s = lr.CASES[name]
    C, gamma, A, B = lr.case_model(name)
    P, Gc, W = coeffs(name)
    x, ref, U, y, row0 = lr.case_inputs(name)
    base = lr.case_solver(name)[0]
    nan, inf = float("nan"), float("inf")

    def call(fn, rec=base, **kw):
        a = dict(n=s["n"], r=s["r"], k=s["k"], gamma=gamma, C=C, A=A, B=B, P=P, Gc=Gc, W=W, nb=s["nb"], H=s["H"], dt=DT, x=x, ref=ref,
                 ref_total=ref.shape[1], row0=row0, cfg=True)
        a.update(kw)
        p = lambda v: None if v is None else v.ctypes.data
        c = _lib.BrovLmpc()
        for i in range(rec.n):
            c.q[i], c.qf[i] = rec.q[i], rec.qf[i]
        for j in range(rec.nu):
            c.r[j], c.u_min[j], c.u_max[j] = rec.r[j], rec.u_min[j], rec.u_max[j]
        c.rho, c.tol, c.hold, c.iters = rec.rho, rec.tol, rec.hold, rec.iters
        return fn(ctx.h, a["n"], a["r"], a["k"], a["gamma"], p(a["C"]), p(a["A"]), p(a["B"]), p(a["P"]), p(a["Gc"]), p(a["W"]), a["nb"],
                  ctypes.byref(c) if a["cfg"] else None, a["H"], a["dt"], p(a["x"]), p(a["ref"]), a["ref_total"], a["row0"], p(a["U"]), None, 0,
                  None, None, None)

    w = lambda **kw: lr.with_(base, **kw)
    arr = lambda v, i, val: np.concatenate([v[:i], [val], v[i + 1:]])
    rules = [(dict(n=11), "n must be 12"), (dict(r=7), "r must be 6 or 8"), (dict(k=-1), "k must be >= 0"), (dict(k=1025), "k must be <= 1024"),
             (dict(nb=-1), "negative size"), (dict(nb=65536), "B must be <= 65535"), (dict(H=0), "H must be >= 1"),
             (dict(cfg=False), "NULL input"), (dict(x=None), "NULL input"), (dict(ref=None), "NULL input"), (dict(U=None), "NULL input"),
             (dict(A=None), "NULL A, B, P or Gc"), (dict(Gc=None), "NULL A, B, P or Gc"), (dict(W=None), "NULL W"),
             (dict(C=None), "NULL C with k > 0"), (dict(gamma=nan), "NaN gamma"), (dict(dt=0.0), "dt must be finite"), (dict(dt=inf), "dt must be finite"),
             (dict(rec=w(hold=0)), "hold must be >= 1"), (dict(rec=w(iters=-1)), "iters must be"), (dict(rec=w(iters=1000001)), "iters must be"),
             (dict(rec=w(rho=0.0)), "rho must be finite and > 0"), (dict(rec=w(rho=inf)), "rho must be finite and > 0"),
             (dict(rec=w(tol=-1e-9)), "tol must be >= 0"), (dict(rec=w(tol=nan)), "NaN in the record"),
             (dict(rec=w(q=arr(base.q, 3, -1.0))), "q and qf must be >= 0"), (dict(rec=w(r=arr(base.r, 7, -1.0))), "r must be >= 0"),
             (dict(rec=w(u_min=arr(base.u_min, 0, 1.0))), "u_min must be <= u_max"), (dict(rec=w(u_max=arr(base.u_max, 2, nan))), "NaN in the record"),
             (dict(row0=row0 + lr.REF_TOTAL + 1), "reference window"), (dict(ref_total=1, row0=1), "reference window"),
             (dict(H=s["H"] + 3 * 40, ref_total=1, row0=0), "M nu = 344 must be <= 312")]
    for dev in (False, True):                                 # the device form is handed the same host pointers: refused before any is read
        fn = ctx.lib.edmdc_lmpc_step_dev if dev else ctx.lib.edmdc_lmpc_step
        for kw, text in rules:
            U_ = U.copy()
            rc = call(fn, **{"U": U_, **kw})
            msg = ctx.lib.brov_last_error(ctx.h).decode()
            assert rc == -1 and text in msg and msg.startswith("edmdc_lmpc_step: "), (list(kw), rc, msg)
            assert np.array_equal(U_, U)
        U_ = U.copy()
        assert call(fn, nb=0, U=U_) == 0 and np.array_equal(U_, U)


# ------------------------------------------------------------------------------------------ 6. the closed loop
def test_simulate_lmpc(eng):
    """20 ticks (hold = 2, H = 10), three plants of which one is mismatched (V5), planned with the `small` golden model while the
    plants are Fossen thruster vehicles.  Tick by tick from what the driver recorded: koopman_lmpc_step fed the recorded (x, U_nom,
    y) reproduces the next recorded plan and the applied command bit for bit; the plant states equal engine.rollout_pop on the
    applied commands."""
    from bluerov2_dynamics_amd.fossen.BlueROV2 import BlueROV2
    from bluerov2_dynamics_amd.fossen import control, identify
    from bluerov2_dynamics_amd.Koopman.koopmanEDMDc import KoopmanEDMDc
    f, X = load_golden("edmdc_fit.npz"), load_golden("edmdc.npz")["X"]
    C, A, Bm = f["small_centers"], f["small_A"], f["small_B"]
    hold, H, nb, nt, dt = 2, 10, 3, 20, 0.05
    T = nt * hold
    rng = np.random.default_rng(lr.SEED + 3)
    x0 = X[rng.choice(len(X), nb, replace=False)]
    ref = np.stack([X[i:i + T + H + 1] for i in rng.choice(len(X) - T - H - 1, nb, replace=False)])
    rov = BlueROV2()
    km = KoopmanEDMDc(state_dim=12, input_dim=8, n_rbfs=C.shape[0], gamma=1.0)
    km.centers_, km.A_, km.B_ = C, A, Bm
    cfg = control.lmpc(np.linspace(1.0, 2.0, 12), qf=np.linspace(4.0, 6.0, 12), r=0.1, u_min=-0.7, u_max=0.7, hold=hold, iters=60)
    planner = km.lmpc_planner(H, cfg, dt)
    M = 5
    assert (planner.n, planner.r, planner.k, planner.M) == (12, 8, C.shape[0], M) and planner.Hq.shape == (M * 8, M * 8)
    ev = np.linalg.eigvalsh(planner.Hq)
    assert planner.rho == planner.cfg.rho == pytest.approx(np.sqrt(ev[0] * ev[-1]), rel=1e-12) and cfg.rho == 0.0
    plants = [identify.params_of(rov), identify.params_of(rov), fv.params("V5")]
    r = rov.simulate_lmpc(x0, ref, dt, planner, T, plant_params=plants, integrator="rk4")
    tk = r["ticks"]
    assert r["traj"].shape == (nb, T + 1, 12) and r["u"].shape == (nb, T, 8) and r["info"].shape == (nt, nb, 6)
    assert tk["x"].shape == (nt, nb, 12) and tk["U_nom"].shape == tk["y"].shape == (nt, nb, M, 8)
    assert list(tk["ref_row0"]) == [n * hold for n in range(nt)]
    assert np.array_equal(tk["x"][0], x0) and not tk["U_nom"][0].any() and not tk["y"][0].any()
    for n in range(nt):
        o = planner.step(tk["x"][n], ref, tk["U_nom"][n], tk["y"][n], ref_row0=n * hold, shift=True)
        seg = slice(n * hold, (n + 1) * hold)
        assert np.array_equal(o["u_apply"], r["u"][:, seg]) and np.array_equal(o["info"], r["info"][n])
        if n + 1 < nt:
            assert np.array_equal(o["U_nom"], tk["U_nom"][n + 1]) and np.array_equal(o["y"], tk["y"][n + 1])
            assert np.array_equal(tk["x"][n + 1], r["traj"][:, (n + 1) * hold])
        p = eng.rollout_pop(0, "rk4", plants, tk["x"][n][:, None], r["u"][:, seg][:, None], dt, lag=tk["lag"][n][:, None], per_candidate=True,
                            ctx=rov._ctx)
        assert np.array_equal(p["traj"][:, 0], r["traj"][:, n * hold:(n + 1) * hold + 1])
    assert np.max(np.abs(r["u"])) <= 0.7 and np.max(np.abs(r["u"])) > 0.01
    assert np.all(np.isfinite(r["info"])) and np.all(r["info"][:, :, 4] == 60)
    with pytest.raises(ValueError, match="condensed for dt"):
        rov.simulate_lmpc(x0, ref, 0.1, planner, T)
