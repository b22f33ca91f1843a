"""Linear model-predictive control with an EDMDc model (edmdc_lmpc_step), the parts that need no GPU: the condensed form of the cost
(engine.koopman_qp_condense and the reference's g, c) against the cost of the ITERATED recursion, the reference's ADMM loop
(tests/koopman_lmpc_ref.py) against an independent exact solver and in its limiting cases, the stop rule of the tolerance cases the
GPU tests use, the ABI mirror and the argument checks that run before any device is touched.

The set-up of the solver tests: tests/golden/edmdc.npz, q = (40,40,60,4,4,6,2,2,3,.2,.2,.4), qf = 5 q, r = 0.05, dt = 0.02, limits
+-0.3, x = X[10], the set-point X[60], a zero warm start, rho = sqrt(lambda_min lambda_max) of Hq, 2 000 iterations."""
import ctypes

import numpy as np
import pytest

import koopman_lmpc_ref as lr
import koopman_mppi_ref as kr
from conftest import load_golden, rel_err

L = np.longdouble
Q = np.array([40, 40, 60, 4, 4, 6, 2, 2, 3, .2, .2, .4])
SHAPES = ((50, 5), (20, 1), (7, 3))          # (H, hold): Nv = 80, 160, 24


def golden_model(name):
    e = load_golden("edmdc.npz")
    if name == "edmdc":
        return e["centers"], float(e["gamma"]), e["A"], e["B"], e["X"]
    f = load_golden("edmdc_fit.npz")
    return f["small_centers"], 1.0, f["small_A"], f["small_B"], e["X"]


def setup(H, hold, r=0.05, lim=0.3, iters=2000):
    """(record with rho, Hq, W, g, model, x, adjusted reference rows) of the set-up above, through the ENGINE's condensation"""
    from bluerov2_dynamics_amd import engine
    C, gamma, A, B, X = golden_model("edmdc")
    c = lr.rec(12, 8, Q, 5 * Q, r, -lim, lim, hold=hold, iters=iters)
    P, Gc = engine.koopman_markov(A, B, 12, H, hold)
    Hq, _ = engine.koopman_qp_condense(Gc, lr.to_struct(lr.with_(c, rho=1.0)), 0.02, H)
    ev = np.linalg.eigvalsh(Hq)
    c = lr.with_(c, rho=float(np.sqrt(ev[0] * ev[-1])))
    W = engine._qp_inverse(Hq, c.rho)
    rt = lr.adjust(lr.window(X[60:61], 0, H), X[10])
    g, _ = lr.gradient(c, P @ kr.lift(X[10], C, gamma), Gc, rt, 0.02, H)
    return c, Hq, W, g, (C, gamma, A, B), X[10], rt


@pytest.mark.parametrize("name", ["edmdc", "small", "quat"])
@pytest.mark.parametrize("H,hold", [(7, 3), (10, 1)])
def test_condensation_identity(name, H, hold):
    """1/2 v' Hq v + g' v + c is the cost of the iterated recursion z <- A z + B v[m(t)] from phi(x), for random v: Hq from
    engine.koopman_qp_condense on engine.koopman_markov's Gc, g and c from the reference; 1e-10 mixed"""
    from bluerov2_dynamics_amd import engine
    rng = np.random.default_rng(31 + H + len(name))
    if name == "quat":
        n, r = 13, 6
        C, gamma, A, B = lr.synth_model(13, 6, 20, 77)
        x, ref = rng.uniform(-0.5, 0.5, 13), rng.uniform(-0.5, 0.5, (1, 13))
        x[3:7] /= np.linalg.norm(x[3:7])
        ref[0, 3:7] = -(x[3:7] + 0.1 * ref[0, 3:7])          # the far hemisphere: flipped by the adjustment
        q = rng.uniform(0.5, 2.0, 13)
    else:
        n, r = 12, 8
        C, gamma, A, B, X = golden_model(name)
        x, ref, q = X[10], X[60:61].copy(), Q
        ref[0, 5] += 2 * np.pi                               # taken back by the adjustment
    c = lr.rec(n, r, q, 5 * q, rng.uniform(0.01, 0.1, r), hold=hold)
    M = lr.knots(H, hold)
    P, Gc = engine.koopman_markov(A, B, n, H, hold)
    Hq, steps = engine.koopman_qp_condense(Gc, lr.to_struct(c), 0.02, H)
    assert Hq.shape == (M * r, M * r) and np.array_equal(Hq, Hq.T) and steps.sum() == H and steps[-1] == H - hold * (M - 1)
    assert rel_err(Hq, lr.condense(Gc, c, 0.02, H)[0]) < 1e-13
    rt = lr.adjust(lr.window(ref, 0, H), x)
    if name == "quat":
        assert np.array_equal(rt[0, 3:7], -ref[0, 3:7])
    else:
        assert abs(rt[0, 5] - X[60, 5]) < 1e-12
    g, c0 = lr.gradient(c, P @ kr.lift(x, C, gamma), Gc, rt, 0.02, H)
    worst = 0.0
    for _ in range(6):
        v = rng.uniform(-0.5, 0.5, (M, r))
        J = lr.cost(c, kr.predict(C, gamma, A, B, x, v[None], H, hold, dtype=L)[0], rt.astype(L), v, 0.02, H, dtype=L)
        vv = v.ravel()
        worst = max(worst, rel_err(0.5 * vv @ Hq @ vv + g @ vv + c0, float(J)))
    print(f"condensation identity, {name} H = {H} hold = {hold}: {worst:.2e}  bound 1e-10")
    assert worst <= 1e-10


@pytest.mark.parametrize("H,hold", SHAPES)
def test_admm_against_an_independent_solver(H, hold):
    """2 000 iterations of the reference from a zero warm start: the projected-gradient residual of its result is <= 1e-9 (measured
    1.6e-11, 2.5e-14, 4.7e-16), and at H = 7 / hold 3 the result is SciPy's exact active-set solution (BVLS on the Cholesky factor)
    to 1e-10 (measured 3.8e-15)"""
    c, Hq, W, g, _, _, _ = setup(H, hold)
    nv = Hq.shape[0]
    z, y, rp, rd, it, _ = lr.admm(c, W, g, np.zeros(nv), np.zeros(nv))
    lo, hi = np.full(nv, -0.3), np.full(nv, 0.3)
    res = lr.projected_gradient_residual(Hq, g, z, lo, hi)
    print(f"H = {H} hold = {hold} (Nv = {nv}): projected-gradient residual {res:.2e}  bound 1e-9; r_prim {rp:.1e} r_dual {rd:.1e}; "
          f"{int(np.sum((z == lo) | (z == hi)))} entries at a limit")
    assert it == 2000 and np.all((z >= lo) & (z <= hi))
    assert res <= 1e-9
    if (H, hold) != (7, 3):
        return
    try:
        from scipy.optimize import lsq_linear
    except ImportError:
        pytest.skip("SciPy is needed for the BVLS comparison only")
    R = np.linalg.cholesky(Hq).T                              # Hq = R' R: 1/2 v' Hq v + g' v = 1/2 |R v - b|^2 + const, b = -R^-T g
    sol = lsq_linear(R, -np.linalg.solve(R.T, g), bounds=(lo, hi), method="bvls", tol=1e-15)
    d = float(np.max(np.abs(z - sol.x)))
    print(f"against BVLS: {d:.2e}  bound 1e-10")
    assert d <= 1e-10


def test_exact_limiting_cases():
    """without limits the iteration converges to -Hq^-1 g; with limits so tight that every entry is clamped it returns the active
    limit exactly"""
    H, hold = 7, 3
    c, Hq, W, g, _, _, _ = setup(H, hold, lim=np.inf, iters=3000)
    nv = Hq.shape[0]
    z, y, rp, rd, it, _ = lr.admm(c, W, g, np.zeros(nv), np.zeros(nv))
    zs = -np.linalg.solve(Hq, g)
    # Without a clip y stays 0 and the error obeys e+ = rho W e, so z+ - z = -(W Hq) e: |e|_2 <= (lambda_min + rho) / lambda_min
    # |z+ - z|_2 <= sqrt(Nv) (lambda_min + rho) / (lambda_min rho) r_dual; on top the rounding of the solve, cond(Hq) eps |z*|
    ev = np.linalg.eigvalsh(Hq)
    bound = np.sqrt(nv) * (ev[0] + c.rho) / (ev[0] * c.rho) * rd + 10 * (ev[-1] / ev[0]) * np.finfo(float).eps * np.max(np.abs(zs))
    d = float(np.max(np.abs(z - zs)))
    print(f"no limits: |z - z*| {d:.2e}  bound {bound:.2e} (r_prim {rp:.1e}, r_dual {rd:.1e})")
    assert it == 3000 and rp == 0.0 and not y.any()
    assert d <= bound and bound < 1e-9
    lim = 1e-4
    c, Hq, W, g, _, _, _ = setup(H, hold, lim=lim, iters=3000)
    z, y, rp, rd, it, _ = lr.admm(c, W, g, np.zeros(nv), np.zeros(nv))
    # |g_i| > sum_j |Hq_ij| lim: the gradient keeps its sign on the whole box, so the minimiser is the corner -sign(g) lim
    assert np.all(np.abs(g) > np.abs(Hq).sum(axis=1) * lim), "the limits are not tight enough for the case"
    assert np.array_equal(z, np.where(g > 0, -lim, lim))


@pytest.mark.parametrize("name", [k for k, s in lr.CASES.items() if s["tol"] > 0])
def test_the_stop_rule_of_the_gpu_cases_is_well_posed(name):
    """The iteration count of a tolerance case is compared EXACTLY on the GPU, so the decision `both residuals <= tol` must not hang
    on rounding: for every problem the reference's deciding residual, max(r_prim, r_dual), is at least a factor 10 away from tol at
    the stop iteration and at the one before it (koopman_lmpc_ref.stop_well_posed), in float64 and in long double, and both
    precisions stop at the same iteration.  A problem where that fails is left out of the comparison on the GPU; at most 2 % may
    be, and with these seeds none is.  The problems of the first block stop at different iterations.
    This test runs the reference alone (no code of the library): it secures the inputs of the GPU test."""
    s = lr.CASES[name]
    res = {dt: lr.case_reference(name, dtype=dt) for dt in (np.float64, L)}
    left_out = []
    for b in range(s["nb"]):
        ok = int(res[np.float64]["info"][b, 4]) == int(res[L]["info"][b, 4])
        for dt in (np.float64, L):
            h = res[dt]["hist"][b].max(axis=1)
            assert 2 <= h.shape[0] < s["iters"], "the case must stop by its residuals, after at least two iterations"
            ok = ok and lr.stop_well_posed(res[dt]["hist"][b], s["tol"])
            print(f"{name}[{b}] {np.dtype(dt).name}: stops at {h.shape[0]}, residual {float(h[-2]):.3e} -> {float(h[-1]):.3e} around tol {s['tol']:.1e}")
        if not ok:
            left_out.append(b)
    assert len(set(res[np.float64]["info"][:4, 4])) > 1, "the problems of the first block must stop at different iterations"
    assert len(left_out) <= 0.02 * s["nb"], left_out
    assert not left_out, left_out


def test_the_switch_between_w_in_lds_and_w_in_global_memory():
    """edmdc_lmpc_block_lds is the solve kernel's own block-size function: W is staged while two blocks fit a CU's 160 KB of LDS
    together, 8 Nv^2 + 4 waves x 3 Nv x 8 bytes each, which holds up to Nv = 95 -- so the GPU cases Nv = 90 and Nv = 96 take the two
    paths"""
    from bluerov2_dynamics_amd import _build, _lib
    _build.build_library()
    lib = _lib.load_library()
    w = ctypes.c_int(-1)
    for nv in range(1, 313):
        got = lib.edmdc_lmpc_block_lds(nv, ctypes.byref(w))
        slices = 4 * 3 * nv * 8
        staged = 2 * (8 * nv * nv + slices) <= 160 * 1024
        assert w.value == int(staged) == int(nv <= 95) and got == slices + (8 * nv * nv if staged else 0), nv
    nvs = {name: lr.knots(c["H"], c["hold"]) * c["r"] for name, c in lr.CASES.items()}
    assert nvs["nv90"] == 90 and nvs["nv96"] == 96 and lib.edmdc_lmpc_block_lds(90, ctypes.byref(w)) > 0 and w.value == 1
    assert lib.edmdc_lmpc_block_lds(96, ctypes.byref(w)) == 4 * 3 * 96 * 8 and w.value == 0
    assert lib.edmdc_lmpc_block_lds(0, None) == -1 and lib.edmdc_lmpc_block_lds(313, None) == -1 and lib.edmdc_lmpc_block_lds(24, None) > 0


def test_abi_mirror_and_record_layout():
    from bluerov2_dynamics_amd import _build, _lib
    _build.build_library()
    lib = _lib.load_library()
    R = _lib.BrovLmpc
    assert ctypes.sizeof(R) == (13 + 13 + 8 + 8 + 8 + 2 + 1) * 8 == 53 * 8
    assert [(f, getattr(R, f).offset) for f, _ in R._fields_] == [("q", 0), ("qf", 104), ("r", 208), ("u_min", 272), ("u_max", 336),
                                                                   ("rho", 400), ("tol", 408), ("hold", 416), ("iters", 420)]
    import re
    from conftest import REPO
    import os
    txt = open(os.path.join(REPO, "include", "brov2.h")).read()
    body = re.search(r"typedef struct brov_lmpc \{(.*?)\} brov_lmpc;", txt, flags=re.S).group(1)
    names = re.findall(r"(\w+)(?:\[\d+\])?\s*[,;]", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert names == ["q", "qf", "r", "u_min", "u_max", "rho", "tol", "hold", "iters"]
    for name in ("edmdc_lmpc_step", "edmdc_lmpc_step_dev"):
        fn = getattr(lib, name)
        assert fn.restype is ctypes.c_int and len(fn.argtypes) == 25
        assert fn.argtypes[4] is ctypes.c_double and fn.argtypes[14] is ctypes.c_double and fn.argtypes[21] is ctypes.c_int
        # a NULL context is refused without touching anything
        assert fn(None, 12, 8, 0, 1.0, *([None] * 6), 1, None, 1, 0.02, None, None, 1, 0, None, None, 0, None, None, None) == -1


def test_argument_checks_that_need_no_device():
    from bluerov2_dynamics_amd import engine
    from bluerov2_dynamics_amd.fossen import control
    from bluerov2_dynamics_amd.Koopman.koopmanEDMDc import KoopmanEDMDc
    ok = dict(q=1.0, r=0.1, u_min=-1.0, u_max=1.0)
    cfg = control.lmpc(**ok)
    assert (cfg.hold, cfg.iters, cfg.tol, cfg.rho) == (1, 200, 0.0, 0.0) and cfg.qf[11] == 1.0 and cfg.q[12] == 0.0
    assert control.lmpc(np.ones(13), n=13, nu=6, rho=2.5).rho == 2.5
    nan = float("nan")
    for kw in (dict(q=-1.0), dict(qf=-1.0), dict(r=-0.1), dict(q=nan), dict(u_min=nan), dict(tol=nan), dict(tol=-1e-3), dict(rho=0.0),
               dict(rho=-1.0), dict(rho=np.inf), dict(rho=nan), dict(u_min=2.0), dict(hold=0), dict(hold=1.5), dict(iters=-1),
               dict(iters=1000001), dict(nu=7), dict(n=11), dict(q=np.ones(13))):
        with pytest.raises(ValueError):
            control.lmpc(**{**ok, **kw})
    # the condensation: steps of a short last knot, and a shape that does not fit the record
    A, B = 0.9 * np.eye(14), 0.1 * np.ones((14, 8))
    P, Gc = engine.koopman_markov(A, B, 12, 7, 3)
    Hq, steps = engine.koopman_qp_condense(Gc, control.lmpc(q=1.0, r=0.1, hold=3), 0.05, 7)
    assert list(steps) == [3, 3, 1] and Hq.shape == (24, 24)
    with pytest.raises(AssertionError):
        engine.koopman_qp_condense(Gc, control.lmpc(q=1.0, r=0.1, hold=2), 0.05, 7)
    # a cost that leaves some knot without a weight has no unique minimum: refused before any device is touched
    with pytest.raises(ValueError, match="positive definite"):
        engine.KoopmanLmpc(np.zeros((2, 12)), 1.0, A, B, 7, control.lmpc(q=0.0, r=0.0, hold=3), 0.05)
    with pytest.raises(ValueError, match="fit"):
        KoopmanEDMDc(state_dim=12, input_dim=8).lmpc_planner(10, cfg, 0.05)
    m = KoopmanEDMDc(state_dim=12, input_dim=8)
    m.centers_, m.A_, m.B_ = np.zeros((2, 12)), A, B
    with pytest.raises(ValueError):
        m.lmpc_planner(0, cfg, 0.05)
    with pytest.raises(ValueError):
        m.lmpc_planner(5, cfg, 0.0)
