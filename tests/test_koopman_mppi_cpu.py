"""The model-predictive update with an EDMDc planning model (edmdc_mppi_step), the parts that need no GPU: the tests' own reference
(tests/koopman_mppi_ref.py) pinned to the reference's `simulate` through the committed fixtures, engine.koopman_markov (the
coefficients of the linear form the kernel evaluates) against that reference in long double, the ABI mirror, and the argument
checks that run before any device is touched.

The models: tests/golden/edmdc.npz (d = 60), simscript.npz (d = 72) and the ill-conditioned edmdc_fit.npz small_* (d = 212, ridge
1e-8, |E A^50| ~ 50).  Bounds on the linear form against the long-double iterated recursion, mixed error |a-b| / max(1,|b|): 1e-11 for
the first two (the NumPy linear form measures 3e-15 .. 2e-14 there) and 1e-9 for small_* (measured 5e-13 .. 1.2e-11)."""
import ctypes

import numpy as np
import pytest

import koopman_mppi_ref as kr
from conftest import load_golden

L = np.longdouble
SHAPES = ((6, 2), (7, 3), (20, 5), (50, 5))          # (H, hold); (7, 3): the last knot covers one step


def err(a, b):
    """max |a-b| / max(1, |b|), formed in long double"""
    a, b = np.asarray(a, dtype=L), np.asarray(b, dtype=L)
    return float(np.max(np.abs(a - b) / np.maximum(L(1), np.abs(b)))) if a.size else 0.0


def models():
    """name -> (C, gamma, A, B, X): the three fixture models and the recording their start states come from"""
    e, s, f = load_golden("edmdc.npz"), load_golden("simscript.npz"), load_golden("edmdc_fit.npz")
    return {"edmdc": (e["centers"], float(e["gamma"]), e["A"], e["B"], e["X"]),
            "simscript": (s["centers"], 1.0, s["A"], s["B"], s["X"]),
            "small": (f["small_centers"], 1.0, f["small_A"], f["small_B"], e["X"])}


def test_the_reference_reproduces_the_recorded_simulations():
    """koopman_mppi_ref.predict on the fixtures' own commands (one sample, hold = 1) is the reference's `simulate`: sim50 of edmdc.npz
    and pred200 of simscript.npz at 1e-12"""
    e = load_golden("edmdc.npz")
    nt = int(e["n_train"])
    got = kr.predict(e["centers"], float(e["gamma"]), e["A"], e["B"], e["X"][nt], e["U"][nt:nt + 50][None], 50, 1)
    assert got.shape == (1, 51, 12) and err(got[0], e["sim50"]) < 1e-12
    s = load_golden("simscript.npz")
    split = int(0.8 * int(s["N"]))
    got = kr.predict(s["centers"], 1.0, s["A"], s["B"], s["X"][split - 1], s["U"][split - 1:split - 1 + 200][None], 200, 1)
    assert err(got[0], s["pred200"]) < 1e-12
    # the long-double run of the same recursion stays within rounding of it, and a held knot is the same command repeated
    gl = kr.predict(s["centers"], 1.0, s["A"], s["B"], s["X"][split - 1], s["U"][split - 1:split - 1 + 200][None], 200, 1, dtype=L)
    assert err(got, gl) < 1e-12
    held = kr.predict(e["centers"], float(e["gamma"]), e["A"], e["B"], e["X"][nt], e["U"][nt:nt + 2][None], 6, 3)
    rep = kr.predict(e["centers"], float(e["gamma"]), e["A"], e["B"], e["X"][nt], np.repeat(e["U"][nt:nt + 2], 3, axis=0)[None], 6, 1)
    assert np.array_equal(held, rep)


@pytest.mark.parametrize("name,bound", [("edmdc", 1e-11), ("simscript", 1e-11), ("small", 1e-9)])
def test_markov_coefficients_against_the_iterated_recursion(name, bound):
    """engine.koopman_markov: P[t] phi(x) + sum_m Gc[t][m] v[m] in float64 against the long-double iterated recursion, for random
    clipped commands (8 samples) from four start states of the recording; Gc is exactly zero where m hold >= t and P[0] = E"""
    from bluerov2_dynamics_amd import engine
    C, gamma, A, B, X = models()[name]
    n, d, r = 12, A.shape[0], B.shape[1]
    rng = np.random.default_rng(20 + len(name))
    worst = 0.0
    for H, hold in SHAPES:
        M = (H + hold - 1) // hold
        P, Gc = engine.koopman_markov(A, B, n, H, hold)
        assert P.shape == (H + 1, n, d) and Gc.shape == (H + 1, M, n, r) and P.dtype == Gc.dtype == np.float64
        assert np.array_equal(P[0], np.eye(n, d)) and np.array_equal(P[1], A[:n])
        for t in range(H + 1):
            for m in range(M):
                assert (m * hold >= t) == (not Gc[t, m].any()), (t, m)
        assert np.array_equal(Gc[1, 0], B[:n])
        if (H, hold) == (7, 3):                           # the last knot has acted for one step at t = H: the newest Markov block alone
            assert np.array_equal(Gc[7, 2], B[:n]) and np.array_equal(Gc[7, 1], Gc[4, 0]) and not np.array_equal(Gc[7, 0], Gc[7, 1])
        for row in rng.choice(len(X), 4, replace=False):
            v = np.clip(rng.normal(0.0, 0.4, (8, M, r)), -0.6, 0.6)
            want = kr.predict(C, gamma, A, B, X[row], v, H, hold, dtype=L)
            phi = kr.lift(X[row], C, gamma)
            got = np.einsum("tid,d->ti", P, phi)[None] + np.einsum("tmij,kmj->kti", Gc, v)
            worst = max(worst, err(got, want))
    print(f"koopman_markov, {name}: linear form against the long-double recursion {worst:.2e}  bound {bound:.0e}")
    assert worst <= bound


def test_abi_mirror():
    from bluerov2_dynamics_amd import _build, _lib
    _build.build_library()
    lib = _lib.load_library()
    for name in ("edmdc_mppi_step", "edmdc_mppi_step_dev"):
        fn = getattr(lib, name)
        assert fn.restype is ctypes.c_int and len(fn.argtypes) == 27
        assert fn.argtypes[4] is ctypes.c_double and fn.argtypes[14] is ctypes.c_double and fn.argtypes[15] is ctypes.c_uint64
    # a NULL context is refused without touching anything
    assert lib.edmdc_mppi_step(None, 12, 8, 0, 1.0, *([None] * 5), 1, None, 1, 1, 0.02, 0, None, None, 1, 0, None, None, 0, *([None] * 4)) == -1


def test_argument_checks_that_need_no_device():
    from bluerov2_dynamics_amd import engine
    from bluerov2_dynamics_amd.Koopman.koopmanEDMDc import KoopmanEDMDc
    A, B = np.eye(14), np.ones((14, 8))
    for kw in (dict(H=0, hold=1), dict(H=4, hold=0), dict(n=15), dict(n=0), dict(A=np.ones((14, 13))), dict(B=np.ones((13, 8)))):
        args = dict(A=A, B=B, n=12, H=4, hold=2)
        args.update(kw)
        with pytest.raises(AssertionError):
            engine.koopman_markov(**args)
    with pytest.raises(ValueError, match="fit"):
        KoopmanEDMDc(state_dim=12, input_dim=8).mppi_planner(10, 5)
    m = KoopmanEDMDc(state_dim=12, input_dim=8)
    m.centers_, m.A_, m.B_ = np.zeros((2, 12)), A, B
    for H, hold in ((0, 1), (5, 0)):
        with pytest.raises(ValueError):
            m.mppi_planner(H, hold)
