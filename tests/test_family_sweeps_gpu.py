"""Shape sweeps over the five newer kernel families on the GPU: population rollouts, closed-loop rollouts, the Fossen and the Koopman
MPPI step, and the population window evaluator with fd_normal_eq.  Each family's own test file runs one hand-picked shape; here every
family runs the 48 cases of tests/sweep_cases.py (a hand-written corner list over every block edge, knot count, window and stride
rule, then seeded draws) in four slices, each case against the family's NumPy / long-double reference by the recipe of
tests/sweep_run.py: mixed error in long double against 1e-10 on every output, the soft-min update from the kernel's own costs at
1e-12, counts exact, a lane compared only where the reference itself is well-posed (tests/test_sweep_cases_cpu.py asserts on the CPU
that this leaves out at most 2 % of a case's lanes and never a whole case).  Then the exact identities the code promises, on the
first cases of each list.  A failure message carries the case dict: sweep_run.sweep_one(eng, ctx, case) reruns it alone."""
import numpy as np
import pytest

import mppi_ref as mr
import sweep_cases as sc
import sweep_run as sr

pytestmark = pytest.mark.gpu

SLICES = 4
IDENTITY_CASES = 4


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


@pytest.mark.parametrize("part", range(SLICES))
@pytest.mark.parametrize("family", sc.FAMILIES)
def test_sweep(eng, ctx, family, part):
    cases = sc.cases(family)[part::SLICES]
    worst = second = gap = 0.0
    left = 0
    for c in cases:
        e, e2, out, g = sr.sweep_one(eng, ctx, c)
        worst, second, gap, left = max(worst, e), max(second, e2), max(gap, g), left + out
    print(f"{family} slice {part}: {len(cases)} cases, worst kernel err {worst:.2e} (bound {sr.TOL_ROLL:.0e}), update / normal equations "
          f"{second:.2e}, worst reference gap {gap:.2e}, lanes left out {left}")


def _same_bytes(a, b, case):
    assert a.keys() == b.keys()
    for k in a:
        assert (a[k] is None and b[k] is None) or np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes(), (k, case)


@pytest.mark.parametrize("family", ["rollout_pop", "feedback"])
def test_rollouts_repeat_and_store_off_gives_the_stored_end_state(eng, ctx, family):
    """two identical calls give identical bytes; store=False gives the stored run's xT (and lag, z, u, metrics)"""
    run = sr.run_rollout_pop if family == "rollout_pop" else sr.run_feedback
    for c in sc.cases(family)[:IDENTITY_CASES]:
        ref = sr.PREPARE[family](c)
        a, b = run(eng, ctx, c, ref), run(eng, ctx, c, ref)
        _same_bytes(a, b, c)
        other = run(eng, ctx, c, ref, store=not c["store"])
        for k in a:
            if k != "traj":
                assert (a[k] is None and other[k] is None) or np.array_equal(a[k], other[k]), (k, c)
        stored = a if c["store"] else other
        assert np.array_equal(stored["traj"][:, :, 0], np.broadcast_to(ref["x0"], stored["traj"][:, :, 0].shape)), ("row 0 is x0", c)
        if c["T"] and c["T"] % c["stride"] == 0:
            assert np.array_equal(stored["traj"][:, :, -1], stored["xT"]), ("the last stored row is xT", c)


@pytest.mark.parametrize("family", ["mppi", "koopman_mppi"])
def test_mppi_shift_repeat_and_seeded_stream(eng, ctx, family):
    """shift = 1 against shift = 0 (tests/test_mppi_gpu.py: test_shift_and_determinism): the knots move by one and the last is
    repeated, u_apply is U_new[0] in hold rows either way, costs and info do not change; two identical calls give identical bytes;
    the seeded stream gives the costs of the explicit mppi_ref.normals to TOL_ROLL.  On the first cases of the list plus the first
    with the seeded stream at K > 256."""
    run = sr.run_mppi if family == "mppi" else sr.run_koopman_mppi
    cases = sc.cases(family)
    picked = cases[:IDENTITY_CASES] + [c for c in cases[IDENTITY_CASES:] if not c["eps"] and c["K"] > 256][:1]
    assert any(not c["eps"] for c in picked)
    for c in picked:
        ref = sr.PREPARE[family](c)
        lam = ref["lam_update"]
        a, a2 = run(eng, ctx, c, ref, lam=lam, shift=False), run(eng, ctx, c, ref, lam=lam, shift=False)
        s = run(eng, ctx, c, ref, lam=lam, shift=True)
        _same_bytes(a, a2, c)
        assert np.array_equal(s["U_nom"][:, :-1], a["U_nom"][:, 1:]) and np.array_equal(s["U_nom"][:, -1], a["U_nom"][:, -1]), c
        for r in (a, s):
            assert np.array_equal(r["u_apply"], np.repeat(a["U_nom"][:, :1], c["hold"], axis=1)), c
        assert np.array_equal(a["cost"], s["cost"]) and np.array_equal(a["info"], s["info"]), c
        if not c["eps"]:
            xi = mr.normals(c["stream_seed"], c["B"], c["K"], c["M"], ref["nu"])
            b = run(eng, ctx, c, ref, lam=lam, shift=False, eps=xi)
            e = sr.err(a["cost"], b["cost"])
            assert e < sr.TOL_ROLL, ("seeded stream against explicit normals", e, c)


def test_window_pop_repeats(eng, ctx):
    for c in sc.cases("window_pop")[:IDENTITY_CASES]:
        ref = sr.PREPARE["window_pop"](c)
        a, b = sr.run_window_pop(eng, ctx, c, ref), sr.run_window_pop(eng, ctx, c, ref)
        assert a["rmse"].tobytes() == b["rmse"].tobytes() and a["E"].tobytes() == b["E"].tobytes(), c
        if a["fd"] is not None:
            assert a["fd"][0].tobytes() == b["fd"][0].tobytes() and a["fd"][1].tobytes() == b["fd"][1].tobytes(), c
