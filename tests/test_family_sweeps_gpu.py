"""Shape sweeps over the five newer kernel families on the GPU: population rollouts, closed-loop rollouts, the Fossen and the Koopman
MPPI step, and the population window evaluator with fd_normal_eq.  Each family's own test file runs one hand-picked shape; here every
family runs the 48 cases of tests/sweep_cases.py (a hand-written corner list over every block edge, knot count, window and stride
rule, then seeded draws) in four slices, each case against the family's NumPy / long-double reference by the recipe of
tests/sweep_run.py: mixed error in long double against 1e-10 on every output, the soft-min update from the kernel's own costs at
1e-12, counts exact, a lane compared only where the reference itself is well-posed (tests/test_sweep_cases_cpu.py asserts on the CPU
that this leaves out at most 2 % of a case's lanes and never a whole case).  Then the exact identities the code promises, on the
first cases of each list.  A failure message carries the case dict: sweep_run.sweep_one(eng, ctx, case) reruns it alone.

The EDMDc families (lift, gram in its three entry forms, pinv_apply in both variants, the propagated and the linear multistep
evaluator, simulate_lifted) run their 32 cases each in four slices of 8, by the measures and bounds of tests/sweep_edmdc.py: Gram and
apply entries per entry against sum |terms| at 1e-12, x_hat per window and simulate rows per trajectory at 1e-10, the lift at 1e-13
absolute and relative to the reference's own gap."""
import numpy as np
import pytest

import mppi_ref as mr
import sweep_cases as sc
import sweep_edmdc as se
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
    if family in sc.EDMDC_FAMILIES:
        print(f"{family} slice {part}: {len(cases)} cases, worst kernel err {worst:.2e}, second figure (tests/sweep_edmdc.py: sweep_one) "
              f"{second:.2e}, worst reference gap {gap:.2e}, lanes left out {left}")
        return
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


# ------------------------------------------------------------------------------------------ EDMDc: the exact identities
def test_lift_repeats_and_splits(eng, ctx):
    """two identical calls give identical bytes; lifting N rows at once equals lifting them in two calls"""
    for c in sc.cases("lift")[:IDENTITY_CASES + 2]:
        ref = sr.PREPARE["lift"](c)
        a, b = se.run_lift(eng, ctx, c, ref), se.run_lift(eng, ctx, c, ref)
        assert a.tobytes() == b.tobytes(), c
        h = c["N"] // 2
        two = np.concatenate([eng.lift(ref["X"][:h], ref["C"], c["gamma"], ctx=ctx), eng.lift(ref["X"][h:], ref["C"], c["gamma"], ctx=ctx)])
        assert two.tobytes() == a.tobytes(), ("two calls", h, c)


def test_gram_repeats_and_accumulates(eng, ctx):
    """two identical calls give identical bytes; the device forms with accumulate over a split of the bags equal the one-call result
    to the family bound, in the family's measure"""
    cases = sc.cases("gram")
    dev = [c for c in cases if c["form"] != "host" and len(c["lens"]) > 1]
    for c in cases[:IDENTITY_CASES] + dev[:IDENTITY_CASES]:
        ref = sr.PREPARE["gram"](c)
        a, b = se.run_gram(eng, ctx, c, ref), se.run_gram(eng, ctx, c, ref)
        _same_bytes(a, b, c)
        if c["form"] != "host" and len(c["lens"]) > 1:
            one = se.run_gram(eng, ctx, c, ref, split=0)
            for s in range(1, len(c["lens"])):
                two = se.run_gram(eng, ctx, c, ref, split=s)
                d = max(float(se.measure(two[k], one[k].astype(se.L), ref["mag"][i]).max()) for i, k in enumerate(("GtG", "GtY")) if one[k] is not None)
                assert d < se.TOL_GRAM, ("accumulate over a split", s, d, c)


def test_pinv_apply_repeats(eng, ctx):
    for c in sc.cases("pinv_apply")[:IDENTITY_CASES]:
        ref = sr.PREPARE["pinv_apply"](c)
        a, b = se.run_pinv_apply(eng, ctx, c, ref), se.run_pinv_apply(eng, ctx, c, ref)
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes(), c


def test_multistep_repeats_and_a_short_u_is_the_padded_u(eng, ctx):
    """two identical calls give identical bytes; U one row shorter than X gives the bytes of the full U, for both evaluators"""
    cases = sc.cases("multistep")
    for c in cases[:IDENTITY_CASES] + [c for c in cases[IDENTITY_CASES:] if c["nw"] >= 1921 and c["H"] > 1][:1]:
        ref = sr.PREPARE["multistep"](c)
        a, b = se.run_multistep(eng, ctx, c, ref), se.run_multistep(eng, ctx, c, ref)
        short, full = se.run_multistep(eng, ctx, c, ref, short_u=True), se.run_multistep(eng, ctx, c, ref, short_u=False)
        for x, y in ((a, b), (short, full)):
            for (s1, x1), (s2, x2) in zip(x, y):
                assert s1 == s2 and x1.tobytes() == x2.tobytes(), c


def test_simulate_repeats_and_a_trajectory_alone_is_the_batch_row(eng, ctx):
    """two identical calls give identical bytes; a trajectory run alone equals its row of the batch bit for bit"""
    cases = sc.cases("simulate")
    for c in cases[:IDENTITY_CASES] + [c for c in cases[IDENTITY_CASES:] if c["nb"] > 256][:2]:
        ref = sr.PREPARE["simulate"](c)
        a, b = se.run_simulate(eng, ctx, c, ref), se.run_simulate(eng, ctx, c, ref)
        assert a.tobytes() == b.tobytes(), c
        for j in sorted({0, c["nb"] // 2, c["nb"] - 1} | {j for j in (127, 128, 255, 256) if j < c["nb"]}):
            alone = se.run_simulate(eng, ctx, c, ref, rows=slice(j, j + 1))
            assert alone.tobytes() == a[j:j + 1].tobytes(), ("trajectory alone", j, c)
