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
absolute and relative to the reference's own gap.

The unscented Kalman filter (ukf) and the QP of the Koopman linear MPC (lmpc) run 32 cases each in four slices of 8, by
tests/sweep_ukf_lmpc.py: a lane is a (candidate, recording) filter or a problem, every output at 1e-10, counts exact.  Their lists hold
what the hand-picked shapes of tests/test_ukf_gpu.py and tests/test_koopman_lmpc_gpu.py never execute: the three thruster filters
without a start lag, full and lone-wave blocks for every instantiation, T = 1, 12 updates per row and none at all; three and four rows
per lane of the QP, the second and third trip of its epilogue and of its u_apply loop, the scalar tail of the blocked W loop with W
from global memory, the shift and the residual stop beyond one row per lane.

The k-means families (colstats, kmeanspp, lloyd) run 32 cases each in four slices of 8, by tests/sweep_kmeans.py, against exact
references: column statistics per column against long double (1e-13 of mean |x|, 1e-12 of the variance); the seeding's indices equal
to a long-double restatement of scikit-learn's `_kmeans_plusplus` whose every round is decided, and to scikit-learn itself, the
centres X[idx] - mean bit for bit; Lloyd's n_iter, labels and centres (bit for bit) equal to the fixed-point restatement of
oracle/kmeans_numpy.py with a certified E-step, the inertia at 1e-10 against long double, the relocation count, the same bytes from
every public variant, both bounds rates and every operand form (host arrays, device rows with strides n, n + 1 and 40, on and off a
16-byte boundary), and kmeans_loop_info showing that the path a case is tagged for ran.  For these families the fourth figure of
sweep_one is the smallest decision gap of the reference, not a reference gap."""
import numpy as np
import pytest

import mppi_ref as mr
import sweep_cases as sc
import sweep_edmdc as se
import sweep_kmeans as sk
import sweep_run as sr
import sweep_ukf_lmpc as su

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
    left, least = 0, np.inf
    for c in cases:
        e, e2, out, g = sr.sweep_one(eng, ctx, c)
        worst, second, gap, left, least = max(worst, e), max(second, e2), max(gap, g), left + out, min(least, g)
    if family in sc.KMEANS_FAMILIES:
        print(f"{family} slice {part}: {len(cases)} cases, first figure {worst:.2e}, second {second:.2e} (tests/sweep_kmeans.py: sweep_one), smallest "
              f"decision gap {least:.2e}" + (" of R^2" if family == "lloyd" else " of its threshold"))
        return
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


# ------------------------------------------------------------------------------------------ ukf: the exact identities
UKF_KEYS = su.UKF_OUTS + ("lag",)


def _ukf_same(a, b, what, ia=(), ib=()):
    """a[k][ia] and b[k][ib] hold the same bits (NaN where NaN), for every output"""
    for k in UKF_KEYS:
        if a[k] is None or b[k] is None:
            assert a[k] is None and b[k] is None, (k, what)
        else:
            assert np.array_equal(a[k][ia], b[k][ib], equal_nan=True), (k, what)


def test_ukf_repeats_and_candidates_and_recordings_alone(eng, ctx):
    """two calls give equal bytes; candidate j equals the P = 1 call; a recording run alone equals its row of the batch bit for bit:
    B = 4 and 8 (every wave slot of full blocks), B = 5 (the lone wave of a ragged block), B = 1"""
    cases = sc.cases("ukf")[:IDENTITY_CASES]
    assert {c["B"] for c in cases} == {4, 5, 8, 1} and any(c["P"] == 3 and c["nrec"] == 3 for c in cases)
    for c in cases:
        ref = sr.PREPARE["ukf"](c)
        a = su.run_ukf(eng, ctx, c, ref)
        _ukf_same(a, su.run_ukf(eng, ctx, c, ref), ("repeat", c))
        for j in range(c["P"]):
            _ukf_same(su.run_ukf(eng, ctx, c, ref, cand=slice(j, j + 1)), a, ("candidate alone", j, c), (0,), (j,))
        for b in range(c["B"]):
            _ukf_same(su.run_ukf(eng, ctx, c, ref, rec=slice(b, b + 1)), a, ("recording alone", b, c), (slice(None), 0), (slice(None), b))


def test_ukf_split_at_every_row_and_resumed(eng, ctx):
    """T = 12 rows = T1 + (12 - T1) rows resumed from (xT, PT, lag_io), for every T1 = 1 .. 11: the unbroken bits in every row
    output, xT, PT and lag_io; the update counts add up exactly and the log-likelihoods to rounding.  A thruster case with a start
    lag and a wrench case (without a lag_io the thruster filter cannot be resumed: it restarts from a zero lag)."""
    corners = sc.corners("ukf")
    picked = [[c for c in corners if c["T"] == 12 and c["model"] == m and (c["lag"] or m == 1) and c["P"] > 1][0] for m in (0, 1)]
    for c in picked:
        ref = sr.PREPARE["ukf"](c)
        a = su.run_ukf(eng, ctx, c, ref)
        assert np.all(a["info"][..., 2] == -1), c
        for T1 in range(1, c["T"]):
            h = su.run_ukf(eng, ctx, c, ref, rows=slice(0, T1))
            parts = [su.run_ukf(eng, ctx, c, ref, cand=slice(j, j + 1), rows=slice(T1, None), x0=h["xT"][j], P0=h["PT"][j],
                                lag=None if h["lag"] is None else h["lag"][j:j + 1]) for j in range(c["P"])]       # x0 and P0 are shared: one by one
            for k in ("xf", "pstd", "innov"):
                both = np.concatenate([h[k], np.concatenate([p[k] for p in parts])], axis=2)
                assert np.array_equal(both, a[k], equal_nan=True), (k, T1, c)
            for k in ("xT", "PT") + (("lag",) if a["lag"] is not None else ()):
                assert np.array_equal(np.concatenate([p[k] for p in parts]), a[k]), (k, T1, c)
            info = np.concatenate([p["info"] for p in parts])
            assert np.array_equal(h["info"][..., 1] + info[..., 1], a["info"][..., 1]), (T1, c)
            assert np.max(np.abs(h["info"][..., 0] + info[..., 0] - a["info"][..., 0]) / np.maximum(1.0, np.abs(a["info"][..., 0]))) < 1e-12, (T1, c)


def test_ukf_lag_io_is_rollout_pops(eng, ctx):
    """lag_io out is rollout_pop's lag_io on the same commands, from the case's start lag and from a zero one: Euler, RK4 with the
    lag per call and per step"""
    import fossen_vehicles as fv
    corners = [c for c in sc.corners("ukf") if c["lag"]]
    picked = [[c for c in corners if (c["integ"], c["lag_mode"]) == v][0] for v in (("euler", 0), ("rk4", 0), ("rk4", 1))]
    for c in picked:
        ref = sr.PREPARE["ukf"](c)
        for lag in (ref["lag"], np.zeros_like(ref["lag"])):
            f = su.run_ukf(eng, ctx, c, ref, lag=lag)
            pop = eng.rollout_pop(0, c["integ"], [fv.params(n) for n in c["names"]], np.zeros((c["B"], 12)), ref["U"], su.DT_UKF, lag=lag,
                                  lag_mode=c["lag_mode"], store=False, ctx=ctx)
            assert np.all(f["info"][..., 2] == -1) and np.array_equal(f["lag"], pop["lag"]), c


# ------------------------------------------------------------------------------------------ lmpc: the exact identities
LMPC_KEYS = ("U_nom", "y", "u_apply", "pred", "info")


def _lmpc_same(a, b, keys=LMPC_KEYS, ia=slice(None), ib=slice(None)):
    return all((a[k] is None and b[k] is None) or a[k][ia].tobytes() == b[k][ib].tobytes() for k in keys)


def _lmpc_of_rows(nq, **want):
    """the first corner with nq rows per lane (W from global memory from nq = 2 on) that holds `want`"""
    return [c for c in sc.corners("lmpc") if sc.lmpc_rows(c)[0] == nq and all(c[k] == v for k, v in want.items())][0]


def test_lmpc_repeats_and_a_problem_alone_is_the_batch_row(eng, ctx):
    """two calls give equal bytes; a problem run alone equals its row of the batch in every wave slot: one case per rows-per-lane
    count and W source, each with at least four problems"""
    corners = sc.corners("lmpc")
    picked = []
    for rows in ((1, True), (2, True), (2, False), (3, False), (4, False), (5, False)):
        fit = [c for c in corners if sc.lmpc_rows(c) == rows and c["nb"] >= 4]
        picked.append(([c for c in fit if c["iters"] == 40] or fit)[0])
    for c in corners[:IDENTITY_CASES] + picked:
        ref = sr.PREPARE["lmpc"](c)
        a = su.run_lmpc(eng, ctx, c, ref)
        assert _lmpc_same(a, su.run_lmpc(eng, ctx, c, ref)), ("repeat", c)
        for b in range(c["nb"]):
            assert _lmpc_same(su.run_lmpc(eng, ctx, c, ref, sel=slice(b, b + 1)), a, ib=slice(b, b + 1)), ("problem alone", b, c)


@pytest.mark.parametrize("nq", [3, 4, 5])
def test_lmpc_resume_and_shift_beyond_two_rows_per_lane(eng, ctx, nq):
    """iters = a, then iters = b on the returned (U_nom, y), is one call with iters = a + b; shift = 1 moves z and y one knot forward
    with the last knot repeated and changes nothing else (tests/test_koopman_lmpc_gpu.py: test_resume, test_shift, which run one
    and two rows per lane)"""
    c = _lmpc_of_rows(nq, iters=40, tol=0.0)
    ref = sr.PREPARE["lmpc"](c)
    y0 = np.zeros_like(ref["U"])
    for a, b in ((1, 1), (17, 23)):
        first = su.run_lmpc(eng, ctx, c, ref, y=y0, iters=a, shift=False)
        second = su.run_lmpc(eng, ctx, c, ref, U_nom=first["U_nom"], y=first["y"], iters=b, shift=False)
        whole = su.run_lmpc(eng, ctx, c, ref, y=y0, iters=a + b, shift=False)
        assert _lmpc_same(second, whole, ("U_nom", "y", "u_apply", "pred")), (a, b, c)
        assert np.array_equal(second["info"][:, [0, 2, 3, 5]], whole["info"][:, [0, 2, 3, 5]]), (a, b, c)
        assert np.all(second["info"][:, 4] == b) and np.all(whole["info"][:, 4] == a + b), (a, b, c)
    plain, moved = su.run_lmpc(eng, ctx, c, ref, y=y0, shift=False), su.run_lmpc(eng, ctx, c, ref, y=y0, shift=True)
    for key in ("U_nom", "y"):
        assert np.array_equal(moved[key], np.concatenate([plain[key][:, 1:], plain[key][:, -1:]], axis=1)), (key, c)
    assert _lmpc_same(plain, moved, ("u_apply", "pred", "info")), c


# ------------------------------------------------------------------------------------------ k-means: the exact identities
@pytest.fixture(scope="module", autouse=True)
def _kmeans_contexts():
    yield
    sk.close_contexts()


def _lloyd_same(a, b):
    return a["n_iter"] == b["n_iter"] and a["C"].tobytes() == b["C"].tobytes() and a["labels"].tobytes() == b["labels"].tobytes()


def test_lloyd_repeats_and_resumes(eng, ctx):
    """two identical calls give identical bytes; max_iter = a + b equals a run of a followed by a run of b from the returned centres
    (centres, labels and the total n_iter: the loop carries no state besides the centres), on cases that do not stop early"""
    cases = sc.cases("lloyd")
    picked = cases[:IDENTITY_CASES] + [c for c in cases[IDENTITY_CASES:] if c["stop"] == "max_iter" and c["max_iter"] >= 3 and c["init"] == "rows"][:IDENTITY_CASES]
    resumed = 0
    for c in picked:
        ref = sr.PREPARE["lloyd"](c)
        lc = sk.lloyd_ctx(ctx)
        whole = sk.lloyd_once(eng, lc, c, ref, c["form"])
        assert _lloyd_same(whole, sk.lloyd_once(eng, lc, c, ref, c["form"])), ("repeat", c)
        if c["stop"] == "max_iter" and c["max_iter"] >= 2 and not ref["nreloc"]:
            for a in range(1, c["max_iter"]):
                first = sk.lloyd_once(eng, lc, c, ref, c["form"], max_iter=a)
                second = sk.lloyd_once(eng, lc, c, ref, c["form"], max_iter=c["max_iter"] - a, C0=first["C"])
                assert first["n_iter"] == a and first["n_iter"] + second["n_iter"] == whole["n_iter"], (a, c)
                assert second["C"].tobytes() == whole["C"].tobytes() and second["labels"].tobytes() == whole["labels"].tobytes(), ("resumed after", a, c)
                resumed += 1
    assert resumed >= 4


def test_kmeans_centers_dev_on_a_strided_tensor_is_the_contiguous_call(eng, ctx):
    """kmeans_centers_dev (column statistics, seeding, Lloyd) on rows n + 1 and 40 doubles apart, on and off a 16-byte boundary,
    equals the same call on the contiguous copy: centres bit for bit, inertia, n_iter"""
    done = 0
    for c in sc.cases("lloyd"):
        if c["init"] != "rows" or not (64 <= c["N"] <= 16385) or c["k"] > 128 or done == IDENTITY_CASES:
            continue
        X = sk.lloyd_inputs(c)[0]
        want = None
        for form in ("dev", "dev_stride", "block_odd", "block_even"):
            C, inertia, n_iter = eng.kmeans_centers_dev(sk.operand(eng, ctx, X, form), c["k"], max_iter=8, ctx=ctx)
            got = (C.cpu().numpy().tobytes(), inertia, n_iter)
            want = want or got
            assert got == want, (form, n_iter, want[2], c)
        done += 1
    assert done == IDENTITY_CASES
