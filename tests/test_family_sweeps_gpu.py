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
sweep_one is the smallest decision gap of the reference, not a reference gap.

The unscented RTS smoother (smooth) runs 32 cases in four slices of 8, by tests/sweep_smooth.py: a lane is a (candidate, recording)
problem; every case runs as tape filter plus backward pass (with the case's terminal pair), as one brov_ukf_smooth call and as a
chunked one; xs and pstd_s in the mixed error, Ps, Ps0 and the tape's Pf and Pp as |dP_ij| / sqrt(P_ii P_jj), the tape's C as
|dC_ab| / sqrt(Pf_aa Pp_bb), all at 1e-10 with the reference's own gap below a tenth of it; counts, nrows and the bit identities
between the three runs exact.  Over the eight problems of tests/test_ukf_smooth_gpu.py (P = 2, T = 12, B = 3 or 5, every thruster
case with a start lag, chunks 4 + 1 only) the list adds the three tape filters without a start lag, T = 1, 2 and 3 with and without a
terminal pair, P = 1 and 3, B = 1, 4, 8, 9 and 13, a noise record per candidate in chunks, rows with 12 updates and recordings with
none, r = +inf on 0 and 3 components, q = 0, middle chunks and a ragged second chunk, a budget rounded down to whole blocks, and strict
subsets of the outputs.  The identities after it: repeats and problems alone, a split at every row, failures in the second and third
chunk, a terminal pair given to a short prefix, an nrows edited by the caller (include/brov2.h: the clamp) and the life of the ctx's
tape buffer.

The filter and the smoother of the quaternion model (ukf_quat, smooth_quat) run 32 cases each in four slices of 8, by
tests/sweep_quat.py, with the measures, the bound 1e-10 and the three runs per case of the smooth family and |e_w| > 0.5 in every
[-] in place of the wrap margin.  Over the five problems of tests/ukf_quat_cases.py (P = 2, T = 12, B = 3 or 5, chunks 4 + 1, starts
near level or near vertical, Euler in one of five) the lists add P = 1 and 3 (blockIdx.y = 2 reads its own noise record), T = 1, 2 and
3 with and without a terminal pair, B = 1, 4, 8, 9 and 13, chunks 4 + 4, 4 + 4 + 1, 8 + 5 and 4 + 4 + 4 + 1, a budget of a block and a
half, a noise record per candidate in chunks under both integrators, strict subsets of the outputs with and without chunks, rows
with 12 updates and recordings with none, r = +inf on no component and on three with an attitude component among them, q = 0,
starts anywhere on the sphere (half of them with q_w < 0), inverted with the yaw at +-(pi - 0.05), and an attitude block of P0 of
sigma 0.3 in chart units.  Largest kernel error per slice against the 9e-14 of the pinned cases: ukf_quat 5.5e-14, 2.0e-13, 6.8e-14,
9.0e-14; smooth_quat 2.1e-13, 5.7e-13, 5.1e-12, 7.5e-12 (the last two on wide, inverted starts whose own float64-to-long-double gap
is 4.6e-12 and 5.0e-12); no lane left out.  The identities after them: repeats and problems alone with a noise record per
candidate, a split at every row from a start on the sphere, the three stopping conditions in the second and third chunk of P = 3,
a terminal pair given to a short prefix, and both smoothers alternating on one ctx's tape buffer."""
import numpy as np
import pytest

import mppi_ref as mr
import sweep_cases as sc
import sweep_edmdc as se
import sweep_kmeans as sk
import sweep_quat as sq
import sweep_run as sr
import sweep_smooth as ss
import sweep_ukf_lmpc as su
import ukf_cases as uc

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
    if family == "smooth":
        print(f"{family} slice {part}: {len(cases)} cases, worst kernel err {worst:.2e} (bound {ss.TOL:.0e}; two calls and one call, smoother, tape "
              f"and filter outputs), worst reference gap {gap:.2e}, lanes left out {left}")
        return
    if family in sq.PREPARE:
        print(f"{family} slice {part}: {len(cases)} cases, worst kernel err {worst:.2e} (bound {sq.TOL:.0e}; " +
              ("two calls and one call, smoother, tape and filter outputs" if family == "smooth_quat" else "every filter output") +
              f"), worst reference gap {gap:.2e}, lanes left out {left}")
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


# ------------------------------------------------------------------------------------------ smooth: the exact identities
SM_ALL = ss.F_OUTS + ss.S_OUTS + ("lag",)
SM_TAPE = SM_ALL + ss.TAPE_KEYS


def _smooth_corner(**want):
    """the first corner of the smooth list that holds `want` (a callable value is a predicate on the field)"""
    return [c for c in sc.corners("smooth") if all(v(c[k]) if callable(v) else c[k] == v for k, v in want.items())][0]


@pytest.mark.parametrize("model", [0, 1])
def test_smooth_repeats_and_problems_alone(eng, ctx, model):
    """a thruster case without a start lag (TRACK = false) and a wrench case, 12 rows, run on their first B = 4, 8, 5 and 1 recordings:
    two calls give equal bytes; candidate j alone and recording b alone carry the bits they have in the batch, in every filter and
    smoother output and in the tape; the one-call smoother says the same"""
    c = _smooth_corner(model=model, lag=False, B=8, T=12, P=lambda v: v > 1)
    ins = su.ukf_inputs(c)
    for B in (4, 8, 5, 1):
        rec = slice(0, B)
        a = ss.two_step(eng, ctx, c, ins, rec=rec)
        assert np.all(a["nrows"] == c["T"]) and np.all(a["sinfo"][..., 0] == -1), (B, c)
        ss.same(ss.two_step(eng, ctx, c, ins, rec=rec), a, SM_TAPE, ("repeat", B, c))
        one = ss.smooth(eng, ctx, c, ins, rec=rec)
        ss.same(one, a, SM_ALL, ("one call", B, c))
        ss.same(ss.smooth(eng, ctx, c, ins, rec=rec), one, SM_ALL, ("one call, repeated", B, c))
        for j in range(c["P"]):
            ss.same(ss.two_step(eng, ctx, c, ins, cand=slice(j, j + 1), rec=rec), a, SM_TAPE, ("candidate alone", j, B, c), (0,), (j,))
        for b in range(B):
            ss.same(ss.two_step(eng, ctx, c, ins, rec=slice(b, b + 1)), a, SM_TAPE, ("recording alone", b, B, c), (slice(None), 0), (slice(None), b))
            ss.same(ss.smooth(eng, ctx, c, ins, rec=slice(b, b + 1)), a, SM_ALL, ("recording alone, one call", b, B, c), (slice(None), 0), (slice(None), b))


@pytest.mark.parametrize("model", [0, 1])
def test_smooth_split_at_every_row(eng, ctx, model):
    """T = 12 rows = T1 + (12 - T1), for every T1 = 1 .. 11: filter rows 0 .. T1 - 1 with a tape, smooth rows T1 .. 11 from (xT, PT,
    lag_io), then the backward pass over the first span with the second's (xs[0], Ps0) as its terminal pair: the bits of the unbroken
    call in xs, pstd_s, Ps and Ps0.  A thruster case with a start lag and a wrench case, more than one candidate each."""
    c = _smooth_corner(model=model, lag=model == 0, T=12, P=lambda v: v > 1, measured="std")
    ins = su.ukf_inputs(c)
    whole = ss.smooth(eng, ctx, c, ins)
    assert np.all(whole["info"][..., 2] == -1) and np.all(whole["sinfo"][..., 0] == -1), c
    for T1 in range(1, c["T"]):
        for j in range(c["P"]):                                      # x0 and P0 are shared by the candidates: resume one by one
            cj = slice(j, j + 1)
            first = ss.call(eng.ukf_filter, ctx, c, ins, cand=cj, rows=slice(0, T1), extra=dict(tape=True))
            second = ss.smooth(eng, ctx, c, ins, cand=cj, rows=slice(T1, None), x0=first["xT"][0], P0=first["PT"][0], lag=first["lag"])
            back = eng.ukf_rts(first["xf"], first["tape"], first["nrows"], terminal=(second["xs"][:, :, 0], second["Ps0"]), ctx=ctx)
            for k in ss.ROWS:
                assert np.array_equal(np.concatenate([back[k], second[k]], axis=2), whole[k][cj]), (k, T1, j, c)
            assert np.array_equal(back["Ps0"], whole["Ps0"][cj]), (T1, j, c)


def _nan_like(got, want):
    return np.array_equal(np.isnan(got), np.isnan(want))


def test_smooth_chunking_with_failures(eng, ctx):
    """P = 3 candidates with a noise record each, B = 9 recordings, a tape budget of 4: chunks 4 + 4 + 1.  The corner of the list with
    12 rows instead of its 3 (the row budget of the references does not bind here: the reference runs on the failing recording
    alone).  The three conditions under which a filter stops, by the mechanisms of tests/test_ukf_smooth_gpu.py:
    test_valid_prefix_in_every_wave_slot -- an indefinite P0 under a row 0 without measurements (n = 1), an infinite command at row 6
    (n = 7), P0[i][i] = -2 r[i] on the last measured component of row 0 (n = 0; the largest r[i] of the candidates) -- in recording 5
    (second chunk, wave slot 1, where the chunk-local index of the tape and of nrows is not the output row) and in recording 8 (the
    lone recording of the third chunk): nrows, the NaN pattern of the rows and of the tape, info[2] and sinfo are the reference's; the
    valid prefix is the problem cut to n rows, bit for bit; every other problem carries the bits of the clean call; the chunked
    call equals the one-chunk call and the two calls."""
    c3 = _smooth_corner(P=3, nrec=3, B=9, chunk=4, measured="std", terminal=False)
    c = dict(c3, T=12)
    assert sc.smooth_chunks(c) == [4, 4, 1]
    ins = su.ukf_inputs(c)
    P, B, T = c["P"], c["B"], c["T"]
    Y0 = ins["Y"].copy()
    Y0[:, 0] = np.nan
    clean = ss.two_step(eng, ctx, c, ins)
    clean_y0 = ss.two_step(eng, ctx, c, ins, Y=Y0)
    assert np.all(clean["nrows"] == T) and np.all(clean_y0["nrows"] == T) and np.all(clean["sinfo"][..., 0] == -1), c
    rmax = np.max([k.r for k in ins["cfgs"]], axis=0)
    for b in (5, 8):
        P0a = ins["P0"].copy()
        P0a[b, 1, 0] = 2.0 * P0a[b, 0, 0]                            # (the upper triangle is NaN: never read)
        U = ins["U"].copy()
        U[b, 6, 0] = np.inf
        comp = [k for k in range(12) if not np.isnan(ins["Y"][b, 0, k]) and np.isfinite(rmax[k])][-1]
        P0c = ins["P0"].copy()
        P0c[b, comp, comp] = -2.0 * rmax[comp]
        for n, stage, base, kw in ((1, 2, clean_y0, dict(P0=P0a, Y=Y0)), (7, 2, clean, dict(U=U)), (0, 1, clean, dict(P0=P0c))):
            what = (b, n, c)
            got = ss.two_step(eng, ctx, c, ins, **kw)
            with np.errstate(all="ignore"):
                o = ss.ref_smooth(c, dict(ins, **kw), rec=slice(b, b + 1))
            assert np.all(o["nrows"] == n) and np.all(o["info"][..., 2] == (n if stage == 1 else n - 1)), ("the reference stops there too", what)
            assert np.array_equal(got["nrows"][:, b], o["nrows"][:, 0]) and np.array_equal(got["info"][:, b, 2], o["info"][:, 0, 2]), what
            for k in ss.ROWS + ("tape", "xf", "pstd", "Ps0"):
                assert _nan_like(got[k][:, b], o[k][:, 0]), (k, what)
            assert np.array_equal(got["sinfo"][:, b, 0], o["sinfo"][:, 0, 0], equal_nan=True), what
            assert uc.err(got["sinfo"][:, b, 1], o["sinfo"][:, 0, 1]) < ss.TOL, what
            for k in ss.ROWS:
                assert np.isnan(got[k][:, b, n:]).all() and np.isfinite(got[k][:, b, :n]).all(), (k, what)
            if n:
                cut = ss.smooth(eng, ctx, c, ins, rows=slice(0, n), **{k: (v[:, :n] if k in ("U", "Y") else v) for k, v in kw.items()})
                for k in ss.ROWS:
                    assert np.array_equal(got[k][:, b, :n], cut[k][:, b]), (k, "the valid prefix", what)
                assert np.array_equal(got["Ps0"][:, b], cut["Ps0"][:, b]) and np.array_equal(got["sinfo"][:, b], cut["sinfo"][:, b]), what
            for other in range(B):
                if other != b:
                    ss.same(got, base, SM_TAPE, ("another problem, with a failure in", other, what), (slice(None), other), (slice(None), other))
            one = ss.smooth(eng, ctx, c, ins, **kw)
            ss.same(one, got, SM_ALL, ("one chunk against two calls", what))
            ss.same(ss.smooth(eng, ctx, c, ins, tape_bytes=sc.smooth_tape_bytes(c), **kw), one, SM_ALL, ("chunks 4 + 4 + 1 against one chunk", what))


def test_smooth_terminal_pair_and_a_short_prefix(eng, ctx):
    """a terminal pair (sweep_smooth.terminal_pair, from the filter's own xT and PT where they are finite) in a call in which one
    problem stopped early: that problem is the call without a pair, bit for bit (the law ignores the pair when n < T); the problems
    with n = T move by more than 1e3 TOL.  The upper triangle of Ps_T is NaN."""
    c = _smooth_corner(B=4, T=12, P=lambda v: v > 1, measured="std")
    ins = su.ukf_inputs(c)
    b, n = 2, 7
    U = ins["U"].copy()
    U[b, n - 1, 0] = np.inf
    f = ss.call(eng.ukf_filter, ctx, c, ins, extra=dict(tape=True), U=U)
    want_n = np.full((c["P"], c["B"]), float(c["T"]))
    want_n[:, b] = n
    assert np.array_equal(f["nrows"], want_n), (f["nrows"], c)
    clean = ss.call(eng.ukf_filter, ctx, c, ins)
    pair = ss.terminal_pair(c, dict(xT=np.where(np.isnan(f["xT"]), clean["xT"], f["xT"]), PT=np.where(np.isnan(f["PT"]), clean["PT"], f["PT"])))
    assert np.isnan(pair[1][..., 0, 1]).all() and np.isfinite(pair[0]).all()
    without = eng.ukf_rts(f["xf"], f["tape"], f["nrows"], ctx=ctx)
    with_pair = eng.ukf_rts(f["xf"], f["tape"], f["nrows"], terminal=pair, ctx=ctx)
    ss.same(with_pair, without, ss.S_OUTS, ("a pair given to a short prefix", c), (slice(None), b), (slice(None), b))
    assert np.isfinite(with_pair["xs"][:, b, :n]).all() and np.isnan(with_pair["xs"][:, b, n:]).all(), c
    for other in range(c["B"]):
        if other != b:
            assert np.all(with_pair["sinfo"][:, other, 0] == -1) and np.isfinite(with_pair["Ps"][:, other]).all(), (other, c)
            for j in range(c["P"]):
                moved = uc.err(with_pair["xs"][j, other], without["xs"][j, other])
                assert moved > 1e3 * ss.TOL, ("the pair must move a complete problem", moved, j, other, c)
    optional = eng.ukf_rts(f["xf"], f["tape"], f["nrows"], terminal=pair, want=(), ctx=ctx)      # a pair with every optional output NULL
    assert all(v is None for v in optional.values())
    ss.same(eng.ukf_rts(f["xf"], f["tape"], f["nrows"], terminal=pair, want=("sinfo",), ctx=ctx), with_pair, ("sinfo",), ("sinfo alone", c))


def test_smooth_nrows_edited_by_the_caller(eng, ctx):
    """include/brov2.h: the tape and nrows are plain arrays, n = nrows clamped to 0 .. T, the fraction dropped, NaN as 0.  On a clean
    T = 12 tape of B = 4, nrows of one problem in turn (every wave slot) is NaN, -inf, -1, 0, 0.5: every output NaN, sinfo included;
    1: row 0 with the filter's bits, sinfo = (-1, +inf); 6.7: the problem cut to 6 rows; 12, 17, +inf: the clean bits.  The other
    three problems never change."""
    c = _smooth_corner(B=4, T=12, P=lambda v: v > 1, measured="std")
    ins = su.ukf_inputs(c)
    T = c["T"]
    clean = ss.two_step(eng, ctx, c, ins)
    assert np.all(clean["nrows"] == T), c
    Pf = ss.us.tape_fields(clean["tape"])["Pf"]
    cut6 = ss.smooth(eng, ctx, c, ins, rows=slice(0, 6))
    for i, v in enumerate((np.nan, -np.inf, -1.0, 0.0, 0.5, 1.0, 6.7, 12.0, 17.0, np.inf)):
        b = i % c["B"]
        nrows = clean["nrows"].copy()
        nrows[:, b] = v
        got = eng.ukf_rts(clean["xf"], clean["tape"], nrows, ctx=ctx)
        what = (v, b, c)
        n = 0 if not v >= 1 else int(min(v, T))
        for k in ss.ROWS:
            assert np.isnan(got[k][:, b, n:]).all() and np.isfinite(got[k][:, b, :n]).all(), (k, what)
        if n == 0:
            assert np.isnan(got["Ps0"][:, b]).all() and np.isnan(got["sinfo"][:, b]).all(), what
        elif n == 1:
            assert np.array_equal(got["xs"][:, b, 0], clean["xf"][:, b, 0]) and np.array_equal(got["pstd_s"][:, b, 0], clean["pstd"][:, b, 0]), what
            assert np.array_equal(got["Ps"][:, b, 0], Pf[:, b, 0]) and np.array_equal(got["Ps0"][:, b], Pf[:, b, 0]), what
            assert np.all(got["sinfo"][:, b, 0] == -1) and np.all(got["sinfo"][:, b, 1] == np.inf), what
        elif n == 6:
            for k in ss.ROWS:
                assert np.array_equal(got[k][:, b, :6], cut6[k][:, b]), (k, what)
            assert np.array_equal(got["Ps0"][:, b], cut6["Ps0"][:, b]) and np.array_equal(got["sinfo"][:, b], cut6["sinfo"][:, b]), what
        else:
            ss.same(got, clean, ss.S_OUTS, ("the clean bits", what), (slice(None), b), (slice(None), b))
        for other in range(c["B"]):
            if other != b:
                ss.same(got, clean, ss.S_OUTS, ("another problem", other, what), (slice(None), other), (slice(None), other))


def test_smooth_tape_buffer_life():
    """the ctx's tape buffer grows, shrinks below half and grows again between calls: every call gives the bits it gives on a fresh
    ctx"""
    from bluerov2_dynamics_amd import _lib, engine
    large, small = _smooth_corner(B=13, T=12), _smooth_corner(B=1, T=1)
    assert 2 * large["P"] * large["B"] * large["T"] > 8 * small["P"] * small["B"] * small["T"]
    ins = {id(c): su.ukf_inputs(c) for c in (large, small)}
    fresh = {}
    for c in (large, small):
        one = _lib.Context(0)
        try:
            fresh[id(c)] = ss.smooth(engine, one, c, ins[id(c)])
        finally:
            one.close()
    kept = _lib.Context(0)
    try:
        for step, c in enumerate((large, small, large, small, large)):
            ss.same(ss.smooth(engine, kept, c, ins[id(c)]), fresh[id(c)], SM_ALL, ("call", step, "on one ctx", c))
            if step == 2:                                            # and a chunked call on the grown buffer, which needs less than half of it
                ss.same(ss.smooth(engine, kept, c, ins[id(c)], tape_bytes=c["P"] * 4 * c["T"] * sc.SMOOTH_RECORD), fresh[id(c)], SM_ALL, ("chunked", c))
    finally:
        kept.close()


# ------------------------------------------------------------------------------------------ ukf_quat, smooth_quat: the exact identities
SQ_ALL = sq.F_OUTS + sq.S_OUTS
SQ_TAPE = SQ_ALL + sq.TAPE_KEYS


def _quat_corner(**want):
    """the first corner of the smooth_quat list that holds `want` (a callable value is a predicate on the field)"""
    return [c for c in sc.corners("smooth_quat") if all(v(c[k]) if callable(v) else c[k] == v for k, v in want.items())][0]


@pytest.mark.parametrize("integ", ["euler", "rk4"])
def test_smooth_quat_repeats_and_problems_alone(eng, ctx, integ):
    """a corner with a noise record per candidate, P > 1 and 12 rows, run on its first B = 4, 8, 5 and 1 recordings: two calls give equal
    bytes; candidate j alone (blockIdx.y = 0 with the record of candidate j) and recording b alone carry the bits they have in the
    batch, in every filter and smoother output and in the tape; the one-call smoother says the same"""
    c = _quat_corner(integ=integ, T=12, B=lambda v: v >= 8, P=lambda v: v > 1, nrec=lambda v: v > 1)
    assert c["nrec"] == c["P"]
    ins = sq.quat_inputs(c)
    for B in (4, 8, 5, 1):
        rec = slice(0, B)
        a = sq.two_step(eng, ctx, c, ins, rec=rec)
        assert np.all(a["nrows"] == c["T"]) and np.all(a["sinfo"][..., 0] == -1), (B, c)
        sq.same(sq.two_step(eng, ctx, c, ins, rec=rec), a, SQ_TAPE, ("repeat", B, c))
        one = sq.smooth(eng, ctx, c, ins, rec=rec)
        sq.same(one, a, SQ_ALL, ("one call", B, c))
        sq.same(sq.smooth(eng, ctx, c, ins, rec=rec), one, SQ_ALL, ("one call, repeated", B, c))
        for j in range(c["P"]):
            sq.same(sq.two_step(eng, ctx, c, ins, cand=slice(j, j + 1), rec=rec), a, SQ_TAPE, ("candidate alone", j, B, c), (0,), (j,))
        for b in range(B):
            sq.same(sq.two_step(eng, ctx, c, ins, rec=slice(b, b + 1)), a, SQ_TAPE, ("recording alone", b, B, c), (slice(None), 0), (slice(None), b))
            sq.same(sq.smooth(eng, ctx, c, ins, rec=slice(b, b + 1)), a, SQ_ALL, ("recording alone, one call", b, B, c), (slice(None), 0), (slice(None), b))


@pytest.mark.parametrize("attitude", ["sphere", "level"])
def test_smooth_quat_split_at_every_row(eng, ctx, attitude):
    """T = 12 rows = T1 + (12 - T1), for every T1 = 1 .. 11: filter rows 0 .. T1 - 1 with a tape, smooth rows T1 .. 11 from (xT, PT),
    then the backward pass over the first span with the second's (xs[0], Ps0) as its terminal pair: the bits of the unbroken call in
    xs, pstd_s, Ps and Ps0.  A start anywhere on the sphere and a level one, more than one candidate each."""
    c = _quat_corner(attitude=attitude, T=12, P=lambda v: v > 1, measured="std")
    ins = sq.quat_inputs(c)
    whole = sq.smooth(eng, ctx, c, ins)
    assert np.all(whole["info"][..., 2] == -1) and np.all(whole["sinfo"][..., 0] == -1), c
    for T1 in range(1, c["T"]):
        for j in range(c["P"]):                                      # x0 and P0 are shared by the candidates: resume one by one
            cj = slice(j, j + 1)
            first = sq.call(eng.ukf_filter_quat, ctx, c, ins, cand=cj, rows=slice(0, T1), extra=dict(tape=True))
            second = sq.smooth(eng, ctx, c, ins, cand=cj, rows=slice(T1, None), x0=first["xT"][0], P0=first["PT"][0])
            back = eng.ukf_rts_quat(first["xf"], first["tape"], first["nrows"], terminal=(second["xs"][:, :, 0], second["Ps0"]), ctx=ctx)
            for k in sq.ROWS:
                assert np.array_equal(np.concatenate([back[k], second[k]], axis=2), whole[k][cj]), (k, T1, j, c)
            assert np.array_equal(back["Ps0"], whole["Ps0"][cj]), (T1, j, c)


def _measured_component(ins, b, rmax):
    """the last error component that row 0 of recording b measures with a finite r"""
    y = ins["Y"][b, 0]
    seen = [not np.isnan(y[i]) for i in range(3)] + [not np.isnan(y[3:7]).any()] * 3 + [not np.isnan(y[i + 1]) for i in range(6, 12)]
    return [k for k in range(12) if seen[k] and np.isfinite(rmax[k])][-1]


def test_smooth_quat_chunking_with_failures(eng, ctx):
    """P = 3 candidates with a noise record each, B = 9 recordings, a tape budget of one block: chunks 4 + 4 + 1.  The corner of the
    list with 12 rows instead of its 3 (the row budget of the references does not bind here: the reference runs on the failing
    recording alone).  The three conditions under which a filter stops, by the mechanisms of tests/test_ukf_quat_smooth_gpu.py and
    tests/test_ukf_quat_gpu.py -- a measured quaternion of zeros at row 3 (stage 1 fails before any update: n = 3), an infinite
    command at row 6 (n = 7), P0[i][i] = -2 r[i] on the last measured component of row 0 (n = 0; the largest r[i] of the candidates)
    -- in recording 5 (second chunk, wave slot 1, where the chunk-local index of the tape and of nrows is not the output row) and in
    recording 8 (the lone recording of the third chunk): nrows, the NaN pattern of the rows and of the tape, info[2] and sinfo are the
    reference's; the valid prefix is the problem cut to n rows, bit for bit; every other problem carries the bits of the clean
    call; the chunked call equals the one-chunk call and the two calls.  These are numerical conditions of the input, which the
    kernels detect and report."""
    c3 = _quat_corner(P=3, nrec=3, B=9, chunk=1, measured="std", terminal=False)
    c = dict(c3, T=12)
    assert sc.smooth_quat_chunks(c) == [4, 4, 1]
    ins = sq.quat_inputs(c)
    P, B, T = c["P"], c["B"], c["T"]
    clean = sq.two_step(eng, ctx, c, ins)
    assert np.all(clean["nrows"] == T) and np.all(clean["sinfo"][..., 0] == -1), c
    rmax = np.max([k.r for k in ins["cfgs"]], axis=0)
    for b in (5, 8):
        Yz = ins["Y"].copy()
        Yz[b, 3, 3:7] = 0.0
        U = ins["U"].copy()
        U[b, 6, 0] = np.inf
        comp = _measured_component(ins, b, rmax)
        P0c = ins["P0"].copy()
        P0c[b, comp, comp] = -2.0 * rmax[comp]
        for n, stage, kw in ((3, 1, dict(Y=Yz)), (7, 2, dict(U=U)), (0, 1, dict(P0=P0c))):
            what = (b, n, c)
            got = sq.two_step(eng, ctx, c, ins, **kw)
            with np.errstate(all="ignore"):
                o = sq.ref_smooth(c, dict(ins, **kw), rec=slice(b, b + 1))
            assert np.all(o["nrows"] == n) and np.all(o["info"][..., 2] == (n if stage == 1 else n - 1)), ("the reference stops there too", what)
            assert np.array_equal(got["nrows"][:, b], o["nrows"][:, 0]) and np.array_equal(got["info"][:, b, 2], o["info"][:, 0, 2]), what
            for k in sq.ROWS + ("tape", "xf", "pstd", "innov", "Ps0", "xT", "PT"):
                assert _nan_like(got[k][:, b], o[k][:, 0]), (k, what)
            assert np.array_equal(got["sinfo"][:, b, 0], o["sinfo"][:, 0, 0], equal_nan=True), what
            assert uc.err(got["sinfo"][:, b, 1], o["sinfo"][:, 0, 1]) < sq.TOL, what
            for k in sq.ROWS:
                assert np.isnan(got[k][:, b, n:]).all() and np.isfinite(got[k][:, b, :n]).all(), (k, what)
            if n:
                cut = sq.smooth(eng, ctx, c, ins, rows=slice(0, n), **{k: (v[:, :n] if k in ("U", "Y") else v) for k, v in kw.items()})
                for k in sq.ROWS:
                    assert np.array_equal(got[k][:, b, :n], cut[k][:, b]), (k, "the valid prefix", what)
                assert np.array_equal(got["Ps0"][:, b], cut["Ps0"][:, b]) and np.array_equal(got["sinfo"][:, b], cut["sinfo"][:, b]), what
            for other in range(B):
                if other != b:
                    sq.same(got, clean, SQ_TAPE, ("another problem, with a failure in", other, what), (slice(None), other), (slice(None), other))
            one = sq.smooth(eng, ctx, c, ins, **kw)
            sq.same(one, got, SQ_ALL, ("one chunk against two calls", what))
            sq.same(sq.smooth(eng, ctx, c, ins, tape_bytes=sc.smooth_quat_tape_bytes(c), **kw), one, SQ_ALL, ("chunks 4 + 4 + 1 against one chunk", what))


def test_smooth_quat_terminal_pair_and_a_short_prefix(eng, ctx):
    """a terminal pair (sweep_quat.terminal_pair, from the filter's own xT and PT where they are finite) in a call in which one problem
    was stopped at n = 7 by an infinite command: that problem is the call without a pair, bit for bit (the law ignores the pair when
    n < T); the problems with n = T move by more than 1e3 TOL.  The upper triangle of Ps_T is NaN.  With a pair and want = () every
    output is None."""
    c = _quat_corner(B=4, T=12, P=lambda v: v > 1, measured="std")
    ins = sq.quat_inputs(c)
    b, n = 2, 7
    U = ins["U"].copy()
    U[b, n - 1, 0] = np.inf
    f = sq.call(eng.ukf_filter_quat, ctx, c, ins, extra=dict(tape=True), U=U)
    want_n = np.full((c["P"], c["B"]), float(c["T"]))
    want_n[:, b] = n
    assert np.array_equal(f["nrows"], want_n), (f["nrows"], c)
    clean = sq.call(eng.ukf_filter_quat, ctx, c, ins)
    pair = sq.terminal_pair(c, dict(xT=np.where(np.isnan(f["xT"]), clean["xT"], f["xT"]), PT=np.where(np.isnan(f["PT"]), clean["PT"], f["PT"])))
    assert np.isnan(pair[1][..., 0, 1]).all() and np.isfinite(pair[0]).all() and pair[0].shape == (c["P"], c["B"], 13)
    without = eng.ukf_rts_quat(f["xf"], f["tape"], f["nrows"], ctx=ctx)
    with_pair = eng.ukf_rts_quat(f["xf"], f["tape"], f["nrows"], terminal=pair, ctx=ctx)
    sq.same(with_pair, without, sq.S_OUTS, ("a pair given to a short prefix", c), (slice(None), b), (slice(None), b))
    assert np.isfinite(with_pair["xs"][:, b, :n]).all() and np.isnan(with_pair["xs"][:, b, n:]).all(), c
    for other in range(c["B"]):
        if other != b:
            assert np.all(with_pair["sinfo"][:, other, 0] == -1) and np.isfinite(with_pair["Ps"][:, other]).all(), (other, c)
            for j in range(c["P"]):
                moved = uc.err(with_pair["xs"][j, other], without["xs"][j, other])
                assert moved > 1e3 * sq.TOL, ("the pair must move a complete problem", moved, j, other, c)
    optional = eng.ukf_rts_quat(f["xf"], f["tape"], f["nrows"], terminal=pair, want=(), ctx=ctx)      # a pair with every optional output NULL
    assert all(v is None for v in optional.values())
    sq.same(eng.ukf_rts_quat(f["xf"], f["tape"], f["nrows"], terminal=pair, want=("sinfo",), ctx=ctx), with_pair, ("sinfo",), ("sinfo alone", c))


def test_smooth_tape_buffer_shared_by_both_smoothers():
    """brov_ukf_smooth (records of 312 doubles) and brov_ukf_smooth_quat (313) use one tape buffer of the ctx.  They alternate on one
    ctx so that the buffer grows, shrinks below half and grows again across the two: large quat, small Euler, large Euler, small
    quat, large quat, with large B = 13, T = 12 and small B = 1, T = 1.  After the large Euler call a quaternion call in chunks of
    8 + 5 needs between half and all of the buffer the Euler call grew, so it runs on that buffer.  Every call gives the bits it gives
    on a fresh ctx."""
    from bluerov2_dynamics_amd import _lib, engine
    lq, sq_ = _quat_corner(B=13, T=12), _quat_corner(B=1, T=1)
    le, se_ = _smooth_corner(B=13, T=12), _smooth_corner(B=1, T=1)
    size = lambda c, rec, B: c["P"] * B * c["T"] * (rec + 8)       # tape and nrows of B recordings
    assert 2 * size(se_, sc.SMOOTH_RECORD, 1) + 512 < size(lq, sc.SMOOTH_QUAT_RECORD, 13), "small Euler: below half of large quat"
    assert 2 * size(sq_, sc.SMOOTH_QUAT_RECORD, 1) + 512 < size(le, sc.SMOOTH_RECORD, 13), "small quat: below half of large Euler"
    assert sc.smooth_quat_chunks(lq) == [8, 5] and 2 * size(lq, sc.SMOOTH_QUAT_RECORD, 8) > size(le, sc.SMOOTH_RECORD, 13) + 512 \
        and size(lq, sc.SMOOTH_QUAT_RECORD, 8) + 512 < size(le, sc.SMOOTH_RECORD, 13), "chunks of 8: kept on the Euler call's buffer"
    runs = {"lq": lambda k, **kw: sq.smooth(engine, k, lq, ins["lq"], **kw), "sq": lambda k, **kw: sq.smooth(engine, k, sq_, ins["sq"], **kw),
            "le": lambda k, **kw: ss.smooth(engine, k, le, ins["le"], **kw), "se": lambda k, **kw: ss.smooth(engine, k, se_, ins["se"], **kw)}
    ins = dict(lq=sq.quat_inputs(lq), sq=sq.quat_inputs(sq_), le=su.ukf_inputs(le), se=su.ukf_inputs(se_))
    keys = dict(lq=SQ_ALL, sq=SQ_ALL, le=SM_ALL, se=SM_ALL)
    fresh = {}
    for name in runs:
        one = _lib.Context(0)
        try:
            fresh[name] = runs[name](one)
        finally:
            one.close()
    kept = _lib.Context(0)
    try:
        for step, name in enumerate(("lq", "se", "le", "sq", "lq")):
            same = sq.same if name.endswith("q") else ss.same
            same(runs[name](kept), fresh[name], keys[name], ("call", step, name, "on one ctx"))
            if step == 2:
                sq.same(runs["lq"](kept, tape_bytes=sc.smooth_quat_tape_bytes(lq)), fresh["lq"], SQ_ALL, ("chunks 8 + 5 on the Euler call's buffer", lq))
    finally:
        kept.close()


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
