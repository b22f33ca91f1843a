"""The case lists of tests/sweep_cases.py, without a GPU: (a) every value and corner pair of the sixteen families' value sets occurs in
the hand-written corner list, by name, so that a list cannot shrink silently; (b) for every case the reference alone meets the
conditions of tests/sweep_run.py (float64 against long double below a tenth of the bound on the compared lanes, at most 2 % of the
lanes left out, never all), so that tests/test_family_sweeps_gpu.py can fail only because of a kernel; (c) the lists are a function
of the seed alone and their hashes are pinned.  The vehicles come from tests/fossen_vehicles.py, which needs the built library.
The EDMDc families' reference is oracle/edmdc_numpy.py restated with a dtype (tests/sweep_edmdc.py): (d) its float64 form is the
oracle's bit for bit.  The filter (ukf) and QP (lmpc) families take their references from tests/ukf_ref.py and
tests/koopman_lmpc_ref.py through tests/sweep_ukf_lmpc.py; with at most 27 lanes a case the 2 % cap means that no lane is left out.
The k-means families (colstats, kmeanspp, lloyd; tests/sweep_kmeans.py) have exact references: (e) preparing one asserts that NumPy's
own float64 statistics stay within a tenth of the bounds, that no round of the long-double k-means++ is undecided, and that no sample
of any iteration of the certified Lloyd reference is undecided -- here for every case below 2^18 rows and for two of the larger ones
(tests/test_family_sweeps_gpu.py prepares the others where it runs them).
The smoother family (smooth; tests/sweep_smooth.py) takes its reference from tests/ukf_smooth_ref.py with and without the case's
terminal pair: a lane needs the gaps of tests/ukf_smooth_cases.py and of the filter below a tenth of 1e-10, wrap margins above 1e-6,
forward and backward pivots above 1e-4 and every row and transition completed in both precisions; with at most 39 lanes a case the
2 % cap again means that no lane is left out, and (f) the reference's clamp of an edited nrows is the header's.
The quaternion families (ukf_quat, smooth_quat; tests/sweep_quat.py) take theirs from tests/ukf_quat_ref.py and
tests/ukf_quat_smooth_ref.py: a lane needs every gap below a tenth of 1e-10, |e_w| above 0.5 in every [-] taken, pivots above 1e-4 and
every row and transition completed in both precisions; again no lane is left out.  (g) Their corner lists tell the law from every
neighbour that the two references offer, by orders of magnitude more than the five pinned problems of tests/ukf_quat_cases.py do."""
import numpy as np
import pytest

import sweep_cases as sc

SLICES = 4
PINNED = dict(rollout_pop="b4f7b2290e6ab13c", feedback="4c9883ac5a6cc7c3", mppi="74fd85dc3ab0bb0a", koopman_mppi="ba6fde35b7fbdb03", window_pop="eb2644555a733e52",
              lift="62c586556d519270", gram="c447b4abb5b3d59e", pinv_apply="54c93dc0a5e3b343", multistep="552e6e4e744eb655", simulate="9f4f465e2cfbb921",
              ukf="53cf8c7f5c12aeab", lmpc="473db34e0cdb6f88", colstats="36c523c381e38c6e", kmeanspp="ee864b94e8c1c124", lloyd="fedd81db4999f98f", smooth="805feafecaca48a9",
              ukf_quat="b64cbbd87c7bbd2a", smooth_quat="fd328c6822245314")
CORNERS = dict(rollout_pop=12, feedback=12, mppi=12, koopman_mppi=12, window_pop=12, lift=12, gram=24, pinv_apply=14, multistep=14, simulate=12, ukf=17, lmpc=26,
               colstats=12, kmeanspp=14, lloyd=29, smooth=20, ukf_quat=16, smooth_quat=20)
LLOYD_LARGE_ON_CPU = 2                    # cases from 2^18 rows on whose reference is prepared here too: the first with bounds, the first without


def _value(c, key):
    """the value a case holds for a key of its family's value set"""
    if key == "nr":
        return (c["n"], c["r"])
    if key == "shape":
        return (c["n"], c["k"], c["r"])
    return c.get(key + "_as", c.get(key))


def _seen(family, key):
    cs = sc.corners(family)
    if family == "window_pop" and key == "nbags":
        return {len(c["lens"]) for c in cs}
    if family in ("mppi",) and key == "nparams":
        return {"1" if c["nparams"] == 1 and c["B"] > 1 else "B" if c["nparams"] == c["B"] and c["B"] > 1 else None for c in cs} - {None}
    return {_value(c, key) for c in cs}


# ------------------------------------------------------------------------------------------ (a) coverage
@pytest.mark.parametrize("family", sc.FAMILIES)
def test_every_value_is_in_the_corner_list(family):
    assert len(sc.corners(family)) == CORNERS[family] == sc.N_CORNERS[family], (family, len(sc.corners(family)))
    assert len(sc.cases(family)) == (32 if family in sc.EDMDC_FAMILIES + sc.FILTER_FAMILIES + sc.KMEANS_FAMILIES else sc.N_CASES) == sc.N_CASES_OF[family]
    for key, values in sc.SETS[family].items():
        missing = set(values) - _seen(family, key)
        assert not missing, (family, key, "not in the corner list", missing)
    for c in sc.cases(family):
        for key, values in sc.SETS[family].items():
            if family == "window_pop" and key in ("nbags", "nwin"):      # a bag list: up to five bags of up to H + 65 rows each
                assert (len(c["lens"]) in sc.SETS[family]["nbags"] and c["nwin"] <= 5 * 65) if c["bags"] else c["nwin"] in sc.SETS[family]["nwin"], c
            elif family == "lmpc" and key == "H":                      # a draw's H: anywhere in the last knot, up to the third epilogue trip
                assert (c["M"] - 1) * c["hold"] < c["H"] <= min(c["M"] * c["hold"], sc.LMPC_H_MAX), c
            elif family == "lloyd" and c["init"] == "allzero" and key in ("N", "k"):      # the integer-point set has its own size
                assert (c["N"], c["k"]) == sc.KM_ALLZERO, c
            elif not (family == "mppi" and key == "nparams"):
                assert _value(c, key) in values, (family, key, c)


def _has(family, **want):
    return any(all(c[k] == v for k, v in want.items()) for c in sc.corners(family))


def test_corner_pairs():
    assert _has("rollout_pop", B=64, P=5, per_candidate=True)
    assert _has("rollout_pop", B=65, stride_as="T+1")
    assert _has("rollout_pop", T=0, lag=True)
    assert _has("mppi", M=1, shift=True)
    assert _has("mppi", K=513, eps=False, B=3)
    assert _has("mppi", K=64, integ="euler") and _has("mppi", K=65, integ="euler")
    assert _has("mppi", nparams=1, B=3) and _has("mppi", lag_mode=1)
    for c in sc.cases("mppi"):
        assert c["M"] == (c["H"] + c["hold"] - 1) // c["hold"] and (c["rows"] == 1 or 0 <= c["row0"] <= c["rows"] - 1 - c["H"]), c
    assert {c["row0"] for c in sc.cases("mppi") if c["rows_as"] == "H+4"} >= {0, 1, 2, 3}, "ref_row0 over its whole legal range"
    for r, edge in ((6, (36, 42, 78, 84)), (8, (8, 40, 72, 80))):        # both sides of M r = 39 / 40 and 79 / 80, for both r
        for mr_ in edge:
            assert _has("koopman_mppi", r=r, Mr=mr_), (r, mr_)
    for c in sc.cases("koopman_mppi"):
        assert c["M"] == (c["H"] + c["hold"] - 1) // c["hold"] and c["M"] * c["r"] == c["Mr"], c
    assert any(c["H"] % c["hold"] for c in sc.corners("koopman_mppi")) and any(c["hold"] >= c["H"] for c in sc.corners("koopman_mppi"))
    assert _has("feedback", hold_as="T+1", ref="set") and _has("feedback", T=0) and _has("feedback", T=130)
    w = sc.corners("window_pop")
    assert any(c["bags"] and 0 in c["lens"] for c in w) and any(c["bags"] and c["H"] in c["lens"] for c in w), "bags without a window"
    assert any(c["bags"] and c["lens"][0] == c["H"] + 64 and c["nwin"] > 64 for c in w), "a join at a chunk edge"
    assert any(c["bags"] for c in w) and any(not c["bags"] for c in w)


def test_filter_and_qp_corner_pairs():
    """the edges the ukf and lmpc corner lists must contain, by name"""
    u = sc.corners("ukf")
    inst = {(0, "euler", 0, True), (0, "euler", 0, False), (0, "rk4", 0, True), (0, "rk4", 0, False), (0, "rk4", 1, True), (0, "rk4", 1, False),
            (1, "euler", 0, False), (1, "rk4", 0, False)}
    assert {sc.ukf_instance(c) for c in u} == inst, "the eight instantiations of ukf_filter_kernel"
    for i in inst:                                                   # every instantiation with a full and with a ragged last block
        assert any(sc.ukf_instance(c) == i and c["B"] % 4 == 0 for c in u) and any(sc.ukf_instance(c) == i and c["B"] % 4 for c in u), i
    for model in (0, 1):
        assert _has("ukf", model=model, measured="none") and _has("ukf", model=model, measured="all", r_inf=0, T=12), model
    assert _has("ukf", P=3, nrec=3) and _has("ukf", B=9) and _has("ukf", B=1, T=12) and _has("ukf", wrap=True, T=12)
    assert all(c["P"] * c["B"] * c["T"] <= sc.UKF_ROWS and c["nrec"] in (1, c["P"]) for c in sc.cases("ukf"))
    assert all(not c["lag"] and c["lag_mode"] == 0 for c in sc.cases("ukf") if c["model"] == 1)
    q = sc.corners("lmpc")
    rows = {sc.lmpc_rows(c) for c in q}
    assert rows == {(1, True), (2, True), (2, False), (3, False), (4, False), (5, False)}, "every rows-per-lane count with both W sources where both exist"
    for c in sc.cases("lmpc"):
        assert c["M"] * c["r"] == c["Nv"] <= 312 and c["M"] == (c["H"] + c["hold"] - 1) // c["hold"] and 1 <= c["H"] <= sc.LMPC_H_MAX, c
        assert (c["special"] == "warm") == (c["tol"] > 0) and (c["special"] != "quat_flip" or c["n"] == 13) and (c["special"] != "angle_wrap" or c["n"] == 12), c
    assert {c["H"] + 1 for c in q} >= {64, 65, 66, 128, 129, 130}, "both sides of the epilogue's second and third trip"
    assert any(c["H"] + 1 > 64 and c["Nv"] > 128 and c["H"] % c["hold"] for c in q), "a second trip with a short last knot at three rows per lane"
    for nq in (3, 4, 5):
        assert any(sc.lmpc_rows(c)[0] == nq and c["H"] + 1 > 64 for c in q), nq
        assert any(sc.lmpc_rows(c)[0] == nq and c["shift"] and c["iters"] == 40 for c in q), ("the shift", nq)
        assert any(sc.lmpc_rows(c)[0] == nq and c["Nv"] % 8 for c in q), ("the scalar tail of the blocked loop", nq)
    assert any(sc.lmpc_rows(c) == (2, False) and c["Nv"] % 8 for c in q), "the scalar tail with W from global memory at two rows per lane"
    assert {c["hold"] * c["r"] for c in q} >= {60, 64, 66, 72}, "hold r on both sides of 64"
    assert {sc.lmpc_rows(c) for c in q if c["special"] == "warm"} == {(2, False), (3, False), (5, False)}
    assert any(c["hold"] > c["H"] for c in q) and any(c["M"] == 1 and c["shift"] for c in q)


def test_smoother_corner_pairs():
    """the edges the smooth corner list must contain, by name"""
    s = sc.corners("smooth")
    inst = {(0, "euler", 0, True), (0, "euler", 0, False), (0, "rk4", 0, True), (0, "rk4", 0, False), (0, "rk4", 1, True), (0, "rk4", 1, False),
            (1, "euler", 0, False), (1, "rk4", 0, False)}
    assert {sc.ukf_instance(c) for c in s} == inst, "the eight tape instantiations of ukf_filter_kernel"
    for i in inst:                                                   # every instantiation with a full and with a ragged last block
        assert any(sc.ukf_instance(c) == i and c["B"] % 4 == 0 for c in s) and any(sc.ukf_instance(c) == i and c["B"] % 4 for c in s), i
    for T in (1, 2, 3):
        assert _has("smooth", T=T, terminal=True) and _has("smooth", T=T, terminal=False), T
    assert any(c["P"] == 3 and c["nrec"] == 3 and len(sc.smooth_chunks(c)) > 1 for c in s), "a noise record per candidate at P = 3, chunked"
    chunks = [(c["B"], c["chunk"], sc.smooth_chunks(c)) for c in s]
    assert (9, 4, [4, 4, 1]) in chunks and (13, 8, [8, 5]) in chunks and (13, 4, [4, 4, 4, 1]) in chunks, chunks
    assert any(c["chunk"] == 5 and c["B"] >= 8 and sc.smooth_chunks(c)[0] == 4 for c in s), "room for 5 recordings is rounded down to 4"
    assert any(c["P"] == 3 and c["nrec"] == 3 and c["B"] == 9 and sc.smooth_chunks(c) == [4, 4, 1] and c["measured"] == "std" and not c["terminal"]
               for c in s), "the corner of test_smooth_chunking_with_failures"
    for model in (0, 1):
        assert _has("smooth", model=model, measured="none") and _has("smooth", model=model, measured="all"), model
        assert any(c["model"] == model and c["B"] == 8 and c["T"] == 12 and not c["lag"] for c in s), ("two full blocks of 12 rows", model)
    assert _has("smooth", q_zero=True) and _has("smooth", r_inf=0) and _has("smooth", r_inf=3) and _has("smooth", wrap=True, T=12, terminal=True)
    assert _has("smooth", B=1) and _has("smooth", B=4, T=12) and any(c["lag"] and c["T"] == 12 and c["P"] > 1 for c in s)
    assert {c["want_as"] for c in s} == set(sc.SMOOTH_WANT) and all(c["want"] == list(sc.SMOOTH_WANT[c["want_as"]]) for c in sc.cases("smooth"))
    allc = sc.cases("smooth")
    assert all(c["P"] * c["B"] * c["T"] <= sc.UKF_ROWS and c["nrec"] in (1, c["P"]) and sum(sc.smooth_chunks(c)) == c["B"] for c in allc)
    assert all(not c["lag"] and c["lag_mode"] == 0 for c in allc if c["model"] == 1)
    assert all(sc.smooth_tape_bytes(c) >= c["P"] * 4 * c["T"] * sc.SMOOTH_RECORD for c in allc), "never below the one block the host demands"
    assert 3 * sum(c["T"] >= 2 for c in allc) >= 2 * len(allc), "at least two thirds of the cases have a transition"


def _quat_has(family, **want):
    """a corner of the family holds `want` (a callable value is a predicate on the field)"""
    return any(all(v(c[k]) if callable(v) else c[k] == v for k, v in want.items()) for c in sc.corners(family))


def test_quaternion_corner_pairs():
    """the edges the ukf_quat and smooth_quat corner lists must contain, by name"""
    chunked = lambda c: len(sc.smooth_quat_chunks(c)) > 1
    for fam in ("ukf_quat", "smooth_quat"):
        for integ in ("euler", "rk4"):
            assert _quat_has(fam, integ=integ, B=4) and _quat_has(fam, integ=integ, B=5) and _quat_has(fam, integ=integ, P=3, nrec=3), (fam, integ)
            for att in sc.SETS[fam]["attitude"]:
                assert _quat_has(fam, integ=integ, attitude=att), (fam, integ, att)
        assert _quat_has(fam, measured="all", T=12) and _quat_has(fam, measured="none", T=1) and _quat_has(fam, measured="none", T=12), fam
        assert _quat_has(fam, measured="all", r_inf=3) and _quat_has(fam, measured="all", r_inf=0), fam
        assert _quat_has(fam, attitude="sphere", spread="wide") and _quat_has(fam, attitude="inverted", spread="wide"), fam
        assert _quat_has(fam, B=13, T=12) and _quat_has(fam, B=1, T=1), fam
        assert all(c["P"] * c["B"] * c["T"] <= sc.UKF_ROWS and c["nrec"] in (1, c["P"]) for c in sc.cases(fam)), fam
    s = sc.corners("smooth_quat")
    for integ in ("euler", "rk4"):
        assert any(c["integ"] == integ and chunked(c) for c in s), (integ, "a chunked call")
        assert any(c["integ"] == integ and c["nrec"] == c["P"] > 1 and c["T"] == 12 and c["B"] >= 8 for c in s), (integ, "the corner of the repeat test")
    for T in (1, 2, 3):
        assert _quat_has("smooth_quat", T=T, terminal=True) and _quat_has("smooth_quat", T=T, terminal=False), T
    sets = [sc.smooth_quat_chunks(c) for c in s]
    for want in ([4, 4, 1], [4, 1], [8, 5], [4, 4]):
        assert want in sets, (want, sets)
    assert any(c["chunk"] == 1.5 and c["B"] > 4 and sc.smooth_quat_chunks(c)[0] == 4 for c in s), "1.5 blocks are rounded down to one"
    assert any(c["P"] == 3 and c["nrec"] == 3 and chunked(c) for c in s), "a noise record per candidate at P = 3, chunked"
    assert any(c["P"] == 3 and c["nrec"] == 3 and c["B"] == 9 and sc.smooth_quat_chunks(c) == [4, 4, 1] and c["measured"] == "std" and not c["terminal"]
               for c in s), "the corner of test_smooth_quat_chunking_with_failures"
    for want in sc.SMOOTH_WANT:
        if want != "all":
            assert any(c["want_as"] == want and chunked(c) for c in s) and any(c["want_as"] == want and not chunked(c) for c in s), want
    for att in ("sphere", "level"):
        assert any(c["attitude"] == att and c["T"] == 12 and c["P"] > 1 and c["measured"] == "std" for c in s), (att, "the corner of the split test")
    assert any(c["B"] == 4 and c["T"] == 12 and c["P"] > 1 and c["measured"] == "std" for c in s), "the corner of the short-prefix test"
    allc = sc.cases("smooth_quat")
    assert all(sum(sc.smooth_quat_chunks(c)) == c["B"] and c["want"] == list(sc.SMOOTH_WANT[c["want_as"]]) for c in allc)
    assert all(sc.smooth_quat_tape_bytes(c) >= c["P"] * 4 * c["T"] * sc.SMOOTH_QUAT_RECORD for c in allc), "never below the one block the host demands"
    assert 3 * sum(c["T"] >= 2 for c in allc) >= 2 * len(allc), "at least two thirds of the cases have a transition"


# (variant) -> (family, index in the corner list, the output that must tell it from the law)
QUAT_NEIGHBOURS = dict(plus_left=("ukf_quat", 2, "xf"), minus_left=("ukf_quat", 2, "xf"), no_d=("ukf_quat", 2, "xf"), no_mean=("ukf_quat", 2, "xf"),
                       no_wc0=("ukf_quat", 2, "PT"))
QUAT_SMOOTH_NEIGHBOURS = dict(minus_left=("smooth_quat", 16, "xs"), dx_linear=("smooth_quat", 16, "xs"), plus_left=("smooth_quat", 16, "xs"),
                              C_T=("smooth_quat", 16, "xs"), no_Pp=("smooth_quat", 16, "Ps"), dx_from_xf=("smooth_quat", 16, "xs"))


def test_quaternion_corners_tell_the_law_from_its_neighbours():
    """(g) every variant of ukf_quat_ref.VARIANTS on ukf_quat corner 2 (Euler, P = 3, inverted, wide, every entry measured) and every variant
    of ukf_quat_smooth_ref.VARIANTS on smooth_quat corner 16 (Euler, P = 2, B = 5, sphere, wide, a terminal pair) lies more than 1e3 TOL
    from the law in the named output; printed next to the figure of the pinned problem q_rk4"""
    import sweep_quat as sq
    import ukf_quat_cases as qc
    import ukf_quat_ref as uq
    import ukf_quat_smooth_ref as qs
    assert set(QUAT_NEIGHBOURS) == set(uq.VARIANTS) and set(QUAT_SMOOTH_NEIGHBOURS) == set(qs.VARIANTS)
    c = sc.corners("ukf_quat")[2]
    assert (c["attitude"], c["spread"], c["measured"]) == ("inverted", "wide", "all")
    ins = sq.quat_inputs(c)
    law = sq.ref_filter(c, ins)
    for v, (_, _, key) in QUAT_NEIGHBOURS.items():
        with np.errstate(all="ignore"):
            g = sq.filter_gaps(sq.ref_filter(c, ins, variant=v), law)[key]
        pinned = qc.gaps(qc.reference("q_rk4", variant=v), qc.reference("q_rk4"))[key]
        print(f"filter {v}: {key} apart by {g:.1e} on ukf_quat corner 2, by {pinned:.1e} on the pinned q_rk4")
        assert g > 1e3 * sq.TOL, (v, key, g)
        if v in ("plus_left", "minus_left"):
            assert g > 50 * pinned, (v, "a wide inverted start must separate the side of the product far better than the pinned cases", g, pinned)
    c = sc.corners("smooth_quat")[16]
    assert (c["attitude"], c["spread"], c["terminal"]) == ("sphere", "wide", True)
    ins = sq.quat_inputs(c)
    plain = sq.ref_smooth(c, ins)
    term = sq.terminal_pair(c, plain)
    law = sq.with_terminal(plain, term, np.float64)
    for v, (_, _, key) in QUAT_SMOOTH_NEIGHBOURS.items():
        with np.errstate(all="ignore"):
            g = qs.gaps(sq.with_terminal(plain, term, np.float64, v), law)[key]      # the forward pass is the law under every variant
        pinned = qs.gaps(qs.reference("q_rk4", variant=v), qs.reference("q_rk4"))[key]
        print(f"smoother {v}: {key} apart by {g:.1e} on smooth_quat corner 16, by {pinned:.1e} on the pinned q_rk4")
        assert g > 1e3 * sq.TOL, (v, key, g)


def test_reference_clamps_an_edited_nrows_as_the_header_says():
    """(f) include/brov2.h: n = nrows clamped to 0 .. T, the fraction dropped, NaN as 0 -- and every n the filter itself writes as before"""
    import sweep_smooth as ss
    import ukf_smooth_ref as usr
    c = [c for c in sc.corners("smooth") if c["B"] == 1 and c["T"] == 12][0]
    o = ss.ref_smooth(c, ss.su.ukf_inputs(c), cand=slice(0, 1))
    xf, tape = o["xf"][0, 0], o["tape"][0, 0]
    rows = lambda n: int(np.isfinite(usr.rts_one(xf, tape, n, np.float64)["xs"][:, 0]).sum())
    for n, want in ((np.nan, 0), (-np.inf, 0), (-1, 0), (0, 0), (0.5, 0), (1, 1), (6.7, 6), (12, 12), (17, 12), (np.inf, 12), (np.float64(7.0), 7),
                    (np.longdouble(5), 5)):
        assert rows(n) == want, (n, rows(n), want)
    r = usr.rts_one(xf, tape, 0.5, np.float64)
    assert np.isnan(r["sinfo"]).all() and np.isnan(r["Ps0"]).all()
    r = usr.rts_one(xf, tape, 1, np.float64)
    assert np.array_equal(r["sinfo"], [-1.0, np.inf]) and np.array_equal(r["xs"][0], xf[0])
    for k in ("xs", "Ps", "sinfo"):
        assert np.array_equal(usr.rts_one(xf, tape, np.inf, np.float64)[k], o[k][0, 0]) and np.array_equal(usr.rts_one(xf, tape, 6.7, np.float64)[k],
                                                                                                             usr.rts_one(xf, tape, 6, np.float64)[k], equal_nan=True), k


def _chunk_edges(c):
    """(bag ends on a chunk's last row, one row before it, one row after it, chunks that hold no pair) of a list-form case"""
    ch, lens = sc.chunk_rows(c["chunk"], c["lens"]), c["lens"]
    ends = sc.bag_ends(lens)
    starts = np.concatenate([[0], np.cumsum(lens)])[:-1]
    pair = np.zeros(sum(lens), dtype=bool)                  # rows that start a pair
    for a, m in zip(starts, lens):
        pair[a:a + max(m - 1, 0)] = True
    nchunks = -(-max(sum(lens) - 1, 0) // ch)
    empty = sum(1 for i in range(nchunks) if not pair[i * ch:(i + 1) * ch].any())
    at = lambda off: any(e > ch and (e + off) % ch == 0 for e in ends) or any(e + off == ch for e in ends)
    return at(0), at(1), at(-1), empty


def test_edmdc_corner_pairs():
    """the edges the EDMDc corner lists must contain, by name"""
    # lift: every instantiation, both block edges, the far corner
    assert _has("lift", N=65, k=257, n=13) and _has("lift", N=64, k=256, n=12) and _has("lift", N=130, k=513, n=16) and _has("lift", n=5)
    far = [c for c in sc.corners("lift") if c["scale"] == 12.0 and c["gamma"] == 3.0 and c["n"] == 12]
    assert far, "rows far from every centre"
    import sweep_edmdc as se
    ref = se.prepare_lift(far[0])
    assert ref["far"].all() and np.all(ref["o"][:, 12:] == 0.0) and float(ref["ol"][:, 12:].max()) < 1e-300, "the float64 reference is exactly 0"
    assert float(np.log(ref["ol"][:, 12:].max())) < -1000, "exponents far beyond float64's underflow: the clamped ldexp of exp_fast"
    # gram: the three forms, G^T G alone on both layouts, both strides, both xplus, r = 0 and 1, tile counts, bags, chunk edges
    g = sc.corners("gram")
    assert _has("gram", form="host") and _has("gram", form="ragged_dev", gty=False) and _has("gram", form="uniform_dev", gty=False)
    assert any(c["form"] == "uniform_dev" and c["split"] and c["xpad"] == 0 and c["upad"] == 0 for c in g), "strides L + 1 / L, two halves"
    assert any(c["form"] == "uniform_dev" and c["split"] and c["xpad"] > 0 and c["upad"] > 0 for c in g), "larger strides, two halves"
    assert any(c["form"] == "ragged_dev" and c["split"] for c in g)
    assert {(c["n"], c["r"]): c["xplus"] for c in g} == {(12, 8): 1, (13, 8): 0, (12, 10): 0, (13, 6): 1, (9, 4): 0, (5, 2): 1, (12, 0): 0, (12, 1): 0}
    assert {c["nt"] for c in g} >= {2, 3, 4, 5, 6, 7, 8, 9, 11, 18, 34, 35}, sorted({c["nt"] for c in g})
    assert {c["nt"] for c in g if not c["gty"]} >= {4, 9, 34} and {c["xplus"] for c in g if not c["gty"]} == {0, 1}
    lists = [c for c in g if c["form"] != "uniform_dev"]
    for m in (0, 1, 2, 3):
        assert any(c["lens"][0] == m for c in lists) and any(c["lens"][-1] == m for c in lists) and any(m in c["lens"][1:-1] for c in lists), ("bag of rows", m)
    for chunk in (64, 100, 257):
        edges = [_chunk_edges(c) for c in lists if c["chunk"] == chunk]
        assert any(e[0] for e in edges) and any(e[1] for e in edges) and any(e[2] for e in edges), ("bag ends on / before / after a chunk's last row", chunk)
    assert any(_chunk_edges(c)[3] for c in lists if c["chunk"] == 64), "a chunk that holds no pair"
    assert {c["pairs"] for c in g if c["k"] <= 17} >= {1, 2, 3}, "fewer pairs than K-slabs"
    assert any(c["short_u"] and c["form"] == "host" for c in g) and any(c["short_u"] and c["form"] == "ragged_dev" for c in g)
    assert any(c["chunk"] == 0 for c in g)
    hard = [c for c in lists if c["chunk"] == 64 and (0 in c["lens"] or 1 in c["lens"])]
    assert any(any(e % 64 in (0, 1, 63) for e in sc.bag_ends(c["lens"])) for c in hard), "bags of 0 or 1 rows next to a chunk edge"
    # pinv_apply: the forms, the 192-row unit, every chunk size
    a = sc.corners("pinv_apply")
    assert {c["form"] for c in a} == {"host", "ragged_dev", "uniform_dev"} and {c["chunk"] for c in a} == {64, 192, 257}
    assert {m for c in a for m in c["lens"]} >= {2, 3, 192, 193, 257}
    assert {c["nt"] % 6 for c in a} == {0, 1, 2, 3, 4, 5}, "every nt mod 6 of the W-rows plan"
    assert any(c["form"] == "uniform_dev" and c["xpad"] and c["upad"] for c in a) and any(c["form"] == "uniform_dev" and not c["xpad"] and not c["upad"] for c in a)
    # multistep: window blocks, the two-stream edge, K-step parities, d around 48 and 96, r = 0, H >= N
    m = sc.corners("multistep")
    assert any(c["nw"] == 1920 and c["H"] > 1 for c in m) and any(c["nw"] == 1921 and c["H"] > 1 for c in m) and any(c["nw"] == 2176 and c["H"] > 1 for c in m)
    two = [c for c in m if c["nw"] >= 1921 and c["H"] > 1]
    assert {c["ksteps"] % 2 for c in two} == {0, 1} and {c["H"] % 2 for c in two} == {0, 1} and any(c["ksteps"] == 1 for c in two)
    assert all(c["d"] <= 20 for c in m if c["nw"] >= 1920), "a small d for the long lists"
    for fam in ("multistep", "simulate"):
        cs = sc.corners(fam)
        assert {c["ksteps"] for c in cs} >= {1, 2} and any(c["ksteps"] % 2 and c["ksteps"] > 2 for c in cs) and any(c["ksteps"] % 2 == 0 and c["ksteps"] > 2 for c in cs), fam
        assert {c["d"] for c in cs} >= {47, 48, 49, 95, 97} and any(c["r"] == 0 for c in cs), fam
        assert all(c["ksteps"] == (c["n"] + c["k"] + c["r"] + 3) // 4 and c["d"] == c["n"] + c["k"] for c in sc.cases(fam)), fam
    assert _has("multistep", n=1, k=1, r=1, ksteps=1) and any(c["nw"] == 0 and c["H"] >= c["N"] for c in m)
    assert any(c["r"] == 0 and c["H"] == 0 for c in m) or (any(c["H"] == 0 for c in m) and any(c["r"] == 0 for c in m))
    assert any(c["short_u"] for c in m) and any(not c["short_u"] for c in m)
    s = sc.corners("simulate")
    assert any(c["r"] == 0 and c["nb"] > 256 for c in s) and any(c["r"] > 0 and c["nb"] > 256 and c["T"] == 50 for c in s) and _has("simulate", T=0)


def test_kmeans_corner_pairs():
    """the edges the colstats, kmeanspp and lloyd corner lists must contain, by name"""
    cs = sc.corners("colstats")
    assert sum(c["N"] > sc.CS_SATURATED for c in cs) >= 1 and _has("colstats", N=256) and _has("colstats", N=257) and _has("colstats", N=1, n=1)
    assert {c["null"] for c in cs} == {"none", "mean", "var"} and _has("colstats", form="dev_stride", n=12), "x_stride 13"
    for form in ("block_odd", "block_even"):
        assert any(c["form"] == form and c["n"] % 2 == 0 for c in cs) and any(c["form"] == form and c["n"] % 2 for c in cs), form
    assert any(c["const_col"] and c["offset"] for c in cs) and any(c["offset"] and c["scale"] == 1e-4 for c in cs) and _has("colstats", scale=1e4)
    pp = sc.corners("kmeanspp")
    assert _has("kmeanspp", N=60, k=60) and _has("kmeanspp", N=1, k=1) and any(c["N"] > 60000 and c["k"] > sc.PP_SCREEN_FROM for c in pp)
    assert {c["N"] - sc.PP_CHUNK for c in pp} >= {-1, 0, 1} and {c["N"] - 2 * sc.PP_CHUNK for c in pp} >= {-1, 0, 1} and {c["N"] - sc.PP_ROW for c in pp} >= {-1, 0, 1}
    assert {c["k"] for c in pp} >= {sc.PP_SCREEN_FROM, sc.PP_SCREEN_FROM + 1} and {c["trials"] for c in pp} >= {1, sc.PP_LMAX}
    assert any(c["trials_as"] == "sk" and c["trials"] == 8 for c in pp), "k = 512: eight trials"
    assert any(not c["mean"] for c in pp) and any(not c["ind"] for c in pp) and {c["first_as"] for c in pp} == {"0", "N-1"}
    assert all(c["trials"] == sc.pp_trials(c) and 1 <= c["k"] <= c["N"] and 0 <= c["first"] < c["N"] and (c["mean"] or not c["offset"])
               and (c["k"] - 1) * c["trials"] * c["N"] * c["n"] <= sc.PP_WORK for c in sc.cases("kmeanspp"))
    ll = sc.corners("lloyd")
    large = [c for c in ll if c["N"] >= sc.KM_SORTED_FROM and c["k"] >= 64]
    assert len(large) >= 8 and all(c["rate1"] and "resort" in c["expect"] for c in large) and all(not c["expect"] and not c["rate1"] for c in ll if c not in large)
    paths = {(c["n"], sc.lloyd_paths(c)[2:]) for c in large}      # (n, (packed-fp32 kernel, screening, bounds))
    assert paths >= {(12, (False, True, True)), (13, (False, True, True)), (5, (False, False, False)), (13, (True, False, False))}, paths
    assert any(c["k"] == 600 and sc.lloyd_paths(c)[2] for c in large) and any(c["k"] == 513 and sc.lloyd_paths(c)[2] for c in large)
    assert all(("list" in c["expect"]) == sc.lloyd_paths(c)[4] for c in sc.cases("lloyd"))
    assert {c["scale"] for c in large if "list" in c["expect"]} >= {1e-13, 1e13}, "M^2 outside 1e-24 .. 1e24 in the screened loop"
    assert {c["N"] for c in large} >= {1 << 18, (1 << 18) + 1, (1 << 18) + 2049} and _has("lloyd", N=(1 << 18) - 1)
    assert {c["stop"] for c in ll} == {"max_iter", "strict", "shift"} and _has("lloyd", stop="strict", order="blobs")
    assert {c["init"] for c in ll} == {"rows", "dup", "far2", "far3", "allzero"}
    assert _has("lloyd", k=63) and _has("lloyd", k=64) and _has("lloyd", k=65) and _has("lloyd", k=512) and _has("lloyd", k=513)
    assert any(c["n"] == 15 and c["k"] * 16 * 8 == sc.KM_LDS_BYTES for c in ll), "the LDS limit met from below at n = 15"
    assert any(c["k"] == c["N"] > 1 and c["offset"] for c in ll) and _has("lloyd", N=65, k=63, n=1, offset=True), "an inertia of 0, and one tiny against sum |x|^2"
    assert sc.corners("colstats") == sc.cases("colstats")[:len(sc.corners("colstats"))], "a reseeded corner is the same case in both lists"
    assert _has("lloyd", form="dev_stride", n=12) and any(c["form"] == "block_even" and c["n"] % 2 == 0 for c in ll) and any(c["form"] == "block_odd" for c in ll)
    assert any(c["const_col"] for c in ll) and any(c["offset"] for c in ll)
    for c in sc.cases("lloyd"):
        assert 1 <= c["k"] <= c["N"] and c["k"] * (c["n"] + 1) * 8 <= sc.KM_LDS_BYTES and c["n"] <= 15, c
    import sweep_kmeans as sk
    from oracle import kmeans_numpy as kn
    wide = [c for c in ll if c["N"] == 1 << 20][0]                   # a member sum beyond 2^64: the high word of kmeans.hip: km_to_double
    ref = sk.prepare_lloyd(wide)
    Xc = ref["X"] - ref["mean"]
    tot = kn._int_sums(np.rint(Xc * kn.fix_scales(np.abs(Xc).max(axis=0))[0]).astype(np.int64), ref["labels"], wide["k"])
    assert max(abs(v) for row in tot for v in row) > 1 << 64, wide
    for f in sc.KMEANS_FAMILIES:                                     # the slices share the expensive cases evenly
        for part in range(SLICES):
            heavy = [c for c in sc.cases(f)[part::SLICES] if c["N"] >= sc.KM_SORTED_FROM]
            assert len(heavy) <= 3, (f, part, len(heavy))


# ------------------------------------------------------------------------------------------ (b) well-posedness
@pytest.mark.parametrize("part", range(SLICES))
@pytest.mark.parametrize("family", sc.FAMILIES)
def test_reference_alone_meets_the_conditions(family, part):
    import sweep_run as sr
    cases = sc.cases(family)[part::SLICES]
    if family == "lloyd":                                            # (e): the large references belong to the GPU test, but for two of them
        large = [c for c in sc.cases(family) if c["rate1"]]
        here = [[c for c in large if ("list" in c["expect"]) == want][0] for want in (True, False)]
        assert len(here) == LLOYD_LARGE_ON_CPU
        cases = [c for c in cases if not c["rate1"] or c in here]
    lanes = left = 0
    gap = 0.0
    for c in cases:
        ref = sr.PREPARE[family](c)
        left += sr.well_posed(c, ref)
        lanes += ref["keep"].size
        gap = max(gap, ref["gap"])
        if ref["keep"].size == 1:
            assert ref["keep"].all(), ("a case with one lane must keep it", c)
    print(f"{family} slice {part}: {len(cases)} cases, {lanes} lanes, {left} left out, worst reference gap on the compared lanes {gap:.2e}")


# ------------------------------------------------------------------------------------------ (d) the restated reference
def test_restated_reference_is_the_oracle_in_float64():
    import sweep_edmdc as se
    from oracle import edmdc_numpy as ek
    rng = np.random.default_rng(7)
    X, C = rng.uniform(-0.5, 0.5, (70, 13)), rng.uniform(-0.5, 0.5, (33, 13))
    assert np.array_equal(se.lift(X, C, 3.0), ek.lift(X, C, 3.0)) and se.lift(X, C, 3.0, np.longdouble).dtype == np.longdouble
    c = sc.corners("gram")[0]
    ref = se.prepare_gram(c)
    GtG, GtY, npairs = ek.gram(ref["Xs"], ref["Us"], ref["C"], c["gamma"])
    assert npairs == ref["pairs"] and np.allclose(GtG, ref["o"][0], rtol=0, atol=1e-13) and np.allclose(GtY, ref["o"][1], rtol=0, atol=1e-13)
    c = sc.corners("multistep")[2]
    ref = se.prepare_multistep(c)
    rmse = ek.multistep_rmse(ref["X"], ref["U"], ref["C"], ref["gamma"], ref["A"], ref["B"], c["H"])
    assert rmse == float(np.sqrt(np.mean((ref["X"][c["H"]:] - ref["o"]) ** 2)))
    c = sc.corners("simulate")[3]
    ref = se.prepare_simulate(c)
    one = ek.simulate(ref["x0"][5], ref["U"][5], ref["C"], ref["gamma"], ref["A"], ref["B"])
    assert np.allclose(one, ref["o"][5], rtol=0, atol=1e-14)       # A @ z per trajectory there, Z @ A^T batched here


# ------------------------------------------------------------------------------------------ (c) byte stability
@pytest.mark.parametrize("family", sc.FAMILIES)
def test_lists_are_byte_stable(family):
    a, b = sc.cases(family), getattr(sc, family)(sc.SEED)
    assert sc.digest(a) == sc.digest(b) and a == b
    assert sc.digest(sc.cases(family, seed=sc.SEED + 1)) != sc.digest(a), "the seed must matter"
    assert sc.digest(a) == PINNED[family], (family, sc.digest(a))
