"""The case lists of tests/sweep_cases.py, without a GPU: (a) every value and corner pair of the five families' value sets occurs in
the hand-written corner list, by name, so that a list cannot shrink silently; (b) for every case the reference alone meets the
conditions of tests/sweep_run.py (float64 against long double below a tenth of the bound on the compared lanes, at most 2 % of the
lanes left out, never all), so that tests/test_family_sweeps_gpu.py can fail only because of a kernel; (c) the lists are a function
of the seed alone and their hashes are pinned.  The vehicles come from tests/fossen_vehicles.py, which needs the built library."""
import pytest

import sweep_cases as sc

SLICES = 4
PINNED = dict(rollout_pop="b4f7b2290e6ab13c", feedback="4c9883ac5a6cc7c3", mppi="74fd85dc3ab0bb0a", koopman_mppi="ba6fde35b7fbdb03", window_pop="eb2644555a733e52")


def _seen(family, key):
    cs = sc.corners(family)
    if family == "window_pop" and key == "nbags":
        return {len(c["lens"]) for c in cs}
    if family in ("mppi",) and key == "nparams":
        return {"1" if c["nparams"] == 1 and c["B"] > 1 else "B" if c["nparams"] == c["B"] and c["B"] > 1 else None for c in cs} - {None}
    return {c.get(key + "_as", c.get(key)) for c in cs}


# ------------------------------------------------------------------------------------------ (a) coverage
@pytest.mark.parametrize("family", sc.FAMILIES)
def test_every_value_is_in_the_corner_list(family):
    assert len(sc.corners(family)) == 12 and len(sc.cases(family)) == sc.N_CASES
    for key, values in sc.SETS[family].items():
        missing = set(values) - _seen(family, key)
        assert not missing, (family, key, "not in the corner list", missing)
    for c in sc.cases(family):
        for key, values in sc.SETS[family].items():
            if family == "window_pop" and key in ("nbags", "nwin"):      # a bag list: up to five bags of up to H + 65 rows each
                assert (len(c["lens"]) in sc.SETS[family]["nbags"] and c["nwin"] <= 5 * 65) if c["bags"] else c["nwin"] in sc.SETS[family]["nwin"], c
            elif not (family == "mppi" and key == "nparams"):
                assert c.get(key + "_as", c.get(key)) in values, (family, key, c)


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


# ------------------------------------------------------------------------------------------ (b) well-posedness
@pytest.mark.parametrize("part", range(SLICES))
@pytest.mark.parametrize("family", sc.FAMILIES)
def test_reference_alone_meets_the_conditions(family, part):
    import sweep_run as sr
    cases = sc.cases(family)[part::SLICES]
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


# ------------------------------------------------------------------------------------------ (c) byte stability
@pytest.mark.parametrize("family", sc.FAMILIES)
def test_lists_are_byte_stable(family):
    a, b = sc.cases(family), getattr(sc, family)(sc.SEED)
    assert sc.digest(a) == sc.digest(b) and a == b
    assert sc.digest(sc.cases(family, seed=sc.SEED + 1)) != sc.digest(a), "the seed must matter"
    assert sc.digest(a) == PINNED[family], (family, sc.digest(a))
