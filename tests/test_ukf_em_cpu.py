"""The EM fit of the filter's q and r without a GPU: the identity that makes the lag-one covariance unnecessary, the M-step of
fossen/estimate.py (em_update), and the well-posedness of what tests/test_ukf_em_gpu.py compares the kernel against
(tests/ukf_em_ref.py on the cases of tests/ukf_em_cases.py)."""
import numpy as np
import pytest

import fossen_vehicles as fv
import ukf_cases as uc
import ukf_em_cases as ue
import ukf_em_ref as uer
import ukf_ref as ur


def test_local_term_equals_the_lag_one_form():
    """on a seeded linear-Gaussian model (n = 5, T = 30, dropped measurements, one q_i = 0) the diagonal of
    Q + Q Pp^-1 (Ps_{t+1} - Pp + d d^T) Pp^-1 Q equals that of the Shumway-Stoffer expression with the lag-one covariance"""
    lag, loc = uer.linear_identity()
    rel = np.max(np.abs(lag - loc)) / np.max(np.abs(lag))
    print("largest difference, relative to the largest term:", rel)
    assert lag.shape == (29, 5) and np.all(loc[:, 2] == 0.0)
    assert rel <= 1e-12


def _em(P=2, B=3):
    rng = np.random.default_rng(5)
    em = rng.uniform(0.5, 2.0, (P, B, 37))
    em[..., 24:36] = rng.integers(1, 9, (P, B, 12))
    em[..., 36] = 11.0
    info = np.zeros((P, B, 4))
    info[..., 2] = -1
    sinfo = np.zeros((P, B, 2))
    sinfo[..., 0] = -1
    return em, info, sinfo


def test_em_update():
    from bluerov2_dynamics_amd.fossen import estimate
    em, info, sinfo = _em()
    r0 = np.full(12, 0.25)
    r0[7] = np.inf
    em[..., 12 + 7] = 0.0
    em[..., 24 + 7] = 0.0                      # never measured: no terms
    em[..., 24 + 3] = 0.0                      # measured in principle, but no row carried it
    em[..., 12 + 3] = 0.0
    cfg = estimate.ukf(q=0.5, r=r0, alpha=0.5)
    new, left = estimate.em_update(em, info, sinfo, cfg)
    assert left == 0 and len(new) == 2
    for j in range(2):
        q, r = np.array(list(new[j].q)), np.array(list(new[j].r))
        assert np.allclose(q, em[j, :, :12].sum(axis=0) / 33.0, rtol=1e-15)                      # pooled over the recordings
        ok = np.ones(12, bool)
        ok[[3, 7]] = False
        assert np.allclose(r[ok], em[j, :, 12:24].sum(axis=0)[ok] / em[j, :, 24:36].sum(axis=0)[ok], rtol=1e-15)
        assert r[7] == np.inf and r[3] == 0.25, "nr = 0 keeps r; +inf stays +inf"
        assert new[j].alpha == 0.5
    # masks, scalar and per component
    new, _ = estimate.em_update(em, info, sinfo, cfg, fit_q=False)
    assert np.all(np.array(list(new[0].q)) == 0.5) and new[0].r[0] != 0.25
    mask = np.zeros(12, bool)
    mask[[0, 5]] = True
    new, _ = estimate.em_update(em, info, sinfo, [cfg, cfg], fit_q=mask, fit_r=~mask)
    q, r = np.array(list(new[1].q)), np.array(list(new[1].r))
    assert np.all(q[~mask] == 0.5) and np.all(q[mask] != 0.5) and np.all(r[mask] == 0.25) and r[1] != 0.25
    # floors
    new, _ = estimate.em_update(em, info, sinfo, cfg, q_floor=10.0, r_floor=20.0)
    assert np.all(np.array(list(new[0].q)) == 10.0) and new[0].r[0] == 20.0 and new[0].r[7] == np.inf and new[0].r[3] == 0.25
    # failed problems are left out and counted: a failed filter, a failed backward pass, no row at all (NaN statistics)
    info2, sinfo2, em2 = info.copy(), sinfo.copy(), em.copy()
    info2[0, 0, 2] = 4
    sinfo2[0, 1, 0] = 2
    em2[0, 1] = np.nan
    sinfo2[1, 2] = np.nan
    em2[1, 2] = np.nan
    new, left = estimate.em_update(em2, info2, sinfo2, cfg)
    assert left == 3
    assert np.allclose(np.array(list(new[0].q)), em[0, 2, :12] / 11.0, rtol=1e-15)
    assert np.allclose(np.array(list(new[1].q)), em[1, :2, :12].sum(axis=0) / 22.0, rtol=1e-15)
    info2[0, 2, 2] = 0
    with pytest.raises(ValueError, match="candidate 0"):
        estimate.em_update(em2, info2, sinfo2, cfg)
    # the reference's M-step says the same
    want, left = uer.m_step(em, info, sinfo, [ur.cfg(0.5, r0, 0.5)] * 2)
    new, _ = estimate.em_update(em, info, sinfo, cfg)
    assert left == 0 and all(np.array_equal(np.array(list(n.q)), w[0]) and np.array_equal(np.array(list(n.r)), w[1]) for n, w in zip(new, want))


@pytest.mark.parametrize("name", ue.NAMES)
def test_gpu_cases_are_well_posed(name):
    """the fp64 against long-double gap of em is below a tenth of the bound of tests/test_ukf_em_gpu.py, with and without a terminal
    pair; counts, zeros and the never-measured component are exact"""
    i = ue.inputs(name)
    for pair in (False, True):
        o, ol = ue.reference(name, pair=pair), ue.reference(name, ld=True, pair=pair)
        gap = ue.em_err(o["em"], ol["em"])
        print(name, "pair" if pair else "no pair", "gap", gap)
        assert gap < 0.1 * ue.TOL
        em = o["em"]
        assert np.isfinite(em).all() and np.all(em[..., 36] == (uc.T if pair else uc.T - 1))
        assert np.all(em[..., 12 + uc.UNMEASURED] == 0) and np.all(em[..., 24 + uc.UNMEASURED] == 0)
        seen = (~np.isnan(i["Y"])).sum(axis=1).astype(float)
        seen[:, uc.UNMEASURED] = 0
        assert np.array_equal(em[..., 24:36], np.broadcast_to(seen, em[..., 24:36].shape))
        if name == "zeroq":
            assert np.all(em[..., [2, 9]] == 0.0) and np.all(em[..., [0, 1, 3]] > 0)
    if name == "bigq":
        q = i["cfgs"].q
        corr = 1.0 - ue.reference(name)["em"][..., :12] / (11 * q)
        print("bigq: the correction term over q, smallest and largest", corr.min(), corr.max())
        assert corr.max() > 0.1, "the correction term must be no 2 % effect in this case"


@pytest.mark.parametrize("name", ["wr_rk4", "thr_rk4"])
def test_em_loop_on_the_reference(name):
    """eight EM iterations at T = 40, B = 3 under the true vehicle from (q x 100, sigma x 3): the log-likelihood rises at every
    iteration, every measured component ends with sqrt(r) / sigma in [0.6, 1.5], component 7 stays +inf"""
    i = ue.long_inputs(name)
    o = uer.em(i["model"], uc.INTEG[i["integ"]], i["lag_mode"], [fv.vehicle(uc.TRUE)], i["cfgs"], i["x0"], i["P0"], i["U"], i["Y"], uc.DT, 8)
    ll = o["loglik"][:, 0]
    print(name, "loglik", ll)
    assert ll.shape == (9,) and np.all(np.diff(ll) > 0)
    ratio = np.sqrt(o["r"][0] / uc.SIGMA ** 2)
    print(name, "sqrt(r) / sigma", ratio)
    m = np.arange(12) != uc.UNMEASURED
    assert np.isposinf(o["r"][0, uc.UNMEASURED]) and np.all(ratio[m] >= 0.6) and np.all(ratio[m] <= 1.5)
    assert np.all(o["q"] > 0) and np.all(np.isfinite(o["q"]))
