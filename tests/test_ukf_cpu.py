"""The unscented Kalman filter without a GPU: the reference of the parity tests (tests/ukf_ref.py, the law of include/brov2.h:
brov_ukf_filter restated in NumPy) against textbook forms, on a simulated recording, and the well-posedness of every problem that
tests/test_ukf_gpu.py runs on the device (tests/ukf_cases.py); then the validation of fossen/estimate.py: ukf."""
import numpy as np
import pytest

import fossen_vehicles as fv
import ukf_cases as uc
import ukf_ref as ur
from oracle import fossen_params as fp

L = np.longdouble
TOL_ROLL = 1e-10            # the bound of tests/test_ukf_gpu.py


def test_sequential_update_equals_joint_update():
    """Every component measured, diagonal R: the scalar updates in sequence are the joint update K = P H^T (H P H^T + R)^-1 with
    H = I, and their log-likelihood terms add up to the joint Gaussian's.  Long double, 1e-12 mixed error."""
    rng = np.random.default_rng(11)
    for _ in range(5):
        M = rng.normal(size=(12, 12))
        Pm = (0.5 * np.eye(12) + M @ M.T / 12.0).astype(L) * L(1e-3)
        Pm = (Pm + Pm.T) / L(2)
        x = rng.uniform(-0.3, 0.3, 12).astype(L)
        r = rng.uniform(1e-4, 1e-3, 12).astype(L)
        y = (x + rng.normal(size=12) * 0.03).astype(L)
        xs, Ps, innov, dl, napp, _, shifted, bad = ur.update_row(x, Pm, y, r, L)
        assert not bad and napp == 12 and shifted == 0 and not np.isnan(innov).any()
        S = Pm + np.diag(r)
        v = y - x
        Sv = fp._solve(S, v[:, None])[:, 0]
        SP = fp._solve(S, Pm)
        xj = x + Pm @ Sv
        Pj = Pm - Pm @ SP
        Ls, fail, _ = ur.cholesky(S, L)
        assert not fail
        two_pi = L(2) * np.arccos(L(-1))
        lj = -(L(12) * np.log(two_pi) + L(2) * np.sum(np.log(np.diagonal(Ls))) + v @ Sv) / L(2)
        assert uc.err(xs, xj) < 1e-12 and uc.cov_err(Ps, Pj) < 1e-12 and uc.err(dl, lj) < 1e-12, (uc.err(xs, xj), uc.cov_err(Ps, Pj), uc.err(dl, lj))
        assert np.array_equal(Ps, Ps.T)


def _recording(T=200, seed=5):
    """a seeded recording of the thruster vehicle with a current (V5) under smooth commands: truth X [T+1,12], U [T,8], noisy Y with
    30 % dropouts and component 7 never measured"""
    rng = np.random.default_rng(seed)
    t = np.arange(T) * uc.DT
    U = 0.5 * np.sin(2 * np.pi * np.outer(t, np.linspace(0.3, 1.0, 8)) + rng.uniform(0, 6, 8))
    x0 = np.zeros(12)
    X = fp.rollout(0, fp.EULER, 0, fv.vehicle("V5"), x0[None], U[None], uc.DT)["traj"][0]
    Y = X[:T] + rng.normal(size=(T, 12)) * uc.SIGMA
    Y[rng.uniform(size=Y.shape) < 0.3] = np.nan
    Y[:, uc.UNMEASURED] = np.nan
    return X, U, Y


def test_filter_beats_raw_measurements_and_ranks_the_true_vehicle():
    """T = 200: the filtered RMSE over the second half is below the raw RMSE on the same entries, the normalised innovations have
    a mean square near 1, and the log-likelihood of the true vehicle exceeds that of the vehicle with mass + 20 %."""
    T = 200
    X, U, Y = _recording(T)
    heavy = fv.params("V5")
    heavy.m *= 1.2
    k = uc.noise_cfg(1.0)
    P0 = np.diag(np.where(np.isfinite(k.r), 4.0 * np.where(np.isfinite(k.r), k.r, 0.0), 1.0))
    o = ur.filter(0, fp.EULER, 0, [fv.vehicle("V5"), fp.from_brov_params(heavy)], k, np.zeros((1, 12)), P0[None], U[None], Y[None], uc.DT)
    assert np.all(o["info"][:, 0, 2] == -1)
    half = slice(T // 2, T)
    seen = ~np.isnan(Y[half])
    raw = np.sqrt(np.mean((Y[half] - X[:T][half])[seen] ** 2))
    filt = np.sqrt(np.mean((o["xf"][0, 0, half] - X[:T][half])[seen] ** 2))
    inn = o["innov"][0, 0]
    nis = np.nanmean(inn ** 2)
    ll = o["info"][:, 0, 0]
    print(f"raw RMSE {raw:.4f}  filtered RMSE {filt:.4f}  mean squared normalised innovation {nis:.2f}  log-likelihood true {ll[0]:.1f}, mass + 20 % {ll[1]:.1f}")
    assert filt < raw
    assert 0.7 < nis < 1.3
    assert ll[0] > ll[1]


@pytest.mark.parametrize("name", sorted(uc.CASES))
def test_gpu_cases_are_well_posed(name):
    """Every problem of tests/test_ukf_gpu.py on the reference alone: fp64 against long double within a tenth of the parity bound,
    no wrap near its threshold, no small pivot, no failed filter."""
    o, ol = uc.reference(name), uc.reference(name, ld=True)
    g = uc.gaps(o, ol)
    print(name, {k: f"{v:.1e}" for k, v in g.items()}, "wrap margin", o["wrap_margin"].min(), "smallest pivot", o["pivot_min"].min())
    assert max(g.values()) < 0.1 * TOL_ROLL, g
    assert min(o["wrap_margin"].min(), ol["wrap_margin"].min()) > 1e-6
    assert min(o["pivot_min"].min(), ol["pivot_min"].min()) > 1e-4
    assert np.all(o["info"][..., 2] == -1) and np.all(np.isfinite(o["xT"])) and np.all(np.isfinite(o["PT"]))
    i = uc.inputs(name)
    seen = np.delete(i["Y"], uc.UNMEASURED, axis=2)            # (the never-measured column carries numbers on purpose)
    assert 0.2 < np.isnan(seen).mean() < 0.45 and np.isnan(seen[:, uc.EMPTY_ROW]).all()
    assert np.isnan(o["innov"][:, :, uc.EMPTY_ROW]).all() and np.isnan(o["innov"][..., uc.UNMEASURED]).all()
    if uc.CASES[name][5] == "wrap":
        assert o["shifted"].min() > 0, "at least one innovation of every filter must be shifted by 2 pi"
    if name == "thr_rk4_lagstep":
        assert uc.err(o["xf"], uc.reference(name, lag_mode=0)["xf"]) > 1e3 * TOL_ROLL, "the lag mode must matter"
    if uc.CASES[name][5] == "nrec2":
        one = ur.filter(i["model"], uc.INTEG[i["integ"]], i["lag_mode"], [fv.vehicle(n) for n in uc.NAMES], i["cfgs"][0], i["x0"], i["P0"],
                        i["U"], i["Y"], uc.DT)
        assert uc.err(o["xf"][1], one["xf"][1]) > 1e3 * TOL_ROLL, "the second noise record must matter"


def test_ukf_record_validation():
    from bluerov2_dynamics_amd.fossen import estimate
    c = estimate.ukf(1e-6, [1e-4] * 11 + [np.inf], alpha=0.5, beta=2.0, kappa=1.0)
    assert list(c.q) == [1e-6] * 12 and list(c.r)[:11] == [1e-4] * 11 and c.r[11] == np.inf
    assert (c.alpha, c.beta, c.kappa) == (0.5, 2.0, 1.0)
    d = estimate.ukf(0.0, 0.0)
    assert (d.alpha, d.beta, d.kappa) == (1.0, 2.0, 1.0)
    for bad in (dict(q=-1e-6, r=1e-4), dict(q=1e-6, r=-1e-4), dict(q=np.inf, r=1e-4), dict(q=np.nan, r=1e-4), dict(q=1e-6, r=np.nan),
                dict(q=1e-6, r=1e-4, alpha=0.0), dict(q=1e-6, r=1e-4, alpha=-1.0), dict(q=1e-6, r=1e-4, alpha=np.inf),
                dict(q=1e-6, r=1e-4, alpha=np.nan), dict(q=1e-6, r=1e-4, kappa=-12.0), dict(q=1e-6, r=1e-4, kappa=-13.0),
                dict(q=1e-6, r=1e-4, kappa=np.nan), dict(q=1e-6, r=1e-4, beta=np.nan), dict(q=[1e-6] * 11, r=1e-4), dict(q=1e-6, r=1e-4, n=13)):
        with pytest.raises(ValueError):
            estimate.ukf(**bad)
    # the default start of filter_states: the first fully measured row (the never-measured component aside), diag(4 r) with the stand-in
    Y = np.full((2, 5, 12), np.nan)
    Y[0, 2], Y[1, 0] = 1.0, 2.0
    Y[0, 2, 11] = np.nan
    Y[0, 1, :5] = 3.0
    x0, P0 = estimate.default_start(Y, c)
    assert np.array_equal(x0[0], [1.0] * 11 + [0.0]) and np.array_equal(x0[1], [2.0] * 11 + [0.0])      # never measured: starts at 0
    assert np.array_equal(P0[0], np.diag([4e-4] * 11 + [estimate.P0_STAND_IN])) and np.array_equal(P0[0], P0[1])
    with pytest.raises(ValueError):
        estimate.default_start(Y[:, 3:], c)
