"""The multiplicative filter of the quaternion model without a GPU: the reference of the parity tests (tests/ukf_quat_ref.py, the law
of include/brov2.h: brov_ukf_filter_quat restated in NumPy) -- the well-posedness of every problem that tests/test_ukf_quat_gpu.py
runs on the device (tests/ukf_quat_cases.py), its agreement with the Euler filter's update where the two coincide, a simulated
recording that starts near vertical, and the power of the cases to tell the law from its neighbours; then the ABI mirror and the
host-side helpers of fossen/estimate.py."""
import ctypes

import numpy as np
import pytest

import fossen_vehicles as fv
import ukf_cases as uc
import ukf_quat_cases as qc
import ukf_quat_ref as uq
import ukf_ref as ur
from oracle import fossen_params as fp

L = np.longdouble
TOL_ROLL = 1e-10            # the bound of tests/test_ukf_quat_gpu.py


@pytest.fixture(scope="module")
def lib():
    from bluerov2_dynamics_amd import _build, _lib
    _build.build_library()
    return _lib.load_library()


# ------------------------------------------------------------------------------------------ the reference
@pytest.mark.parametrize("name", sorted(qc.CASES))
def test_gpu_cases_are_well_posed(name):
    """Every problem of tests/test_ukf_quat_gpu.py on the reference alone: fp64 against long double within a tenth of the parity
    bound in every output, no [-] beyond a third of a turn (|e_w| > 0.5), no small pivot, no failed filter."""
    o, ol = qc.reference(name), qc.reference(name, ld=True)
    g = qc.gaps(o, ol)
    print(name, {k: f"{v:.1e}" for k, v in g.items()}, "smallest |e_w|", o["ew_min"].min(), "smallest pivot", o["pivot_min"].min())
    assert max(g.values()) < 0.1 * TOL_ROLL, g
    assert min(o["ew_min"].min(), ol["ew_min"].min()) > 0.5
    assert min(o["pivot_min"].min(), ol["pivot_min"].min()) > 1e-4
    assert np.all(o["info"][..., 2] == -1) and np.all(np.isfinite(o["xT"])) and np.all(np.isfinite(o["PT"]))
    i = qc.inputs(name)
    seen = np.delete(i["Y"], qc.UNMEASURED + 1, axis=2)       # (the never-measured column carries numbers on purpose)
    assert 0.2 < np.isnan(seen).mean() < 0.45 and np.isnan(seen[:, qc.EMPTY_ROW]).all()
    assert np.isnan(o["innov"][:, :, qc.EMPTY_ROW]).all() and np.isnan(o["innov"][..., qc.UNMEASURED]).all()
    part = np.isnan(i["Y"][..., 3:7]).any(-1) & ~np.isnan(i["Y"][..., 3:7]).all(-1)
    assert part.any(), "a row with one number of the quaternion missing"
    assert np.isnan(o["innov"][0][part][:, 3:6]).all(), "such a row has no attitude measurement"
    assert np.all(np.isnan(i["P0"][:, np.triu_indices(12, 1)[0], np.triu_indices(12, 1)[1]]))
    assert qc.err(o["xf"][0], o["xf"][1]) > 1e3 * TOL_ROLL, "the candidates must differ"
    if qc.CASES[name][3] == "nrec2":
        one = uq.filter(qc.INTEG[i["integ"]], [fv.vehicle(n) for n in qc.NAMES], i["cfgs"][0], i["x0"], i["P0"], i["U"], i["Y"], qc.DT)
        assert qc.err(o["xf"][1], one["xf"][1]) > 1e3 * TOL_ROLL, "the second noise record must matter"
    if qc.CASES[name][3] == "vertical":
        q = i["X"][:, 0, 3:7]
        pitch = np.arcsin(2 * (q[:, 0] * q[:, 2] - q[:, 3] * q[:, 1]))
        assert np.all(np.abs(pitch - np.pi / 2) < 0.1)
        assert np.all(np.sum(i["x0"][:, 3:7] * q, -1) < -0.9), "x0's quaternion is on the other hemisphere"
        n = np.linalg.norm(i["Y"][:, :, 3:7], axis=-1)
        assert np.nanmax(n) > 1.9 and np.nanmin(n) < 1.1, "scaled and unit measured quaternions"


def test_cases_tell_the_law_from_its_neighbours():
    """Five edited copies of the reference -- [+] on the left, e = q_y (x) conj(q), v = z[i] without - d[i], x = chi_0' without
    [+] m, no Wc_0 m m^T term -- each move xf or PT by more than 1e3 TOL_ROLL on at least one case: a kernel that computed one of
    them would fail the parity tests."""
    for v in uq.VARIANTS:
        moves = []
        for name in sorted(qc.CASES):
            o, e = qc.reference(name), qc.reference(name, variant=v)
            moves.append(max(qc.err(e["xf"], o["xf"]), qc.cov_err(e["PT"], o["PT"])))
        print(v, " ".join(f"{m:.1e}" for m in moves))
        assert max(moves) > 1e3 * TOL_ROLL, (v, moves)


def test_position_and_velocity_update_is_the_euler_filter_s():
    """A row with every component measured and P block-diagonal between attitude and the rest: position and velocity do not see the
    attitude, and their outputs equal ukf_ref.update_row on the same numbers.  Long double, 1e-12."""
    rng = np.random.default_rng(23)
    lin = [0, 1, 2, 6, 7, 8, 9, 10, 11]
    for _ in range(5):
        M = rng.normal(size=(12, 12))
        Pm = (0.5 * np.eye(12) + M @ M.T / 12.0).astype(L) * L(1e-3)
        Pm = (Pm + Pm.T) / L(2)
        Pm[np.ix_(lin, [3, 4, 5])] = 0
        Pm[np.ix_([3, 4, 5], lin)] = 0
        x = qc.start_states(rng, 1, True)[0].astype(L)
        r = rng.uniform(1e-4, 1e-3, 12).astype(L)
        y = uq.boxplus(x, (rng.normal(size=12) * 0.03).astype(L))
        y[3:7] *= L(-1.7)
        xs, Ps, innov, dl, napp, ew, bad = uq.update_row(x, Pm, y, r, L)
        assert not bad and napp == 12 and not np.isnan(innov).any() and ew > 0.99
        # the same numbers through the Euler filter: its components 3 .. 5 carry the chart's innovation from an estimate of zero
        x12 = np.concatenate([x[:3], np.zeros(3, dtype=L), x[7:]])
        y12 = np.concatenate([y[:3], uq.att_minus(y[3:7], x[3:7])[0], y[7:]])
        xe, Pe, inn_e, dle, nappe, _, shifted, bade = ur.update_row(x12, Pm, y12, r, L)
        assert not bade and nappe == 12 and shifted == 0
        got = np.concatenate([xs[:3], xs[7:]])
        assert uc.err(got, xe[lin]) < 1e-12 and uc.err(innov, inn_e) < 1e-12 and uc.cov_err(Ps, Pe) < 1e-12 and uc.err(dl, dle) < 1e-12
        assert uc.err(uq.boxminus(xs, x)[0][3:6], xe[3:6]) < 1e-12, "the attitude correction is the Euler filter's, applied through [+]"
        assert np.array_equal(Ps, Ps.T)


def _recording(T=200, seed=3):
    """a seeded recording of the quaternion vehicle with a current (V5) under smooth commands, started within 0.1 rad of pitch 90
    degrees: truth X [T+1,13], U [T,6], noisy Y with the dropouts of tests/ukf_quat_cases.py and error component 7 never measured"""
    rng = np.random.default_rng(seed)
    t = np.arange(T) * qc.DT
    U = 0.5 * np.sin(2 * np.pi * np.outer(t, np.linspace(0.3, 1.0, 6)) + rng.uniform(0, 6, 6)) * uc.chan_scale(1)
    x0 = qc.start_states(rng, 1, True)
    X = fp.rollout(fp.WRENCH_QUAT, fp.EULER, 0, fv.vehicle("V5"), x0, U[None], qc.DT)["traj"][0]
    Y = qc.measure(rng, X[:T])
    Y[:, qc.UNMEASURED + 1] = np.nan
    xs = qc.boxplus(X[0], rng.normal(size=12) * qc.SIGMA)              # a start as good as one measurement (row 0 itself may be gappy)
    return X, U, Y, xs


def test_filter_beats_raw_measurements_and_ranks_the_true_vehicle():
    """T = 200 from a start near vertical: the filtered RMSE over the second half is below the raw RMSE on the same entries in
    position, attitude (through [-]) and velocity, the normalised innovations have a mean square near 1, and the log-likelihood of
    the true vehicle exceeds that of the vehicle with mass + 20 %."""
    T = 200
    X, U, Y, xs = _recording(T)
    heavy = fv.params("V5")
    heavy.m *= 1.2
    k = uc.noise_cfg(1.0)
    P0 = np.diag(np.where(np.isfinite(k.r), 4.0 * np.where(np.isfinite(k.r), k.r, 0.0), 1.0))
    o = uq.filter(fp.EULER, [fv.vehicle("V5"), fp.from_brov_params(heavy)], k, xs[None], P0[None], U[None], Y[None], qc.DT)
    assert np.all(o["info"][:, 0, 2] == -1) and o["ew_min"].min() > 0.5
    half = slice(T // 2, T)
    att = ~np.isnan(Y[:, 3:7]).any(-1)
    seen = np.concatenate([~np.isnan(Y[:, :3]), np.repeat(att[:, None], 3, 1), ~np.isnan(Y[:, 7:])], 1)[half]
    Yf = np.where(np.isnan(Y), X[:T], Y)                              # (entries that are not seen are masked below)
    raw, filt = qc.boxminus(Yf, X[:T])[half], qc.boxminus(o["xf"][0, 0], X[:T])[half]
    nis = np.nanmean(o["innov"][0, 0] ** 2)
    ll = o["info"][:, 0, 0]
    for what, cols in (("position", slice(0, 3)), ("attitude", slice(3, 6)), ("velocity", slice(6, 12))):
        a, b = np.sqrt(np.mean(raw[:, cols][seen[:, cols]] ** 2)), np.sqrt(np.mean(filt[:, cols][seen[:, cols]] ** 2))
        print(f"{what}: raw RMSE {a:.4f}  filtered RMSE {b:.4f}")
        assert b < a, what
    print(f"mean squared normalised innovation {nis:.2f}  log-likelihood true {ll[0]:.1f}, mass + 20 % {ll[1]:.1f}")
    assert 0.7 < nis < 1.3
    assert ll[0] > ll[1]


# ------------------------------------------------------------------------------------------ the ABI, the build
def test_signatures_and_symbols(lib):
    """_lib.SIGNATURES carries both forms with the 19 arguments of the header, and the built library exports them"""
    from bluerov2_dynamics_amd import _build, _lib
    assert "ukf_quat.hip" in _build.SOURCES and not _build.stale()
    for name in ("brov_ukf_filter_quat", "brov_ukf_filter_quat_dev"):
        res, args = _lib.SIGNATURES[name]
        assert res is ctypes.c_int and len(args) == 19
        assert args[3] == ctypes.POINTER(_lib.BrovParams) and args[5] == ctypes.POINTER(_lib.BrovUkf) and args[8] is ctypes.c_double
        fn = getattr(lib, name)
        assert fn.restype is ctypes.c_int and len(fn.argtypes) == 19
    assert lib.brov_ukf_filter_quat(None, 1, 1, None, 1, None, 1, 1, 0.02, *([None] * 10)) == -1      # a NULL ctx, without a device


# ------------------------------------------------------------------------------------------ fossen/estimate.py
def test_boxplus_boxminus():
    """estimate.quat_boxplus / quat_boxminus over leading dimensions: they are the reference's, they round-trip to 1e-15, and they
    do not see the sign (boxminus: nor the norm) of either quaternion"""
    from bluerov2_dynamics_amd.fossen import estimate
    rng = np.random.default_rng(31)
    X = np.concatenate([qc.start_states(rng, 6, False), qc.start_states(rng, 6, True)]).reshape(3, 4, 13)
    D = rng.uniform(-0.5, 0.5, (3, 4, 12))
    Z = estimate.quat_boxplus(X, D)
    assert Z.shape == (3, 4, 13) and np.max(np.abs(Z - qc.boxplus(X, D))) < 1e-15
    assert np.max(np.abs(np.linalg.norm(Z[..., 3:7], axis=-1) - 1)) < 1e-15
    back = estimate.quat_boxminus(Z, X)
    assert back.shape == (3, 4, 12) and np.max(np.abs(back - D)) < 1e-15, np.max(np.abs(back - D))
    assert np.max(np.abs(back - qc.boxminus(Z, X))) < 1e-15
    assert np.max(np.abs(estimate.quat_boxplus(X, estimate.quat_boxminus(Z, X)) - Z)) < 1e-15
    flip = np.concatenate([np.ones(3), -np.ones(4), np.ones(6)])
    assert np.array_equal(estimate.quat_boxminus(Z * flip, X), back) and np.array_equal(estimate.quat_boxminus(Z, X * flip), back)
    scale = np.concatenate([np.ones(3), -2.0 * np.ones(4), np.ones(6)])
    assert np.array_equal(estimate.quat_boxminus(Z * scale, X), back)
    assert np.array_equal(estimate.quat_boxplus(X * flip, D), Z * flip)
    assert np.array_equal(estimate.quat_boxplus(X[0, 0], np.zeros(12)), X[0, 0])
    half = X[0, 0].copy()
    half[3:7] = uq.qmul(X[0, 0, 3:7], np.array([0.0, 1.0, 0.0, 0.0]))
    assert not np.isfinite(estimate.quat_boxminus(half, X[0, 0])[3:6]).all(), "half a turn leaves the finite numbers"


def test_default_start_quat():
    """the documented rules: the first row with every component of finite r present (the quaternion as a whole), its quaternion
    normalised, never-measured components at 0, the identity where the attitude is never measured, diag(4 r) with the stand-in"""
    from bluerov2_dynamics_amd.fossen import estimate
    c = estimate.ukf(1e-6, [1e-4] * 11 + [np.inf])
    Y = np.full((2, 5, 13), np.nan)
    Y[0, 2], Y[1, 0] = 1.0, 2.0
    Y[0, 2, 12] = np.nan                                       # never measured: need not be there
    Y[0, 1] = 3.0
    Y[0, 1, 5] = np.nan                                        # one number of the quaternion missing: not a complete row
    Y[1, 0, 3:7] = (0.0, -3.0, 0.0, 4.0)
    x0, P0 = estimate.default_start_quat(Y, c)
    assert np.allclose(x0[0], [1.0] * 3 + [0.5] * 4 + [1.0] * 5 + [0.0], atol=1e-15)
    assert np.allclose(x0[1], [2.0] * 3 + [0.0, -0.6, 0.0, 0.8] + [2.0] * 5 + [0.0], atol=1e-15)
    assert P0.shape == (2, 12, 12) and np.array_equal(P0[0], np.diag([4e-4] * 11 + [estimate.P0_STAND_IN])) and np.array_equal(P0[0], P0[1])
    with pytest.raises(ValueError):
        estimate.default_start_quat(Y[:, 3:], c)
    zero = Y.copy()
    zero[1, 0, 3:7] = 0.0
    with pytest.raises(ValueError):
        estimate.default_start_quat(zero, c)
    r = np.full(12, 1e-4)
    r[3:6] = np.inf
    x0, P0 = estimate.default_start_quat(Y, estimate.ukf(1e-6, r))
    assert np.array_equal(x0[:, 3:7], [[1.0, 0.0, 0.0, 0.0]] * 2) and np.all(np.diagonal(P0[0])[3:6] == estimate.P0_STAND_IN)
    assert np.array_equal(x0[0, :3], [3.0] * 3), "without an attitude to wait for, row 1 is complete"
    with pytest.raises(ValueError):
        estimate.ukf(1e-6, 1e-4, n=13)
