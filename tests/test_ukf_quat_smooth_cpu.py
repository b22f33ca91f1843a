"""The smoother of the quaternion model without a GPU: the reference of the parity tests (tests/ukf_quat_smooth_ref.py, the law of
include/brov2.h: brov_ukf_filter_tape_quat_dev / brov_ukf_rts_quat_dev restated in NumPy) -- the well-posedness of every problem that
tests/test_ukf_quat_smooth_gpu.py runs on the device (the five cases of tests/ukf_quat_cases.py), the properties of the law that
the GPU tests assert as bit identities, and the power of the cases to tell the law from six of its neighbours; then the ABI mirror
and the vehicle methods' refusals."""
import ctypes

import numpy as np
import pytest

import ukf_quat_cases as qc
import ukf_quat_smooth_ref as qs

TOL = qs.TOL
T = qc.T


@pytest.fixture(scope="module")
def lib():
    from bluerov2_dynamics_amd import _build, _lib
    _build.build_library()
    return _lib.load_library()


# ------------------------------------------------------------------------------------------ the reference
@pytest.mark.parametrize("name", qs.NAMES)
def test_gpu_cases_are_well_posed(name):
    """Every problem of tests/test_ukf_quat_smooth_gpu.py on the reference alone: fp64 against long double within a tenth of the parity
    bound in every smoothed output and tape field; no delta beyond a third of a turn (|e_w| > 0.5); no small pivot in either pass;
    no failed filter or transition; the forward half is ukf_quat_ref.filter; smoothing moves the estimate and the candidates differ."""
    o, ol = qs.reference(name), qs.reference(name, ld=True)
    g = qs.gaps(o, ol)
    print(name, {k: f"{v:.1e}" for k, v in g.items()}, "smallest |e_w| of a delta", o["ew_min"].min(), "smallest Pp pivot", o["pivot_min"].min(),
          "C compact vs chart", o["c_form"].max())
    assert max(g.values()) < 0.1 * TOL, g
    assert min(o["ew_min"].min(), ol["ew_min"].min(), o["f_ew_min"].min(), ol["f_ew_min"].min()) > qs.EW
    assert min(o["pivot_min"].min(), ol["pivot_min"].min(), o["f_pivot_min"].min(), ol["f_pivot_min"].min()) > qs.PIVOT
    assert np.all(o["nrows"] == T) and np.all(o["sinfo"][..., 0] == -1) and np.all(o["info"][..., 2] == -1)
    assert np.isfinite(o["xs"]).all() and np.isfinite(o["Ps"]).all() and np.isfinite(o["tape"][:, :, :T]).all()
    f = qc.reference(name)
    for k in ("xf", "pstd", "innov", "xT", "PT", "info"):
        assert np.array_equal(o[k], f[k], equal_nan=True), k
    assert np.array_equal(o["xs"][:, :, T - 1], o["xf"][:, :, T - 1]) and np.array_equal(o["pstd_s"][:, :, T - 1], o["pstd"][:, :, T - 1])
    assert np.array_equal(o["Ps"], o["Ps"].transpose(0, 1, 2, 4, 3))
    # chi_i [-] x = +-c L[:, i-1] holds to rounding, so the compact C is the sum over the sigma points
    assert o["c_form"].max() < 1e-12
    move = qc.err(o["xs"], o["xf"])
    att = np.abs(qc.boxminus(o["xs"], o["xf"])[..., 3:6]).max()
    print(name, "xs against xf", move, "largest attitude correction", att)
    assert move > 1e3 * TOL and att > 1e3 * TOL, "smoothing must move the estimate, attitude included"
    assert qc.err(o["xs"][0], o["xs"][1]) > 1e3 * TOL, "the candidates must differ"
    assert np.all(np.diagonal(o["Ps"], axis1=-2, axis2=-1)[:, :, :T - 1] <= np.diagonal(unpacked_Pf(o), axis1=-2, axis2=-1)[:, :, :T - 1] * (1 + 1e-12))


def unpacked_Pf(o):
    return qs.tape_fields(o["tape"])["Pf"]


def test_cases_tell_the_law_from_its_neighbours():
    """Six edited copies of the backward pass each move xs or Ps by more than 1e3 TOL on every case: a kernel that computed one of
    them would fail every parity test."""
    for v in qs.VARIANTS:
        moves = []
        for name in qs.NAMES:
            o, e = qs.reference(name), qs.reference(name, variant=v)
            moves.append(max(qc.err(e["xs"], o["xs"]), qc.cov_err(e["Ps"], o["Ps"])))
        print(v, " ".join(f"{m:.1e}" for m in moves))
        assert min(moves) > 1e3 * TOL, (v, moves)


def _negq(x):
    x = np.array(x)
    x[..., 3:7] = -x[..., 3:7]
    return x


def test_signs_norms_and_the_split_in_time():
    """What the GPU tests assert bit for bit, on the reference: a negated x0 quaternion negates xf's and xs's quaternions and nothing
    else; a negated or doubled terminal quaternion changes nothing; a span split at row s and chained through (xT, PT) forwards and
    (xs[0], Ps0) backwards is the unbroken call (here to rounding: NumPy's sums are not pinned)."""
    name = "q_rk4_vertical"
    i, o = qc.inputs(name), qs.reference(name)
    n = qs.smooth_case(name, x0=_negq(i["x0"]))
    for k in ("xf", "xs"):
        assert np.array_equal(n[k], _negq(o[k])), k
    for k in ("pstd", "innov", "PT", "info", "pstd_s", "Ps", "Ps0", "sinfo"):
        assert np.array_equal(n[k], o[k], equal_nan=True), k
    s = 5
    P = o["xf"].shape[0]
    for j in range(P):
        v = [qs.vehicles()[j]]
        integ = qc.INTEG[i["integ"]]
        first = qs.smooth(integ, v, i["cfgs"], i["x0"], i["P0"], i["U"][:, :s], i["Y"][:, :s], qc.DT)
        second = qs.smooth(integ, v, i["cfgs"], first["xT"][0], first["PT"][0], i["U"][:, s:], i["Y"][:, s:], qc.DT)
        term = (second["xs"][:, :, 0], second["Ps0"])
        back = qs.smooth(integ, v, i["cfgs"], i["x0"], i["P0"], i["U"][:, :s], i["Y"][:, :s], qc.DT, terminal=term)
        both = np.concatenate([back["xs"], second["xs"]], axis=2)
        assert qc.err(both, o["xs"][j:j + 1]) < 1e-13
        assert qc.cov_err(np.concatenate([back["Ps"], second["Ps"]], axis=2), o["Ps"][j:j + 1]) < 1e-12
        for scale in (-1.0, 2.0):
            t2 = term[0].copy()
            t2[..., 3:7] *= scale
            again = qs.smooth(integ, v, i["cfgs"], i["x0"], i["P0"], i["U"][:, :s], i["Y"][:, :s], qc.DT, terminal=(t2, term[1]))
            assert np.array_equal(again["xs"], back["xs"]) and np.array_equal(again["Ps"], back["Ps"]), scale


def test_failure_paths_of_the_reference():
    """The three numerical failures that the GPU tests provoke, on the reference: a zero measured quaternion at row s (nrows = s, rows
    < s are the T = s problem); a negative Pp diagonal entry at transition t (sinfo[0] = t, rows <= t NaN, rows > t kept); a terminal
    quaternion half a turn from xp_T (transition T-1 fails)."""
    name = "q_rk4"
    i, o = qc.inputs(name), qs.reference(name)
    s = 6
    Y = i["Y"].copy()
    Y[1, s, 3:7] = 0.0
    got = qs.smooth_case(name, Y=Y)
    short = qs.smooth_case(name, U=i["U"][:, :s], Y=i["Y"][:, :s])
    assert np.all(got["nrows"][:, 1] == s) and np.all(got["info"][:, 1, 2] == s)
    assert np.isnan(got["xs"][:, 1, s:]).all() and np.array_equal(got["xs"][:, 1, :s], short["xs"][:, 1]) and np.array_equal(got["Ps"][:, 1, :s], short["Ps"][:, 1])
    assert np.isnan(got["tape"][:, 1, s:]).all() and np.isfinite(got["tape"][:, 1, :s]).all()
    for b in (0, 2):
        assert np.array_equal(got["xs"][:, b], o["xs"][:, b])
    t = 4
    tape = o["tape"][0, 0].copy()
    tape[t, 91] = -tape[t, 91]
    r = qs.rts_one(o["xf"][0, 0], tape, T, np.float64)
    assert r["sinfo"][0] == t and np.isnan(r["xs"][:t + 1]).all() and np.isnan(r["Ps0"]).all()
    assert np.array_equal(r["xs"][t + 1:], o["xs"][0, 0, t + 1:]) and np.array_equal(r["Ps"][t + 1:], o["Ps"][0, 0, t + 1:])
    import ukf_quat_ref as uq
    xT = o["xT"][0, 0].copy()
    xT[3:7] = uq.qmul(np.array([0.5, 0.5, -0.5, 0.5]), np.array([0.0, 1.0, 0.0, 0.0]))
    tape = o["tape"][0, 0].copy()
    tape[T - 1, 81:85] = (0.5, 0.5, -0.5, 0.5)                     # every product is +-0.25: the four terms of e_w cancel exactly
    r = qs.rts_one(o["xf"][0, 0], tape, T, np.float64, terminal=(xT, o["PT"][0, 0]))
    assert r["sinfo"][0] == T - 1 and np.isnan(r["xs"]).all() and r["ew_min"] == 0.0


# ------------------------------------------------------------------------------------------ the ABI, the Python layers
def test_signatures_and_symbols(lib):
    """_lib.SIGNATURES carries the four entry points with the argument counts of the header, and the built library exports them"""
    from bluerov2_dynamics_amd import _lib, engine
    counts = dict(brov_ukf_filter_tape_quat_dev=21, brov_ukf_rts_quat_dev=14, brov_ukf_smooth_quat=25, brov_ukf_smooth_quat_dev=25)
    for name, n in counts.items():
        res, args = _lib.SIGNATURES[name]
        assert res is ctypes.c_int and len(args) == n, name
        fn = getattr(lib, name)
        assert fn.restype is ctypes.c_int and len(fn.argtypes) == n
    assert _lib.SIGNATURES["brov_ukf_smooth_quat"][1][-1] is ctypes.c_int64
    assert engine.UKF_TAPE_QUAT == 313 == qs.TAPE
    # a NULL ctx, without a device
    assert lib.brov_ukf_smooth_quat(None, 1, 1, None, 1, None, 1, 1, 0.02, *([None] * 15), 0) == -1
    assert lib.brov_ukf_rts_quat_dev(None, 1, 1, 1, *([None] * 10)) == -1


def test_vehicle_methods_refuse_the_other_family():
    """smooth_states stays the Euler vehicles' method and smooth_states_quat the quaternion vehicle's: each raises on the other family
    before anything reaches the library, and its message names the method to use"""
    from bluerov2_dynamics_amd.fossen import _vehicle
    from bluerov2_dynamics_amd import engine

    class Quat(_vehicle.VehicleBase):
        MODEL = engine.WRENCH_QUAT

        def __init__(self):
            pass

    class Euler(Quat):
        MODEL = engine.WRENCH_EULER
    with pytest.raises(NotImplementedError, match="smooth_states_quat"):
        Quat().smooth_states(None, None, 0.02, None)
    with pytest.raises(NotImplementedError, match="have smooth_states$"):
        Euler().smooth_states_quat(None, None, 0.02, None)
