"""CPU checks of the PINc inference path (bluerov2_dynamics_amd/pinc.py): weight packing and validation, the NumPy oracle
(oracle/pinc_numpy.py: PINcNet.forward, simulate_pinc, the windowed evaluator; training/train_tank_brov2_full_comparison.py:601-721,
838-890) pinned to the reference's outputs in tests/golden/pinc_kat.npz, pinc_rand_kat.npz and cfg5_pinc.npz, the torch-free import,
and the C ABI's answer without a GPU.  No kernel is launched."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, REPO, load_golden, rel_err
from oracle import fossen_c, pinc_numpy


def _weights_npz():
    return os.path.join(GOLDEN, "pinc_weights.npz")


def test_blob_is_state_dict_order_whatever_the_source():
    from bluerov2_dynamics_amd import pinc
    g = load_golden("pinc_weights.npz")
    sd = {k: g[k] for k in g.files}
    assert list(sd) == list(pinc.KEYS) and len(pinc.KEYS) == 22
    w_npz = pinc.PINcWeights(_weights_npz())
    assert w_npz.blob.dtype == np.float32 and w_npz.blob.size == pinc.NPARAMS == 14541
    np.testing.assert_array_equal(w_npz.blob, np.concatenate([sd[k].ravel() for k in pinc.KEYS]))

    class Duck:                      # the reference's PINcNet is read through .state_dict() only
        def state_dict(self):
            return {k: sd[k].astype(np.float64) for k in reversed(list(sd))}

    for src in (dict(sd), Duck(), w_npz):
        assert pinc.PINcWeights(src).blob.tobytes() == w_npz.blob.tobytes()
    # the first layer's rows, then its bias, then the scalar beta: offsets of the packed layout
    assert w_npz.blob[896] == sd["net.0.bias"][0] and w_npz.blob[960] == sd["net.1.beta"]
    assert w_npz.blob[13956] == sd["net.12.weight"][0, 0] and w_npz.blob[-1] == sd["net.12.bias"][-1]


def test_bad_weights_raise_value_error_naming_the_key():
    from bluerov2_dynamics_amd import pinc
    g = load_golden("pinc_weights.npz")
    sd = {k: g[k] for k in g.files}
    bad = dict(sd)
    bad["net.6.weight"] = np.zeros((64, 32), np.float32)
    with pytest.raises(ValueError, match=r"net\.6\.weight"):
        pinc.PINcWeights(bad)
    missing = dict(sd)
    del missing["net.10.beta"]
    with pytest.raises(ValueError, match=r"net\.10\.beta"):
        pinc.PINcWeights(missing)
    extra = dict(sd)
    extra["net.13.weight"] = np.zeros((9, 9), np.float32)
    with pytest.raises(ValueError, match=r"net\.13\.weight"):
        pinc.PINcWeights(extra)


def test_numpy_restatement_reproduces_the_reference_forward():
    g = load_golden("pinc_weights.npz")
    sd = {k: g[k] for k in g.files}
    kat = load_golden("pinc_kat.npz")
    assert kat["z"].shape[1] == 14 and len(kat["z"]) >= 900 and int(kat["n_threshold_rows"]) > 0
    assert rel_err(pinc_numpy.forward(sd, kat["z"], fp32=True), kat["x_next"]) < 1e-5
    # the fixture's own evaluator sequence reproduces the committed fourth row of config 5
    assert rel_err(kat["rmse_seq"], load_golden("cfg5_pinc.npz")["pinc_row"]) < 1e-12


def test_importing_pinc_does_not_import_torch():
    code = ("import sys; sys.path.insert(0, sys.argv[1]); import numpy as np\n"
            "from bluerov2_dynamics_amd import pinc\n"
            "w = pinc.PINcWeights(sys.argv[2])\n"
            "assert 'torch' not in sys.modules, 'torch imported'\n"
            "print(w.blob.size)")
    out = subprocess.run([sys.executable, "-c", code, REPO, _weights_npz()], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    assert out.stdout.strip() == "14541"


def test_entry_points_without_a_gpu_report_nodevice():
    from bluerov2_dynamics_amd import _build, _lib, pinc
    _build.build_library()
    lib = _lib.load_library()
    import ctypes
    h = ctypes.c_void_p()
    rc = lib.brov_create(0, ctypes.byref(h))
    if rc == 0:                      # a gfx950 device is visible (the GPU box): tests/test_pinc_gpu.py covers the device path
        lib.brov_destroy(h)
    else:
        assert rc == -4                                                    # BROV_ERR_NODEVICE
        with pytest.raises(_lib.BrovError, match="BROV_ERR_NODEVICE"):
            pinc.PINc(_weights_npz(), ctx=_lib.Context(0))
    # without a ctx the entry points refuse the call (BROV_ERR_ARG) instead of touching a device
    blob = pinc.PINcWeights(_weights_npz()).blob
    assert lib.brov_pinc_set_weights(None, blob.ctypes.data, blob.size) == -1
    assert lib.brov_pinc_forward_dev(None, 1, None, None) == -1
    assert lib.brov_pinc_rollout(None, 1, 1, 0.02, None, None, None, None, 1, None) == -1
    assert lib.brov_pinc_rollout_dev(None, 1, 1, 0.02, None, None, None, None, 1, None) == -1
    assert lib.brov_pinc_window_endpoint_se(None, 10, 1, 0.02, None, None, 1, None, None, None, None) == -1
    assert lib.brov_pinc_window_endpoint_se_dev(None, 10, 1, 0.02, None, None, 1, None, None, None, None) == -1


def _rand_sets():
    from bluerov2_dynamics_amd.pinc import KEYS
    g = load_golden("pinc_rand_kat.npz")
    return [({k: g[f"w{s}_{k}"] for k in KEYS}, g[f"z{s}"], g[f"y32_{s}"], g[f"y64_{s}"]) for s in range(3)]


def test_oracle_forward_equals_the_reference_in_fp64_on_random_weights():
    """beta 8 / 0.05 / -0.5 past softplus's threshold, LayerNorm variance ~ eps, cos/sin at the 1e-6 clamp: the oracle's fp64
    forward is the reference's net.double() to rounding, and its fp32 mode lands as close to torch's fp32 as fp32 itself allows."""
    sets = _rand_sets()
    assert float(sets[0][0]["net.1.beta"]) == 8.0 and float(sets[1][0]["net.1.beta"]) == -0.5
    for sd, z, y32, y64 in sets:
        assert rel_err(pinc_numpy.forward(sd, z), y64) < 1e-12
        dev = rel_err(y32, y64)                                  # torch's own fp32 error on these rows
        assert rel_err(pinc_numpy.forward(sd, z, fp32=True), y32) < 4 * dev + 1e-6
    # set 2: 70 rows whose (cos, sin) before renormalisation is a few fp32 ulps, below the clamp
    sd, z, _, y64 = sets[2]
    c, s = z[:70, 3] + sd["net.12.bias"][3], z[:70, 4] + sd["net.12.bias"][4]
    assert np.all(np.hypot(c, s) < 1e-6) and np.all(np.hypot(y64[:70, 3], y64[:70, 4]) < 0.5)


def test_oracle_reproduces_the_checkpoint_fixtures():
    """forward, simulate_pinc (500 steps) and the evaluator sequence H = 1 / 10 / 100 with one map vehicle, within the bounds
    tests/test_pinc_gpu.py puts on the kernels."""
    g = load_golden("pinc_weights.npz")
    sd = {k: g[k] for k in g.files}
    kat = load_golden("pinc_kat.npz")
    c5 = load_golden("cfg5.npz")
    X, U, dt, split = c5["X"], c5["U"], float(c5["dt"]), int(c5["split"])
    assert rel_err(pinc_numpy.forward(sd, kat["z"]), kat["x_next"]) < 1e-5
    k = int(kat["start500"])
    r = pinc_numpy.rollout(sd, X[k][None], U[k:k + 500][None], dt)
    assert np.array_equal(r["traj"][0, 0], X[k]) and np.array_equal(r["traj"][0, -1], r["xT"][0])
    assert rel_err(r["traj"][0], kat["traj500"]) < 2e-5
    assert rel_err(r["lag"][0], kat["lag500"]) < 1e-12
    Xte, Ute = X[split:], U[split:]
    lag, row = None, []
    for H in (1, 10, 100):
        if H == 10:
            assert rel_err(lag, kat["lag_before_H10"]) < 1e-12
        w = pinc_numpy.window_endpoint_se(sd, Xte, Ute, H, dt, lag=lag)
        if H == 10:
            se_ref = np.sum((kat["endpoints_H10"] - Xte[10:]) ** 2, axis=1)
            assert np.max(np.abs(w["per_window"] - se_ref) / np.maximum(se_ref, 1e-12)) < 1e-4
        row.append(np.sqrt(w["se"] / ((len(Xte) - H) * 12)))
        lag = w["lag"]
    ref = load_golden("cfg5_pinc.npz")["pinc_row"]
    assert np.max(np.abs(np.array(row) - ref) / np.abs(ref)) < 1e-5, (row, ref)
    assert rel_err(lag, kat["lag_after_seq"]) < 1e-9


@pytest.mark.parametrize("dt", [0.02, 0.05])
def test_oracle_lag_recurrence_and_u4_equal_the_c_thruster_map(dt):
    """The NumPy lag recurrence (vectorised over the 8 thrusters) and its u4 = tau[0, 1, 2, 5] against one
    fossen_c.thruster_forces call per sample, from a nonzero lag; the window starts against the same loop."""
    rng = np.random.default_rng(5)
    U = rng.uniform(-1, 1, (300, 8))
    s0 = rng.normal(0, 0.5, (8, 3))
    u4, lag_np = pinc_numpy.thruster_stream(U, dt, lag=s0)
    lag = s0[None].copy()
    want = np.empty((len(U), 4))
    for t in range(len(U)):
        tau, lag = fossen_c.thruster_forces(U[t], dt, lag=lag)
        want[t] = tau[0, [0, 1, 2, 5]]
    assert rel_err(u4, want) < 1e-12 and rel_err(lag_np, lag[0]) < 1e-12
    H, nwin = 7, 40
    starts, end = pinc_numpy.lag_starts(U, H, dt, nwin, lag=s0)
    lag = s0[None].copy()
    for k in range(nwin):
        assert np.array_equal(starts[k], lag[0])                 # the same operations in the same order: equal bits
        for t in range(H):
            _, lag = fossen_c.thruster_forces(U[k + t], dt, lag=lag)
    assert np.array_equal(end, lag[0])
