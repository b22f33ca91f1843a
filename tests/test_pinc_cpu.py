"""CPU checks of the PINc inference path (bluerov2_dynamics_amd/pinc.py): weight packing and validation, a NumPy fp32
restatement of PINcNet.forward (training/train_tank_brov2_full_comparison.py:648-721) against the reference's outputs in
tests/golden/pinc_kat.npz, the torch-free import, and the C ABI's answer without a GPU.  No kernel is launched."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, REPO, load_golden, rel_err


def _weights_npz():
    return os.path.join(GOLDEN, "pinc_weights.npz")


def np_pinc_forward(sd, z):
    """PINcNet.forward in fp32 NumPy (summation order differs from torch's)."""
    f32 = np.float32
    z = np.asarray(z, dtype=f32)
    h = z
    for idx in (0, 3, 6, 9):
        a = h @ sd[f"net.{idx}.weight"].T + sd[f"net.{idx}.bias"]
        beta = f32(sd[f"net.{idx + 1}.beta"])
        y = beta * a
        sp = np.where(y > f32(20), y, np.log1p(np.exp(np.minimum(y, f32(20))))) / (beta + f32(1e-12))
        mean = sp.mean(axis=1, keepdims=True, dtype=f32)
        d = sp - mean
        var = (d * d).mean(axis=1, keepdims=True, dtype=f32)
        h = d / np.sqrt(var + f32(1e-5)) * sd[f"net.{idx + 2}.weight"] + sd[f"net.{idx + 2}.bias"]
    dx = h @ sd["net.12.weight"].T + sd["net.12.bias"]
    c, s = z[:, 3], z[:, 4]
    out = z[:, :9] + dx
    out[:, 0] = c * dx[:, 0] - s * dx[:, 1] + z[:, 0]
    out[:, 1] = s * dx[:, 0] + c * dx[:, 1] + z[:, 1]
    nrm = np.maximum(np.sqrt(out[:, 3] ** 2 + out[:, 4] ** 2), f32(1e-6))
    out[:, 3] /= nrm
    out[:, 4] /= nrm
    return out


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
    assert rel_err(np_pinc_forward(sd, kat["z"]), kat["x_next"]) < 1e-5
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
