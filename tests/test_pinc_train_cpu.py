"""PINc training without a GPU: the NumPy restatement (tests/pinc_train_ref.py) against the reference's own autograd and AdamW
(tests/golden/pinc_train*.npz, written by tools/gen_golden.py gen_pinc_train), the dataset builder, and the host-side API."""
import os
import subprocess
import sys

import numpy as np
import pytest

import pinc_train_ref as R
from conftest import REPO

GOLD = os.path.join(REPO, "tests", "golden")
BATCHES = ("b256", "b254", "b2")


@pytest.fixture(scope="module")
def fx():
    d = np.load(os.path.join(GOLD, "pinc_train.npz"))
    ck = np.load(os.path.join(GOLD, "pinc_weights.npz"))
    return dict(d=d, grad=np.load(os.path.join(GOLD, "pinc_train_grad.npz")), opt=np.load(os.path.join(GOLD, "pinc_train_opt.npz")),
                opt20=np.load(os.path.join(GOLD, "pinc_train_opt20.npz")),
                sets=dict(ckpt={k: ck[k] for k in R.KEYS}, fresh={k: d["fresh." + k] for k in R.KEYS}),
                Z=d["z"].astype(np.float32), Y=d["y"].astype(np.float32), U=d["U4"][:-1].astype(np.float32))


@pytest.fixture(scope="module")
def run64(fx):
    return R.train(fx["sets"]["fresh"], fx["Z"], fx["Y"], fx["U"], fx["d"]["iters"])


@pytest.mark.parametrize("wset", ["ckpt", "fresh"])
@pytest.mark.parametrize("batch", BATCHES)
def test_gradient_oracle_matches_reference_autograd(fx, wset, batch):
    """fp64 restatement vs the reference's PINcNet / rollout_loss / physics_loss under autograd in fp64, per tensor |dg|/|g|.
    Measured: at most 2.4e-13 over the 22 tensors x 6 cases (the beta scalars are the worst), loss terms at most 1.5e-15.
    Bounds: 2.4e-12 (10 x measured) and 2e-14."""
    idx = fx["d"]["idx_" + batch]
    loss, _, g = R.loss_and_grad(fx["sets"][wset], fx["Z"][idx], fx["Y"][idx], fx["U"][idx], min(10, len(idx) - 1))
    err = R.tensor_rel_errors(g, fx["grad"][f"grad_{wset}_{batch}"])
    ref = fx["d"][f"loss_f64_{wset}_{batch}"]
    lerr = float(np.max(np.abs(loss - ref) / np.abs(ref)))
    print(wset, batch, "grad", max(err.values()), max(err, key=err.get), "loss", lerr)
    assert max(err.values()) < 2.4e-12, err
    assert lerr < 2e-14, (loss, ref)


def test_optimiser_oracle_matches_reference_adamw(fx, run64):
    """Weights, exp_avg and exp_avg_sq after 1, 5 and 20 iterations of the reference's loop body (fp64) and its loss terms.
    Measured: at most 7.4e-13 per tensor (exp_avg after 20), losses 3.3e-13.  Bounds: 7.4e-12 and 3.3e-12 (10 x measured)."""
    worst = 0.0
    for it, src in ((1, fx["opt"]), (5, fx["opt"]), (20, fx["opt20"])):
        for a, name in zip(run64["snap"][it], "wmv"):
            e = max(R.tensor_rel_errors(a, src[f"{name}_{it}"]).values())
            print(it, name, e)
            worst = max(worst, e)
    ref = fx["d"]["train_losses_f64"]
    lerr = float(np.max(np.abs(run64["losses"] - ref) / np.abs(ref)))
    print("losses", lerr)
    assert worst < 7.4e-12 and lerr < 3.3e-12


def test_fp32_mode_stays_inside_the_component_cap(fx, run64):
    """Adam divides by sqrt(v): components whose gradient is near zero are ill-conditioned.  The restatement's own fp32 mode after
    20 iterations must keep the share of components further than 1e-4 (absolute; a step is lr = 3e-3) from fp64 under 0.1 %.
    Measured: per-tensor at most 6.4e-5, largest component error 1.4e-5, share 0."""
    r32 = R.train(fx["sets"]["fresh"], fx["Z"], fx["Y"], fx["U"], fx["d"]["iters"], fp32=True)
    comp = np.abs(r32["w"].astype(np.float64) - run64["w"])
    share = float(np.mean(comp > 1e-4))
    print("per tensor", max(R.tensor_rel_errors(r32["w"], run64["w"]).values()), "max component", comp.max(), "share", share)
    assert share <= 1e-3


def test_fp32_mode_is_a_fair_yardstick_for_torch_fp32(fx, run64):
    """The GPU bounds are multiples of the restatement's fp32-mode error.  torch's own fp32 run of the same cases (loss terms of
    the six minibatches, loss terms and final weights of the 20 iterations) must land within the multi-step multiple, 8 x that
    error + 5e-6, of fp64: the yardstick is not an outlier of fp32 arithmetic."""
    d = fx["d"]
    for wset in ("ckpt", "fresh"):
        for b in BATCHES:
            idx = d["idx_" + b]
            a = (fx["sets"][wset], fx["Z"][idx], fx["Y"][idx], fx["U"][idx], min(10, len(idx) - 1))
            l64, l32 = R.loss_and_grad(*a)[0], R.loss_and_grad(*a, fp32=True)[0]
            t32 = d[f"loss_f32_{wset}_{b}"]
            assert np.all(np.abs(t32 - l64) / np.abs(l64) <= 8 * np.abs(l32 - l64) / np.abs(l64) + 5e-6), (wset, b)
    r32 = R.train(fx["sets"]["fresh"], fx["Z"], fx["Y"], fx["U"], d["iters"], fp32=True)
    e_t, e_r = R.tensor_rel_errors(fx["opt20"]["w_20_f32"], run64["w"]), R.tensor_rel_errors(r32["w"], run64["w"])
    print({k: (e_t[k], e_r[k]) for k in e_t})
    assert all(e_t[k] <= 8 * e_r[k] + 5e-6 for k in e_t), {k: (e_t[k], e_r[k]) for k in e_t if e_t[k] > 8 * e_r[k] + 5e-6}
    l = d["train_losses_f32"]
    assert np.all(np.abs(l - run64["losses"]) <= 8 * np.abs(r32["losses"] - run64["losses"]) + 5e-6 * np.abs(run64["losses"]))


def test_dataset_restatement_matches_reference(fx):
    """make_pinc_dataset on cfg5's train split: U4 and the vehicle's lag to 1e-12 (measured 3.6e-15 / 1.7e-16), z and y likewise."""
    c5 = np.load(os.path.join(GOLD, "cfg5.npz"))
    sp, d = int(c5["split"]), fx["d"]
    z, y, U4, lag = R.make_dataset(c5["X"][:sp], c5["U"][:sp], float(c5["dt"]))
    assert z.shape == d["z"].shape == (sp - 1, 14) and y.shape == (sp - 1, 9) and U4.shape == (sp, 4)
    assert z.dtype == y.dtype == U4.dtype == np.float64
    errs = [float(np.abs(a - b).max()) for a, b in ((U4, d["U4"]), (lag, d["lag_after"]), (z, d["z"]), (y, d["y"]))]
    print(errs)
    assert max(errs) < 1e-12


def test_init_has_torch_default_distributions():
    from bluerov2_dynamics_amd import pinc
    w = pinc.PINcWeights.init(7)
    assert w.blob.size == pinc.NPARAMS == 14541 and w.blob.dtype == np.float32
    assert w.blob.tobytes() == pinc.PINcWeights.init(7).blob.tobytes() and w.blob.tobytes() != pinc.PINcWeights.init(8).blob.tobytes()
    for k, a in w.arrays.items():
        assert a.size == int(np.prod(pinc.SHAPES[k])) and a.dtype == np.float32, k
        idx = int(k.split(".")[1])
        if idx in (0, 3, 6, 9, 12):
            bound = 1 / np.sqrt(14 if idx == 0 else 64)
            assert np.abs(a).max() <= bound and np.abs(a).max() > 0.8 * bound, k
            if a.size >= 576:
                assert abs(float(a.mean())) < 0.1 * bound and abs(float(a.std()) - bound / np.sqrt(3)) < 0.1 * bound, k
        elif k.endswith("beta"):
            assert a == 1
        else:
            assert np.all(a == (1 if k.endswith("weight") else 0)), k
    assert pinc.PINcWeights.from_blob(w.blob).blob.tobytes() == w.blob.tobytes()
    with pytest.raises(ValueError):
        pinc.PINcWeights.from_blob(np.zeros(10))


def test_train_pinc_checks_its_arguments_before_touching_a_device():
    from bluerov2_dynamics_amd import pinc
    z, y, u = np.zeros((5, 14)), np.zeros((5, 9)), np.zeros((6, 4))
    for bad in (dict(z_train=np.zeros((5, 13))), dict(y_train=np.zeros((4, 9))), dict(u4_train=np.zeros((5, 4))), dict(epochs=-1),
                dict(batch=0), dict(perms=np.zeros((2, 5), dtype=int))):
        kw = dict(z_train=z, y_train=y, u4_train=u, dt=0.1, epochs=1, verbose=False)
        kw.update(bad)
        with pytest.raises(ValueError):
            pinc.train_pinc(**kw)


def test_importing_the_training_api_does_not_import_torch():
    code = ("import sys; import bluerov2_dynamics_amd.pinc as p; p.PINcWeights.init(0); "
            "assert callable(p.train_pinc) and callable(p.make_pinc_dataset) and p.PINcTrainer; assert 'torch' not in sys.modules")
    subprocess.check_call([sys.executable, "-c", code], cwd=REPO)
