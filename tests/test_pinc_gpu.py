"""PINc network inference on the MI355X (csrc/pinc.hip through bluerov2_dynamics_amd/pinc.py) against the reference's own outputs
(tests/golden/pinc_kat.npz, cfg5_pinc.npz; tools/gen_golden.py: gen_pinc): forward, simulate_pinc, the windowed evaluator with
its lag carried across windows and calls, batch independence, the four-row comparison script, and a torch-free process."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, REPO, load_golden, rel_err

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def weights():
    from bluerov2_dynamics_amd.pinc import PINcWeights
    return PINcWeights(os.path.join(GOLDEN, "pinc_weights.npz"))


@pytest.fixture(scope="module")
def cfg5():
    g = load_golden("cfg5.npz")
    return g["X"], g["U"], float(g["dt"]), int(g["split"])


def test_forward_matches_reference(weights):
    from bluerov2_dynamics_amd.pinc import PINc
    kat = load_golden("pinc_kat.npz")
    y = PINc(weights).forward(kat["z"])
    assert y.dtype == np.float32 and y.shape == kat["x_next"].shape
    assert rel_err(y, kat["x_next"]) < 1e-5
    n = len(kat["z"]) - 333                 # the scaled rows (softplus past its threshold 20) alone
    assert rel_err(y[n:], kat["x_next"][n:]) < 1e-5


def test_simulate_pinc_500_steps_and_vehicle_lag(weights, cfg5):
    from bluerov2_dynamics_amd.fossen.BlueROV2 import BlueROV2
    from bluerov2_dynamics_amd.pinc import simulate_pinc
    X, U, dt, _ = cfg5
    kat = load_golden("pinc_kat.npz")
    k = int(kat["start500"])
    rov = BlueROV2(dt=dt)
    traj = simulate_pinc(X[k], U[k:k + 500], dt, weights, rov, device="cuda")
    assert traj.shape == (501, 12) and np.array_equal(traj[0], X[k])
    assert rel_err(traj, kat["traj500"]) < 2e-5
    assert rel_err(rov._lag, kat["lag500"]) < 1e-12


def test_dropin_evaluator_sequence_h1_h10_h100(weights, cfg5):
    from bluerov2_dynamics_amd.fossen.BlueROV2 import BlueROV2
    from bluerov2_dynamics_amd.pinc import multistep_rmse_endpoint_pinc
    X, U, dt, split = cfg5
    ref = load_golden("cfg5_pinc.npz")["pinc_row"]
    kat = load_golden("pinc_kat.npz")
    rov = BlueROV2(dt=dt)
    row = [multistep_rmse_endpoint_pinc(X[split:], U[split:], H, dt, weights, rov) for H in (1, 10, 100)]
    assert np.max(np.abs(np.array(row) - ref) / np.abs(ref)) < 1e-5, (row, ref)
    assert rel_err(rov._lag, kat["lag_after_seq"]) < 1e-9
    # n_start <= 0: NaN and the vehicle is not touched
    lag = rov._lag.copy()
    assert np.isnan(multistep_rmse_endpoint_pinc(X[:5], U[:5], 5, dt, weights, rov))
    assert np.array_equal(rov._lag, lag)


def test_per_window_endpoints_h10(weights, cfg5):
    from bluerov2_dynamics_amd.pinc import PINc
    X, U, dt, split = cfg5
    kat = load_golden("pinc_kat.npz")
    Xte, Ute = X[split:], U[split:]
    r = PINc(weights).window_endpoint_se(Xte, Ute, 10, dt, lag=kat["lag_before_H10"])
    ends = kat["endpoints_H10"]
    assert len(r["per_window"]) == len(ends) == 390
    se_ref = np.sum((ends - Xte[10:]) ** 2, axis=1)
    assert np.max(np.abs(r["per_window"] - se_ref) / np.maximum(se_ref, 1e-12)) < 1e-4
    assert abs(r["se"] - se_ref.sum()) / se_ref.sum() < 1e-5
    assert rel_err(r["lag"], kat["lag_before_H100"]) < 1e-9


def test_carried_lag_from_nonzero_start_equals_sequential_map(weights, cfg5):
    from bluerov2_dynamics_amd import engine
    from bluerov2_dynamics_amd.pinc import PINc
    X, U, dt, _ = cfg5
    H = 10
    s0 = load_golden("pinc_kat.npz")["lag500"]
    assert np.abs(s0).max() > 0
    r = PINc(weights).window_endpoint_se(X, U, H, dt, lag=s0, want_lag_starts=True)
    nwin = len(X) - H
    assert r["lag_starts"].shape == (nwin, 8, 3) and nwin == 1990
    seq = np.empty((nwin, 8, 3))
    lag = s0.copy()
    for k in range(nwin):
        seq[k] = lag
        for t in range(H):
            _, lag = engine.thruster_forces(U[k + t], dt, lag=lag)
            lag = lag[0]
    assert rel_err(r["lag_starts"], seq) < 1e-12
    assert rel_err(r["lag"], lag) < 1e-12
    # carry_lag=False: every window from the given lag, which stays as it was
    r0 = PINc(weights).window_endpoint_se(X[:300], U[:300], H, dt, lag=s0, carry_lag=False)
    assert np.array_equal(r0["lag"], s0)
    one = PINc(weights).rollout(X[7][None], U[7:7 + H][None], dt, lag=s0[None])
    e = np.sum((one["xT"][0] - X[7 + H]) ** 2)
    assert abs(r0["per_window"][7] - e) <= 1e-12 * e


def test_batch_rollout_is_bitwise_independent_of_the_batch(weights, cfg5):
    from bluerov2_dynamics_amd.pinc import PINc
    X, U, dt, _ = cfg5
    rng = np.random.default_rng(7)
    B, T = 1000, 60
    x0 = X[rng.integers(0, len(X), B)]
    Ub = rng.uniform(-1, 1, (B, T, 8))
    lag0 = rng.normal(0, 0.5, (B, 8, 3))
    net = PINc(weights)
    r = net.rollout(x0, Ub, dt, lag=lag0, stride=3)
    assert r["traj"].shape == (B, T // 3 + 1, 12)
    for b in (0, 1, 517, 999):
        a = net.rollout(x0[b:b + 1], Ub[b:b + 1], dt, lag=lag0[b:b + 1], stride=3)
        assert np.array_equal(a["traj"][0], r["traj"][b]) and np.array_equal(a["xT"][0], r["xT"][b])
        assert np.array_equal(a["lag"][0], r["lag"][b])
    assert np.array_equal(r["traj"][:, -1], r["xT"])          # T = 60 is a multiple of the stride


def test_full_comparison_four_rows_on_the_engine(weights):
    import importlib.util
    spec = importlib.util.spec_from_file_location("full_comparison", os.path.join(REPO, "examples", "full_comparison.py"))
    fcmp = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(fcmp)
    g = load_golden("cfg5.npz")
    gp = load_golden("cfg5_pinc.npz")
    csv = os.path.join(GOLDEN, "cfg5_dataset.csv.gz")
    r = fcmp.compare(csv, n_rbfs=int(g["k"]), gamma=float(g["gamma"]), ridge=float(g["ridge"]), centers=g["centers"], verbose=False,
                     pinc=weights)
    ref4 = np.vstack([g["table"], gp["pinc_row"]])
    assert r["table"].shape == (4, 3) and r["rows"][3].startswith("PINc")
    assert np.max(np.abs(r["table"][3] - gp["pinc_row"])) < 1e-5
    assert np.array_equal(np.argsort(r["table"], axis=0), np.argsort(ref4, axis=0))
    assert np.array_equal(r["ranking"][3], [3, 3, 3])


def test_dropin_evaluator_without_torch(tmp_path):
    out = tmp_path / "pinc.npz"
    env = dict(os.environ, BROV2_TORCH="0")
    p = subprocess.run([sys.executable, os.path.join(REPO, "tests", "pinc_worker.py"), str(out)], capture_output=True, text=True,
                       timeout=600, env=env)
    assert p.returncode == 0, p.stderr[-3000:]
    d = np.load(out)
    assert not bool(d["torch_loaded"])
    ref = load_golden("cfg5_pinc.npz")["pinc_row"]
    assert np.max(np.abs(d["row"] - ref) / np.abs(ref)) < 1e-5
    assert rel_err(d["lag"], load_golden("pinc_kat.npz")["lag_after_seq"]) < 1e-9
