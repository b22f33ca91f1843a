"""Child process of tests/test_pinc_gpu.py::test_dropin_evaluator_without_torch: the drop-in PINc evaluator
(multistep_rmse_endpoint_pinc, H = 1, 10, 100 with one map vehicle) from the committed .npz weights in a process that never
imports torch; results to an .npz.

    python tests/pinc_worker.py <out.npz>"""
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
GOLDEN = os.path.join(REPO, "tests", "golden")


def main():
    os.environ["BROV2_TORCH"] = "0"
    from bluerov2_dynamics_amd.fossen.BlueROV2 import BlueROV2
    from bluerov2_dynamics_amd.pinc import PINcWeights, multistep_rmse_endpoint_pinc
    g = np.load(os.path.join(GOLDEN, "cfg5.npz"))
    X, U, dt, split = g["X"], g["U"], float(g["dt"]), int(g["split"])
    w = PINcWeights(os.path.join(GOLDEN, "pinc_weights.npz"))
    rov = BlueROV2(dt=dt)
    row = [multistep_rmse_endpoint_pinc(X[split:], U[split:], H, dt, w, rov) for H in (1, 10, 100)]
    assert "torch" not in sys.modules, "torch was imported"
    np.savez(sys.argv[1], row=np.array(row), lag=rov._lag.copy(), torch_loaded=np.array("torch" in sys.modules))


if __name__ == "__main__":
    main()
