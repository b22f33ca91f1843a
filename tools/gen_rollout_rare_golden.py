#!/usr/bin/env python3
"""Record what the loaded libbrov2.so computes for the start sets of tests/rollout_rare_cases.py (on the GPU box):

    BROV2_LIBRARY=<the build to record> python tools/gen_rollout_rare_golden.py tests/golden/rollout_pair_parent_bits.npz

tests/golden/rollout_pair_parent_bits.npz was recorded with the build of the commit BEFORE the body wave of rollout_pair_kernel lost its
copies (carry, clamp, trig_delta: changes that reorder no floating-point operation), and tests/test_rollout_rare_paths.py holds every
later build to those bits.  Per start set and integrator: the end states of all 70 lanes, every third stored state of four lanes, and
a SHA-256 of the whole canonicalised output (end states, stride 1, stride 3) per layout.  The three layouts must agree bit for bit
(one step function); the script refuses to write a file otherwise."""
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))


def main(out):
    import rollout_rare_cases as rc
    from bluerov2_dynamics_amd import _lib, engine
    gold = {}
    for name in rc.SETS:
        x0, U, dt = rc.start_set(name)
        Ul = rc.layouts_of(U)
        for integ in ("euler", "rk4"):
            ref = None
            for lay in ("tpb", "tub", "btu"):
                r1 = engine.rollout(_lib.THRUSTER_EULER, integ, x0, Ul[lay], dt, layout=lay, stride=1, return_lag=False)
                r3 = engine.rollout(_lib.THRUSTER_EULER, integ, x0, Ul[lay], dt, layout=lay, stride=3, return_lag=False)
                t1, t3 = rc.to_btx(r1["traj"], lay, rc.B), rc.to_btx(r3["traj"], lay, rc.B)
                assert rc.bits_equal(t1[:, ::3], t3) and rc.bits_equal(r1["xT"], r3["xT"]) and rc.bits_equal(t1[:, -1], r1["xT"]), (name, integ, lay)
                if ref is None:
                    ref = (t1, r1["xT"])
                assert rc.bits_equal(t1, ref[0]) and rc.bits_equal(r1["xT"], ref[1]), ("layouts differ", name, integ, lay)
                gold[f"{name}_{integ}_{lay}_sha"] = np.stack([rc.digest(r1["xT"]), rc.digest(t1), rc.digest(t3)])
            gold[f"{name}_{integ}_xT"] = rc.canon(ref[1])
            gold[f"{name}_{integ}_lanes"] = rc.canon(ref[0][list(rc.GOLD_LANES), ::3])
            live = np.arange(rc.B) != rc.NAN_LANE
            print(name, integ, "finite live lanes:", bool(np.isfinite(ref[0][live]).all()), "NaN lane all NaN:", bool(np.isnan(ref[0][rc.NAN_LANE]).all()), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    np.savez_compressed(out, **gold)
    print("wrote", out, os.path.getsize(out), "bytes", "with", _lib.library_path(), flush=True)


if __name__ == "__main__":
    main(sys.argv[1])
