"""rollout_pair_kernel on the paths a benchmark-like start hardly ever takes -- the cos(theta) clamp of each dynamics() call, the range
extension of trig_delta with one and with several halvings, NaN lanes, dead lanes of a partial wave -- at the smallest shapes that
reach them (rollout_rare_cases.py describes the start sets and why they look as they do).

Two references.  The C oracle, at the 1e-11 mixed error of the other rollout tests.  And the bits the build before the body wave's
hot-path copies were removed produced (tests/golden/rollout_pair_parent_bits.npz, tools/gen_rollout_rare_golden.py): those changes
reorder no floating-point operation, so every stored state must be the same double, NaNs canonicalised."""
import functools

import numpy as np
import pytest

import rollout_rare_cases as rc
from conftest import load_golden, rel_err

pytestmark = pytest.mark.gpu

TOL = 1e-11


@functools.lru_cache(maxsize=None)
def _inputs(name):
    x0, U, dt = rc.start_set(name)
    return x0, rc.layouts_of(U), dt


@functools.lru_cache(maxsize=None)
def _oracle(name, integ):
    from oracle import fossen_c as fc
    x0, Ul, dt = _inputs(name)
    o = fc.rollout(fc.MODEL_THRUSTER_EULER, fc.INTEG_RK4 if integ == "rk4" else fc.INTEG_EULER, x0, Ul["btu"], dt, sub=1, nthreads=4)
    live = np.arange(rc.B) != rc.NAN_LANE
    tr = o["traj"]
    assert np.isfinite(tr[live]).all() and np.isnan(tr[rc.NAN_LANE]).all()      # the reference itself is usable on this set
    if name in ("fast", "spin"):
        # the range extension is reached with one halving and with several: full-step angle increments in (1/8, 1/4] and above 1/4 rad
        inc = np.abs(np.diff(tr[live][:, :, 3:6], axis=1)).max(axis=2)
        assert ((inc > 0.125) & (inc <= 0.25)).sum() >= 5 and (inc > 0.25).sum() >= 5, (name, integ)
    if name == "clamp":
        # the clamped reciprocal shows in the result: roll and yaw of the lanes with an out-of-plane seed move -- by at least the seed
        # (>= 1e-12 rad/s, times q >= 0.5 for a roll seed) x 1e7 x the weight h / 6 of one RK4 call = 1.7e-8 rad; for Euler, whose only
        # call is the first, by 5e-9 x 1e7 x h = 1e-3 rad in the lanes aimed at that call -- and stay put in the in-plane lanes
        stage, kind = rc.clamp_kinds()
        seeded = live & ((kind == 1) | (kind == 2)) & ((stage == 0) | (integ == "rk4"))
        move = np.abs(tr[:, :, [3, 5]] - x0[:, None, [3, 5]]).max(axis=1)
        assert (move[seeded] > (1e-8 if integ == "rk4" else 5e-4)).all(), (integ, move[seeded].min())
        assert (move[live & (kind == 0)][:, 0] == 0).all()
    return o


@functools.lru_cache(maxsize=None)
def _gold():
    return load_golden("rollout_pair_parent_bits.npz")


@pytest.mark.parametrize("stride", [1, 3])
@pytest.mark.parametrize("lay", ["tpb", "tub", "btu"])
@pytest.mark.parametrize("integ", ["rk4", "euler"])
@pytest.mark.parametrize("name", rc.SETS)
def test_rare_paths_against_the_oracle_and_the_parent_bits(name, integ, lay, stride):
    from bluerov2_dynamics_amd import _lib, engine
    x0, Ul, dt = _inputs(name)
    o = _oracle(name, integ)
    r = engine.rollout(_lib.THRUSTER_EULER, integ, x0, Ul[lay], dt, layout=lay, stride=stride, return_lag=False)
    traj, xT = rc.to_btx(r["traj"], lay, rc.B), r["xT"]
    want = o["traj"][:, ::stride]
    assert traj.shape == want.shape == (rc.B, rc.T // stride + 1, 12)
    live = np.arange(rc.B) != rc.NAN_LANE
    # the NaN lane stays NaN in every component from the first step on, and its neighbours are finite
    assert np.isnan(traj[rc.NAN_LANE]).all() and np.isnan(xT[rc.NAN_LANE]).all()
    assert np.isfinite(traj[live]).all() and np.isfinite(xT[live]).all()
    e_traj, e_xT = rel_err(traj[live], want[live]), rel_err(xT[live], o["xT"][live])
    print(f"{name} {integ} {lay} stride {stride}: mixed error vs oracle traj {e_traj:.3e} xT {e_xT:.3e}")
    assert e_traj < TOL and e_xT < TOL
    # bit equality with the recorded build
    g = _gold()
    sha = g[f"{name}_{integ}_{lay}_sha"]
    lanes = traj[list(rc.GOLD_LANES)] if stride == 3 else traj[list(rc.GOLD_LANES), ::3]
    assert rc.bits_equal(xT, g[f"{name}_{integ}_xT"])
    assert rc.bits_equal(lanes, g[f"{name}_{integ}_lanes"])
    assert np.array_equal(rc.digest(xT), sha[0]) and np.array_equal(rc.digest(traj), sha[1 if stride == 1 else 2])
