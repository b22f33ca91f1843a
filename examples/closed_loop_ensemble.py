#!/usr/bin/env python3
"""Does a depth-and-heading controller still work on the vehicles a fit cannot tell apart?

A step of +1 m in depth and +0.5 rad in heading under PID gains in wrench space, mapped to the eight thrusters
(fossen/control.py: pid_thrusters), first on the nominal vehicle (rov.simulate_closed_loop), then with the same controller on
--ensemble N vehicles in one launch (engine.rollout_feedback: the law is evaluated inside the rollout kernel).  The vehicles are
drawn with identify.sample_parameters from a fit to a recording when a CSV is given, and from a +-10 % box around the nominal
damping and added mass otherwise; engine.ensemble_stats reduces their final errors to a band.  Reads no file unless asked to.

    python examples/closed_loop_ensemble.py [--ensemble 256 --seconds 20 --hold 5 --rk4]
    python examples/closed_loop_ensemble.py path/to/koopman_dataset_50Hz.csv --ensemble 256
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bluerov2_dynamics_amd import engine                             # noqa: E402
from bluerov2_dynamics_amd.fossen import control, identify           # noqa: E402
from bluerov2_dynamics_amd.fossen.BlueROV2 import BlueROV2             # noqa: E402

BOX = ("Xu", "Yv", "Zw", "Nr", "Xu_abs", "Yv_abs", "Zw_abs", "Nr_abs", "Xu_dot", "Yv_dot", "Zw_dot", "Nr_dot")


def box_vehicles(base, n, rng, width=0.10):
    """n vehicles with the damping and added-mass terms of BOX each moved by up to +-width"""
    out = []
    for _ in range(n):
        p = identify.copy_params(base)
        for name in BOX:
            identify.set_param(p, name, identify.get_param(p, name) * (1.0 + rng.uniform(-width, width)))
        out.append(p)
    return out


def run(csv_path=None, ensemble=256, seconds=20.0, dt=0.02, hold=5, integrator="euler", seed=0, fit_iters=20, verbose=True):
    """Returns dict(traj, u, metrics of the nominal vehicle; settle [N,2] = |depth error|, |heading error| at the end per vehicle,
    band = ensemble_stats of settle, saturating = share of vehicles with a saturated step, metrics [N,4])."""
    rov = BlueROV2(dt=dt)
    vehicles = None
    if csv_path is not None:
        from bluerov2_dynamics_amd.data import load_dataset
        X, U, dt = load_dataset(csv_path, verbose=verbose, variant="thruster")
        rov = BlueROV2(dt=dt)
        fit = rov.fit_parameters(X, U, dt, H=10, integrator=integrator, iters=fit_iters, covariance=True)
        vehicles = identify.sample_parameters(fit, int(ensemble), seed=seed)
    T = int(round(seconds / dt))
    x0 = np.zeros(12)
    x0[2] = 5.0
    ref = x0.copy()
    ref[2], ref[5] = 6.0, 0.5
    fb = control.pid_thrusters(rov, [40.0, 40.0, 60.0, 4.0, 4.0, 6.0], [20.0, 20.0, 30.0, 1.0, 1.0, 2.0], [4.0, 4.0, 6.0, 0.4, 0.4, 0.6],
                               z_max=2.0, hold=hold)
    traj, u, metrics = rov.simulate_closed_loop(x0, ref, dt, fb, T=T, integrator=integrator)
    if vehicles is None:
        vehicles = box_vehicles(identify.params_of(rov), int(ensemble), np.random.default_rng(seed))
    r = engine.rollout_feedback(rov.MODEL, integrator, vehicles, fb, x0[None], ref[None, None], dt, T=T, store=False, ctx=rov._ctx)
    e = control.error_numpy(rov.MODEL, r["xT"][:, 0], ref)
    settle = np.abs(e[:, [2, 5]])
    band = engine.ensemble_stats(settle, ctx=rov._ctx)
    saturating = float((r["metrics"][:, 0, 3] > 0).mean())
    if verbose:
        en = control.error_numpy(rov.MODEL, traj[-1], ref)
        print(f"[nominal] {T} steps of {dt} s, hold {hold}: final depth error {en[2]:+.4f} m, heading error {en[5]:+.4f} rad, "
              f"{int(metrics[3])} saturated steps, sum dt |u|^2 = {metrics[2]:.3f}")
        src = "drawn around the fit" if csv_path else "from a +-10 % box around the nominal vehicle"
        print(f"[ensemble] {len(vehicles)} vehicles {src}, one launch:")
        for i, name in enumerate(("depth error [m]", "heading error [rad]")):
            print(f"  final |{name}|: mean {band['mean'][i]:.4g}, std {band['std'][i]:.4g}, band {band['min'][i]:.4g} .. {band['max'][i]:.4g}")
        print(f"  vehicles that saturate at some step: {100 * saturating:.0f} %")
    return dict(traj=traj, u=u, metrics_nominal=metrics, settle=settle, band=band, saturating=saturating, metrics=r["metrics"][:, 0])


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("csv", nargs="?", default=None)
    ap.add_argument("--ensemble", type=int, default=256)
    ap.add_argument("--seconds", type=float, default=20.0)
    ap.add_argument("--hold", type=int, default=5)
    ap.add_argument("--rk4", action="store_true")
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    run(a.csv, ensemble=a.ensemble, seconds=a.seconds, hold=a.hold, integrator="rk4" if a.rk4 else "euler", seed=a.seed)
