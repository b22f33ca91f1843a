#!/usr/bin/env python3
"""Do the gains still hold when the controller sees an estimate instead of the true state?

The step of examples/closed_loop_ensemble.py (+1 m in depth, +0.5 rad in heading, PID gains in wrench space mapped to the eight
thrusters), run twice on the same vehicles with the same gains:
  state feedback   engine.rollout_feedback: the law reads the TRUE state, which no real vehicle has;
  output feedback  engine.output_feedback: the unscented Kalman filter runs inside the rollout kernel on tank-odometry noise with a
                   depth channel that drops out and a linear velocity that is never measured, and the law reads its estimate.
One true vehicle (the nominal one) is controlled through --ensemble N filter models: the draws of identify.sample_parameters around a
fit when a CSV is given, a +-10 % box around the nominal damping and added mass otherwise.  So the spread over the ensemble is what
model error costs the estimator-plus-controller pair.  Each run is one launch.  Reads no file unless asked to.

    python examples/output_feedback_ensemble.py [--ensemble 256 --seconds 20 --hold 5 --rk4 --dropout 0.3]
    python examples/output_feedback_ensemble.py path/to/koopman_dataset_50Hz.csv --ensemble 256
    python examples/output_feedback_ensemble.py --small
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bluerov2_dynamics_amd import engine                             # noqa: E402
from bluerov2_dynamics_amd.fossen import control, estimate, identify  # noqa: E402
from bluerov2_dynamics_amd.fossen.BlueROV2 import BlueROV2             # noqa: E402

BOX = ("Xu", "Yv", "Zw", "Nr", "Xu_abs", "Yv_abs", "Zw_abs", "Nr_abs", "Xu_dot", "Yv_dot", "Zw_dot", "Nr_dot")
SIGMA = np.array([0.02] * 3 + [0.01] * 3 + [0.03] * 3 + [0.02] * 3)      # tank odometry: m, rad, m/s, rad/s
DEPTH, VELOCITY = 2, (6, 7, 8)


def box_vehicles(base, n, rng, width=0.10):
    """n vehicles with the damping and added-mass terms of BOX each moved by up to +-width"""
    out = []
    for _ in range(n):
        p = identify.copy_params(base)
        for name in BOX:
            identify.set_param(p, name, identify.get_param(p, name) * (1.0 + rng.uniform(-width, width)))
        out.append(p)
    return out


def run(csv_path=None, ensemble=256, seconds=20.0, dt=0.02, hold=5, integrator="euler", seed=0, fit_iters=20, dropout=0.3, small=False,
        verbose=True):
    """Returns dict(P, T, state_feedback = dict(metrics [P,4], settle [P,2]), output_feedback = dict(traj [P,T+1,12], y, x, u, metrics
    [P,7], settle [P,2], failed_step [P])); settle = |depth error|, |heading error| of the TRUE state at the end."""
    if small:
        ensemble, seconds = 4, 0.5
    rov = BlueROV2(dt=dt)
    models = None
    if csv_path is not None:
        from bluerov2_dynamics_amd.data import load_dataset
        X, U, dt = load_dataset(csv_path, verbose=verbose, variant="thruster")
        rov = BlueROV2(dt=dt)
        fit = rov.fit_parameters(X, U, dt, H=10, integrator=integrator, iters=fit_iters, covariance=True)
        models = identify.sample_parameters(fit, int(ensemble), seed=seed)
    if models is None:
        models = box_vehicles(identify.params_of(rov), int(ensemble), np.random.default_rng(seed))
    P, T = len(models), int(round(seconds / dt))
    x0 = np.zeros(12)
    x0[2] = 5.0
    ref = x0.copy()
    ref[2], ref[5] = 6.0, 0.5
    fb = control.pid_thrusters(rov, [40.0, 40.0, 60.0, 4.0, 4.0, 6.0], [20.0, 20.0, 30.0, 1.0, 1.0, 2.0], [4.0, 4.0, 6.0, 0.4, 0.4, 0.6],
                               z_max=2.0, hold=hold)
    plant = identify.params_of(rov)
    # the true state fed back: the plant alone matters, so one run stands for every model
    sf = engine.rollout_feedback(rov.MODEL, integrator, [plant], fb, x0[None], ref[None, None], dt, T=T, store=False, ctx=rov._ctx)
    settle_sf = np.abs(control.error_numpy(rov.MODEL, sf["xT"][:, 0], ref)[:, [2, 5]])
    # the estimate fed back: depth drops out, the linear velocity is never measured
    r = SIGMA ** 2
    r[list(VELOCITY)] = np.inf
    cfg = estimate.ukf(q=1e-6, r=r)
    V = estimate.measurement_noise(cfg, (T,), seed=seed)
    V[np.random.default_rng(seed + 1).random(T) < dropout, DEPTH] = np.nan
    P0 = np.diag(np.where(np.isfinite(r), 4.0 * SIGMA ** 2, estimate.P0_STAND_IN))
    of = engine.output_feedback(rov.MODEL, integrator, models, fb, cfg, x0[None], x0[None], P0[None], V[None], ref[None, None], dt,
                                plant_params=plant, ctx=rov._ctx)
    settle_of = np.abs(control.error_numpy(rov.MODEL, of["xT_true"][:, 0], ref)[:, [2, 5]])
    failed = of["info"][:, 0, 2].astype(np.int64)
    if verbose:
        m = of["metrics"][:, 0]
        print(f"{T} steps of {dt} s, hold {hold}, one true vehicle, {P} filter models; depth dropout {100 * dropout:.0f} %, u v w never measured")
        print(f"[state feedback ] final |depth error| {settle_sf[0, 0]:.4f} m, |heading error| {settle_sf[0, 1]:.4f} rad, "
              f"sum dt |e_pos|^2 = {sf['metrics'][0, 0, 0]:.4f}, {int(sf['metrics'][0, 0, 3])} saturated steps")
        print(f"[output feedback] final |depth error| {settle_of[:, 0].mean():.4f} m (worst {settle_of[:, 0].max():.4f}), |heading error| "
              f"{settle_of[:, 1].mean():.4f} rad (worst {settle_of[:, 1].max():.4f}), sum dt |e_pos|^2 = {m[:, 0].mean():.4f} (worst {m[:, 0].max():.4f})")
        print(f"  estimation error, sum dt |xf - x|^2: position {m[:, 4].mean():.3g}, attitude {m[:, 5].mean():.3g}, velocity {m[:, 6].mean():.3g}; "
              f"filters that failed: {int((failed >= 0).sum())} of {P}")
    return dict(P=P, T=T, state_feedback=dict(metrics=np.repeat(sf["metrics"][:, 0], P, axis=0), settle=np.repeat(settle_sf, P, axis=0)),
                output_feedback=dict(traj=of["traj"][:, 0], y=of["y"][:, 0], x=of["xf"][:, 0], u=of["u"][:, 0], metrics=of["metrics"][:, 0],
                                     settle=settle_of, failed_step=failed))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("csv", nargs="?", default=None)
    ap.add_argument("--ensemble", type=int, default=256)
    ap.add_argument("--seconds", type=float, default=20.0)
    ap.add_argument("--hold", type=int, default=5)
    ap.add_argument("--rk4", action="store_true")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--dropout", type=float, default=0.3)
    ap.add_argument("--small", action="store_true", help="4 models, half a second: what the tests run")
    a = ap.parse_args()
    run(a.csv, ensemble=a.ensemble, seconds=a.seconds, hold=a.hold, integrator="rk4" if a.rk4 else "euler", seed=a.seed, dropout=a.dropout,
        small=a.small)
