#!/usr/bin/env python3
"""Model-predictive tracking under model mismatch: the nominal vehicle plans, other vehicles are steered.

A smooth move of +1 m in depth and +0.5 rad in heading.  The planner is the sampling-based model-predictive update
(rov.simulate_mppi: K perturbed command sequences per tick, rolled out and scored on the device with the NOMINAL vehicle's model);
the plants are --plants N vehicles drawn with identify.sample_parameters around the nominal one (5 % standard deviation on the
damping and added-mass terms), or, with --current, the nominal vehicle in N different currents.  The same scenario is run under the
PID law of examples/closed_loop_ensemble.py (engine.rollout_feedback), and the four closed-loop metrics of brov_rollout_feedback --
sum dt |e_pos|^2, sum dt |e_att|^2, sum dt |u|^2, steps with a channel on a limit -- are printed side by side, averaged over the plants.

--planner koopman plans with a learned model instead: a Koopman EDMDc model (KoopmanEDMDc.fit_multi) fitted here on a short simulated
recording of the NOMINAL vehicle (on-device AR(1) commands, as examples/sim_koopman.py makes them) and handed to the same update
through model.mppi_planner (engine.koopman_mppi_step: the learned model is linear in the command, so a sample costs a block
convolution, not a rollout).  The plants, the seeds and the cost stay the same; the learned model never sees the thruster lag.
--planner koopman-qp plans with the same learned model but without samples: the model is linear in the command, so with a linear
error the tracking problem of a tick is a box-constrained QP in the knots, solved on the device by ADMM (model.lmpc_planner,
rov.simulate_lmpc: engine.koopman_lmpc_step) -- same weights, limits, horizon and plants.
--planner both (or all) prints a column per planner: Fossen-MPPI, Koopman-MPPI and Koopman-QP ranked by the same realised metrics.

    python examples/mppi_tracking.py [--plants 16 --seconds 6 --samples 1024 --horizon 25 --hold 5 --current 0.2 --planner both]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bluerov2_dynamics_amd import _lib, engine                       # noqa: E402
from bluerov2_dynamics_amd.Koopman.koopmanEDMDc import KoopmanEDMDc   # noqa: E402
from bluerov2_dynamics_amd.fossen import control, identify           # noqa: E402
from bluerov2_dynamics_amd.fossen.BlueROV2 import BlueROV2             # noqa: E402

SPREAD = ("Xu", "Yv", "Zw", "Nr", "Xu_abs", "Yv_abs", "Zw_abs", "Nr_abs", "Xu_dot", "Yv_dot", "Zw_dot", "Nr_dot")
NAMES = ("sum dt |e_pos|^2", "sum dt |e_att|^2", "sum dt |u|^2", "steps on a limit")
LABEL = {"mppi": "fossen", "koopman": "koopman", "koopman_qp": "koopman-qp"}
HEAD = {"mppi": "MPPI fossen", "koopman": "MPPI koopman", "koopman_qp": "QP koopman"}


def drawn_plants(base, n, seed, rel_std=0.05):
    """n vehicles around `base` through identify.sample_parameters: a stand-in fit whose covariance is diagonal, rel_std per term"""
    theta = {k: identify.get_param(base, k) for k in SPREAD}
    cov = np.diag([(rel_std * v) ** 2 for v in theta.values()])
    fit = identify.FitResult(params=theta, rmse_history=[], accepted=[], n_evals=0, brov_params=base, covariance=cov)
    return identify.sample_parameters(fit, n, seed=seed)


def current_plants(base, n, speed, rng):
    out = []
    for _ in range(n):
        p = identify.copy_params(base)
        d = rng.normal(size=3) * np.array([1.0, 1.0, 0.3])
        d *= speed / np.linalg.norm(d)
        for i in range(3):
            p.current[i] = d[i]
        out.append(p)
    return out


def metrics_of(model, traj, u, ref, dt, lo, hi):
    """the four metrics of brov_rollout_feedback from a trajectory [B,T+1,nx], its commands [B,T,nu] and the reference rows [B,T,nx]"""
    e = control.error_numpy(model, traj[:, :-1], ref)
    on = np.any((u <= lo) | (u >= hi), axis=2)
    return np.stack([dt * np.sum(e[..., 0:3] ** 2, axis=(1, 2)), dt * np.sum(e[..., 3:6] ** 2, axis=(1, 2)), dt * np.sum(u ** 2, axis=(1, 2)),
                     on.sum(axis=1).astype(float)], axis=1)


def fit_koopman(rov, x0, dt, rollouts=64, steps=300, n_rbfs=64, gamma=1.0, ridge=1e-3, seed=0xED3D):
    """A KoopmanEDMDc model of the nominal vehicle at step dt: `rollouts` recordings of `steps` steps under AR(1) commands, simulated on
    the device from starts spread around x0 (depth and heading over the range of the move), fitted with fit_multi"""
    ctx = rov._ctx
    ctx.use_null_stream()
    rng = np.random.default_rng(seed)
    starts = np.repeat(x0[None], rollouts, axis=0)
    starts[:, 2] += rng.uniform(-0.5, 1.5, rollouts)
    starts[:, 5] += rng.uniform(-0.3, 0.8, rollouts)
    U = engine.DevArray(ctx, (rollouts, steps, 8))
    engine.fill_controls_dev(U, "btu", "ar1", seed=seed, ctx=ctx)
    X = engine.DevArray(ctx, (rollouts, steps + 1, 12))
    engine.rollout_dev(_lib.THRUSTER_EULER, "euler", engine.DevArray.from_host(ctx, starts), U, dt, traj=X, layout="btu", ctx=ctx)
    Xh, Uh = X.numpy(), U.numpy()
    model = KoopmanEDMDc(state_dim=12, input_dim=8, n_rbfs=n_rbfs, gamma=gamma, ridge=ridge)
    model.fit_multi([Xh[b] for b in range(rollouts)], [np.vstack([Uh[b], np.zeros((1, 8))]) for b in range(rollouts)])
    return model


def run(plants=16, seconds=6.0, dt=0.02, samples=1024, horizon=25, hold=5, current=0.0, integrator="rk4", seed=0, verbose=True,
        planner="fossen", fit_rollouts=64, fit_steps=300, n_rbfs=64, qp_iters=200):
    """Returns dict(mppi [N,4] (planner fossen / both), koopman [N,4] (planner koopman / both), koopman_qp [N,4] (planner koopman-qp /
    both), pid [N,4]): the closed-loop metrics of every plant under the controllers ("all" is "both")"""
    rov = BlueROV2(dt=dt)
    base = identify.params_of(rov)
    n = int(plants)
    ps = current_plants(base, n, float(current), np.random.default_rng(seed)) if current > 0 else drawn_plants(base, n, seed)
    T = int(round(seconds / dt)) // hold * hold
    x0 = np.zeros(12)
    x0[2] = 5.0
    rows = T + horizon + 1
    s = np.clip(np.arange(rows) * dt / 3.0, 0.0, 1.0)
    s = s * s * (3.0 - 2.0 * s)                                        # a smooth ramp over three seconds, then hold
    ref = np.tile(x0, (rows, 1))
    ref[:, 2], ref[:, 5] = 5.0 + s, 0.5 * s
    ref[:-1, 8], ref[:-1, 11] = np.diff(ref[:, 2]) / dt, np.diff(ref[:, 5]) / dt
    REF = np.repeat(ref[None], n, axis=0)
    cfg = control.mppi(q=[40.0, 40.0, 60.0, 4.0, 4.0, 6.0, 2.0, 2.0, 3.0, 0.2, 0.2, 0.4], qf=[80.0, 80.0, 120.0, 8.0, 8.0, 12.0, 4.0, 4.0, 6.0, 0.4, 0.4, 0.8],
                       r=0.05, sigma=0.15, lam=0.2, u_min=-1.0, u_max=1.0, hold=hold, nu=8)
    out, info, model = {}, {}, None
    for key, label in LABEL.items():
        if planner not in (label, "both", "all"):
            continue
        if label != "fossen" and model is None:
            model = fit_koopman(rov, x0, dt, fit_rollouts, fit_steps, n_rbfs)
        X0 = np.repeat(x0[None], n, axis=0)
        if label == "koopman-qp":
            qp = control.lmpc(q=list(cfg.q), qf=list(cfg.qf), r=0.05, u_min=-1.0, u_max=1.0, hold=hold, iters=int(qp_iters), nu=8)
            r = rov.simulate_lmpc(X0, REF, dt, model.lmpc_planner(int(horizon), qp, dt, ctx=rov._ctx), T, plant_params=ps, integrator=integrator)
        else:
            kp = model.mppi_planner(int(horizon), hold, ctx=rov._ctx) if label == "koopman" else None
            r = rov.simulate_mppi(X0, REF, dt, cfg, T, int(samples), int(horizon), plant_params=ps, integrator=integrator, seed=seed, planner=kp)
        out[key] = metrics_of(rov.MODEL, r["traj"], r["u"], REF[:, :T], dt, -1.0, 1.0)
        info[key] = r["info"]
    fb = control.pid_thrusters(rov, [40.0, 40.0, 60.0, 4.0, 4.0, 6.0], [20.0, 20.0, 30.0, 1.0, 1.0, 2.0], [4.0, 4.0, 6.0, 0.4, 0.4, 0.6],
                               z_max=2.0, hold=hold)
    p = engine.rollout_feedback(rov.MODEL, integrator, ps, fb, x0[None], ref[None, :T], dt, store=False, ctx=rov._ctx)
    out["pid"] = p["metrics"][:, 0]
    if verbose:
        what = f"in currents of {current} m/s" if current > 0 else "drawn around the nominal vehicle"
        for key, i in info.items():
            if key == "koopman_qp":
                print(f"{n} plants {what}, {T} steps of {dt} s, hold {hold}; QP (koopman model): {qp_iters} ADMM iterations over {horizon} steps "
                      f"per tick, last residuals {i[:, :, 2].max():.1e} / {i[:, :, 3].max():.1e}, {i[:, :, 5].mean():.1f} knot entries at a limit")
                continue
            print(f"{n} plants {what}, {T} steps of {dt} s, hold {hold}; MPPI{'' if planner == 'fossen' else ' (' + LABEL[key] + ' model)'}: "
                  f"{samples} samples over {horizon} steps per tick, effective sample size {i[:, :, 2].mean():.1f}, "
                  f"{int(i[:, :, 3].sum())} non-finite samples")
        cols = [(k, "MPPI" if planner == "fossen" else HEAD[k]) for k in info] + [("pid", "PID")]
        print(f"{'mean over the plants':<22}" + "".join(f"{label:>14}" for _, label in cols))
        for i, name in enumerate(NAMES):
            print(f"{name:<22}" + "".join(f"{out[k][:, i].mean():>14.5g}" for k, _ in cols))
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--plants", type=int, default=16)
    ap.add_argument("--seconds", type=float, default=6.0)
    ap.add_argument("--samples", type=int, default=1024)
    ap.add_argument("--horizon", type=int, default=25)
    ap.add_argument("--hold", type=int, default=5)
    ap.add_argument("--current", type=float, default=0.0)
    ap.add_argument("--euler", action="store_true")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--planner", choices=["fossen", "koopman", "koopman-qp", "both", "all"], default="fossen")
    ap.add_argument("--qp-iters", type=int, default=200, help="koopman-qp: ADMM iterations per tick")
    ap.add_argument("--fit-rollouts", type=int, default=64, help="koopman: simulated recordings of the nominal vehicle")
    ap.add_argument("--fit-steps", type=int, default=300, help="koopman: steps per recording")
    ap.add_argument("--rbfs", type=int, default=64, help="koopman: RBF centres")
    a = ap.parse_args(argv)
    out = run(a.plants, a.seconds, samples=a.samples, horizon=a.horizon, hold=a.hold, current=a.current,
              integrator="euler" if a.euler else "rk4", seed=a.seed, planner=a.planner, fit_rollouts=a.fit_rollouts, fit_steps=a.fit_steps,
              n_rbfs=a.rbfs, qp_iters=a.qp_iters)
    return {k: v.mean(axis=0) for k, v in out.items()}


if __name__ == "__main__":
    main()
