#!/usr/bin/env python3
"""The reference's 4-model comparison (training/train_tank_brov2_full_comparison.py: main :894-1048) on the MI355X
engine: Koopman EDMDc, Fossen (BlueROV2), the learned double integrator and, given the PINc checkpoint (--pinc-ckpt: the
reference's models/pinc_best.pt or a .npz of its arrays), the PINc residual network's row (bluerov2_dynamics_amd.pinc: one
thruster-map vehicle for H = 1, 10, 100, as the script's rov_old).  Without a checkpoint the PINc row's three RMSEs can still be
trained here with --pinc-train EPOCHS (train_pinc on the train split), or handed in with --pinc-row to complete the table and the ranking (tests/golden/cfg5_pinc.npz holds them for the CSV fixture).

    python examples/full_comparison.py path/to/koopman_dataset_50Hz.csv [--rbfs 500 --gamma 3 --ridge 0.1 --rk4]
    python examples/full_comparison.py path/to/koopman_dataset_50Hz.csv --pinc-ckpt models/pinc_best.pt
    python examples/full_comparison.py path/to/koopman_dataset_50Hz_with_wrench.csv --variant wrench   # train_tank_brov2_wrench_comp.py
    python examples/full_comparison.py path/to/koopman_dataset_50Hz_with_wrench.csv --variant quat     # train_tank_brov2_wrench_quat.py

Same data handling (load_dataset, 80/20 split), same metrics (endpoint RMSE at H = 1/10/100 over all sliding
windows, one vehicle object for all windows => thruster lag carried across windows), same table layout.
"""
import argparse
import os
import sys
from time import perf_counter

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bluerov2_dynamics_amd import engine                             # noqa: E402
from bluerov2_dynamics_amd.baselines import DoubleIntegrator          # noqa: E402
from bluerov2_dynamics_amd.data import load_dataset                   # noqa: E402
from bluerov2_dynamics_amd.fossen import identify                    # noqa: E402
from bluerov2_dynamics_amd.fossen.BlueROV2 import BlueROV2             # noqa: E402
from bluerov2_dynamics_amd.fossen.BlueROV2_thrust import BlueROV2 as BlueROV2Wrench          # noqa: E402
from bluerov2_dynamics_amd.fossen.BlueROV2_wrench import BlueROV2 as BlueROV2Quat            # noqa: E402
from bluerov2_dynamics_amd.Koopman.koopmanEDMDc import KoopmanEDMDc    # noqa: E402
from bluerov2_dynamics_amd.pinc import PINcWeights, make_pinc_dataset, multistep_rmse_endpoint_pinc, train_pinc      # noqa: E402

TRAIN_SPLIT = 0.80


ROWS = ("Koopman", "Fossen (BlueROV2)", "Double Integrator", "PINc (ResDNN)")


def compare(csv_path, n_rbfs=500, gamma=3.0, ridge=1e-1, integrator="euler", centers=None, verbose=True, variant="thruster", pinc_row=None,
            pinc=None, pinc_train=None, pinc_seed=0, fit_fossen=False, fit_iters=20, fit_fossen_bags=None, ensemble=0):
    """Returns dict(table [3,3] rows Koopman / Fossen / DI x H = 1, 10, 100, timings, dt, split); with pinc (the PINc network's
    weights: a PINcWeights, a .npz / .pt path, a state dict or the reference's PINcNet; thruster variant only) or pinc_row (its
    three RMSEs, computed elsewhere) or pinc_train (epochs: the network is trained on the train split with train_pinc, seed
    pinc_seed, and returned as `pinc_weights`) the table has the reference's four rows and `ranking` [4,3] gives each model's rank per
    horizon (0 = best), training/train_tank_brov2_full_comparison.py:996-1001.
    variant: "thruster" (8 PWM inputs, Euler angles), "wrench" (6-D body wrench, Euler angles), "quat" (wrench, quaternion
    state; RK4 exists only for the thruster script in the reference).
    fit_fossen: also fit the Fossen model's damping to the train split (fossen/identify.py, H = 10, at most fit_iters iterations) and
    score the fitted vehicle on the test split: `fossen_fitted` [3] and `fossen_fit` (the FitResult); printed as one more line under
    the table, which -- like `table` and `ranking` -- is otherwise unchanged.
    fit_fossen_bags: CSV paths of several recordings (free decay on each axis, a driven run, ...) to fit the damping on INSTEAD of
    the train split, each file one bag (fossen/identify.py: fit_parameters_multi): no window crosses from one file into the next and
    every file starts from zero thruster lag.  Scored and reported like fit_fossen.
    ensemble: N > 0 together with a fit: the fit also estimates its covariance, N vehicles are drawn from it
    (identify.sample_parameters) and rolled open loop over the first 500 steps of the test split together with the fitted and the
    nominal vehicle, all in one engine.rollout_pop call; engine.ensemble_stats reduces the draws to a band.  `ensemble` in the
    result: dict(band_width [nx] = mean of max - min over the steps, inside [nx] = share of the recorded samples inside the band,
    traj_fitted, traj_nominal, stats); printed per state under the fit line.  Without a fit, or with N = 0, nothing changes."""
    if sum(v is not None for v in (pinc, pinc_row, pinc_train)) > 1:
        raise ValueError("give the PINc network (pinc), its precomputed row (pinc_row) or the epochs to train it for (pinc_train), "
                         "not more than one")
    if (pinc is not None or pinc_train is not None) and variant != "thruster":
        raise ValueError("the PINc network takes the thruster commands: variant must be 'thruster'")
    if pinc is not None:
        pinc = PINcWeights(pinc)               # before the first device context (a .pt checkpoint imports torch)
    X, U, dt = load_dataset(csv_path, verbose=verbose, variant=variant)
    nx, nu = X.shape[1], U.shape[1]
    make_rov = {"thruster": lambda: BlueROV2(dt=dt), "wrench": BlueROV2Wrench, "quat": BlueROV2Quat}[variant]
    if len(X) < 3:
        raise RuntimeError("Not enough samples to train/evaluate.")
    split = int(TRAIN_SPLIT * len(X))
    Xtr, Utr, Xte, Ute = X[:split], U[:split], X[split:], U[split:]
    t = {}
    t0 = perf_counter()
    koop = KoopmanEDMDc(state_dim=nx, input_dim=nu, n_rbfs=n_rbfs, gamma=gamma, ridge=ridge)
    koop.fit(Xtr, Utr, centers=centers)
    t["fit_koopman"] = perf_counter() - t0
    t0 = perf_counter()
    di = DoubleIntegrator.fit(Xtr, Utr, dt, ridge=1e-3, quaternion=(variant == "quat"))
    t["fit_di"] = perf_counter() - t0
    if pinc_train is not None:
        t0 = perf_counter()
        rov_old = BlueROV2(dt=dt)              # the script's one map vehicle: the dataset advances its lag by the train split (:947-960)
        z_tr, y_tr, u4_tr = make_pinc_dataset(Xtr, Utr, dt, rov_old)
        pinc = train_pinc(z_tr, y_tr, u4_tr, dt, epochs=int(pinc_train), seed=pinc_seed, verbose=verbose)
        t["train_pinc"] = perf_counter() - t0
    rows = []
    for name, fn in (("Koopman", lambda H: koop.multistep_rmse(Xte, Ute, H=H)),
                     ("Fossen (BlueROV2)", lambda H: make_rov().multistep_rmse_endpoint(Xte, Ute, H, dt, integrator)),
                     ("Double Integrator", lambda H: di.multistep_rmse_endpoint(Xte, Ute, H, dt, integrator))):
        vals = []
        for H in (1, 10, 100):
            t0 = perf_counter()
            vals.append(fn(H))
            t[f"{name}_H{H}"] = perf_counter() - t0
        rows.append(vals)
    if pinc is not None:
        if pinc_train is None:
            rov_old = BlueROV2(dt=dt)          # the script's thruster-map vehicle: its lag carries across H = 1, 10, 100 (:947, :992-994)
        vals = []
        for H in (1, 10, 100):
            t0 = perf_counter()
            vals.append(multistep_rmse_endpoint_pinc(Xte, Ute, H, dt, pinc, rov_old))
            t[f"PINc_H{H}"] = perf_counter() - t0
        rows.append(vals)
    elif pinc_row is not None:
        rows.append([float(v) for v in pinc_row])
    table = np.array(rows)
    fitted_row = fit = None
    fit_on = "train-split"
    cov_kw = dict(covariance=True) if ensemble else {}     # one more population call at the fitted point, only when asked for
    if fit_fossen_bags:
        bags = [load_dataset(path, verbose=verbose, variant=variant) for path in fit_fossen_bags]
        off_dt = [path for path, b in zip(fit_fossen_bags, bags) if abs(b[2] - dt) > 1e-6 * dt]
        if off_dt:
            raise ValueError(f"recordings sampled at another dt than {csv_path} ({dt}): {off_dt}")
        t0 = perf_counter()
        rov_fit = make_rov()
        fit = rov_fit.fit_parameters_multi([b[0] for b in bags], [b[1] for b in bags], dt, H=10, integrator=integrator, iters=fit_iters,
                                           **cov_kw)
        t["fit_fossen"] = perf_counter() - t0
        fit_on = f"{len(bags)}-recording ({fit.n_windows} windows)"
    elif fit_fossen:
        t0 = perf_counter()
        rov_fit = make_rov()
        fit = rov_fit.fit_parameters(Xtr, Utr, dt, H=10, integrator=integrator, iters=fit_iters, **cov_kw)
        t["fit_fossen"] = perf_counter() - t0
    if fit is not None:
        fitted_row = [rov_fit.multistep_rmse_endpoint(Xte, Ute, H, dt, integrator) for H in (1, 10, 100)]
    ens = None
    if fit is not None and ensemble:
        t0 = perf_counter()
        steps = min(500, len(Xte) - 1)
        vehicles = identify.sample_parameters(fit, int(ensemble)) + [identify.params_of(rov_fit), identify.params_of(make_rov())]
        r = engine.rollout_pop(rov_fit.MODEL, integrator, vehicles, Xte[:1], Ute[None, :steps], dt, ctx=rov_fit._ctx)
        traj = r["traj"][:, 0]                             # [N + 2, steps + 1, nx]
        stats = engine.ensemble_stats(traj[:int(ensemble)], ctx=rov_fit._ctx)
        rec = Xte[:steps + 1]
        ens = dict(band_width=(stats["max"] - stats["min"]).mean(0), inside=((rec >= stats["min"]) & (rec <= stats["max"])).mean(0),
                   traj_fitted=traj[-2], traj_nominal=traj[-1], stats=stats, steps=steps)
        t["ensemble"] = perf_counter() - t0
    if verbose:
        print(f"\n[metrics] Endpoint RMSE (full {nx}D state) with identical evaluator:")
        print("  Model                 | 1-step RMSE | 10-step RMSE | 100-step RMSE")
        print("  ----------------------|------------:|-------------:|--------------:")
        for name, r in zip(ROWS, table):
            print(f"  {name:<21s} | {r[0]:11.6f} | {r[1]:12.6f} | {r[2]:13.6f}")
        if fitted_row is not None:
            print(f"  {'Fossen (fitted)':<21s} | {fitted_row[0]:11.6f} | {fitted_row[1]:12.6f} | {fitted_row[2]:13.6f}")
            print(f"  [fit] {fit_on} 10-step RMSE {fit.rmse_history[0]:.6f} -> {fit.rmse_history[-1]:.6f} in {sum(fit.accepted)} steps, "
                  f"{fit.n_evals} window evaluations: " + ", ".join(f"{k} = {v:.4g}" for k, v in fit.params.items()))
        if ens is not None:
            print(f"  [ensemble] {int(ensemble)} vehicles drawn around the fit, {ens['steps']}-step open-loop rollout of the test split; "
                  "per state: mean band width (max - min) / share of recorded samples inside the band")
            print("    " + "  ".join(f"x{i}: {w:.3g} / {100 * s:.0f}%" for i, (w, s) in enumerate(zip(ens["band_width"], ens["inside"]))))
        print("\n[timing] seconds:", {k: round(v, 4) for k, v in t.items()})
    return dict(table=table, timings=t, dt=dt, split=split, model=koop, ranking=np.argsort(np.argsort(table, axis=0), axis=0), rows=ROWS[:len(table)],
                pinc_weights=pinc, fossen_fitted=None if fitted_row is None else np.array(fitted_row), fossen_fit=fit, ensemble=ens)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("csv")
    ap.add_argument("--rbfs", type=int, default=500)
    ap.add_argument("--gamma", type=float, default=3.0)
    ap.add_argument("--ridge", type=float, default=1e-1)
    ap.add_argument("--rk4", action="store_true")
    ap.add_argument("--variant", default="thruster", choices=["thruster", "wrench", "quat"])
    ap.add_argument("--pinc-row", type=float, nargs=3, default=None, metavar=("RMSE1", "RMSE10", "RMSE100"),
                    help="the reference PINc network's endpoint RMSEs on the same test split (completes the table)")
    ap.add_argument("--pinc-ckpt", default=None, metavar="PATH",
                    help="PINc checkpoint (.pt state dict or .npz of its arrays): computes the fourth row on the engine")
    ap.add_argument("--pinc-train", type=int, default=None, metavar="EPOCHS",
                    help="train the PINc network on the train split for EPOCHS epochs on the engine, then compute the fourth row with it")
    ap.add_argument("--fit-fossen", action="store_true",
                    help="fit the Fossen model's damping to the train split at H = 10 and print a 'Fossen (fitted)' row under the table")
    ap.add_argument("--fit-fossen-bags", nargs="+", default=None, metavar="CSV",
                    help="fit the Fossen model's damping on these recordings instead, each file one bag (no window crosses from one "
                         "file into the next), and print the 'Fossen (fitted)' row")
    ap.add_argument("--ensemble", type=int, default=0, metavar="N",
                    help="with --fit-fossen / --fit-fossen-bags: draw N vehicles from the fit's covariance, roll all of them over 500 steps "
                         "of the test split in one launch and print the band they span per state")
    a = ap.parse_args()
    if sum(v is not None for v in (a.pinc_row, a.pinc_ckpt, a.pinc_train)) > 1:
        ap.error("--pinc-row, --pinc-ckpt and --pinc-train are mutually exclusive")
    compare(a.csv, a.rbfs, a.gamma, a.ridge, "rk4" if a.rk4 else "euler", variant=a.variant, pinc_row=a.pinc_row, pinc=a.pinc_ckpt,
            pinc_train=a.pinc_train, fit_fossen=a.fit_fossen, fit_fossen_bags=a.fit_fossen_bags, ensemble=a.ensemble)
