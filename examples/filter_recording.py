#!/usr/bin/env python3
"""State estimation from a noisy, gappy recording, and which vehicle explains it best.

A vehicle in a current is simulated under smooth thruster commands.  Its state rows get measurement noise (0.02 m, 0.01 rad,
0.03 m/s, 0.02 rad/s), 30 % of the entries are dropped and the roll rate is never measured at all: what tank odometry looks like.
rov.filter_states runs the unscented Kalman filter of include/brov2.h (brov_ukf_filter) over it on the device and the script prints
the raw against the filtered RMSE (second half of the recording) and the mean squared normalised innovation, which is near 1 when
the noise model fits.  Then the innovation log-likelihood ranks candidates: the true vehicle and --draws vehicles drawn around it
with identify.sample_parameters (rov.log_likelihood_population: every candidate filters the recording in ONE launch).

With --smooth, rov.smooth_states (the unscented Rauch-Tung-Striebel smoother, brov_ukf_smooth) runs instead of the filter alone and
the smoothed RMSE is printed beside the filtered one: the recording is complete, so every row may be estimated from all rows.

With --fit-noise the noise model is not given but fitted: rov.fit_noise runs expectation-maximisation on q and r (brov_ukf_smooth_em,
one smoother call per iteration that stores no rows) from a deliberately wrong guess, q x 100 and sigma x 3, and the script prints
the log-likelihood per iteration, the fitted against the true sigma, and the filtered and smoothed RMSE under the guess and under
the fit.  EM finds r within a few updates and moves q slowly (some 75 updates until the log-likelihood rises by less than 1e-4 of
itself here); stopped after 10 or 20, r has already shrunk to the truth while q is still far too large, and the RMSE is then worse
than under the guess, so the loop runs to its tolerance.

With --quat the vehicle is the quaternion one (fossen/BlueROV2_wrench.py) and the recording starts within 0.1 rad of pitch 90
degrees, where the Euler-angle vehicles have their 1 / cos(theta): rov.filter_states then runs the multiplicative filter
(brov_ukf_filter_quat), whose covariance lives in a 12-component error state.  The attitude errors are taken through
estimate.quat_boxminus (rad at small angles); every third measured quaternion is reported negated, which the filter must not see.
The small sizes (3 s, 7 draws).  With --quat --smooth, rov.smooth_states_quat (brov_ukf_smooth_quat) runs instead of the filter alone
and the smoothed RMSE of position, attitude and velocity is printed beside the filtered one; --quat --fit-noise is an error: the
quaternion vehicle has no EM fit.

    python examples/filter_recording.py [--seconds 10 --draws 31 --std 0.1 --seed 0] [--small] [--smooth] [--fit-noise] [--quat]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bluerov2_dynamics_amd import engine                                # noqa: E402
from bluerov2_dynamics_amd.fossen import estimate, identify            # noqa: E402
from bluerov2_dynamics_amd.fossen.BlueROV2 import BlueROV2              # noqa: E402

SIGMA = np.array([0.02] * 3 + [0.01] * 3 + [0.03] * 3 + [0.02] * 3)
UNMEASURED = 9                      # the roll rate
SPREAD = ("Xu", "Yv", "Zw", "Nr", "Xu_abs", "Yv_abs", "Zw_abs", "Nr_abs", "Xu_dot", "Yv_dot", "Zw_dot", "Nr_dot")


def drawn_vehicles(base, n, seed, rel_std):
    """n vehicles around `base` through identify.sample_parameters: a stand-in fit whose covariance is diagonal, rel_std per term"""
    theta = {k: identify.get_param(base, k) for k in SPREAD}
    cov = np.diag([(rel_std * v) ** 2 for v in theta.values()])
    fit = identify.FitResult(params=theta, rmse_history=[], accepted=[], n_evals=0, brov_params=base, covariance=cov)
    return identify.sample_parameters(fit, n, seed=seed)


def fit_noise_demo(rov, true, X, Y, U, dt, start, P0, integrator, iters, verbose):
    """EM from (q x 100, sigma x 3): dict(sigma_start, sigma_fit [12], q_fit, loglik_fit [its + 1], fit_converged,
    rmse_filtered_before / _after, rmse_smoothed_before / _after (second half, measured entries))"""
    T = Y.shape[0]
    r = (3.0 * SIGMA) ** 2
    r[UNMEASURED] = np.inf
    guess = estimate.ukf(q=1e-4, r=r)
    half = slice(T // 2, T)
    seen = ~np.isnan(Y[half])
    rmse = lambda x: float(np.sqrt(np.mean((x[half] - X[:T][half])[seen] ** 2)))
    before = rov.smooth_states(Y, U, dt, guess, x0=start, P0=P0, params=true, integrator=integrator)
    fit = rov.fit_noise(Y, U, dt, guess, x0=start, P0=P0, params=true, integrator=integrator, iters=iters)
    after = rov.smooth_states(Y, U, dt, fit["cfg"], x0=start, P0=P0, params=true, integrator=integrator)
    out = dict(sigma_start=3.0 * SIGMA, sigma_fit=np.sqrt(fit["r"]), q_fit=fit["q"], loglik_fit=fit["loglik"], fit_converged=fit["converged"],
               rmse_filtered_before=rmse(before["x"]), rmse_filtered_after=rmse(after["x"]),
               rmse_smoothed_before=rmse(before["xs"]), rmse_smoothed_after=rmse(after["xs"]))
    if verbose:
        print(f"EM fit of q and r from q x 100 and sigma x 3, {len(fit['loglik']) - 1} updates" + (" (converged)" if fit["converged"] else ""))
        for k, l in enumerate(fit["loglik"]):
            if k < 5 or k % 10 == 0 or k == len(fit["loglik"]) - 1:
                print(f"    after {k:3d} updates   log-likelihood {l:12.1f}")
        print("    component   sigma true    start   fitted")
        for i in range(12):
            if i != UNMEASURED:
                print(f"    {i:9d}   {SIGMA[i]:10.4f} {3 * SIGMA[i]:8.4f} {out['sigma_fit'][i]:8.4f}")
        print(f"    RMSE filtered {out['rmse_filtered_before']:.4f} -> {out['rmse_filtered_after']:.4f}, "
              f"smoothed {out['rmse_smoothed_before']:.4f} -> {out['rmse_smoothed_after']:.4f}")
    return out


def run(seconds=10.0, dt=0.02, draws=31, rel_std=0.1, dropout=0.3, integrator="rk4", seed=0, verbose=True, smooth=False, fit_noise=False,
        fit_iters=100):
    """Returns dict(X [T+1,12] the truth, Y [T,12] the noisy rows, x, std, innov [T,12] of the filter, rmse_raw, rmse_filtered, nis,
    loglik [draws + 1] with the true vehicle at index 0, order: the candidates from best to worst); with smooth also xs, std_s
    [T,12] of the smoother, rmse_smoothed and rmse_unmeasured_filtered / _smoothed (the never-measured roll rate)"""
    rov = BlueROV2(dt=dt)
    true = identify.copy_params(identify.params_of(rov))
    for i, v in enumerate((0.15, -0.1, 0.03)):
        true.current[i] = v
    T = int(round(seconds / dt))
    rng = np.random.default_rng(seed)
    t = np.arange(T) * dt
    U = 0.5 * np.sin(2 * np.pi * np.outer(t, np.linspace(0.3, 1.0, 8)) + rng.uniform(0, 6, 8))
    x0 = np.zeros(12)
    x0[2] = 5.0
    X = engine.rollout_pop(rov.MODEL, integrator, [true], x0[None], U[None], dt, ctx=rov._ctx)["traj"][0, 0]
    Y = X[:T] + rng.normal(size=(T, 12)) * SIGMA
    Y[rng.uniform(size=Y.shape) < dropout] = np.nan
    Y[:, UNMEASURED] = np.nan
    r = SIGMA ** 2
    r[UNMEASURED] = np.inf
    cfg = estimate.ukf(q=1e-6, r=r)
    start = x0 + rng.normal(size=12) * SIGMA
    P0 = np.diag(np.where(np.isfinite(r), 4.0 * SIGMA ** 2, estimate.P0_STAND_IN))
    estimator = rov.smooth_states if smooth else rov.filter_states
    f = estimator(Y, U, dt, cfg, x0=start, P0=P0, params=true, integrator=integrator)
    half = slice(T // 2, T)
    seen = ~np.isnan(Y[half])
    rmse_raw = float(np.sqrt(np.mean((Y[half] - X[:T][half])[seen] ** 2)))
    rmse_f = float(np.sqrt(np.mean((f["x"][half] - X[:T][half])[seen] ** 2)))
    nis = float(np.nanmean(f["innov"] ** 2))
    extra = {}
    if smooth:
        miss = lambda x: float(np.sqrt(np.mean((x[half, UNMEASURED] - X[:T][half, UNMEASURED]) ** 2)))
        extra = dict(xs=f["xs"], std_s=f["std_s"], rmse_smoothed=float(np.sqrt(np.mean((f["xs"][half] - X[:T][half])[seen] ** 2))),
                     rmse_unmeasured_filtered=miss(f["x"]), rmse_unmeasured_smoothed=miss(f["xs"]))
    if fit_noise:
        extra.update(fit_noise_demo(rov, true, X, Y, U, dt, start, P0, integrator, fit_iters, verbose))
    cands = [true] + drawn_vehicles(true, int(draws), seed + 1, rel_std)
    ll = rov.log_likelihood_population(cands, Y, U, dt, cfg, x0=start, P0=P0, integrator=integrator)[:, 0]
    order = np.argsort(-ll)
    if verbose:
        print(f"{T} rows of {dt} s, {np.isnan(Y).mean():.0%} of the entries missing, {f['n_updates']} scalar updates, "
              f"smallest Cholesky pivot {f['min_pivot']:.2e}")
        print(f"RMSE over the second half, measured entries: raw {rmse_raw:.4f}, filtered {rmse_f:.4f}")
        print(f"error of the never-measured roll rate: {np.sqrt(np.mean((f['x'][half, UNMEASURED] - X[:T][half, UNMEASURED]) ** 2)):.4f} rad/s "
              f"(its own scale: {np.std(X[:, UNMEASURED]):.4f})")
        if smooth:
            print(f"smoothed (every row from all rows): RMSE {extra['rmse_smoothed']:.4f} against {rmse_f:.4f} filtered; "
                  f"roll rate {extra['rmse_unmeasured_smoothed']:.4f} against {extra['rmse_unmeasured_filtered']:.4f} rad/s")
        print(f"mean squared normalised innovation {nis:.2f} (1 when the noise model fits)")
        print(f"log-likelihood of {len(cands)} candidates (0 = the true vehicle, the others drawn with {rel_std:.0%} on {len(SPREAD)} terms):")
        for k in order[:5]:
            print(f"    candidate {k:3d}   {ll[k]:12.1f}")
        print(f"    ...   worst   {ll[order[-1]]:12.1f}")
    return dict(X=X, Y=Y, x=f["x"], std=f["std"], innov=f["innov"], rmse_raw=rmse_raw, rmse_filtered=rmse_f, nis=nis, loglik=ll, order=order,
                **extra)


def run_quat(seconds=3.0, dt=0.02, draws=7, rel_std=0.1, dropout=0.3, integrator="rk4", seed=0, verbose=True, smooth=False):
    """The quaternion vehicle, started near vertical.  Returns dict(X [T+1,13], Y [T,13], x [T,13], std, innov [T,12], rmse_raw,
    rmse_filtered: dict(position, attitude, velocity) over the measured entries of the second half, nis, loglik [draws + 1] with the
    true vehicle at index 0, order, rank_true); with smooth also xs [T,13], std_s [T,12] of the smoother and rmse_smoothed, a dict
    like rmse_filtered"""
    from bluerov2_dynamics_amd.fossen.BlueROV2_wrench import BlueROV2 as BlueROV2Quat, euler_to_quat
    rov = BlueROV2Quat()
    true = identify.copy_params(identify.params_of(rov))
    for i, v in enumerate((0.15, -0.1, 0.03)):
        true.current[i] = v
    T = int(round(seconds / dt))
    rng = np.random.default_rng(seed)
    t = np.arange(T) * dt
    U = 0.5 * np.sin(2 * np.pi * np.outer(t, np.linspace(0.3, 1.0, 6)) + rng.uniform(0, 6, 6)) * np.array([10.0, 10.0, 10.0, 0.5, 0.5, 0.5])
    x0 = np.zeros(13)
    x0[2] = 5.0
    x0[3:7] = euler_to_quat(0.1, np.pi / 2 - rng.uniform(0.0, 0.1), -0.2)
    X = engine.rollout_pop(rov.MODEL, integrator, [true], x0[None], U[None], dt, ctx=rov._ctx)["traj"][0, 0]
    Y = estimate.quat_boxplus(X[:T], rng.normal(size=(T, 12)) * SIGMA)
    gone = rng.uniform(size=(T, 12)) < dropout
    gone[:, UNMEASURED] = True
    Y[np.concatenate([gone[:, :3], np.repeat(gone[:, 3:4], 4, 1), gone[:, 6:]], 1)] = np.nan     # the attitude is measured as a whole
    Y[::3, 3:7] *= -1.0                                                                          # q and -q are the same attitude
    r = SIGMA ** 2
    r[UNMEASURED] = np.inf
    cfg = estimate.ukf(q=1e-6, r=r)
    start = estimate.quat_boxplus(x0, rng.normal(size=12) * SIGMA)
    P0 = np.diag(np.where(np.isfinite(r), 4.0 * SIGMA ** 2, estimate.P0_STAND_IN))
    estimator = rov.smooth_states_quat if smooth else rov.filter_states
    f = estimator(Y, U, dt, cfg, x0=start, P0=P0, params=true, integrator=integrator)
    half = slice(T // 2, T)
    att = ~np.isnan(Y[:, 3:7]).any(axis=1)
    seen = np.concatenate([~np.isnan(Y[:, :3]), np.repeat(att[:, None], 3, 1), ~np.isnan(Y[:, 7:])], 1)[half]
    e_raw = estimate.quat_boxminus(np.where(np.isnan(Y), X[:T], Y), X[:T])[half]                 # (what is not seen is masked below)
    e_f = estimate.quat_boxminus(f["x"], X[:T])[half]
    parts = dict(position=slice(0, 3), attitude=slice(3, 6), velocity=slice(6, 12))
    rmse = lambda e: {k: float(np.sqrt(np.mean(e[:, c][seen[:, c]] ** 2))) for k, c in parts.items()}
    rmse_raw, rmse_f = rmse(e_raw), rmse(e_f)
    nis = float(np.nanmean(f["innov"] ** 2))
    extra = {}
    if smooth:
        extra = dict(xs=f["xs"], std_s=f["std_s"], rmse_smoothed=rmse(estimate.quat_boxminus(f["xs"], X[:T])[half]))
    cands = [true] + drawn_vehicles(true, int(draws), seed + 1, rel_std)
    ll = rov.log_likelihood_population(cands, Y, U, dt, cfg, x0=start, P0=P0, integrator=integrator)[:, 0]
    order = np.argsort(-ll)
    rank = int(np.flatnonzero(order == 0)[0])
    if verbose:
        pitch = np.degrees(np.arcsin(np.clip(2.0 * (X[:, 3] * X[:, 5] - X[:, 6] * X[:, 4]), -1.0, 1.0)))
        print(f"{T} rows of {dt} s on the quaternion vehicle, pitch between {pitch.min():.1f} and {pitch.max():.1f} degrees, "
              f"{f['n_updates']} scalar updates, smallest Cholesky pivot {f['min_pivot']:.2e}")
        for k in parts:
            print(f"RMSE over the second half, measured entries, {k}: raw {rmse_raw[k]:.4f}, filtered {rmse_f[k]:.4f}")
        for k in parts if smooth else ():
            print(f"smoothed (every row from all rows), {k}: RMSE {extra['rmse_smoothed'][k]:.4f} against {rmse_f[k]:.4f} filtered")
        print(f"mean squared normalised innovation {nis:.2f} (1 when the noise model fits)")
        print(f"the true vehicle ranks {rank + 1} of {len(cands)} by log-likelihood ({ll[0]:.1f}; best {ll[order[0]]:.1f}, worst {ll[order[-1]]:.1f})")
    return dict(X=X, Y=Y, x=f["x"], std=f["std"], innov=f["innov"], rmse_raw=rmse_raw, rmse_filtered=rmse_f, nis=nis, loglik=ll, order=order,
                rank_true=rank, **extra)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--draws", type=int, default=31)
    ap.add_argument("--std", type=float, default=0.1, help="relative standard deviation of the drawn vehicles' terms")
    ap.add_argument("--euler", action="store_true")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--small", action="store_true", help="3 s and 7 draws: runs in seconds")
    ap.add_argument("--smooth", action="store_true", help="also smooth the recording (rov.smooth_states) and print the smoothed RMSE")
    ap.add_argument("--fit-noise", action="store_true", help="fit q and r by EM from a wrong guess (rov.fit_noise) and print what it gains")
    ap.add_argument("--quat", action="store_true", help="the quaternion vehicle from a start near pitch 90 degrees, in the small sizes")
    a = ap.parse_args(argv)
    if a.quat:
        if a.fit_noise:
            ap.error("--quat: the quaternion vehicle has the filter and the smoother, no EM fit (no --fit-noise)")
        return run_quat(rel_std=a.std, integrator="euler" if a.euler else "rk4", seed=a.seed, smooth=a.smooth)
    if a.small:
        a.seconds, a.draws = 3.0, 7
    return run(a.seconds, draws=a.draws, rel_std=a.std, integrator="euler" if a.euler else "rk4", seed=a.seed, smooth=a.smooth,
               fit_noise=a.fit_noise)


if __name__ == "__main__":
    main()
