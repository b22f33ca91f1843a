"""The filter problems of the quaternion model that tests/test_ukf_quat_gpu.py runs on the device and tests/test_ukf_quat_cpu.py
checks for well-posedness on the reference alone (tests/ukf_quat_ref.py).  Not collected.  The recipe of tests/ukf_cases.py:

Every case: P = 2 candidates (V0, V5 of tests/fossen_vehicles.py), T = 12 rows at dt = 0.02.  The recordings are simulated with V5
(the vehicle with a current) by the oracle, then noise of sigma = 0.02 m / 0.01 (chart units, rad) / 0.03 m/s / 0.02 rad/s is added
through [+], about 30 % of the measurements are dropped (NaN; the attitude as a whole, and in about a tenth of the rows a single
one of its four numbers, which must drop the attitude of that row too), row 4 of every recording is dropped entirely, and error
component 7 (state column 8) is never measured (r = +inf, its Y column still carries numbers, which the filter must ignore).  P0 is
a dense positive-definite matrix whose UPPER triangle is NaN in the input: only the lower one may be read.  The seeds are pinned:
with them the margins of test_ukf_quat_cpu.py::test_gpu_cases_are_well_posed hold."""
import functools

import numpy as np

import fossen_vehicles as fv
import ukf_cases as uc
import ukf_quat_ref as uq
import ukf_ref as ur
from oracle import fossen_params as fp

L = np.longdouble
T, DT = uc.T, uc.DT
NAMES, TRUE = uc.NAMES, uc.TRUE
SIGMA = uc.SIGMA
UNMEASURED = 7                      # in the error state; column UNMEASURED + 1 of Y
EMPTY_ROW = 4
INTEG = uc.INTEG
SEED = 9107

# name -> integrator, alpha, B, kind
CASES = {
    "q_euler": ("euler", 0.5, 3, "std"),
    "q_rk4": ("rk4", 1.0, 3, "std"),
    "q_rk4_ragged": ("rk4", 1.0, 5, "std"),
    "q_rk4_nrec2": ("rk4", 1.0, 3, "nrec2"),
    "q_rk4_vertical": ("rk4", 1.0, 3, "vertical"),
}


def quat_of_euler(phi, th, psi):
    """Z-Y-X Euler angles -> quaternion [..., 4], w first"""
    cf, sf, ct, st, cp, sp = np.cos(phi / 2), np.sin(phi / 2), np.cos(th / 2), np.sin(th / 2), np.cos(psi / 2), np.sin(psi / 2)
    return np.stack([cf * ct * cp + sf * st * sp, sf * ct * cp - cf * st * sp, cf * st * cp + sf * ct * sp, cf * ct * sp - sf * st * cp], -1)


def boxplus(X, D):
    """ukf_quat_ref.boxplus over leading dimensions"""
    X, D = np.asarray(X), np.asarray(D)
    out = np.empty(X.shape, dtype=X.dtype)
    for i in np.ndindex(X.shape[:-1]):
        out[i] = uq.boxplus(X[i], D[i])
    return out


def boxminus(A, B):
    A, B = np.asarray(A), np.asarray(B)
    out = np.empty(A.shape[:-1] + (12,), dtype=A.dtype)
    for i in np.ndindex(A.shape[:-1]):
        out[i] = uq.boxminus(A[i], B[i])[0]
    return out


def start_states(rng, B, vertical):
    """[B,13]: positions, Euler angles and velocities in +-0.3; vertical: the pitch within 0.1 rad of 90 degrees"""
    e = rng.uniform(-0.3, 0.3, (B, 12))
    th = np.pi / 2 + rng.uniform(-0.1, 0.1, B) if vertical else e[:, 4]
    return np.concatenate([e[:, :3], quat_of_euler(e[:, 3], th, e[:, 5]), e[:, 6:]], 1)


def measure(rng, X, sigma=SIGMA, drop=0.3):
    """Y [B,T,13] from the true rows X [B,T,13]: noise through [+], then the dropouts of the module text (without the empty row and
    the unmeasured column)"""
    Y = boxplus(X, rng.normal(size=X.shape[:-1] + (12,)) * sigma)
    m = rng.uniform(size=X.shape[:-1] + (12,)) < drop
    m13 = np.concatenate([m[..., :3], np.repeat(m[..., 3:4], 4, -1), m[..., 6:]], -1)
    Y[m13] = np.nan
    one = m[..., 4] & m[..., 5]                              # a single number of the quaternion missing
    Y[..., 4] = np.where(one, np.nan, Y[..., 4])
    return Y


@functools.lru_cache(maxsize=None)
def inputs(name):
    """dict(integ, B, cfgs, x0 [B,13], P0 [B,12,12], U [B,T,6], Y [B,T,13], X [B,T+1,13])"""
    integ, alpha, B, kind = CASES[name]
    rng = np.random.default_rng(SEED + sorted(CASES).index(name))
    vertical = kind == "vertical"
    xs = start_states(rng, B, vertical)
    U = rng.uniform(-0.3, 0.3, (B, T, 6)) * uc.chan_scale(1)
    X = fp.rollout(fp.WRENCH_QUAT, INTEG[integ], 0, fv.vehicle(TRUE), xs, U, DT)["traj"]
    Y = measure(rng, X[:, :T])
    Y[:, EMPTY_ROW] = np.nan
    Y[:, :, UNMEASURED + 1] = X[:, :T, UNMEASURED + 1] + 5.0          # numbers the filter must not look at
    x0 = boxplus(X[:, 0], rng.normal(size=(B, 12)) * SIGMA)
    if vertical:
        assert np.all(np.abs(np.arcsin(np.clip(2 * (xs[:, 3] * xs[:, 5] - xs[:, 6] * xs[:, 4]), -1, 1)) - np.pi / 2) < 0.1 + 1e-6)
        x0[:, 3:7] = -x0[:, 3:7]
        Y[:, ::3, 3:7] *= -2.0
    d = np.sqrt(4.0 * SIGMA ** 2)
    M = rng.normal(size=(B, 12, 12))
    C = 0.7 * np.eye(12) + 0.3 * (M @ M.transpose(0, 2, 1)) / 12.0
    P0 = d[None, :, None] * C * d[None, None, :]
    P0 = 0.5 * (P0 + P0.transpose(0, 2, 1))
    P0[:, np.triu_indices(12, 1)[0], np.triu_indices(12, 1)[1]] = np.nan
    cfgs = [uc.noise_cfg(alpha), uc.noise_cfg(0.5 if alpha == 1.0 else 1.0, scale=1.5)] if kind == "nrec2" else uc.noise_cfg(alpha)
    return dict(integ=integ, B=B, cfgs=cfgs, x0=x0, P0=P0, U=U, Y=Y, X=X)


@functools.lru_cache(maxsize=None)
def reference(name, ld=False, variant=None):
    """ukf_quat_ref.filter on inputs(name), in fp64 or long double; variant: one of the law's neighbours"""
    i = inputs(name)
    return uq.filter(INTEG[i["integ"]], [fv.vehicle(n) for n in NAMES], i["cfgs"], i["x0"], i["P0"], i["U"], i["Y"], DT,
                     dtype=L if ld else np.float64, variant=variant)


err, cov_err = uc.err, uc.cov_err
PARITY_KEYS = uc.PARITY_KEYS


def gaps(o, ol):
    """{output: error of o against ol}: the mixed error, and the covariance measure for PT"""
    g = {k: err(o[k], ol[k]) for k in PARITY_KEYS}
    g["PT"] = cov_err(o["PT"], ol["PT"])
    return g
