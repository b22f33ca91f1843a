"""The filter problems that tests/test_ukf_gpu.py runs on the device and tests/test_ukf_cpu.py checks for well-posedness on the
reference alone (tests/ukf_ref.py).  Not collected.

Every case: P = 2 candidates (V0, V5 of tests/fossen_vehicles.py), T = 12 rows at dt = 0.02.  The recordings are simulated with V5
(the vehicle with a current) by the oracle, then noise of sigma = 0.02 m / 0.01 rad / 0.03 m/s / 0.02 rad/s is added, about 30 % of
the entries are dropped (NaN), row 4 of every recording is dropped entirely, and component 7 is never measured (r = +inf, its Y
column still carries numbers, which the filter must ignore).  P0 is a dense positive-definite matrix whose UPPER triangle is NaN
in the input: only the lower one may be read.  The thruster model starts from a random lag.  The seeds are pinned: with them the
margins of test_ukf_cpu.py::test_gpu_cases_are_well_posed hold."""
import functools

import numpy as np

import fossen_vehicles as fv
import ukf_ref as ur
from oracle import fossen_params as fp

L = np.longdouble
T, DT = 12, 0.02
NAMES = ("V0", "V5")
TRUE = "V5"
SIGMA = np.array([0.02] * 3 + [0.01] * 3 + [0.03] * 3 + [0.02] * 3)
UNMEASURED = 7
EMPTY_ROW = 4
INTEG = {"euler": fp.EULER, "rk4": fp.RK4}
SEED = 7301

# name -> model, integrator, lag mode, alpha, B, kind
CASES = {
    "thr_euler": (0, "euler", 0, 1.0, 3, "std"),
    "thr_rk4": (0, "rk4", 0, 0.5, 3, "std"),
    "wr_euler": (1, "euler", 0, 0.5, 3, "std"),
    "wr_rk4": (1, "rk4", 0, 1.0, 3, "std"),
    "thr_rk4_lagstep": (0, "rk4", 1, 1.0, 3, "std"),
    "thr_rk4_ragged": (0, "rk4", 0, 1.0, 5, "std"),
    "wr_rk4_nrec2": (1, "rk4", 0, 1.0, 3, "nrec2"),
    "thr_euler_wrap": (0, "euler", 0, 1.0, 3, "wrap"),
}


def chan_scale(model):
    """size of a command channel: thruster commands ~1, forces ~10 N, moments ~0.5 N m"""
    return np.ones(8) if model == 0 else np.array([10.0, 10.0, 10.0, 0.5, 0.5, 0.5])


def noise_cfg(alpha, scale=1.0):
    r = (SIGMA * scale) ** 2
    r[UNMEASURED] = np.inf
    return ur.cfg(q=1e-6 * np.linspace(1.0, 3.0, 12), r=r, alpha=alpha, beta=2.0, kappa=1.0)


@functools.lru_cache(maxsize=None)
def inputs(name):
    """dict(model, integ, lag_mode, B, cfgs, x0 [B,12], P0 [B,12,12], U [B,T,nu], Y [B,T,12], lag [2,B,8,3] | None, X [B,T+1,12])"""
    model, integ, lag_mode, alpha, B, kind = CASES[name]
    rng = np.random.default_rng(SEED + sorted(CASES).index(name))
    nu = fp.NU[model]
    xs = rng.uniform(-0.3, 0.3, (B, 12))
    U = rng.uniform(-0.3, 0.3, (B, T, nu)) * chan_scale(model)
    lag = rng.uniform(-1, 1, (len(NAMES), B, 8, 3)) if model == 0 else None
    if kind == "wrap":                   # the yaw starts just below pi and turns through it
        xs[:, 5] = 3.1
        xs[:, 11] = 0.9
    X = fp.rollout(model, INTEG[integ], lag_mode, fv.vehicle(TRUE), xs, U, DT, lag=None if lag is None else lag[1])["traj"]
    Ym = X[:, :T].copy()
    if kind == "wrap":
        assert X[:, :T, 5].max() > np.pi + 0.02, "the true yaw must leave [-pi, pi]"
        Ym[:, :, 5] = Ym[:, :, 5] - 2 * np.pi * np.rint(Ym[:, :, 5] / (2 * np.pi))
    Y = Ym + rng.normal(size=Ym.shape) * SIGMA
    Y[rng.uniform(size=Y.shape) < 0.3] = np.nan
    Y[:, EMPTY_ROW] = np.nan
    Y[:, :, UNMEASURED] = X[:, :T, UNMEASURED] + 5.0          # numbers the filter must not look at
    x0 = X[:, 0] + rng.normal(size=(B, 12)) * SIGMA
    d = np.sqrt(4.0 * SIGMA ** 2)
    M = rng.normal(size=(B, 12, 12))
    C = 0.7 * np.eye(12) + 0.3 * (M @ M.transpose(0, 2, 1)) / 12.0
    P0 = d[None, :, None] * C * d[None, None, :]
    P0 = 0.5 * (P0 + P0.transpose(0, 2, 1))
    P0[:, np.triu_indices(12, 1)[0], np.triu_indices(12, 1)[1]] = np.nan
    cfgs = [noise_cfg(alpha), noise_cfg(0.5 if alpha == 1.0 else 1.0, scale=1.5)] if kind == "nrec2" else noise_cfg(alpha)
    return dict(model=model, integ=integ, lag_mode=lag_mode, B=B, cfgs=cfgs, x0=x0, P0=P0, U=U, Y=Y, lag=lag, X=X)


@functools.lru_cache(maxsize=None)
def reference(name, ld=False, lag_mode=None):
    """ukf_ref.filter on inputs(name), in fp64 or long double; lag_mode overrides the case's"""
    i = inputs(name)
    return ur.filter(i["model"], INTEG[i["integ"]], i["lag_mode"] if lag_mode is None else lag_mode, [fv.vehicle(n) for n in NAMES], i["cfgs"],
                     i["x0"], i["P0"], i["U"], i["Y"], DT, lag=i["lag"], dtype=L if ld else np.float64)


def err(a, b):
    """max |a-b| / max(1, |b|) over the finite entries of b, formed in long double; inf where the NaN patterns differ"""
    a, b = np.asarray(a, dtype=L), np.asarray(b, dtype=L)
    if a.shape != b.shape or np.any(np.isnan(a) != np.isnan(b)):
        return np.inf
    ok = ~np.isnan(b)
    both_inf = ok & np.isinf(a) & np.isinf(b) & (a == b)
    ok &= ~both_inf
    return float(np.max(np.abs(a[ok] - b[ok]) / np.maximum(L(1), np.abs(b[ok])))) if ok.any() else 0.0


def cov_err(a, b):
    """max |a_ij - b_ij| / sqrt(b_ii b_jj) over [..., 12, 12], formed in long double (entries of 1e-5 would hide behind err)"""
    a, b = np.asarray(a, dtype=L), np.asarray(b, dtype=L)
    if a.shape != b.shape or np.any(np.isnan(a) != np.isnan(b)):
        return np.inf
    dg = np.sqrt(np.diagonal(b, axis1=-2, axis2=-1))
    rel = np.abs(a - b) / (dg[..., :, None] * dg[..., None, :])
    ok = ~np.isnan(rel)
    return float(np.max(rel[ok])) if ok.any() else 0.0


PARITY_KEYS = ("xf", "pstd", "innov", "xT", "info")


def gaps(o, ol):
    """{output: error of o against ol}: the mixed error, and the covariance measure for PT"""
    g = {k: err(o[k], ol[k]) for k in PARITY_KEYS + ("lag",) if o.get(k) is not None}
    g["PT"] = cov_err(o["PT"], ol["PT"])
    return g
