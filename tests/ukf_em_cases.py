"""The problems of the EM statistics (brov_ukf_rts_em_dev, brov_ukf_smooth_em), computed once and shared by tests/test_ukf_em_cpu.py
and tests/test_ukf_em_gpu.py (tests/ukf_em_ref.py is the law).  Not collected.

The eight cases of tests/ukf_smooth_cases.py (P = 2, B = 3 or 5, T = 12) and two of their inputs under another noise model:
  bigq    wr_rk4 with q x 100 and sigma x 3: the correction term q^2 u^T (M + dx dx^T) u is then no 2 % effect next to q
  zeroq   thr_rk4 with q[2] = q[9] = 0: Sq of those components is 0.0 exactly"""
import functools

import numpy as np

import fossen_vehicles as fv
import ukf_cases as uc
import ukf_em_ref as uer
import ukf_ref as ur
import ukf_smooth_cases as us

TOL = us.TOL
EXTRA = {"bigq": "wr_rk4", "zeroq": "thr_rk4"}
NAMES = us.NAMES + tuple(EXTRA)


def start_cfg(alpha=1.0):
    """the start of the EM tests: q x 100 and sigma x 3 of tests/ukf_cases.py"""
    c = uc.noise_cfg(alpha, scale=3.0)
    return ur.Cfg(q=c.q * 100.0, r=c.r, alpha=c.alpha, beta=c.beta, kappa=c.kappa)


@functools.lru_cache(maxsize=None)
def inputs(name):
    """uc.inputs of the case, for bigq and zeroq with their own cfgs"""
    if name not in EXTRA:
        return uc.inputs(name)
    i = dict(uc.inputs(EXTRA[name]))
    c = i["cfgs"]
    if name == "bigq":
        i["cfgs"] = start_cfg(c.alpha)
    else:
        q = c.q.copy()
        q[2] = q[9] = 0.0
        i["cfgs"] = ur.Cfg(q=q, r=c.r, alpha=c.alpha, beta=c.beta, kappa=c.kappa)
    return i


def vehicles():
    return [fv.vehicle(n) for n in uc.NAMES]


def stats(name, ld=False, **kw):
    """ukf_em_ref.stats on inputs(name) with the entries of kw replaced"""
    i = inputs(name)
    a = dict(x0=i["x0"], P0=i["P0"], U=i["U"], Y=i["Y"], lag=i["lag"], terminal=None, cfgs=i["cfgs"])
    a.update(kw)
    return uer.stats(i["model"], uc.INTEG[i["integ"]], i["lag_mode"], vehicles(), a["cfgs"], a["x0"], a["P0"], a["U"], a["Y"], uc.DT, lag=a["lag"],
                     dtype=uc.L if ld else np.float64, terminal=a["terminal"])


@functools.lru_cache(maxsize=None)
def reference(name, ld=False, pair=False):
    """read-only: shared among the tests.  pair: with terminal(name) as the terminal pair"""
    return stats(name, ld, terminal=terminal(name) if pair else None)


def terminal(name):
    """a terminal pair for the case: the fp64 reference filter's (xT, PT), the estimate of row T before its measurement"""
    o = reference(name)
    return o["xT"].astype(np.float64), o["PT"].astype(np.float64)


def em_err(a, b):
    """largest relative difference per entry of em [.., 37] against b, formed in long double; the counts (entries 24 ..) and the
    NaN pattern must agree exactly (inf otherwise).  An entry that is 0 in b must be 0 in a."""
    a, b = np.asarray(a, dtype=uc.L), np.asarray(b, dtype=uc.L)
    if a.shape != b.shape or np.any(np.isnan(a) != np.isnan(b)) or not np.array_equal(a[..., 24:], b[..., 24:], equal_nan=True):
        return np.inf
    x, y = a[..., :24], b[..., :24]
    ok = ~np.isnan(y)
    if np.any((y == 0) & ok & (x != 0)):
        return np.inf
    nz = ok & (y != 0)
    return float(np.max(np.abs(x[nz] - y[nz]) / np.abs(y[nz]))) if nz.any() else 0.0


@functools.lru_cache(maxsize=None)
def long_inputs(name, T=40, B=3):
    """the recipe of uc.inputs at T rows for the EM loop on the reference alone: recordings of the true vehicle with the noise of
    uc.SIGMA, 30 % of the entries and row 4 dropped, component 7 never measured; P0 = diag(4 sigma^2), full"""
    from oracle import fossen_params as fp
    model, integ, lag_mode, alpha, _, _ = uc.CASES[name]
    rng = np.random.default_rng(uc.SEED + 100 + sorted(uc.CASES).index(name))
    xs = rng.uniform(-0.3, 0.3, (B, 12))
    U = rng.uniform(-0.3, 0.3, (B, T, fp.NU[model])) * uc.chan_scale(model)
    X = fp.rollout(model, uc.INTEG[integ], lag_mode, fv.vehicle(uc.TRUE), xs, U, uc.DT, lag=None)["traj"]
    Y = X[:, :T] + rng.normal(size=(B, T, 12)) * uc.SIGMA
    Y[rng.uniform(size=Y.shape) < 0.3] = np.nan
    Y[:, uc.EMPTY_ROW] = np.nan
    Y[:, :, uc.UNMEASURED] = X[:, :T, uc.UNMEASURED] + 5.0
    x0 = X[:, 0] + rng.normal(size=(B, 12)) * uc.SIGMA
    P0 = np.repeat(np.diag(4.0 * uc.SIGMA ** 2)[None], B, axis=0)
    return dict(model=model, integ=integ, lag_mode=lag_mode, B=B, cfgs=start_cfg(alpha), x0=x0, P0=P0, U=U, Y=Y, lag=None, X=X)
