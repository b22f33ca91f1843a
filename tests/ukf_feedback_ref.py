"""NumPy restatement of the output-feedback closed loop of include/brov2.h (brov_output_feedback), and the problems that
tests/test_output_feedback_gpu.py runs on the device and tests/test_output_feedback_cpu.py checks for well-posedness on the
reference alone.  Not collected.

loop() composes what is already pinned: ukf_ref.update_row / predict (the filter's two stages), feedback_ref.error_lanes (the
tracking error) and the parameterised oracle's step (the plant), in the order of the header: measure, update, command, plant,
predict.  Dtype-generic (np.float64 / np.longdouble); plain loops over (candidate, run).  Besides the outputs of the entry point it
returns, per (candidate, run):
  wrap_margin  the smallest distance of a wrapped difference from its threshold: the filter's (innovations, sigma deviations), the
               two tracking errors (estimate at a tick, true state at every step) and the estimation error of the metrics
  sat_margin   the smallest |u_raw - limit| over channels, finite limits and ticks
  pivot_min    the smallest Cholesky pivot seen

Cases (CASES): the smallest shapes that reach every edge.  P in {1, 3} candidates and B in {1, 5} runs (the kernel packs four runs, one
per wave, into a block: B = 5 is a full block and a block with one live wave); T in {7, 12} and hold in {1, 3}, so that T is no multiple
of hold; both models, both integrators, both lag modes, with and without the lag banks; nplant, nfb and nrec each 1 and P; with and
without W and u_ff; a set-point and a moving reference.  In every case V is NaN in about 20 % of its entries and component 7 is
never measured (r = +inf while its V column carries numbers).  In the runs with an even index the reference yaw is a ramp through pi,
given wrapped to [-pi, pi], and the true yaw starts next to it; run 1 starts its ESTIMATE one turn away from the truth (yaw - 2 pi), so
that every wrap of the law -- innovation, tracking error, estimation error -- moves by 2 pi there.  The limits sit in the tails of
the raw commands: some runs saturate (asserted on the reference).

What was chosen for the closed loop's own amplification: T <= 12 and the gains of tests/sweep_run.py: gains (dense, 0.3 of a
channel per unit error).  With them the float64-to-long-double gap of the reference stays below a tenth of TOL_ROLL (at most 4.7e-13)
on every lane of every case, so all are compared (tests/test_output_feedback_cpu.py asserts the share); nothing had to be shortened
or weakened."""
import functools

import numpy as np

import feedback_ref as fr
import fossen_vehicles as fv
import ukf_ref as ur
from oracle import fossen_params as fp

L = np.longdouble
N = 12
DT = 0.02
TOL_ROLL, TOL_UPDATE, MARGIN = 1e-10, 1e-12, 1e-6      # tests/sweep_run.py
SIGMA = np.array([0.02] * 3 + [0.01] * 3 + [0.03] * 3 + [0.02] * 3)
UNMEASURED = 7
INTEG = {"euler": fp.EULER, "rk4": fp.RK4}
MODELS = ("V0", "V5", "V2")             # the filter models of the candidates
PLANTS = ("V5", "V1", "V4")             # the plants (nplant = 1: the first)
SEED = 9100


# ------------------------------------------------------------------------------------------ the law
def loop_one(cm, cp, model, integ, lag_mode, dt, law, k, x0_true, x0_est, P0, V, W, u_ff, ref, lag_est, lag_plant, z, dtype):
    """one (candidate, run): cm / cp the prepared filter model / plant, law a feedback_ref.Law, k a ukf_ref.Cfg"""
    T, nu = V.shape[0], fp.NU[model]
    w = ur.weights(k, dtype)
    q, r = np.asarray(k.q, dtype=dtype), np.asarray(k.r, dtype=dtype)
    K, Ki = law.K.astype(dtype), law.Ki.astype(dtype)
    lo, hi, zm = law.u_min.astype(dtype), law.u_max.astype(dtype), law.z_max.astype(dtype)
    h = dtype(dt)
    xt = np.asarray(x0_true, dtype=dtype).copy()
    x = np.asarray(x0_est, dtype=dtype).copy()
    Pm = np.tril(np.asarray(P0, dtype=dtype))
    Pm = Pm + np.tril(Pm, -1).T
    le0, lp0, z0 = lag_est, lag_plant, z
    le, lp, z = lag_est, lag_plant, np.asarray(z, dtype=dtype).copy()
    ref = np.asarray(ref, dtype=dtype)
    nan = lambda *s: np.full(s, np.nan, dtype=dtype)
    traj, y_out, us = nan(T + 1, N), nan(T, N), nan(T, nu)
    xf, pstd, innov = nan(T, N), nan(T, N), nan(T, N)
    traj[0] = xt
    m = np.zeros(7, dtype=dtype)
    ell, nupd, failed, pivmin, wrap_margin, sat_margin = dtype(0), 0, -1, np.inf, np.inf, np.inf
    u = np.zeros(nu, dtype=dtype)
    for t in range(T):
        # 1. measure
        y = xt + np.asarray(V[t], dtype=dtype)
        y_out[t] = y
        # 2. update
        x, Pm, inn, dl, napp, mg, _, bad = ur.update_row(x, Pm, y, r, dtype)
        nupd, wrap_margin, ell = nupd + napp, min(wrap_margin, mg), ell + dl
        if bad:
            failed = t
            break
        xf[t], innov[t] = x, inn
        with np.errstate(invalid="ignore"):
            pstd[t] = np.sqrt(np.diagonal(Pm))
        # 3. command, from the estimate
        rr = ref[t if ref.shape[0] > 1 else 0]
        if t % law.hold == 0:
            e, mg = fr.error_lanes(model, x[None], rr[None], dtype)
            e, wrap_margin = e[0], min(wrap_margin, float(mg[0]))
            raw = np.zeros(nu, dtype=dtype) if u_ff is None else np.asarray(u_ff[t], dtype=dtype).copy()
            for j in range(12):
                raw = raw + K[:, j] * e[j]
            for j in range(6):
                raw = raw + Ki[:, j] * z[j]
            for lim in (lo, hi):
                fin = np.isfinite(lim)
                if fin.any():
                    sat_margin = min(sat_margin, float(np.min(np.abs(raw[fin] - lim[fin]))))
            u = np.minimum(np.maximum(raw, lo), hi)
            z = np.minimum(np.maximum(z + (dtype(law.hold) * h) * e[0:6], -zm), zm)
        us[t] = u
        # the metrics: on the true state at the start of the step, and the estimation error
        e, mg = fr.error_lanes(model, xt[None], rr[None], dtype)
        e, wrap_margin = e[0], min(wrap_margin, float(mg[0]))
        d = x - xt
        wr, mg = ur._wrap(d[3:6], dtype)
        wrap_margin = min(wrap_margin, float(np.min(mg)))
        m[0] += h * np.sum(e[0:3] ** 2)
        m[1] += h * np.sum(e[3:6] ** 2)
        m[2] += h * np.sum(u ** 2)
        m[3] += float(np.any((u == lo) | (u == hi)))
        m[4] += h * np.sum(d[0:3] ** 2)
        m[5] += h * np.sum(wr ** 2)
        m[6] += h * np.sum(d[6:12] ** 2)
        # 4. plant
        xn, lpn = fp._step(cp, model, integ, lag_mode, dt, xt[None], u[None], lp[None])
        xt, lp = xn[0], lpn[0]
        if W is not None:
            xt = xt + np.asarray(W[t], dtype=dtype)
        traj[t + 1] = xt
        # 5. predict
        x, Pm, le, piv, mg, bad = ur.predict(cm, model, integ, lag_mode, dt, x, Pm, u, le, w, q, dtype)
        pivmin = min([pivmin] + [float(v) for v in piv])
        wrap_margin = min(wrap_margin, mg)
        if bad:
            failed = t
            break
    if failed >= 0:
        xt, x, Pm, m = nan(N), nan(N), nan(N, N), nan(7)
        ell, le, lp, z = dtype(-np.inf), le0, lp0, np.asarray(z0, dtype=dtype)
    return dict(traj=traj, y=y_out, u=us, xf=xf, pstd=pstd, innov=innov, xT_true=xt, xT=x, PT=Pm, metrics=m,
                info=np.array([ell, nupd, failed, pivmin], dtype=dtype), lag_est=le, lag_plant=lp, z=z,
                wrap_margin=wrap_margin, sat_margin=sat_margin, pivot_min=pivmin)


KEYS = ("traj", "y", "u", "xf", "pstd", "innov", "xT_true", "xT", "PT", "metrics", "info", "lag_est", "lag_plant", "z", "wrap_margin",
        "sat_margin", "pivot_min")


def loop(model, integ, lag_mode, vehicles, plants, laws, cfgs, x0_true, x0_est, P0, V, ref, dt, W=None, u_ff=None, lag_est=None,
         lag_plant=None, z=None, dtype=np.float64):
    """brov_output_feedback: vehicles [P] and plants [1 or P] (oracle Vehicles), laws [1 or P] (feedback_ref.Law), cfgs [1 or P]
    (ukf_ref.Cfg); the arrays of the header, lag_est / lag_plant [P,B,8,3] or None, z [P,B,6] or None.  Returns the outputs stacked
    to [P,B,...] (the lag banks always, zeros-started when None was given) and the margins [P,B]."""
    assert model in (fp.THRUSTER_EULER, fp.WRENCH_EULER)
    P, B = len(vehicles), np.asarray(V).shape[0]
    pick = lambda seq, j: seq[j if len(seq) > 1 else 0]
    out = {k: [] for k in KEYS}
    for j in range(P):
        cm, cp = fp._Prep(vehicles[j], dt, dtype), fp._Prep(pick(plants, j), dt, dtype)
        rows = []
        for b in range(B):
            bank = lambda a: np.zeros((8, 3), dtype=dtype) if a is None else np.asarray(a, dtype=dtype).reshape(P, B, 8, 3)[j, b]
            zz = np.zeros(6, dtype=dtype) if z is None else np.asarray(z, dtype=dtype).reshape(P, B, 6)[j, b]
            rows.append(loop_one(cm, cp, model, integ, lag_mode, dt, pick(laws, j), pick(cfgs, j), x0_true[b], x0_est[b], P0[b], V[b],
                                 None if W is None else W[b], None if u_ff is None else u_ff[b], ref[b], bank(lag_est), bank(lag_plant), zz,
                                 dtype))
        for k in KEYS:
            out[k].append(np.stack([np.asarray(r[k]) for r in rows]))
    return {k: np.stack(v) for k, v in out.items()}


# ------------------------------------------------------------------------------------------ the cases
# name -> model, integrator, lag mode, lag banks, P, B, T, hold, nplant = P, nfb = P, nrec = P, W, u_ff, moving reference, start z
CASES = {
    "thr_rk4": (0, "rk4", 0, True, 3, 5, 12, 3, True, False, False, False, True, True, True),
    "thr_rk4_lagstep": (0, "rk4", 1, True, 3, 5, 7, 3, False, True, True, True, False, True, True),
    "thr_euler_nobank": (0, "euler", 0, False, 1, 1, 12, 1, False, False, False, False, True, False, False),
    "thr_rk4_nobank": (0, "rk4", 0, False, 3, 1, 7, 3, True, False, True, False, False, True, True),
    "wr_rk4": (1, "rk4", 0, False, 3, 5, 12, 3, False, True, False, True, True, True, True),
    "wr_euler": (1, "euler", 0, False, 1, 5, 7, 1, True, False, False, False, False, True, False),
}
FIELDS = ("model", "integ", "lag_mode", "banks", "P", "B", "T", "hold", "plant_P", "fb_P", "rec_P", "W", "u_ff", "moving", "z")


def case(name):
    return dict(zip(FIELDS, CASES[name]))


def chan_scale(model):
    """size of a command channel: thruster commands ~1, forces ~10 N, moments ~0.5 N m"""
    return np.ones(8) if model == 0 else np.array([10.0, 10.0, 10.0, 0.5, 0.5, 0.5])


def gains(rng, model, hold):
    """tests/sweep_run.py: gains at T <= 24 -- random dense gains, limits in the tails of the raw commands, an integral clamp that part
    of the integral states reach"""
    nu, s = fp.NU[model], chan_scale(model)
    return fr.law(nu, K=rng.uniform(-1, 1, (nu, 12)) * 0.3 * s[:, None], Ki=rng.uniform(-1, 1, (nu, 6)) * 1.0 * s[:, None],
                  u_min=-np.linspace(1.0, 0.6, nu) * s, u_max=np.linspace(0.6, 1.0, nu) * s, z_max=np.linspace(0.01, 0.03, 6), hold=hold)


def noise_cfg(alpha, scale=1.0):
    r = (SIGMA * scale) ** 2
    r[UNMEASURED] = np.inf
    return ur.cfg(q=1e-6 * np.linspace(1.0, 3.0, 12), r=r, alpha=alpha, beta=2.0, kappa=1.0)


def wrap_pi(a):
    return a - 2 * np.pi * np.rint(a / (2 * np.pi))


@functools.lru_cache(maxsize=None)
def inputs(name):
    """the arrays of a case (seeded by its name): dict(c, models, plants, laws, cfgs, x0_true, x0_est, P0, V, W, u_ff, ref, lag_est,
    lag_plant, z)"""
    c = case(name)
    rng = np.random.default_rng(SEED + sorted(CASES).index(name))
    model, P, B, T = c["model"], c["P"], c["B"], c["T"]
    nu = fp.NU[model]
    x0_true = rng.uniform(-0.3, 0.3, (B, 12))
    ref = rng.uniform(-0.3, 0.3, (B, T if c["moving"] else 1, 12))
    if c["moving"]:
        for b in range(0, B, 2):            # a yaw ramp through pi, given wrapped; the vehicle starts next to it
            ref[b, :, 5] = wrap_pi(np.linspace(3.05, 3.25, T))
            x0_true[b, 5] = 3.0
    x0_est = x0_true + rng.normal(size=(B, 12)) * SIGMA
    if B > 1:
        x0_est[1, 5] -= 2 * np.pi           # an estimate one turn away from the truth
    d = np.sqrt(4.0 * SIGMA ** 2)
    M = rng.normal(size=(B, 12, 12))
    C = 0.7 * np.eye(12) + 0.3 * (M @ M.transpose(0, 2, 1)) / 12.0
    P0 = d[None, :, None] * C * d[None, None, :]
    P0 = 0.5 * (P0 + P0.transpose(0, 2, 1))
    P0[:, np.triu_indices(12, 1)[0], np.triu_indices(12, 1)[1]] = np.nan          # only the lower triangle may be read
    V = rng.normal(size=(B, T, 12)) * SIGMA
    V[rng.uniform(size=V.shape) < 0.2] = np.nan
    V[:, :, UNMEASURED] = 5.0               # numbers the filter must not look at
    W = rng.normal(size=(B, T, 12)) * 1e-3 * SIGMA if c["W"] else None
    u_ff = rng.uniform(-0.2, 0.2, (B, T, nu)) * chan_scale(model) if c["u_ff"] else None
    banks = c["banks"] and model == 0
    lag_est = rng.uniform(-1, 1, (P, B, 8, 3)) if banks else None
    lag_plant = rng.uniform(-1, 1, (P, B, 8, 3)) if banks else None
    z = rng.uniform(-0.01, 0.01, (P, B, 6)) if c["z"] else None
    laws = [gains(rng, model, c["hold"]) for _ in range(P if c["fb_P"] else 1)]
    cfgs = [noise_cfg((1.0, 0.5)[j % 2], scale=1.0 + 0.5 * j) for j in range(P if c["rec_P"] else 1)]
    return dict(c=c, models=MODELS[:P], plants=PLANTS[:P] if c["plant_P"] else PLANTS[:1], laws=laws, cfgs=cfgs, x0_true=x0_true,
                x0_est=x0_est, P0=P0, V=V, W=W, u_ff=u_ff, ref=ref, lag_est=lag_est, lag_plant=lag_plant, z=z)


def run_reference(i, dtype=np.float64, **kw):
    """loop() on the arrays of a case, with overrides"""
    c = i["c"]
    a = {k: i[k] for k in ("x0_true", "x0_est", "P0", "V", "ref", "W", "u_ff", "lag_est", "lag_plant", "z")}
    a.update(kw)
    return loop(c["model"], INTEG[c["integ"]], c["lag_mode"], [fv.vehicle(n) for n in i["models"]], [fv.vehicle(n) for n in i["plants"]],
                i["laws"], i["cfgs"], a["x0_true"], a["x0_est"], a["P0"], a["V"], a["ref"], DT, W=a["W"], u_ff=a["u_ff"],
                lag_est=a["lag_est"], lag_plant=a["lag_plant"], z=a["z"], dtype=dtype)


@functools.lru_cache(maxsize=None)
def reference(name, ld=False):
    return run_reference(inputs(name), L if ld else np.float64)


# ------------------------------------------------------------------------------------------ the measures
PARITY = ("traj", "y", "u", "xf", "pstd", "innov", "xT_true", "xT", "lag_est", "lag_plant", "z")
METRIC_SUMS = (0, 1, 2, 4, 5, 6)


def lane_err(a, b):
    """max |a-b| / max(1, |b|) per (candidate, run) over the entries where b is a number, formed in long double; inf where the NaN
    patterns differ"""
    a, b = np.asarray(a, dtype=L), np.asarray(b, dtype=L)
    assert a.shape == b.shape, (a.shape, b.shape)
    P, B = a.shape[:2]
    a, b = a.reshape(P, B, -1), b.reshape(P, B, -1)
    same = np.all(np.isnan(a) == np.isnan(b), axis=2)
    with np.errstate(invalid="ignore"):
        rel = np.abs(a - b) / np.maximum(L(1), np.abs(b))
    rel = np.where(np.isnan(b) | (np.isinf(b) & (a == b)), L(0), rel)
    return np.where(same, np.max(rel, axis=2), np.inf).astype(np.float64)


def cov_lane_err(a, b):
    """max |a_ij - b_ij| / sqrt(b_ii b_jj) per (candidate, run) over [P,B,12,12], formed in long double"""
    a, b = np.asarray(a, dtype=L), np.asarray(b, dtype=L)
    dg = np.sqrt(np.diagonal(b, axis1=-2, axis2=-1))
    rel = np.abs(a - b) / (dg[..., :, None] * dg[..., None, :])
    return np.max(rel.reshape(rel.shape[0], rel.shape[1], -1), axis=2).astype(np.float64)


def lane_gaps(o, ol):
    """the error of o against ol per (candidate, run): the worst of the parity outputs, the metric sums, the log-likelihood and the
    smallest pivot, and the covariance measure for PT"""
    g = np.zeros(np.asarray(o["info"]).shape[:2])
    for k in PARITY:
        g = np.maximum(g, lane_err(o[k], ol[k]))
    g = np.maximum(g, lane_err(np.asarray(o["metrics"])[..., METRIC_SUMS], np.asarray(ol["metrics"])[..., METRIC_SUMS]))
    g = np.maximum(g, lane_err(np.asarray(o["info"])[..., [0, 3]], np.asarray(ol["info"])[..., [0, 3]]))
    return np.maximum(g, cov_lane_err(o["PT"], ol["PT"]))


@functools.lru_cache(maxsize=None)
def compared(name):
    """(keep [P,B], gaps [P,B]): the lane rule of tests/sweep_run.py on the reference alone -- a lane is compared if its own
    float64-to-long-double gap is below a tenth of TOL_ROLL, its wrap and saturation margins exceed MARGIN in both precisions and
    both count the same saturated steps and the same scalar updates"""
    o, ol = reference(name), reference(name, ld=True)
    gaps = lane_gaps(o, ol)
    keep = gaps < 0.1 * TOL_ROLL
    for r in (o, ol):
        keep &= (np.asarray(r["wrap_margin"], dtype=np.float64) > MARGIN) & (np.asarray(r["sat_margin"], dtype=np.float64) > MARGIN)
    keep &= o["metrics"][..., 3] == ol["metrics"][..., 3].astype(np.float64)
    keep &= np.all(o["info"][..., 1:3] == ol["info"][..., 1:3].astype(np.float64), axis=-1)
    return keep, gaps
