"""What the shape sweeps do with a case of tests/sweep_cases.py.  Not collected.

Per family:
  prepare(case)                  the case's arrays (seeded by the case), the reference in float64 and in np.longdouble, and from the two
                                 a mask of the lanes (trajectories, samples, windows) that are compared.  CPU only.
  well_posed(case, ref)          the conditions on the reference alone: at most 2 % of the lanes left out, never all of them, a
                                 single lane kept.  tests/test_sweep_cases_cpu.py asserts them for every case without a GPU.
  run(eng, ctx, case, ref)       the engine call(s)
  compare(case, ref, got)        the assertions; returns the worst kernel error over the compared lanes

The recipe is that of the families' own test files: the mixed error max |a-b| / max(1,|b|) formed in long double against
TOL_ROLL = 1e-10; a lane is compared if the reference's own float64-to-long-double gap on it is below a tenth of the bound and
its wrap and saturation margins exceed 1e-6 (conditions on the inputs, not measurements of the kernel).  Counts are exact.  The
soft-min update is checked against a long-double soft-min of the kernel's OWN costs at 1e-12: a fixed-order sum of K <= 513 terms
errs by at most 513 x 2^-53 = 6e-14 of sum |terms|.  Every assertion message carries the case dict.

The EDMDc families (lift, gram, pinv_apply, multistep, simulate) have their prepare / run / compare in tests/sweep_edmdc.py, with
their own measures and bounds (a reference states its own gap condition as ref["gap_bound"]); PREPARE and sweep_one here cover them.
So do the unscented Kalman filter (ukf) and the QP of the Koopman linear MPC (lmpc) in tests/sweep_ukf_lmpc.py, by the recipe above:
a lane is a (candidate, recording) filter or a problem.  The k-means families (colstats, kmeanspp, lloyd) are in tests/sweep_kmeans.py:
their references are exact (indices, labels and centres bit for bit), a reference asserts in prepare that every decision it takes
is certified, no lane is left out, and the fourth figure of sweep_one is the smallest decision gap instead of a reference gap.  The
unscented RTS smoother (smooth) is in tests/sweep_smooth.py, by the recipe above with the covariance measures of
tests/ukf_smooth_cases.py: a lane is a (candidate, recording) problem, every case runs as two calls, as one call and chunked.  The
filter and the smoother of the quaternion model (ukf_quat, smooth_quat) are in tests/sweep_quat.py, in the same shape, with the
references of tests/ukf_quat_ref.py and tests/ukf_quat_smooth_ref.py and |e_w| > 0.5 in place of the wrap margin."""
import numpy as np

import feedback_ref as fr
import fossen_vehicles as fv
import koopman_mppi_ref as kr
import mppi_ref as mr
import sweep_edmdc as se
import sweep_kmeans as sk
import sweep_quat as sq
import sweep_smooth as ss
import sweep_ukf_lmpc as su
from oracle import fossen_params as fp

TOL_ROLL = 1e-10
TOL_UPDATE = 1e-12
TOL_FD = 1e-13                            # tests/test_identify_gpu.py: test_fd_normal_equations_against_longdouble
MARGIN = 1e-6
CAP = 0.02                                # the largest share of a case's lanes that may be left out
L = np.longdouble
DT, DT_KOOPMAN = 0.02, 0.05
INTEG = {"euler": fp.EULER, "rk4": fp.RK4}


def chan_scale(model):
    """size of a command channel: thruster commands ~1, forces ~10 N, moments ~0.5 N m"""
    return np.ones(8) if model == 0 else np.array([10.0, 10.0, 10.0, 0.5, 0.5, 0.5])


def lane_err(a, b):
    """max |a-b| / max(1, |b|) over everything but the leading axis, formed in long double: one figure per lane"""
    a, b = np.asarray(a, dtype=L), np.asarray(b, dtype=L)
    assert a.shape == b.shape, (a.shape, b.shape)
    n = a.shape[0]
    if a.size == 0:
        return np.zeros(n)
    return np.max((np.abs(a - b) / np.maximum(L(1), np.abs(b))).reshape(n, -1), axis=1).astype(np.float64)


def err(a, b):
    e = lane_err(np.asarray(a)[None], np.asarray(b)[None])
    return float(e[0])


def _unit(q):
    return q / np.linalg.norm(q, axis=-1, keepdims=True)


def _states(rng, model, shape):
    """states in +-0.5, unit quaternions for model 2"""
    x = rng.uniform(-0.5, 0.5, shape + (fp.NX[model],))
    if model == 2:
        x[..., 3:7] = _unit(x[..., 3:7])
    return x


def well_posed(case, ref):
    keep = ref["keep"]
    out = int(keep.size - keep.sum())
    assert keep.size > 0 and keep.any(), ("no lane left to compare", case)
    assert out <= CAP * keep.size, (f"{out} of {keep.size} lanes left out: inputs too hard for fp64", ref["gap_all"], case)
    assert ref["gap"] < ref.get("gap_bound", 0.1 * TOL_ROLL), ("reference gap on the compared lanes", ref["gap"], case)
    return out


def _finish(ref, gaps, margins=None):
    """keep mask and the gap figures from per-lane gaps (and margins) of any shape"""
    gaps = np.asarray(gaps, dtype=np.float64)
    keep = gaps < 0.1 * TOL_ROLL
    if margins is not None:
        keep &= np.asarray(margins, dtype=np.float64) > MARGIN
    ref.update(keep=keep, gap=float(gaps[keep].max()) if keep.any() else np.inf, gap_all=float(gaps.max()) if gaps.size else 0.0)
    return ref


def _worst(case, what, e, keep):
    """assert the per-lane errors of one output on the compared lanes"""
    e = np.asarray(e)
    assert e.shape == keep.shape, (what, e.shape, keep.shape, case)
    w = float(e[keep].max()) if keep.any() else 0.0
    assert np.isfinite(w) and w < TOL_ROLL, (what, w, "worst lane", int(np.argmax(np.where(keep, e, -1.0))), case)
    return w


# ------------------------------------------------------------------------------------------ population rollouts
def prepare_rollout_pop(case):
    """x0 in +-0.5, commands uniform in +- chan_scale (a new command every step), start lag in +-1; per candidate: its own draw"""
    c, rng = case, np.random.default_rng(case["seed"])
    model, P, B, T = c["model"], c["P"], c["B"], c["T"]
    lead = (P,) if c["per_candidate"] else ()
    x0 = _states(rng, model, lead + (B,))
    U = rng.uniform(-1, 1, lead + (B, T, fp.NU[model])) * chan_scale(model)
    lag = rng.uniform(-1, 1, (P, B, 8, 3)) if c["lag"] else None
    ref = dict(x0=x0, U=U, lag=lag, o=[], ol=[])
    gaps = np.zeros((P, B))
    for j, name in enumerate(c["names"]):
        xj, Uj = (x0[j], U[j]) if c["per_candidate"] else (x0, U)
        for key, dtype in (("o", np.float64), ("ol", L)):
            ref[key].append(fp.rollout(model, INTEG[c["integ"]], c["lag_mode"], fv.vehicle(name), xj, Uj, DT, lag=None if lag is None else lag[j],
                                       sub=c["stride"], dtype=dtype))
        for k in _pop_keys(c):
            gaps[j] = np.maximum(gaps[j], lane_err(ref["o"][j][k], ref["ol"][j][k]))
    return _finish(ref, gaps)


def _pop_keys(c):
    return (("traj",) if c["store"] else ()) + ("xT",) + (("lag",) if c["lag"] else ())


def run_rollout_pop(eng, ctx, case, ref, **kw):
    c = case
    args = dict(lag=ref["lag"], lag_mode=c["lag_mode"], stride=c["stride"], store=c["store"], per_candidate=c["per_candidate"], ctx=ctx)
    args.update(kw)
    return eng.rollout_pop(c["model"], c["integ"], [fv.params(n) for n in c["names"]], ref["x0"], ref["U"], DT, **args)


def compare_rollout_pop(case, ref, got):
    c = case
    assert (got["traj"] is None) == (not c["store"]) and (got["lag"] is None) == (not c["lag"]), case
    worst = 0.0
    for k in _pop_keys(c):
        assert got[k].shape == (c["P"],) + ref["o"][0][k].shape, (k, got[k].shape, case)
        e = np.stack([lane_err(got[k][j], ref["o"][j][k]) for j in range(c["P"])])
        worst = max(worst, _worst(case, "rollout_pop " + k, e, ref["keep"]))
    return worst


# ------------------------------------------------------------------------------------------ closed-loop rollouts
def gains(rng, model, hold, T):
    """tests/test_feedback_gpu.py: gains -- random dense gains, limits in the tails of the raw commands, an integral clamp that part
    of the integral states reach.  That recipe is for T = 24; random dense gains do not stabilise the vehicle, and beyond it the
    float64-to-long-double gap of some trajectories grows past the bound (13 of 514 at T = 130), so the gains shrink as 24 / T."""
    nu, s = fp.NU[model], chan_scale(model) * min(1.0, 24.0 / max(T, 1))
    return fr.law(nu, K=rng.uniform(-1, 1, (nu, 12)) * 0.3 * s[:, None], Ki=rng.uniform(-1, 1, (nu, 6)) * 1.0 * s[:, None],
                  u_min=-np.linspace(1.0, 0.6, nu) * chan_scale(model), u_max=np.linspace(0.6, 1.0, nu) * chan_scale(model),
                  z_max=np.linspace(0.01, 0.03, 6), hold=hold)


def _fb_keys(c):
    return (("traj",) if c["store"] else ()) + ("xT",) + (("lag",) if c["lag"] else ()) + (("z",) if c["z"] else ()) + ("u", "metrics")


def prepare_feedback(case):
    """tests/test_feedback_gpu.py: inputs -- shared scenarios: x0 and reference in +-0.5, u_ff 0.2 chan_scale, start lag +-1, z +-0.01"""
    c, rng = case, np.random.default_rng(case["seed"])
    model, P, B, T = c["model"], c["P"], c["B"], c["T"]
    nu = fp.NU[model]
    x0 = _states(rng, model, (B,))
    REF = _states(rng, model, (B, 1 if c["ref"] == "set" else T))
    u_ff = rng.uniform(-0.2, 0.2, (B, T, nu)) * chan_scale(model) if c["u_ff"] else None
    lag = rng.uniform(-1, 1, (B, 8, 3)) if c["lag"] else None
    z = rng.uniform(-0.01, 0.01, (B, 6)) if c["z"] else None
    laws = [gains(rng, model, c["hold"], T) for _ in range(P if c["gain_sets"] else 1)]
    ref = dict(x0=x0, REF=REF, u_ff=u_ff, lag=lag, z=z, laws=laws, o=[], ol=[])
    gaps, margins = np.zeros((P, B)), np.full((P, B), np.inf)
    for j, name in enumerate(c["names"]):
        for key, dtype in (("o", np.float64), ("ol", L)):
            o = fr.rollout(model, INTEG[c["integ"]], c["lag_mode"], fv.vehicle(name), laws[j if c["gain_sets"] else 0], x0, REF, DT, T=T,
                           u_ff=u_ff, lag=lag, z=z, sub=c["stride"], dtype=dtype)
            ref[key].append(o)
            margins[j] = np.minimum(margins[j], np.minimum(o["wrap_margin_lane"], o["sat_margin_lane"]).astype(np.float64))
        o, ol = ref["o"][j], ref["ol"][j]
        for k in _fb_keys(c):
            gaps[j] = np.maximum(gaps[j], lane_err(o[k][:, :3] if k == "metrics" else o[k], ol[k][:, :3] if k == "metrics" else ol[k]))
        # a saturated-step count on which float64 and long double differ is a lane on a branch
        margins[j] = np.where(o["metrics"][:, 3] == ol["metrics"][:, 3].astype(np.float64), margins[j], 0.0)
    return _finish(ref, gaps, margins)


def run_feedback(eng, ctx, case, ref, **kw):
    c, P = case, case["P"]
    bc = lambda a: None if a is None else np.broadcast_to(a, (P,) + a.shape)
    fbs = [fr.to_struct(l) for l in ref["laws"]]
    args = dict(T=c["T"], u_ff=ref["u_ff"], lag=bc(ref["lag"]), z=bc(ref["z"]), lag_mode=c["lag_mode"], stride=c["stride"], store=c["store"],
                want_u=True, ctx=ctx)
    args.update(kw)
    return eng.rollout_feedback(c["model"], c["integ"], [fv.params(n) for n in c["names"]], fbs if c["gain_sets"] else fbs[0], ref["x0"],
                                ref["REF"], DT, **args)


def compare_feedback(case, ref, got):
    c, P, keep = case, case["P"], ref["keep"]
    assert (got["traj"] is None) == (not c["store"]) and (got["lag"] is None) == (not c["lag"]) and (got["z"] is None) == (not c["z"]), case
    worst = 0.0
    for k in _fb_keys(c):
        assert got[k].shape == (P,) + ref["o"][0][k].shape, (k, got[k].shape, case)
        cut = (lambda a: a[:, :3]) if k == "metrics" else (lambda a: a)
        e = np.stack([lane_err(cut(got[k][j]), cut(ref["o"][j][k])) for j in range(P)])
        worst = max(worst, _worst(case, "feedback " + k, e, keep))
    count = np.stack([o["metrics"][:, 3] for o in ref["o"]])
    assert np.array_equal(got["metrics"][..., 3][keep], count[keep]), ("saturated-step count", case)
    return worst


# ------------------------------------------------------------------------------------------ MPPI: what both planning models share
def _record(rng, nu, s, hold, sigma0):
    """tests/test_mppi_gpu.py: record -- random weights; sigma 0.2 s with one channel unperturbed; per-channel limits 0.5 .. 0.8 s, in
    the tails of the sample commands.  lam = 1; with_lam() gives the same record at another temperature."""
    sigma = 0.2 * s
    sigma[sigma0] = 0.0
    q, qf, r = rng.uniform(0.5, 2.0, 12), rng.uniform(2.0, 8.0, 12), rng.uniform(0.05, 0.2, nu) / (s * s)
    return dict(q=q, qf=qf, r=r, sigma=sigma, u_min=-np.linspace(0.8, 0.5, nu) * s, u_max=np.linspace(0.5, 0.8, nu) * s, hold=hold)


def with_lam(ref, lam, gamma=None):
    return mr.cfg(ref["nu"], lam=lam, gamma=gamma, **ref["record"])


def spread_lambda(S):
    """a tenth of the reference's cost spread (the smallest over the problems); 1 where there is none (K = 1)"""
    spread = float(np.min(S.max(axis=1) - S.min(axis=1)))
    return spread / 10.0 if spread > 0 else 1.0


def _finish_mppi(ref, keys):
    o, ol = ref["o"], ref["ol"]
    gaps = np.zeros(o["cost"].shape)
    for k in keys:
        B, K = o[k].shape[:2]
        gaps = np.maximum(gaps, lane_err(o[k].reshape((B * K,) + o[k].shape[2:]), ol[k].reshape((B * K,) + o[k].shape[2:])).reshape(B, K))
    ref["lam_update"] = spread_lambda(o["cost"])
    return _finish(ref, gaps, np.minimum(o["wrap_margin_lane"], ol["wrap_margin_lane"]).astype(np.float64))


def _compare_mppi(case, ref, got, upd, keys, what):
    """costs (and predictions) of the lam = 1 run per sample; the update of the lam_update run from the kernel's own costs"""
    c, keep, o = case, ref["keep"], ref["o"]
    B, K, hold = c["B"], c["K"], c["hold"]
    worst = 0.0
    for k in keys:
        assert got[k].shape == o[k].shape and np.all(np.isfinite(got[k])), (k, got[k].shape, case)
        e = lane_err(got[k].reshape((B * K,) + o[k].shape[2:]), o[k].reshape((B * K,) + o[k].shape[2:])).reshape(B, K)
        worst = max(worst, _worst(case, what + " " + k, e, keep))
    cfg = with_lam(ref, ref["lam_update"], ref.get("gamma"))
    assert upd["U_nom"].shape == ref["U"].shape and upd["u_apply"].shape == (B, hold, ref["nu"]) and upd["info"].shape == (B, 4), case
    e_up = 0.0
    for b in range(B):
        Un, info, _ = mr.softmin(cfg, upd["cost"][b], ref["ol"]["delta"][b], ref["U"][b], dtype=L)
        plan = np.concatenate([Un[1:], Un[-1:]], axis=0) if c["shift"] else Un
        e_up = max(e_up, err(upd["U_nom"][b], plan), err(upd["u_apply"][b], np.repeat(Un[:1], hold, axis=0)), err(upd["info"][b, 2], info[2]))
        assert upd["info"][b, 0] == upd["cost"][b, 0] and upd["info"][b, 1] == upd["cost"][b].min() and upd["info"][b, 3] == 0, \
            ("S_0, beta and the non-finite count are exact", b, upd["info"][b], case)
    assert e_up < TOL_UPDATE, (what + " update from the kernel's own costs", e_up, case)
    return worst, e_up


# ------------------------------------------------------------------------------------------ MPPI with the Fossen model
def prepare_mppi(case):
    """tests/test_mppi_gpu.py: inputs -- x and reference rows in +-0.5, knots 0.3 chan_scale, a start lag for the thruster model"""
    c, rng = case, np.random.default_rng(case["seed"])
    model, B, K, H, M = c["model"], c["B"], c["K"], c["H"], c["M"]
    nu, s = fp.NU[model], chan_scale(model)
    x, REF = _states(rng, model, (B,)), _states(rng, model, (B, c["rows"]))
    U = rng.uniform(-0.3, 0.3, (B, M, nu)) * s
    lag = rng.uniform(-1, 1, (B, 8, 3)) if model == 0 else None
    eps = rng.normal(size=(B, K, M, nu)) if c["eps"] else None
    ref = dict(x=x, REF=REF, U=U, lag=lag, eps=eps, nu=nu, record=_record(rng, nu, s, c["hold"], c["sigma0"]))
    veh = [fv.vehicle(n) for n in c["names"]]
    for key, dtype in (("o", np.float64), ("ol", L)):
        ref[key] = mr.step(model, INTEG[c["integ"]], c["lag_mode"], veh, with_lam(ref, 1.0), x, REF, U, DT, K, H, lag=lag, seed=c["stream_seed"],
                           eps=eps, ref_row0=c["row0"], shift=c["shift"], dtype=dtype)
    return _finish_mppi(ref, ("cost",))


def run_mppi(eng, ctx, case, ref, lam=1.0, **kw):
    c = case
    args = dict(H=c["H"], lag=ref["lag"], lag_mode=c["lag_mode"], seed=c["stream_seed"], eps=ref["eps"], ref_row0=c["row0"], shift=c["shift"],
                want_cost=True, ctx=ctx)
    args.update(kw)
    return eng.mppi_step(c["model"], c["integ"], [fv.params(n) for n in c["names"]], mr.to_struct(with_lam(ref, lam)), ref["x"], ref["REF"],
                         ref["U"], DT, c["K"], **args)


def compare_mppi(case, ref, got, upd):
    return _compare_mppi(case, ref, got, upd, ("cost",), "mppi")


# ------------------------------------------------------------------------------------------ MPPI with a Koopman model
def koopman_model(rng, n, r, k):
    """tests/test_koopman_mppi_gpu.py: model -- A = 0.98 A0 / rho(A0) with A0 = I + 0.3 G / sqrt(d), B and the centres of the size of
    the states"""
    d = n + k
    A0 = np.eye(d) + 0.3 * rng.normal(size=(d, d)) / np.sqrt(d)
    A = 0.98 * A0 / np.max(np.abs(np.linalg.eigvals(A0)))
    return (rng.uniform(-0.5, 0.5, (k, n)) if k else None), 0.5, A, 0.1 * rng.normal(size=(d, r))


def prepare_koopman_mppi(case):
    c, rng = case, np.random.default_rng(case["seed"])
    n, r, B, K, H, M = c["n"], c["r"], c["B"], c["K"], c["H"], c["M"]
    em = kr.ERROR_MODEL[n]
    C, gamma, A, Bm = koopman_model(rng, n, r, c["k"])
    x, REF = _states(rng, em, (B,)), _states(rng, em, (B, c["rows"]))
    U = rng.uniform(-0.3, 0.3, (B, M, r))
    eps = rng.normal(size=(B, K, M, r)) if c["eps"] else None
    ref = dict(x=x, REF=REF, U=U, eps=eps, nu=r, gamma=1.0, model=(C, gamma, A, Bm), record=_record(rng, r, np.ones(r), c["hold"], c["sigma0"]))
    for key, dtype in (("o", np.float64), ("ol", L)):
        ref[key] = kr.step(C, gamma, A, Bm, with_lam(ref, 1.0, 1.0), x, REF, U, DT_KOOPMAN, K, H, seed=c["stream_seed"], eps=eps,
                           ref_row0=c["row0"], shift=c["shift"], dtype=dtype)
    return _finish_mppi(ref, ("pred", "cost"))


def run_koopman_mppi(eng, ctx, case, ref, lam=1.0, **kw):
    c = case
    C, gamma, A, Bm = ref["model"]
    args = dict(H=c["H"], seed=c["stream_seed"], eps=ref["eps"], ref_row0=c["row0"], shift=c["shift"], want_cost=True, want_pred=True, ctx=ctx)
    args.update(kw)
    return eng.koopman_mppi_step(C, gamma, A, Bm, mr.to_struct(with_lam(ref, lam, 1.0)), ref["x"], ref["REF"], ref["U"], DT_KOOPMAN, c["K"], **args)


def compare_koopman_mppi(case, ref, got, upd):
    return _compare_mppi(case, ref, got, upd, ("pred", "cost"), "koopman_mppi")


# ------------------------------------------------------------------------------------------ population window evaluator
def window_rows(lens, H):
    """first row of every window, bag after bag"""
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    return off, np.array([a + k for a, b in zip(off[:-1], off[1:]) for k in range(max(int(b - a) - H, 0))], dtype=np.int64)


def prepare_window_pop(case):
    """tests/test_identify_gpu.py: _recording -- unrelated rows: positions +-1, angles and velocities +-0.5, commands +-1 (thrusters)
    or +-20 N / +-2 N m.  short_u: the last row of U, which no window reads, is NaN for the kernel and absent for the oracle."""
    c, rng = case, np.random.default_rng(case["seed"])
    model, P, H = c["model"], c["P"], c["H"]
    N = int(sum(c["lens"]))
    X = np.concatenate([rng.uniform(-1, 1, (N, 3)), _states(rng, model, (N,))[:, 3:]], axis=1)
    U = rng.uniform(-1, 1, (N, 8)) if model == 0 else rng.uniform(-1, 1, (N, 6)) * np.array([20, 20, 20, 2, 2, 2.0])
    off, rows = window_rows(c["lens"], H)
    W = len(rows)
    assert W == c["nwin"]
    Ugpu = U.copy()
    if c["short_u"]:
        Ugpu[N - 1] = np.nan
    ref = dict(X=X, U=Ugpu, off=off, rows=rows, target=X[rows + H], delta=rng.choice([-1.0, 1.0], P - 1) * rng.uniform(1e-3, 1e-1, P - 1),
               weights=rng.uniform(0.2, 3.0, fp.NX[model]) if rng.integers(0, 2) else None)
    gaps = np.zeros((P, W))
    for key, dtype in (("o", np.float64), ("ol", L)):
        E, se = [], []
        for name in c["names"]:
            parts = [fp.window_endpoints(model, INTEG[c["integ"]], fv.vehicle(name), X[a:b], U[a:b][:int(b - a) - (1 if c["short_u"] and b == N else 0)],
                                         H, DT, carry_lag=c["carry"], dtype=dtype) for a, b in zip(off[:-1], off[1:]) if b - a > H]
            E.append(np.concatenate([p[2] for p in parts]))
            se.append(sum(p[0] for p in parts))
        ref[key] = dict(E=np.stack(E), rmse=np.sqrt(np.array(se, dtype=dtype) / dtype(W * fp.NX[model])))
    for j in range(P):
        gaps[j] = lane_err(ref["o"]["E"][j], ref["ol"]["E"][j])
    return _finish(ref, gaps)


def run_window_pop(eng, ctx, case, ref):
    """(rmse [P], end states [P,W,nx] on the host, (JtJ, Jtr) | None of fd_normal_eq on the device's end states)"""
    c = case
    rmse, E = eng.window_pop(c["model"], c["integ"], [fv.params(n) for n in c["names"]], ref["X"], ref["U"], c["H"], DT, carry_lag=c["carry"],
                             endpoints=True, ctx=ctx, bag_offsets=ref["off"] if c["bags"] else None)
    fd = None
    if c["P"] > 1:
        fd = eng.fd_normal_eq(E, eng.DevArray.from_host(ctx, ref["target"]), ref["delta"], ref["weights"], ctx=ctx)
    return dict(rmse=rmse, E=E.numpy(), fd=fd)


def compare_window_pop(case, ref, got):
    c, keep, o = case, ref["keep"], ref["o"]
    assert got["E"].shape == o["E"].shape and got["rmse"].shape == (c["P"],), (got["E"].shape, case)
    e = np.stack([lane_err(got["E"][j], o["E"][j]) for j in range(c["P"])])
    worst = _worst(case, "window_pop end states", e, keep)
    if keep.all():                   # the total has no lanes to leave out
        worst = max(worst, _worst(case, "window_pop rmse", lane_err(got["rmse"], o["rmse"]), np.ones(c["P"], dtype=bool)))
    e_fd = 0.0
    if got["fd"] is not None:
        JtJ, Jtr = got["fd"]
        m, nx = c["P"] - 1, o["E"].shape[2]
        Eh = got["E"].astype(L)
        wl = np.ones(nx, dtype=L) if ref["weights"] is None else ref["weights"].astype(L)
        J = ((Eh[1:] - Eh[0]) * wl).reshape(m, -1).T / ref["delta"].astype(L)
        r = ((Eh[0] - ref["target"].astype(L)) * wl).reshape(-1)
        mag_JtJ, mag_Jtr = np.abs(J).T @ np.abs(J), np.abs(J).T @ np.abs(r)
        e1 = np.max(np.abs(JtJ.astype(L) - J.T @ J) / (mag_JtJ + L(1e-300)))
        e2 = np.max(np.abs(Jtr.astype(L) - J.T @ r) / (mag_Jtr + L(1e-300)))
        e_fd = float(max(e1, e2))
        assert e_fd <= TOL_FD and np.array_equal(JtJ, JtJ.T), ("fd_normal_eq against long double, |err| / sum |terms|", e_fd, case)
    return worst, e_fd


PREPARE = dict(rollout_pop=prepare_rollout_pop, feedback=prepare_feedback, mppi=prepare_mppi, koopman_mppi=prepare_koopman_mppi,
               window_pop=prepare_window_pop, **se.PREPARE, **su.PREPARE, **sk.PREPARE, **ss.PREPARE, **sq.PREPARE)


def sweep_one(eng, ctx, case, ref=None):
    """one case end to end: (worst kernel error, second figure: update / normal-equation error or 0 -- for the EDMDc families what
    sweep_edmdc.sweep_one says --, lanes left out, reference gap)"""
    fam = case["family"]
    ref = PREPARE[fam](case) if ref is None else ref
    out = well_posed(case, ref)
    if fam in se.PREPARE:
        e, e2 = se.sweep_one(eng, ctx, case, ref)
    elif fam in su.PREPARE:
        e, e2 = su.sweep_one(eng, ctx, case, ref)
    elif fam in ss.PREPARE:
        e, e2 = ss.sweep_one(eng, ctx, case, ref)
    elif fam in sq.PREPARE:
        e, e2 = sq.sweep_one(eng, ctx, case, ref)
    elif fam in sk.PREPARE:
        e, e2 = sk.sweep_one(eng, ctx, case, ref)
        return e, e2, out, ref["min_gap"]
    elif fam == "rollout_pop":
        e, e2 = compare_rollout_pop(case, ref, run_rollout_pop(eng, ctx, case, ref)), 0.0
    elif fam == "feedback":
        e, e2 = compare_feedback(case, ref, run_feedback(eng, ctx, case, ref)), 0.0
    elif fam == "mppi":
        e, e2 = compare_mppi(case, ref, run_mppi(eng, ctx, case, ref), run_mppi(eng, ctx, case, ref, lam=ref["lam_update"]))
    elif fam == "koopman_mppi":
        e, e2 = compare_koopman_mppi(case, ref, run_koopman_mppi(eng, ctx, case, ref), run_koopman_mppi(eng, ctx, case, ref, lam=ref["lam_update"]))
    else:
        e, e2 = compare_window_pop(case, ref, run_window_pop(eng, ctx, case, ref))
    return e, e2, out, ref["gap"]
