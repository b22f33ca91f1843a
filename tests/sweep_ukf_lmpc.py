"""What the shape sweeps do with a case of the families `ukf` (unscented Kalman filter, csrc/ukf.hip) and `lmpc` (the batched ADMM QP
of the Koopman linear MPC, csrc/koopman_qp.hip) of tests/sweep_cases.py: prepare / run / compare as in tests/sweep_run.py, which
registers them.  Not collected.

ukf.  Inputs by the recipe of tests/ukf_cases.py: inputs -- recordings simulated by the oracle with the last candidate's vehicle,
noise of ukf_cases.SIGMA, a dense positive-definite P0 whose upper triangle is NaN -- with what the case switches: no start lag (the
kernel's TRACK = false form), T down to 1, every entry measured (12 scalar updates per row), none measured (pure prediction: no
update, l = 0, innov all NaN), 0, 1 or 3 components with r = +inf whose Y columns carry numbers, process variances exactly 0, a
noise record per candidate.  The reference is ukf_ref.filter in float64 and in long double.  A lane is one (candidate, recording)
filter; it is compared if its own float64-to-long-double gap (ukf_cases.err per output, ukf_cases.cov_err for PT) is below a tenth of
TOL_ROLL = 1e-10, its wrap margin exceeds 1e-6, its smallest pivot 1e-4 and it did not fail: the conditions of
tests/test_ukf_cpu.py: test_gpu_cases_are_well_posed.  Compared: xf, pstd, innov (same NaN pattern), xT, PT, info[0], info[3] and
lag at 1e-10; info[1:3] exactly; PT bit-symmetric.

lmpc.  Models, records, solvers and inputs by tests/koopman_lmpc_ref.py (synth_model, rec, condense, rho and W as case_solver, the
inputs as case_inputs), the reference is its step() in float64 and long double.  A lane is a problem; it is compared if its gap over
U_nom, y, u_apply, pred and info[:4] is below a tenth of 1e-10 and both precisions count the same iterations and entries at a limit;
a lane of a residual-stop case also needs stop_well_posed in both.  Compared by the recipe of tests/test_koopman_lmpc_gpu.py: check
at its 1e-10; iteration and bound counts exactly; feasibility; u_apply is the first knot in hold rows; J(z) <= J(z0) wherever the
reference shows the descent in both precisions by more than 1e-9.

What the two lists add to the hand-picked shapes of tests/test_ukf_gpu.py and tests/test_koopman_lmpc_gpu.py: the three TRACK = false
instantiations of the thruster filter, full blocks (B = 4, 8), B = 1, P = 1 and 3, T = 1, 2, 3, a noise record per candidate at P = 3,
rows with 12 updates and recordings with none; qp_solve<3> and <4> (129 <= Nv <= 256), the second and third trip of the epilogue
(H + 1 = 64 .. 130) with its per-lane partial sums and the pred rows from 64 on, a second trip of the u_apply loop (hold r > 64), the
scalar tail of the blocked W loop (Nv % 8 != 0) with W from global memory at two to five rows per lane, and the shift and the
residual stop at more than one row per lane."""
import numpy as np

import fossen_vehicles as fv
import koopman_lmpc_ref as lr
import koopman_mppi_ref as kr
import ukf_cases as uc
import ukf_ref as ur
from oracle import fossen_params as fp

L = np.longdouble
TOL_ROLL = 1e-10
MARGIN = 1e-6
PIVOT = 1e-4
DT_UKF, DT_LMPC = uc.DT, lr.DT
INTEG = {"euler": fp.EULER, "rk4": fp.RK4}
UKF_OUTS = ("xf", "pstd", "innov", "xT", "PT", "info")
UKF_NEVER = (7, 2, 4)                      # the components with r = +inf, in the order r_inf takes them
UKF_Q_ZERO = (0, 5, 9)                     # the process variances that q_zero sets to 0
YAW_START, YAW_RATE = 3.13, 0.9            # wrap: the true yaw passes pi within the first step


def _finish(ref, gaps, ok):
    gaps = np.asarray(gaps, dtype=np.float64)
    keep = (gaps < 0.1 * TOL_ROLL) & ok
    ref.update(keep=keep, gap=float(gaps[keep].max()) if keep.any() else np.inf, gap_all=float(gaps.max()) if gaps.size else 0.0)
    return ref


def _worst(case, what, e, keep):
    e = np.asarray(e, dtype=np.float64)
    assert e.shape == keep.shape, (what, e.shape, keep.shape, case)
    w = float(e[keep].max()) if keep.any() else 0.0
    assert np.isfinite(w) and w < TOL_ROLL, (what, w, "worst lane", np.unravel_index(int(np.argmax(np.where(keep, e, -1.0))), e.shape), case)
    return w


# ------------------------------------------------------------------------------------------ unscented Kalman filter
def ukf_cfgs(case):
    """one ukf_ref.Cfg, or one per candidate: the later ones with the other alpha and a larger measurement sigma"""
    def one(alpha, scale):
        k = uc.noise_cfg(alpha, scale)
        r, q = k.r.copy(), k.q.copy()
        r[uc.UNMEASURED] = (uc.SIGMA[uc.UNMEASURED] * scale) ** 2
        r[list(UKF_NEVER[:case["r_inf"]])] = np.inf
        if case["q_zero"]:
            q[list(UKF_Q_ZERO)] = 0.0
        return ur.cfg(q=q, r=r, alpha=alpha, beta=k.beta, kappa=k.kappa)
    a = case["alpha"]
    if case["nrec"] == 1:
        return one(a, 1.0)
    return [one(a if j % 2 == 0 else (0.5 if a == 1.0 else 1.0), 1.0 + 0.25 * j) for j in range(case["P"])]


def ukf_inputs(case):
    """dict(cfgs, x0 [B,12], P0 [B,12,12], U [B,T,nu], Y [B,T,12], lag [P,B,8,3] | None)"""
    c, rng = case, np.random.default_rng(case["seed"])
    model, P, B, T = c["model"], c["P"], c["B"], c["T"]
    nu = fp.NU[model]
    xs = rng.uniform(-0.3, 0.3, (B, 12))
    U = rng.uniform(-0.3, 0.3, (B, T, nu)) * uc.chan_scale(model)
    lag = rng.uniform(-1, 1, (P, B, 8, 3)) if c["lag"] else None
    if c["wrap"]:
        xs[:, 5] = YAW_START
        xs[:, 11] = YAW_RATE
    X = fp.rollout(model, INTEG[c["integ"]], c["lag_mode"], fv.vehicle(c["names"][-1]), xs, U, DT_UKF, lag=None if lag is None else lag[-1])["traj"]
    Ym = X[:, :T].copy()
    if c["wrap"]:
        Ym[:, :, 5] = Ym[:, :, 5] - 2 * np.pi * np.rint(Ym[:, :, 5] / (2 * np.pi))
    Y = Ym + rng.normal(size=Ym.shape) * uc.SIGMA
    drop = rng.uniform(size=Y.shape) < 0.3
    if c["measured"] == "std":
        Y[drop] = np.nan
        if T > 1:                                                 # one row without any measurement (a single row keeps its own)
            Y[:, min(uc.EMPTY_ROW, T - 1)] = np.nan
    elif c["measured"] == "none":
        Y[:] = np.nan
    for i in UKF_NEVER[:c["r_inf"]]:
        Y[:, :, i] = X[:, :T, i] + 5.0                          # numbers the filter must not look at
    x0 = X[:, 0] + rng.normal(size=(B, 12)) * uc.SIGMA
    d = np.sqrt(4.0 * uc.SIGMA ** 2)
    M = rng.normal(size=(B, 12, 12))
    C = 0.7 * np.eye(12) + 0.3 * (M @ M.transpose(0, 2, 1)) / 12.0
    P0 = d[None, :, None] * C * d[None, None, :]
    P0 = 0.5 * (P0 + P0.transpose(0, 2, 1))
    P0[:, np.triu_indices(12, 1)[0], np.triu_indices(12, 1)[1]] = np.nan
    return dict(cfgs=ukf_cfgs(c), x0=x0, P0=P0, U=U, Y=Y, lag=lag, X=X)


def ukf_lane(o, j, b):
    """the outputs of filter (j, b) as a dict of arrays with a leading axis of one, for ukf_cases.gaps"""
    return {k: (None if o.get(k) is None else np.asarray(o[k])[j:j + 1, b:b + 1]) for k in UKF_OUTS + ("lag",)}


def ukf_lane_gaps(a, o, with_lag):
    """[P,B] of the largest of ukf_cases.gaps over the outputs, per filter"""
    P, B = o["info"].shape[:2]
    g = np.zeros((P, B))
    for j in range(P):
        for b in range(B):
            la, lo = ukf_lane(a, j, b), ukf_lane(o, j, b)
            la["info"], lo["info"] = la["info"][..., [0, 3]], lo["info"][..., [0, 3]]       # the counts are compared exactly, elsewhere
            if not with_lag:
                la["lag"] = lo["lag"] = None
            g[j, b] = max(uc.gaps(la, lo).values())
    return g


def prepare_ukf(case):
    c = case
    ref = ukf_inputs(c)
    veh = [fv.vehicle(n) for n in c["names"]]
    for key, dtype in (("o", np.float64), ("ol", L)):
        ref[key] = ur.filter(c["model"], INTEG[c["integ"]], c["lag_mode"], veh, ref["cfgs"], ref["x0"], ref["P0"], ref["U"], ref["Y"], DT_UKF,
                             lag=ref["lag"], dtype=dtype)
    o, ol = ref["o"], ref["ol"]
    ok = (np.minimum(o["wrap_margin"], ol["wrap_margin"]) > MARGIN) & (np.minimum(o["pivot_min"], ol["pivot_min"]) > PIVOT)
    ok &= (o["info"][..., 2] == -1) & (ol["info"][..., 2] == -1) & (o["info"][..., 1] == ol["info"][..., 1].astype(np.float64))
    return _finish(ref, ukf_lane_gaps(o, ol, c["model"] == 0), ok)


def _structs(cfgs):
    return ur.to_struct(cfgs) if isinstance(cfgs, ur.Cfg) else [ur.to_struct(k) for k in cfgs]


def run_ukf(eng, ctx, case, ref, cand=None, rec=None, rows=None, **kw):
    """engine.ukf_filter on the case; cand / rec / rows: slices of the candidates, the recordings, the time rows; kw overrides
    x0, P0, U, Y, lag"""
    c = case
    cand, rec, rows = (slice(None) if v is None else v for v in (cand, rec, rows))
    cfgs = ref["cfgs"] if isinstance(ref["cfgs"], ur.Cfg) else ref["cfgs"][cand]
    a = dict(x0=ref["x0"][rec], P0=ref["P0"][rec], U=ref["U"][rec, rows], Y=ref["Y"][rec, rows], lag=None if ref["lag"] is None else ref["lag"][cand, rec])
    a.update(kw)
    return eng.ukf_filter(c["model"], c["integ"], [fv.params(n) for n in c["names"]][cand], _structs(cfgs), a["x0"], a["P0"], a["U"], a["Y"], DT_UKF,
                          lag=a["lag"], lag_mode=c["lag_mode"], ctx=ctx)


def compare_ukf(case, ref, got):
    c, o, keep = case, ref["o"], ref["keep"]
    P, B, T = c["P"], c["B"], c["T"]
    assert (got["lag"] is None) == (not c["lag"]), case
    for k in UKF_OUTS:
        assert got[k].shape == o[k].shape, (k, got[k].shape, case)
    have = dict(got)
    if have["lag"] is None:
        have["lag"] = o["lag"]
    worst = _worst(case, "ukf", ukf_lane_gaps(have, o, c["lag"]), keep)
    assert np.array_equal(got["info"][..., 1:3][keep], o["info"][..., 1:3][keep]), ("the number of updates and the failed step are exact", case)
    assert np.array_equal(got["PT"], got["PT"].transpose(0, 1, 3, 2)), ("PT must be bit-symmetric", case)
    if c["measured"] == "none":
        assert np.isnan(got["innov"]).all() and not got["info"][..., 0].any() and not got["info"][..., 1].any(), ("pure prediction", case)
    if c["measured"] == "all":
        assert np.all(got["info"][..., 1] == T * (12 - c["r_inf"])), ("every measured component of every row is an update", case)
    return worst


# ------------------------------------------------------------------------------------------ Koopman linear MPC
def lmpc_record(case, rng):
    """tests/koopman_lmpc_ref.py: case_record -- random weights; limits +-(0.2 .. 0.35) per channel, channel 1 fixed (u_min = u_max),
    channel 2 free; "warm": limits out of reach"""
    c = case
    n, r = c["n"], c["r"]
    lo, hi = -np.linspace(0.35, 0.2, r), np.linspace(0.2, 0.35, r)
    lo[1] = hi[1] = 0.1
    if c["special"] == "warm":
        lo, hi = np.full(r, -5.0), np.full(r, 5.0)
    lo[2], hi[2] = -np.inf, np.inf
    return lr.rec(n, r, rng.uniform(0.5, 2.0, n), rng.uniform(2.0, 8.0, n), rng.uniform(0.05, 0.2, r), lo, hi, hold=c["hold"], iters=c["iters"],
                  tol=c["tol"])


def lmpc_inputs(case):
    """dict(model (C, gamma, A, B), rec with rho, Hq, W, x [nb,n], ref [nb,rows,n], U [nb,M,r], y | None, row0): the recipe of
    koopman_lmpc_ref.case_solver and case_inputs"""
    c, rng = case, np.random.default_rng(case["seed"])
    n, r, nb, H, hold, M = c["n"], c["r"], c["nb"], c["H"], c["hold"], c["M"]
    C, gamma, A, B = lr.synth_model(n, r, c["k"], c["seed"] % 100000)
    rec = lmpc_record(c, rng)
    P, Gc = lr.markov(A, B, n, H, hold)
    Hq = lr.condense(Gc, rec, DT_LMPC, H)[0]
    Hq = 0.5 * (Hq + Hq.T)
    ev = np.linalg.eigvalsh(Hq)
    rec = lr.with_(rec, rho=float(ev[0] / 1e4 if c["special"] == "warm" else np.sqrt(ev[0] * ev[-1])))
    W = np.linalg.inv(Hq + rec.rho * np.eye(M * r))
    W = np.ascontiguousarray(0.5 * (W + W.T))
    rows = H + 1 + lr.REF_TOTAL if c["traj"] else 1
    row0 = lr.ROW0 if c["traj"] else 0
    x, ref = rng.uniform(-0.5, 0.5, (nb, n)), rng.uniform(-0.5, 0.5, (nb, rows, n))
    if n == 13:
        x[:, 3:7] /= np.linalg.norm(x[:, 3:7], axis=1, keepdims=True)
        ref[:, :, 3:7] = x[:, None, 3:7] + 0.2 * ref[:, :, 3:7]
        ref[:, :, 3:7] /= np.linalg.norm(ref[:, :, 3:7], axis=2, keepdims=True)
    if c["special"] == "quat_flip":
        ref[::2, :, 3:7] = -ref[::2, :, 3:7]
    if c["special"] == "angle_wrap":
        ref[:, :, 5] = x[:, None, 5] + 2 * np.pi + 0.1 + 0.01 * ref[:, :, 5]
        ref[:, :, 3] = x[:, None, 3] - 2 * np.pi + 0.2 + 0.01 * ref[:, :, 3]
    U = rng.uniform(-0.4, 0.4, (nb, M, r))
    if c["special"] == "warm":
        for b in range(1, nb, 2):
            rt = lr.adjust(lr.window(ref[b], row0, H), x[b])
            zs = -np.linalg.solve(Hq, lr.gradient(rec, P @ kr.lift(x[b], C, gamma), Gc, rt, DT_LMPC, H)[0]).reshape(M, r)
            U[b] = zs + 1e-4 * (U[b] - zs)
    y = rng.uniform(-0.05, 0.05, (nb, M, r)) if c["y"] else None
    return dict(model=(C, gamma, A, B), rec=rec, Hq=Hq, W=W, x=np.ascontiguousarray(x), ref=np.ascontiguousarray(ref), U=U, y=y, row0=row0)


LMPC_KEYS = ("U_nom", "y", "u_apply", "pred")


def _lmpc_err(a, b):
    """per problem: max |a-b| / max(1, |b|) in long double; equal infinities and NaN in both agree (test_koopman_lmpc_gpu.py: err)"""
    a, b = np.asarray(a, dtype=L), np.asarray(b, dtype=L)
    assert a.shape == b.shape, (a.shape, b.shape)
    same = (a == b) | (np.isnan(a) & np.isnan(b))
    with np.errstate(invalid="ignore"):
        e = np.where(same, L(0), np.abs(a - b) / np.maximum(L(1), np.abs(b)))
    e = np.where(np.isnan(e), L(np.inf), e)
    return np.max(e.reshape(a.shape[0], -1), axis=1).astype(np.float64)


def lmpc_lane_err(a, o, case):
    e = np.zeros(case["nb"])
    for k in LMPC_KEYS:
        if k == "y" and not case["y"]:
            continue
        e = np.maximum(e, _lmpc_err(a[k], o[k]))
    return np.maximum(e, _lmpc_err(np.asarray(a["info"])[:, :4], np.asarray(o["info"])[:, :4]))


def prepare_lmpc(case):
    c = case
    ref = lmpc_inputs(c)
    C, gamma, A, B = ref["model"]
    for key, dtype in (("o", np.float64), ("ol", L)):
        ref[key] = lr.step(C, gamma, A, B, ref["rec"], ref["W"], ref["x"], ref["ref"], ref["U"], DT_LMPC, c["H"], y=ref["y"], ref_row0=ref["row0"],
                           shift=c["shift"], dtype=dtype)
    o, ol = ref["o"], ref["ol"]
    ok = np.all(o["info"][:, 4:] == ol["info"][:, 4:].astype(np.float64), axis=1)
    if c["tol"] > 0:
        ok &= np.array([lr.stop_well_posed(a, c["tol"]) and lr.stop_well_posed(b, c["tol"]) for a, b in zip(o["hist"], ol["hist"])])
    # descent (J(z) <= J(z0)) is asserted on the device where the reference shows it with room to spare
    ref["descent"] = np.minimum(o["info"][:, 1] - o["info"][:, 0], (ol["info"][:, 1] - ol["info"][:, 0]).astype(np.float64)) > 1e-9
    return _finish(ref, lmpc_lane_err(o, ol, c), ok)


def run_lmpc(eng, ctx, case, ref, sel=None, **kw):
    """engine.koopman_lmpc_step on the case; sel: a subset of the problems; kw: iters / tol override the record, U_nom / y the start,
    shift the case's"""
    c = case
    C, gamma, A, B = ref["model"]
    if "coeffs" not in ref:
        ref["coeffs"] = eng.koopman_markov(A, B, c["n"], c["H"], c["hold"]) + (ref["W"],)
    rec = lr.with_(ref["rec"], **{k: kw.pop(k) for k in ("iters", "tol") if k in kw})
    X, R, U, Y = ref["x"], ref["ref"], kw.pop("U_nom", ref["U"]), kw.pop("y", ref["y"])
    if sel is not None:
        X, R, U, Y = X[sel], R[sel], U[sel], (None if Y is None else Y[sel])
    kw.setdefault("shift", c["shift"])
    return eng.koopman_lmpc_step(C, gamma, A, B, lr.to_struct(rec), X, R, U, DT_LMPC, H=c["H"], y=Y, ref_row0=ref["row0"], want_pred=True,
                                 coeffs=ref["coeffs"], ctx=ctx, **kw)


def compare_lmpc(case, ref, got):
    c, o, keep, rec = case, ref["o"], ref["keep"], ref["rec"]
    for k in LMPC_KEYS:
        if got[k] is None:
            assert k == "y" and not c["y"], (k, case)
        else:
            assert got[k].shape == o[k].shape, (k, got[k].shape, o[k].shape, case)
    assert got["info"].shape == o["info"].shape, case
    worst = _worst(case, "lmpc", lmpc_lane_err(got, o, c), keep)
    assert np.array_equal(got["info"][keep, 4], o["info"][keep, 4]), ("iterations", got["info"][:, 4], o["info"][:, 4], case)
    assert np.array_equal(got["info"][keep, 5], o["info"][keep, 5]), ("entries at a limit", got["info"][:, 5], o["info"][:, 5], case)
    if not c["shift"]:
        z = got["U_nom"]
        assert np.all((z >= rec.u_min) & (z <= rec.u_max)), ("feasibility", case)
        assert np.array_equal(got["u_apply"], np.repeat(z[:, :1], c["hold"], axis=1)), ("u_apply is the first knot in hold rows", case)
    d = ref["descent"] & keep
    assert np.all(got["info"][d, 0] <= got["info"][d, 1]), ("descent", got["info"][:, :2], case)
    return worst


PREPARE = dict(ukf=prepare_ukf, lmpc=prepare_lmpc)


def sweep_one(eng, ctx, case, ref):
    """(worst kernel error, 0.0) of one case"""
    if case["family"] == "ukf":
        return compare_ukf(case, ref, run_ukf(eng, ctx, case, ref)), 0.0
    return compare_lmpc(case, ref, run_lmpc(eng, ctx, case, ref)), 0.0
