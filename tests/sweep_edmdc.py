"""What the shape sweeps do with a case of the EDMDc families of tests/sweep_cases.py (lift, gram, pinv_apply, multistep, simulate):
prepare / run / compare as in tests/sweep_run.py, which registers them.  Not collected.

The reference is oracle/edmdc_numpy.py restated with a dtype argument (lift() there forces float64): the same expanded distance form,
in float64 (bit for bit the oracle's, asserted by tests/test_sweep_cases_cpu.py) and in np.longdouble.  The centres are inputs.

Error measures and bounds:
  trajectories (xhat per window, simulate rows per trajectory)   sweep_run.lane_err in long double against TOL_ROLL = 1e-10; a lane is
                                 compared if the reference's float64-to-long-double gap on it is below a tenth of that.
  Gram and apply entries         per entry |got - ref_longdouble| / sum |terms| against TOL_GRAM = 1e-12, sum |terms| formed from
                                 |G|^T |G|, |G|^T |Y| and (|P| |G|^T) |Y|; an entry is compared if the reference's own gap in the same
                                 measure is below 1e-13.  G^T G equals its transpose bit for bit; pair counts are exact.
  lift                           absolute 1e-13 per row; for values above 1e-280 also the relative error against 8 x the reference's own
                                 float64-to-long-double relative gap on the case + 2^-50 (the kernel evaluates the same expanded form
                                 in another order with FMAs: its error is of the reference's order, and 8 covers the order of a 16-term
                                 dot product).  Rows whose reference values are all below 1e-300 (far from every centre): finite,
                                 non-negative, below 1e-290.
  se of the multistep evaluators against the sum of the kernel's OWN per-window errors formed in long double: each of the m = nw n terms
                                 is a rounded difference squared (3 x 2^-53 relative), a fixed-order sum of m positive terms adds
                                 (m - 1) x 2^-53 of the sum: bound (m + 4) x 2^-53 of the sum.
Every assertion message carries the case dict."""
import numpy as np

L = np.longdouble
TOL_ROLL = 1e-10
TOL_GRAM = 1e-12
TOL_LIFT = 1e-13
LIFT_REL_FLOOR = 1e-280                   # values above it are compared by relative error too
LIFT_FAR_REF, LIFT_FAR = 1e-300, 1e-290     # a row whose reference values are all below the first: the kernel's are below the second
LIFT_ORDER = 8.0
TINY = L(1e-300)
DEFAULT_CHUNK = 1 << 20                   # csrc/capi.hip: chunk_rows


# ------------------------------------------------------------------------------------------ the reference
def rbf_mat(X, C, gamma, dtype=np.float64):
    """oracle/edmdc_numpy.py: rbf_mat -- the EXPANDED distance form, in dtype"""
    X, C = np.asarray(X).astype(dtype), np.asarray(C).astype(dtype)
    x2 = np.sum(X ** 2, axis=1)[:, None]
    c2 = np.sum(C ** 2, axis=1)[None, :]
    return np.exp(-dtype(gamma) * (x2 + c2 - 2 * X @ C.T))


def lift(X, C, gamma, dtype=np.float64):
    """oracle/edmdc_numpy.py: lift for 2-D X"""
    return np.hstack([np.asarray(X).astype(dtype), rbf_mat(X, C, gamma, dtype)])


def pairs(Xs, Us, C, gamma, dtype):
    """(G, Y) of every pair of every bag, stacked: G = [phi(x_t), u_t], Y = phi(x_t+1); no pair crosses a bag"""
    n, k, r = C.shape[1], C.shape[0], Us[0].shape[1]
    G, Y = [np.zeros((0, n + k + r), dtype=dtype)], [np.zeros((0, n + k), dtype=dtype)]
    for X, U in zip(Xs, Us):
        if len(X) >= 2:
            Z = lift(X, C, gamma, dtype)
            G.append(np.hstack([Z[:-1], U[:len(X) - 1].astype(dtype)]))
            Y.append(Z[1:])
    return np.vstack(G), np.vstack(Y)


def multistep(X, U, C, gamma, A, B, H, dtype):
    """oracle/edmdc_numpy.py: multistep_rmse up to the end states: x_hat [N - H, n]"""
    ns = len(X) - H
    At, Bt, Ud = A.astype(dtype).T, B.astype(dtype).T, U.astype(dtype)
    Z = lift(X[:ns], C, gamma, dtype)
    for t in range(H):
        Z = Z @ At + Ud[t:t + ns] @ Bt
    return Z[:, :X.shape[1]]


def simulate(x0, U, C, gamma, A, B, dtype):
    """oracle/edmdc_numpy.py: simulate, batched: [nb, T + 1, n]"""
    nb, n = x0.shape
    At, Bt, Ud = A.astype(dtype).T, B.astype(dtype).T, U.astype(dtype)
    out = np.zeros((nb, U.shape[1] + 1, n), dtype=dtype)
    out[:, 0] = x0
    Z = lift(x0, C, gamma, dtype)
    for t in range(U.shape[1]):
        Z = Z @ At + Ud[:, t] @ Bt
        out[:, t + 1] = Z[:, :n]
    return out


def _finish(ref, gaps, bound):
    gaps = np.asarray(gaps, dtype=np.float64)
    keep = gaps < bound
    ref.update(keep=keep, gap=float(gaps[keep].max()) if keep.any() else np.inf, gap_all=float(gaps.max()) if gaps.size else 0.0, gap_bound=bound)
    return ref


def _worst(case, what, e, keep, tol):
    e = np.asarray(e, dtype=np.float64)
    assert e.shape == keep.shape, (what, e.shape, keep.shape, case)
    w = float(e[keep].max()) if keep.any() else 0.0
    assert np.isfinite(w) and w < tol, (what, w, "bound", tol, "worst lane", int(np.argmax(np.where(keep, e, -1.0))), case)
    return w


def _lane_err(a, b):
    import sweep_run as sr
    return sr.lane_err(a, b)


# ------------------------------------------------------------------------------------------ lift
def prepare_lift(case):
    """centres in +-0.5; rows uniform in +- scale, at scale 12 with every |x_j| in 6 .. 12 (far from every centre).  A lane is a row."""
    c, rng = case, np.random.default_rng(case["seed"])
    N, n, k = c["N"], c["n"], c["k"]
    C = rng.uniform(-0.5, 0.5, (k, n))
    if c["scale"] >= 12.0:
        X = rng.choice([-1.0, 1.0], (N, n)) * rng.uniform(0.5 * c["scale"], c["scale"], (N, n))
    else:
        X = rng.uniform(-c["scale"], c["scale"], (N, n))
    o, ol = lift(X, C, c["gamma"]), lift(X, C, c["gamma"], L)
    big = ol[:, n:] > LIFT_REL_FLOOR
    relgap = float(np.max(np.abs(o[:, n:].astype(L) - ol[:, n:])[big] / ol[:, n:][big])) if big.any() else 0.0
    ref = dict(X=X, C=C, o=o, ol=ol, big=big, relgap=relgap, far=np.max(ol[:, n:], axis=1) < LIFT_FAR_REF)
    return _finish(ref, np.max(np.abs(o.astype(L) - ol), axis=1), 0.1 * TOL_LIFT)


def run_lift(eng, ctx, case, ref):
    return eng.lift(ref["X"], ref["C"], case["gamma"], ctx=ctx)


def compare_lift(case, ref, got):
    """(worst absolute error, worst relative error as a share of its bound)"""
    n, ol = case["n"], ref["ol"]
    assert got.shape == ol.shape and np.all(np.isfinite(got)) and np.all(got[:, n:] >= 0.0), (got.shape, case)
    assert np.array_equal(got[:, :n], ref["X"]), ("the state columns are the states", case)
    worst = _worst(case, "lift", np.max(np.abs(got.astype(L) - ol), axis=1), ref["keep"], TOL_LIFT)
    if ref["far"].any():
        assert float(got[ref["far"], n:].max()) < LIFT_FAR, ("rows far from every centre", float(got[ref["far"], n:].max()), case)
    share = 0.0
    if ref["big"].any():
        rel = np.abs(got[:, n:].astype(L) - ol[:, n:])[ref["big"]] / ol[:, n:][ref["big"]]
        bound = LIFT_ORDER * ref["relgap"] + 2.0 ** -50
        share = float(rel.max()) / bound
        assert share <= 1.0, ("lift relative error", float(rel.max()), "bound", bound, "reference's own gap", ref["relgap"], case)
    return worst, share


# ------------------------------------------------------------------------------------------ Gram and pinv_apply: the bags
def _bag_arrays(case, rng):
    """tests/stress_parity.py: grams -- random-walk states (steps 0.05), inputs in +-1, centres N(0, 0.4)"""
    c = case
    Xs = [np.cumsum(rng.normal(0, 0.05, (m, c["n"])), 0) for m in c["lens"]]
    Us = [rng.uniform(-1, 1, (m, c["r"])) for m in c["lens"]]
    return Xs, Us, rng.normal(0, 0.4, (c["k"], c["n"]))


def _uniform_layout(case, Xs, Us, rng):
    """the bags at strides L + 1 + xpad / L + upad; the rows in between hold values of the size of the data that no pair may read"""
    c = case
    nb, L1 = len(c["lens"]), c["lens"][0]
    xs, us = L1 + c["xpad"], L1 - 1 + c["upad"]
    X = rng.uniform(2.0, 3.0, ((nb - 1) * xs + L1, c["n"]))
    U = rng.uniform(2.0, 3.0, ((nb - 1) * us + L1 - 1, c["r"]))
    for b in range(nb):
        X[b * xs:b * xs + L1] = Xs[b]
        U[b * us:b * us + L1 - 1] = Us[b][:L1 - 1]
    return X, U, xs, us


def _given_inputs(case, Us):
    """the list forms' inputs: the last bag's one row shorter than its states where the case says so"""
    return Us[:-1] + [Us[-1][:len(Us[-1]) - 1]] if case["short_u"] else Us


class _settings:
    """the chunk size of a case, and the defaults back afterwards (tests/stress_parity.py: grams)"""

    def __init__(self, ctx, chunk):
        self.ctx, self.chunk = ctx, chunk

    def __enter__(self):
        self.ctx.check(self.ctx.lib.edmdc_set_chunk_rows(self.ctx.h, self.chunk or DEFAULT_CHUNK), "edmdc_set_chunk_rows")

    def __exit__(self, *exc):
        self.ctx.check(self.ctx.lib.edmdc_set_chunk_rows(self.ctx.h, DEFAULT_CHUNK), "edmdc_set_chunk_rows")
        self.ctx.set_apply_variant(0)
        return False


def measure(a, b, mag):
    """per entry |a - b| / sum |terms|, b in long double"""
    return (np.abs(np.asarray(a).astype(L) - b) / (mag.astype(L) + TINY)).astype(np.float64)


def prepare_gram(case):
    """A lane is an entry of G^T G (and of G^T Y where the case asks for it)."""
    c, rng = case, np.random.default_rng(case["seed"])
    Xs, Us, C = _bag_arrays(c, rng)
    ref = dict(Xs=Xs, Us=Us, C=C)
    if c["form"] == "uniform_dev":
        ref["Xu"], ref["Uu"], ref["xs"], ref["us"] = _uniform_layout(c, Xs, Us, rng)
    G, Y = pairs(Xs, Us, C, c["gamma"], np.float64)
    Gl, Yl = pairs(Xs, Us, C, c["gamma"], L)
    both = Gl.T @ np.hstack([Gl, Yl])
    p = G.shape[1]
    ref.update(o=(G.T @ G, G.T @ Y), ol=(both[:, :p], both[:, p:]), mag=(np.abs(G).T @ np.abs(G), np.abs(G).T @ np.abs(Y)), pairs=len(G))
    assert ref["pairs"] == c["pairs"], case
    gaps = [measure(ref["o"][i], ref["ol"][i], ref["mag"][i]).ravel() for i in range(2 if c["gty"] else 1)]
    return _finish(ref, np.concatenate(gaps), 0.1 * TOL_GRAM)


def _gram_dev(eng, ctx, case, ref, split):
    """the device forms: one call, or two with accumulate over `split` bags and the rest"""
    c = case
    n, r, k = c["n"], c["r"], c["k"]
    p, d, nb = n + k + r, n + k, len(c["lens"])
    D = eng.DevArray
    Cd, Gd = D.from_host(ctx, ref["C"]), D(ctx, (p, p)).zero_()
    Yd = D(ctx, (p, d)).zero_() if c["gty"] else None
    parts = [(0, nb)] if not split else [(0, split), (split, nb)]
    if c["form"] == "ragged_dev":
        Xd, Ud, off = eng.upload_bags(ref["Xs"], _given_inputs(c, ref["Us"]), n, r, ctx=ctx)
        for i, (a, b) in enumerate(parts):
            eng.gram_ragged_dev(Xd.rows(off[a], off[b]), Ud.rows(off[a], off[b]), Cd, c["gamma"], off[a:b + 1] - off[a], Gd, Yd, accumulate=i > 0, ctx=ctx)
    else:
        Xd, Ud, xs, us = D.from_host(ctx, ref["Xu"]), D.from_host(ctx, ref["Uu"]), ref["xs"], ref["us"]
        L1 = c["lens"][0]
        for i, (a, b) in enumerate(parts):
            eng.gram_dev(Xd.rows(a * xs, (b - 1) * xs + L1), Ud.rows(a * us, (b - 1) * us + L1 - 1), Cd, c["gamma"], b - a, L1 - 1, xs, us, Gd, Yd,
                         accumulate=i > 0, ctx=ctx)
    return dict(GtG=Gd.numpy(), GtY=None if Yd is None else Yd.numpy(), npairs=None)


def run_gram(eng, ctx, case, ref, split=None):
    c = case
    with _settings(ctx, c["chunk"]):
        if c["form"] == "host":
            GtG, GtY, npairs = eng.gram(ref["Xs"], _given_inputs(c, ref["Us"]), ref["C"], c["gamma"], ctx=ctx)
            return dict(GtG=GtG, GtY=GtY, npairs=npairs)
        return _gram_dev(eng, ctx, c, ref, c["split"] if split is None else split)


def gram_errors(case, ref, got):
    """per-entry errors of G^T G (and G^T Y), flattened like the keep mask"""
    out = [measure(got["GtG"], ref["ol"][0], ref["mag"][0]).ravel()]
    if case["gty"]:
        out.append(measure(got["GtY"], ref["ol"][1], ref["mag"][1]).ravel())
    return np.concatenate(out)


def compare_gram(case, ref, got):
    c = case
    p, d = c["n"] + c["k"] + c["r"], c["n"] + c["k"]
    assert got["GtG"].shape == (p, p) and (got["GtY"] is None) == (not c["gty"]) and (got["GtY"] is None or got["GtY"].shape == (p, d)), case
    assert np.all(np.isfinite(got["GtG"])) and (got["GtY"] is None or np.all(np.isfinite(got["GtY"]))), ("finite", case)
    assert np.array_equal(got["GtG"], got["GtG"].T), ("G^T G equals its transpose bit for bit", case)
    assert got["npairs"] is None or got["npairs"] == ref["pairs"], ("pair count", got["npairs"], ref["pairs"], case)
    return _worst(case, "gram, |err| / sum |terms| per entry", gram_errors(c, ref, got), ref["keep"], TOL_GRAM)


# ------------------------------------------------------------------------------------------ pinv_apply
def prepare_pinv_apply(case):
    """tests/stress_parity.py: applies -- P random with entries ~ 1 / sqrt(p).  A lane is an entry of M = (P G^T) Y."""
    c, rng = case, np.random.default_rng(case["seed"])
    Xs, Us, C = _bag_arrays(c, rng)
    p = c["n"] + c["k"] + c["r"]
    P = rng.normal(0, 1, (p, p)) / np.sqrt(p)
    ref = dict(Xs=Xs, Us=Us, C=C, P=P)
    if c["form"] == "uniform_dev":
        ref["Xu"], ref["Uu"], ref["xs"], ref["us"] = _uniform_layout(c, Xs, Us, rng)
    G, Y = pairs(Xs, Us, C, c["gamma"], np.float64)
    Gl, Yl = pairs(Xs, Us, C, c["gamma"], L)
    ref.update(o=(P @ G.T) @ Y, ol=(P.astype(L) @ Gl.T) @ Yl, mag=(np.abs(P) @ np.abs(G).T) @ np.abs(Y))
    return _finish(ref, measure(ref["o"], ref["ol"], ref["mag"]).ravel(), 0.1 * TOL_GRAM)


def run_pinv_apply(eng, ctx, case, ref):
    """M of both apply variants"""
    c = case
    n, r, k = c["n"], c["r"], c["k"]
    out = []
    with _settings(ctx, c["chunk"]):
        D = eng.DevArray
        if c["form"] == "ragged_dev":
            Xd, Ud, off = eng.upload_bags(ref["Xs"], ref["Us"], n, r, ctx=ctx)
        elif c["form"] == "uniform_dev":
            Xd, Ud = D.from_host(ctx, ref["Xu"]), D.from_host(ctx, ref["Uu"])
        if c["form"] != "host":
            Cd = D.from_host(ctx, ref["C"])
        for v in (0, 1):
            ctx.set_apply_variant(v)
            if c["form"] == "host":
                out.append(eng.pinv_apply(ref["Xs"], ref["Us"], ref["C"], c["gamma"], ref["P"], ctx=ctx))
                continue
            Md = D(ctx, (n + k + r, n + k)).zero_()
            if c["form"] == "ragged_dev":
                eng.pinv_apply_ragged_dev(Xd, Ud, Cd, c["gamma"], off, ref["P"], Md, ctx=ctx)
            else:
                eng.pinv_apply_dev(Xd, Ud, Cd, c["gamma"], len(c["lens"]), c["lens"][0] - 1, ref["xs"], ref["us"], ref["P"], Md, ctx=ctx)
            out.append(Md.numpy())
    return out


def compare_pinv_apply(case, ref, got):
    """(worst error of variant 0, of variant 1): each against the long-double reference"""
    worst = []
    for v, M in enumerate(got):
        assert M.shape == ref["ol"].shape and np.all(np.isfinite(M)), (v, M.shape, case)
        worst.append(_worst(case, f"pinv_apply variant {v}, |err| / sum |terms| per entry", measure(M, ref["ol"], ref["mag"]).ravel(), ref["keep"], TOL_GRAM))
    return tuple(worst)


# ------------------------------------------------------------------------------------------ multistep evaluators
def _model(case, rng):
    import sweep_run as sr
    return sr.koopman_model(rng, case["n"], case["r"], case["k"])


def prepare_multistep(case):
    """sweep_run.koopman_model (spectral radius 0.98), states in +-0.5, inputs in +-1.  A lane is a window; a case without a window
    (H >= N) has one lane, the total, which must be 0."""
    c, rng = case, np.random.default_rng(case["seed"])
    N, H, n, r = c["N"], c["H"], c["n"], c["r"]
    C, gamma, A, B = _model(c, rng)
    X, U = rng.uniform(-0.5, 0.5, (N, n)), rng.uniform(-1, 1, (N, r))
    ref = dict(X=X, U=U, C=C, gamma=gamma, A=A, B=B)
    if c["nw"] == 0:
        return _finish(ref, np.zeros(1), 0.1 * TOL_ROLL)
    ref.update(o=multistep(X, U, C, gamma, A, B, H, np.float64), ol=multistep(X, U, C, gamma, A, B, H, L))
    return _finish(ref, _lane_err(ref["o"], ref["ol"]), 0.1 * TOL_ROLL)


def run_multistep(eng, ctx, case, ref, short_u=None):
    """((se, xhat) of multistep_se, (se, xhat) of multistep_se_linear)"""
    short = case["short_u"] if short_u is None else short_u
    U = ref["U"][:case["N"] - 1] if short else ref["U"]
    args = (ref["X"], U, ref["C"], ref["gamma"], ref["A"], ref["B"], case["H"])
    return eng.multistep_se(*args, want_xhat=True, ctx=ctx), eng.multistep_se_linear(*args, want_xhat=True, ctx=ctx)


def compare_multistep(case, ref, got):
    """(worst x_hat error of the propagated evaluator, of the linear one)"""
    c = case
    worst = []
    for what, (se, xh) in zip(("multistep_se", "multistep_se_linear"), got):
        assert xh.shape == (c["nw"], c["n"]) and np.isfinite(se), (what, xh.shape, se, case)
        if c["nw"] == 0:
            assert se == 0.0, (what, "H >= N gives 0", se, case)
            worst.append(0.0)
            continue
        worst.append(_worst(case, what + " x_hat", _lane_err(xh, ref["o"]), ref["keep"], TOL_ROLL))
        own = float(np.sum((ref["X"][c["H"]:].astype(L) - xh.astype(L)) ** 2))
        bound = (c["nw"] * c["n"] + 4) * 2.0 ** -53
        assert abs(se - own) <= bound * own, (what + " se against the sum of its own window errors", se, own, abs(se - own) / max(own, 1e-300), bound, case)
    return tuple(worst)


# ------------------------------------------------------------------------------------------ simulate
def prepare_simulate(case):
    """the same model and input sizes.  A lane is a trajectory."""
    c, rng = case, np.random.default_rng(case["seed"])
    C, gamma, A, B = _model(c, rng)
    x0, U = rng.uniform(-0.5, 0.5, (c["nb"], c["n"])), rng.uniform(-1, 1, (c["nb"], c["T"], c["r"]))
    ref = dict(x0=x0, U=U, C=C, gamma=gamma, A=A, B=B, o=simulate(x0, U, C, gamma, A, B, np.float64), ol=simulate(x0, U, C, gamma, A, B, L))
    return _finish(ref, _lane_err(ref["o"], ref["ol"]), 0.1 * TOL_ROLL)


def run_simulate(eng, ctx, case, ref, rows=slice(None)):
    return eng.simulate_lifted(ref["x0"][rows], ref["U"][rows], ref["C"], ref["gamma"], ref["A"], ref["B"], ctx=ctx)


def compare_simulate(case, ref, got):
    assert got.shape == ref["o"].shape and np.all(np.isfinite(got)), (got.shape, case)
    assert got[:, 0].tobytes() == ref["x0"].tobytes(), ("row 0 is x0 bit for bit", case)
    return _worst(case, "simulate", _lane_err(got, ref["o"]), ref["keep"], TOL_ROLL)


PREPARE = dict(lift=prepare_lift, gram=prepare_gram, pinv_apply=prepare_pinv_apply, multistep=prepare_multistep, simulate=prepare_simulate)


def sweep_one(eng, ctx, case, ref):
    """(worst kernel error, second figure) of one case: lift -- relative error as a share of its bound; pinv_apply -- the second variant;
    multistep -- the linear evaluator"""
    fam = case["family"]
    if fam == "lift":
        return compare_lift(case, ref, run_lift(eng, ctx, case, ref))
    if fam == "gram":
        return compare_gram(case, ref, run_gram(eng, ctx, case, ref)), 0.0
    if fam == "pinv_apply":
        return compare_pinv_apply(case, ref, run_pinv_apply(eng, ctx, case, ref))
    if fam == "multistep":
        return compare_multistep(case, ref, run_multistep(eng, ctx, case, ref))
    return compare_simulate(case, ref, run_simulate(eng, ctx, case, ref)), 0.0
