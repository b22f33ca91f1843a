"""What the shape sweeps do with a case of the k-means families of tests/sweep_cases.py (colstats, kmeanspp, lloyd): prepare / run /
compare as in tests/sweep_run.py, which registers them.  Not collected.

The three references are exact in the sense that matters for each kernel:

  colstats   mean and population variance per column in np.longdouble.  The mean is held at TOL_MEAN = 1e-13 of mean_i |x_ij|, the
             variance at TOL_VAR = 1e-12 of the column's variance, per column; a column whose variance is exactly 0 (constant, or
             N = 1) absolutely at 1e-12 mean_j^2.  NumPy's own float64 mean / var stay within a tenth of both (asserted in prepare).
  kmeanspp   scikit-learn 1.7.2's `_kmeans_plusplus` for unit weights restated in long double, fed (first_index, uniforms, n_trials).
             It records per round whether the round is DECIDED: every drawn value u pot farther than PP_EDGE = 1e-12 pot from both
             running-sum boundaries of the row it falls in, and the best candidate's potential more than PP_TIE = 1e-10 relative
             below the best other candidate's.  prepare asserts that every round of a case is decided; then the indices are exact,
             the centres X[idx] - mean bit for bit, and scikit-learn itself (fed the same numbers) picks the same rows.
  lloyd      oracle/kmeans_numpy.py: lloyd_fixed_point -- the device loop's integer member sums restated -- with a CERTIFIED E-step:
             float64 scores x.c - |c|^2 / 2 by GEMM decide a sample whose best and second-best differ by more than E_FP64 = 1e-9 R^2
             (R^2 = 2 max |x|^2, as in the kernel); the others are scored again in long double against every centre and decided
             if the best exceeds the best NON-IDENTICAL centre by more than E_MARGIN = 1e-11 R^2 (identical centres tie exactly in
             any arithmetic: the lowest index wins).  1e-11 R^2 is 10^4 times the 1.1e-15 R^2 the kernel's header derives for its
             FMA chain and 20 times the 5e-13 R^2 by which the candidate filter certifies a skip.  prepare asserts that no sample
             of any iteration is undecided; then n_iter and the labels are exact and the centres equal bit for bit.  The inertia
             is held at 1e-10 relative against the long-double sum over the returned labels and centres.

Data: sweep_cases.py describes the recipe and the operand forms.  The padding of the strided forms is NaN: no kernel may read it.
Every assertion message carries the case dict."""
import json

import numpy as np

import sweep_cases as sc
from oracle import kmeans_numpy as kn

L = np.longdouble


class IllPosed(AssertionError):
    """a condition on the REFERENCE alone that a case does not meet: a fixed case that raises it gets another data seed, a random draw of
    tests/stress_parity.py is skipped and counted.  (Everything else prepare asserts is a mistake in the case or in the reference.)"""


def _posed(ok, *what):
    if not ok:
        raise IllPosed(what)


TOL_MEAN, TOL_VAR = 1e-13, 1e-12
PP_EDGE, PP_TIE = 1e-12, 1e-10
E_FP64, E_MARGIN = 1e-9, 1e-11
TOL_INERTIA = 1e-10
LLOYD_VARIANTS = (1, 2, 4, 6)             # the public ones besides 0 (include/brov2.h: edmdc_set_kmeans_variant)
FORMS = sc.SETS["lloyd"]["form"]


# ------------------------------------------------------------------------------------------ data and operands
def data(case):
    """(X [N,n] float64, the generator after it) by the recipe of tests/sweep_cases.py"""
    c, rng = case, np.random.default_rng(case["seed"])
    N, n = c["N"], c["n"]
    X = np.cumsum(rng.normal(0, 0.05, (N, n)), 0) + 0.3 * np.sin(np.arange(N)[:, None] * rng.uniform(0.001, 0.01, n))
    if c["order"] == "shuffled":
        X = X[rng.permutation(N)]
    elif c["order"] == "blobs":
        X = rng.normal(0, 1.0, (4, n))[rng.integers(0, 4, N)] + rng.normal(0, 0.02, (N, n))
    X = X * c["scale"]
    if c["offset"]:
        X = X + c["scale"] * rng.uniform(20.0, 100.0, n) * rng.choice([-1.0, 1.0], n)
    if c["const_col"]:
        j = int(rng.integers(0, n))
        X[:, j] = float(np.float32(X[0, j]))                        # 24 bits: every partial sum of the column is exact, its mean the value
    return np.ascontiguousarray(X), rng


def operand(eng, ctx, X, form):
    """X as the device operand of a form: a DevArray ("host": uploaded as it is) or a torch tensor"""
    if form == "host":
        return eng.DevArray.from_host(ctx, X)
    import torch
    dev = torch.device("cuda", ctx.device)
    N, n = X.shape
    t = torch.from_numpy(X).to(dev)
    if form == "dev":
        return t
    if form == "dev_stride":
        W = torch.full((N, n + 1), float("nan"), dtype=torch.float64, device=dev)
        col = 0
    else:
        W = torch.full((N, sc.KM_BLOCK_WIDTH), float("nan"), dtype=torch.float64, device=dev)
        col = sc.KM_BLOCK_COL[form]
    W[:, col:col + n] = t
    v = W[:, col:col + n]
    assert v.stride(0) == W.shape[1] and v.stride(1) == 1 and v.data_ptr() % 16 == (8 if form == "block_odd" else 0)
    return v


def _done(ref, decided, min_gap):
    """the keys tests/sweep_run.py: well_posed reads; a k-means reference leaves nothing out"""
    ref.update(keep=np.asarray(decided, dtype=bool).reshape(-1), gap=0.0, gap_all=0.0, gap_bound=1.0, min_gap=float(min_gap))
    return ref


# ------------------------------------------------------------------------------------------ colstats
def prepare_colstats(case):
    X, _ = data(case)
    Xl = X.astype(L)
    ml = Xl.mean(axis=0)
    vl = ((Xl - ml) ** 2).mean(axis=0)
    mag = np.abs(Xl).mean(axis=0)
    flat = vl == 0                                                   # a constant column (or N = 1): compared absolutely
    bound_m = TOL_MEAN * mag
    bound_v = np.where(flat, TOL_VAR * ml * ml, TOL_VAR * vl)
    ref = dict(X=X, ml=ml, vl=vl, flat=flat, bound_m=bound_m, bound_v=bound_v)
    gm = np.abs(X.mean(axis=0).astype(L) - ml) / bound_m
    gv = np.abs(np.var(X, axis=0).astype(L) - vl) / bound_v
    ref["numpy_share"] = float(max(gm.max(), gv.max()))
    _posed(ref["numpy_share"] < 0.1, "NumPy's float64 mean / var beyond a tenth of the bound", float(gm.max()), float(gv.max()), case)
    if case["const_col"]:
        assert flat.any(), case
    return _done(ref, np.ones(case["n"], dtype=bool), np.inf)


def _col_stats_c(eng, ctx, op, null):
    """edmdc_col_stats_dev with either output pointer NULL; an output that is not asked for stays NaN"""
    eng._bind(op, ctx)
    N, n = op.shape
    mean, var = np.full(n, np.nan), np.full(n, np.nan)
    ctx.check(ctx.lib.edmdc_col_stats_dev(ctx.h, N, n, eng._drows(op), op.stride(0), None if null == "mean" else mean.ctypes.data,
                                          None if null == "var" else var.ctypes.data), "edmdc_col_stats_dev")
    return mean, var


def run_colstats(eng, ctx, case, ref):
    """the case's form through engine.col_stats_dev and through the C ABI with the case's NULL pointer; the contiguous data as a
    DevArray and as a torch tensor"""
    op = operand(eng, ctx, ref["X"], case["form"])
    return dict(full=eng.col_stats_dev(op, ctx=ctx), part=_col_stats_c(eng, ctx, op, case["null"]),
                native=eng.col_stats_dev(operand(eng, ctx, ref["X"], "host"), ctx=ctx), torch=eng.col_stats_dev(operand(eng, ctx, ref["X"], "dev"), ctx=ctx))


def compare_colstats(case, ref, got):
    """(worst share of the mean's bound, of the variance's) over the columns"""
    mean, var = got["full"]
    em = np.abs(mean.astype(L) - ref["ml"]) / ref["bound_m"]
    ev = np.abs(var.astype(L) - ref["vl"]) / ref["bound_v"]
    assert np.all(np.isfinite(mean)) and float(em.max()) < 1.0, ("colstats mean, share of 1e-13 mean |x| per column", em.astype(float), case)
    assert np.all(np.isfinite(var)) and float(ev.max()) < 1.0, ("colstats variance, share of 1e-12 var per column", ev.astype(float), case)
    pm, pv = got["part"]
    null = case["null"]
    assert np.all(np.isnan(pm)) if null == "mean" else pm.tobytes() == mean.tobytes(), ("mean with var_host " + ("given" if null == "mean" else "NULL"), case)
    assert np.all(np.isnan(pv)) if null == "var" else pv.tobytes() == var.tobytes(), ("variance with mean_host NULL", case)
    assert got["native"][0].tobytes() == got["torch"][0].tobytes() and got["native"][1].tobytes() == got["torch"][1].tobytes(), ("DevArray against torch", case)
    return float(em.max()), float(ev.max())


# ------------------------------------------------------------------------------------------ kmeanspp
def kmeanspp_ref(Xc, first, U, k):
    """scikit-learn 1.7.2 sklearn/cluster/_kmeans.py: _kmeans_plusplus with unit weights, in long double, with the random numbers
    given: U [k - 1, n_trials].  Returns (indices [k], decided [k - 1], smallest boundary margin / pot, smallest relative separation)."""
    Xl = Xc.astype(L)
    N = len(Xl)
    idx = [int(first)]
    closest = ((Xl - Xl[first]) ** 2).sum(axis=1)
    pot = closest.sum()
    decided, edge_min, tie_min = [], np.inf, np.inf
    for c in range(1, k):
        r = U[c - 1].astype(L) * pot
        cs = np.cumsum(closest)
        cand = np.minimum(np.searchsorted(cs, r), N - 1)             # side="left", then the clip
        lo = np.where(cand > 0, cs[np.maximum(cand - 1, 0)], L(0))
        edge = float(np.min(np.minimum(r - lo, cs[cand] - r)) / pot) if pot > 0 else 0.0
        uniq = list(dict.fromkeys(int(v) for v in cand))             # the same row drawn twice is one candidate
        D = np.stack([np.minimum(closest, ((Xl - Xl[j]) ** 2).sum(axis=1)) for j in uniq])
        pots = D.sum(axis=1)
        b = int(np.argmin(pots))
        others = np.delete(pots, b)
        tie = float((others.min() - pots[b]) / others.min()) if len(others) and others.min() > 0 else (np.inf if not len(others) else 0.0)
        decided.append(edge > PP_EDGE and tie > PP_TIE)
        edge_min, tie_min = min(edge_min, edge), min(tie_min, tie)
        idx.append(uniq[b])
        closest, pot = D[b], pots[b]
    return np.array(idx, dtype=np.int64), np.array(decided, dtype=bool), edge_min, tie_min


class _Fed(np.random.RandomState):
    """a RandomState that hands scikit-learn the case's own numbers: choice() the first index, uniform() the next row of U"""

    def feed(self, first, U):
        self._first, self._rows = int(first), [np.array(u) for u in U]
        return self

    def choice(self, *a, **kw):
        return self._first

    def uniform(self, *a, **kw):
        return self._rows.pop(0)


def sklearn_indices(Xc, first, U, k, trials):
    from sklearn.cluster import kmeans_plusplus
    return np.asarray(kmeans_plusplus(Xc, k, random_state=_Fed(0).feed(first, U), n_local_trials=trials)[1], dtype=np.int64)


def prepare_kmeanspp(case):
    c = case
    X, rng = data(c)
    mean = X.mean(axis=0) if c["mean"] else None
    Xc = X - mean if c["mean"] else X
    U = rng.uniform(size=(c["k"] - 1, c["trials"]))
    idx, decided, edge, tie = kmeanspp_ref(Xc, c["first"], U, c["k"])
    _posed(decided.all(), "k-means++ reference: undecided rounds", np.where(~decided)[0] + 1, "smallest edge / tie margins", edge, tie, case)
    # the restatement is scikit-learn's: fed the same numbers, kmeans_plusplus itself picks the same rows (no GPU in this)
    sk_idx = sklearn_indices(Xc, c["first"], U, c["k"], c["trials"])
    assert np.array_equal(sk_idx, idx), ("scikit-learn's kmeans_plusplus fed the same numbers", int(np.sum(sk_idx != idx)), case)
    ref = dict(X=X, mean=mean, Xc=Xc, U=np.ascontiguousarray(U), idx=idx, sk_idx=sk_idx, centres=Xc[idx], edge=edge, tie=tie)
    return _done(ref, decided if len(decided) else np.ones(1, dtype=bool), min(edge / PP_EDGE, tie / PP_TIE))


def run_kmeanspp(eng, ctx, case, ref):
    """edmdc_kmeanspp_dev through the C ABI (the test's own uniforms and n_trials): (centres [k,n], indices [k] | None)"""
    from bluerov2_dynamics_amd._lib import _hptr
    c = case
    op = operand(eng, ctx, ref["X"], c["form"])
    ns = eng.arrays_of(op, ctx)
    ns.bind()
    C = ns.empty((c["k"], c["n"]))
    ind = np.full(c["k"], -1, dtype=np.int64)
    ns.sync()
    ctx.check(ctx.lib.edmdc_kmeanspp_dev(ctx.h, c["N"], c["n"], c["k"], eng._drows(op), op.stride(0), _hptr(ref["mean"]), c["first"], c["trials"],
                                         _hptr(ref["U"]) if c["k"] > 1 else None, eng._dptr(C), ind.ctypes.data if c["ind"] else None),
              "edmdc_kmeanspp_dev")
    return ns.download(C), (ind if c["ind"] else None)


def compare_kmeanspp(case, ref, got):
    """(indices that differ from the reference, from scikit-learn): both 0"""
    C, ind = got
    if ind is not None:
        bad = int(np.sum(ind != ref["idx"]))
        assert bad == 0, ("k-means++ indices against the long-double restatement", bad, "first at round", int(np.argmax(ind != ref["idx"])), case)
    assert C.tobytes() == ref["centres"].tobytes(), ("k-means++ centres are X[idx] - mean bit for bit", int(np.sum(np.any(C != ref["centres"], axis=1))), case)
    bad_sk = int(np.sum(ind != ref["sk_idx"])) if ind is not None else 0
    assert bad_sk == 0, ("k-means++ indices against scikit-learn's kmeans_plusplus fed the same numbers", bad_sk, case)
    return 0.0, float(bad_sk)


# ------------------------------------------------------------------------------------------ lloyd: the certified E-step
class Certified:
    """e_step(X, C) for kmeans_numpy.lloyd_fixed_point that knows which labels no rounding can change (module docstring).  Keeps the
    smallest decision gap (relative to R^2), the undecided samples and the labels changed per call."""
    CHUNK = 32768

    def __init__(self, X):
        self.R2 = 2.0 * float(np.max(np.einsum("ij,ij->i", X, X))) if len(X) else 0.0
        self.min_gap, self.undecided, self.rescored, self.changed, self.prev = np.inf, 0, 0, [], None

    def __call__(self, X, C):
        N, k = len(X), len(C)
        labels = np.zeros(N, dtype=np.int32)
        if k > 1:
            half = 0.5 * np.einsum("ij,ij->i", C, C)
            _, inv = np.unique(C, axis=0, return_inverse=True)
            inv = np.asarray(inv).reshape(-1)
            lowest = np.full(inv.max() + 1, k, dtype=np.int64)
            np.minimum.at(lowest, inv, np.arange(k))
            canon = lowest[inv]                                       # the lowest index among the centres identical to this one
            for s in range(0, N, self.CHUNK):
                S = X[s:s + self.CHUNK] @ C.T - half
                rows = np.arange(len(S))
                b = np.argmax(S, axis=1)
                best = S[rows, b]
                S[rows, b] = -np.inf
                gap = best - S.max(axis=1)
                labels[s:s + self.CHUNK] = b
                hard = np.where(~(gap > E_FP64 * self.R2))[0]
                easy = np.delete(gap, hard)
                if easy.size:
                    self.min_gap = min(self.min_gap, float(easy.min()) / self.R2)
                for h in range(0, len(hard), 2048):
                    self._rescore(X, C, canon, s + hard[h:h + 2048], labels)
        self.changed.append(int(N if self.prev is None else np.sum(labels != self.prev)))
        self.prev = labels
        return labels

    def _rescore(self, X, C, canon, rows, labels):
        Cl = C.astype(L)
        sl = X[rows].astype(L) @ Cl.T - L(0.5) * np.einsum("ij,ij->i", Cl, Cl)
        w = np.argmax(sl, axis=1)
        cw = canon[w]
        other = np.where(canon[None, :] == cw[:, None], -np.inf, sl).max(axis=1)
        margin = (sl[np.arange(len(rows)), w] - other).astype(np.float64)      # +inf where every centre is identical
        ok = margin > E_MARGIN * self.R2
        self.rescored += len(rows)
        self.undecided += int(np.sum(~ok))
        if ok.any() and np.isfinite(margin[ok]).any():
            self.min_gap = min(self.min_gap, float(margin[ok][np.isfinite(margin[ok])].min()) / self.R2)
        labels[rows] = cw


# ------------------------------------------------------------------------------------------ lloyd
_REFS = {}                                # a reference is computed once per case and shared by the tests of a process


def _allzero(n):
    """symmetric integer points with power-of-two multiplicities (tests/test_gpu_parity.py: test_lloyd_empty_clusters_follow_sklearn):
    the column means are exactly 0, every sum and mean exact, all distances zero after the first M-step -- nothing is relocated, and
    cluster 1 (empty, in front of the biggest cluster 3) takes that cluster's SUM"""
    z = np.zeros(n)
    pA, pC = z.copy(), z.copy()
    pA[:2], pC[2] = (1.0, 2.0), 4.0
    X = np.concatenate([np.tile(pA, (2, 1)), np.tile(-pA, (2, 1)), np.tile(pC, (4, 1)), np.tile(-pC, (4, 1))])
    return X, np.array([pA, pA, -pA, pC, -pC, pC])


def lloyd_inputs(case):
    """(X, mean, C0 in the centred frame, tol_abs)"""
    c = case
    if c["init"] == "allzero":
        X, C0 = _allzero(c["n"])
        return X, np.zeros(c["n"]), C0, 0.0
    X, rng = data(c)
    mean = X.mean(axis=0)
    Xc = X - mean
    N, k = c["N"], c["k"]
    C0 = Xc[rng.choice(N, k, replace=False)].copy()
    if c["init"] == "dup":
        C0[1] = C0[k - 1] = C0[0]
    elif c["init"] in ("far2", "far3"):
        C0[0] += 40.0 * c["scale"]
        C0[k - 1] -= 70.0 * c["scale"]
        if c["init"] == "far3":
            C0[k // 2] += 25.0 * c["scale"]
    tol_abs = 1e-4 * float(np.var(X, axis=0).mean()) if c["stop"] == "shift" else 0.0
    return X, mean, C0, tol_abs


def prepare_lloyd(case):
    key = json.dumps(case, sort_keys=True)
    if key in _REFS:
        return _REFS[key]
    c = case
    X, mean, C0, tol_abs = lloyd_inputs(c)
    Xc = X - mean
    if c["const_col"]:
        assert np.any(np.all(Xc == 0.0, axis=0)), ("a column that is exactly 0 after centring", case)
    cert = Certified(Xc)
    C, labels, n_iter, nreloc = kn.lloyd_fixed_point(Xc, C0, c["max_iter"], tol_abs, far_rows=kn.far_rows_introselect, e_step=cert)
    _posed(cert.undecided == 0, "Lloyd reference: undecided samples", cert.undecided, "of", cert.rescored, "rescored", case)
    last = cert.changed[n_iter - 1]                                  # labels changed by the last E-step of the loop
    if c["stop"] == "max_iter":
        _posed(n_iter == c["max_iter"] and last > 0, "the loop was to run out of iterations", n_iter, last, case)
    elif c["stop"] == "strict":
        _posed(n_iter < c["max_iter"] and last == 0, "the loop was to stop on unchanged labels", n_iter, last, case)
    else:
        _posed(tol_abs > 0 and n_iter < c["max_iter"] and last > 0, "the loop was to stop on the centre shift", n_iter, last, case)
    if c["init"] in ("dup", "far2", "far3"):
        assert nreloc > 0, ("a relocation", case)
    if c["init"] == "allzero":
        assert nreloc == 0 and np.array_equal(C[1], 4.0 * C[3]), ("the sum of the biggest cluster", C, case)
    d = Xc.astype(L) - C[labels].astype(L)
    ref = dict(X=X, mean=mean, C0=C0, tol_abs=tol_abs, C=C, labels=labels, n_iter=n_iter, nreloc=nreloc, R2=cert.R2, rescored=cert.rescored,
               inertia=(d * d).sum())
    _REFS[key] = _done(ref, np.ones(1, dtype=bool), cert.min_gap)
    return _REFS[key]


_CTXS = {}


def lloyd_ctx(ctx, variant=0, rate=None):
    """a context of its own per (variant, bounds rate), with the library's selection rule for the empty clusters' rows"""
    from bluerov2_dynamics_amd import _lib
    key = (ctx.device, variant, rate)
    if key not in _CTXS:
        c = _lib.Context(ctx.device)
        c.set_kmeans_variant(variant)
        c.set_kmeans_far_select(False)
        if rate is not None:
            c.set_kmeans_bounds_rate(rate)
        _CTXS[key] = c
    return _CTXS[key]


def close_contexts():
    while _CTXS:
        _CTXS.popitem()[1].close()


def lloyd_once(eng, c, case, ref, form, max_iter=None, C0=None):
    """one Lloyd call on context c: dict(C, labels, inertia, n_iter, info, reloc); "host": engine.kmeans_lloyd on host arrays, every
    other form engine.kmeans_lloyd_dev on the device operand"""
    max_iter = case["max_iter"] if max_iter is None else max_iter
    C0 = ref["C0"] if C0 is None else C0
    if form == "host":
        C, labels, inertia, n_iter = eng.kmeans_lloyd(ref["X"], C0, max_iter=max_iter, tol_abs=ref["tol_abs"], mean=ref["mean"], ctx=c)
    else:
        op = operand(eng, c, ref["X"], form)
        ns = eng.arrays_of(op, c)
        Cd, ld, inertia, n_iter = eng.kmeans_lloyd_dev(op, C0, max_iter=max_iter, tol_abs=ref["tol_abs"], mean=ref["mean"], ctx=c)
        C, labels = ns.download(Cd), ns.download(ld)
    return dict(C=C, labels=labels, inertia=inertia, n_iter=n_iter, info=c.kmeans_loop_info(), reloc=c.kmeans_relocations())


def run_lloyd(eng, ctx, case, ref):
    """the case's form at variant 0 (bounds_rate 1 from 2^18 rows on) first; then every other public variant, the other bounds rate
    and every other form"""
    rate = 1.0 if case["rate1"] else None
    out = [("variant 0", lloyd_once(eng, lloyd_ctx(ctx, 0, rate), case, ref, case["form"]))]
    for v in LLOYD_VARIANTS:
        out.append((f"variant {v}", lloyd_once(eng, lloyd_ctx(ctx, v, rate), case, ref, case["form"])))
    out.append(("the other bounds rate", lloyd_once(eng, lloyd_ctx(ctx, 0, None if case["rate1"] else 1.0), case, ref, case["form"])))
    for form in FORMS:
        if form != case["form"]:
            out.append((form, lloyd_once(eng, lloyd_ctx(ctx, 0, rate), case, ref, form)))
    return out


def _inertia_err(case, ref, what, r):
    Xc = ref["X"] - ref["mean"]
    d = Xc.astype(L) - r["C"][r["labels"]].astype(L)
    want = (d * d).sum()
    e = float(abs(L(r["inertia"]) - want) / want) if want > 0 else (0.0 if r["inertia"] == 0.0 else np.inf)
    assert e < TOL_INERTIA, ("lloyd inertia against the long-double sum over the returned labels and centres", what, e, r["inertia"], float(want), case)
    return e


def compare_lloyd(case, ref, got):
    """(worst relative inertia error, 0)"""
    what, a = got[0]
    assert a["n_iter"] == ref["n_iter"], ("lloyd n_iter", a["n_iter"], ref["n_iter"], case)
    bad = int(np.sum(a["labels"] != ref["labels"]))
    assert bad == 0, ("lloyd labels", bad, "of", case["N"], "differ; first", int(np.argmax(a["labels"] != ref["labels"])), case)
    assert a["C"].tobytes() == ref["C"].tobytes(), ("lloyd centres bit for bit", int(np.sum(a["C"] != ref["C"])), "entries differ, worst",
                                                    float(np.max(np.abs(a["C"] - ref["C"]))), case)
    assert a["reloc"] == ref["nreloc"] == a["info"]["relocations"], ("iterations with a relocation", a["reloc"], ref["nreloc"], a["info"], case)
    if "resort" in case["expect"]:
        assert a["info"]["resorts"] > 0, ("the sorted order was to be re-sorted", a["info"], case)
    if "list" in case["expect"]:
        assert a["info"]["list_form_e_steps"] > 0, ("the list form was to run", a["info"], case)
    if not case["expect"]:
        assert a["info"]["resorts"] == 0 and a["info"]["list_form_e_steps"] == 0, ("neither a sort nor a list was expected", a["info"], case)
    worst = _inertia_err(case, ref, what, a)
    for what, r in got[1:]:
        assert r["n_iter"] == a["n_iter"] and r["labels"].tobytes() == a["labels"].tobytes() and r["C"].tobytes() == a["C"].tobytes() and \
            r["reloc"] == a["reloc"], ("lloyd: the same bytes from " + what, r["n_iter"], int(np.sum(r["labels"] != a["labels"])), int(np.sum(r["C"] != a["C"])), case)
        worst = max(worst, _inertia_err(case, ref, what, r))
    return worst, 0.0


PREPARE = dict(colstats=prepare_colstats, kmeanspp=prepare_kmeanspp, lloyd=prepare_lloyd)


def sweep_one(eng, ctx, case, ref):
    """(first figure, second figure) of a case: colstats the worst share of the mean's and of the variance's bound; kmeanspp the indices
    that differ from the reference and from scikit-learn (0, 0); lloyd the worst relative inertia error and 0"""
    fam = case["family"]
    if fam == "colstats":
        return compare_colstats(case, ref, run_colstats(eng, ctx, case, ref))
    if fam == "kmeanspp":
        return compare_kmeanspp(case, ref, run_kmeanspp(eng, ctx, case, ref))
    return compare_lloyd(case, ref, run_lloyd(eng, ctx, case, ref))
