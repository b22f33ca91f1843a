"""The host entry points of csrc/capi.hip (NumPy arrays staged by the library through the ctx arena) against their `_dev` forms on
device arrays: both launch the same kernels on the same shapes, so every output is compared with tobytes().  The `_dev` forms are
called through ctx.lib like the host forms, so that one argument list serves both.  The EDMDc and k-means entry points that exist
in one form only are called alone in a fresh context and behind a much larger call (alone_and_behind).

Every case runs in two fresh contexts (one per form) and makes its call twice in each: the first call grows the arena, the second
reuses it, and both give the same bytes.  Output buffers start from a pattern, so what a call leaves unwritten is compared too.

Shapes are the smallest that reach every staging branch: B = 3 trajectories, T = 5 steps at stride 2 (3 stored rows), P = 3
vehicles of tests/fossen_vehicles.py, N = 70 rows at H = 5 (65 windows: two scan chunks of 64, the second with one window)."""
import ctypes
import os

import numpy as np
import pytest

import fossen_vehicles as fv
import feedback_ref as fr
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

THR, WE, WQ = 0, 1, 2
EULER, RK4 = 0, 1
BTU, TUB, TPB = 0, 1, 2
NX, NU = {THR: 12, WE: 12, WQ: 13}, {THR: 8, WE: 6, WQ: 6}
DT, PAT = 0.02, -7.25
B, T, STRIDE, ROWS = 3, 5, 2, 3
NAMES = ("V1", "V5", "V7")
P = len(NAMES)
N, H = 70, 5
OFF = np.array([0, 40, 43, 113], dtype=np.int64)          # bags of 40, 3 and 70 rows: 35 + 0 + 65 = 100 windows
W_RAGGED = 100


class Buf:
    """an array argument: staged by the library in the host form, a DevArray in the `_dev` form; out = compared afterwards.
    host = True: host memory in both forms (ptr: the ctypes type the binding declares a pointer to, where it is not void)"""

    def __init__(self, name, a, out, dtype=np.float64, host=False, ptr=None):
        self.name, self.a, self.out, self.host, self.ptr = name, np.ascontiguousarray(a, dtype=dtype), out, host, ptr


def I(a):
    return Buf(None, a, False)


def O(name, *shape):
    return Buf(name, np.full(shape, PAT), True)


def IO(name, a):
    return Buf(name, a, True)


def _call(ctx, name, args):
    """one call of ctx.lib.<name>; the outputs by name"""
    from bluerov2_dynamics_amd import engine
    ctx.use_null_stream()
    live, cargs = [], []
    for a in args:
        if isinstance(a, Buf):
            dev = name.endswith("_dev") and not a.host
            h = engine.DevArray.from_host(ctx, a.a, a.a.dtype) if dev else a.a.copy()
            live.append((a, h, dev))
            cargs.append(h.ptr if dev else h.ctypes.data_as(ctypes.POINTER(a.ptr)) if a.ptr else h.ctypes.data)
        else:
            cargs.append(a)
    rc = getattr(ctx.lib, name)(ctx.h, *cargs)
    assert rc == 0, (name, rc, ctx.lib.brov_last_error(ctx.h))
    ctx.sync()
    return {a.name: (h.numpy() if dev else h) for a, h, dev in live if a.out}


def both(name, host_args, dev_args=None, setup=None, view=None, after=None):
    """host form and `_dev` form, twice each in a fresh context: the outputs both forms have agree byte for byte (view[name]: the
    part of that output which is compared; after(ctx): called behind the two calls of a form).  Returns the host form's outputs."""
    from bluerov2_dynamics_amd import _lib
    res = []
    for nm, args in ((name, host_args), (name + "_dev", dev_args or host_args)):
        ctx = _lib.Context(0)
        try:
            if setup:
                setup(ctx)
            first, second = _call(ctx, nm, args), _call(ctx, nm, args)
            if after:
                after(ctx)
        finally:
            ctx.close()
        for k in first:
            assert first[k].tobytes() == second[k].tobytes(), (nm, k, "second call in the same context")
        res.append(first)
    host, dev = res
    common = [k for k in host if k in dev]
    assert common
    for k in common:
        part = (view or {}).get(k, lambda a: a)
        assert part(host[k]).tobytes() == part(dev[k]).tobytes(), (name, k)
    return host


def written(a):
    return not np.any(a == PAT)


def states(rng, model, *lead):
    x = rng.uniform(-0.5, 0.5, lead + (NX[model],))
    if model == WQ:
        x[..., 3:7] /= np.linalg.norm(x[..., 3:7], axis=-1, keepdims=True)
    return x


def controls(rng, model, *lead):
    s = np.ones(8) if model == THR else np.array([10.0, 10.0, 10.0, 0.5, 0.5, 0.5])
    return rng.uniform(-0.3, 0.3, lead + (NU[model],)) * s


def param_array(names=NAMES):
    from bluerov2_dynamics_amd import _lib
    return (_lib.BrovParams * len(names))(*[fv.params(n) for n in names])


def own_vehicle(ctx):
    ctx.set_params(fv.params("V7"))


def pinc_weights(ctx):
    from bluerov2_dynamics_amd.pinc import PINcWeights
    blob = PINcWeights(os.path.join(GOLDEN, "pinc_weights.npz")).blob
    ctx.check(ctx.lib.brov_pinc_set_weights(ctx.h, blob.ctypes.data, int(blob.size)), "brov_pinc_set_weights")
    own_vehicle(ctx)


# ------------------------------------------------------------------------------------------ brov_rollout
@pytest.mark.parametrize("model,layout,steps,traj", [(THR, BTU, T, True), (THR, TUB, T, True), (WQ, TPB, T, True), (THR, BTU, T, False),
                                                    (THR, TUB, 0, True)])
def test_rollout(model, layout, steps, traj):
    """the thruster model with lag_io under BTU and TUB; the quaternion model under TPB, where nx = 13 pads to 14 and the trajectory
    buffer has the padded width (the pad element of a row pair is unused and not compared); traj = NULL; T = 0, where U is never
    copied"""
    rng = np.random.default_rng(11)
    nx, nu = NX[model], NU[model]
    nxw, nuw = (nx + 1) // 2 * 2 if layout == TPB else nx, (nu + 1) // 2 * 2 if layout == TPB else nu
    rows = steps // STRIDE + 1
    x0, U, lag = states(rng, model, B), rng.uniform(-0.3, 0.3, (B * steps * nuw,)), rng.uniform(-1, 1, (B, 8, 3))
    args = [model, RK4, 0, layout, B, steps, DT, I(x0), I(U), IO("lag", lag) if model == THR else None,
            O("traj", B * rows * nxw) if traj else None, STRIDE, O("xT", B, nx)]

    def real_channels(t):       # TPB: [rows][7][B][2] without the pad element of the last pair
        t = t.reshape(rows, nxw // 2, B, 2)
        return np.concatenate([t[:, :-1].reshape(rows, -1), t[:, -1, :, 0]], axis=1)

    r = both("brov_rollout", args, view=dict(traj=real_channels) if layout == TPB else None)
    if steps:
        assert written(r["xT"]) and (model != THR or r["lag"].tobytes() != lag.tobytes())
        assert not traj or written(real_channels(r["traj"]) if layout == TPB else r["traj"])


# ------------------------------------------------------------------------------------------ brov_rhs, brov_thruster_forces
def _host_call(ctx, name, *args):
    rc = getattr(ctx.lib, name)(ctx.h, *args)
    assert rc == 0, (name, rc, ctx.lib.brov_last_error(ctx.h))


@pytest.mark.parametrize("with_lag", [True, False])
def test_rhs_across_the_staging_threshold(with_lag):
    """B = 17 is the first size staged through the arena; 16 rows and then one more go through the pinned, mapped block.  The same
    per-row kernel either way: the 17 rows agree byte for byte."""
    from bluerov2_dynamics_amd import _lib
    rng = np.random.default_rng(12)
    n = 17
    x, u, lag = states(rng, THR, n), controls(rng, THR, n), rng.uniform(-1, 1, (n, 8, 3))
    ctx = _lib.Context(0)
    try:
        own_vehicle(ctx)
        ctx.use_null_stream()
        outs = []
        for _ in range(2):
            xd, l = np.full((n, 12), PAT), lag.copy()
            _host_call(ctx, "brov_rhs", THR, n, x.ctypes.data, u.ctypes.data, DT, l.ctypes.data if with_lag else None, xd.ctypes.data)
            outs.append((xd, l))
        xs, ls = np.full((n, 12), PAT), lag.copy()
        for a, b in ((0, 16), (16, 17)):
            _host_call(ctx, "brov_rhs", THR, b - a, x[a:b].ctypes.data, u[a:b].ctypes.data, DT, ls[a:b].ctypes.data if with_lag else None,
                       xs[a:b].ctypes.data)
    finally:
        ctx.close()
    for xd, l in outs:
        assert written(xd) and xd.tobytes() == xs.tobytes() and l.tobytes() == ls.tobytes()
    assert (ls.tobytes() != lag.tobytes()) == with_lag


def test_thruster_forces_across_the_staging_threshold():
    from bluerov2_dynamics_amd import _lib
    rng = np.random.default_rng(13)
    n = 17
    u, lag = controls(rng, THR, n), rng.uniform(-1, 1, (n, 8, 3))
    ctx = _lib.Context(0)
    try:
        own_vehicle(ctx)
        ctx.use_null_stream()
        outs = []
        for _ in range(2):
            tau, l = np.full((n, 6), PAT), lag.copy()
            _host_call(ctx, "brov_thruster_forces", n, u.ctypes.data, DT, l.ctypes.data, tau.ctypes.data)
            outs.append((tau, l))
        ts, ls = np.full((n, 6), PAT), lag.copy()
        for a, b in ((0, 16), (16, 17)):
            _host_call(ctx, "brov_thruster_forces", b - a, u[a:b].ctypes.data, DT, ls[a:b].ctypes.data, ts[a:b].ctypes.data)
    finally:
        ctx.close()
    for tau, l in outs:
        assert written(tau) and tau.tobytes() == ts.tobytes() and l.tobytes() == ls.tobytes()
    assert ls.tobytes() != lag.tobytes()


# ------------------------------------------------------------------------------------------ the window evaluator
def recording(rows):
    rng = np.random.default_rng(14)
    return states(rng, THR, rows), controls(rng, THR, rows)


@pytest.mark.parametrize("per_window", [True, False])
@pytest.mark.parametrize("carry", [1, 0])
def test_window_se(carry, per_window):
    X, U = recording(N)
    head = [THR, RK4, N, H, DT, I(X), I(U), carry, O("total", 1)]
    r = both("brov_window_endpoint_se", head + [O("per_window", N - H) if per_window else None], head + [O("per_window", N - H)],
             setup=own_vehicle)
    assert written(r["total"]) and r["total"][0] > 0 and (not per_window or written(r["per_window"]))


@pytest.mark.parametrize("per_window", [True, False])
@pytest.mark.parametrize("carry", [1, 0])
def test_window_se_ragged(carry, per_window):
    X, U = recording(int(OFF[-1]))
    head = [THR, RK4, len(OFF) - 1, OFF.ctypes.data, H, DT, I(X), I(U), carry, O("total", 1)]
    r = both("brov_window_endpoint_se_ragged", head + [O("per_window", W_RAGGED) if per_window else None], head + [O("per_window", W_RAGGED)],
             setup=own_vehicle)
    assert written(r["total"]) and r["total"][0] > 0 and (not per_window or written(r["per_window"]))


def test_window_se_without_windows():
    """N == H: the total is 0 and nothing else is written"""
    X, U = recording(H)
    r = both("brov_window_endpoint_se", [THR, RK4, H, H, DT, I(X), I(U), 1, O("total", 1), O("per_window", 4)], setup=own_vehicle)
    assert r["total"][0] == 0.0 and np.all(r["per_window"] == PAT)
    off = np.array([0, H, 2 * H - 1], dtype=np.int64)
    r = both("brov_window_endpoint_se_ragged", [THR, RK4, 2, off.ctypes.data, H, DT, I(X), I(U), 1, O("total", 1), O("per_window", 4)],
             setup=own_vehicle)
    assert r["total"][0] == 0.0 and np.all(r["per_window"] == PAT)


@pytest.mark.parametrize("endpoints", [True, False])
@pytest.mark.parametrize("carry", [1, 0])
def test_window_pop(carry, endpoints):
    X, U = recording(N)
    r = both("brov_window_endpoint_pop", [THR, RK4, P, param_array(), N, H, DT, I(X), I(U), carry, O("se", P),
                                          O("endpoints", P, N - H, 12) if endpoints else None])
    assert written(r["se"]) and len(set(r["se"])) == P and (not endpoints or written(r["endpoints"]))


@pytest.mark.parametrize("endpoints,target,own_per_window", [(True, True, True), (False, False, False), (False, True, False)])
@pytest.mark.parametrize("carry", [1, 0])
def test_window_pop_ragged(carry, endpoints, target, own_per_window):
    """... and the `_dev` form once with d_per_window given and once with arena scratch in its place"""
    X, U = recording(int(OFF[-1]))
    head = [THR, RK4, P, param_array(), len(OFF) - 1, OFF.ctypes.data, H, DT, I(X), I(U), carry, O("se", P),
            O("endpoints", P, W_RAGGED, 12) if endpoints else None, O("target", W_RAGGED, 12) if target else None]
    r = both("brov_window_endpoint_pop_ragged", head, head + [O("per_window", P, W_RAGGED) if own_per_window else None])
    assert written(r["se"]) and len(set(r["se"])) == P
    assert (not endpoints or written(r["endpoints"])) and (not target or written(r["target"]))


def test_window_pop_ragged_target_alone():
    """P = 0: the targets of the windows and nothing else"""
    X, U = recording(int(OFF[-1]))
    head = [THR, RK4, 0, None, len(OFF) - 1, OFF.ctypes.data, H, DT, I(X), None, 1, O("se", 2), None, O("target", W_RAGGED, 12)]
    r = both("brov_window_endpoint_pop_ragged", head, head + [None])
    assert written(r["target"]) and np.all(r["se"] == PAT)
    rows = np.array([a + k for a, b in zip(OFF[:-1], OFF[1:]) for k in range(max(int(b - a) - H, 0))])
    assert r["target"].tobytes() == X[rows + H].tobytes()


# ------------------------------------------------------------------------------------------ brov_rollout_pop, brov_rollout_feedback
@pytest.mark.parametrize("per_candidate,traj", [(0, True), (1, True), (0, False)])
def test_rollout_pop(per_candidate, traj):
    rng = np.random.default_rng(15)
    lead = (P, B) if per_candidate else (B,)
    x0, U, lag = states(rng, THR, *lead), controls(rng, THR, *lead, T), rng.uniform(-1, 1, (P, B, 8, 3))
    r = both("brov_rollout_pop", [THR, RK4, 0, P, param_array(), per_candidate, B, T, DT, I(x0), I(U), IO("lag", lag),
                                  O("traj", P, B, ROWS, 12) if traj else None, STRIDE, O("xT", P, B, 12)])
    assert written(r["xT"]) and r["lag"].tobytes() != lag.tobytes() and (not traj or written(r["traj"]))
    assert r["xT"][0].tobytes() != r["xT"][1].tobytes()


def feedback_records(n):
    rng = np.random.default_rng(16)
    laws = [fr.law(8, K=rng.normal(0, 0.2, (8, 12)), Ki=rng.normal(0, 0.05, (8, 6)), u_min=-0.6, u_max=0.7, z_max=2.0, hold=2) for _ in range(n)]
    from bluerov2_dynamics_amd import _lib
    return (_lib.BrovFeedback * n)(*[fr.to_struct(l) for l in laws])


@pytest.mark.parametrize("nfb,ref_rows,u_ff,given", [(1, 1, False, "zum"), (P, T, True, "zum"), (P, 1, True, ""), (1, T, False, ""),
                                                   (P, T, True, "um"), (1, 1, True, "zm"), (1, T, False, "zu")])
def test_rollout_feedback(nfb, ref_rows, u_ff, given):
    """given: which of z_io (z), u_applied (u) and metrics (m) are passed; the others are NULL -- all, none, and each one alone
    missing beside the other two"""
    rng = np.random.default_rng(17)
    x0, ref, uff = states(rng, THR, B), states(rng, THR, B, ref_rows), controls(rng, THR, B, T)
    lag, z = rng.uniform(-1, 1, (P, B, 8, 3)), rng.uniform(-0.1, 0.1, (P, B, 6))
    r = both("brov_rollout_feedback", [THR, RK4, 0, P, param_array(), nfb, feedback_records(nfb), 0, B, T, DT, I(x0), I(uff) if u_ff else None,
                                       I(ref), ref_rows, IO("lag", lag), IO("z", z) if "z" in given else None, O("traj", P, B, ROWS, 12), STRIDE,
                                       O("xT", P, B, 12), O("u_applied", P, B, T, 8) if "u" in given else None,
                                       O("metrics", P, B, 4) if "m" in given else None])
    assert set(r) == {"lag", "traj", "xT"} | {k for k, v in (("z", "z"), ("u_applied", "u"), ("metrics", "m")) if v in given}
    assert all(written(v) for v in r.values()) and r["lag"].tobytes() != lag.tobytes()
    assert "z" not in given or r["z"].tobytes() != z.tobytes()


# ------------------------------------------------------------------------------------------ PINc, the thruster stream
@pytest.mark.parametrize("with_lag", [True, False])
def test_pinc_rollout(with_lag):
    rng = np.random.default_rng(18)
    x0, U, lag = states(rng, THR, B), controls(rng, THR, B, T), rng.uniform(-1, 1, (B, 8, 3))
    r = both("brov_pinc_rollout", [B, T, DT, I(x0), I(U), IO("lag", lag) if with_lag else None, O("traj", B, ROWS, 12), STRIDE, O("xT", B, 12)],
             setup=pinc_weights)
    assert all(written(v) for v in r.values()) and (not with_lag or r["lag"].tobytes() != lag.tobytes())


@pytest.mark.parametrize("carry,with_lag,starts", [(1, True, True), (0, True, False), (1, False, True), (0, False, False), (0, True, True)])
def test_pinc_window(carry, with_lag, starts):
    """U has N - 1 rows only, the shape the header allows (window k reads U[k .. k + H - 1]).  This exercises that shape; it cannot
    catch a host form that reads row N - 1, since 64 bytes past a NumPy array go unnoticed.  lag_io = NULL starts from a zeroed lag
    state (the `_dev` form is given zeros).  lag_starts is written with carry_lag only: given without it, it comes back untouched."""
    X, U = recording(N)
    rng = np.random.default_rng(19)
    lag = rng.uniform(-1, 1, 24)
    head = [N, H, DT, I(X), I(U[:N - 1]), carry]
    tail = [O("total", 1), O("per_window", N - H), O("lag_starts", N - H, 24) if starts else None]
    r = both("brov_pinc_window_endpoint_se", head + [IO("lag", lag) if with_lag else None] + tail,
             head + [IO("lag", lag if with_lag else np.zeros(24))] + tail, setup=pinc_weights)
    assert written(r["total"]) and written(r["per_window"])
    assert not starts or (written(r["lag_starts"]) if carry else np.all(r["lag_starts"] == PAT))
    if with_lag:
        assert (r["lag"].tobytes() != lag.tobytes()) == bool(carry)


def test_thruster_stream():
    rng = np.random.default_rng(20)
    n = 65
    U, lag = controls(rng, THR, n), rng.uniform(-1, 1, 24)
    r = both("brov_thruster_stream", [n, I(U), DT, IO("lag", lag), O("tau", n, 6)], setup=own_vehicle)
    assert written(r["tau"]) and r["lag"].tobytes() != lag.tobytes()


# ------------------------------------------------------------------------------------------ EDMDc and k-means
# n = 12 states, r = 8 inputs, k = 20 centres (the feature tiles have padding columns), 64 rows per lifted chunk.  A fresh context's
# arena is exactly what the call's layout declared: a take that the layout missed fails with BROV_ERR_NOMEM, a kernel that counted
# on bytes behind the last take reads something else in the second call or in the other form.
EN, ER, EK, GAMMA = 12, 8, 20, 1.0
EP, ED = EN + EK + ER, EN + EK
UNI = dict(nbags=3, L=37, xs=40, us=38)                                  # 3 bags of 37 pairs, gap rows between them: 117 pair rows = 64 + 53
RAG = np.array([0, 40, 41, 41, 113], dtype=np.int64)                     # a one-row bag, an empty bag, a bag across the chunk edge: 64 + 48


def chunk64(ctx):
    ctx.check(ctx.lib.edmdc_set_chunk_rows(ctx.h, 64), "edmdc_set_chunk_rows")


def H_(name, a, dtype=np.float64, ptr=None):
    """a host array in both forms, compared afterwards"""
    return Buf(name, a, True, dtype, host=True, ptr=ptr)


def edmdc_data(layout):
    rng = np.random.default_rng(21)
    xrows, urows = ((UNI["nbags"] - 1) * UNI["xs"] + UNI["L"] + 1, (UNI["nbags"] - 1) * UNI["us"] + UNI["L"]) if layout == "uniform" else (int(RAG[-1]),) * 2
    return np.cumsum(rng.normal(0, 0.05, (xrows, EN)), 0), rng.uniform(-1, 1, (urows, ER)), rng.normal(0, 0.4, (EK, EN)), rng


def bag_args(layout):
    return [UNI["nbags"], UNI["L"], UNI["xs"], UNI["us"]] if layout == "uniform" else [len(RAG) - 1, RAG.ctypes.data]


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("layout", ["uniform", "ragged"])
def test_gram(layout, accumulate):
    """accumulate = 1 adds to a non-zero G^T G / G^T Y; the ragged `_dev` form once more without G^T Y (the task table of G^T G alone)"""
    X, U, C, rng = edmdc_data(layout)
    G0, Y0 = rng.normal(size=(EP, EP)), rng.normal(size=(EP, ED))
    name = "edmdc_gram" if layout == "uniform" else "edmdc_gram_ragged"
    outs = [IO("GtG", G0), IO("GtY", Y0)] if accumulate else [O("GtG", EP, EP), O("GtY", EP, ED)]
    head = [EN, ER, EK, GAMMA, I(C)] + bag_args(layout) + [I(X), I(U), accumulate]
    r = both(name, head + outs, setup=chunk64)
    assert written(r["GtG"]) and written(r["GtY"]) and (accumulate or np.array_equal(r["GtG"], r["GtG"].T))
    assert not accumulate or (r["GtG"].tobytes() != G0.tobytes() and r["GtY"].tobytes() != Y0.tobytes())
    if layout == "ragged":
        from bluerov2_dynamics_amd import _lib
        ctx = _lib.Context(0)
        try:
            chunk64(ctx)
            alone = _call(ctx, name + "_dev", head + [outs[0], None])
        finally:
            ctx.close()
        assert alone["GtG"].tobytes() == r["GtG"].tobytes()


@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("layout", ["uniform", "ragged"])
def test_pinv_apply(layout, variant):
    """P is a host array in both forms"""
    X, U, C, rng = edmdc_data(layout)
    P = rng.normal(size=(EP, EP)) / np.sqrt(EP)

    def setup(ctx):
        chunk64(ctx)
        ctx.set_apply_variant(variant)

    name = "edmdc_pinv_apply" if layout == "uniform" else "edmdc_pinv_apply_ragged"
    r = both(name, [EN, ER, EK, GAMMA, I(C)] + bag_args(layout) + [I(X), I(U), P.ctypes.data, O("M", EP, ED)], setup=setup)
    assert written(r["M"])


def lloyd_data(k, empty=False):
    rng = np.random.default_rng(22)
    X = np.cumsum(rng.normal(0, 0.05, (300, EN)), 0)
    C0 = X[rng.choice(300, k, replace=False)].copy()
    if empty:
        C0[1] += 100.0                                    # tests/test_gpu_parity.py: test_lloyd_empty_clusters_follow_sklearn -- a far initial centre
    return X, C0


@pytest.mark.parametrize("k,mean,empty,host_labels", [(5, True, False, True), (5, False, False, False), (5, True, True, True), (64, True, False, True)])
def test_kmeans_lloyd(k, mean, empty, host_labels):
    """with and without a mean; labels = NULL in the host form (arena scratch takes their place); an initial centre far from all
    samples leaves its cluster empty, so that kmeans_relocate and its own allocations run beside the bound arena; k = 64 takes the
    candidate filter's buffers.  inertia and n_iter are host scalars in both forms."""
    X, C0 = lloyd_data(k, empty)
    m = X.mean(0) if mean else None
    if mean:
        C0 = C0 - m
    mp, seen = None if m is None else m.ctypes.data, []
    labels = Buf("labels", np.full(300, -7), True, np.int32)
    tail = [H_("inertia", np.full(1, PAT), ptr=ctypes.c_double), H_("n_iter", np.full(1, -7), np.int32, ptr=ctypes.c_int)]
    r = both("edmdc_kmeans_lloyd", [300, EN, k, I(X), mp, IO("C", C0), 20, 0.0, labels if host_labels else None] + tail,
             [300, EN, k, I(X), EN, mp, IO("C", C0), 20, 0.0, labels] + tail, after=lambda ctx: seen.append(ctx.kmeans_relocations()))
    assert r["C"].tobytes() != C0.tobytes() and r["inertia"][0] > 0 and 1 <= r["n_iter"][0] <= 20
    assert not host_labels or np.all((r["labels"] >= 0) & (r["labels"] < k))
    assert all(v >= 1 for v in seen) if empty else seen == [0, 0]


def alone_and_behind(name, args, bigger, setup=None):
    """twice alone in a fresh context, and once in a context whose arena a much larger call has grown: the same bytes all three times --
    nothing depends on what lies behind the arena's last take.  Returns the outputs."""
    from bluerov2_dynamics_amd import _lib
    res = []
    for first in (args, bigger):
        ctx = _lib.Context(0)
        try:
            if setup:
                setup(ctx)
            res += [_call(ctx, name, first), _call(ctx, name, args)]
        finally:
            ctx.close()
    a, b, _, c = res
    for k in a:
        assert a[k].tobytes() == b[k].tobytes() == c[k].tobytes(), (name, k)
    return a


def sweep_case(family, pick=None):
    import sweep_cases as sc
    return next(c for c in sc.cases(family) if pick is None or pick(c))


def test_lift_alone():
    c = sweep_case("lift")

    def args(N, n, k):
        rng = np.random.default_rng(23)
        return [N, n, k, c["gamma"], I(rng.uniform(-0.5, 0.5, (N, n))), I(rng.uniform(-0.5, 0.5, (k, n))), O("Z", N, n + k)]

    r = alone_and_behind("edmdc_lift", args(c["N"], c["n"], c["k"]), args(3000, 12, 300))
    assert written(r["Z"])


def multistep_args(c, N, want_xhat, linear):
    import sweep_run as sr
    from bluerov2_dynamics_amd import engine
    rng = np.random.default_rng(24)
    n, r, k, Hh = c["n"], c["r"], c["k"], c["H"]
    C, gamma, A, B = sr.koopman_model(rng, n, r, k)
    X, U = rng.uniform(-0.5, 0.5, (N, n)), rng.uniform(-1, 1, (max(N - 1, 1), r))       # the shape the header allows: N - 1 rows of U
    model = [I(m) if m.size else None for m in engine.linear_coefficients(A, B, n, Hh)] if linear else [I(A), I(B)]
    return [n, r, k, gamma, I(C)] + model + [N, Hh, I(X), I(U), O("se", 1), O("xhat", N - Hh, n) if want_xhat else None]


@pytest.mark.parametrize("want_xhat", [True, False])
@pytest.mark.parametrize("two_groups", [False, True])
@pytest.mark.parametrize("name", ["edmdc_multistep_se", "edmdc_multistep_se_linear"])
def test_multistep_alone(name, two_groups, want_xhat):
    """the family's first case, and its first with H > 1 and 1921 windows or more (16 window blocks: two stream groups)"""
    c = sweep_case("multistep", (lambda c: c["nw"] >= 1921 and c["H"] > 1) if two_groups else None)
    linear = name.endswith("linear")
    r = alone_and_behind(name, multistep_args(c, c["N"], want_xhat, linear), multistep_args(dict(c, H=max(c["H"], 2)), 6000, True, linear))
    assert written(r["se"]) and (not want_xhat or written(r["xhat"]))


def test_simulate_alone():
    import sweep_run as sr
    c = sweep_case("simulate")

    def args(nb, T):
        rng = np.random.default_rng(25)
        C, gamma, A, B = sr.koopman_model(rng, c["n"], c["r"], c["k"])
        return [c["n"], c["r"], c["k"], gamma, I(C), I(A), I(B), nb, T, I(rng.uniform(-0.5, 0.5, (nb, c["n"]))),
                I(rng.uniform(-1, 1, (nb, T, c["r"]))) if T else None, O("Xp", nb, T + 1, c["n"])]

    r = alone_and_behind("edmdc_simulate", args(c["nb"], c["T"]), args(700, 9))
    assert written(r["Xp"])


def test_col_stats_alone():
    """X is a device array; mean and variance are host arrays"""
    c = sweep_case("colstats")

    def args(N, n):
        X = np.random.default_rng(26).normal(size=(N, n))
        return [N, n, I(X), n, H_("mean", np.full(n, PAT)), H_("var", np.full(n, PAT))]

    r = alone_and_behind("edmdc_col_stats_dev", args(c["N"], c["n"]), args(70000, 12))
    assert written(r["mean"]) and written(r["var"])


def test_kmeanspp_alone():
    """X and C are device arrays; the mean, the uniforms and the indices are host arrays"""
    c = sweep_case("kmeanspp")
    keep = []

    def args(N, n, k, trials):
        rng = np.random.default_rng(27)
        X = rng.normal(size=(N, n))
        keep.extend([X.mean(0), rng.uniform(0, 1, (max(k - 1, 1), trials))])
        return [N, n, k, I(X), n, keep[-2].ctypes.data, c["first"], trials, keep[-1].ctypes.data if k > 1 else None, O("C", k, n),
                H_("ind", np.full(k, -7), np.int64)]

    r = alone_and_behind("edmdc_kmeanspp_dev", args(c["N"], c["n"], c["k"], c["trials"]), args(5000, 12, 16, 3))
    assert written(r["C"]) and np.all((r["ind"] >= 0) & (r["ind"] < c["N"]))
