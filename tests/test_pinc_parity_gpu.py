"""PINc kernels (csrc/pinc.hip through pinc.py / engine.py) against the fp64 NumPy oracle (oracle/pinc_numpy.py) where the fixture
tests (test_pinc_gpu.py) do not reach: batches and window counts across the grid-stride cap of 2048 waves, the 8-bank lag scan at
many sizes, random weight sets (beta 8 / 0.05 / -0.5, LayerNorm variance ~ eps, cos/sin at the clamp), the recorded size, the
device entry points, the per-context dt and weight caches, and a U one row shorter than X.

Tolerances calibrate themselves: the kernel may differ from the fp64 oracle by TOL_MULT times what the oracle's own fp32 mode differs
from fp64 on the same inputs, plus FLOOR (a mixed error, conftest.rel_err).  Multi-step rollouts get STEP_MULT: the dynamics amplify
each step's rounding, and the kernel's fp32 sums (other orders than NumPy's) land up to ~3x the oracle's fp32 deviation at T = 20.
The thruster lag is fp64 in both: 1e-12."""
import numpy as np
import pytest
import torch  # noqa: F401  (imported before the first HIP context: torch tensors are operands of the _dev entry points below)

from conftest import load_golden, rel_err

pytestmark = pytest.mark.gpu

TOL_MULT, STEP_MULT, FLOOR = 4.0, 8.0, 5e-6
WAVES = 2048                                     # PINC_MAX_WAVES: above it every wave loops


def _tol(o32, o64, mult=TOL_MULT):
    return mult * rel_err(o32, o64) + FLOOR


def _check(name, got, o32, o64, mult=TOL_MULT):
    err, tol = rel_err(got, o64), _tol(o32, o64, mult)
    print(f"[pinc parity] {name}: kernel {err:.2e}  bound {tol:.2e}")
    assert err <= tol, (name, err, tol)


@pytest.fixture(scope="module")
def sets():
    """name -> (PINcWeights, state dict, z pool [n,14] fp32)"""
    from bluerov2_dynamics_amd.pinc import KEYS, PINcWeights
    g = load_golden("pinc_weights.npz")
    out = {"ckpt": (PINcWeights({k: g[k] for k in g.files}), {k: g[k] for k in g.files}, load_golden("pinc_kat.npz")["z"])}
    r = load_golden("pinc_rand_kat.npz")
    for s in range(3):
        sd = {k: r[f"w{s}_{k}"] for k in KEYS}
        out[f"rand{s}"] = (PINcWeights(sd), sd, r[f"z{s}"])
    return out


@pytest.fixture(scope="module")
def cfg5():
    g = load_golden("cfg5.npz")
    return g["X"], g["U"], float(g["dt"])


def _extend(X, U, n):
    """n rows of a synthetic recording: cfg5 tiled, each copy shifted in x/y so that no two windows are alike."""
    reps = -(-n // len(X))
    Xs = np.concatenate([X + np.array([0.37 * i, -0.21 * i] + [0.0] * 10) for i in range(reps)])[:n]
    Us = np.concatenate([U[::(-1) ** i] for i in range(reps)])[:n]
    return np.ascontiguousarray(Xs), np.ascontiguousarray(Us)


def test_forward_every_weight_set_across_the_wave_cap(sets):
    from oracle import pinc_numpy
    from bluerov2_dynamics_amd.pinc import PINc
    rng = np.random.default_rng(1)
    for name, (w, sd, pool) in sets.items():
        z = pool[rng.integers(0, len(pool), 10000)]
        z[WAVES + 5] = z[5]
        o64, o32 = pinc_numpy.forward(sd, z), pinc_numpy.forward(sd, z, fp32=True)
        net = PINc(w)
        for B in (1, 63, 64, 2047, 2048, 2049, 4097, 10000):
            y = net.forward(z[:B])
            assert y.shape == (B, 9) and y.dtype == np.float32
            _check(f"forward {name} B={B}", y, o32[:B], o64[:B])
        assert np.array_equal(y[5], y[WAVES + 5])                   # row b and b + 2048: one wave's two rounds, the same bits
        assert PINc(w).forward(np.zeros((0, 14))).shape == (0, 9)


def test_rollout_edges_across_the_wave_cap(sets, cfg5):
    from oracle import pinc_numpy
    from bluerov2_dynamics_amd.pinc import PINc
    X, _, dt = cfg5
    rng = np.random.default_rng(2)
    B = WAVES + 1
    x0 = X[rng.integers(0, len(X), B)]
    U = rng.uniform(-1, 1, (B, 20, 8))
    lag0 = rng.normal(0, 0.5, (B, 8, 3))
    grid = [("ckpt", T) for T in (0, 1, 2, 7, 20)] + [(f"rand{s}", 7) for s in range(3)]
    for name, T in grid:
        w, sd, _ = sets[name]
        net = PINc(w)
        for lag in (None, lag0):
            o64 = pinc_numpy.rollout(sd, x0, U[:, :T], dt, lag=lag)
            o32 = pinc_numpy.rollout(sd, x0, U[:, :T], dt, lag=lag, fp32=True)
            for stride in sorted({1, 3, max(T, 1), T + 1}):
                for store in (True, False):
                    r = net.rollout(x0, U[:, :T], dt, lag=lag, stride=stride, store=store)
                    tag = f"rollout {name} T={T} stride={stride} lag={'given' if lag is not None else 'None'}"
                    if store:
                        assert r["traj"].shape == (B, T // stride + 1, 12)
                        _check(tag + " traj", r["traj"], o32["traj"][:, ::stride], o64["traj"][:, ::stride], STEP_MULT)
                    else:
                        assert r["traj"] is None
                    _check(tag + " xT", r["xT"], o32["xT"], o64["xT"], STEP_MULT)
                    assert rel_err(r["lag"], o64["lag"]) < 1e-12
                    if T == 0:
                        assert np.array_equal(r["xT"], x0) and np.array_equal(r["lag"], np.zeros((B, 8, 3)) if lag is None else lag0)
                        if store:
                            assert np.array_equal(r["traj"][:, 0], x0)


def test_rollout_8192_by_50_on_a_sample(sets, cfg5):
    from oracle import pinc_numpy
    from bluerov2_dynamics_amd.pinc import PINc
    X, _, dt = cfg5
    w, sd, _ = sets["ckpt"]
    rng = np.random.default_rng(3)
    B, T = 8192, 50
    x0 = X[rng.integers(0, len(X), B)]
    U = rng.uniform(-1, 1, (B, T, 8))
    lag0 = rng.normal(0, 0.5, (B, 8, 3))
    r = PINc(w).rollout(x0, U, dt, lag=lag0, stride=5)
    ks = np.unique(np.concatenate([[0, 1, 2047, 2048, 4095, 4096, 6143, 6144, 8191], rng.integers(0, B, 23)]))
    o64 = pinc_numpy.rollout(sd, x0[ks], U[ks], dt, lag=lag0[ks], stride=5)
    o32 = pinc_numpy.rollout(sd, x0[ks], U[ks], dt, lag=lag0[ks], stride=5, fp32=True)
    _check("rollout 8192x50 traj (sample)", r["traj"][ks], o32["traj"], o64["traj"], STEP_MULT)
    assert rel_err(r["lag"][ks], o64["lag"]) < 1e-12


def _window_oracle(sd, X, U, H, dt, lag, carry, ks):
    """fp64 oracle on windows ks and the fp32-mode endpoints from the same starts"""
    from oracle import pinc_numpy
    o = pinc_numpy.window_endpoint_se(sd, X, U, H, dt, lag=lag, carry_lag=carry, windows=ks)
    l0 = o["lag_starts"][ks] if carry else np.broadcast_to(lag, (len(ks), 8, 3))
    Uw = U[ks[:, None] + np.arange(H)[None, :]]
    x32 = pinc_numpy.rollout(sd, X[ks], Uw, dt, lag=l0, store=False, fp32=True)["xT"]
    return o, x32


def _check_windows(name, r, o, x32, ks):
    """sqrt(per_window) is the endpoint-error norm: its error is at most the endpoint difference (triangle inequality)"""
    tol = _tol(x32, o["x_end"], STEP_MULT)
    scale = np.maximum(1.0, np.linalg.norm(o["x_end"], axis=1))
    d = np.abs(np.sqrt(r["per_window"][ks]) - np.sqrt(o["per_window"])) / scale
    err = float(d.max()) if d.size else 0.0
    print(f"[pinc parity] {name}: kernel {err:.2e}  bound {np.sqrt(12) * tol:.2e}")
    assert err <= np.sqrt(12) * tol, (name, err, tol)
    tot = float(np.sum(r["per_window"]))
    assert abs(r["se"] - tot) <= 1e-12 * max(tot, 1e-300)


def test_window_evaluator_edges_across_the_wave_cap(sets, cfg5):
    from oracle import pinc_numpy
    from bluerov2_dynamics_amd.pinc import PINc
    X, U, dt = cfg5
    Xs, Us = _extend(X, U, 4500 + 17)
    rng = np.random.default_rng(4)
    s0 = rng.normal(0, 0.5, (8, 3))
    w, sd, _ = sets["ckpt"]
    net = PINc(w)
    nwins = (1, 63, 64, 65, 129, 2047, 2048, 2049, 4500)
    for H in (0, 1, 3, 17):
        # every window count is a prefix of the longest: one oracle per (H, carry) on the union of the samples
        starts, _ = pinc_numpy.lag_starts(Us, H, dt, 4501, lag=s0)
        pick = np.unique(np.concatenate([[0, 62, 63, 64, 128, 2046, 2047, 2048, 4095, 4499], rng.integers(0, 4500, 20)]))
        for carry in (True, False):
            o, x32 = _window_oracle(sd, Xs[:4500 + H], Us[:4500 + H], H, dt, s0, carry, pick)
            for nwin in nwins:
                N = nwin + H
                r = net.window_endpoint_se(Xs[:N], Us[:N], H, dt, lag=s0, carry_lag=carry, want_lag_starts=True)
                assert r["per_window"].shape == (nwin,)
                sel = pick < nwin
                sub = dict(per_window=o["per_window"][sel], x_end=o["x_end"][sel])
                _check_windows(f"windows nwin={nwin} H={H} carry={carry}", r, sub, x32[sel], pick[sel])
                if carry:
                    assert rel_err(r["lag_starts"], starts[:nwin]) < 1e-12
                    assert rel_err(r["lag"], starts[nwin]) < 1e-12            # the lag after window nwin-1 = window nwin's start
                else:
                    assert r["lag_starts"] is None and np.array_equal(r["lag"], s0)
                if H == 0:
                    assert np.all(r["per_window"] == 0.0)


def test_window_evaluator_at_the_recorded_size(sets, cfg5):
    """45 823 rows, H = 10: 45 813 windows, ~22 per wave"""
    from oracle import pinc_numpy
    from bluerov2_dynamics_amd.pinc import PINc
    X, U, dt = cfg5
    Xs, Us = _extend(X, U, 45823)
    H = 10
    nwin = len(Xs) - H
    s0 = load_golden("pinc_kat.npz")["lag500"]
    w, sd, _ = sets["ckpt"]
    r = PINc(w).window_endpoint_se(Xs, Us, H, dt, lag=s0, want_lag_starts=True)
    rng = np.random.default_rng(5)
    ks = np.unique(np.concatenate([[0, 63, 64, 2047, 2048, 4095, 4096, nwin - 1], rng.integers(0, nwin, 24)]))
    o, x32 = _window_oracle(sd, Xs, Us, H, dt, s0, True, ks)
    _check_windows("windows recorded size H=10 (sample)", r, o, x32, ks)
    assert rel_err(r["lag_starts"], o["lag_starts"]) < 1e-12
    assert rel_err(r["lag"], o["lag"]) < 1e-12


def test_device_entry_points_equal_the_host_ones(sets, cfg5):
    import torch
    from bluerov2_dynamics_amd import _lib, engine
    from bluerov2_dynamics_amd.pinc import PINc, set_weights
    X, U, dt = cfg5
    w, _, pool = sets["rand1"]
    ctx = _lib.default_context()
    net = PINc(w, ctx=ctx)
    rng = np.random.default_rng(6)
    B, T, H = WAVES + 3, 9, 6
    z = pool[rng.integers(0, len(pool), B)]
    x0 = X[rng.integers(0, len(X), B)]
    Ub = rng.uniform(-1, 1, (B, T, 8))
    lag0 = rng.normal(0, 0.5, (B, 8, 3))
    Xw, Uw = _extend(X, U, 2600)
    s0 = rng.normal(0, 0.5, (8, 3))
    y = net.forward(z)
    ro = net.rollout(x0, Ub, dt, lag=lag0, stride=2)
    ro0 = net.rollout(x0, Ub, dt, lag=None, stride=2)
    wo = net.window_endpoint_se(Xw, Uw, H, dt, lag=s0, want_lag_starts=True)
    wo0 = net.window_endpoint_se(Xw, Uw, H, dt, lag=None)
    nwin = len(Xw) - H
    for kind in ("devarray", "torch"):
        set_weights(ctx, w)
        if kind == "devarray":
            up = lambda a, dtype=np.float64: engine.DevArray.from_host(ctx, a, dtype)      # noqa: E731
            new = lambda shape, dtype=np.float64: engine.DevArray(ctx, shape, dtype)      # noqa: E731
            get = lambda d: d.numpy()                                                      # noqa: E731
            sync = lambda: None                                                            # noqa: E731
        else:
            up = lambda a, dtype=np.float64: torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()   # noqa: E731
            new = lambda shape, dtype=np.float64: torch.empty(shape, dtype=getattr(torch, np.dtype(dtype).name), device="cuda")  # noqa: E731
            get = lambda d: d.cpu().numpy()                                                # noqa: E731
            sync = torch.cuda.synchronize
        dy = new((B, 9), np.float32)
        engine.pinc_forward_dev(up(z, np.float32), dy, ctx=ctx)
        sync()
        assert np.array_equal(get(dy), y), kind
        for lag, ref in ((lag0, ro), (None, ro0)):
            dl = None if lag is None else up(lag)
            dtr, dxT = new((B, T // 2 + 1, 12)), new((B, 12))
            engine.pinc_rollout_dev(up(x0), up(Ub), dt, lag=dl, traj=dtr, xT=dxT, stride=2, ctx=ctx)
            sync()
            assert np.array_equal(get(dtr), ref["traj"]) and np.array_equal(get(dxT), ref["xT"]), kind
            if lag is not None:
                assert np.array_equal(get(dl), ref["lag"]), kind
        for lag, ref in ((s0, wo), (None, wo0)):
            dl = None if lag is None else up(lag)
            dse, dper = new((1,)), new((nwin,))
            dst = new((nwin, 8, 3)) if lag is not None else None
            engine.pinc_window_endpoint_se_dev(up(Xw), up(Uw), H, dt, dse, dper, lag=dl, lag_starts=dst, ctx=ctx)
            sync()
            assert np.array_equal(get(dper), ref["per_window"]) and get(dse)[0] == ref["se"], kind
            if lag is not None:
                assert np.array_equal(get(dst), ref["lag_starts"]) and np.array_equal(get(dl), ref["lag"]), kind


def test_one_context_alternating_dt_and_weights(sets, cfg5):
    from oracle import pinc_numpy
    from bluerov2_dynamics_amd import _lib
    from bluerov2_dynamics_amd.pinc import PINc
    X, _, _ = cfg5
    ctx = _lib.default_context()
    rng = np.random.default_rng(7)
    B, T = 300, 12
    x0 = X[rng.integers(0, len(X), B)]
    U = rng.uniform(-1, 1, (B, T, 8))
    lag0 = rng.normal(0, 0.5, (B, 8, 3))
    w, sd, _ = sets["ckpt"]
    net = PINc(w, ctx=ctx)
    for dt in (0.02, 0.05, 0.02):
        r = net.rollout(x0, U, dt, lag=lag0)
        o64 = pinc_numpy.rollout(sd, x0, U, dt, lag=lag0)
        o32 = pinc_numpy.rollout(sd, x0, U, dt, lag=lag0, fp32=True)
        _check(f"rollout dt={dt} (alternating on one context)", r["traj"], o32["traj"], o64["traj"], STEP_MULT)
        assert rel_err(r["lag"], o64["lag"]) < 1e-12
    a, b = PINc(sets["ckpt"][0], ctx=ctx), PINc(sets["rand0"][0], ctx=ctx)
    ra = a.rollout(x0, U, 0.02, lag=lag0)
    rb = b.rollout(x0, U, 0.02, lag=lag0)
    ra2 = a.rollout(x0, U, 0.02, lag=lag0)
    assert not np.array_equal(ra["traj"], rb["traj"])
    assert np.array_equal(ra["traj"], ra2["traj"]) and np.array_equal(ra["lag"], ra2["lag"])


def test_inputs_one_row_shorter_than_states(sets, cfg5):
    """The reference's multistep_rmse_endpoint_pinc reads U[k:k+H] only, rows up to N-2: len(U) == len(X) - 1 works and gives the
    number a padded U gives."""
    from bluerov2_dynamics_amd.fossen.BlueROV2 import BlueROV2
    from bluerov2_dynamics_amd.pinc import PINc, multistep_rmse_endpoint_pinc
    X, U, dt = cfg5
    w, _, _ = sets["ckpt"]
    N = 700
    Xn, Un = X[:N], U[:N]
    for H in (1, 10, 100):
        # a U that ends exactly where the reads end, placed at the end of its own buffer: an over-read would leave the array
        Ushort = np.ascontiguousarray(Un[:N - 1])
        full = PINc(w).window_endpoint_se(Xn, Un, H, dt)
        short = PINc(w).window_endpoint_se(Xn, Ushort, H, dt)
        assert short["se"] == full["se"] and np.array_equal(short["per_window"], full["per_window"])
        rov_a, rov_b = BlueROV2(dt=dt), BlueROV2(dt=dt)
        ma = multistep_rmse_endpoint_pinc(Xn, Un, H, dt, w, rov_a)
        mb = multistep_rmse_endpoint_pinc(Xn, Ushort, H, dt, w, rov_b)
        assert ma == mb and np.array_equal(rov_a._lag, rov_b._lag)
    with pytest.raises(AssertionError):
        PINc(w).window_endpoint_se(Xn, Un[:N - 2], 1, dt)
    with pytest.raises(AssertionError):
        multistep_rmse_endpoint_pinc(Xn, Un[:N - 2], 10, dt, w, BlueROV2(dt=dt))
