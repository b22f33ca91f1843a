"""PINc training kernels (csrc/pinc_train.hip through pinc.py / engine.py) against the fp64 NumPy restatement
(tests/pinc_train_ref.py, itself pinned to the reference's autograd by test_pinc_train_cpu.py).

Tolerances calibrate themselves as in test_pinc_parity_gpu.py: per tensor, the kernel may differ from fp64 by TOL_MULT times what
the restatement's own fp32 mode differs from fp64 on the same inputs, plus FLOOR; STEP_MULT for a run of training iterations.
The four beta GRADIENTS are one-element tensors: each is the sum of 64 terms per row, and the fp32 mode's error on it is a single
draw that lands anywhere below the sum's own error scale, so it is no yardstick.  A beta gradient and the same layer's Linear bias
gradient are sums over the same backpropagated factors; with cancellation of condition c = |t|_1 / |sum t| (from the fp64
restatement's terms) the beta sum cannot be better than c times what those factors are held to.  Its bound is therefore c times the
bound of that bias gradient, c x (TOL_MULT x the bias gradient's fp32-mode error + FLOOR): the same multiple, no other constant.
Where c reaches 1 / eps32 (net.7.beta of the second random set) fp32 cannot know the value and the bound says so; a wrong formula
(a sign error is a relative error of 2) fails in every well-conditioned case, c = 3 .. 1e3 in most.  Measured on the MI355X over
the 63 gradient cases: the worst beta is at 0.43 of its bound (1.4e-5 of 3.3e-5, c = 5.7, first random set, B = 256, K = 10), all
others below 0.2.  Trained beta WEIGHTS are ordinary values and get the ordinary rule."""
import os
import sys

import numpy as np
import pytest
import torch  # noqa: F401  (imported before the first HIP context, as in the other PINc GPU tests)

import pinc_train_ref as R
from conftest import REPO, load_golden, rel_err

pytestmark = pytest.mark.gpu

TOL_MULT, STEP_MULT, FLOOR = 4.0, 8.0, 5e-6
EPS32 = float(np.finfo(np.float32).eps)
SIZES = (1, 2, 63, 64, 254, 256, 1000, 2100)       # 2100 rows: past the cap of 255 batch workgroups x 8 rows


def _per_tensor(name, got, o32, o64, mult, beta_cond=None):
    """per-tensor |got - o64| / |o64| against mult x the fp32 mode's own error + FLOOR; prints the worst tensor of each kind.
    beta_cond (gradients only): the condition numbers of the beta sums, see the module docstring."""
    e_k, e_o = R.tensor_rel_errors(got, o64), R.tensor_rel_errors(o32, o64)
    scale = dict(e_o)
    if beta_cond is not None:
        for k, c in beta_cond.items():
            scale[k] = max(c, 1.0) * (max(e_o[f"net.{int(k.split('.')[1]) - 1}.bias"], EPS32) + FLOOR / mult)
    tol = {k: mult * scale[k] + (0.0 if beta_cond is not None and k in beta_cond else FLOOR) for k in e_k}
    for kind in ("beta", "weight", "bias"):
        worst = max((k for k in e_k if k.endswith(kind)), key=lambda k: e_k[k] / tol[k])
        extra = f", cond {beta_cond[worst]:.1e}" if beta_cond is not None and kind == "beta" else ""
        print(f"[pinc train] {name}: worst {worst} kernel {e_k[worst]:.2e} bound {tol[worst]:.2e} (fp32 mode {e_o[worst]:.2e}{extra})")
    bad = {k: (e_k[k], tol[k]) for k in e_k if e_k[k] > tol[k]}
    assert not bad, (name, bad)


def _scalars(name, got, o32, o64, mult):
    for i, term in enumerate(("mse", "physics", "rollout")):
        err = abs(float(got[i]) - float(o64[i])) / max(abs(float(o64[i])), 1e-30) if o64[i] != 0 else abs(float(got[i]))
        ref = abs(float(o32[i]) - float(o64[i])) / max(abs(float(o64[i])), 1e-30) if o64[i] != 0 else 0.0
        print(f"[pinc train] {name} {term}: kernel {err:.2e} bound {mult * ref + FLOOR:.2e}")
        assert err <= mult * ref + FLOOR, (name, term, err, ref)


@pytest.fixture(scope="module")
def fx():
    d = load_golden("pinc_train.npz")
    ck = load_golden("pinc_weights.npz")
    return dict(d=d, sets=dict(ckpt={k: ck[k] for k in R.KEYS}, fresh={k: d["fresh." + k] for k in R.KEYS}),
                Z=d["z"].astype(np.float32), Y=d["y"].astype(np.float32), U=d["U4"][:-1].astype(np.float32))


@pytest.fixture(scope="module")
def run20(fx):
    """the fp64 and fp32-mode restatements of the fixture's 20 iterations (shared, not modified)"""
    a = (fx["sets"]["fresh"], fx["Z"], fx["Y"], fx["U"], fx["d"]["iters"])
    return R.train(*a), R.train(*a, fp32=True)


def _trainer(sd, **kw):
    from bluerov2_dynamics_amd.pinc import PINcTrainer, PINcWeights
    return PINcTrainer(PINcWeights(sd), **kw)


@pytest.mark.parametrize("wset", ["ckpt", "fresh"])
def test_loss_and_grad_on_the_fixture_batches(fx, wset):
    for b in ("b256", "b254", "b2"):
        idx = fx["d"]["idx_" + b]
        z, y, u = fx["Z"][idx], fx["Y"][idx], fx["U"][idx]
        K = min(10, len(idx) - 1)
        tr = _trainer(fx["sets"][wset])
        loss, g = tr.loss_and_grad(z, y, u)
        tr.close()
        terms = {}
        l64, _, g64 = R.loss_and_grad(fx["sets"][wset], z, y, u, K, terms=terms)
        l32, _, g32 = R.loss_and_grad(fx["sets"][wset], z, y, u, K, fp32=True)
        _per_tensor(f"{wset} {b}", g, g32, g64, TOL_MULT, R.beta_conditions(terms))
        _scalars(f"{wset} {b}", loss, l32, l64, TOL_MULT)


@pytest.mark.parametrize("s", [0, 1, 2])
def test_loss_and_grad_random_weight_sets_every_size(s):
    """beta 8 / 0.05 / -0.5, LayerNorm variance near eps, cos/sin at the clamp; B across one row, one workgroup's share of 8 rows and
    the cap of 255 batch workgroups (B > 2040); K = 0, 1, 10; physics on and off."""
    r = load_golden("pinc_rand_kat.npz")
    sd = {k: r[f"w{s}_{k}"] for k in R.KEYS}
    pool = r[f"z{s}"].astype(np.float32)
    rng = np.random.default_rng(100 + s)
    case = 0
    for B in SIZES:
        z = pool[rng.integers(0, len(pool), B)]
        y = (pool[rng.integers(0, len(pool), B), :9] + rng.normal(0, 0.01, (B, 9))).astype(np.float32)
        u = z[:, 9:13].copy()
        for K in (0, 1, 10):
            if K >= B:
                continue
            phys = bool((case := case + 1) % 2)
            tr = _trainer(sd, rollout_steps=K, use_rollout=K > 0, use_physics=phys)
            loss, g = tr.loss_and_grad(z, y, u)
            tr.close()
            terms = {}
            l64, _, g64 = R.loss_and_grad(sd, z, y, u, K, phys, terms=terms)
            l32, _, g32 = R.loss_and_grad(sd, z, y, u, K, phys, fp32=True)
            _per_tensor(f"rand{s} B={B} K={K} physics={phys}", g, g32, g64, TOL_MULT, R.beta_conditions(terms))
            _scalars(f"rand{s} B={B} K={K}", loss, l32, l64, TOL_MULT)


def test_adamw_step_clip_active_and_inactive(fx):
    """Elementwise: every component within a few fp32 roundings of the fp64 restatement: 8 ulp of the largest magnitude the
    component passes through (the weight before, the update, the weight after: an update that nearly cancels the weight leaves
    the update's rounding, not the result's) for the weights; 8 ulp (mixed) for m and v."""
    from bluerov2_dynamics_amd import _lib, engine
    ctx = _lib.default_context()
    ctx.use_null_stream()
    rng = np.random.default_rng(5)
    w0 = R.flatten(fx["sets"]["ckpt"], np.float32)
    m0 = rng.normal(0, 1e-2, w0.size).astype(np.float32)
    v0 = (rng.uniform(0, 1e-3, w0.size) ** 2).astype(np.float32)
    eps32 = float(np.finfo(np.float32).eps)
    for scale, active in ((1e-3, False), (3.0, True)):
        g = (rng.normal(0, scale, w0.size)).astype(np.float32)
        d = [engine.DevArray.from_host(ctx, a, np.float32) for a in (w0, m0, v0, g)]
        nrm = engine.DevArray(ctx, (1,), np.float32)
        engine.pinc_adamw_step_dev(d[0], d[1], d[2], d[3], 7, norm_out=nrm, ctx=ctx)
        w, m, v, n = d[0].numpy(), d[1].numpy(), d[2].numpy(), float(nrm.numpy()[0])
        assert np.array_equal(d[3].numpy(), g)
        for a in d + [nrm]:
            a.free()
        w64, m64, v64, n64 = R.adamw_step(w0, m0, v0, g, 7)
        assert (n64 > 5.0) == active
        ew = float(np.max(np.abs(w - w64) / np.maximum.reduce([np.abs(w64), np.abs(w0).astype(np.float64), np.abs(w64 - w0)])))
        em, ev = rel_err(m, m64), rel_err(v, v64)
        print(f"[pinc train] adamw clip active={active}: w {ew / eps32:.2f} ulp, m {em / eps32:.2f} ulp, v {ev / eps32:.2f} ulp, norm {abs(n - n64) / n64:.1e}")
        assert ew <= 8 * eps32 and em <= 8 * eps32 and ev <= 8 * eps32 and abs(n - n64) <= 4 * eps32 * n64


def test_twenty_iterations_follow_the_restatement(fx, run20):
    r64, r32 = run20
    tr = _trainer(fx["sets"]["fresh"])
    # the fixture's index lists are 20 minibatches of 256 rows drawn independently: each is an "epoch" over its own 256 rows
    iters = fx["d"]["iters"]
    logs = []
    from bluerov2_dynamics_amd import engine
    for idx in iters:
        sub = [engine.DevArray.from_host(tr.ctx, a[idx], np.float32) for a in (fx["Z"], fx["Y"], fx["U"])]
        logs.append(tr.epoch_on(sub, np.arange(len(idx)))[0])
        for a in sub:
            a.free()
    st = tr.state()
    tr.close()
    assert st["step"] == 20
    _per_tensor("20 iterations, weights", st["blob"], r32["w"], r64["w"], STEP_MULT)
    logs = np.array(logs)
    for i in range(len(logs)):
        _scalars(f"iteration {i + 1}", logs[i], r32["losses"][i], r64["losses"][i], STEP_MULT)
    comp = np.abs(st["blob"].astype(np.float64) - r64["w"])
    share = float(np.mean(comp > 1e-4))
    print(f"[pinc train] 20 iterations: largest component error {comp.max():.2e}, share beyond 1e-4: {share:.2e}")
    assert share <= 1e-3


def test_sessions_are_bit_reproducible_and_resumable(fx):
    Z, Y, U = fx["Z"], fx["Y"], fx["U"]
    rng = np.random.default_rng(9)
    perms = [rng.permutation(len(Z)) for _ in range(2)]

    def run(split):
        tr = _trainer(fx["sets"]["fresh"])
        logs = [tr.epoch(Z, Y, U, perms[0])]
        if split:
            st = tr.state()
            tr.close()
            tr = _trainer(fx["sets"]["ckpt"])
            tr.load_state(st)
        logs.append(tr.epoch(Z, Y, U, perms[1]))
        st = tr.state()
        tr.close()
        return st, np.concatenate(logs)

    (a, la), (b, lb), (c, lc) = run(False), run(False), run(True)
    assert a["step"] == b["step"] == c["step"] == 2 * 7
    for k in ("blob", "m", "v"):
        assert a[k].tobytes() == b[k].tobytes() == c[k].tobytes(), k
    assert la.tobytes() == lb.tobytes() == lc.tobytes() and np.all(np.isfinite(la))


def test_short_last_batches(fx):
    """1599 rows at batch 256 end with 63 rows; 257 rows end with ONE row, whose iteration has no rollout term."""
    Z, Y, U = fx["Z"], fx["Y"], fx["U"]
    for N in (len(Z), 257):
        perm = np.random.default_rng(N).permutation(N)
        lists = [perm[i:i + 256] for i in range(0, N, 256)]
        tr = _trainer(fx["sets"]["fresh"])
        log = tr.epoch(Z[:N], Y[:N], U[:N], perm)
        w = tr.state()["blob"]
        tr.close()
        r64 = R.train(fx["sets"]["fresh"], Z[:N], Y[:N], U[:N], lists)
        r32 = R.train(fx["sets"]["fresh"], Z[:N], Y[:N], U[:N], lists, fp32=True)
        assert log.shape == (len(lists), 3)
        if N == 257:
            assert log[-1, 2] == 0.0 and r64["losses"][-1, 2] == 0.0
        _per_tensor(f"epoch of {N} rows", w, r32["w"], r64["w"], STEP_MULT)
        _scalars(f"epoch of {N} rows, last iteration", log[-1], r32["losses"][-1], r64["losses"][-1], STEP_MULT)


@pytest.mark.parametrize("N", [1, 7, 4096, 45823])
def test_thruster_stream(N):
    from bluerov2_dynamics_amd import engine
    from oracle import pinc_numpy
    rng = np.random.default_rng(N)
    U = rng.uniform(-1, 1, (N, 8))
    lag0 = rng.normal(0, 0.3, (8, 3))
    tau, lag = engine.thruster_stream(U, 0.02, lag=lag0)
    u4, lag_ref = pinc_numpy.thruster_stream(U, 0.02, lag0)
    e1, e2 = rel_err(tau[:, [0, 1, 2, 5]], u4), rel_err(lag, lag_ref)
    print(f"[pinc train] thruster_stream N={N}: u4 {e1:.1e} lag {e2:.1e}")
    assert e1 < 1e-12 and e2 < 1e-12
    if N <= 7:
        l = lag0[None].copy()
        seq = []
        for k in range(N):
            t, l = engine.thruster_forces(U[k:k + 1], 0.02, lag=l)
            seq.append(t[0])
        assert rel_err(tau, np.array(seq)) < 1e-12 and rel_err(lag, l[0]) < 1e-12


def test_errors_are_status_codes(fx):
    from bluerov2_dynamics_amd import _lib, engine
    ctx = _lib.Context(0)
    d = engine.DevArray(ctx, (4, 14), np.float32)
    assert ctx.lib.brov_pinc_train_epoch_dev(ctx.h, 4, d.ptr, d.ptr, d.ptr, d.ptr, d.ptr) == -1          # no trainer
    assert b"brov_pinc_train_begin" in ctx.lib.brov_last_error(ctx.h)
    assert ctx.lib.brov_pinc_loss_grad_dev(ctx.h, d.ptr, 0, d.ptr, d.ptr, d.ptr, 0, 0, d.ptr, d.ptr) == -1   # B < 1
    blob = np.zeros(100, dtype=np.float32)
    h = _lib.PincHyper(3e-3, 0.9, 0.999, 1e-8, 0.01, 5.0, 256, 10, 1, 1)
    import ctypes
    assert ctx.lib.brov_pinc_train_begin(ctx.h, blob.ctypes.data, 100, ctypes.byref(h)) == -1           # wrong blob size
    d.free()


def test_training_leaves_the_inference_weights_alone(fx):
    from bluerov2_dynamics_amd.pinc import PINc, PINcWeights
    net = PINc(PINcWeights(fx["sets"]["ckpt"]))
    z = fx["Z"][:300]
    before = net.forward(z)
    tr = _trainer(fx["sets"]["fresh"], ctx=net.ctx)
    tr.epoch(fx["Z"][:600], fx["Y"][:600], fx["U"][:600], np.arange(600))
    during = net.forward(z)
    tr.close()
    assert before.tobytes() == during.tobytes() == net.forward(z).tobytes()


def test_train_pinc_end_to_end():
    """A few epochs on cfg5's train split lower the one-step loss; the result runs through the evaluator and the comparison."""
    from bluerov2_dynamics_amd.fossen.BlueROV2 import BlueROV2
    from bluerov2_dynamics_amd.pinc import PINc, PINcWeights, make_pinc_dataset, multistep_rmse_endpoint_pinc, train_pinc
    g = load_golden("cfg5.npz")
    X, U, dt, sp = g["X"], g["U"], float(g["dt"]), int(g["split"])
    rov = BlueROV2(dt=dt)
    z, y, U4 = make_pinc_dataset(X[:sp], U[:sp], dt, rov)
    d = load_golden("pinc_train.npz")
    assert rel_err(U4, d["U4"]) < 1e-12 and rel_err(rov._lag, d["lag_after"]) < 1e-12 and rel_err(z, d["z"]) < 1e-12

    def one_step(w):
        e = PINc(w).forward(z).astype(np.float64) - y
        return float(np.mean(e * e))

    w0 = PINcWeights.init(3)
    w1 = train_pinc(z, y, U4, dt, epochs=1, init=w0, seed=3, verbose=False)
    w4 = train_pinc(z, y, U4, dt, epochs=4, init=w0, seed=3, verbose=False)
    l0, l1, l4 = one_step(w0), one_step(w1), one_step(w4)
    print(f"[pinc train] one-step loss: init {l0:.4e}, after 1 epoch {l1:.4e}, after 4 epochs {l4:.4e}")
    assert l4 < l1 and l4 < l0                  # the first epoch (7 Adam steps at lr 3e-3 from a fresh net) may overshoot
    assert set(w4.state_dict()) == set(R.KEYS)
    rmse = multistep_rmse_endpoint_pinc(X[sp:], U[sp:], 10, dt, w4, BlueROV2(dt=dt))
    assert np.isfinite(rmse) and rmse > 0
    sys.path.insert(0, os.path.join(REPO, "examples"))
    try:
        import full_comparison
    finally:
        sys.path.pop(0)
    out = full_comparison.compare(os.path.join(REPO, "tests", "golden", "cfg5_dataset.csv.gz"), n_rbfs=50, verbose=False, pinc_train=1)
    assert out["table"].shape == (4, 3) and np.all(np.isfinite(out["table"])) and out["rows"][3].startswith("PINc")
    with pytest.raises(ValueError):
        full_comparison.compare("unused.csv", pinc_train=1, pinc_row=[1, 2, 3])


def test_a_second_trainer_takes_the_session_over(fx):
    """A ctx holds one session: the trainer that lost it raises instead of reading the other's state, and its close() leaves the
    new session alone."""
    a = _trainer(fx["sets"]["fresh"])
    with _trainer(fx["sets"]["ckpt"]) as b:
        for call in (a.weights, a.state, lambda: a.loss_and_grad(fx["Z"][:4], fx["Y"][:4], fx["U"][:4])):
            with pytest.raises(RuntimeError, match="replaced"):
                call()
        a.close()
        assert b.weights().blob.tobytes() == R.flatten(fx["sets"]["ckpt"], np.float32).tobytes()
    with pytest.raises(RuntimeError):
        b.weights()
