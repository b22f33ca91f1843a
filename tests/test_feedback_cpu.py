"""Closed-loop rollouts, the parts that need no GPU: the ABI mirror, the builders of fossen/control.py, the host error, and the
tests' own reference (tests/feedback_ref.py) pinned to the oracle."""
import ctypes

import numpy as np
import pytest

import feedback_ref as fr
import fossen_vehicles as fv
from oracle import fossen_params as fp


@pytest.fixture(scope="module")
def lib():
    from bluerov2_dynamics_amd import _build, _lib
    _build.build_library()
    return _lib.load_library()


def test_struct_size_and_symbols(lib):
    """struct brov_feedback: K 8x12, Ki 8x6, u_min 8, u_max 8, z_max 6 = 166 doubles, then two int32: 167 x 8 bytes, the size
    csrc/capi.hip asserts for the C struct."""
    from bluerov2_dynamics_amd import _lib
    assert ctypes.sizeof(_lib.BrovFeedback) == (8 * 12 + 8 * 6 + 8 + 8 + 6 + 1) * 8 == 167 * 8
    assert _lib.BrovFeedback.hold.offset == 166 * 8 and _lib.BrovFeedback.Ki.offset == 96 * 8
    for name in ("brov_rollout_feedback", "brov_rollout_feedback_dev"):
        fn = getattr(lib, name)
        assert fn.restype is ctypes.c_int and len(fn.argtypes) == 23
    assert lib.brov_abi_version() == 1


def test_feedback_builder_shapes_and_rules(lib):
    from bluerov2_dynamics_amd.fossen import control
    rng = np.random.default_rng(1)
    K, Ki = rng.normal(size=(8, 12)), rng.normal(size=(8, 6))
    fb = control.feedback(K, Ki, u_min=-1.0, u_max=np.linspace(0.5, 1.2, 8), z_max=2.0, hold=5)
    assert np.array_equal(np.ctypeslib.as_array(fb.K), K) and np.array_equal(np.ctypeslib.as_array(fb.Ki), Ki)
    assert list(fb.u_min) == [-1.0] * 8 and list(fb.u_max) == list(np.linspace(0.5, 1.2, 8)) and list(fb.z_max) == [2.0] * 6
    assert fb.hold == 5
    fb = control.feedback(K[:6])                       # nu = 6: rows 6, 7 stay zero; defaults are no limits, no integral action
    assert np.array_equal(np.ctypeslib.as_array(fb.K)[:6], K[:6]) and not np.ctypeslib.as_array(fb.K)[6:].any()
    assert not np.ctypeslib.as_array(fb.Ki).any()
    assert list(fb.u_min)[:6] == [-np.inf] * 6 and list(fb.u_max)[:6] == [np.inf] * 6 and list(fb.z_max) == [np.inf] * 6 and fb.hold == 1
    bad = [dict(K=K[:, :11]), dict(K=K[:7]), dict(K=K, nu=6), dict(K=K, Ki=Ki[:6]), dict(K=K, u_min=np.zeros(6)),
           dict(K=K, z_max=np.ones(5)), dict(K=K, hold=0), dict(K=K, hold=2.5), dict(K=K, u_min=0.5, u_max=0.4), dict(K=K, z_max=-1.0),
           dict(K=np.where(np.arange(12) == 3, np.nan, K)), dict(K=K, Ki=np.full((8, 6), np.nan)), dict(K=K, u_max=np.nan),
           dict(K=K, z_max=np.nan)]
    for kw in bad:
        with pytest.raises(ValueError):
            control.feedback(**kw)


def test_pid_builders(lib):
    """pid_wrench lays [Kp | Kd] and Ki out as K [6,12], Ki [6,6]; pid_thrusters maps them through the pseudo-inverse of the
    nominal 6x8 allocation, computed here by hand as T^T (T T^T)^-1 (T has full row rank), over the slope thrust_poly[0]."""
    from bluerov2_dynamics_amd import _lib
    from bluerov2_dynamics_amd.fossen import control
    kp, kd, ki = np.arange(1.0, 7.0), 0.1 * np.arange(6.0, 0.0, -1.0), np.full(6, 0.3)
    fb = control.pid_wrench(kp, kd, ki, u_min=-15.0, u_max=15.0, z_max=1.0, hold=2)
    K, Ki = np.ctypeslib.as_array(fb.K), np.ctypeslib.as_array(fb.Ki)
    assert np.array_equal(K[:6], np.hstack([np.diag(kp), np.diag(kd)])) and np.array_equal(Ki[:6], np.diag(ki)) and fb.hold == 2
    full = np.random.default_rng(2).normal(size=(6, 6))
    assert np.array_equal(np.ctypeslib.as_array(control.pid_wrench(full, 0.0).K)[:6, :6], full)
    with pytest.raises(ValueError):
        control.pid_wrench(np.ones(5), kd)
    p = _lib.default_params()
    _, T = _lib.derived(p)
    pinv = T.T @ np.linalg.inv(T @ T.T)
    fb = control.pid_thrusters(None, kp, kd, ki)
    want_K, want_Ki = pinv @ np.hstack([np.diag(kp), np.diag(kd)]) / 8.9, pinv @ np.diag(ki) / 8.9
    assert p.thrust_poly[0] == 8.9
    assert np.allclose(np.ctypeslib.as_array(fb.K), want_K, rtol=1e-12, atol=1e-14)
    assert np.allclose(np.ctypeslib.as_array(fb.Ki), want_Ki, rtol=1e-12, atol=1e-14)
    assert list(fb.u_min) == [-1.0] * 8 and list(fb.u_max) == [1.0] * 8
    # a wrench demand comes back through the allocation: T (slope u) = tau for u = pinv tau / slope
    tau = np.array([3.0, -2.0, 5.0, 0.2, -0.1, 0.4])
    assert np.allclose(T @ (8.9 * control.allocation_inverse(p) @ tau), tau, atol=1e-12)
    assert np.array_equal(np.ctypeslib.as_array(control.pid_thrusters(p, kp, kd, ki).K), np.ctypeslib.as_array(fb.K))


@pytest.mark.parametrize("model", [0, 1, 2])
def test_error_numpy_matches_the_reference(lib, model):
    """control.error_numpy against feedback_ref.error (written independently) at random states; rows 0 and 1 carry a yaw error
    whose raw difference is +6.0 / -6.0 rad (wraps to -0.283 / +0.283), rows 2 and 3 a quaternion pair with q_e.w < 0."""
    from bluerov2_dynamics_amd.fossen import control
    rng = np.random.default_rng(30 + model)
    n, nx = 64, fp.NX[model]
    x, r = rng.uniform(-2, 2, (n, nx)), rng.uniform(-2, 2, (n, nx))
    if model == 2:
        x[:, 3:7] /= np.linalg.norm(x[:, 3:7], axis=1, keepdims=True)
        r[:, 3:7] /= np.linalg.norm(r[:, 3:7], axis=1, keepdims=True)
        r[2:4, 3:7] = -x[2:4, 3:7] + 0.1 * rng.normal(size=(2, 4))
        r[2:4, 3:7] /= np.linalg.norm(r[2:4, 3:7], axis=1, keepdims=True)
    else:
        x[0, 5], r[0, 5] = -3.0, 3.0
        x[1, 5], r[1, 5] = 3.0, -3.0
    want, margin = fr.error(model, x, r)
    got = control.error_numpy(model, x, r)
    assert got.shape == (n, 12) and margin > 1e-6
    assert np.max(np.abs(got - want)) < 1e-14
    if model == 2:
        qe_w = np.sum(x[2:4, 3:7] * r[2:4, 3:7], axis=1)
        assert np.all(qe_w < 0)
        # the short way round: the same rotation written with -q_ref gives the same error
        r2 = r.copy()
        r2[2:4, 3:7] *= -1
        assert np.allclose(control.error_numpy(model, x, r2)[2:4], got[2:4], atol=1e-15)
    else:
        assert abs(got[0, 5] - (6.0 - 2 * np.pi)) < 1e-15 and abs(got[1, 5] - (2 * np.pi - 6.0)) < 1e-15
    assert np.array_equal(control.error_numpy(model, x[0], r[0]), got[0])         # one state, no batch axis


@pytest.mark.parametrize("integ", [fp.EULER, fp.RK4])
@pytest.mark.parametrize("model", [0, 1, 2])
def test_reference_with_zero_gains_is_the_oracle_rollout(model, integ):
    """feedback_ref.rollout with K = Ki = 0 and infinite limits applies u_ff unchanged: traj and lag equal fp.rollout on U = u_ff
    bit for bit.  This pins the reference the GPU tests compare against to the oracle."""
    rng = np.random.default_rng(50 + model)
    B, T, dt = 7, 9, 0.02
    nx, nu = fp.NX[model], fp.NU[model]
    x0 = rng.uniform(-0.5, 0.5, (B, nx))
    if model == 2:
        x0[:, 3:7] /= np.linalg.norm(x0[:, 3:7], axis=1, keepdims=True)
    u_ff = rng.uniform(-1, 1, (B, T, nu)) * (1.0 if model == 0 else 15.0)
    ref = rng.uniform(-0.5, 0.5, (B, T, nx))
    lag0 = rng.uniform(-1, 1, (B, 8, 3)) if model == 0 else None
    v = fv.vehicle("V7")
    got = fr.rollout(model, integ, 0, v, fr.law(nu), x0, ref, dt, u_ff=u_ff, lag=lag0, z=rng.uniform(-1, 1, (B, 6)))
    want = fp.rollout(model, integ, 0, v, x0, u_ff, dt, lag=lag0)
    assert np.array_equal(got["traj"], want["traj"]) and np.array_equal(got["xT"], want["xT"])
    assert np.array_equal(got["lag"], want["lag"]) and np.array_equal(got["u"], u_ff)
    assert got["sat_margin"] == np.inf and np.all(got["metrics"][:, 3] == 0)
