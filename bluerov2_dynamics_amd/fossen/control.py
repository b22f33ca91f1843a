"""Feedback laws for the closed-loop rollouts (engine.rollout_feedback, VehicleBase.simulate_closed_loop) and the record of the
model-predictive updates (engine.mppi_step, VehicleBase.simulate_mppi; engine.koopman_lmpc_step, VehicleBase.simulate_lmpc): builders of
struct brov_feedback, struct brov_mppi and struct brov_lmpc, and
the tracking error on the host.  include/brov2.h (brov_rollout_feedback) is the specification of the law:

    e[0:3]  = R(att)^T (p_ref - p)          e[3:6] = attitude error (wrapped Euler difference, or 2 s q_e.xyz)
    e[6:12] = nu_ref - nu
    u = clip(u_ff + K e + Ki z, u_min, u_max),    z <- clip(z + hold dt e[0:6], -z_max, z_max)

Nothing here runs on the device; the structs go to the kernel through engine.rollout_feedback."""
import numpy as np

from .. import _lib

NU = {_lib.THRUSTER_EULER: 8, _lib.WRENCH_EULER: 6, _lib.WRENCH_QUAT: 6}


def _vec(v, n, default, name):
    if v is None:
        return np.full(n, float(default))
    a = np.asarray(v, dtype=float)
    if a.ndim == 0:
        return np.full(n, float(a))
    if a.shape != (n,):
        raise ValueError(f"{name} must be a scalar or have shape ({n},), got {a.shape}")
    return a.copy()


def feedback(K, Ki=None, u_min=None, u_max=None, z_max=None, hold=1, nu=None):
    """struct brov_feedback from K [nu,12], Ki [nu,6] (None = 0), limits u_min / u_max (scalar or [nu]; None = -inf / +inf), z_max
    (scalar or [6]; None = inf) and hold (controller period in steps).  nu (6 or 8) defaults to the rows of K.  ValueError where
    the library would refuse the record: a NaN, u_min > u_max, a negative z_max, hold < 1."""
    K = np.asarray(K, dtype=float)
    if K.ndim != 2 or K.shape[1] != 12:
        raise ValueError(f"K must be [nu,12], got {K.shape}")
    nu = K.shape[0] if nu is None else int(nu)
    if nu not in (6, 8) or K.shape[0] != nu:
        raise ValueError(f"K must have nu = 6 or 8 rows (nu = {nu}, K {K.shape})")
    Ki = np.zeros((nu, 6)) if Ki is None else np.asarray(Ki, dtype=float)
    if Ki.shape != (nu, 6):
        raise ValueError(f"Ki must be [{nu},6], got {Ki.shape}")
    lo, hi = _vec(u_min, nu, -np.inf, "u_min"), _vec(u_max, nu, np.inf, "u_max")
    zm = _vec(z_max, 6, np.inf, "z_max")
    if isinstance(hold, float) and hold != int(hold):
        raise ValueError(f"hold must be an integer, got {hold}")
    hold = int(hold)
    if hold < 1 or hold >= 2 ** 31:
        raise ValueError(f"hold must be >= 1, got {hold}")
    if any(np.isnan(a).any() for a in (K, Ki, lo, hi, zm)):
        raise ValueError("NaN in the feedback record")
    if np.any(lo > hi):
        raise ValueError("u_min must be <= u_max")
    if np.any(zm < 0):
        raise ValueError("z_max must be >= 0")
    fb = _lib.BrovFeedback()
    for i in range(nu):
        for j in range(12):
            fb.K[i][j] = K[i, j]
        for j in range(6):
            fb.Ki[i][j] = Ki[i, j]
        fb.u_min[i], fb.u_max[i] = lo[i], hi[i]
    for j in range(6):
        fb.z_max[j] = zm[j]
    fb.hold = hold
    return fb


def mppi(q, qf=None, r=0.0, sigma=0.1, lam=1.0, gamma=None, u_min=None, u_max=None, hold=1, nu=None):
    """struct brov_mppi (include/brov2.h: brov_mppi_step) from the stage weights q and terminal weights qf on the tracking error
    (scalar or [12]; qf=None means q), the command weights r and the noise sigma (scalar or [nu]), the temperature lam, the weight
    gamma of the importance term (None means lam), limits u_min / u_max (scalar or [nu]; None = -inf / +inf) and hold (steps per
    knot).  nu (6 or 8) defaults to the length of the first of r, sigma, u_min, u_max given as a vector, else 8.  ValueError where
    the library would refuse the record: a NaN, a negative weight, sigma or gamma, lam <= 0, u_min > u_max, hold < 1."""
    if nu is None:
        nu = next((np.asarray(v).shape[0] for v in (r, sigma, u_min, u_max) if v is not None and np.ndim(v) == 1), 8)
    nu = int(nu)
    if nu not in (6, 8):
        raise ValueError(f"nu must be 6 or 8, got {nu}")
    q = _vec(q, 12, 0.0, "q")
    qf = q.copy() if qf is None else _vec(qf, 12, 0.0, "qf")
    r, sg = _vec(r, nu, 0.0, "r"), _vec(sigma, nu, 0.0, "sigma")
    lo, hi = _vec(u_min, nu, -np.inf, "u_min"), _vec(u_max, nu, np.inf, "u_max")
    lam = float(lam)
    gamma = lam if gamma is None else float(gamma)
    if isinstance(hold, float) and hold != int(hold):
        raise ValueError(f"hold must be an integer, got {hold}")
    hold = int(hold)
    if hold < 1 or hold >= 2 ** 31:
        raise ValueError(f"hold must be >= 1, got {hold}")
    if any(np.isnan(a).any() for a in (q, qf, r, sg, lo, hi)) or np.isnan(lam) or np.isnan(gamma):
        raise ValueError("NaN in the MPPI record")
    if np.any(q < 0) or np.any(qf < 0) or np.any(r < 0):
        raise ValueError("the weights q, qf and r must be >= 0")
    if np.any(sg < 0):
        raise ValueError("sigma must be >= 0")
    if not lam > 0:
        raise ValueError("lam must be > 0")
    if gamma < 0:
        raise ValueError("gamma must be >= 0")
    if np.any(lo > hi):
        raise ValueError("u_min must be <= u_max")
    cfg = _lib.BrovMppi()
    for i in range(12):
        cfg.q[i], cfg.qf[i] = q[i], qf[i]
    for j in range(nu):
        cfg.r[j], cfg.sigma[j], cfg.u_min[j], cfg.u_max[j] = r[j], sg[j], lo[j], hi[j]
    cfg.lam, cfg.gamma, cfg.hold = lam, gamma, hold
    return cfg


def lmpc(q, qf=None, r=0.0, u_min=None, u_max=None, hold=1, iters=200, tol=0.0, rho=None, nu=None, n=12):
    """struct brov_lmpc (include/brov2.h: edmdc_lmpc_step) from the stage weights q and terminal weights qf on the linear error
    (scalar or [n]; qf=None means q), the command weights r (scalar or [nu]), limits u_min / u_max (scalar or [nu]; None = -inf /
    +inf), hold (steps per knot), the iteration limit, the stop tolerance (0: always `iters` iterations) and the ADMM penalty rho.
    rho=None leaves the field 0, which the library refuses: engine.KoopmanLmpc fills it with sqrt(lambda_min lambda_max) of the
    condensed matrix.  n (12 or 13) is the state size, nu (6 or 8) defaults to the length of the first of r, u_min, u_max given as a
    vector, else 8.  ValueError where the library would refuse the record: a NaN, a negative weight or tol, u_min > u_max, hold < 1,
    iters outside 0 .. 1 000 000, a rho that is not finite and > 0."""
    if nu is None:
        nu = next((np.asarray(v).shape[0] for v in (r, u_min, u_max) if v is not None and np.ndim(v) == 1), 8)
    nu, n = int(nu), int(n)
    if nu not in (6, 8):
        raise ValueError(f"nu must be 6 or 8, got {nu}")
    if n not in (12, 13):
        raise ValueError(f"n must be 12 or 13, got {n}")
    q = _vec(q, n, 0.0, "q")
    qf = q.copy() if qf is None else _vec(qf, n, 0.0, "qf")
    r = _vec(r, nu, 0.0, "r")
    lo, hi = _vec(u_min, nu, -np.inf, "u_min"), _vec(u_max, nu, np.inf, "u_max")
    for name, v in (("hold", hold), ("iters", iters)):
        if isinstance(v, float) and v != int(v):
            raise ValueError(f"{name} must be an integer, got {v}")
    hold, iters, tol = int(hold), int(iters), float(tol)
    if hold < 1 or hold >= 2 ** 31:
        raise ValueError(f"hold must be >= 1, got {hold}")
    if not 0 <= iters <= 1000000:
        raise ValueError(f"iters must be 0 .. 1 000 000, got {iters}")
    if any(np.isnan(a).any() for a in (q, qf, r, lo, hi)) or np.isnan(tol) or (rho is not None and np.isnan(rho)):
        raise ValueError("NaN in the linear-MPC record")
    if np.any(q < 0) or np.any(qf < 0) or np.any(r < 0):
        raise ValueError("the weights q, qf and r must be >= 0")
    if tol < 0:
        raise ValueError("tol must be >= 0")
    if rho is not None and not (rho > 0 and np.isfinite(rho)):
        raise ValueError("rho must be finite and > 0")
    if np.any(lo > hi):
        raise ValueError("u_min must be <= u_max")
    cfg = _lib.BrovLmpc()
    for i in range(n):
        cfg.q[i], cfg.qf[i] = q[i], qf[i]
    for j in range(nu):
        cfg.r[j], cfg.u_min[j], cfg.u_max[j] = r[j], lo[j], hi[j]
    cfg.rho, cfg.tol, cfg.hold, cfg.iters = (0.0 if rho is None else float(rho)), tol, hold, iters
    return cfg


def _gain6(g, name):
    """a 6x6 gain from a scalar, a diagonal [6] or a full [6,6]"""
    if g is None:
        return np.zeros((6, 6))
    a = np.asarray(g, dtype=float)
    if a.ndim == 0:
        return np.eye(6) * float(a)
    if a.shape == (6,):
        return np.diag(a)
    if a.shape == (6, 6):
        return a.copy()
    raise ValueError(f"{name} must be a scalar, [6] or [6,6], got {a.shape}")


def wrench_gains(Kp6, Kd6, Ki6=None):
    """(K [6,12], Ki [6,6]) of tau = Kp e[0:6] + Kd e[6:12] + Ki z"""
    return np.hstack([_gain6(Kp6, "Kp6"), _gain6(Kd6, "Kd6")]), _gain6(Ki6, "Ki6")


def pid_wrench(Kp6, Kd6, Ki6=None, u_min=None, u_max=None, z_max=None, hold=1):
    """PID on pose, velocity and the integral of the pose error for the wrench models: diagonal ([6]) or full ([6,6]) gains."""
    K, Ki = wrench_gains(Kp6, Kd6, Ki6)
    return feedback(K, Ki, u_min, u_max, z_max, hold, nu=6)


def allocation_inverse(rov_or_params=None):
    """[8,6]: thruster commands per unit wrench at small signal -- the Moore-Penrose inverse of the 6x8 allocation matrix of
    brov_get_derived, divided by the slope thrust_poly[0] of the thrust polynomial at zero command."""
    from . import identify
    p = _lib.default_params() if rov_or_params is None else identify.params_of(rov_or_params)
    _, T = _lib.derived(p)
    slope = float(p.thrust_poly[0])
    if slope == 0.0 or not np.isfinite(slope):
        raise ValueError("thrust_poly[0] must be finite and non-zero")
    return np.linalg.pinv(T) / slope


def pid_thrusters(rov_or_params, Kp6, Kd6, Ki6=None, u_min=-1.0, u_max=1.0, z_max=None, hold=1):
    """The wrench-space gains of pid_wrench mapped to the eight thruster commands of a vehicle (a drop-in object, a BrovParams or
    None for the nominal one) through allocation_inverse; the commands are limited to u_min .. u_max (default +-1)."""
    A = allocation_inverse(rov_or_params)
    K, Ki = wrench_gains(Kp6, Kd6, Ki6)
    return feedback(A @ K, A @ Ki, u_min, u_max, z_max, hold, nu=8)


def _rot_euler(phi, th, psi):
    cf, sf, ct, st, cp, sp = np.cos(phi), np.sin(phi), np.cos(th), np.sin(th), np.cos(psi), np.sin(psi)
    R = np.empty(phi.shape + (3, 3))
    R[..., 0, 0], R[..., 0, 1], R[..., 0, 2] = cp * ct, cp * st * sf - sp * cf, cp * st * cf + sp * sf
    R[..., 1, 0], R[..., 1, 1], R[..., 1, 2] = sp * ct, sp * st * sf + cp * cf, sp * st * cf - cp * sf
    R[..., 2, 0], R[..., 2, 1], R[..., 2, 2] = -st, ct * sf, ct * cf
    return R


def _rot_quat(q):
    n = np.sqrt(np.sum(q * q, axis=-1, keepdims=True))
    ident = np.zeros_like(q)
    ident[..., 0] = 1.0
    with np.errstate(all="ignore"):
        q = np.where(n < 1e-12, ident, q / n)
    w, x, y, z = (q[..., i] for i in range(4))
    R = np.empty(q.shape[:-1] + (3, 3))
    R[..., 0, 0], R[..., 0, 1], R[..., 0, 2] = 1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)
    R[..., 1, 0], R[..., 1, 1], R[..., 1, 2] = 2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)
    R[..., 2, 0], R[..., 2, 1], R[..., 2, 2] = 2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)
    return R


def error_numpy(model, x, r):
    """The tracking error e [...,12] of the law on the host, for states x and reference rows r [...,nx] (broadcast against each
    other): what the kernel forms at a step, for users' own cost functions."""
    x, r = np.broadcast_arrays(np.asarray(x, dtype=float), np.asarray(r, dtype=float))
    quat = model == _lib.WRENCH_QUAT
    nx = 13 if quat else 12
    if x.shape[-1] != nx:
        raise ValueError(f"states of model {model} have {nx} values, got {x.shape[-1]}")
    e = np.empty(x.shape[:-1] + (12,))
    if quat:
        R = _rot_quat(x[..., 3:7])
        qw, qv, rw, rv = x[..., 3], x[..., 4:7], r[..., 3], r[..., 4:7]
        we = qw * rw + np.sum(qv * rv, axis=-1)
        ve = qw[..., None] * rv - rw[..., None] * qv - np.cross(qv, rv)
        e[..., 3:6] = 2.0 * np.where(we >= 0.0, 1.0, -1.0)[..., None] * ve
    else:
        R = _rot_euler(x[..., 3], x[..., 4], x[..., 5])
        d = r[..., 3:6] - x[..., 3:6]
        e[..., 3:6] = d - 2.0 * np.pi * np.rint(d / (2.0 * np.pi))
    e[..., 0:3] = np.einsum("...ji,...j->...i", R, r[..., 0:3] - x[..., 0:3])
    e[..., 6:12] = r[..., nx - 6:] - x[..., nx - 6:]
    return e
