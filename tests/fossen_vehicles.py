"""The non-nominal vehicles of tests/test_fossen_params_gpu.py and of the host-only checks in tests/test_oracle_golden.py, each
built from _lib.default_params() (struct brov_params).  tools/gen_golden.py: gen_fossen_vehicles applies the same edits to the
reference's objects.  Every edit is large enough that the oracle's RHS and window score move by more than 1e3 x the parity
bounds (test_each_edit_matters), so a kernel that ignored a field fails the parity tests.

  V0  nominal
  V1  mass, volume, rho, g, inertias, added mass        -> the non-GENERIC rollout kernels at other constants
  V2  linear damping (zeros replaced), quadratic damping, zb
  V3  lag Ac, Bc, Cc and the thrust polynomial          -> the observer-basis lag with non-default constants
  V4  xb, yb                                            -> has_xy
  V5  a current                                         -> has_current
  V6  every thruster direction tilted, thr_r[0] shifted -> tm_dense
  V7  V1 .. V6 together
  V8  a diagonal lag Ac with Cc = (1, 0, 0): Cc Ad^k spans one direction only, no observer basis -> obs_bad
"""
import numpy as np

NAMES = ("V0", "V1", "V2", "V3", "V4", "V5", "V6", "V7", "V8")
WRENCH_NAMES = ("V0", "V1", "V2", "V4", "V5", "V7")          # the edits of V3, V6, V8 touch thrusters only
FIXTURE_NAMES = ("V1", "V2", "V3n", "V4", "V5", "V6")         # V3n: V3 without the polynomial change (the reference hard-codes it)


def _mass(p):
    p.m *= 1.15
    p.volume *= 0.97
    p.rho, p.g = 1025.0, 9.81
    p.Ix *= 1.2
    p.Iy *= 0.8
    p.Iz *= 1.1
    for i, f in enumerate((1.2, 0.9, 0.7, 1.3, 0.8, 1.1)):
        p.added_mass[i] *= f


def _damping(p):
    for i, (fl, fq) in enumerate(zip(np.linspace(0.7, 1.4, 6), np.linspace(1.3, 0.6, 6))):
        p.lin_damp[i] = p.lin_damp[i] * fl if p.lin_damp[i] != 0.0 else -0.5
        p.quad_damp[i] *= fq
    p.zb *= 2.0


def _lag(p, poly=True):
    for j in range(9):
        p.lag_Ac[j] *= 0.9
    for j in range(3):
        p.lag_Bc[j] *= 1.1
        p.lag_Cc[j] = (0.4, 5.0, 3.9)[j]
    if poly:
        for j in range(5):
            p.thrust_poly[j] *= 1.1


def _cb(p):
    p.xb, p.yb = 0.01, -0.02


def _current(p):
    for j in range(3):
        p.current[j] = (0.2, -0.1, 0.05)[j]


def _tilted(p):
    rng = np.random.default_rng(66)
    for i in range(8):
        d = np.array([p.thr_dir[i][j] for j in range(3)]) + rng.uniform(-0.2, 0.2, 3)
        d /= np.linalg.norm(d)
        for j in range(3):
            p.thr_dir[i][j] = d[j]
    for j in range(3):
        p.thr_r[0][j] += (0.02, -0.015, 0.03)[j]


def _unobservable(p):
    for j in range(9):
        p.lag_Ac[j] = np.diag([-10.0, -20.0, -30.0]).ravel()[j]
    for j in range(3):
        p.lag_Bc[j] = (10.0, 0.0, 0.0)[j]
        p.lag_Cc[j] = (1.0, 0.0, 0.0)[j]


_EDITS = dict(V0=(), V1=(_mass,), V2=(_damping,), V3=(_lag,), V3n=(lambda p: _lag(p, poly=False),), V4=(_cb,), V5=(_current,),
              V6=(_tilted,), V7=(_mass, _damping, _lag, _cb, _current, _tilted), V8=(_unobservable,))


def params(name):
    """_lib.BrovParams of vehicle `name`"""
    from bluerov2_dynamics_amd import _lib
    p = _lib.default_params()
    for edit in _EDITS[name]:
        edit(p)
    return p


def vehicle(name):
    """oracle.fossen_params.Vehicle of vehicle `name`"""
    from oracle import fossen_params
    return fossen_params.from_brov_params(params(name))
