"""The smoother's references on the filter problems of tests/ukf_cases.py, computed once and shared by tests/test_ukf_smooth_cpu.py
and tests/test_ukf_smooth_gpu.py (tests/ukf_smooth_ref.py is the law).  Not collected."""
import functools

import numpy as np

import fossen_vehicles as fv
import ukf_cases as uc
import ukf_smooth_ref as usr

NAMES = tuple(uc.CASES)
TOL = 1e-10                 # the bound of tests/test_ukf_gpu.py
MARGIN = 1e-6
PIVOT = 1e-4
T1 = 5                      # where the split-span identities cut the 12 rows


def vehicles():
    return [fv.vehicle(n) for n in uc.NAMES]


def smooth(name, ld=False, **kw):
    """ukf_smooth_ref.smooth on inputs(name) with the entries of kw replaced"""
    i = uc.inputs(name)
    a = dict(x0=i["x0"], P0=i["P0"], U=i["U"], Y=i["Y"], lag=i["lag"], terminal=None, cfgs=i["cfgs"])
    a.update(kw)
    return usr.smooth(i["model"], uc.INTEG[i["integ"]], i["lag_mode"], vehicles(), a["cfgs"], a["x0"], a["P0"], a["U"], a["Y"], uc.DT, lag=a["lag"],
                      dtype=uc.L if ld else np.float64, terminal=a["terminal"])


@functools.lru_cache(maxsize=None)
def reference(name, ld=False):
    """read-only: shared among the tests"""
    return smooth(name, ld)


def tape_fields(tape):
    """the four fields of a tape [..., 312]: Pf and Pp unpacked to [..., 12, 12] (for uc.cov_err), xp [..., 12], C [..., 12, 12]"""
    tape = np.asarray(tape)

    def sym(v):
        Pm = np.zeros(v.shape[:-1] + (12, 12), dtype=v.dtype)
        Pm[..., usr.TRIL[0], usr.TRIL[1]] = v
        Pm[..., usr.TRIL[1], usr.TRIL[0]] = v
        return Pm
    return dict(Pf=sym(tape[..., usr.PF]), xp=tape[..., usr.XP], Pp=sym(tape[..., usr.PP]), C=tape[..., usr.CC].reshape(tape.shape[:-1] + (12, 12)))


def cross_err(C, ref):
    """max |dC_ab| / sqrt(Pf_aa Pp_bb) over a tape: the covariance measure of uc.cov_err for the cross covariance C = cov(x_t, x_t+1)"""
    a, b = tape_fields(C), tape_fields(ref)
    if np.any(np.isnan(a["C"]) != np.isnan(b["C"])):
        return np.inf
    sa = np.sqrt(np.diagonal(b["Pf"], axis1=-2, axis2=-1)).astype(uc.L)
    sb = np.sqrt(np.diagonal(b["Pp"], axis1=-2, axis2=-1)).astype(uc.L)
    rel = np.abs(a["C"].astype(uc.L) - b["C"].astype(uc.L)) / (sa[..., :, None] * sb[..., None, :])
    ok = ~np.isnan(rel)
    return float(np.max(rel[ok])) if ok.any() else 0.0


def gaps(o, ol):
    """{output: error of o against ol} for the smoother's outputs and the four tape fields"""
    g = {k: uc.err(o[k], ol[k]) for k in ("xs", "pstd_s")}
    g["Ps"], g["Ps0"] = uc.cov_err(o["Ps"], ol["Ps"]), uc.cov_err(o["Ps0"], ol["Ps0"])
    a, b = tape_fields(o["tape"]), tape_fields(ol["tape"])
    g["tape Pf"], g["tape Pp"] = uc.cov_err(a["Pf"], b["Pf"]), uc.cov_err(a["Pp"], b["Pp"])
    g["tape xp"] = uc.err(a["xp"], b["xp"])
    g["tape C"] = cross_err(o["tape"], ol["tape"])
    g["sinfo[1]"] = uc.err(np.asarray(o["sinfo"])[..., 1], np.asarray(ol["sinfo"])[..., 1])
    return g
