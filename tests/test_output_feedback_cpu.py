"""The output-feedback closed loop, the parts that need no GPU: the ABI mirror and the cross-compiled library, the Python-side
argument checks, the draw of the measurement noise, and the tests' own reference (tests/ukf_feedback_ref.py) -- pinned to the
state-feedback reference, checked against the text of the header, and the well-posedness of the cases that
tests/test_output_feedback_gpu.py compares on the device."""
import ctypes

import numpy as np
import pytest

import feedback_ref as fr
import fossen_vehicles as fv
import ukf_feedback_ref as ofr
import ukf_ref as ur
from oracle import fossen_params as fp

PIVOT = 1e-4                             # tests/test_ukf_gpu.py


@pytest.fixture(scope="module")
def lib():
    from bluerov2_dynamics_amd import _build, _lib
    _build.build_library()
    return _lib.load_library()


# ------------------------------------------------------------------------------------------ the ABI, the build
def test_signatures_and_symbols(lib):
    """_lib.SIGNATURES carries both forms with the 37 arguments of the header, and the built library exports them"""
    from bluerov2_dynamics_amd import _lib
    for name in ("brov_output_feedback", "brov_output_feedback_dev"):
        res, args = _lib.SIGNATURES[name]
        assert res is ctypes.c_int and len(args) == 37
        assert args[5] == args[7] == ctypes.POINTER(_lib.BrovParams) and args[9] == ctypes.POINTER(_lib.BrovFeedback)
        assert args[11] == ctypes.POINTER(_lib.BrovUkf) and args[14] is ctypes.c_double
        fn = getattr(lib, name)
        assert fn.restype is ctypes.c_int and len(fn.argtypes) == 37


def test_library_is_built_from_the_new_source(lib):
    """the kernel's file is one of the library's sources, its shared header one of the dependencies that make the library stale, and
    the library that cross-compiles from them is up to date"""
    import os
    from bluerov2_dynamics_amd import _build
    assert "ukf_feedback.hip" in _build.SOURCES and "brov2_ukf.h" in _build.HEADERS
    for f in ("ukf_feedback.hip", "brov2_ukf.h"):
        assert os.path.exists(os.path.join(_build.CSRC, f))
    assert not _build.stale()


def test_null_ctx_is_refused_without_a_device(lib):
    assert lib.brov_output_feedback(None, 0, 1, 0, 1, None, 1, None, 1, None, 1, None, 1, 1, 0.02, *([None] * 7), 1, *([None] * 14)) == -1


# ------------------------------------------------------------------------------------------ the Python side
def test_python_side_errors_fire_before_any_device_call(lib, monkeypatch):
    """engine.output_feedback checks counts and shapes first: with the context out of reach every bad call still fails on its own
    assertion, and a good call gets as far as asking for the context"""
    from bluerov2_dynamics_amd import _lib, engine

    class Reached(Exception):
        pass

    def no_device(*a, **k):
        raise Reached()
    monkeypatch.setattr(engine, "default_context", no_device)
    i = ofr.inputs("thr_rk4")
    c = i["c"]
    P, B, T = c["P"], c["B"], c["T"]
    good = dict(params=[fv.params(n) for n in i["models"]], fb=fr.to_struct(i["laws"][0]), cfg=ur.to_struct(i["cfgs"][0]), x0_true=i["x0_true"],
                x0_est=i["x0_est"], P0=i["P0"], V=i["V"], ref=i["ref"], plant_params=None, W=None, u_ff=i["u_ff"],
                lag=(i["lag_est"], i["lag_plant"]), z=i["z"], want=engine.OUTPUT_FEEDBACK_OUTPUTS, model=0)

    def call(**kw):
        a = dict(good, **kw)
        return engine.output_feedback(a["model"], "rk4", a["params"], a["fb"], a["cfg"], a["x0_true"], a["x0_est"], a["P0"], a["V"], a["ref"], ofr.DT,
                                      plant_params=a["plant_params"], W=a["W"], u_ff=a["u_ff"], lag=a["lag"], z=a["z"], want=a["want"])
    with pytest.raises(Reached):
        call()
    bad = [dict(want=("traj", "xs")), dict(model=_lib.WRENCH_QUAT), dict(plant_params=good["params"][:2]), dict(fb=[good["fb"]] * 2),
           dict(cfg=[good["cfg"]] * 2), dict(lag=(i["lag_est"], None)), dict(V=i["V"][:, :, :11]), dict(V=i["V"][:, :0]),
           dict(ref=i["ref"][:, :T - 1]), dict(ref=i["ref"][:B - 1]), dict(x0_true=i["x0_true"][:, :11]), dict(x0_est=i["x0_est"][:B - 1]),
           dict(P0=i["P0"][:, :11]), dict(W=i["V"][:, :T - 1]), dict(u_ff=i["u_ff"][:, :, :6]), dict(lag=(i["lag_est"], i["lag_plant"][:2])),
           dict(z=i["z"][:, :, :5])]
    for kw in bad:
        with pytest.raises(AssertionError):
            call(**kw)


def test_measurement_noise_helper(lib):
    """estimate.measurement_noise: seeded and reproducible; the scale of r; the dropout rate; never-measured and r = +inf columns NaN;
    the numbers do not depend on dropout or never"""
    from bluerov2_dynamics_amd.fossen import estimate
    r = ofr.SIGMA ** 2
    r[7] = np.inf
    cfg = estimate.ukf(q=1e-6, r=r)
    V = estimate.measurement_noise(cfg, (40, 500), dropout=0.2, never=(2,), seed=11)
    assert V.shape == (40, 500, 12)
    assert np.array_equal(V, estimate.measurement_noise(cfg, (40, 500), dropout=0.2, never=(2,), seed=11), equal_nan=True)
    assert not np.array_equal(V, estimate.measurement_noise(cfg, (40, 500), dropout=0.2, never=(2,), seed=12), equal_nan=True)
    assert np.isnan(V[..., 7]).all() and np.isnan(V[..., 2]).all()
    live = [k for k in range(12) if k not in (2, 7)]
    rate = np.isnan(V[..., live]).mean()
    assert abs(rate - 0.2) < 0.01, rate                      # 200 000 draws: three standard deviations are 0.003
    std = np.nanstd(V[..., live], axis=(0, 1))
    assert np.max(np.abs(std / ofr.SIGMA[live] - 1.0)) < 0.03
    full = estimate.measurement_noise(cfg, (40, 500), seed=11)
    assert not np.isnan(full[..., live]).any() and np.isnan(full[..., 7]).all()
    keep = ~np.isnan(V)
    assert np.array_equal(V[keep], full[keep])
    assert estimate.measurement_noise(cfg, 9, seed=1).shape == (9, 12)
    for kw in (dict(dropout=-0.1), dict(dropout=1.5), dict(never=(12,))):
        with pytest.raises(ValueError):
            estimate.measurement_noise(cfg, (3,), **kw)


# ------------------------------------------------------------------------------------------ the reference
@pytest.mark.parametrize("name", list(ofr.CASES))
def test_gpu_cases_are_well_posed(name):
    """on the reference alone: at least 3 in 4 lanes are compared, their float64-to-long-double gap is below a tenth of TOL_ROLL, at
    least 3 in 4 runs have a saturation margin above MARGIN (the runs on which the count of saturated steps is asserted exactly), no
    run fails and no pivot comes near zero"""
    o, ol = ofr.reference(name), ofr.reference(name, ld=True)
    keep, gaps = ofr.compared(name)
    print(f"{name}: lanes compared {int(keep.sum())} of {keep.size}; fp64-vs-long-double gap {gaps.max():.2e} (all), {gaps[keep].max():.2e} (compared); "
          f"wrap margin {o['wrap_margin'].min():.2e}, saturation margin {o['sat_margin'].min():.2e}, smallest pivot {o['pivot_min'].min():.2e}")
    assert keep.sum() >= 0.75 * keep.size
    assert gaps[keep].max() < 0.1 * ofr.TOL_ROLL
    assert (o["sat_margin"] > ofr.MARGIN).mean() >= 0.75
    for r in (o, ol):
        assert np.all(r["info"][..., 2] == -1) and r["pivot_min"].min() > PIVOT
    c = ofr.case(name)
    assert o["traj"].shape == (c["P"], c["B"], c["T"] + 1, 12) and o["metrics"].shape == (c["P"], c["B"], 7)
    frac = np.isnan(ofr.inputs(name)["V"][..., [k for k in range(12) if k != ofr.UNMEASURED]]).mean()
    assert 0.1 < frac < 0.3, frac


def test_cases_reach_the_edges():
    """over the case list: every value of the issue's shape list occurs, some run saturates, a reference yaw crosses pi, and the
    wraps of the run whose estimate starts one turn away all move by 2 pi"""
    cs = [ofr.case(n) for n in ofr.CASES]
    for key, values in (("model", {0, 1}), ("integ", {"euler", "rk4"}), ("P", {1, 3}), ("B", {1, 5}), ("T", {7, 12}), ("hold", {1, 3}),
                        ("plant_P", {False, True}), ("fb_P", {False, True}), ("rec_P", {False, True}), ("W", {False, True}),
                        ("u_ff", {False, True}), ("moving", {False, True}), ("z", {False, True})):
        assert {c[key] for c in cs} == values, key
    assert {(c["lag_mode"], c["banks"]) for c in cs if c["model"] == 0} == {(0, True), (1, True), (0, False)}
    assert any(c["T"] % c["hold"] for c in cs)
    assert sum(float(ofr.reference(n)["metrics"][..., 3].sum()) for n in ofr.CASES) > 0, "at least one run saturates"
    i, o = ofr.inputs("thr_rk4"), ofr.reference("thr_rk4")
    assert np.abs(np.diff(i["ref"][0, :, 5])).max() > 6.0, "the wrapped reference yaw jumps by 2 pi"
    assert np.all(np.abs(o["xf"][:, 1, :, 5] - o["traj"][:, 1, :-1, 5]) > 6.0), "run 1: the estimate lives one turn away"
    assert np.all(o["metrics"][:, 1, 5] < 1e-2), "and its wrapped attitude error is small"


def test_matched_plant_and_exact_measurements_give_state_feedback():
    """with V = 0, r tiny against P, a start on the truth and the plant equal to the model, the estimate is the true state to rounding,
    and the reference's true trajectory agrees with feedback_ref.rollout (the state-feedback law on the oracle) within the gap
    bound, a tenth of TOL_ROLL.  This pins the composition to the two references it is made of."""
    name = "thr_rk4"
    i, c = ofr.inputs(name), ofr.case(name)
    B, T = c["B"], c["T"]
    k = ur.cfg(q=1e-12, r=1e-20)
    P0 = np.repeat(1e-10 * np.eye(12)[None], B, axis=0)
    v, law = fv.vehicle("V5"), i["laws"][0]
    lag = i["lag_plant"][:1]
    o = ofr.loop(c["model"], fp.RK4, c["lag_mode"], [v], [v], [law], [k], i["x0_true"], i["x0_true"], P0, np.zeros((B, T, 12)), i["ref"], ofr.DT,
                 u_ff=i["u_ff"], lag_est=lag, lag_plant=lag, z=i["z"][:1])
    want = fr.rollout(c["model"], fp.RK4, c["lag_mode"], v, law, i["x0_true"], i["ref"], ofr.DT, T=T, u_ff=i["u_ff"], lag=lag[0], z=i["z"][0])
    assert np.all(o["info"][..., 2] == -1)
    e = {k_: float(np.max(np.abs(o[a][0] - want[b]) / np.maximum(1.0, np.abs(want[b]))))
         for k_, a, b in (("traj", "traj", "traj"), ("u", "u", "u"), ("z", "z", "z"), ("lag", "lag_plant", "lag"))}
    e["metrics"] = float(np.max(np.abs(o["metrics"][0][:, :3] - want["metrics"][:, :3]) / np.maximum(1.0, np.abs(want["metrics"][:, :3]))))
    print(e)
    assert max(e.values()) < 0.1 * ofr.TOL_ROLL
    assert np.array_equal(o["metrics"][0][:, 3], want["metrics"][:, 3])
    assert np.max(np.abs(o["xf"][0] - o["traj"][0][:, :T])) < 1e-12 and np.all(o["metrics"][0][:, 4:] < 1e-20)


@pytest.mark.parametrize("name", ["thr_rk4_lagstep", "wr_rk4"])
def test_reference_hold_and_resume(name):
    """the reference holds the command between ticks and, split at a tick, continues from its checkpoint with the same bits, as the
    header says of the entry point"""
    i, c, o = ofr.inputs(name), ofr.case(name), ofr.reference(name)
    T, hold, P = c["T"], c["hold"], c["P"]
    t = np.arange(T)
    assert np.array_equal(o["u"], o["u"][:, :, t - t % hold])
    T1 = (T - 1) // hold * hold
    cut = lambda v, s: None if v is None else v[:, s]
    h = ofr.run_reference(i, V=i["V"][:, :T1], W=cut(i["W"], slice(0, T1)), u_ff=cut(i["u_ff"], slice(0, T1)), ref=i["ref"][:, :T1])
    pick = lambda seq, j: seq[j:j + 1] if len(seq) > 1 else seq
    for j in range(P):
        one = dict(i, models=i["models"][j:j + 1], plants=pick(i["plants"], j), laws=pick(i["laws"], j), cfgs=pick(i["cfgs"], j))
        s = ofr.run_reference(one, x0_true=h["xT_true"][j], x0_est=h["xT"][j], P0=h["PT"][j], V=i["V"][:, T1:], W=cut(i["W"], slice(T1, T)),
                              u_ff=cut(i["u_ff"], slice(T1, T)), ref=i["ref"][:, T1:], lag_est=h["lag_est"][j:j + 1],
                              lag_plant=h["lag_plant"][j:j + 1], z=h["z"][j:j + 1])
        for k in ("y", "u", "xf", "pstd", "innov"):
            assert np.array_equal(np.concatenate([h[k][j], s[k][0]], axis=1), o[k][j], equal_nan=True), k
        assert np.array_equal(np.concatenate([h["traj"][j], s["traj"][0][:, 1:]], axis=1), o["traj"][j])
        for k in ("xT_true", "xT", "PT", "lag_est", "lag_plant", "z"):
            assert np.array_equal(s[k][0], o[k][j]), k
        assert np.array_equal(h["info"][j][:, 1] + s["info"][0][:, 1], o["info"][j][:, 1])


@pytest.mark.parametrize("stage", [1, 2])
def test_reference_failure_patterns_match_the_header(stage):
    """what the header keeps and what it turns into NaN for a stage-1 and for a stage-2 failure at row t = 0, on the reference"""
    name = "thr_rk4"
    i, c = ofr.inputs(name), ofr.case(name)
    P0, V = i["P0"].copy(), i["V"].copy()
    if stage == 1:                           # s = P[0][0] + r[0] <= 0 with component 0 measured at row 0
        P0[1, 0, 0] = -1.0
        V[1, 0, 0] = 0.01
    else:                                    # nothing measured at row 0: the factorisation of an indefinite P0 fails in the predict
        P0[1, 1, 0] = P0[1, 0, 1] = 2.0 * P0[1, 0, 0]
        V[1, 0, :] = np.nan
    o, good = ofr.run_reference(i, P0=P0, V=V), ofr.reference(name)
    n = 0 if stage == 1 else 1
    for j in range(c["P"]):
        assert o["info"][j, 1, 0] == -np.inf and o["info"][j, 1, 2] == 0 and o["info"][j, 1, 1] == 0
        for k in ("xf", "pstd", "innov", "u"):
            assert np.isnan(o[k][j, 1, n:]).all(), k
            if n == 1:                       # row 0 was complete; nothing was measured in it, so its innovations are NaN as in any such row
                assert np.isnan(o[k][j, 1, 0]).all() if k == "innov" else np.isfinite(o[k][j, 1, 0]).all(), k
        assert np.isfinite(o["traj"][j, 1, :n + 1]).all() and np.isnan(o["traj"][j, 1, n + 1:]).all()
        assert np.isnan(o["y"][j, 1, 1:]).all() and np.array_equal(np.isnan(o["y"][j, 1, 0]), np.isnan(V[1, 0]))
        for k in ("xT_true", "xT", "PT", "metrics"):
            assert np.isnan(o[k][j, 1]).all(), k
        assert np.array_equal(o["lag_est"][j, 1], i["lag_est"][j, 1]) and np.array_equal(o["lag_plant"][j, 1], i["lag_plant"][j, 1])
        assert np.array_equal(o["z"][j, 1], i["z"][j, 1])
    others = [0, 2, 3, 4]
    for k in ("traj", "y", "u", "xf", "xT", "PT", "metrics", "info", "z"):
        assert np.array_equal(o[k][:, others], good[k][:, others], equal_nan=True), k
