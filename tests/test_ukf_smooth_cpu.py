"""The smoother's law on the reference alone (tests/ukf_smooth_ref.py), no GPU: the eight problems of tests/ukf_cases.py are
well-posed for the backward pass too, so that tests/test_ukf_smooth_gpu.py may hold the kernels to the bound of
tests/test_ukf_gpu.py (1e-10, the fp64 against long-double gap of the reference below a tenth of it, pivots above 1e-4, no wrap
within 1e-6 of its threshold), and the smoother does what a smoother is for."""
import numpy as np
import pytest

import ukf_cases as uc
import ukf_smooth_cases as us

TRUE = uc.NAMES.index(uc.TRUE)
SCORED = [k for k in range(12) if k not in (5, uc.UNMEASURED)]        # the measured components other than yaw


@pytest.mark.parametrize("name", us.NAMES)
def test_cases_are_well_posed_for_the_smoother(name):
    o, ol = us.reference(name), us.reference(name, ld=True)
    g = us.gaps(o, ol)
    print(name, {k: f"{v:.1e}" for k, v in g.items()}, "pivots", o["rts_pivot_min"].min(), "C form", o["c_form"].max())
    for k, v in g.items():
        assert v < 0.1 * us.TOL, (name, k, v)
    for r in (o, ol):
        assert np.all(r["nrows"] == uc.T) and np.all(r["sinfo"][..., 0] == -1)
        assert min(r["rts_pivot_min"].min(), r["pivot_min"].min()) > us.PIVOT
        assert r["wrap_margin"].min() > us.MARGIN
        assert r["c_form"].max() < 1e-12, "the compact form of C against the textbook sum over the sigma points"
        assert np.array_equal(r["sinfo"][..., 1], r["rts_pivot_min"])
    # the forward pass of the smoother's reference is the filter's reference
    f = uc.reference(name)
    for k in ("xf", "pstd", "innov", "xT", "PT", "info", "lag"):
        assert np.array_equal(o[k], f[k], equal_nan=True), k


@pytest.mark.parametrize("name", us.NAMES)
def test_smoothing_helps_and_never_widens(name):
    o, X = us.reference(name), uc.inputs(name)["X"][:, :uc.T]
    rmse = lambda x: float(np.sqrt(np.mean((x[TRUE][..., SCORED] - X[..., SCORED]) ** 2)))
    print(name, "RMSE at the true vehicle, filtered", rmse(o["xf"]), "smoothed", rmse(o["xs"]))
    assert rmse(o["xs"]) < rmse(o["xf"])
    dPf, dPs = (np.diagonal(o[k], axis1=-2, axis2=-1) for k in ("Pf", "Ps"))
    assert np.all(dPs <= dPf), "a smoothed variance above the filtered one"
    assert np.array_equal(dPs[:, :, -1], dPf[:, :, -1]) and np.array_equal(o["xs"][:, :, -1], o["xf"][:, :, -1])
    assert np.array_equal(o["Ps"], o["Ps"].transpose(0, 1, 2, 4, 3))


@pytest.mark.parametrize("name", us.NAMES)
def test_split_span_is_exact(name):
    """filter rows 0..4, filter rows 5..11 from (xT, PT, lag), smooth the second span, smooth the first with the second's
    (xs[0], Ps0) as its terminal pair: the unbroken result, bit for bit"""
    i, whole = uc.inputs(name), us.reference(name)
    h = us.smooth(name, U=i["U"][:, :us.T1], Y=i["Y"][:, :us.T1])
    second = us.smooth(name, x0=h["xT"], P0=h["PT"], U=i["U"][:, us.T1:], Y=i["Y"][:, us.T1:], lag=None if i["lag"] is None else h["lag"])
    first = us.smooth(name, U=i["U"][:, :us.T1], Y=i["Y"][:, :us.T1], terminal=(second["xs"][:, :, 0], second["Ps0"]))
    for k in ("xs", "pstd_s", "Ps"):
        assert np.array_equal(np.concatenate([first[k], second[k]], axis=2), whole[k]), k
    assert np.array_equal(first["Ps0"], whole["Ps0"])


def test_valid_prefix_and_backward_failure_in_the_reference():
    """nrows and the NaN pattern of the law: an indefinite P0 (stage 2 of row 0 fails: n = 1, row 0 keeps the filter's values), and a
    tape whose Pp block of transition 6 is made indefinite (rows <= 6 NaN, rows > 6 kept)"""
    import ukf_smooth_ref as usr
    name = "wr_euler"
    i, clean = uc.inputs(name), us.reference(name)
    P0 = i["P0"].copy()
    P0[1, 1, 0] = 2.0 * P0[1, 0, 0]
    Y = i["Y"].copy()
    Y[:, 0] = np.nan
    o = us.smooth(name, P0=P0, Y=Y)
    assert np.all(o["nrows"][:, 1] == 1) and np.all(o["nrows"][:, [0, 2]] == uc.T)
    assert np.array_equal(o["xs"][:, 1, 0], o["xf"][:, 1, 0]) and np.isnan(o["xs"][:, 1, 1:]).all() and np.isfinite(o["Ps0"][:, 1]).all()
    assert np.isnan(o["tape"][:, 1, 0, 78:]).all() and np.isfinite(o["tape"][:, 1, 0, :78]).all() and np.isnan(o["tape"][:, 1, 1:]).all()
    tape = clean["tape"][0, 0].copy()
    bad = usr.unpack(tape[6, usr.PP], np.float64)
    bad[1, 0] = bad[0, 1] = 2.0 * bad[0, 0]
    tape[6, usr.PP] = usr.pack(bad)
    r = usr.rts_one(clean["xf"][0, 0], tape, uc.T, np.float64)
    assert r["sinfo"][0] == 6 and np.isnan(r["xs"][:7]).all() and np.isnan(r["Ps0"]).all()
    assert np.array_equal(r["xs"][7:], clean["xs"][0, 0, 7:]) and np.array_equal(r["Ps"][7:], clean["Ps"][0, 0, 7:])


def test_stage_one_failure_at_a_later_row_in_the_reference():
    """the inputs of tests/test_ukf_smooth_gpu.py::test_valid_prefix_in_every_wave_slot for a stage-1 failure at row 6: q[0] = 5e305,
    r[0] = 1.797e308 and component 0 measured in row 6 of recording 1 alone.  s = P[0][0] + r[0] overflows there (n = 6, transition
    5 -> 6 complete, rows < 6 smoothed from Pf_5), nothing overflows before, and the recordings that never measure it complete."""
    import ukf_ref as ur
    import ukf_smooth_ref as usr
    name = "thr_rk4_ragged"
    i = uc.inputs(name)
    good = i["cfgs"]
    q, r = good.q.copy(), good.r.copy()
    q[0], r[0] = 5e305, 1.797e308
    Y = i["Y"].copy()
    Y[:, :, 0] = np.nan
    Y[1, 6, 0] = i["X"][1, 6, 0]
    with np.errstate(over="ignore"):
        o = us.smooth(name, cfgs=ur.Cfg(q=q, r=r, alpha=good.alpha, beta=good.beta, kappa=good.kappa), Y=Y)
    want = np.full((2, i["B"]), float(uc.T))
    want[:, 1] = 6
    assert np.array_equal(o["nrows"], want) and np.all(o["info"][:, 1, 2] == 6) and np.all(o["info"][:, [0, 2, 3, 4], 2] == -1)
    assert np.isfinite(o["tape"][:, 1, :6]).all() and np.isnan(o["tape"][:, 1, 6:]).all() and np.isfinite(o["tape"][:, [0, 2, 3, 4]]).all()
    assert np.isfinite(o["xs"][:, 1, :6]).all() and np.isnan(o["xs"][:, 1, 6:]).all() and np.all(o["sinfo"][..., 0] == -1)
    P00 = o["tape"][..., usr.PF][..., 0]
    assert 13.0 * np.nanmax(P00) < 1e308 and np.all(P00[:, 1, 5] > 10.0 * (np.finfo(float).max - r[0])), "far from either edge"
