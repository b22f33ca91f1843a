"""Shared host-side plumbing of the three drop-in vehicle classes: parameter struct <-> attributes,
one brov_ctx per object, batched helpers."""
import os

import numpy as np

from .. import _lib, engine

_ATTR6 = ("Xu_dot", "Yv_dot", "Zw_dot", "Kp_dot", "Mq_dot", "Nr_dot")
_LIN6 = ("Xu", "Yv", "Zw", "Kp", "Mq", "Nr")
# attributes whose assignment has to reach the device before the next call
_TRACKED = frozenset(("rho", "m", "g", "volume", "xb", "yb", "zb", "Ix", "Iy", "Iz", "current_speed") + _ATTR6 + _LIN6 +
                     tuple(l + "_abs" for l in _LIN6))


class VehicleBase:
    """Holds the vehicle constants as plain attributes (same names as the reference objects,
    fossen/BlueROV2.py:81-140) and mirrors them into the device context before each call."""
    MODEL = None
    _dirty = True
    _cs_pushed = None

    def __setattr__(self, name, value):
        # the reference reads its attributes on every dynamics() call, so an assignment takes effect on the next one; here it
        # marks the object dirty, and a call on a clean object skips the comparison of all constants (the per-call entry
        # points are latency: 40 attribute reads cost as much as the launch)
        if name in _TRACKED:
            object.__setattr__(self, "_dirty", True)
        object.__setattr__(self, name, value)

    def _init_common(self, rho, current_speed, device=None):
        if device is None:
            device = int(os.environ.get("BROV2_DEVICE", os.environ.get("LOCAL_RANK", "0")))
        self._ctx = _lib.Context(device)
        p = self._ctx.get_params()
        self.rho = rho
        self.g, self.m, self.volume = p.g, p.m, p.volume
        self.xg = self.yg = self.zg = 0.0
        self.xb, self.yb, self.zb = p.xb, p.yb, p.zb
        self.Ix, self.Iy, self.Iz = p.Ix, p.Iy, p.Iz
        for i, (a, l) in enumerate(zip(_ATTR6, _LIN6)):
            setattr(self, a, p.added_mass[i])
            setattr(self, l, p.lin_damp[i])
            setattr(self, l + "_abs", p.quad_damp[i])
        self.current_speed = current_speed
        self._pushed = None
        self._params = p

    # Derived quantities.  The reference stores W, B, MRB, MA, M, Minv as plain attributes computed once in __init__ and reads
    # them on every dynamics() call (fossen/BlueROV2.py:96-126,340-355,391).  Here the device holds the primary constants
    # (m, g, rho, volume, inertias, added mass), so the derived ones are views of those: reading always reflects the
    # current primaries; B can be assigned (it maps onto `volume`); the others refuse assignment instead of silently
    # ignoring it.
    @property
    def W(self):
        return self.m * self.g

    @W.setter
    def W(self, v):
        raise AttributeError("W is derived (m * g): set m or g")

    @property
    def B(self):
        return self.rho * self.g * self.volume

    @B.setter
    def B(self, v):
        self.volume = float(v) / (self.rho * self.g)

    @property
    def MRB(self):
        return np.diag([self.m, self.m, self.m, self.Ix, self.Iy, self.Iz]).astype(float)

    @property
    def MA(self):
        return np.diag([-getattr(self, a) for a in _ATTR6]).astype(float)

    @property
    def M(self):
        return self.MRB + self.MA

    @property
    def Minv(self):
        return np.linalg.inv(self.M)

    def _derived_readonly(self, name):
        raise AttributeError(f"{name} is derived from m, Ix..Iz and the added-mass attributes: set those")

    MRB = MRB.setter(lambda self, v: self._derived_readonly("MRB"))
    MA = MA.setter(lambda self, v: self._derived_readonly("MA"))
    M = M.setter(lambda self, v: self._derived_readonly("M"))
    Minv = Minv.setter(lambda self, v: self._derived_readonly("Minv"))

    def _sync_params(self):
        """Push attribute values that differ from what the device context holds.  Fast path: nothing was assigned since the
        last push and the arrays that can be edited in place (current_speed, the thruster geometry) still hold the same bytes."""
        cs = self.current_speed
        csb = b"" if cs is None else np.asarray(cs, dtype=float).tobytes()
        if not self._dirty and csb == self._cs_pushed and self._extra_clean():
            return
        cur = np.zeros(3) if cs is None else np.asarray(cs, dtype=float).reshape(3)
        key = (float(self.rho), float(self.m), float(self.g), float(self.volume), float(self.zb), tuple(cur),
               tuple(float(getattr(self, a)) for a in _ATTR6),
               tuple(float(getattr(self, l)) for l in _LIN6), tuple(float(getattr(self, l + "_abs")) for l in _LIN6),
               float(self.Ix), float(self.Iy), float(self.Iz), float(self.xb), float(self.yb), self._extra_key())
        if key != self._pushed:
            p = self._params
            p.rho, p.m, p.g, p.volume = self.rho, self.m, self.g, self.volume
            p.xb, p.yb, p.zb = self.xb, self.yb, self.zb
            p.Ix, p.Iy, p.Iz = self.Ix, self.Iy, self.Iz
            for i, (a, l) in enumerate(zip(_ATTR6, _LIN6)):
                p.added_mass[i] = getattr(self, a)
                p.lin_damp[i] = getattr(self, l)
                p.quad_damp[i] = getattr(self, l + "_abs")
            for i in range(3):
                p.current[i] = cur[i]
            self._push_extra(p)
            self._ctx.set_params(p)
            self._pushed = key
        object.__setattr__(self, "_dirty", False)
        object.__setattr__(self, "_cs_pushed", csb)
        self._extra_mark_clean()

    def _rhs_single(self, x, u, dt, lag=None):
        """One dynamics() call through preallocated buffers and cached ctypes pointers (the per-call path is latency: the
        generic batched wrapper spends more time converting and allocating than the launch takes).  x, u: anything that
        reshapes to (nx,), (nu,) -- ValueError otherwise, like the reference's reshape.  lag: [8,3] array advanced in place."""
        io = self.__dict__.get("_io")
        if io is None:
            nx, nu = _lib.NX[self.MODEL], _lib.NU[self.MODEL]
            xb, ub, out = np.zeros(nx), np.zeros(nu), np.zeros(nx)
            io = (xb, ub, out, xb.ctypes.data, ub.ctypes.data, out.ctypes.data, nx, nu, self._ctx.lib.brov_rhs)
            object.__setattr__(self, "_io", io)
        xb, ub, out, xp, up, op, nx, nu, fn = io
        xb[...] = np.asarray(x, dtype=float).reshape(nx)
        ub[...] = np.asarray(u, dtype=float).reshape(nu)
        ctx = self._ctx
        if ctx._stream:
            ctx.set_stream(0)          # host path: back to the null stream (see Context.use_null_stream)
        rc = fn(ctx.h, self.MODEL, 1, xp, up, float(dt), lag.ctypes.data if lag is not None else None, op)
        if rc:
            ctx.check(rc, "brov_rhs")
        return out.copy()

    def _extra_clean(self):
        """Model-specific part of the fast check (the thruster model compares its geometry block)."""
        return True

    def _extra_mark_clean(self):
        pass

    def _push_extra(self, p):
        pass

    def _extra_key(self):
        """Model-specific part of the change key (the thruster model adds its geometry)."""
        return ()

    # ---- batched API (new; the reference only has the scalar dynamics()) --------------------
    def rollout(self, x0, U, dt, integrator="euler", lag=None, stride=1, lag_mode=_lib.LAG_PER_CALL):
        """simulate_physics for a batch: x0 [B,nx], U [B,T,nu] -> dict(traj [B,T//stride+1,nx], xT, lag)."""
        self._sync_params()
        return engine.rollout(self.MODEL, integrator, x0, U, dt, lag=lag, lag_mode=lag_mode, stride=stride, ctx=self._ctx)

    def simulate(self, x0, U_seq, dt, integrator="euler"):
        """One trajectory, the reference's simulate_physics signature: returns (len(U_seq)+1, nx).
        Starts from this object's current thruster-lag state and leaves it advanced, like the reference."""
        self._sync_params()
        lag = getattr(self, "_lag", None)
        r = engine.rollout(self.MODEL, integrator, np.asarray(x0, float)[None], np.asarray(U_seq, float)[None], dt,
                           lag=None if lag is None else lag[None], ctx=self._ctx)
        if lag is not None:
            self._lag[...] = r["lag"][0]
        return r["traj"][0]

    def simulate_population(self, x0, U_seq, dt, params_list, integrator="euler"):
        """simulate() for P vehicles in one launch (engine.rollout_pop): returns (P, len(U_seq)+1, nx), row j what simulate
        returns on a fresh vehicle with the parameters params_list[j] (_lib.BrovParams, e.g. identify.sample_parameters' draws).
        Every vehicle starts from zero thruster lag; this object's own lag state and parameters are neither read nor changed."""
        r = engine.rollout_pop(self.MODEL, integrator, list(params_list), np.asarray(x0, float)[None], np.asarray(U_seq, float)[None],
                               dt, ctx=self._ctx)
        return r["traj"][:, 0]

    def simulate_closed_loop(self, x0, ref, dt, feedback, T=None, params_list=None, integrator="euler", hold=None):
        """One trajectory under a feedback law evaluated inside the rollout kernel (engine.rollout_feedback; fossen/control.py builds
        `feedback`): x0 [nx], ref [nx] (a set-point; T required) or [T,nx] (row t tracked at step t).  hold overrides the
        controller period of `feedback`.  Returns (traj [T+1,nx], u [T,nu] the applied commands, metrics [4]).  With params_list
        (P _lib.BrovParams) the same controller runs on P vehicles in one launch and every result gains a leading P axis.
        Starts from zero thruster lag and zero integral state; this object's own lag state is neither read nor changed, and its
        parameters reach the kernel as arguments (params_of), not through the ctx."""
        import ctypes
        from . import identify
        ref = np.asarray(ref, float)
        ref = ref[None] if ref.ndim == 1 else ref
        if T is None and ref.shape[0] == 1:
            raise ValueError("T is needed with a set-point reference")
        if hold is not None:
            fb = _lib.BrovFeedback()
            ctypes.memmove(ctypes.byref(fb), ctypes.byref(feedback), ctypes.sizeof(fb))
            fb.hold = int(hold)
            feedback = fb
        single = params_list is None
        ps = [identify.params_of(self)] if single else list(params_list)
        r = engine.rollout_feedback(self.MODEL, integrator, ps, feedback, np.asarray(x0, float)[None], ref[None], dt, T=T, want_u=True,
                                    ctx=self._ctx)
        out = (r["traj"][:, 0], r["u"][:, 0], r["metrics"][:, 0])
        return tuple(v[0] for v in out) if single else out

    def simulate_output_feedback(self, x0, ref, dt, feedback, cfg, V, T=None, W=None, x0_est=None, P0=None, params_list=None, plant_params=None,
                                 integrator="euler"):
        """One closed loop through the ESTIMATE (engine.output_feedback; include/brov2.h: brov_output_feedback holds the law): the
        unscented Kalman filter of filter_states runs inside the rollout kernel on y = x_true + V[t], and `feedback` reads its
        filtered mean, never the true state.  x0 [12] the plant's start; ref [12] (a set-point) or [T,12]; V [T,12] the measurement
        noise, NaN = not measured at this row (estimate.measurement_noise draws it); W [T,12] an optional process disturbance; T
        defaults to the rows of V and must equal them.  x0_est defaults to x0, P0 to estimate.default_start's diag(4 r) with
        estimate.P0_STAND_IN where r is infinite.  The filter models: this vehicle, or params_list (P _lib.BrovParams, e.g. the draws of
        identify.sample_parameters), and then every result gains a leading P axis.  The plant: plant_params (one _lib.BrovParams),
        default this vehicle -- so params_list alone asks how much model error the estimator-plus-controller pair tolerates on the
        one true vehicle.  Returns dict(traj [T+1,12] the true states, y [T,12], u [T,nu], x [T,12] the filtered means, std, innov
        [T,12], metrics [7], loglik, n_updates, failed_step, min_pivot).  Thruster and Euler-wrench vehicles (the quaternion vehicle
        raises NotImplementedError: its filter, filter_states, does not run inside the loop); starts from zero thruster lag and zero
        integral state; this object's own lag state is neither read nor changed."""
        from . import estimate, identify
        self._euler_only("simulate_output_feedback")
        V = np.asarray(V, float)
        if V.ndim != 2 or V.shape[1] != 12:
            raise ValueError("V must be [T,12]")
        if T is not None and int(T) != V.shape[0]:
            raise ValueError(f"T = {T} but V has {V.shape[0]} rows")
        ref = np.asarray(ref, float)
        ref = ref[None] if ref.ndim == 1 else ref
        x0 = np.asarray(x0, float).reshape(1, 12)
        x0_est = x0 if x0_est is None else np.asarray(x0_est, float).reshape(1, 12)
        if P0 is None:
            r = np.array(list(cfg.r), dtype=float)
            P0 = np.diag(np.where(np.isfinite(r), 4.0 * np.where(np.isfinite(r), r, 0.0), estimate.P0_STAND_IN))
        P0 = np.asarray(P0, float).reshape(1, 12, 12)
        single = params_list is None
        me = identify.params_of(self)
        ps = [me] if single else list(params_list)
        r = engine.output_feedback(self.MODEL, integrator, ps, feedback, cfg, x0, x0_est, P0, V[None], ref[None], dt,
                                   plant_params=me if plant_params is None else plant_params, W=None if W is None else np.asarray(W, float)[None],
                                   ctx=self._ctx)
        out = dict(traj=r["traj"][:, 0], y=r["y"][:, 0], u=r["u"][:, 0], x=r["xf"][:, 0], std=r["pstd"][:, 0], innov=r["innov"][:, 0],
                   metrics=r["metrics"][:, 0], loglik=r["info"][:, 0, 0], n_updates=r["info"][:, 0, 1].astype(np.int64),
                   failed_step=r["info"][:, 0, 2].astype(np.int64), min_pivot=r["info"][:, 0, 3])
        return {k: v[0] for k, v in out.items()} if single else out

    def _ukf_inputs(self, Y, U, cfg, x0, P0, params):
        """What filter_states and smooth_states make of their arguments: (single, Y [B,T,nx], U [B,T,nu], x0 [B,nx], P0 [B,12,12],
        the parameters to filter under), with estimate.default_start where x0 / P0 are None.  The quaternion vehicle: nx = 13,
        estimate.default_start_quat, and the quaternion of a given x0 normalised."""
        from . import estimate, identify
        Y, U = np.asarray(Y, float), np.asarray(U, float)
        single = Y.ndim == 2
        if single:
            Y, U = Y[None], U[None]
        quat = self.MODEL == engine.WRENCH_QUAT
        nx = 13 if quat else 12
        if x0 is None or P0 is None:
            dx0, dP0 = (estimate.default_start_quat if quat else estimate.default_start)(Y, cfg)
        if x0 is None:
            x0 = dx0
        else:
            x0 = np.array(x0, float).reshape(Y.shape[0], nx)
            if quat:
                x0[:, 3:7] /= np.linalg.norm(x0[:, 3:7], axis=1, keepdims=True)
        P0 = dP0 if P0 is None else np.asarray(P0, float).reshape(Y.shape[0], 12, 12)
        return single, Y, U, x0, P0, identify.params_of(self) if params is None else params

    def _ukf_filter(self, integrator, params_list, cfg, x0, P0, U, Y, dt, **kw):
        """engine.ukf_filter, or engine.ukf_filter_quat on the quaternion vehicle"""
        if self.MODEL == engine.WRENCH_QUAT:
            return engine.ukf_filter_quat(integrator, params_list, cfg, x0, P0, U, Y, dt, ctx=self._ctx, **kw)
        return engine.ukf_filter(self.MODEL, integrator, params_list, cfg, x0, P0, U, Y, dt, ctx=self._ctx, **kw)

    def _euler_only(self, what):
        if self.MODEL == engine.WRENCH_QUAT:
            raise NotImplementedError(f"{what}: thruster and Euler-wrench vehicles only; the quaternion vehicle has filter_states and "
                                      "log_likelihood_population")

    @staticmethod
    def _filter_dict(r):
        """the filter's part of the dicts of filter_states and smooth_states, from engine.ukf_filter's / ukf_smooth's outputs at P = 1"""
        return dict(x=r["xf"][0], std=r["pstd"][0], innov=r["innov"][0], xT=r["xT"][0], PT=r["PT"][0], loglik=r["info"][0, :, 0],
                    n_updates=r["info"][0, :, 1].astype(np.int64), failed_step=r["info"][0, :, 2].astype(np.int64), min_pivot=r["info"][0, :, 3])

    def filter_states(self, Y, U, dt, cfg, x0=None, P0=None, params=None, integrator="euler"):
        """Unscented Kalman filter over noisy recordings of the state (engine.ukf_filter; fossen/estimate.py: ukf builds `cfg`;
        include/brov2.h: brov_ukf_filter holds the law).  Y [T,12] or [B,T,12]: the measured state rows, NaN where a component was
        not measured; U [T,nu] or [B,T,nu] the commands.  x0 / P0 default to estimate.default_start: the first fully measured row
        and diag(4 r), with estimate.P0_STAND_IN where r is infinite.  params: a _lib.BrovParams to filter under instead of this
        vehicle's own.  Returns dict(x [.,T,12] the filtered means, std [.,T,12], innov [.,T,12] the normalised innovations (NaN
        where nothing was measured), xT, PT, loglik, n_updates, failed_step (-1: none), min_pivot), without the leading B when Y
        was one recording.  Starts from zero thruster lag; this object's own lag state is neither read nor changed, and its
        parameters reach the kernel as arguments.
        The quaternion vehicle runs the multiplicative filter (engine.ukf_filter_quat; brov_ukf_filter_quat holds the law): Y is
        [.,T,13], x and xT are 13 wide, std, innov, PT and cfg live in the 12-component error state (dp, g, dnu; estimate.quat_boxminus
        gives g), the attitude of a row is measured when none of its four numbers is NaN, the default start is
        estimate.default_start_quat, and the quaternion of a given x0 is normalised here."""
        single, Y, U, x0, P0, p = self._ukf_inputs(Y, U, cfg, x0, P0, params)
        r = self._ukf_filter(integrator, [p], cfg, x0, P0, U, Y, dt)
        out = self._filter_dict(r)
        return {k: v[0] for k, v in out.items()} if single else out

    def smooth_states(self, Y, U, dt, cfg, x0=None, P0=None, params=None, integrator="euler", tape_bytes=0):
        """Unscented Rauch-Tung-Striebel smoother over complete recordings (engine.ukf_smooth; include/brov2.h: brov_ukf_smooth
        holds the law): the estimate of every row from ALL rows, where filter_states uses the rows up to it.  Arguments and
        defaults as filter_states.  Returns the dict of filter_states plus xs [.,T,12] the smoothed means, std_s [.,T,12], Ps
        [.,T,12,12] the smoothed covariances, Ps0 [.,12,12] and failed_transition (-1: none, also where the filter completed no
        row and there was nothing to smooth), without the leading B when Y was one recording.  tape_bytes bounds the library's tape buffer (0: 2 GiB).
        Thruster and Euler-wrench vehicles: on the quaternion vehicle this raises NotImplementedError; smooth_states_quat is its smoother."""
        if self.MODEL == engine.WRENCH_QUAT:
            raise NotImplementedError("smooth_states: thruster and Euler-wrench vehicles only; the quaternion vehicle has smooth_states_quat")
        single, Y, U, x0, P0, p = self._ukf_inputs(Y, U, cfg, x0, P0, params)
        r = engine.ukf_smooth(self.MODEL, integrator, [p], cfg, x0, P0, U, Y, dt, tape_bytes=tape_bytes, ctx=self._ctx)
        return self._smooth_dict(r, single)

    def _smooth_dict(self, r, single):
        """the dict of smooth_states and smooth_states_quat, from engine.ukf_smooth's / ukf_smooth_quat's outputs at P = 1"""
        out = dict(self._filter_dict(r), xs=r["xs"][0], std_s=r["pstd_s"][0], Ps=r["Ps"][0], Ps0=r["Ps0"][0],
                   failed_transition=np.nan_to_num(r["sinfo"][0, :, 0], nan=-1.0).astype(np.int64))
        return {k: v[0] for k, v in out.items()} if single else out

    def smooth_states_quat(self, Y, U, dt, cfg, x0=None, P0=None, params=None, integrator="euler", tape_bytes=0):
        """smooth_states of the quaternion vehicle (engine.ukf_smooth_quat; include/brov2.h: brov_ukf_smooth_quat holds the law).  Arguments
        and defaults as filter_states on that vehicle: Y [.,T,13], the default start of estimate.default_start_quat, the quaternion of a
        given x0 normalised here.  Returns the dict of smooth_states with x, xs and xT 13 wide; std_s, Ps and Ps0 live in the
        12-component error state, and the smoothed quaternion keeps the sign of the filtered one.
        Thruster and Euler-wrench vehicles raise NotImplementedError: smooth_states is their smoother."""
        if self.MODEL != engine.WRENCH_QUAT:
            raise NotImplementedError("smooth_states_quat: the quaternion vehicle only; thruster and Euler-wrench vehicles have smooth_states")
        single, Y, U, x0, P0, p = self._ukf_inputs(Y, U, cfg, x0, P0, params)
        r = engine.ukf_smooth_quat(integrator, [p], cfg, x0, P0, U, Y, dt, tape_bytes=tape_bytes, ctx=self._ctx)
        return self._smooth_dict(r, single)

    def log_likelihood_population(self, params_list, Y, U, dt, cfg, x0=None, P0=None, integrator="euler"):
        """Which of P vehicles explains noisy recordings best: the innovation log-likelihood of filter_states for every candidate
        of params_list (P _lib.BrovParams, e.g. identify.sample_parameters' draws) in one launch.  Y [B,T,12] (or [T,12]), U, cfg,
        x0, P0 as in filter_states.  Returns l [P,B]; -inf where a filter failed.  Unlike the window evaluator's endpoint error this
        does not take the measured rows as truth: noise, dropouts and never-measured components are part of the model.
        The quaternion vehicle: Y [B,T,13] and x0 [B,13], as in filter_states."""
        _, Y, U, x0, P0, _ = self._ukf_inputs(Y, U, cfg, x0, P0, None)
        r = self._ukf_filter(integrator, list(params_list), cfg, x0, P0, U, Y, dt, want=("info",))
        return r["info"][:, :, 0]

    def fit_noise(self, Y, U, dt, cfg, x0=None, P0=None, params=None, integrator="euler", iters=20, tol=1e-4, **kw):
        """Fit the filter's q and r to recordings by expectation-maximisation from the guess `cfg` (fossen/estimate.py: fit_noise; an
        iteration is one engine.ukf_smooth that stores no rows).  Y, U, x0, P0, params and their defaults as smooth_states; x0 and
        P0 come from the START record and are not re-estimated.  kw: fit_q, fit_r (bool or bool[12]), q_floor, r_floor,
        tape_bytes.  Returns dict(cfg: the fitted record, for filter_states / smooth_states, q, r [12], loglik [its + 1] the
        log-likelihood summed over the recordings after each update, q_hist, r_hist [its + 1, 12], n_excluded, converged).
        Thruster and Euler-wrench vehicles: EM needs the smoother, so the quaternion vehicle raises NotImplementedError."""
        from . import estimate
        self._euler_only("fit_noise")
        _, Y, U, x0, P0, p = self._ukf_inputs(Y, U, cfg, x0, P0, params)
        f = estimate.fit_noise(self.MODEL, integrator, [p], cfg, x0, P0, U, Y, dt, iters=iters, tol=tol, ctx=self._ctx, **kw)
        return dict(cfg=f["cfg"][0], q=f["q"][0], r=f["r"][0], loglik=f["loglik"][:, 0], q_hist=f["q_hist"][:, 0], r_hist=f["r_hist"][:, 0],
                    n_excluded=f["n_excluded"], converged=f["converged"])

    def fit_noise_population(self, params_list, Y, U, dt, cfg, x0=None, P0=None, integrator="euler", iters=20, tol=1e-4, **kw):
        """fit_noise for each of P vehicles (params_list) in the same launches: one noise model per candidate, so that
        log_likelihood_population need not score every candidate under one guessed noise model.  cfg: the start, one record or P.
        Returns the dict of estimate.fit_noise (cfg: P records, q, r [P,12], loglik [its + 1, P], ..) plus loglik_fitted [P] =
        loglik[-1], the log-likelihood of each candidate under its own fitted noise, summed over the recordings.  Thruster and
        Euler-wrench vehicles, as fit_noise."""
        from . import estimate
        self._euler_only("fit_noise_population")
        _, Y, U, x0, P0, _ = self._ukf_inputs(Y, U, cfg if isinstance(cfg, _lib.BrovUkf) else cfg[0], x0, P0, None)
        f = estimate.fit_noise(self.MODEL, integrator, list(params_list), cfg, x0, P0, U, Y, dt, iters=iters, tol=tol, ctx=self._ctx, **kw)
        return dict(f, loglik_fitted=f["loglik"][-1])

    def simulate_mppi(self, x0, ref, dt, cfg, T, K, H, plant_params=None, integrator="euler", seed=0, planner=None):
        """Receding-horizon control of B plants by the sampling-based model-predictive update (engine.mppi_step; fossen/control.py:
        mppi builds `cfg`), planned with THIS vehicle's parameters.  The loop is device-resident: the state, the thruster lag and
        the plan never come back to the host between ticks.

        x0 [B,nx] (or [nx], repeated for every plant); ref [nx] or [B,nx] (a set-point) or [B,T+H+1,nx] (row t tracked at step t).
        T steps, a multiple of cfg.hold.  Tick n starts at step n hold: one update with K samples over a horizon of H steps
        (shift=True, seed + n, reference rows from n hold), then hold plant steps on the first knot.  plant_params=None: the plants
        are this vehicle (B from x0); a list of B _lib.BrovParams: plant b runs under plant_params[b] while the planner keeps this
        vehicle's model -- the model-mismatch case.  Every plant starts from zero thruster lag and a zero plan.
        planner=None plans with this vehicle's Fossen model.  An engine.KoopmanPlanner (KoopmanEDMDc.mppi_planner(H, cfg.hold)) plans
        every tick with that learned model instead (edmdc_mppi_step_dev) while the plants stay Fossen vehicles as above: the planner
        sees the state alone, never the thruster lag.
        Returns dict(traj [B,T+1,nx], u [B,T,nu] the applied commands, info [ticks,B,4], ticks = dict(x [ticks,B,nx], lag
        [ticks,B,8,3] | None, U_nom [ticks,B,M,nu], seed [ticks], ref_row0 [ticks]): what the planner saw at each tick, before
        its update)."""
        import ctypes
        from . import identify
        hold, T, K, H = int(cfg.hold), int(T), int(K), int(H)
        if hold < 1 or H < 1 or K < 1:
            raise ValueError("hold, H and K must be >= 1")
        s = self._receding_setup(x0, ref, T, H, hold, plant_params, integrator)
        model, ctx, B, nx, nu = s.model, s.ctx, s.B, s.nx, s.nu
        if planner is not None and (planner.n, planner.r, planner.H, planner.hold) != (nx, nu, H, hold):
            raise ValueError(f"the planner is for n = {planner.n}, r = {planner.r}, H = {planner.H}, hold = {planner.hold}; this call needs {(nx, nu, H, hold)}")
        if planner is not None and planner.ctx.device != ctx.device:
            raise ValueError("the planner's arrays live on another device than this vehicle's")
        plan_params = (_lib.BrovParams * 1)(identify.params_of(self))          # the Fossen planning model: this vehicle
        self._receding_device_state(s)
        D = engine.DevArray
        U = D(ctx, (B, s.M, nu)).zero_()
        info = D(ctx, (max(s.nt, 1), B, 4))
        rec_U = D(ctx, (max(s.nt, 1), B, s.M, nu))
        seeds = []
        p_ = lambda a: None if a is None else a.ptr
        for n in range(s.nt):
            row0, xn = self._receding_tick_begin(s, n)
            seeds.append(int(seed) + n)
            rec_U.rows(n, n + 1).copy_from_device(U)
            if planner is None:
                ctx.check(ctx.lib.brov_mppi_step_dev(ctx.h, model, s.integ, _lib.LAG_PER_CALL, B, 1, plan_params, ctypes.byref(cfg), K, H, float(dt),
                                                     seeds[-1] & 0xFFFFFFFFFFFFFFFF, xn.ptr, p_(s.lag), s.d_ref.ptr, s.ref.shape[1], row0, None, U.ptr, 1,
                                                     s.ua.rows(n, n + 1).ptr, None, info.rows(n, n + 1).ptr), "brov_mppi_step_dev")
            else:
                ctx.check(ctx.lib.edmdc_mppi_step_dev(ctx.h, planner.n, planner.r, planner.k, planner.gamma, p_(planner.C), planner.A.ptr, planner.B.ptr, planner.P.ptr, planner.Gc.ptr, B,
                                                      ctypes.byref(cfg), K, H, float(dt), seeds[-1] & 0xFFFFFFFFFFFFFFFF, xn.ptr, s.d_ref.ptr,
                                                      s.ref.shape[1], row0, None, U.ptr, 1, s.ua.rows(n, n + 1).ptr, None,
                                                      info.rows(n, n + 1).ptr, None), "edmdc_mppi_step_dev")
            self._receding_plant_tick(s, n, dt)
        return self._receding_results(s, info, dict(U_nom=rec_U.numpy()[:s.nt], seed=np.array(seeds, dtype=np.int64)))

    # What simulate_mppi and simulate_lmpc share: the arguments, the device-resident state of the plants, the plant part of a tick and
    # the assembly of the results.  The planners differ in what they carry from tick to tick, which stays with each of them.
    def _receding_setup(self, x0, ref, T, H, hold, plant_params, integrator):
        import types
        from . import identify
        s = types.SimpleNamespace(model=self.MODEL, ctx=self._ctx, hold=hold, H=H)
        s.nx, s.nu = _lib.NX[s.model], _lib.NU[s.model]
        nx = s.nx
        if T < 0 or T % hold:
            raise ValueError(f"T = {T} must be a multiple of hold = {hold}")
        plants = None if plant_params is None else list(plant_params)
        x0 = np.asarray(x0, float)
        if x0.ndim == 1:
            x0 = np.repeat(x0[None], len(plants) if plants else 1, axis=0)
        B = x0.shape[0]
        if x0.shape != (B, nx) or (plants is not None and len(plants) != B):
            raise ValueError(f"x0 must be [B,{nx}] with one row per plant")
        ref = np.asarray(ref, float)
        if ref.ndim == 1:
            ref = np.repeat(ref[None, None], B, axis=0)
        elif ref.ndim == 2:
            ref = ref[:, None]
        s.setpoint = ref.shape[1] == 1
        if ref.shape[0] != B or ref.shape[2] != nx or not (s.setpoint or ref.shape[1] >= T + H + 1):
            raise ValueError(f"ref must be a set-point or [B,T+H+1,{nx}], got {ref.shape}")
        s.x0, s.ref, s.B, s.T = x0, ref, B, T
        s.nt, s.M = T // hold, (H + hold - 1) // hold
        s.integ = engine.INTEGRATORS[integrator]
        s.pa = (_lib.BrovParams * 1)(identify.params_of(self)) if plants is None else (_lib.BrovParams * B)(*plants)
        s.P, s.Bp, s.per = (1, B, 0) if plants is None else (B, 1, 1)          # [1][B] or [B][1] rows: the same bytes either way
        return s

    def _receding_device_state(self, s):
        ctx, B, nx, nu, nt, hold = s.ctx, s.B, s.nx, s.nu, s.nt, s.hold
        ctx.use_null_stream()
        D = engine.DevArray
        s.X = D(ctx, (nt + 1, B, nx))
        s.X.rows(0, 1).copy_from_host(s.x0)
        s.d_ref = D.from_host(ctx, s.ref)
        s.thr = s.model == _lib.THRUSTER_EULER
        s.lag = D(ctx, (B, 8, 3)).zero_() if s.thr else None
        s.traj, s.ua = D(ctx, (max(nt, 1), B, hold + 1, nx)), D(ctx, (max(nt, 1), B, hold, nu))
        s.rec_lag = D(ctx, (max(nt, 1), B, 8, 3)) if s.thr else None
        s.rows = []

    def _receding_tick_begin(self, s, n):
        """records what the planner sees at tick n; returns (first reference row, the state of the tick)"""
        row0 = 0 if s.setpoint else n * s.hold
        s.rows.append(row0)
        if s.thr:
            s.rec_lag.rows(n, n + 1).copy_from_device(s.lag)
        return row0, s.X.rows(n, n + 1)

    def _receding_plant_tick(self, s, n, dt):
        """hold plant steps on the command the planner left in ua[n]"""
        ctx = s.ctx
        ctx.check(ctx.lib.brov_rollout_pop_dev(ctx.h, s.model, s.integ, _lib.LAG_PER_CALL, s.P, s.pa, s.per, s.Bp, s.hold, float(dt),
                                               s.X.rows(n, n + 1).ptr, s.ua.rows(n, n + 1).ptr, None if s.lag is None else s.lag.ptr,
                                               s.traj.rows(n, n + 1).ptr, 1, s.X.rows(n + 1, n + 2).ptr), "brov_rollout_pop_dev")

    def _receding_results(self, s, info, planner_ticks):
        nt = s.nt
        tr = s.traj.numpy()[:nt]                                         # [nt,B,hold+1,nx]: drop every segment's first row but the first's
        states = np.concatenate([s.x0[:, None]] + [tr[n][:, 1:] for n in range(nt)], axis=1)
        u = np.concatenate([s.ua.numpy()[n] for n in range(nt)], axis=1) if nt else np.zeros((s.B, 0, s.nu))
        ticks = dict(x=s.X.numpy()[:nt], lag=s.rec_lag.numpy()[:nt] if s.thr else None, **planner_ticks,
                     ref_row0=np.array(s.rows, dtype=np.int64))
        return dict(traj=states, u=u, info=info.numpy()[:nt], ticks=ticks)

    def simulate_lmpc(self, x0, ref, dt, planner, T, plant_params=None, integrator="euler"):
        """Receding-horizon control of B plants by LINEAR model-predictive control with a learned Koopman model: every tick solves
        the box-constrained QP of an engine.KoopmanLmpc (KoopmanEDMDc.lmpc_planner(H, cfg, dt); edmdc_lmpc_step_dev) from the
        measured state, while the plants are Fossen vehicles as in simulate_mppi: this vehicle, or plant_params[b] for plant b -- the
        model-mismatch case.  The planner sees the state alone, never the thruster lag.  The loop is device-resident: the state, the
        lag, the plan z and the scaled dual variable y never come back to the host between ticks; (z, y) are carried from tick to
        tick, moved one knot forward.

        x0, ref and T as in simulate_mppi with H = planner.H and hold = planner.hold; dt must be the planner's.  Every plant starts
        from zero thruster lag, a zero plan and y = 0.
        Returns dict(traj [B,T+1,nx], u [B,T,nu] the applied commands, info [ticks,B,6] (edmdc_lmpc_step's), ticks = dict(x
        [ticks,B,nx], lag [ticks,B,8,3] | None, U_nom [ticks,B,M,nu], y [ticks,B,M,nu], ref_row0 [ticks]): what the planner saw at
        each tick, before its update)."""
        import ctypes
        hold, H, T = int(planner.hold), int(planner.H), int(T)
        s = self._receding_setup(x0, ref, T, H, hold, plant_params, integrator)
        ctx, B, nu = s.ctx, s.B, s.nu
        if (planner.n, planner.r) != (s.nx, nu):
            raise ValueError(f"the planner is for n = {planner.n}, r = {planner.r}; this vehicle needs {(s.nx, nu)}")
        if float(dt) != planner.dt:
            raise ValueError(f"the planner was condensed for dt = {planner.dt}, not {dt}")
        if planner.ctx.device != ctx.device:
            raise ValueError("the planner's arrays live on another device than this vehicle's")
        self._receding_device_state(s)
        D = engine.DevArray
        U, Y = D(ctx, (B, s.M, nu)).zero_(), D(ctx, (B, s.M, nu)).zero_()
        info = D(ctx, (max(s.nt, 1), B, 6))
        rec_U, rec_Y = D(ctx, (max(s.nt, 1), B, s.M, nu)), D(ctx, (max(s.nt, 1), B, s.M, nu))
        for n in range(s.nt):
            row0, xn = self._receding_tick_begin(s, n)
            rec_U.rows(n, n + 1).copy_from_device(U)
            rec_Y.rows(n, n + 1).copy_from_device(Y)
            ctx.check(ctx.lib.edmdc_lmpc_step_dev(ctx.h, planner.n, planner.r, planner.k, planner.gamma, None if planner.C is None else planner.C.ptr,
                                                  planner.A.ptr, planner.B.ptr, planner.P.ptr, planner.Gc.ptr, planner.W.ptr, B,
                                                  ctypes.byref(planner.cfg), H, float(dt), xn.ptr, s.d_ref.ptr, s.ref.shape[1], row0, U.ptr, Y.ptr, 1,
                                                  s.ua.rows(n, n + 1).ptr, None, info.rows(n, n + 1).ptr), "edmdc_lmpc_step_dev")
            self._receding_plant_tick(s, n, dt)
        return self._receding_results(s, info, dict(U_nom=rec_U.numpy()[:s.nt], y=rec_Y.numpy()[:s.nt]))

    def one_step_rmse(self, X, U, dt):
        """one_step_rmse_physics (training/train_tank_brov2_koopmanEDMDc.py:237-247): Euler one-step predictions over a
        recording with ONE vehicle object (the lag runs through the whole sequence) == the H = 1 window evaluator."""
        return self.multistep_rmse_endpoint(X, U, 1, dt, "euler", carry_lag=True)

    def multistep_rmse_endpoint(self, X, U, H, dt, integrator="euler", carry_lag=True):
        """multistep_rmse_endpoint_physics (training/train_tank_brov2_full_comparison.py:469-487)."""
        self._sync_params()
        return engine.window_rmse(self.MODEL, integrator, X, U, H, dt, carry_lag=carry_lag, ctx=self._ctx)

    def multistep_rmse_endpoint_multi(self, X_list, U_list, H, dt, integrator="euler", carry_lag=True):
        """multistep_rmse_endpoint over several recordings scored together: no window crosses from one recording into the next,
        every recording is a fresh vehicle, and the RMSE is over the windows of all of them (NaN when none has more than H rows).
        U_list[b] is row-aligned with X_list[b] (at least as many rows)."""
        from . import identify
        X, U, off = identify.stack_recordings(X_list, U_list, self.MODEL)
        self._sync_params()
        return engine.window_rmse(self.MODEL, integrator, X, U, H, dt, carry_lag=carry_lag, ctx=self._ctx, bag_offsets=off)

    def fit_parameters(self, X, U, dt, H=10, integrator="euler", assign=True, **kwargs):
        """Fit this vehicle's parameters to a recording (fossen/identify.py: fit_parameters; `free`, `iters`, `weights`, `bounds`,
        ... pass through).  assign=True stores the fitted values in the attributes, so the next call uses them."""
        from . import identify
        res = identify.fit_parameters(self, X, U, dt, H=H, integrator=integrator, **kwargs)
        if assign:
            self._assign_fitted(res)
        return res

    def fit_parameters_multi(self, X_list, U_list, dt, H=10, integrator="euler", assign=True, **kwargs):
        """fit_parameters on several recordings at once (fossen/identify.py: fit_parameters_multi): windows never cross from one
        recording into the next, and every recording starts from zero thruster lag."""
        from . import identify
        res = identify.fit_parameters_multi(self, X_list, U_list, dt, H=H, integrator=integrator, **kwargs)
        if assign:
            self._assign_fitted(res)
        return res

    def _assign_fitted(self, res):
        from . import identify
        cur = None
        for name, value in res.params.items():
            if name in identify._CURRENT:
                if cur is None:
                    cs = self.current_speed
                    cur = np.zeros(3) if cs is None else np.array(cs, dtype=float).reshape(3)
                cur[identify._CURRENT.index(name)] = value
            else:
                setattr(self, name, value)
        if cur is not None:
            self.current_speed = cur
