// ukf_feedback.hip -- output-feedback closed loop: the unscented Kalman filter of ukf.hip inside the time loop of a closed-loop
// rollout (include/brov2.h: brov_output_feedback, which is the specification of the law).  Candidate j pairs a filter model
// params[j] with a plant; the law of rollout_feedback_kernel (feedback.hip) reads the ESTIMATE, the plant sees the command, and
// the filter sees the plant through the caller's noise rows.
//
// The filter's decomposition (ukf.hip's head comment): one wave per (candidate, run), candidate = blockIdx.y, UKF_WAVES runs per
// block, the time loop inside the kernel, the wave's (x, P) image in LDS with the stride-13 rows, ukf_wave_sync between the phases
// and no workgroup barrier after the quadrant table, so a ragged block or a run whose filter failed leaves alone.  The update and
// the predict phases call the functions ukf_filter_kernel calls (brov2_ukf.h: ukf_own, ukf_point, ukf_update<true>, ukf_cholesky_col,
// ukf_mean_dev, ukf_cov, ukf_nan_rows, ukf_put_tail), in its order and around the same sigma step, so that the estimator is that
// filter bit for bit on the rows (u_applied, y_out) this kernel records.  Between them, per step:
//   measure   y = x_true + V[t], lane i its component.
//   command   at a tick every lane evaluates the law of rollout_feedback_kernel (its statements, its fma order) on the tracking error
//             of the filtered mean, read from the image; the feedback record comes through the constant address space, one gain row
//             at a time.  The held command is what both the plant and the sigma points are stepped with.
//   plant     one more GENERIC step_fast, rollout_pop_kernel's, under the plant's own HotConsts and constants pointer (scalar loads:
//             the plant cannot sit on a spare lane of the sigma step, whose constants are the model's).  All 64 lanes take it with
//             equal operands.
// Everything wave-uniform that lives from step to step -- the true state, the plant's lag, the held command, the integral state, the
// metric sums -- lies in the wave's LDS next to the filter's image: the command and plant section reads it into registers, lane 0
// writes it back, and none of it holds a register over the filter's phases, which need nearly all of them.  The filter's own lag
// bank and its pinned vehicle constants, which ukf_filter_kernel keeps in registers, go the same way (the bank through the image,
// the constants re-read at every step), so that the plant's step has the registers the sigma step has.  Lane 0 stores the wave-uniform rows (traj, u_applied); lanes 0..11 store the
// per-component rows.  No atomics.
#include "brov2_device.h"
#include "brov2_error.h"
#include "brov2_fast.h"
#include "brov2_kernels.h"
#include "brov2_rows.h"
#include "brov2_ukf.h"

namespace brov {

typedef const FeedbackRec __attribute__((address_space(4)))* CFBK;
__device__ __forceinline__ CFBK as_constant_fbk(const FeedbackRec* g) { return (CFBK)(unsigned long long)g; }
// makes the compiler re-issue the scalar loads behind `f` here (relaunder in brov2_fast.h, for the feedback record)
__device__ __forceinline__ CFBK relaunder_fbk(CFBK f) {
    asm volatile("" : "+s"(f));
    return f;
}

struct UkfFbLds {
    UkfLds f;                           // the filter's image
    double y[12];                       // the measured row
    double xt[12];                      // the true state
    double plag[24], flag[24];          // the plant's lag and the filter's: per-thruster [8][3] (TRACK), else the acceleration-space bank [6][3]
    double uh[8], z[6];                 // the held command, the integral state
    double m[9];                        // the metric sums [7]; dt |u|^2 and 1 / 0 (a channel on a limit) of the held command
};

template <int MODEL, int INTEG, int LAGMODE, bool TRACK>
__global__ void __launch_bounds__(64 * UKF_WAVES) ukf_feedback_kernel(const UkfFbArgs a) {
    constexpr int NU = Dims<MODEL>::NU;
    constexpr bool THR = MODEL == MODEL_THRUSTER_EULER;
    static_assert(Dims<MODEL>::NX == 12, "the filter's state is the 12-state Euler model");
    __shared__ double2 qt[4];
    __shared__ UkfFbLds lds[UKF_WAVES];
    init_quadrant_table(qt);
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t B = a.B, T = a.T;
    const int64_t b = (int64_t)blockIdx.x * UKF_WAVES + wave;
    if (b >= B) return;                                       // a whole wave: no workgroup barrier follows
    UkfFbLds& Q = lds[wave];
    UkfLds& S = Q.f;
    const int64_t row = (int64_t)blockIdx.y * B + b;          // run b of candidate blockIdx.y in the outputs
    const CFP p = as_constant(a.fp + blockIdx.y);                                    // the filter's model
    const CFP pp = as_constant(a.plant + (a.plant_per_candidate ? blockIdx.y : 0));  // the plant
    const CUK f = as_constant_uk(a.rec + (a.rec_per_candidate ? blockIdx.y : 0));
    const CFBK fb = as_constant_fbk(a.fb + (a.fb_per_candidate ? blockIdx.y : 0));
    const double dt = a.dt;
    const double NaN = __builtin_nan(""), INF = __builtin_inf();
    const UkfOwn own = ukf_own(lane);                         // the entries of P this lane owns
    const int lr = own.lr;                                    // its row in the per-row phases
    int col;                                                  // its sigma point: x + sc L[:, col]
    double sc;
    const double cw = f->c;
    ukf_point(lane, cw, col, sc);

    if constexpr (THR) {
        if (lane < 24) {
            Q.plag[lane] = TRACK ? a.lag_plant[row * 24 + lane] : 0.0;
            Q.flag[lane] = TRACK ? a.lag_est[row * 24 + lane] : 0.0;
        }
    }
    double p0 = a.P0[b * 144 + own.a0 * 12 + own.b0], p1 = a.P0[b * 144 + own.a1 * 12 + own.b1];
    ukf_put_P(S, own, p0, p1);
    const int64_t hold = fb->hold;
    const double hdt = (double)hold * dt;
    const double* vp = a.V + b * T * 12 + lr;
    const double* wp = a.W ? a.W + b * T * 12 : nullptr;
    const double* ufp = a.u_ff ? a.u_ff + b * T * NU : nullptr;
    const double* rp = a.ref + b * a.ref_rows * 12;
    const int64_t rstep = a.ref_rows > 1 ? 12 : 0;            // a set-point has one row
    double* tjp = a.traj ? a.traj + row * (T + 1) * 12 : nullptr;
    double* uap = a.u_applied ? a.u_applied + row * T * NU : nullptr;
    double* yop = a.y_out ? a.y_out + row * T * 12 + lr : nullptr;
    double* xfp = a.xf ? a.xf + row * T * 12 + lr : nullptr;
    double* psp = a.pstd ? a.pstd + row * T * 12 + lr : nullptr;
    double* inp = a.innov ? a.innov + row * T * 12 + lr : nullptr;
    if (lane < 12) {
        S.x[lane] = a.x0_est[b * 12 + lane];
        const double x0 = a.x0_true[b * 12 + lane];
        Q.xt[lane] = x0;
        if (tjp) tjp[lane] = x0;
    }
    if (lane < 8) Q.uh[lane] = 0.0;
    if (lane < 6) Q.z[lane] = a.z ? a.z[row * 6 + lane] : 0.0;
    if (lane < 9) Q.m[lane] = 0.0;
    ukf_wave_sync();

    double ell = 0.0, nupd = 0.0, minpiv = INF;
    int64_t t = 0, failed = -1, nan_from = T, to_tick = 0;
    for (; t < T; ++t) {
        // ---- measure: y = x_true + V[t], lane i its component -------------------------------------------------------------------
        if (lane < 12) {
            const double yv = Q.xt[lane] + vp[t * 12];
            Q.y[lane] = yv;
            if (yop) yop[t * 12] = yv;
        }
        ukf_wave_sync();                                               // y written
        // ---- 1. update with row t, as in ukf_filter_kernel -------------------------------------------------------------------------
        double inn = NaN;
        bool bad = false;
#pragma unroll
        for (int i = 0; i < 12; ++i) ukf_update<true>(S, S.x, f, i, ukf_uniform(Q.y[i]), own, p0, p1, lane, ell, nupd, inn, bad);
        if (bad) { failed = t; nan_from = t; break; }
        if (lane < 12) {
            if (xfp) xfp[t * 12] = S.x[lane];
            if (psp) psp[t * 12] = sqrt(S.P[lane][lane]);
            if (inp) inp[t * 12] = inn;
        }
        // ---- command and plant: wave-uniform.  Every lane forms the same values from the image; lane 0 writes them back, so that ----
        // ---- none of them holds a register over the filter's phases ---------------------------------------------------------------
        {
            double xt[12], xh[12], r[12], e[12], uh[NU];
            load_row<12>(rp, r);
            rp += t + 1 < T ? rstep : 0;
#pragma unroll
            for (int i = 0; i < 12; ++i) { xt[i] = Q.xt[i]; xh[i] = S.x[i]; }
            double usq = Q.m[7], sat = Q.m[8];
            const bool tick = to_tick == 0;                            // controller tick
            if (tick) {
                // the law of rollout_feedback_kernel, on the tracking error of the estimate
                to_tick = hold;
                double uf[NU], z[6];
#pragma unroll
                for (int i = 0; i < NU; ++i) uf[i] = 0.0;
                if (ufp) load_row<NU>(ufp + t * NU, uf);
#pragma unroll
                for (int i = 0; i < 6; ++i) z[i] = Q.z[i];
                tracking_error<MODEL>(xh, r, qt, e);
                double s2 = 0.0;
                bool on = false;
#pragma unroll
                for (int i = 0; i < NU; ++i) {
                    const CFBK g = relaunder_fbk(fb);      // one gain row at a time
                    double v = uf[i];
#pragma unroll
                    for (int j = 0; j < 12; ++j) v = fma(g->K[i][j], e[j], v);
#pragma unroll
                    for (int j = 0; j < 6; ++j) v = fma(g->Ki[i][j], z[j], v);
                    const double lo = g->u_min[i], hi = g->u_max[i];
                    v = fmin(fmax(v, lo), hi);
                    on = on || v == lo || v == hi;
                    s2 = fma(v, v, s2);
                    uh[i] = v;
                }
                usq = dt * s2;
                sat = on ? 1.0 : 0.0;
                const CFBK g = relaunder_fbk(fb);
#pragma unroll
                for (int j = 0; j < 6; ++j) {
                    const double zm = g->z_max[j];
                    z[j] = fmin(fmax(fma(hdt, e[j], z[j]), -zm), zm);
                }
                if (lane == 0) {
#pragma unroll
                    for (int i = 0; i < NU; ++i) Q.uh[i] = uh[i];
#pragma unroll
                    for (int i = 0; i < 6; ++i) Q.z[i] = z[i];
                    Q.m[7] = usq;
                    Q.m[8] = sat;
                }
            } else {
#pragma unroll
                for (int i = 0; i < NU; ++i) uh[i] = Q.uh[i];
            }
            --to_tick;
            if (uap && lane == 0) store_row<NU>(uap + t * NU, uh);
            {   // the metrics: the four of rollout_feedback_kernel on the true state, then the estimation error xf[t] - x_true[t]
                tracking_error<MODEL>(xt, r, qt, e);
                double d[12];
#pragma unroll
                for (int i = 0; i < 12; ++i) {
                    d[i] = xh[i] - xt[i];
                    if (i >= 3 && i < 6) d[i] = ukf_wrap(d[i]);
                }
                double sv = d[6] * d[6];
#pragma unroll
                for (int i = 7; i < 12; ++i) sv = fma(d[i], d[i], sv);
                const double m0 = fma(dt, fma(e[2], e[2], fma(e[1], e[1], e[0] * e[0])), Q.m[0]);
                const double m1 = fma(dt, fma(e[5], e[5], fma(e[4], e[4], e[3] * e[3])), Q.m[1]);
                const double m2 = Q.m[2] + usq, m3 = Q.m[3] + sat;
                const double m4 = fma(dt, fma(d[2], d[2], fma(d[1], d[1], d[0] * d[0])), Q.m[4]);
                const double m5 = fma(dt, fma(d[5], d[5], fma(d[4], d[4], d[3] * d[3])), Q.m[5]);
                const double m6 = fma(dt, sv, Q.m[6]);
                if (lane == 0) { Q.m[0] = m0; Q.m[1] = m1; Q.m[2] = m2; Q.m[3] = m3; Q.m[4] = m4; Q.m[5] = m5; Q.m[6] = m6; }
            }
            // the plant: the general step of rollout_pop_kernel under the plant's constants, its lag through the image
            HotConsts hp;
            load_hot(relaunder(pp), hp);
            LagZ lzp;
            double Xp[8][3];
            if constexpr (THR) {
                if constexpr (TRACK) {
#pragma unroll
                    for (int i = 0; i < 24; ++i) (&Xp[0][0])[i] = Q.plag[i];
                    lzp.from_thrusters(relaunder(pp), Xp);
                } else {
#pragma unroll
                    for (int i = 0; i < 18; ++i) (&lzp.z[0][0])[i] = Q.plag[i];
                }
            }
            step_fast<MODEL, INTEG, LAGMODE, TRACK, true>(hp, pp, dt, xt, uh, lzp, Xp, qt);
            if (wp) {
                double w[12];
                load_row<12>(wp + t * 12, w);
#pragma unroll
                for (int i = 0; i < 12; ++i) xt[i] += w[i];
            }
            if (lane == 0) {
                if constexpr (THR) {
                    if constexpr (TRACK) {
#pragma unroll
                        for (int i = 0; i < 24; ++i) Q.plag[i] = (&Xp[0][0])[i];
                    } else {
#pragma unroll
                        for (int i = 0; i < 18; ++i) Q.plag[i] = (&lzp.z[0][0])[i];
                    }
                }
#pragma unroll
                for (int i = 0; i < 12; ++i) Q.xt[i] = xt[i];
                if (tjp) store_row<12>(tjp + (t + 1) * 12, xt);
            }
            ukf_wave_sync();                                           // the true state, the command and the sums written
        }
        // ---- 2. predict with the applied command, as in ukf_filter_kernel -----------------------------------------------------------
        double Lr[12];
#pragma unroll
        for (int k = 0; k < 12; ++k) Lr[k] = S.P[lr][k];
#pragma unroll
        for (int j = 0; j < 12; ++j) ukf_cholesky_col(S, Lr, j, lane, lr, bad, minpiv);
        if (bad) { failed = t; nan_from = t + 1; break; }
        double x[12], u[NU];
#pragma unroll
        for (int r = 0; r < 12; ++r) x[r] = S.x[r] + sc * S.L[r][col];
#pragma unroll
        for (int i = 0; i < NU; ++i) u[i] = Q.uh[i];
        HotConsts h;
        load_hot(relaunder(p), h);
        LagZ lz;
        double Xl[8][3];
        if constexpr (THR) {
            if constexpr (TRACK) {
#pragma unroll
                for (int i = 0; i < 24; ++i) (&Xl[0][0])[i] = Q.flag[i];
                lz.from_thrusters(relaunder(p), Xl);      // the per-thruster state is the lag state, as in rollout_pop_kernel
            } else {
#pragma unroll
                for (int i = 0; i < 18; ++i) (&lz.z[0][0])[i] = Q.flag[i];
            }
        }
        step_fast<MODEL, INTEG, LAGMODE, TRACK, true>(h, p, dt, x, u, lz, Xl, qt);
        if (lane == 0) {
#pragma unroll
            for (int r = 0; r < 12; ++r) S.c0[r] = x[r];
            // the lag depends on the commands alone: the 64 copies are equal
            if constexpr (THR) {
                if constexpr (TRACK) {
#pragma unroll
                    for (int i = 0; i < 24; ++i) Q.flag[i] = (&Xl[0][0])[i];
                } else {
#pragma unroll
                    for (int i = 0; i < 18; ++i) Q.flag[i] = (&lz.z[0][0])[i];
                }
            }
        }
        ukf_wave_sync();                                               // c0 written
#pragma unroll
        for (int r = 0; r < 12; ++r) {
            double d = x[r] - S.c0[r];
            if (r >= 3 && r < 6) d = ukf_wrap(d);
            if (lane < UKF_NS) S.D[lane][r] = d;
        }
        ukf_wave_sync();                                               // D written
        const double wi = f->wi;
        bool finite = true;
        if (lane < 12) {
            const double m = ukf_mean_dev(S, wi, lane);
            const double xn = S.c0[lane] + m;
            S.m[lane] = m;
            S.x[lane] = xn;
            finite = fabs(xn) < INF;
        }
        const bool allfinite = __ballot(!finite) == 0;
        ukf_wave_sync();                                               // m, x written
        if (!allfinite) { failed = t; nan_from = t + 1; break; }
        ukf_cov(S, f, wi, own, p0, p1);
        ukf_wave_sync();                                               // P written
    }
    // ---- outputs -------------------------------------------------------------------------------------------------------------
    // A failed run keeps what was complete before the failing stage (include/brov2.h): with n = nan_from (t for stage 1, t + 1 for
    // stage 2) the rows xf, pstd, innov, u_applied [n ..), traj [n + 1 ..) and y_out [t + 1 ..) are NaN.
    const bool ok = failed < 0;
    if (!ok) {
        ukf_nan_rows(xfp, 12, psp, inp, lane, nan_from, T);
        if (lane < 12) {
            for (int64_t s = nan_from; s < T; ++s)
                if (tjp) tjp[(s + 1) * 12 + lane] = NaN;
            for (int64_t s = failed + 1; s < T; ++s)
                if (yop) yop[s * 12] = NaN;
        }
        if (uap && lane < NU) {
            for (int64_t s = nan_from; s < T; ++s) uap[s * NU + lane] = NaN;
        }
    }
    if (lane < 12) {
        if (a.xT_true) a.xT_true[row * 12 + lane] = ok ? Q.xt[lane] : NaN;
        if (a.xT) a.xT[row * 12 + lane] = ok ? S.x[lane] : NaN;
    }
    if (a.metrics && lane < 7) a.metrics[row * 7 + lane] = ok ? Q.m[lane] : NaN;
    ukf_put_tail(S, a.PT, a.info, row, lane, ell, nupd, failed, minpiv);
    if (ok) {                                                          // a failed run leaves z_io and both lag banks as they came
        if (a.z && lane < 6) a.z[row * 6 + lane] = Q.z[lane];
        if constexpr (THR && TRACK) {
            if (lane < 24) {
                a.lag_est[row * 24 + lane] = Q.flag[lane];
                a.lag_plant[row * 24 + lane] = Q.plag[lane];
            }
        }
    }
}

// ---------------------------------------------------------------------------------------
// launch: grid (blocks of UKF_WAVES runs, P), as launch_ukf_filter
// ---------------------------------------------------------------------------------------
template <int MODEL, int INTEG, int LAGMODE>
static hipError_t launch_ukf_fb_t(hipStream_t st, int P, const UkfFbArgs& a) {
    if constexpr (MODEL == MODEL_THRUSTER_EULER) {
        if (a.lag_est) return ukf_launch(ukf_feedback_kernel<MODEL, INTEG, LAGMODE, true>, st, P, a);
    }
    return ukf_launch(ukf_feedback_kernel<MODEL, INTEG, LAGMODE, false>, st, P, a);
}
template <int MODEL>
static hipError_t launch_ukf_fb_m(hipStream_t st, int integ, int lag_mode, int P, const UkfFbArgs& a) {
    if (integ == INTEG_EULER) return launch_ukf_fb_t<MODEL, INTEG_EULER, 0>(st, P, a);
    if constexpr (MODEL == MODEL_THRUSTER_EULER) {
        if (lag_mode == 1) return launch_ukf_fb_t<MODEL, INTEG_RK4, 1>(st, P, a);
    }
    return launch_ukf_fb_t<MODEL, INTEG_RK4, 0>(st, P, a);
}
hipError_t launch_ukf_feedback(hipStream_t st, int model, int integ, int lag_mode, int P, const UkfFbArgs& a0) {
    if (a0.B <= 0 || P <= 0) return hipSuccess;
    UkfFbArgs a = a0;
    if (model != MODEL_THRUSTER_EULER || !a.lag_est || !a.lag_plant) a.lag_est = a.lag_plant = nullptr;
    switch (model) {
        case MODEL_THRUSTER_EULER: return launch_ukf_fb_m<MODEL_THRUSTER_EULER>(st, integ, lag_mode, P, a);
        case MODEL_WRENCH_EULER: return launch_ukf_fb_m<MODEL_WRENCH_EULER>(st, integ, lag_mode, P, a);
        default: return hipErrorInvalidValue;     // the filter's models only
    }
}

}  // namespace brov
