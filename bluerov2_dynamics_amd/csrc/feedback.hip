// feedback.hip -- closed-loop rollouts: the command of every step is a linear feedback law on the tracking error, evaluated
// inside the time loop (include/brov2.h: brov_rollout_feedback, which is the specification of the law).
//
// rollout_feedback_kernel is rollout_pop_kernel (rollout.hip) with the control row replaced by the law: one lane per trajectory,
// candidate = blockIdx.y, vehicle constants through as_constant(pg + blockIdx.y), the GENERIC step_fast, and with TRACK the
// acceleration-space lag bank re-formed from the per-thruster state at every step -- so (x, lag, z) is the whole checkpoint and
// a call resumed at a controller tick gives the bits of one call.  The feedback record is wave-uniform: it is read through the
// constant address space (scalar loads), one gain row at a time inside the tick, and never held in VGPRs across the time loop.
// A lane carries, besides what rollout_pop_kernel carries: the held command (NU), the integral state (6), four metric sums, the
// two held per-step metric increments, and the next reference / feed-forward rows (prefetched one step ahead).
#include "brov2_device.h"
#include "brov2_error.h"
#include "brov2_fast.h"
#include "brov2_kernels.h"
#include "brov2_rows.h"

namespace brov {

typedef const FeedbackRec __attribute__((address_space(4)))* CFB;
__device__ __forceinline__ CFB as_constant_fb(const FeedbackRec* g) { return (CFB)(unsigned long long)g; }
// makes the compiler re-issue the scalar loads behind `f` here (relaunder in brov2_fast.h, for the feedback record)
__device__ __forceinline__ CFB relaunder_fb(CFB f) {
    asm volatile("" : "+s"(f));
    return f;
}

template <int MODEL, int INTEG, int LAGMODE, bool TRACK>
__global__ void __launch_bounds__(256) rollout_feedback_kernel(const FeedbackArgs a) {
    constexpr int NX = Dims<MODEL>::NX, NU = Dims<MODEL>::NU;
    __shared__ double2 qt[4];
    init_quadrant_table(qt);
    __syncthreads();
    const int64_t B = a.B, T = a.T;
    const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const int64_t row = (int64_t)blockIdx.y * B + b;          // trajectory b of candidate blockIdx.y in the per-candidate arrays
    const int64_t in = a.per_candidate ? row : b;             // its row in x0, u_ff and ref
    const CFP p = as_constant(a.fp + blockIdx.y);
    const CFB f = as_constant_fb(a.fb + (a.fb_per_candidate ? blockIdx.y : 0));
    HotConsts h;
    load_hot(p, h);
    double x[NX];
    load_row<NX>(a.x0 + in * NX, x);
    LagZ lz;
    double Xl[8][3];
    if constexpr (MODEL == MODEL_THRUSTER_EULER) {
        if constexpr (TRACK) load_row<24>(a.lag + row * 24, &Xl[0][0]);
        else lz.zero();
    }
    double z[6];
    if (a.z) load_row<6>(a.z + row * 6, z);
    else {
#pragma unroll
        for (int i = 0; i < 6; ++i) z[i] = 0.0;
    }
    const double dt = a.dt;
    const int64_t hold = f->hold;
    const double hdt = (double)hold * dt;
    const int64_t stride = a.stride;
    double* tp = a.traj ? a.traj + row * (T / stride + 1) * NX : nullptr;        // next trajectory row of this lane
    double* uap = a.u_applied ? a.u_applied + row * T * NU : nullptr;            // next row of the applied commands
    const double* up = a.u_ff ? a.u_ff + in * T * NU : nullptr;
    const int64_t rstep = a.ref_rows > 1 ? NX : 0;                               // a set-point is read once
    const double* rp = a.ref + in * a.ref_rows * NX;
    double un[NU], rn[NX];
#pragma unroll
    for (int i = 0; i < NU; ++i) un[i] = 0.0;
    if (T > 0) {
        load_row<NX>(rp, rn);
        if (up) load_row<NU>(up, un);
    }
    if (tp) { store_row<NX>(tp, x); tp += NX; }
    int64_t countdown = stride, to_tick = 0;
    double uh[NU];                  // the held command
    double usq = 0.0, sat = 0.0;    // dt |u|^2 and 1 / 0 (a channel on a limit) of the held command
    double m0 = 0.0, m1 = 0.0, m2 = 0.0, m3 = 0.0;
#pragma unroll
    for (int i = 0; i < NU; ++i) uh[i] = 0.0;
    for (int64_t t = 0; t < T; ++t) {
        double r[NX], uf[NU], e[12];
#pragma unroll
        for (int i = 0; i < NX; ++i) r[i] = rn[i];
#pragma unroll
        for (int i = 0; i < NU; ++i) uf[i] = un[i];
        // the next reference and feed-forward rows, one step ahead as in rollout_pop_kernel
        if (t + 1 < T) {
            if (rstep) { rp += rstep; load_row<NX>(rp, rn); }
            if (up) { up += NU; load_row<NU>(up, un); }
        }
        tracking_error<MODEL>(x, r, qt, e);
        if (to_tick == 0) {         // controller tick (wave-uniform)
            to_tick = hold;
            double s2 = 0.0;
            bool on = false;
#pragma unroll
            for (int i = 0; i < NU; ++i) {
                const CFB g = relaunder_fb(f);      // one gain row at a time
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
            const CFB g = relaunder_fb(f);
#pragma unroll
            for (int j = 0; j < 6; ++j) {
                const double zm = g->z_max[j];
                z[j] = fmin(fmax(fma(hdt, e[j], z[j]), -zm), zm);
            }
        }
        --to_tick;
        m0 = fma(dt, fma(e[2], e[2], fma(e[1], e[1], e[0] * e[0])), m0);
        m1 = fma(dt, fma(e[5], e[5], fma(e[4], e[4], e[3] * e[3])), m1);
        m2 += usq;
        m3 += sat;
        if (uap) { store_row<NU>(uap, uh); uap += NU; }
        // the per-thruster state is the lag state: the acceleration-space bank is formed from it at every step, not carried
        if constexpr (MODEL == MODEL_THRUSTER_EULER && TRACK) lz.from_thrusters(relaunder(p), Xl);
        step_fast<MODEL, INTEG, LAGMODE, TRACK, true>(h, p, dt, x, uh, lz, Xl, qt);
        if (tp && --countdown == 0) {
            countdown = stride;
            store_row<NX>(tp, x);
            tp += NX;
        }
    }
    if (a.xT) store_row<NX>(a.xT + row * NX, x);
    if constexpr (MODEL == MODEL_THRUSTER_EULER && TRACK) store_row<24>(a.lag + row * 24, &Xl[0][0]);
    if (a.z) store_row<6>(a.z + row * 6, z);
    if (a.metrics) {
        const double m[4] = {m0, m1, m2, m3};
        store_row<4>(a.metrics + row * 4, m);
    }
}

// ---------------------------------------------------------------------------------------
// launch: grid (blocks of B, P), 64-lane blocks when B <= 64, as launch_rollout_pop
// ---------------------------------------------------------------------------------------
template <int MODEL, int INTEG, int LAGMODE>
static hipError_t launch_feedback_t(hipStream_t st, int P, const FeedbackArgs& a) {
    const int bs = a.B <= 64 ? 64 : 256;
    const dim3 grid((unsigned)((a.B + bs - 1) / bs), (unsigned)P);
    if constexpr (MODEL == MODEL_THRUSTER_EULER) {
        if (a.lag) {
            hipLaunchKernelGGL((rollout_feedback_kernel<MODEL, INTEG, LAGMODE, true>), grid, dim3(bs), 0, st, a);
            return hipGetLastError();
        }
    }
    hipLaunchKernelGGL((rollout_feedback_kernel<MODEL, INTEG, LAGMODE, false>), grid, dim3(bs), 0, st, a);
    return hipGetLastError();
}
template <int MODEL>
static hipError_t launch_feedback_m(hipStream_t st, int integ, int lag_mode, int P, const FeedbackArgs& a) {
    if (integ == INTEG_EULER) return launch_feedback_t<MODEL, INTEG_EULER, 0>(st, P, a);
    if constexpr (MODEL == MODEL_THRUSTER_EULER) {
        if (lag_mode == 1) return launch_feedback_t<MODEL, INTEG_RK4, 1>(st, P, a);
    }
    return launch_feedback_t<MODEL, INTEG_RK4, 0>(st, P, a);
}
hipError_t launch_rollout_feedback(hipStream_t st, int model, int integ, int lag_mode, int P, const FeedbackArgs& a0) {
    if (a0.B <= 0 || P <= 0) return hipSuccess;
    FeedbackArgs a = a0;
    if (model != MODEL_THRUSTER_EULER) a.lag = nullptr;
    if (!a.traj) a.stride = 1;
    switch (model) {
        case MODEL_THRUSTER_EULER: return launch_feedback_m<MODEL_THRUSTER_EULER>(st, integ, lag_mode, P, a);
        case MODEL_WRENCH_EULER: return launch_feedback_m<MODEL_WRENCH_EULER>(st, integ, lag_mode, P, a);
        case MODEL_WRENCH_QUAT: return launch_feedback_m<MODEL_WRENCH_QUAT>(st, integ, lag_mode, P, a);
        default: return hipErrorInvalidValue;     // the double-integrator gains are not per-candidate parameters
    }
}

}  // namespace brov
