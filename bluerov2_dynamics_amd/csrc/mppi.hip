// mppi.hip -- one sampling-based model-predictive (MPPI) update per call: K perturbed command sequences per problem, each rolled out
// H steps through the Fossen model and scored, then combined through a soft-min (include/brov2.h: brov_mppi_step, which is the
// specification of the law).  Two launches, whatever B, K and H are:
//
// mppi_cost_kernel is rollout_pop_kernel (rollout.hip) with the control row replaced by the sample's held knot and the stores by a
// running cost: one lane per sample k, problem = blockIdx.y, vehicle constants through as_constant(pg + blockIdx.y), the GENERIC
// step_fast.  Everything but the noise is block-uniform -- the brov_mppi record, the problem's nominal knots, the reference rows --
// and is read through the constant address space behind a laundered pointer (scalar loads), as feedback.hip reads its gains, never
// held in VGPRs across the time loop.  A lane's own memory traffic is its eps row per knot (none with the seeded stream) and one
// cost store.  The thruster lag: the acceleration-space bank is formed ONCE from the start lag (LagZ::from_thrusters) and carried
// by the non-TRACK step, as rollout_kernel's GENERIC form does; the per-thruster state is neither advanced nor stored (a planning
// rollout is never resumed, so nothing needs the checkpoint property that rollout_pop_kernel pays the TRACK form for).
//
// mppi_update_kernel: one 256-thread block per (knot, problem).  Each block forms beta, eta, sum w^2 and the non-finite count from the
// problem's K costs itself (K loads: cheaper than a third launch), regenerates delta[k][m][.] from the stream (or re-reads eps)
// with the code the cost kernel used -- so the perturbations never exist as a [B][K][M][nu] array -- and reduces w_k delta through
// LDS in a fixed tree: no atomics, the same bits from call to call.  The knots are read from U_old, the copy the cost kernel's
// first block of each problem made, so the shifted store of one block never races another block's read.
#include "brov2_device.h"
#include "brov2_error.h"
#include "brov2_fast.h"
#include "brov2_kernels.h"
#include "brov2_mppi.h"
#include "brov2_rows.h"
#include "brov2_stream.h"

namespace brov {

template <int MODEL, int INTEG, int LAGMODE>
__global__ void __launch_bounds__(256) mppi_cost_kernel(const MppiArgs a) {
    constexpr int NX = Dims<MODEL>::NX, NU = Dims<MODEL>::NU;
    __shared__ double2 qt[4];
    init_quadrant_table(qt);
    __syncthreads();
    const int64_t K = a.K, H = a.H, M = a.M;
    const int64_t b = blockIdx.y;
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (blockIdx.x == 0) {              // the knots as they came, for the update kernel
        const double* src = a.U_nom + b * M * NU;
        double* dst = a.U_old + b * M * NU;
        for (int64_t i = threadIdx.x; i < M * NU; i += blockDim.x) dst[i] = src[i];
    }
    if (k >= K) return;                 // dead lanes have passed the only barrier and store nothing
    const CFP p = as_constant(a.fp + (a.per_problem ? b : 0));
    const CMR f = as_constant_mr(a.rec);
    const CDP un = as_constant_d(a.U_nom + b * M * NU);
    HotConsts h;
    load_hot(p, h);
    double x[NX];
    {
        const CDP xp = as_constant_d(a.x + b * NX);
#pragma unroll
        for (int i = 0; i < NX; ++i) x[i] = xp[i];
    }
    LagZ lz;
    double Xl[8][3];                    // only to form the bank from: the step below does not track it
    if constexpr (MODEL == MODEL_THRUSTER_EULER) {
        if (a.lag) {
            const CDP lp = as_constant_d(a.lag + b * 24);
#pragma unroll
            for (int i = 0; i < 24; ++i) Xl[i / 3][i % 3] = lp[i];
            lz.from_thrusters(relaunder(p), Xl);
        } else lz.zero();
    }
    const double dt = a.dt;
    const int64_t hold = f->hold;
    const uint64_t s2 = a.seed ^ 0xA5A5A5A5A5A5A5A5ull;
    const int64_t rstep = a.ref_total > 1 ? NX : 0;                               // a set-point is one row
    CDP rp = as_constant_d(a.ref + (b * a.ref_total + a.ref_row0) * NX);          // the reference row of the next step
    uint64_t c = (((uint64_t)b * (uint64_t)K + (uint64_t)k) * (uint64_t)M) * (uint64_t)NU;     // counter of (k, knot m, channel 0)
    CDP up = un;                        // the next knot
    int64_t to_knot = 0;
    double v[NU];                       // the held command of this sample
    double S = 0.0, imp = 0.0, usq = 0.0;
#pragma unroll
    for (int i = 0; i < NU; ++i) v[i] = 0.0;
    for (int64_t t = 0; t < H; ++t) {
        double r[NX], e[12];
        {
            const CDP rr = relaunder_d(rp);
#pragma unroll
            for (int i = 0; i < NX; ++i) r[i] = rr[i];
            rp += rstep;
        }
        tracking_error<MODEL>(x, r, qt, e);
        if (to_knot == 0) {             // knot boundary (wave-uniform)
            to_knot = hold;
            double s = 0.0, im = 0.0;
#pragma unroll
            for (int j = 0; j < NU; ++j) {
                const CMR g = relaunder_mr(f);
                const CDP uu = relaunder_d(up);
                const double U = uu[j], sg = g->sigma[j];
                const double vj = mppi_command(U, sg, g->u_min[j], g->u_max[j], a.eps, s2, c + (uint64_t)j, k == 0);
                v[j] = vj;
                s = fma(g->r[j] * vj, vj, s);
                if (sg > 0.0) im = fma(U, (vj - U) / (sg * sg), im);
            }
            usq = s;
            imp += im;
            up += NU;
            c += (uint64_t)NU;
        }
        --to_knot;
        {
            const CMR g = relaunder_mr(f);
            double qs = 0.0;
#pragma unroll
            for (int i = 0; i < 12; ++i) qs = fma(g->q[i] * e[i], e[i], qs);
            S = fma(dt, qs + usq, S);
        }
        step_fast<MODEL, INTEG, LAGMODE, false, true>(h, p, dt, x, v, lz, Xl, qt);
    }
    {                                   // the end state against row ref_row0 + H, then the importance term
        double r[NX], e[12];
        const CDP rr = relaunder_d(rp);
#pragma unroll
        for (int i = 0; i < NX; ++i) r[i] = rr[i];
        tracking_error<MODEL>(x, r, qt, e);
        const CMR g = relaunder_mr(f);
        double qs = 0.0;
#pragma unroll
        for (int i = 0; i < 12; ++i) qs = fma(g->qf[i] * e[i], e[i], qs);
        S += qs;
        S = fma(g->gamma, imp, S);
    }
    a.cost[b * K + k] = S;
}

// fixed tree over NC columns of sh[.][256]: sums, or with MIN the minimum in column 0 and sums in the others
template <int NC, bool MIN>
__device__ __forceinline__ void block_tree(double (*sh)[256], int tid) {
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) {
#pragma unroll
            for (int cidx = 0; cidx < NC; ++cidx) {
                if (MIN && cidx == 0) sh[0][tid] = fmin(sh[0][tid], sh[0][tid + s]);
                else sh[cidx][tid] += sh[cidx][tid + s];
            }
        }
        __syncthreads();
    }
}

template <int NU>
__global__ void __launch_bounds__(256) mppi_update_kernel(const MppiArgs a) {
    __shared__ double sh[2 + 2 * NU][256];
    const int tid = threadIdx.x;
    const int64_t K = a.K, M = a.M;
    const int64_t m = blockIdx.x, b = blockIdx.y;
    const double* __restrict__ cost = a.cost + b * K;
    const CMR f = as_constant_mr(a.rec);
    // beta = the minimum over the finite costs, and how many are not finite
    double mn = __builtin_inf(), bad = 0.0;
    for (int64_t k = tid; k < K; k += 256) {
        const double S = cost[k];
        if (isfinite(S)) mn = fmin(mn, S);
        else bad += 1.0;
    }
    sh[0][tid] = mn;
    sh[1][tid] = bad;
    __syncthreads();
    block_tree<2, true>(sh, tid);
    const double beta = sh[0][0], nbad = sh[1][0];
    __syncthreads();
    const bool none = !(nbad < (double)K);                    // no finite sample: U_nom stays, u_apply is the clamped first knot
    // the knot this block stores (shift: U_nom[m] <- U_new[m + 1], the last repeated); block 0 also forms U_new[0] for u_apply
    const int64_t ms = a.shift ? (m + 1 < M ? m + 1 : M - 1) : m;
    const bool two = m == 0 && ms != 0;
    const double* __restrict__ Uo = a.U_old + b * M * NU;
    const uint64_t s2 = a.seed ^ 0xA5A5A5A5A5A5A5A5ull;
    const double lambda = f->lambda;
    double eta = 0.0, w2 = 0.0, acc[NU], acc0[NU];
#pragma unroll
    for (int j = 0; j < NU; ++j) acc[j] = acc0[j] = 0.0;
    for (int64_t k = tid; k < K; k += 256) {
        const double S = cost[k];
        if (!isfinite(S)) continue;                           // weight 0, and its delta may be NaN
        const double w = exp(-(S - beta) / lambda);
        eta += w;
        w2 = fma(w, w, w2);
        const uint64_t ck = ((uint64_t)b * (uint64_t)K + (uint64_t)k) * (uint64_t)M;
#pragma unroll
        for (int j = 0; j < NU; ++j) {
            const double U = Uo[ms * NU + j];
            const double vj = mppi_command(U, f->sigma[j], f->u_min[j], f->u_max[j], a.eps, s2, (ck + (uint64_t)ms) * NU + j, k == 0);
            acc[j] = fma(w, vj - U, acc[j]);
        }
        if (two) {
#pragma unroll
            for (int j = 0; j < NU; ++j) {
                const double U = Uo[j];
                const double vj = mppi_command(U, f->sigma[j], f->u_min[j], f->u_max[j], a.eps, s2, ck * NU + j, k == 0);
                acc0[j] = fma(w, vj - U, acc0[j]);
            }
        }
    }
    sh[0][tid] = eta;
    sh[1][tid] = w2;
#pragma unroll
    for (int j = 0; j < NU; ++j) sh[2 + j][tid] = acc[j];
    if (two) {
#pragma unroll
        for (int j = 0; j < NU; ++j) sh[2 + NU + j][tid] = acc0[j];
    }
    __syncthreads();
    if (two) block_tree<2 + 2 * NU, false>(sh, tid);          // block-uniform: only block 0 under shift has a second knot to sum
    else block_tree<2 + NU, false>(sh, tid);
    eta = sh[0][0];
    w2 = sh[1][0];
    if (tid < NU) {
        const int j = tid;
        const double lo = f->u_min[j], hi = f->u_max[j];
        if (!none) a.U_nom[(b * M + m) * NU + j] = clip_keep_nan(Uo[ms * NU + j] + sh[2 + j][0] / eta, lo, hi);
    }
    if (m != 0) return;                                       // block-uniform
    double u0 = 0.0;
    if (tid < NU) {
        const int j = tid;
        const double lo = f->u_min[j], hi = f->u_max[j];
        const double d = none ? 0.0 : (two ? sh[2 + NU + j][0] : sh[2 + j][0]) / eta;
        u0 = clip_keep_nan(Uo[j] + d, lo, hi);
    }
    __syncthreads();                                          // every read of the sums is done
    if (tid < NU) sh[0][tid] = u0;
    __syncthreads();
    if (a.u_apply) {
        const int64_t n = (int64_t)f->hold * NU;
        double* dst = a.u_apply + b * n;
        for (int64_t i = tid; i < n; i += 256) dst[i] = sh[0][i % NU];
    }
    if (a.info && tid == 0) {
        double* o = a.info + b * 4;
        o[0] = cost[0];
        o[1] = beta;
        o[2] = none ? 0.0 : eta * eta / w2;
        o[3] = nbad;
    }
}

// ---------------------------------------------------------------------------------------
// launch: cost grid (blocks of K, B) with 64-lane blocks when K <= 64, as launch_rollout_pop; update grid (M, B)
// ---------------------------------------------------------------------------------------
// the update alone (grid (M, B)): what follows any cost kernel that has filled a.cost and a.U_old (koopman_mppi.hip calls it too)
hipError_t launch_mppi_update(hipStream_t st, int nu, int64_t B, const MppiArgs& a) {
    if (nu == 8) hipLaunchKernelGGL((mppi_update_kernel<8>), dim3((unsigned)a.M, (unsigned)B), dim3(256), 0, st, a);
    else if (nu == 6) hipLaunchKernelGGL((mppi_update_kernel<6>), dim3((unsigned)a.M, (unsigned)B), dim3(256), 0, st, a);
    else return hipErrorInvalidValue;
    return hipGetLastError();
}
template <int MODEL, int INTEG, int LAGMODE>
static hipError_t launch_mppi_t(hipStream_t st, int64_t B, const MppiArgs& a) {
    const int bs = a.K <= 64 ? 64 : 256;
    hipLaunchKernelGGL((mppi_cost_kernel<MODEL, INTEG, LAGMODE>), dim3((unsigned)((a.K + bs - 1) / bs), (unsigned)B), dim3(bs), 0, st, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return launch_mppi_update(st, Dims<MODEL>::NU, B, a);
}
template <int MODEL>
static hipError_t launch_mppi_m(hipStream_t st, int integ, int lag_mode, int64_t B, const MppiArgs& a) {
    if (integ == INTEG_EULER) return launch_mppi_t<MODEL, INTEG_EULER, 0>(st, B, a);
    if constexpr (MODEL == MODEL_THRUSTER_EULER) {
        if (lag_mode == 1) return launch_mppi_t<MODEL, INTEG_RK4, 1>(st, B, a);
    }
    return launch_mppi_t<MODEL, INTEG_RK4, 0>(st, B, a);
}
hipError_t launch_mppi_step(hipStream_t st, int model, int integ, int lag_mode, int64_t B, const MppiArgs& a0) {
    if (B <= 0) return hipSuccess;
    if (B > 65535 || a0.K < 1 || a0.H < 1 || a0.M < 1 || a0.M > 0x7fffffff || (a0.K + 63) / 64 > 0x7fffffff) return hipErrorInvalidValue;
    MppiArgs a = a0;
    if (model != MODEL_THRUSTER_EULER) a.lag = nullptr;
    switch (model) {
        case MODEL_THRUSTER_EULER: return launch_mppi_m<MODEL_THRUSTER_EULER>(st, integ, lag_mode, B, a);
        case MODEL_WRENCH_EULER: return launch_mppi_m<MODEL_WRENCH_EULER>(st, integ, lag_mode, B, a);
        case MODEL_WRENCH_QUAT: return launch_mppi_m<MODEL_WRENCH_QUAT>(st, integ, lag_mode, B, a);
        default: return hipErrorInvalidValue;     // the double-integrator gains are not per-problem parameters
    }
}

}  // namespace brov
