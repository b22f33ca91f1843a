// koopman_mppi.hip -- the model-predictive (MPPI) update of mppi.hip with a Koopman EDMDc model as the planning model
// (include/brov2.h: edmdc_mppi_step, which is the specification of the law).  The model is linear in the command, so no sample ever
// carries the d = n + k lifted state: with E the first n rows of the identity,
//     x_hat_t = (E A^t) phi(x) + sum_m Gc[t][m] v[k][m]          P[t] = E A^t, Gc[t][m] = the Markov blocks P[j] B summed over knot m
// and the caller passes P and Gc.  Three launches, whatever B, K and H are:
//
// koopman_free_kernel: F[b][t] = P[t] phi(x_b), once per problem.  Block = (chunk of 4 steps, problem); the lift is written once into
// LDS (the code of edmdc_lift: the same bits), then a wave per output row, lanes across the d columns, a fixed shuffle tree.  P is
// re-read from L2 by the B blocks of a chunk; this kernel is not the hot one.  launch_koopman_free launches it alone: the linear MPC of
// koopman_qp.hip starts from the same free response.
//
// koopman_cost_kernel: one lane per sample k, problem = blockIdx.y, as mppi_cost_kernel.  The lane forms its M nu commands once with
// mppi_command (the code and so the bits of mppi.hip; the command cost and the importance term in its order) and keeps them
// lane-major in LDS, v[m][j][lane]: a lane reads only its own column, 8 bytes per lane and row, so no bank conflict and no barrier.
// For each step the state is F[b][t] plus the causal block convolution of the lane's commands with Gc[t][.]: F, Gc, the record and the
// reference rows are block-uniform and come through the constant address space behind a laundered pointer (scalar loads), so every
// v_fma_f64 has one scalar operand and the lane's own traffic is LDS reads.  Sum over m ascending, over j ascending within it, one
// accumulator per output i; the loop bound over m depends on t alone.  Then tracking_error (brov2_error.h), the stage cost, and at
// t = H the terminal cost.  Block size by LDS need: koopman_mppi_block.
//
// The update is mppi_update_kernel (mppi.hip: launch_mppi_update), unchanged: it reads the record, U_old, the costs and eps / seed.
#include "brov2_device.h"
#include "brov2_error.h"
#include "brov2_fast.h"
#include "brov2_kernels.h"
#include "brov2_lift.h"
#include "brov2_mppi.h"

namespace brov {

constexpr int FREE_TCHUNK = 4;          // steps per block of koopman_free_kernel

template <int NS>
__global__ void __launch_bounds__(256) koopman_free_kernel(const KoopmanMppiArgs a) {
    __shared__ double phi[LIFT_NMAX + KOOPMAN_MPPI_MAX_K];
    constexpr int n = NS;
    const int k = a.k, d = n + k;
    const int64_t b = blockIdx.y, H = a.m.H;
    const double* xrow = a.m.x + b * n;
    for (int c = threadIdx.x; c < k; c += 256) {              // phi = [x, rbf], as lift_ref_kernel (edmdc.hip) forms it
        double cc[LIFT_NMAX], c2 = 0.0;
#pragma unroll
        for (int j = 0; j < LIFT_NMAX; ++j) { cc[j] = j < n ? a.C[(int64_t)c * n + j] : 0.0; c2 = fma(cc[j], cc[j], c2); }
        phi[n + c] = rbf_one<NS>(n, a.gamma, xrow, cc, c2);
    }
    if ((int)threadIdx.x < n) phi[threadIdx.x] = xrow[threadIdx.x];
    __syncthreads();
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t t0 = (int64_t)blockIdx.x * FREE_TCHUNK;
    const int64_t left = H + 1 - t0;
    const int rows = (int)(left < FREE_TCHUNK ? left : FREE_TCHUNK) * n;
    for (int row = wave; row < rows; row += 4) {              // row (t, i) of P is row t n + i of [(H+1) n][d]
        const double* __restrict__ p = a.P + (t0 * n + row) * d;
        double s = 0.0;
        for (int c = lane; c < d; c += 64) s = fma(p[c], phi[c], s);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
        if (lane == 0) a.F[(b * (H + 1) + t0) * n + row] = s;
    }
}

template <int N, int NU>
__global__ void __launch_bounds__(256) koopman_cost_kernel(const KoopmanMppiArgs ka) {
    constexpr int MODEL = N == 13 ? MODEL_WRENCH_QUAT : MODEL_WRENCH_EULER;       // the tracking error of the state layout
    static_assert(Dims<MODEL>::NX == N, "n = 12: Euler angles, n = 13: quaternion");
    extern __shared__ double vsh[];     // [M][NU][blockDim.x]: the commands of the block's samples, lane-major
    __shared__ double2 qt[4];
    init_quadrant_table(qt);
    __syncthreads();
    const MppiArgs& a = ka.m;
    const int64_t K = a.K, H = a.H, M = a.M;
    const int64_t b = blockIdx.y;
    const int bs = blockDim.x, tid = threadIdx.x;
    const int64_t k = (int64_t)blockIdx.x * bs + tid;
    if (blockIdx.x == 0) {              // the knots as they came, for the update kernel
        const double* src = a.U_nom + b * M * NU;
        double* dst = a.U_old + b * M * NU;
        for (int64_t i = tid; i < M * NU; i += bs) dst[i] = src[i];
    }
    if (k >= K) return;                 // dead lanes have passed the only barrier and store nothing
    const CMR f = as_constant_mr(a.rec);
    const CDP un = as_constant_d(a.U_nom + b * M * NU);
    const uint64_t s2 = a.seed ^ 0xA5A5A5A5A5A5A5A5ull;
    double* vl = vsh + tid;             // this lane's column: v[m][j] at vl[(m NU + j) bs]
    double imp = 0.0;
    {
        uint64_t c = (((uint64_t)b * (uint64_t)K + (uint64_t)k) * (uint64_t)M) * (uint64_t)NU;     // counter of (k, knot m, channel 0)
        for (int64_t m = 0; m < M; ++m) {
            const CMR g = relaunder_mr(f);
            const CDP uu = relaunder_d(un + m * NU);
            double im = 0.0;
#pragma unroll
            for (int j = 0; j < NU; ++j) {
                const double U = uu[j], sg = g->sigma[j];
                const double vj = mppi_command(U, sg, g->u_min[j], g->u_max[j], a.eps, s2, c + (uint64_t)j, k == 0);
                vl[(m * NU + j) * bs] = vj;
                if (sg > 0.0) im = fma(U, (vj - U) / (sg * sg), im);
            }
            imp += im;
            c += (uint64_t)NU;
        }
    }
    const double dt = a.dt;
    const int64_t hold = f->hold;
    const int64_t rstep = a.ref_total > 1 ? N : 0;                               // a set-point is one row
    CDP rp = as_constant_d(a.ref + (b * a.ref_total + a.ref_row0) * N);          // the reference row of the next step
    CDP fp = as_constant_d(ka.F + b * (H + 1) * N);                              // the free response of the next step
    CDP gp = as_constant_d(ka.Gc);                                               // Gc[t][0] of the next step
    double* pr = ka.pred ? ka.pred + (b * K + k) * (H + 1) * N : nullptr;
    int64_t to_knot = 0, nm = 0;        // nm: the knots that act on the state of this step, m hold < t
    double S = 0.0, usq = 0.0;
    for (int64_t t = 0;; ++t) {
        double x[N], r[N], e[12];
        {
            const CDP ff = relaunder_d(fp);
#pragma unroll
            for (int i = 0; i < N; ++i) x[i] = ff[i];
            fp += N;
        }
        for (int64_t m = 0; m < nm; ++m) {                    // wave-uniform bound
            const CDP g = relaunder_d(gp + m * (N * NU));
            double v[NU];
#pragma unroll
            for (int j = 0; j < NU; ++j) v[j] = vl[(m * NU + j) * bs];
#pragma unroll
            for (int j = 0; j < NU; ++j) {
#pragma unroll
                for (int i = 0; i < N; ++i) x[i] = fma(g[i * NU + j], v[j], x[i]);
            }
        }
        gp += M * (N * NU);
        if (pr) {
#pragma unroll
            for (int i = 0; i < N; ++i) pr[i] = x[i];
            pr += N;
        }
        {
            const CDP rr = relaunder_d(rp);
#pragma unroll
            for (int i = 0; i < N; ++i) r[i] = rr[i];
            rp += rstep;
        }
        tracking_error<MODEL>(x, r, qt, e);
        if (t == H) {                   // the end state against row ref_row0 + H, then the importance term
            const CMR g = relaunder_mr(f);
            double qs = 0.0;
#pragma unroll
            for (int i = 0; i < 12; ++i) qs = fma(g->qf[i] * e[i], e[i], qs);
            S += qs;
            S = fma(g->gamma, imp, S);
            break;
        }
        if (to_knot == 0) {             // knot boundary (wave-uniform): knot nm starts here and acts on the states from t + 1 on
            to_knot = hold;
            const CMR g = relaunder_mr(f);
            double s = 0.0;
#pragma unroll
            for (int j = 0; j < NU; ++j) {
                const double vj = vl[(nm * NU + j) * bs];
                s = fma(g->r[j] * vj, vj, s);
            }
            usq = s;
            ++nm;
        }
        --to_knot;
        {
            const CMR g = relaunder_mr(f);
            double qs = 0.0;
#pragma unroll
            for (int i = 0; i < 12; ++i) qs = fma(g->q[i] * e[i], e[i], qs);
            S = fma(dt, qs + usq, S);
        }
    }
    a.cost[b * K + k] = S;
}

// ---------------------------------------------------------------------------------------
// launch
// ---------------------------------------------------------------------------------------
// The LDS of a block: its samples' commands and the quadrant table of the cost kernel (static, 64 B)
static size_t koopman_block_lds(int64_t mnu, int bs) { return (size_t)mnu * 8 * bs + 4 * sizeof(double2); }
// 256 lanes while two such blocks fit the 160 KB of a CU together (M nu <= 39), else 128 (M nu <= 79), else 64 -- of which three are
// resident up to M nu = 106, two up to 159 and one beyond; 64 when K <= 64
int koopman_mppi_block(int64_t K, int64_t mnu) {
    if (mnu < 1 || mnu > KOOPMAN_MPPI_MAX_MNU) return 0;
    const size_t cu = 160 * 1024;
    const int bs = 2 * koopman_block_lds(mnu, 256) <= cu ? 256 : 2 * koopman_block_lds(mnu, 128) <= cu ? 128 : 64;
    return K <= 64 ? 64 : bs;
}

template <int N, int NU>
static hipError_t launch_koopman_cost(hipStream_t st, int64_t B, const KoopmanMppiArgs& a) {
    const int bs = koopman_mppi_block(a.m.K, a.m.M * NU);
    if (!bs) return hipErrorInvalidValue;
    const size_t lds = (size_t)a.m.M * NU * 8 * bs;
    if (lds > 48 * 1024) {              // beyond the default limit of a launch
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&koopman_cost_kernel<N, NU>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL((koopman_cost_kernel<N, NU>), dim3((unsigned)((a.m.K + bs - 1) / bs), (unsigned)B), dim3(bs), lds, st, a);
    return hipGetLastError();
}

hipError_t launch_koopman_free(hipStream_t st, int64_t B, const KoopmanMppiArgs& a) {
    if (B <= 0) return hipSuccess;
    const MppiArgs& m = a.m;
    if (B > 65535 || m.H < 1 || a.k < 0 || a.k > KOOPMAN_MPPI_MAX_K || (a.n != 12 && a.n != 13) || (m.H + FREE_TCHUNK) / FREE_TCHUNK > 0x7fffffff)
        return hipErrorInvalidValue;
    const dim3 fgrid((unsigned)((m.H + FREE_TCHUNK) / FREE_TCHUNK), (unsigned)B);       // ceil((H + 1) / chunk)
    if (a.n == 12) hipLaunchKernelGGL(koopman_free_kernel<12>, fgrid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL(koopman_free_kernel<13>, fgrid, dim3(256), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_koopman_mppi_step(hipStream_t st, int64_t B, const KoopmanMppiArgs& a) {
    if (B <= 0) return hipSuccess;
    const MppiArgs& m = a.m;
    if (B > 65535 || m.K < 1 || m.H < 1 || m.M < 1 || m.M > 0x7fffffff || (m.K + 63) / 64 > 0x7fffffff || a.k < 0 || a.k > KOOPMAN_MPPI_MAX_K ||
        (a.n != 12 && a.n != 13) || (a.r != 6 && a.r != 8) || (m.H + FREE_TCHUNK) / FREE_TCHUNK > 0x7fffffff)
        return hipErrorInvalidValue;
    hipError_t e = launch_koopman_free(st, B, a);
    if (e != hipSuccess) return e;
    if (a.n == 12) e = a.r == 8 ? launch_koopman_cost<12, 8>(st, B, a) : launch_koopman_cost<12, 6>(st, B, a);
    else e = a.r == 8 ? launch_koopman_cost<13, 8>(st, B, a) : launch_koopman_cost<13, 6>(st, B, a);
    if (e != hipSuccess) return e;
    return launch_mppi_update(st, a.r, B, m);
}

}  // namespace brov
