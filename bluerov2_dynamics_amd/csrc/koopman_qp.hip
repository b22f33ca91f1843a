// koopman_qp.hip -- linear model-predictive control on the coefficients of koopman_mppi.hip: per problem the box-constrained QP
//     min 1/2 v' Hq v + g' v,  u_min <= v <= u_max
// solved by scaled ADMM (include/brov2.h: edmdc_lmpc_step, which is the specification of the law).  Hq is one matrix for every
// problem; the caller passes W = (Hq + rho I)^-1.  Three launches, whatever B, H and iters are:
//
// koopman_free_kernel (koopman_mppi.hip: launch_koopman_free): F[b][t] = P[t] phi(x_b), the code and so the bits of edmdc_mppi_step.
//
// koopman_qp_grad_kernel: block = problem, lanes across the Nv columns of Gc[t].  The adjusted reference, e0_t = F[t] - rt_t and the
// weights are block-uniform: x, the reference rows, F and the record come through the constant address space behind a laundered
// pointer (scalar loads), and every lane forms the n products w_t Q_t[i] e0_t[i] of a step itself.  Its own column of Gc[t] is a
// per-lane address and comes through vector loads (runs of nu doubles).  Sum over t ascending, i ascending within it, one accumulator
// per column; g = 2 acc.  c = J(0) in the order of the cost.
//
// koopman_qp_solve_kernel: one wave per problem, four problems per 256-thread block; the whole iteration loop runs in this launch.
// Lane l owns the rows l, l + 64, ... (at most five at Nv = 312) and keeps their z, y, g and limits in registers; only what other
// lanes read lives in the wave's LDS slice: s = rho (z - y) - g, and for the epilogue z and z0 (3 Nv doubles per wave).
// v_i = sum_j W[j][i] s_j uses the symmetry of W: row j is read contiguously across the lanes (8 bytes per lane: no bank conflict),
// s_j is an LDS broadcast; j ascending, one accumulator per owned row; the loads of QP_JB rows are issued before the first is used, so
// that a wave alone on its SIMD has them in flight together.  W is staged once per block into LDS while two such blocks
// fit the 160 KB of a CU together (koopman_qp_block: Nv <= 95), else it is read from global memory: it is shared by every problem,
// at most 779 KB, and stays in L2.  The residual maxima take the fixed __shfl_xor tree, so the stop test is wave-uniform; nothing
// after the staging barrier is a block barrier, so a wave that has stopped cannot stall its neighbours.
// Epilogue, same wave: lanes across the steps t; each forms x_hat_t under z and under z0 (m ascending, j ascending: the order of
// koopman_cost_kernel) from one pass over Gc[t], the stage cost of both, and the sums over t take the per-lane order (t = l, l + 64,
// ...) and then the fixed tree.  Then the shift, u_apply and info.
#include <atomic>

#include "brov2_device.h"
#include "brov2_kernels.h"
#include "brov2_mppi.h"

namespace brov {

typedef const LmpcRec __attribute__((address_space(4)))* CLR;
__device__ __forceinline__ CLR as_constant_lr(const LmpcRec* g) { return (CLR)(unsigned long long)g; }
__device__ __forceinline__ CLR relaunder_lr(CLR f) {
    asm volatile("" : "+s"(f));
    return f;
}

constexpr double QP_TWO_PI = 6.283185307179586476925286766559;
constexpr int QP_MAX_ROWS = (KOOPMAN_MPPI_MAX_MNU + 63) / 64;      // rows a lane owns at most
constexpr int QP_MAX_DEVICES = 64;                               // devices whose raised LDS limit is remembered
constexpr int QP_JB = 8;                                         // rows of W whose loads a wave issues before it uses the first

// The reference row r (in registers) adjusted once against the measured state x: the angles to within pi of x (n = 12), the
// quaternion to the hemisphere of x's (n = 13)
template <int N>
__device__ __forceinline__ void adjust_reference(const double (&x)[N], double (&r)[N]) {
    if (N == 12) {
#pragma unroll
        for (int i = 3; i < 6; ++i) r[i] = fma(-QP_TWO_PI, rint((r[i] - x[i]) / QP_TWO_PI), r[i]);
    } else {
        double s = 0.0;
#pragma unroll
        for (int i = 3; i < 7; ++i) s = fma(x[i], r[i], s);
        if (s < 0.0) {
#pragma unroll
            for (int i = 3; i < 7; ++i) r[i] = -r[i];
        }
    }
}

// max that keeps a NaN from either side
__device__ __forceinline__ double nanmax(double a, double b) { return (a > b || a != a) ? a : b; }

// LDS written by some lanes of a wave is read by others: order the two
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_wave_barrier();
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
}

template <int N, int NU>
__global__ void __launch_bounds__(320) koopman_qp_grad_kernel(const KoopmanQpArgs qa) {
    const MppiArgs& a = qa.f.m;
    const int64_t b = blockIdx.x, H = a.H, M = a.M;
    const int nv = (int)(M * NU), col = threadIdx.x;
    const bool live = col < nv;
    const CLR f = as_constant_lr(qa.rec);
    const int64_t hold = f->hold;
    double x[N];
    {
        const CDP xp = as_constant_d(a.x + b * N);
#pragma unroll
        for (int i = 0; i < N; ++i) x[i] = xp[i];
    }
    const int64_t rstep = a.ref_total > 1 ? N : 0;                               // a set-point is one row
    CDP rp = as_constant_d(a.ref + (b * a.ref_total + a.ref_row0) * N);          // the reference row of the next step
    CDP fp = as_constant_d(qa.f.F + b * (H + 1) * N);                            // the free response of the next step
    const int m = live ? col / NU : 0, j = live ? col - m * NU : 0;
    const double* gc = qa.f.Gc + (int64_t)m * (N * NU) + j;                      // Gc[t][m][i][j] = gc[t M N NU + i NU]
    const int64_t first = (int64_t)m * hold;                                     // knot m acts on the states t > m hold
    const double dt = a.dt;
    double acc = 0.0, c = 0.0;
    for (int64_t t = 0; t <= H; ++t) {
        const bool last = t == H;
        double r[N], s[N];
        {
            const CDP rr = relaunder_d(rp);
#pragma unroll
            for (int i = 0; i < N; ++i) r[i] = rr[i];
            rp += rstep;
        }
        adjust_reference<N>(x, r);
        {
            const CDP ff = relaunder_d(fp);
            const CLR g = relaunder_lr(f);
            double qs = 0.0;
#pragma unroll
            for (int i = 0; i < N; ++i) {
                const double e0 = ff[i] - r[i];
                const double qi = last ? g->qf[i] : g->q[i];
                s[i] = (last ? qi : dt * qi) * e0;
                qs = fma(qi * e0, e0, qs);
            }
            fp += N;
            c = last ? c + qs : fma(dt, qs, c);
        }
        if (live && t > first) {
            const double* __restrict__ gt = gc + t * M * (N * NU);
#pragma unroll
            for (int i = 0; i < N; ++i) acc = fma(gt[i * NU], s[i], acc);
        }
    }
    if (live) qa.g[b * nv + col] = 2.0 * acc;
    if (col == 0) qa.c0[b] = c;
}

struct QpState {
    double rp, rd;
    int it, nbound;
    bool bad;
};

// The iteration of one problem by one wave.  WL: W is the block's LDS copy.  On return zs holds z and z0s the start point; U and y
// (in place: every load of them comes before any store, in this wave's program order) have received z and y, shifted when asked.
template <int Q, int NU, bool WL>
__device__ __forceinline__ QpState qp_solve(const double* wl, const double* __restrict__ wg, const int nv, const int lane, const LmpcRec* rec,
                                            double* U, double* yio, const double* __restrict__ gin, const double c0, const bool shift,
                                            double* s, double* zs, double* z0s) {
    const double rho = rec->rho, tol = rec->tol;
    const int iters = rec->iters;
    int idx[Q], ic[Q];
    bool own[Q];
    double z[Q], y[Q], g[Q], lo[Q], hi[Q];
    bool fin = isfinite(c0);
#pragma unroll
    for (int q = 0; q < Q; ++q) {
        idx[q] = lane + 64 * q;
        own[q] = idx[q] < nv;
        ic[q] = own[q] ? idx[q] : nv - 1;                     // a lane without a row in this group reads a valid one and stores nothing
        const int j = ic[q] % NU;
        lo[q] = rec->u_min[j];
        hi[q] = rec->u_max[j];
        g[q] = gin[ic[q]];
        y[q] = yio ? yio[ic[q]] : 0.0;
        z[q] = clip_keep_nan(U[ic[q]], lo[q], hi[q]);
        if (own[q]) {
            z0s[idx[q]] = z[q];
            zs[idx[q]] = z[q];
            fin = fin && isfinite(g[q]);
        }
    }
    wave_sync();
    QpState o;
    o.rp = o.rd = __builtin_huge_val();
    o.it = 0;
    o.nbound = 0;
    o.bad = !__all(fin);
    if (o.bad) return o;
    while (o.it < iters) {
#pragma unroll
        for (int q = 0; q < Q; ++q)
            if (own[q]) s[idx[q]] = fma(rho, z[q] - y[q], -g[q]);
        wave_sync();
        double v[Q];
#pragma unroll
        for (int q = 0; q < Q; ++q) v[q] = 0.0;
        int j = 0;
#pragma unroll 1
        for (; j + QP_JB <= nv; j += QP_JB) {                 // the loads of QP_JB rows first, so that they are in flight together;
            double sj[QP_JB], w[QP_JB][Q];                    // then the sums in the order of the plain loop below
#pragma unroll
            for (int u = 0; u < QP_JB; ++u) {
                sj[u] = s[j + u];
                const double* row = WL ? wl + (j + u) * nv : wg + (int64_t)(j + u) * nv;
#pragma unroll
                for (int q = 0; q < Q; ++q) w[u][q] = row[ic[q]];
            }
#pragma unroll
            for (int u = 0; u < QP_JB; ++u) {
#pragma unroll
                for (int q = 0; q < Q; ++q) v[q] = fma(w[u][q], sj[u], v[q]);
            }
        }
        for (; j < nv; ++j) {
            const double sj = s[j];
            const double* row = WL ? wl + j * nv : wg + (int64_t)j * nv;
#pragma unroll
            for (int q = 0; q < Q; ++q) v[q] = fma(row[ic[q]], sj, v[q]);
        }
        wave_sync();                                          // every read of s is done before the next iteration writes it
        double p = 0.0, dd = 0.0;
#pragma unroll
        for (int q = 0; q < Q; ++q) {
            const double t = v[q] + y[q];
            const double zn = clip_keep_nan(t, lo[q], hi[q]);
            if (own[q]) {
                p = nanmax(p, fabs(v[q] - zn));
                dd = nanmax(dd, fabs(zn - z[q]));
            }
            y[q] = t - zn;
            z[q] = zn;
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            p = nanmax(p, __shfl_xor(p, off));
            dd = nanmax(dd, __shfl_xor(dd, off));
        }
        o.rp = p;
        o.rd = rho * dd;
        ++o.it;
        if (tol > 0.0 && o.rp <= tol && o.rd <= tol) break;   // wave-uniform: every lane holds the same maxima
    }
    int cnt = 0;
#pragma unroll
    for (int q = 0; q < Q; ++q) {
        if (!own[q]) continue;
        const int i = idx[q];
        zs[i] = z[q];
        cnt += (z[q] == lo[q] || z[q] == hi[q]) ? 1 : 0;
        if (!shift) {
            U[i] = z[q];
            if (yio) yio[i] = y[q];
        } else {                                              // knot m goes to m - 1; the last knot stays as well
            if (i >= NU) {
                U[i - NU] = z[q];
                if (yio) yio[i - NU] = y[q];
            }
            if (i >= nv - NU) {
                U[i] = z[q];
                if (yio) yio[i] = y[q];
            }
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) cnt += __shfl_xor(cnt, off);
    o.nbound = cnt;
    wave_sync();
    return o;
}

template <int N, int NU>
__global__ void __launch_bounds__(64 * KOOPMAN_QP_WAVES) koopman_qp_solve_kernel(const KoopmanQpArgs qa, const int64_t B, const int w_in_lds) {
    extern __shared__ double qsh[];     // [W: Nv x Nv when staged][wave][s | z | z0][Nv]
    const MppiArgs& a = qa.f.m;
    const int64_t H = a.H, M = a.M;
    const int nv = (int)(M * NU);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (w_in_lds) {
        for (int i = threadIdx.x; i < nv * nv; i += 64 * KOOPMAN_QP_WAVES) qsh[i] = qa.W[i];
        __syncthreads();                // the only block barrier: every wave, with or without a problem, has passed it
    }
    const int64_t b = (int64_t)blockIdx.x * KOOPMAN_QP_WAVES + wave;
    if (b >= B) return;
    double* s = qsh + (w_in_lds ? nv * nv : 0) + wave * 3 * nv;
    double* zs = s + nv;
    double* z0s = zs + nv;
    const LmpcRec* rec = qa.rec;
    double* U = a.U_nom + b * nv;
    double* yio = qa.y ? qa.y + b * nv : nullptr;
    const double* gin = qa.g + b * nv;
    const double c0 = qa.c0[b];
    const bool shift = a.shift != 0;
    QpState o;
    const int nq = (nv + 63) >> 6;
    if (w_in_lds) {                     // Nv <= 95: one or two rows per lane
        if (nq == 1) o = qp_solve<1, NU, true>(qsh, qa.W, nv, lane, rec, U, yio, gin, c0, shift, s, zs, z0s);
        else o = qp_solve<2, NU, true>(qsh, qa.W, nv, lane, rec, U, yio, gin, c0, shift, s, zs, z0s);
    } else if (nq <= 2) o = qp_solve<2, NU, false>(qsh, qa.W, nv, lane, rec, U, yio, gin, c0, shift, s, zs, z0s);
    else if (nq == 3) o = qp_solve<3, NU, false>(qsh, qa.W, nv, lane, rec, U, yio, gin, c0, shift, s, zs, z0s);
    else if (nq == 4) o = qp_solve<4, NU, false>(qsh, qa.W, nv, lane, rec, U, yio, gin, c0, shift, s, zs, z0s);
    else o = qp_solve<QP_MAX_ROWS, NU, false>(qsh, qa.W, nv, lane, rec, U, yio, gin, c0, shift, s, zs, z0s);

    const int64_t hold = rec->hold;
    if (a.u_apply) {                    // the first knot of z; of a problem that was not solved: the clamped first knot (z0)
        const double* first = o.bad ? z0s : zs;
        double* ua = a.u_apply + b * hold * NU;
        for (int64_t i = lane; i < hold * NU; i += 64) ua[i] = first[i % NU];
    }
    double* pr = qa.f.pred ? qa.f.pred + b * (H + 1) * N : nullptr;
    if (o.bad) {
        const double inf = __builtin_huge_val();
        if (pr)
            for (int64_t i = lane; i < (H + 1) * N; i += 64) pr[i] = __builtin_nan("");
        if (a.info && lane == 0) {
            double* info = a.info + b * 6;
            info[0] = info[1] = info[2] = info[3] = inf;
            info[4] = info[5] = 0.0;
        }
        return;
    }
    double x[N];
#pragma unroll
    for (int i = 0; i < N; ++i) x[i] = a.x[b * N + i];
    const double dt = a.dt;
    const double* refb = a.ref + (b * a.ref_total + a.ref_row0) * N;
    const int64_t rstep = a.ref_total > 1 ? N : 0;
    const double* Fb = qa.f.F + b * (H + 1) * N;
    double J = 0.0, J0 = 0.0;
    for (int64_t t = lane; t <= H; t += 64) {
        const bool last = t == H;
        double xa[N], xb[N], r[N];
#pragma unroll
        for (int i = 0; i < N; ++i) xa[i] = xb[i] = Fb[t * N + i];
        const int64_t nk = (t + hold - 1) / hold;             // the knots with m hold < t
        const int64_t nm = nk < M ? nk : M;
        const double* __restrict__ gt = qa.f.Gc + t * M * (N * NU);
        for (int64_t m = 0; m < nm; ++m) {
#pragma unroll
            for (int j = 0; j < NU; ++j) {
                const double va = zs[m * NU + j], vb = z0s[m * NU + j];
#pragma unroll
                for (int i = 0; i < N; ++i) {
                    const double gg = gt[m * (N * NU) + i * NU + j];
                    xa[i] = fma(gg, va, xa[i]);
                    xb[i] = fma(gg, vb, xb[i]);
                }
            }
        }
        if (pr) {
#pragma unroll
            for (int i = 0; i < N; ++i) pr[t * N + i] = xa[i];
        }
#pragma unroll
        for (int i = 0; i < N; ++i) r[i] = refb[t * rstep + i];
        adjust_reference<N>(x, r);
        double qa_ = 0.0, qb_ = 0.0;
#pragma unroll
        for (int i = 0; i < N; ++i) {
            const double qi = last ? rec->qf[i] : rec->q[i];
            const double ea = r[i] - xa[i], eb = r[i] - xb[i];
            qa_ = fma(qi * ea, ea, qa_);
            qb_ = fma(qi * eb, eb, qb_);
        }
        if (last) {
            J += qa_;
            J0 += qb_;
        } else {
            const int64_t m = t / hold;
            double ua = 0.0, ub = 0.0;
#pragma unroll
            for (int j = 0; j < NU; ++j) {
                const double va = zs[m * NU + j], vb = z0s[m * NU + j], rj = rec->r[j];
                ua = fma(rj * va, va, ua);
                ub = fma(rj * vb, vb, ub);
            }
            J = fma(dt, qa_ + ua, J);
            J0 = fma(dt, qb_ + ub, J0);
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        J += __shfl_xor(J, off);
        J0 += __shfl_xor(J0, off);
    }
    if (a.info && lane == 0) {
        double* info = a.info + b * 6;
        info[0] = J;
        info[1] = J0;
        info[2] = o.rp;
        info[3] = o.rd;
        info[4] = (double)o.it;
        info[5] = (double)o.nbound;
    }
}

// ---------------------------------------------------------------------------------------
// launch
// ---------------------------------------------------------------------------------------
// The dynamic LDS of a solve block: the slices of its four waves (s, z, z0: 3 Nv doubles each) and, while two such blocks fit the
// 160 KB of a CU together, W itself: Nv^2 + 12 Nv <= 10 240, that is Nv <= 95
size_t koopman_qp_block(int64_t nv, bool* w_in_lds) {
    const size_t slices = (size_t)KOOPMAN_QP_WAVES * 3 * nv * sizeof(double);
    const size_t with_w = (size_t)nv * nv * sizeof(double) + slices;
    const bool w = 2 * with_w <= 160 * 1024;
    if (w_in_lds) *w_in_lds = w;
    return w ? with_w : slices;
}

template <int N, int NU>
static hipError_t launch_qp(hipStream_t st, int64_t B, const KoopmanQpArgs& a) {
    const int64_t nv = a.f.m.M * NU;
    hipLaunchKernelGGL((koopman_qp_grad_kernel<N, NU>), dim3((unsigned)B), dim3((unsigned)((nv + 63) / 64 * 64)), 0, st, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    bool w;
    const size_t lds = koopman_qp_block(nv, &w);
    if (lds > 48 * 1024) {              // beyond the default limit of a launch: raised once per device and instantiation, not per tick
        static std::atomic<int> raised[QP_MAX_DEVICES];
        int dev = 0;
        e = hipGetDevice(&dev);
        if (e != hipSuccess) return e;
        const bool known = dev >= 0 && dev < QP_MAX_DEVICES;
        if (!known || raised[dev].load(std::memory_order_relaxed) < (int)lds) {
            e = hipFuncSetAttribute(reinterpret_cast<const void*>(&koopman_qp_solve_kernel<N, NU>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
            if (e != hipSuccess) return e;
            if (known) raised[dev].store((int)lds, std::memory_order_relaxed);
        }
    }
    hipLaunchKernelGGL((koopman_qp_solve_kernel<N, NU>), dim3((unsigned)((B + KOOPMAN_QP_WAVES - 1) / KOOPMAN_QP_WAVES)), dim3(64 * KOOPMAN_QP_WAVES),
                       lds, st, a, B, w ? 1 : 0);
    return hipGetLastError();
}

hipError_t launch_koopman_qp_step(hipStream_t st, int64_t B, const KoopmanQpArgs& a) {
    if (B <= 0) return hipSuccess;
    const KoopmanMppiArgs& f = a.f;
    if (B > 65535 || f.m.H < 1 || f.m.M < 1 || f.m.M * f.r > KOOPMAN_MPPI_MAX_MNU || (f.n != 12 && f.n != 13) || (f.r != 6 && f.r != 8))
        return hipErrorInvalidValue;
    hipError_t e = launch_koopman_free(st, B, f);
    if (e != hipSuccess) return e;
    if (f.n == 12) return f.r == 8 ? launch_qp<12, 8>(st, B, a) : launch_qp<12, 6>(st, B, a);
    return f.r == 8 ? launch_qp<13, 8>(st, B, a) : launch_qp<13, 6>(st, B, a);
}

}  // namespace brov
