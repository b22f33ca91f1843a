// brov2_ukf.h -- what the unscented Kalman filter kernels share: the wave's LDS image, the cross-lane helpers and the one definition
// of every phase that more than one of them runs.  The kernels are ukf_filter_kernel and ukf_rts_kernel (ukf.hip, whose head comment
// describes the layout and the synchronisation), ukf_feedback_kernel (ukf_feedback.hip), and ukf_quat_filter_kernel and
// ukf_quat_rts_kernel (ukf_quat.hip); they keep their time loop, the order of the phases, the ukf_wave_sync() between phases and the
// failure bookkeeping.  Every function here is inlined, and a template on the image type where the images differ (UkfLds, UkfQuatLds
// and the smoothers' UkfRtsLds and UkfQuatRtsLds all have L and P; the first two share D, m and k).  The tape's record layout, which
// the tape filters write and the two backward kernels read, is UkfTapeRec<NX> of brov2_kernels.h.  A floating-point expression here
// is part of the filters' law -- operands, association, explicit fma, index order of a sum: the filter inside the closed loop is the
// plain filter bit for bit because both call this text.  How arguments are passed is fitted to the register allocator (values that a phase changes by reference, no array
// copies, the column loop of the Cholesky in the caller): profiles/ukf_shared_phases.md has the resource table to check a change against.
#pragma once
#include "brov2_device.h"
#include "brov2_kernels.h"
#include "brov2_rows.h"

namespace brov {

constexpr int UKF_WAVES = 4;            // recordings (waves) per block
constexpr int UKF_LD = 13;              // row stride of the LDS matrices, in doubles
constexpr int UKF_NS = 25;              // sigma points of the 12-state model

struct UkfLds {
    double D[UKF_NS][UKF_LD];           // deviations of the propagated points from point 0 (attitude wrapped)
    double P[12][UKF_LD];               // covariance, both triangles
    double L[12][UKF_LD];               // its lower Cholesky factor
    double x[12], m[12], c0[12], k[12]; // mean, mean deviation, propagated point 0, gain column
};

// the image of the quaternion-model filter (ukf_quat.hip): D, P, L, m and k live in the 12-component error state, the mean and the
// propagated point 0 in the 13-component state; d is the error-state correction that the updates of a row add up
struct UkfQuatLds {
    double D[UKF_NS][UKF_LD];
    double P[12][UKF_LD];
    double L[12][UKF_LD];
    double x[13], c0[13];
    double d[12], m[12], k[12];
};

typedef const UkfRec __attribute__((address_space(4)))* CUK;
__device__ __forceinline__ CUK as_constant_uk(const UkfRec* g) { return (CUK)(unsigned long long)g; }

// LDS written by some lanes of a wave is read by others: order the two
__device__ __forceinline__ void ukf_wave_sync() {
    __builtin_amdgcn_wave_barrier();
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
}
// keeps the image reads of the EM term (ukf_em_term) from mixing with those of the phases around it, which would cost more registers
// than a lane has
__device__ __forceinline__ void ukf_fence() { asm volatile("" ::: "memory"); }
// the value of lane l (a constant) / of the first lane, as a wave-uniform scalar
__device__ __forceinline__ double ukf_lane(double v, int l) {
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), l), __builtin_amdgcn_readlane(__double2loint(v), l));
}
__device__ __forceinline__ double ukf_uniform(double v) {
    return __hiloint2double(__builtin_amdgcn_readfirstlane(__double2hiint(v)), __builtin_amdgcn_readfirstlane(__double2loint(v)));
}
__device__ __forceinline__ double ukf_wrap(double d) {      // the rule of the feedback law (brov2_error.h)
    return fma(-6.28318530717958647692e+00, rint(d * 1.59154943091895335769e-01), d);
}

// ---- ownership: 78 entries of the lower triangle on 64 lanes ---------------------------------------------------------------------
// entry e of the lower triangle, row by row: e = a (a + 1) / 2 + b, b <= a
__device__ __forceinline__ void ukf_entry(int e, int& a, int& b) {
    a = 0;
    while ((a + 1) * (a + 2) / 2 <= e) ++a;
    b = e - a * (a + 1) / 2;
}
// what a lane owns: entry (a0, b0), lanes 0..13 entry (a1, b1) as well (`two`; the others repeat their first), and row lr of the
// per-row phases (lanes >= 12 repeat row 11)
struct UkfOwn {
    int a0, b0, a1, b1, lr;
    bool two;
};
__device__ __forceinline__ UkfOwn ukf_own(int lane) {
    UkfOwn o;
    ukf_entry(lane, o.a0, o.b0);
    o.two = lane + 64 < 78;
    ukf_entry(o.two ? lane + 64 : lane, o.a1, o.b1);
    o.lr = lane < 12 ? lane : 11;
    return o;
}
// an entry goes to both triangles, so the image stays bit-symmetric
__device__ __forceinline__ void ukf_put(double (&M)[12][UKF_LD], int a, int b, double v) {
    M[a][b] = v;
    M[b][a] = v;
}
template <typename Lds>
__device__ __forceinline__ void ukf_put_P(Lds& S, const UkfOwn& o, double p0, double p1) {
    ukf_put(S.P, o.a0, o.b0, p0);
    if (o.two) ukf_put(S.P, o.a1, o.b1, p1);
}

// ---- the sigma point of a lane: mean (+) sc L[:, col]; lanes 0 and 25..63 are point 0 ----------------------------------------------
__device__ __forceinline__ void ukf_point(int lane, double c, int& col, double& sc) {
    const bool point = lane >= 1 && lane < UKF_NS;
    col = point ? (lane - 1) % 12 : 0;
    sc = point ? (lane <= 12 ? c : -c) : 0.0;
}

// ---- scalar update i with the measured value yi (wave-uniform) --------------------------------------------------------------------
// xc is the 12-vector of the image that the gain moves (the mean, or the quaternion filter's correction d); WRAP wraps the innovation
// of components 3..5.  Skipped when the row has failed, yi is NaN or r[i] is infinite; s <= 0 or not finite sets `bad`.  Every branch
// is wave-uniform.  Two ukf_wave_sync() inside: after k and xc are written (and column i of P read), after P is written.
template <bool WRAP, typename Lds>
__device__ __forceinline__ void ukf_update(Lds& S, double (&xc)[12], CUK f, int i, double yi, const UkfOwn& o, double& p0, double& p1,
                                           int lane, double& ell, double& nupd, double& inn, bool& bad) {
    const double INF = __builtin_inf();
    const double ri = f->r[i];
    if (bad || yi != yi || ri == INF) return;
    const double s = ukf_uniform(S.P[i][i]) + ri;
    if (!(s > 0.0) || s == INF) { bad = true; return; }
    double v = yi - ukf_uniform(xc[i]);
    if (WRAP && i >= 3 && i < 6) v = ukf_wrap(v);
    if (lane < 12) {
        const double k = S.P[lane][i] / s;
        S.k[lane] = k;
        xc[lane] += k * v;
    }
    ell -= 0.5 * (log(6.28318530717958647692e+00 * s) + v * v / s);
    nupd += 1.0;
    if (lane == i) inn = v / sqrt(s);
    ukf_wave_sync();                                           // k, xc written; every read of column i of P done
    p0 -= S.k[o.a0] * S.k[o.b0] * s;
    ukf_put(S.P, o.a0, o.b0, p0);
    if (o.two) {
        p1 -= S.k[o.a1] * S.k[o.b1] * s;
        ukf_put(S.P, o.a1, o.b1, p1);
    }
    ukf_wave_sync();                                           // P written
}

// ---- Cholesky, one lane per row: column j, s_i = A[i][j] - sum_k L[i][k] L[j][k] ----------------------------------------------------
// The caller has loaded row lr of the matrix into Lr and calls this for j = 0 .. 11 in an unrolled loop of its own (with the loop in
// here the thruster-Euler tape filter needs 258 registers instead of 251 and loses its second wave per SIMD).  Lane j's own s is the
// pivot argument and travels through v_readlane; row j, which the other lanes need for column j, is in the image since its last entry
// was written at column j - 1.  A pivot that is not positive and finite sets `bad` (the factor goes on with d = 1, the caller
// leaves); minpiv takes the smallest sqrt(pivot).
template <typename Lds>
__device__ __forceinline__ void ukf_cholesky_col(Lds& S, double (&Lr)[12], int j, int lane, int lr, bool& bad, double& minpiv) {
    const double INF = __builtin_inf();
    double s = Lr[j];
#pragma unroll
    for (int k = 0; k < j; ++k) s = fma(-Lr[k], S.L[j][k], s);
    const double piv = ukf_lane(s, j);
    double d = 1.0;
    if (!bad) {
        if (!(piv > 0.0) || piv == INF) bad = true;
        else { d = sqrt(piv); minpiv = fmin(minpiv, d); }
    }
    Lr[j] = lr == j ? d : (lr > j ? s / d : 0.0);
    if (lane < 12) S.L[lane][j] = Lr[j];
    ukf_wave_sync();                                               // column j of L written
}

// ---- moments of the 25 deviations in D, every sum in index order -----------------------------------------------------------------
// component `lane` of the mean deviation (point 0 is the origin: its deviation is zero)
template <typename Lds>
__device__ __forceinline__ double ukf_mean_dev(const Lds& S, double wi, int lane) {
    double m = 0.0;
#pragma unroll
    for (int i = 1; i < UKF_NS; ++i) m = fma(wi, S.D[i][lane], m);
    return m;
}
// entry (a, b) of the predicted covariance, from D and m
template <typename Lds>
__device__ __forceinline__ double ukf_cov_entry(const Lds& S, CUK f, double wi, int a, int b) {
    const double ma = S.m[a], mb = S.m[b];
    double acc = f->wc0 * (ma * mb);
#pragma unroll
    for (int i = 1; i < UKF_NS; ++i) acc = fma(wi, (S.D[i][a] - ma) * (S.D[i][b] - mb), acc);
    if (a == b) acc += f->q[a];
    return acc;
}
// the entries this lane owns, into its registers and both triangles of P
template <typename Lds>
__device__ __forceinline__ void ukf_cov(Lds& S, CUK f, double wi, const UkfOwn& o, double& p0, double& p1) {
    p0 = ukf_cov_entry(S, f, wi, o.a0, o.b0);
    ukf_put(S.P, o.a0, o.b0, p0);
    if (o.two) {
        p1 = ukf_cov_entry(S, f, wi, o.a1, o.b1);
        ukf_put(S.P, o.a1, o.b1, p1);
    }
}

// ---- v <- (L L^T)^-1 v: forward through L, backward through L^T, L read wave-uniformly from the image --------------------------------
template <typename Lds>
__device__ __forceinline__ void ukf_solve_llt(const Lds& S, double (&v)[12]) {
#pragma unroll
    for (int j = 0; j < 12; ++j) {
        double s = v[j];
#pragma unroll
        for (int k = 0; k < j; ++k) s = fma(-S.L[j][k], v[k], s);
        v[j] = s / S.L[j][j];
    }
#pragma unroll
    for (int j = 11; j >= 0; --j) {
        double s = v[j];
#pragma unroll
        for (int k = j + 1; k < 12; ++k) s = fma(-S.L[k][j], v[k], s);
        v[j] = s / S.L[j][j];
    }
}

// ---- closing outputs ---------------------------------------------------------------------------------------------------------------
// rows [from, T) of xf (nx wide), pstd and innov are NaN; each pointer is at this lane's component of row 0, or null
__device__ __forceinline__ void ukf_nan_rows(double* xfp, int nx, double* psp, double* inp, int lane, int64_t from, int64_t T) {
    for (int64_t s = from; s < T; ++s) {
        if (xfp && lane < nx) xfp[s * nx] = __builtin_nan("");
        if (psp && lane < 12) psp[s * 12] = __builtin_nan("");
        if (inp && lane < 12) inp[s * 12] = __builtin_nan("");
    }
}
// PT (the image's P, or NaN) and info = (ell or -inf, nupd, failed, minpiv) of output row `row`
template <typename Lds>
__device__ __forceinline__ void ukf_put_tail(const Lds& S, double* PT, double* info, int64_t row, int lane, double ell, double nupd,
                                             int64_t failed, double minpiv) {
    const bool ok = failed < 0;
    if (PT) {
        for (int e = lane; e < 144; e += 64) PT[row * 144 + e] = ok ? S.P[e / 12][e % 12] : __builtin_nan("");
    }
    if (info && lane == 0) {
        const double v[4] = {ok ? ell : -__builtin_inf(), nupd, (double)failed, minpiv};
        store_row<4>(info + row * 4, v);
    }
}

// ---- launch: one wave per problem, UKF_WAVES problems per block, candidate = blockIdx.y ------------------------------------------------
template <typename Kernel, typename Args>
static inline hipError_t ukf_launch(Kernel kernel, hipStream_t st, int P, const Args& a) {
    const dim3 grid((unsigned)((a.B + UKF_WAVES - 1) / UKF_WAVES), (unsigned)P);
    hipLaunchKernelGGL(kernel, grid, dim3(64 * UKF_WAVES), 0, st, a);
    return hipGetLastError();
}

}  // namespace brov
