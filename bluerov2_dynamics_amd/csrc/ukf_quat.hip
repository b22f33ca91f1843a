// ukf_quat.hip -- unscented Kalman filter on the quaternion model (MODEL_WRENCH_QUAT): candidate j filters B noisy recordings of T
// rows under params[j] (include/brov2.h: brov_ukf_filter_quat, which is the specification of the law).
//
// The multiplicative filter: the mean is a 13-component state whose attitude is a unit quaternion, the covariance, q and r live in
// the 12-component error state (dp, g, dnu) with g twice the Gibbs vector of a body-frame rotation.  That leaves the structure of
// ukf_filter_kernel (ukf.hip) as it is -- 25 sigma points, a 12 x 12 image with stride-13 rows in the wave's own LDS, 78 triangle
// entries on 64 lanes, one wave per (candidate, recording), UKF_WAVES per block, candidate = blockIdx.y, ukf_wave_sync between the
// phases and no workgroup barrier after the quadrant table -- and its phases: the scalar update (ukf_update<false>, on the correction
// d instead of the mean and without a wrap), the Cholesky, the mean deviation, the covariance sums and the closing outputs are the
// functions of brov2_ukf.h that the Euler filters call.  What is this kernel's own is where it touches the manifold:
//   innovation  z = y [-] x, formed once per row by every lane (redundantly: a few dozen FMAs and three divisions from the image);
//               the scalar updates then work on the correction d in the error state, and one x = x [+] d closes the row;
//   sigma       lane i builds chi_i = x [+] (+-c L[:, i-1]) and takes the step of rollout_pop_kernel for the quaternion model;
//   moments     lane i forms d_i = chi_i' [-] chi_0'; the mean deviation m is summed as in the Euler filter and x = chi_0' [+] m.
// Lanes 25..63 repeat point 0, so all 64 lanes stay active through every cross-lane read, and a wave leaves only as a whole.
#include "brov2_device.h"
#include "brov2_fast.h"
#include "brov2_kernels.h"
#include "brov2_rows.h"
#include "brov2_ukf.h"

namespace brov {

// q (x) dq(g) with dq(g) = (1, g / 2) / sqrt(1 + |g|^2 / 4): the attitude part of x [+] delta.  No branch; negating q negates the
// result bit for bit.
__device__ __forceinline__ void uq_plus(const double q[4], double gx, double gy, double gz, double out[4]) {
    const double hx = 0.5 * gx, hy = 0.5 * gy, hz = 0.5 * gz;
    const double inv = 1.0 / sqrt(fma(hz, hz, fma(hy, hy, fma(hx, hx, 1.0))));
    out[0] = fma(-q[3], hz, fma(-q[2], hy, fma(-q[1], hx, q[0]))) * inv;
    out[1] = fma(-q[3], hy, fma(q[2], hz, fma(q[0], hx, q[1]))) * inv;
    out[2] = fma(-q[1], hz, fma(q[3], hx, fma(q[0], hy, q[2]))) * inv;
    out[3] = fma(-q[2], hx, fma(q[1], hy, fma(q[0], hz, q[3]))) * inv;
}
// 2 e_v / e_w with e = conj(b) (x) a: the attitude part of a [-] b.  Invariant to the sign and the norm of either quaternion; not
// finite at half a turn (e_w = 0) or for a zero quaternion.
__device__ __forceinline__ void uq_minus(const double a[4], const double b[4], double g[3]) {
    const double ew = fma(b[3], a[3], fma(b[2], a[2], fma(b[1], a[1], b[0] * a[0])));
    const double ex = fma(b[3], a[2], fma(-b[2], a[3], fma(-b[1], a[0], b[0] * a[1])));
    const double ey = fma(-b[3], a[1], fma(-b[2], a[0], fma(b[1], a[3], b[0] * a[2])));
    const double ez = fma(-b[3], a[0], fma(b[2], a[1], fma(-b[1], a[2], b[0] * a[3])));
    g[0] = (ex + ex) / ew;
    g[1] = (ey + ey) / ew;
    g[2] = (ez + ez) / ew;
}
// x [+] delta on the whole state, every lane for itself: x [13] and delta [12] are in the image
__device__ __forceinline__ void uq_state_plus(const double* x, const double* dl, double out[13]) {
    const double q[4] = {x[3], x[4], x[5], x[6]};
#pragma unroll
    for (int r = 0; r < 3; ++r) out[r] = x[r] + dl[r];
    uq_plus(q, dl[3], dl[4], dl[5], out + 3);
#pragma unroll
    for (int r = 6; r < 12; ++r) out[r + 1] = x[r + 1] + dl[r];
}

template <int INTEG>
__global__ void __launch_bounds__(64 * UKF_WAVES) ukf_quat_filter_kernel(const UkfArgs a) {
    constexpr int MODEL = MODEL_WRENCH_QUAT;
    constexpr int NU = Dims<MODEL>::NU;
    static_assert(Dims<MODEL>::NX == 13, "the state is p[3], q[4], nu[6]");
    __shared__ double2 qt[4];
    __shared__ UkfQuatLds lds[UKF_WAVES];
    init_quadrant_table(qt);
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t B = a.B, T = a.T;
    const int64_t b = (int64_t)blockIdx.x * UKF_WAVES + wave;
    if (b >= B) return;                                       // a whole wave: no workgroup barrier follows
    UkfQuatLds& S = lds[wave];
    const int64_t row = (int64_t)blockIdx.y * B + b;          // recording b of candidate blockIdx.y in the outputs
    const CFP p = as_constant(a.fp + blockIdx.y);
    const CUK f = as_constant_uk(a.rec + (a.rec_per_candidate ? blockIdx.y : 0));
    HotConsts h;
    load_hot(p, h);
    const double dt = a.dt;
    const double NaN = __builtin_nan(""), INF = __builtin_inf();
    const UkfOwn own = ukf_own(lane);                         // the entries of P this lane owns
    const int lr = own.lr;                                    // its row in the error state
    int col;                                                  // its sigma point: x [+] sc L[:, col]
    double sc;
    const double cw = f->c;
    ukf_point(lane, cw, col, sc);
    const int lx = lane < 13 ? lane : 12;                     // its component of the state (lanes >= 13 repeat component 12)

    LagZ lz;                                                  // (the wrench model has no lag: step_fast never looks at these)
    double Xl[8][3];
    double p0 = a.P0[b * 144 + own.a0 * 12 + own.b0], p1 = a.P0[b * 144 + own.a1 * 12 + own.b1];
    ukf_put_P(S, own, p0, p1);
    if (lane < 13) S.x[lane] = a.x0[b * 13 + lane];
    ukf_wave_sync();

    const double* up = a.U + b * T * NU;
    const double* yp = a.Y + b * T * 13;
    double* xfp = a.xf ? a.xf + row * T * 13 + lx : nullptr;
    double* psp = a.pstd ? a.pstd + row * T * 12 + lr : nullptr;
    double* inp = a.innov ? a.innov + row * T * 12 + lr : nullptr;
    double ell = 0.0, nupd = 0.0, minpiv = INF;
    int64_t t = 0, failed = -1, nan_from = T;
    for (; t < T; ++t) {
        // ---- 1. update with row t -------------------------------------------------------------------------------------------
        double y[13], z[12];
        load_row<13>(yp + t * 13, y);
        bool bad = false;
        {
            // z = y [-] x from x as the row found it; every lane forms all of it
            double xq[4], yq[4], g[3];
#pragma unroll
            for (int k = 0; k < 4; ++k) { xq[k] = S.x[3 + k]; yq[k] = y[3 + k]; }
            uq_minus(yq, xq, g);
            const bool att = yq[0] == yq[0] && yq[1] == yq[1] && yq[2] == yq[2] && yq[3] == yq[3];
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                z[i] = y[i] - S.x[i];
                z[3 + i] = att ? g[i] : NaN;
                if (att && !(fabs(g[i]) < INF)) bad = true;
            }
#pragma unroll
            for (int i = 6; i < 12; ++i) z[i] = y[i + 1] - S.x[i + 1];
            if (lane < 12) S.d[lane] = 0.0;
            bad = __ballot(bad) != 0;                                  // (the lanes agree: this makes the flag a scalar)
            ukf_wave_sync();                                           // d written
        }
        if (bad) { failed = t; nan_from = t; break; }                  // q_y = 0 or half a turn away: before any update of the row
        double inn = NaN;
#pragma unroll
        for (int i = 0; i < 12; ++i) ukf_update<false>(S, S.d, f, i, ukf_uniform(z[i]), own, p0, p1, lane, ell, nupd, inn, bad);
        if (bad) { failed = t; nan_from = t; break; }
        {
            // x = x [+] d: one reset per row.  Every lane forms it; lane 0 stores its copy, as it stores c0 below
            double xn[13];
            uq_state_plus(S.x, S.d, xn);
            ukf_wave_sync();                                           // every read of x done
            if (lane == 0) {
#pragma unroll
                for (int r = 0; r < 13; ++r) S.x[r] = xn[r];
            }
            ukf_wave_sync();                                           // x written
            if (lane < 13 && xfp) xfp[t * 13] = S.x[lane];
        }
        if (lane < 12) {
            if (psp) psp[t * 12] = sqrt(S.P[lane][lane]);
            if (inp) inp[t * 12] = inn;
        }
        // ---- 2. predict with U[t] -------------------------------------------------------------------------------------------
        double Lr[12];
#pragma unroll
        for (int k = 0; k < 12; ++k) Lr[k] = S.P[lr][k];
#pragma unroll
        for (int j = 0; j < 12; ++j) ukf_cholesky_col(S, Lr, j, lane, lr, bad, minpiv);
        if (bad) { failed = t; nan_from = t + 1; break; }
        double x[13], u[NU];
        {
            double dl[12];
#pragma unroll
            for (int r = 0; r < 12; ++r) dl[r] = sc * S.L[r][col];
            uq_state_plus(S.x, dl, x);
        }
        load_row<NU>(up + t * NU, u);
        step_fast<MODEL, INTEG, 0, false, true>(h, p, dt, x, u, lz, Xl, qt);
        if (lane == 0) {
#pragma unroll
            for (int r = 0; r < 13; ++r) S.c0[r] = x[r];
        }
        ukf_wave_sync();                                               // c0 written
        {
            // d_i = chi_i' [-] chi_0'
            double c0q[4], g[3];
#pragma unroll
            for (int k = 0; k < 4; ++k) c0q[k] = S.c0[3 + k];
            uq_minus(x + 3, c0q, g);
            if (lane < UKF_NS) {
#pragma unroll
                for (int r = 0; r < 3; ++r) {
                    S.D[lane][r] = x[r] - S.c0[r];
                    S.D[lane][3 + r] = g[r];
                }
#pragma unroll
                for (int r = 6; r < 12; ++r) S.D[lane][r] = x[r + 1] - S.c0[r + 1];
            }
        }
        ukf_wave_sync();                                               // D written
        const double wi = f->wi;
        if (lane < 12) S.m[lane] = ukf_mean_dev(S, wi, lane);
        ukf_wave_sync();                                               // m written
        bool finite = true;
        {
            // x = chi_0' [+] m
            double xn[13];
            uq_state_plus(S.c0, S.m, xn);
#pragma unroll
            for (int r = 0; r < 12; ++r) finite = finite && fabs(S.m[r]) < INF;
#pragma unroll
            for (int r = 0; r < 13; ++r) finite = finite && fabs(xn[r]) < INF;
            if (lane == 0) {
#pragma unroll
                for (int r = 0; r < 13; ++r) S.x[r] = xn[r];
            }
        }
        const bool allfinite = __ballot(!finite) == 0;
        ukf_wave_sync();                                               // x written
        if (!allfinite) { failed = t; nan_from = t + 1; break; }
        ukf_cov(S, f, wi, own, p0, p1);
        ukf_wave_sync();                                               // P written
    }
    // ---- outputs -------------------------------------------------------------------------------------------------------------
    const bool ok = failed < 0;
    if (!ok) ukf_nan_rows(xfp, 13, psp, inp, lane, nan_from, T);
    if (a.xT && lane < 13) a.xT[row * 13 + lane] = ok ? S.x[lane] : NaN;
    ukf_put_tail(S, a.PT, a.info, row, lane, ell, nupd, failed, minpiv);
}

// ---------------------------------------------------------------------------------------
// launch: grid (blocks of UKF_WAVES recordings, P).  Of UkfArgs the fields lag, tape, nrows and Bs are not read; x0, Y, xf and xT
// are 13 wide.
// ---------------------------------------------------------------------------------------
hipError_t launch_ukf_filter_quat(hipStream_t st, int integ, int P, const UkfArgs& a) {
    if (a.B <= 0 || P <= 0) return hipSuccess;
    if (integ == INTEG_EULER) return ukf_launch(ukf_quat_filter_kernel<INTEG_EULER>, st, P, a);
    return ukf_launch(ukf_quat_filter_kernel<INTEG_RK4>, st, P, a);
}

}  // namespace brov
