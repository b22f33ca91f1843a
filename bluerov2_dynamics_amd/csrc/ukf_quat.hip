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
//
// The smoother over it (include/brov2.h: brov_ukf_filter_tape_quat_dev, brov_ukf_rts_quat_dev): the filter's tape variant, which is
// ukf_filter_kernel's tape on this kernel's D with the 13-wide predicted mean (UKF_TAPE_QUAT doubles a record), and the backward
// kernel ukf_quat_rts_kernel further down, ukf_rts_kernel with its manifold touches changed.
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

// TAPE: step t also records what the backward pass (ukf_quat_rts_kernel below) needs for the transition t -> t + 1.  Every tape store
// sits behind `if constexpr (TAPE)`, as in ukf_filter_kernel; the TAPE = false instantiations are the code they were before.
template <int INTEG, bool TAPE>
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
    // recording b of candidate blockIdx.y in the outputs; with a tape the outputs of a chunk lie among those of Bs recordings
    const int64_t row = (int64_t)blockIdx.y * (TAPE ? a.Bs : B) + b;
    double* tp = nullptr;                                     // this problem's tape records
    if constexpr (TAPE) tp = a.tape + ((int64_t)blockIdx.y * B + b) * T * UKF_TAPE_QUAT;
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
        if constexpr (TAPE) {                                          // Pf_t, after the row's reset: the entries this lane holds
            tp[t * UKF_TAPE_QUAT + lane] = p0;
            if (own.two) tp[t * UKF_TAPE_QUAT + 64 + lane] = p1;
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
        if constexpr (TAPE) {
            if (lane < 13) tp[t * UKF_TAPE_QUAT + UkfTapeRec<13>::XP + lane] = S.x[lane];        // xp_{t+1} = chi_0' [+] m
        }
        ukf_cov(S, f, wi, own, p0, p1);
        if constexpr (TAPE) {
            tp[t * UKF_TAPE_QUAT + UkfTapeRec<13>::PP + lane] = p0;                    // Pp_{t+1}
            if (own.two) tp[t * UKF_TAPE_QUAT + UkfTapeRec<13>::PP + 64 + lane] = p1;
            // C_{t+1}[ca][cb] = sum_j L[ca][j] (c W_i (d_{j+1} - d_{j+13})[cb]): chi_i [-] x = +-c L[:, i-1], and L and D are still
            // in the image
            const double g = cw * wi;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const int e = lane + 64 * k;
                if (e < 144) {
                    const int ca = e / 12, cb = e % 12;
                    double acc = 0.0;
#pragma unroll
                    for (int j = 0; j < 12; ++j) acc = fma(S.L[ca][j], g * (S.D[j + 1][cb] - S.D[j + 13][cb]), acc);
                    tp[t * UKF_TAPE_QUAT + UkfTapeRec<13>::C + e] = acc;
                }
            }
        }
        ukf_wave_sync();                                               // P written
    }
    // ---- outputs -------------------------------------------------------------------------------------------------------------
    const bool ok = failed < 0;
    if (!ok) ukf_nan_rows(xfp, 13, psp, inp, lane, nan_from, T);
    if constexpr (TAPE) {
        // of a transition that did not complete xp, Pp and C are NaN; Pf_t stays when the update of row t was complete
        if (!ok) {
            for (int64_t i = (nan_from > failed ? failed * UKF_TAPE_QUAT + UkfTapeRec<13>::XP : failed * UKF_TAPE_QUAT) + lane; i < T * UKF_TAPE_QUAT; i += 64)
                tp[i] = NaN;
        }
        if (lane == 0) a.nrows[(int64_t)blockIdx.y * B + b] = (double)nan_from;
    }
    if (a.xT && lane < 13) a.xT[row * 13 + lane] = ok ? S.x[lane] : NaN;
    ukf_put_tail(S, a.PT, a.info, row, lane, ell, nupd, failed, minpiv);
}

// ---------------------------------------------------------------------------------------
// Backward (Rauch-Tung-Striebel) pass over the tape (include/brov2.h: brov_ukf_rts_quat_dev holds the law).  ukf_rts_kernel's
// decomposition (ukf.hip, whose comment describes it): one wave per (candidate, recording), UKF_WAVES per block, the time loop --
// downwards -- inside, ukf_wave_sync between phases and no workgroup barrier at all, the record fetched one transition ahead into 5
// registers per lane (313 <= 320) with Pf's entries landing on their owners, the filter's Cholesky of Pp with the column loop here,
// the gain row by ukf_solve_llt, M, G M and Ps as there, Ps in the owners' registers over the pass.  What is this kernel's own:
//   xs    a 13-vector in the image.  xf_t comes in with the record (lanes 0..12) and goes to the image; lanes 0..11 form G delta,
//         every lane forms xf_t [+] (G delta) and lane 0 stores it, as the filter stores its mean;
//   delta xs_{t+1} [-] xp_{t+1} through uq_minus, formed by every lane; a component that is not finite (half a turn, a zero
//         quaternion) fails the transition like a bad pivot: the test is a ballot, so the branch is wave-uniform.
// No covariance is transported between the tangent spaces at xf_t, xp_{t+1} and xs_{t+1}: the filter's first-order practice.
// ---------------------------------------------------------------------------------------
struct UkfQuatRtsLds {
    double rec[UKF_TAPE_QUAT];          // the tape record of the transition
    double L[12][UKF_LD];               // Cholesky factor of Pp
    double G[12][UKF_LD];               // the smoother gain
    double M[12][UKF_LD];               // Ps_{t+1} - Pp_{t+1}, both triangles
    double GM[12][UKF_LD];
    double P[12][UKF_LD];               // Ps of the row last finished, both triangles
    double xs[13], xf[13];              // xs of the row last finished; xf_t of the transition
    double dx[12], gd[12];              // delta; G delta
};

__global__ void __launch_bounds__(64 * UKF_WAVES) ukf_quat_rts_kernel(const UkfRtsArgs a) {
    __shared__ UkfQuatRtsLds lds[UKF_WAVES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t B = a.B, T = a.T;
    const int64_t b = (int64_t)blockIdx.x * UKF_WAVES + wave;
    if (b >= B) return;                                       // a whole wave: there is no workgroup barrier
    UkfQuatRtsLds& S = lds[wave];
    const int64_t loc = (int64_t)blockIdx.y * B + b;          // in the tape and nrows
    const int64_t row = (int64_t)blockIdx.y * a.Bs + b;       // in xf, the terminal pair and the outputs
    const double NaN = __builtin_nan(""), INF = __builtin_inf();
    const UkfOwn own = ukf_own(lane);
    const int a0 = own.a0, b0 = own.b0, a1 = own.a1, b1 = own.b1, lr = own.lr;
    const bool two = own.two;
    const int lx = lane < 13 ? lane : 12;                     // its component of the state (lanes >= 13 repeat component 12)
    const double nd = ukf_uniform(a.nrows[loc]);
    const int64_t n = nd >= 1.0 ? (nd < (double)T ? (int64_t)nd : T) : 0;
    const double* tp = a.tape + loc * T * UKF_TAPE_QUAT;
    const double* xfp = a.xf + row * T * 13 + lx;
    double* xsp = a.xs ? a.xs + row * T * 13 : nullptr;
    double* psp = a.pstd ? a.pstd + row * T * 12 : nullptr;
    double* Psp = a.Ps ? a.Ps + row * T * 144 : nullptr;
    // row s of the outputs: NaN, or (the image's xs, the image's P)
    auto put_nan = [&](int64_t s) {
        if (xsp && lane < 13) xsp[s * 13 + lane] = NaN;
        if (psp && lane < 12) psp[s * 12 + lane] = NaN;
        if (Psp) {
            for (int e = lane; e < 144; e += 64) Psp[s * 144 + e] = NaN;
        }
    };
    for (int64_t s = n; s < T; ++s) put_nan(s);
    if (n == 0) {
        if (a.Ps0) {
            for (int e = lane; e < 144; e += 64) a.Ps0[row * 144 + e] = NaN;
        }
        if (a.sinfo && lane == 0) {
            const double v[2] = {NaN, NaN};
            store_row<2>(a.sinfo + row * 2, v);
        }
        return;
    }
    // ---- start: the terminal pair of a later span, or the filter's last row ------------------------------------------------------
    const bool terminal = a.xsT != nullptr && n == T;
    double ps0, ps1;
    if (terminal) {
        if (lane < 13) S.xs[lane] = a.xsT[row * 13 + lane];
        ps0 = a.PsT[row * 144 + a0 * 12 + b0];
        ps1 = a.PsT[row * 144 + a1 * 12 + b1];
    } else {
        if (lane < 13) S.xs[lane] = xfp[(n - 1) * 13];
        ps0 = tp[(n - 1) * UKF_TAPE_QUAT + lane];
        ps1 = tp[(n - 1) * UKF_TAPE_QUAT + (two ? lane + 64 : lane)];
    }
    auto image_P = [&] {
        ukf_put_P(S, own, ps0, ps1);
        ukf_wave_sync();
    };
    auto put_row = [&](int64_t s) {
        if (xsp && lane < 13) xsp[s * 13 + lane] = S.xs[lane];
        if (psp && lane < 12) psp[s * 12 + lane] = sqrt(S.P[lane][lane]);
        if (Psp) {
            for (int e = lane; e < 144; e += 64) Psp[s * 144 + e] = S.P[e / 12][e % 12];
        }
    };
    image_P();                                                // (xs written as well)
    if (!terminal) put_row(n - 1);
    // ---- the transitions, last first ---------------------------------------------------------------------------------------------
    double r[5], xfv;
    auto fetch = [&](int64_t t) {
#pragma unroll
        for (int k = 0; k < 4; ++k) r[k] = tp[t * UKF_TAPE_QUAT + 64 * k + lane];
        r[4] = lane < UKF_TAPE_QUAT - 256 ? tp[t * UKF_TAPE_QUAT + 256 + lane] : 0.0;
        xfv = xfp[t * 13];
    };
    int64_t t = terminal ? n - 1 : n - 2, failed = -1;
    double minpiv = INF;
    if (t >= 0) fetch(t);
    for (; t >= 0; --t) {
#pragma unroll
        for (int k = 0; k < 4; ++k) S.rec[64 * k + lane] = r[k];
        if (lane < UKF_TAPE_QUAT - 256) S.rec[256 + lane] = r[4];
        if (lane < 13) S.xf[lane] = xfv;
        const double pf0 = r[0], pf1 = r[1];                  // Pf's entries lie on their owners
        if (t > 0) fetch(t - 1);
        ukf_wave_sync();                                      // rec, xf written
        // Cholesky of Pp, as in the filter
        double Lr[12];
#pragma unroll
        for (int k = 0; k < 12; ++k) Lr[k] = S.rec[UkfTapeRec<13>::PP + (k <= lr ? lr * (lr + 1) / 2 + k : k * (k + 1) / 2 + lr)];
        bool bad = false;
#pragma unroll
        for (int j = 0; j < 12; ++j) ukf_cholesky_col(S, Lr, j, lane, lr, bad, minpiv);
        if (bad) { failed = t; break; }
        // delta = xs_{t+1} [-] xp_{t+1}: every lane forms the attitude part, lane lr keeps component lr
        double dl;
        {
            double sq[4], pq[4], gq[3];
#pragma unroll
            for (int k = 0; k < 4; ++k) { sq[k] = S.xs[3 + k]; pq[k] = S.rec[UkfTapeRec<13>::XP + 3 + k]; }
            uq_minus(sq, pq, gq);
            const int c = lr < 3 ? lr : lr + 1;               // (of position and velocity) its component of the 13-wide state
            const double lin = S.xs[c] - S.rec[UkfTapeRec<13>::XP + c];
            dl = lr == 3 ? gq[0] : (lr == 4 ? gq[1] : (lr == 5 ? gq[2] : lin));
        }
        if (__ballot(!(fabs(dl) < INF)) != 0) { failed = t; break; }      // half a turn, a zero quaternion: like a bad pivot
        // row lr of G: w L^T = C[lr][:], then g L = w
        double g[12];
#pragma unroll
        for (int j = 0; j < 12; ++j) g[j] = S.rec[UkfTapeRec<13>::C + lr * 12 + j];
        ukf_solve_llt(S, g);
        if (lane < 12) {
#pragma unroll
            for (int k = 0; k < 12; ++k) S.G[lane][k] = g[k];
            S.dx[lane] = dl;
        }
        ukf_put(S.M, a0, b0, ps0 - S.rec[UkfTapeRec<13>::PP + lane]);
        if (two) ukf_put(S.M, a1, b1, ps1 - S.rec[UkfTapeRec<13>::PP + 64 + lane]);
        ukf_wave_sync();                                      // G, dx, M written; every read of xs done
        if (lane < 12) {
            double acc = 0.0;
#pragma unroll
            for (int k = 0; k < 12; ++k) acc = fma(g[k], S.dx[k], acc);
            S.gd[lane] = acc;
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const int e = lane + 64 * k;
            if (e < 144) {
                const int ga = e / 12, gb = e % 12;
                double acc = 0.0;
#pragma unroll
                for (int c = 0; c < 12; ++c) acc = fma(S.G[ga][c], S.M[c][gb], acc);
                S.GM[ga][gb] = acc;
            }
        }
        ukf_wave_sync();                                      // gd, GM written
        {
            // xs_t = xf_t [+] (G delta): every lane forms it; lane 0 stores its copy
            double xn[13];
            uq_state_plus(S.xf, S.gd, xn);
            if (lane == 0) {
#pragma unroll
                for (int q = 0; q < 13; ++q) S.xs[q] = xn[q];
            }
        }
        {
            double acc = 0.0;
#pragma unroll
            for (int c = 0; c < 12; ++c) acc = fma(S.GM[a0][c], S.G[b0][c], acc);
            ps0 = pf0 + acc;
            if (two) {
                double acc1 = 0.0;
#pragma unroll
                for (int c = 0; c < 12; ++c) acc1 = fma(S.GM[a1][c], S.G[b1][c], acc1);
                ps1 = pf1 + acc1;
            }
        }
        image_P();                                            // (xs written as well)
        put_row(t);
    }
    // ---- outputs -------------------------------------------------------------------------------------------------------------
    const bool ok = failed < 0;
    for (int64_t s = failed; s >= 0; --s) put_nan(s);
    if (a.Ps0) {
        for (int e = lane; e < 144; e += 64) a.Ps0[row * 144 + e] = ok ? S.P[e / 12][e % 12] : NaN;
    }
    if (a.sinfo && lane == 0) {
        const double v[2] = {(double)failed, minpiv};
        store_row<2>(a.sinfo + row * 2, v);
    }
}

// ---------------------------------------------------------------------------------------
// launch: grid (blocks of UKF_WAVES recordings, P).  Of UkfArgs the field lag is not read, and tape, nrows and Bs by the tape
// variant alone (tape != nullptr); x0, Y, xf and xT are 13 wide.  Of UkfRtsArgs the fields behind sinfo are not read.
// ---------------------------------------------------------------------------------------
hipError_t launch_ukf_filter_quat(hipStream_t st, int integ, int P, const UkfArgs& a) {
    if (a.B <= 0 || P <= 0) return hipSuccess;
    if (a.tape) {
        if (integ == INTEG_EULER) return ukf_launch(ukf_quat_filter_kernel<INTEG_EULER, true>, st, P, a);
        return ukf_launch(ukf_quat_filter_kernel<INTEG_RK4, true>, st, P, a);
    }
    if (integ == INTEG_EULER) return ukf_launch(ukf_quat_filter_kernel<INTEG_EULER, false>, st, P, a);
    return ukf_launch(ukf_quat_filter_kernel<INTEG_RK4, false>, st, P, a);
}

hipError_t launch_ukf_rts_quat(hipStream_t st, int P, const UkfRtsArgs& a) {
    if (a.B <= 0 || P <= 0) return hipSuccess;
    return ukf_launch(ukf_quat_rts_kernel, st, P, a);
}

}  // namespace brov
