// ukf.hip -- unscented Kalman filter on the Fossen model: candidate j filters B noisy recordings of T rows under params[j]
// (include/brov2.h: brov_ukf_filter, which is the specification of the law), and the unscented Rauch-Tung-Striebel smoother over it:
// the filter's tape variant and the backward kernel ukf_rts_kernel (further down; brov_ukf_filter_tape_dev, brov_ukf_rts_dev).
//
// One wave per (candidate, recording): candidate = blockIdx.y with the vehicle constants through as_constant(fp + blockIdx.y) as in
// rollout_feedback_kernel, UKF_WAVES recordings per block, the time loop inside the kernel.  The wave's (x, P), the Cholesky factor,
// the 25 propagated deviations and their mean live in the wave's own LDS image between the phases of a row:
//   update    12 scalar Kalman updates in order.  Lanes 0..11 form the gain column k = P[:, i] / s and update x; every lane owns one
//             entry of the lower triangle of P (lanes 0..13 a second one: 78 entries on 64 lanes), keeps it in a register over the
//             row and writes it to both triangles of the image, so the image stays bit-symmetric.
//   Cholesky  one lane per row, the rows in registers, column by column; the pivot row is read from the image, into which every lane
//             writes its entry of a column as soon as it has it, and the pivot itself travels through v_readlane.
//   sigma     lanes 0..24 build their point from x and a column of L, lanes 25..63 repeat point 0 (all 64 lanes stay active, so
//             the cross-lane reads never meet an inactive lane) and every lane takes the step of rollout_pop_kernel: the GENERIC
//             step_fast, and with TRACK the acceleration-space bank re-formed from the per-thruster state, which every lane carries
//             (the lag depends on the commands alone, so the 64 copies are equal and lane 0 stores its own).
//   moments   lanes 0..11 sum the mean of the deviations in index order, then every lane sums its entries of P over the 25 points
//             in index order.  No atomics: two calls give the same bits.
// Synchronisation: a wave is the only reader and writer of its image and never leaves its own program order, and the LDS serves a
// wave's accesses in issue order.  So wave_sync() -- a scheduling barrier for the compiler and a wait for the wave's outstanding
// LDS accesses -- is all that a phase needs before it reads what other lanes of the wave wrote; no workgroup barrier is used after
// the quadrant table is set up, which lets a wave leave (ragged block, or a filter that failed) without the others noticing.
// Rows of the image have a stride of 13 doubles: lanes that walk down a column (D[i][a] over i, L[r][col] over col, P[lane][i])
// then start on 26-dword steps, which are distinct even banks within a 32-lane half, so no phase piles onto one bank.
#include "brov2_device.h"
#include "brov2_fast.h"
#include "brov2_kernels.h"
#include "brov2_rows.h"
#include "brov2_ukf.h"

namespace brov {

// TAPE: step t also records what the backward pass (ukf_rts_kernel below) needs for the transition t -> t + 1.  Every tape store sits
// behind `if constexpr (TAPE)`; the TAPE = false instantiations are the code they were before the tape existed.
template <int MODEL, int INTEG, int LAGMODE, bool TRACK, bool TAPE>
__global__ void __launch_bounds__(64 * UKF_WAVES) ukf_filter_kernel(const UkfArgs a) {
    constexpr int NU = Dims<MODEL>::NU;
    static_assert(Dims<MODEL>::NX == 12, "the filter's state is the 12-state Euler model");
    __shared__ double2 qt[4];
    __shared__ UkfLds lds[UKF_WAVES];
    init_quadrant_table(qt);
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t B = a.B, T = a.T;
    const int64_t b = (int64_t)blockIdx.x * UKF_WAVES + wave;
    if (b >= B) return;                                       // a whole wave: no workgroup barrier follows
    UkfLds& S = lds[wave];
    int64_t row = (int64_t)blockIdx.y * B + b;                // recording b of candidate blockIdx.y in the outputs
    double* tp = nullptr;                                     // this problem's tape records
    if constexpr (TAPE) {
        tp = a.tape + row * T * UKF_TAPE;
        row = (int64_t)blockIdx.y * a.Bs + b;                 // the outputs of a chunk lie among those of Bs recordings
    }
    const CFP p = as_constant(a.fp + blockIdx.y);
    const CUK f = as_constant_uk(a.rec + (a.rec_per_candidate ? blockIdx.y : 0));
    HotConsts h;
    load_hot(p, h);
    const double dt = a.dt;
    const double NaN = __builtin_nan(""), INF = __builtin_inf();
    const UkfOwn own = ukf_own(lane);                         // the entries of P this lane owns
    const int lr = own.lr;                                    // its row in the per-row phases
    int col;                                                  // its sigma point: x + sc L[:, col]
    double sc;
    const double cw = f->c;
    ukf_point(lane, cw, col, sc);

    LagZ lz;
    double Xl[8][3];
    if constexpr (MODEL == MODEL_THRUSTER_EULER) {
        if constexpr (TRACK) load_row<24>(a.lag + row * 24, &Xl[0][0]);
        else lz.zero();
    }
    double p0 = a.P0[b * 144 + own.a0 * 12 + own.b0], p1 = a.P0[b * 144 + own.a1 * 12 + own.b1];
    ukf_put_P(S, own, p0, p1);
    if (lane < 12) S.x[lane] = a.x0[b * 12 + lane];
    ukf_wave_sync();

    const double* up = a.U + b * T * NU;
    const double* yp = a.Y + b * T * 12;
    double* xfp = a.xf ? a.xf + row * T * 12 + lr : nullptr;
    double* psp = a.pstd ? a.pstd + row * T * 12 + lr : nullptr;
    double* inp = a.innov ? a.innov + row * T * 12 + lr : nullptr;
    double ell = 0.0, nupd = 0.0, minpiv = INF;
    int64_t t = 0, failed = -1, nan_from = T;
    for (; t < T; ++t) {
        // ---- 1. update with row t -------------------------------------------------------------------------------------------
        double y[12];
        load_row<12>(yp + t * 12, y);
        double inn = NaN;
        bool bad = false;
#pragma unroll
        for (int i = 0; i < 12; ++i) ukf_update<true>(S, S.x, f, i, ukf_uniform(y[i]), own, p0, p1, lane, ell, nupd, inn, bad);
        if (bad) { failed = t; nan_from = t; break; }
        if constexpr (TAPE) {                                          // Pf_t: the entries this lane holds, 8-byte stores side by side
            tp[t * UKF_TAPE + lane] = p0;
            if (own.two) tp[t * UKF_TAPE + 64 + lane] = p1;
        }
        if (lane < 12) {
            if (xfp) xfp[t * 12] = S.x[lane];
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
        double x[12], u[NU];
#pragma unroll
        for (int r = 0; r < 12; ++r) x[r] = S.x[r] + sc * S.L[r][col];
        load_row<NU>(up + t * NU, u);
        // the per-thruster state is the lag state, as in rollout_pop_kernel
        if constexpr (MODEL == MODEL_THRUSTER_EULER && TRACK) lz.from_thrusters(relaunder(p), Xl);
        step_fast<MODEL, INTEG, LAGMODE, TRACK, true>(h, p, dt, x, u, lz, Xl, qt);
        if (lane == 0) {
#pragma unroll
            for (int r = 0; r < 12; ++r) S.c0[r] = x[r];
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
        if constexpr (TAPE) {
            if (lane < 12) tp[t * UKF_TAPE + UkfTapeRec<12>::XP + lane] = S.x[lane];  // xp_{t+1}
        }
        ukf_cov(S, f, wi, own, p0, p1);
        if constexpr (TAPE) {
            tp[t * UKF_TAPE + UkfTapeRec<12>::PP + lane] = p0;                         // Pp_{t+1}
            if (own.two) tp[t * UKF_TAPE + UkfTapeRec<12>::PP + 64 + lane] = p1;
            // C_{t+1}[ca][cb] = sum_j L[ca][j] (c W_i (d_{j+1} - d_{j+13})[cb]): L and D are still in the image
            const double g = cw * wi;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const int e = lane + 64 * k;
                if (e < 144) {
                    const int ca = e / 12, cb = e % 12;
                    double acc = 0.0;
#pragma unroll
                    for (int j = 0; j < 12; ++j) acc = fma(S.L[ca][j], g * (S.D[j + 1][cb] - S.D[j + 13][cb]), acc);
                    tp[t * UKF_TAPE + UkfTapeRec<12>::C + e] = acc;
                }
            }
        }
        ukf_wave_sync();                                               // P written
    }
    // ---- outputs -------------------------------------------------------------------------------------------------------------
    const bool ok = failed < 0;
    if (!ok) ukf_nan_rows(xfp, 12, psp, inp, lane, nan_from, T);
    if constexpr (TAPE) {
        // of a transition that did not complete xp, Pp and C are NaN; Pf_t stays when the update of row t was complete
        if (!ok) {
            for (int64_t i = (nan_from > failed ? failed * UKF_TAPE + UkfTapeRec<12>::XP : failed * UKF_TAPE) + lane; i < T * UKF_TAPE; i += 64) tp[i] = NaN;
        }
        if (lane == 0) a.nrows[(int64_t)blockIdx.y * B + b] = (double)nan_from;
    }
    if (a.xT && lane < 12) a.xT[row * 12 + lane] = ok ? S.x[lane] : NaN;
    ukf_put_tail(S, a.PT, a.info, row, lane, ell, nupd, failed, minpiv);
    if constexpr (MODEL == MODEL_THRUSTER_EULER && TRACK) {
        if (ok && lane == 0) store_row<24>(a.lag + row * 24, &Xl[0][0]);      // a failed filter leaves its lag_io as it came
    }
}

// ---------------------------------------------------------------------------------------
// Backward (Rauch-Tung-Striebel) pass over the tape (include/brov2.h: brov_ukf_rts_dev holds the law).  The filter's decomposition:
// one wave per (candidate, recording), UKF_WAVES per block, the time loop -- downwards -- inside, the wave's image in LDS with the
// stride-13 rows, ukf_wave_sync between phases and no workgroup barrier at all, so a ragged block or a problem without rows leaves.
// A transition t -> t + 1 (tape record t, row xf_t) takes
//   deposit   the record, fetched one transition ahead into 5 registers per lane (lane l holds doubles l, l + 64, ..: coalesced
//             loads, and Pf's entries land on the lanes that own them), goes to the image; the fetch of record t - 1 and of
//             xf_{t-1} is issued right after, so that its latency lies behind the work below;
//   Cholesky  of Pp, the filter's: one lane per row, the same pivot rule;
//   gain      lane a solves row a of G L L^T = C: forward through L, backward through L^T, L read wave-uniformly from the image;
//   M, dx     M = Ps_{t+1} - Pp by the lanes that own the entries (Ps stays in their registers over the pass), dx = xs_{t+1} - xp;
//   xs, G M   lane a: xs_t[a] = xf_t[a] + G[a][:] dx; the 144 entries of G M, one per lane and turn;
//   Ps        Ps_t[a][b] = Pf_t[a][b] + (G M)[a][:] G[b][:] by the owner of (a, b), written to both triangles of the image.
// Per row and problem 2.5 KB of tape come in (what the tape filter wrote), and 1.3 KB go out when Ps is asked for.
//
// EM: the pass also sums the sufficient statistics of the EM fit of q and r (include/brov2.h: brov_ukf_rts_em_dev holds the law) in
// registers of lanes 0..11, lane i owning component i: at the end of a transition, where the fewest values are live (after the gain
// the same code does not fit a lane's registers), lane i adds (Y[t][i] - xs_t[i])^2 + Ps_t[i][i] for the row just finished, solves
// Lp Lp^T u = e_i by the gain's two substitutions through the L image and adds q_i + q_i^2 (u^T M u + (u . dx)^2) with the M and dx
// of the image, which stay until the next deposit.  No LDS and no barrier of its own.  Every EM statement sits behind `if constexpr (EM)`;
// the EM = false instantiation is the code it was before (DESIGN.md section 4 has the comparison of the two listings).
struct UkfRtsLds {
    double rec[UKF_TAPE];               // the tape record of the transition
    double L[12][UKF_LD];               // Cholesky factor of Pp
    double G[12][UKF_LD];               // the smoother gain
    double M[12][UKF_LD];               // Ps_{t+1} - Pp_{t+1}, both triangles
    double GM[12][UKF_LD];
    double P[12][UKF_LD];               // Ps of the row last finished, both triangles
    double dx[12];
};

// EM: the process term of one transition for component i (include/brov2.h: brov_ukf_rts_em_dev), q_i + q_i^2 (u^T M u + (u . dx)^2) with
// u = Pp^-1 e_i: w from L w = e_i, then L^T u = w, the substitutions of a gain row, through the L, M and dx that the transition left
// in the image (they stay until the next transition's deposit).  Every sum in index order.
template <typename Lds>
__device__ __forceinline__ double ukf_em_term(const Lds& S, int i, double qi) {
    asm volatile("" : "+v"(i));                               // (keeps the twelve selects of e_i out of the loop-invariant registers)
    double u[12];
    ukf_fence();
#pragma unroll
    for (int j = 0; j < 12; ++j) u[j] = i == j ? 1.0 : 0.0;
    ukf_solve_llt(S, u);
    double umu = 0.0, udx = 0.0;
#pragma unroll
    for (int c = 0; c < 12; ++c) {
        double mu = 0.0;
#pragma unroll
        for (int k = 0; k < 12; ++k) mu = fma(S.M[c][k], u[k], mu);
        umu = fma(u[c], mu, umu);
        udx = fma(u[c], S.dx[c], udx);
    }
    ukf_fence();
    return qi + qi * qi * (umu + udx * udx);
}

template <bool EM>
__global__ void __launch_bounds__(64 * UKF_WAVES) ukf_rts_kernel(const UkfRtsArgs a) {
    __shared__ UkfRtsLds lds[UKF_WAVES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t B = a.B, T = a.T;
    const int64_t b = (int64_t)blockIdx.x * UKF_WAVES + wave;
    if (b >= B) return;                                       // a whole wave: there is no workgroup barrier
    UkfRtsLds& S = lds[wave];
    const int64_t loc = (int64_t)blockIdx.y * B + b;          // in the tape and nrows
    const int64_t row = (int64_t)blockIdx.y * a.Bs + b;       // in xf, the terminal pair and the outputs
    const double NaN = __builtin_nan(""), INF = __builtin_inf();
    const UkfOwn own = ukf_own(lane);
    const int a0 = own.a0, b0 = own.b0, a1 = own.a1, b1 = own.b1, lr = own.lr;
    const bool two = own.two;
    const double nd = ukf_uniform(a.nrows[loc]);
    const int64_t n = nd >= 1.0 ? (nd < (double)T ? (int64_t)nd : T) : 0;
    const double* tp = a.tape + loc * T * UKF_TAPE;
    const double* xfp = a.xf + row * T * 12 + lr;
    double* xsp = a.xs ? a.xs + row * T * 12 : nullptr;
    double* psp = a.pstd ? a.pstd + row * T * 12 : nullptr;
    double* Psp = a.Ps ? a.Ps + row * T * 144 : nullptr;
    // row s of the outputs: NaN, or (xsv, the image's P)
    auto put_nan = [&](int64_t s) {
        if (lane < 12) {
            if (xsp) xsp[s * 12 + lane] = NaN;
            if (psp) psp[s * 12 + lane] = NaN;
        }
        if (Psp) {
            for (int e = lane; e < 144; e += 64) Psp[s * 144 + e] = NaN;
        }
    };
    for (int64_t s = n; s < T; ++s) put_nan(s);
    // EM: the statistics of component lr, the noise model of this candidate, the rows of this recording
    double sq = 0.0, sr = 0.0, nr = 0.0, nq = 0.0, qi = 0.0, ri = 0.0;
    const double* yp = nullptr;
    if constexpr (EM) {
        const UkfRec* f = a.rec + (a.rec_per_candidate ? blockIdx.y : 0);
        qi = f->q[lr];
        ri = f->r[lr];
        yp = a.Y + b * T * 12 + lr;
    }
    auto put_em = [&](bool ok) {
        if constexpr (EM) {
            double* e = a.em + row * UKF_EM;
            if (lane < 12) {
                e[lane] = ok ? sq : NaN;
                e[12 + lane] = ok ? sr : NaN;
                e[24 + lane] = ok ? nr : NaN;
            }
            if (lane == 0) e[36] = ok ? nq : NaN;
        }
    };
    if (n == 0) {
        put_em(false);
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
    double xsv, ps0, ps1;
    if (terminal) {
        xsv = a.xsT[row * 12 + lr];
        ps0 = a.PsT[row * 144 + a0 * 12 + b0];
        ps1 = a.PsT[row * 144 + a1 * 12 + b1];
    } else {
        xsv = xfp[(n - 1) * 12];
        ps0 = tp[(n - 1) * UKF_TAPE + lane];
        ps1 = tp[(n - 1) * UKF_TAPE + (two ? lane + 64 : lane)];
    }
    auto image_P = [&] {
        ukf_put_P(S, own, ps0, ps1);
        ukf_wave_sync();
    };
    auto put_row = [&](int64_t s) {
        if (lane < 12) {
            if (xsp) xsp[s * 12 + lane] = xsv;
            if (psp) psp[s * 12 + lane] = sqrt(S.P[lane][lane]);
        }
        if (Psp) {
            for (int e = lane; e < 144; e += 64) Psp[s * 144 + e] = S.P[e / 12][e % 12];
        }
    };
    // EM: the measurement term of a row whose (xsv, the image's P) is final; y = Y[s][lr]
    auto em_row = [&](double y) {
        if constexpr (EM) {
            if (y == y && ri != INF) {
                double v = y - xsv;
                if (lr >= 3 && lr < 6) v = ukf_wrap(v);
                sr += v * v + S.P[lr][lr];
                nr += 1.0;
            }
        }
    };
    image_P();
    if (!terminal) {
        put_row(n - 1);
        if constexpr (EM) em_row(yp[(n - 1) * 12]);
    }
    // ---- the transitions, last first ---------------------------------------------------------------------------------------------
    double r[5], xfv, yv = 0.0;
    auto fetch = [&](int64_t t) {
#pragma unroll
        for (int k = 0; k < 4; ++k) r[k] = tp[t * UKF_TAPE + 64 * k + lane];
        r[4] = lane < UKF_TAPE - 256 ? tp[t * UKF_TAPE + 256 + lane] : 0.0;
        xfv = xfp[t * 12];
        if constexpr (EM) yv = yp[t * 12];
    };
    int64_t t = terminal ? n - 1 : n - 2, failed = -1;
    double minpiv = INF;
    if (t >= 0) fetch(t);
    for (; t >= 0; --t) {
#pragma unroll
        for (int k = 0; k < 4; ++k) S.rec[64 * k + lane] = r[k];
        if (lane < UKF_TAPE - 256) S.rec[256 + lane] = r[4];
        const double pf0 = r[0], pf1 = r[1], xft = xfv;       // Pf's entries lie on their owners
        const double yt = yv;
        if (t > 0) fetch(t - 1);
        ukf_wave_sync();                                      // rec written
        // Cholesky of Pp, as in the filter
        double Lr[12];
#pragma unroll
        for (int k = 0; k < 12; ++k) Lr[k] = S.rec[UkfTapeRec<12>::PP + (k <= lr ? lr * (lr + 1) / 2 + k : k * (k + 1) / 2 + lr)];
        bool bad = false;
#pragma unroll
        for (int j = 0; j < 12; ++j) ukf_cholesky_col(S, Lr, j, lane, lr, bad, minpiv);
        if (bad) { failed = t; break; }
        // row lr of G: w L^T = C[lr][:], then g L = w
        double g[12];
#pragma unroll
        for (int j = 0; j < 12; ++j) g[j] = S.rec[UkfTapeRec<12>::C + lr * 12 + j];
        ukf_solve_llt(S, g);
        if (lane < 12) {
#pragma unroll
            for (int k = 0; k < 12; ++k) S.G[lane][k] = g[k];
            S.dx[lane] = xsv - S.rec[UkfTapeRec<12>::XP + lane];              // not wrapped: xs, xp and xf live on the filter's continuous branch
        }
        ukf_put(S.M, a0, b0, ps0 - S.rec[UkfTapeRec<12>::PP + lane]);
        if (two) ukf_put(S.M, a1, b1, ps1 - S.rec[UkfTapeRec<12>::PP + 64 + lane]);
        ukf_wave_sync();                                      // G, dx, M written
        {
            double acc = 0.0;
#pragma unroll
            for (int k = 0; k < 12; ++k) acc = fma(g[k], S.dx[k], acc);
            xsv = xft + acc;
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
        ukf_wave_sync();                                      // GM written
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
        image_P();
        put_row(t);
        if constexpr (EM) {
            em_row(yt);
            sq += ukf_em_term(S, lr, qi);
            nq += 1.0;
        }
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
    put_em(ok);
}

hipError_t launch_ukf_rts(hipStream_t st, int P, const UkfRtsArgs& a) {
    if (a.B <= 0 || P <= 0) return hipSuccess;
    return a.em ? ukf_launch(ukf_rts_kernel<true>, st, P, a) : ukf_launch(ukf_rts_kernel<false>, st, P, a);
}

// ---------------------------------------------------------------------------------------
// launch: grid (blocks of UKF_WAVES recordings, P)
// ---------------------------------------------------------------------------------------
int ukf_waves_per_block() { return UKF_WAVES; }

template <int MODEL, int INTEG, int LAGMODE, bool TAPE>
static hipError_t launch_ukf_t(hipStream_t st, int P, const UkfArgs& a) {
    if constexpr (MODEL == MODEL_THRUSTER_EULER) {
        if (a.lag) return ukf_launch(ukf_filter_kernel<MODEL, INTEG, LAGMODE, true, TAPE>, st, P, a);
    }
    return ukf_launch(ukf_filter_kernel<MODEL, INTEG, LAGMODE, false, TAPE>, st, P, a);
}
template <int MODEL, bool TAPE>
static hipError_t launch_ukf_i(hipStream_t st, int integ, int lag_mode, int P, const UkfArgs& a) {
    if (integ == INTEG_EULER) return launch_ukf_t<MODEL, INTEG_EULER, 0, TAPE>(st, P, a);
    if constexpr (MODEL == MODEL_THRUSTER_EULER) {
        if (lag_mode == 1) return launch_ukf_t<MODEL, INTEG_RK4, 1, TAPE>(st, P, a);
    }
    return launch_ukf_t<MODEL, INTEG_RK4, 0, TAPE>(st, P, a);
}
template <int MODEL>
static hipError_t launch_ukf_m(hipStream_t st, int integ, int lag_mode, int P, const UkfArgs& a) {
    if (a.tape) return launch_ukf_i<MODEL, true>(st, integ, lag_mode, P, a);
    return launch_ukf_i<MODEL, false>(st, integ, lag_mode, P, a);
}
hipError_t launch_ukf_filter(hipStream_t st, int model, int integ, int lag_mode, int P, const UkfArgs& a0) {
    if (a0.B <= 0 || P <= 0) return hipSuccess;
    UkfArgs a = a0;
    if (model != MODEL_THRUSTER_EULER) a.lag = nullptr;
    switch (model) {
        case MODEL_THRUSTER_EULER: return launch_ukf_m<MODEL_THRUSTER_EULER>(st, integ, lag_mode, P, a);
        case MODEL_WRENCH_EULER: return launch_ukf_m<MODEL_WRENCH_EULER>(st, integ, lag_mode, P, a);
        default: return hipErrorInvalidValue;     // the quaternion model's mean lives on a manifold: ukf_quat.hip is its filter
    }
}

}  // namespace brov
