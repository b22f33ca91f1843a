// brov2_kernels.h -- host-side launch entry points of the HIP kernels (internal; the public
// boundary is include/brov2.h).  All pointers are device pointers; all launches are
// asynchronous on `st`.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "brov2_device.h"
#include "brov2_fast.h"

namespace brov {

// done / seq: when done != nullptr every row's thread stores seq to done[row] (system scope, release) after its results
hipError_t launch_rhs(hipStream_t st, const DevParams& p, int model, int64_t B, const double* x, const double* u,
                      double* lag, double* xd, unsigned long long* done = nullptr, unsigned long long seq = 0);
hipError_t launch_thruster_forces(hipStream_t st, const DevParams& p, int64_t B, const double* u, double* lag, double* tau,
                                  unsigned long long* done = nullptr, unsigned long long seq = 0);
hipError_t launch_rollout(hipStream_t st, const FastParams* d_fp, int model, int integ, int lag_mode, int layout, int64_t B,
                          int64_t T, double dt, const double* x0, const double* U, double* lag, double* traj,
                          int64_t stride, double* xT, int btu_staging);
// The BTU rollout for P parameter sets in one launch (d_fp [P], candidate = blockIdx.y; thruster and wrench models, always the
// GENERIC step).  x0 [B][nx] and U [B][T][nu] shared by the candidates, or with per_candidate [P][B][nx] and [P][B][T][nu];
// traj [P][B][T/stride+1][nx], xT [P][B][nx], lag [P][B][24] (in / out) per candidate, each or nullptr.  1 <= P <= 65535.
hipError_t launch_rollout_pop(hipStream_t st, const FastParams* d_fp, int model, int integ, int lag_mode, int P, int per_candidate,
                              int64_t B, int64_t T, double dt, const double* x0, const double* U, double* lag, double* traj,
                              int64_t stride, double* xT);
// Closed-loop form of launch_rollout_pop (feedback.hip): the command of every step comes from a linear feedback law evaluated
// inside the kernel (include/brov2.h: brov_rollout_feedback).  FeedbackRec is struct brov_feedback byte for byte; d_fb holds one
// record (fb_per_candidate = 0) or P.  x0 [.][B][nx], u_ff [.][B][T][nu] (nullptr = 0) and ref [.][B][ref_rows][nx] are shared or per
// candidate together (per_candidate); every output is per candidate and may be nullptr: lag [P][B][24] and z [P][B][6] in / out,
// traj [P][B][T/stride+1][nx], xT [P][B][nx], u_applied [P][B][T][nu], metrics [P][B][4].
struct FeedbackRec {
    double K[8][12], Ki[8][6];
    double u_min[8], u_max[8];
    double z_max[6];
    int32_t hold, pad;
};
struct FeedbackArgs {
    const FastParams* fp;
    const FeedbackRec* fb;
    int fb_per_candidate, per_candidate;
    int64_t B, T, ref_rows, stride;
    double dt;
    const double *x0, *u_ff, *ref;
    double *lag, *z, *traj, *xT, *u_applied, *metrics;
};
hipError_t launch_rollout_feedback(hipStream_t st, int model, int integ, int lag_mode, int P, const FeedbackArgs& a);
// Unscented Kalman filter on the 12-state models (ukf.hip; include/brov2.h: brov_ukf_filter holds the law): candidate j filters B
// recordings of T rows.  UkfRec is what the host derives from one struct brov_ukf (c = sqrt(n + lambda), the centre weight of the
// covariance and the weight of the other 24 points); d_rec holds one record (rec_per_candidate = 0) or P.  x0 [B][12], P0
// [B][12][12], U [B][T][nu] and Y [B][T][12] are shared by the candidates; every output is per candidate and may be nullptr: lag
// [P][B][24] in / out, xf, pstd, innov [P][B][T][12], xT [P][B][12], PT [P][B][144], info [P][B][4].  One launch; T >= 1.
struct UkfRec {
    double q[12], r[12];
    double c, wc0, wi, pad;
};
struct UkfArgs {
    const FastParams* fp;
    const UkfRec* rec;
    int rec_per_candidate, pad;
    int64_t B, T;
    double dt;
    const double *x0, *P0, *U, *Y;
    double *lag, *xf, *pstd, *innov, *xT, *PT, *info;
    // the tape variant (tape != nullptr) alone reads these: tape [P][B][T][UKF_TAPE], nrows [P][B], and Bs, the number of recordings
    // that the per-candidate outputs and lag are laid out for (>= B: the B recordings of this launch are a chunk of Bs, and the
    // input and output pointers already point at the chunk's first recording)
    double *tape, *nrows;
    int64_t Bs;
};
// One tape record of a model whose state is NX wide (include/brov2.h): Pf [78] | xp [NX] | Pp [78] | C [12][12], the triangles row by
// row.  The offsets, in doubles; the filters' tape variants write through them, the backward kernels read through them.
template <int NX_>
struct UkfTapeRec {
    static constexpr int NX = NX_, PF = 0, XP = PF + 78, PP = XP + NX, C = PP + 78, SIZE = C + 144;
};
constexpr int UKF_TAPE = UkfTapeRec<12>::SIZE;          // doubles of one tape record of the Euler models
int ukf_waves_per_block();      // recordings per block of the filter kernel and of the backward kernel
hipError_t launch_ukf_filter(hipStream_t st, int model, int integ, int lag_mode, int P, const UkfArgs& a);
// The multiplicative filter on the quaternion model (ukf_quat.hip; include/brov2.h: brov_ukf_filter_quat holds the law).  UkfArgs with
// x0 [B][13], Y [B][T][13], xf [P][B][T][13] and xT [P][B][13]; P0, pstd, innov, PT and the records stay in the 12-component error
// state; lag is not read.  tape != nullptr selects the tape variant, which alone reads tape [P][B][T][UKF_TAPE_QUAT], nrows [P][B] and
// Bs, with the meaning they have in launch_ukf_filter.  One launch; T >= 1.
constexpr int UKF_TAPE_QUAT = UkfTapeRec<13>::SIZE;     // ... and of the quaternion model
static_assert(UKF_TAPE == 312 && UKF_TAPE_QUAT == 313, "the record sizes that include/brov2.h documents");
hipError_t launch_ukf_filter_quat(hipStream_t st, int integ, int P, const UkfArgs& a);
// Backward (Rauch-Tung-Striebel) pass over a tape (ukf.hip; include/brov2.h: brov_ukf_rts_dev holds the law).  tape [P][B][T][UKF_TAPE]
// and nrows [P][B] are a chunk's own; xf, the terminal pair and every output are laid out for Bs recordings per candidate and point
// at the chunk's first recording.  xsT / PsT both nullptr or both set; every output may be nullptr.
// em != nullptr selects the EM instantiation, which alone reads the fields behind sinfo: em [P][Bs][UKF_EM] (laid out like the other
// outputs), Y [B][T][12] at the chunk's first recording (shared by the candidates), and the filter's records rec (one, or P).
struct UkfRtsArgs {
    int64_t B, T, Bs;
    const double *xf, *tape, *nrows, *xsT, *PsT;
    double *xs, *pstd, *Ps, *Ps0, *sinfo;
    double* em;
    const double* Y;
    const UkfRec* rec;
    int rec_per_candidate, pad;
};
constexpr int UKF_EM = 37;      // doubles of one em record: Sq [12] | Sr [12] | nr [12] | nq  (include/brov2.h)
hipError_t launch_ukf_rts(hipStream_t st, int P, const UkfRtsArgs& a);
// The backward pass of the quaternion model (ukf_quat.hip; include/brov2.h: brov_ukf_rts_quat_dev holds the law): UkfRtsArgs with tape
// [P][B][T][UKF_TAPE_QUAT] and xf, xsT, xs 13 wide; the fields behind sinfo are not read.
hipError_t launch_ukf_rts_quat(hipStream_t st, int P, const UkfRtsArgs& a);
// Output-feedback closed loop (ukf_feedback.hip; include/brov2.h: brov_output_feedback holds the law): candidate j runs B closed loops
// of T steps, the filter of launch_ukf_filter under fp[j] inside the loop, the law of launch_rollout_feedback on its estimate, the
// plant under plant[j] (plant_per_candidate) or plant[0].  rec and fb hold one record or P.  x0_true, x0_est [B][12], P0 [B][12][12],
// V [B][T][12], W [B][T][12] or nullptr, u_ff [B][T][nu] or nullptr and ref [B][ref_rows][12] are shared by the candidates; everything
// else is per candidate and may be nullptr: lag_est, lag_plant [P][B][24] (both or neither) and z [P][B][6] in / out, traj
// [P][B][T+1][12], y_out, xf, pstd, innov [P][B][T][12], u_applied [P][B][T][nu], xT_true, xT [P][B][12], PT [P][B][144], metrics
// [P][B][7], info [P][B][4].  One launch; T >= 1.
struct UkfFbArgs {
    const FastParams *fp, *plant;
    const UkfRec* rec;
    const FeedbackRec* fb;
    int rec_per_candidate, fb_per_candidate, plant_per_candidate, pad;
    int64_t B, T, ref_rows;
    double dt;
    const double *x0_true, *x0_est, *P0, *V, *W, *u_ff, *ref;
    double *lag_est, *lag_plant, *z;
    double *traj, *y_out, *u_applied, *xf, *pstd, *innov;
    double *xT_true, *xT, *PT, *metrics, *info;
};
hipError_t launch_ukf_feedback(hipStream_t st, int model, int integ, int lag_mode, int P, const UkfFbArgs& a);
// One MPPI update for B problems (mppi.hip; include/brov2.h: brov_mppi_step holds the law).  MppiRec is struct brov_mppi byte for
// byte; rec is ONE device record.  fp holds one parameter set (per_problem = 0) or B.  x [B][nx], lag [B][24] or nullptr (zero), ref
// [B][ref_total][nx], eps [B][K][M][nu] or nullptr (the seeded stream), U_nom [B][M][nu] in / out, M = ceil(H / hold).  cost [B][K]
// and U_old [B][M][nu] are never nullptr here (scratch when the caller wants no costs; U_old receives the knots as they came);
// u_apply [B][hold][nu] and info [B][4] may be.  Two launches, whatever B, K and H are.
struct MppiRec {
    double q[12], qf[12];
    double r[8], sigma[8];
    double u_min[8], u_max[8];
    double lambda, gamma;
    int32_t hold, pad;
};
struct MppiArgs {
    const FastParams* fp;
    const MppiRec* rec;
    int per_problem, shift;
    int64_t K, H, M, ref_total, ref_row0;
    double dt;
    uint64_t seed;
    const double *x, *lag, *ref, *eps;
    double *U_nom, *U_old, *u_apply, *cost, *info;
};
hipError_t launch_mppi_step(hipStream_t st, int model, int integ, int lag_mode, int64_t B, const MppiArgs& a);
// the second launch alone (nu = 6 or 8): reads rec, K, M, shift, seed, eps, cost, U_old; writes U_nom, u_apply, info
hipError_t launch_mppi_update(hipStream_t st, int nu, int64_t B, const MppiArgs& a);
// The same update with an EDMDc model as the planning model (koopman_mppi.hip; include/brov2.h: edmdc_mppi_step holds the law).
// m: as above, without fp, per_problem and lag; x [B][n], ref [B][ref_total][n].  C [k][n]; P [H+1][n][n+k] and Gc [H+1][M][n][r] are
// the coefficients of the linear form; F [B][H+1][n] is scratch (the free response), pred [B][K][H+1][n] or nullptr.  n in {12, 13},
// r in {6, 8}, 0 <= k <= KOOPMAN_MPPI_MAX_K, M r <= KOOPMAN_MPPI_MAX_MNU.  Three launches, whatever B, K and H are.
constexpr int KOOPMAN_MPPI_MAX_K = 1024;          // the lift of one state lives in LDS
constexpr int KOOPMAN_MPPI_MAX_MNU = 312;         // a sample's commands live in LDS: 64 lanes x 312 doubles = 156 KB of the 160 KB
struct KoopmanMppiArgs {
    MppiArgs m;
    int n, r, k;
    double gamma;
    const double *C, *P, *Gc;
    double *F, *pred;
};
int koopman_mppi_block(int64_t K, int64_t mnu);   // lanes per block of the cost kernel: 256, 128 or 64 as the LDS allows (0: does not fit)
hipError_t launch_koopman_mppi_step(hipStream_t st, int64_t B, const KoopmanMppiArgs& a);
// the first launch alone, F [B][H+1][n] = P[t] phi(x_b): reads n, k, gamma, C, P, m.x, m.H; writes F
hipError_t launch_koopman_free(hipStream_t st, int64_t B, const KoopmanMppiArgs& a);
// The linear MPC on the same coefficients: a box-constrained QP per problem, solved by ADMM (koopman_qp.hip; include/brov2.h:
// edmdc_lmpc_step holds the law).  LmpcRec is struct brov_lmpc byte for byte; rec is ONE device record.  f: the arguments of
// launch_koopman_free (f.F is scratch) and f.m.ref, ref_total, ref_row0, dt, M, shift, U_nom, u_apply, info [B][6]; f.pred [B][H+1][n] or
// nullptr.  W [Nv][Nv], y [B][Nv] or nullptr, g [B][Nv] and c0 [B] scratch.  Three launches, whatever B, H and iters are.
struct LmpcRec {
    double q[13], qf[13];
    double r[8];
    double u_min[8], u_max[8];
    double rho, tol;
    int32_t hold, iters;
};
struct KoopmanQpArgs {
    KoopmanMppiArgs f;
    const LmpcRec* rec;
    const double* W;
    double *y, *g, *c0;
};
constexpr int KOOPMAN_QP_WAVES = 4;               // problems (waves) per block of the solve kernel
size_t koopman_qp_block(int64_t nv, bool* w_in_lds);   // dynamic LDS bytes of a solve block; *w_in_lds: W is staged into them
hipError_t launch_koopman_qp_step(hipStream_t st, int64_t B, const KoopmanQpArgs& a);
// vals [P][M] -> out [4][M]: mean, sample standard deviation, minimum, maximum over the P candidates; NaN where any is non-finite
hipError_t launch_ensemble_stats(hipStream_t st, int64_t P, int64_t M, const double* vals, double* out);
// The sliding-window evaluator for P parameter sets at once (d_fp [P], candidate = blockIdx.y; P = 1: one set).  Candidate-major
// scratch: d_phi [P][18] ([Phi | Phi^window_scan_chunk()] of each candidate), d_lag [P][N-H][18] and d_chunk [P][chunks][18]
// (thruster model with carry_lag only), d_se [P][N-H]; d_total [P]; d_endpoints [P][N-H][nx] or nullptr.  The launch count does
// not depend on P.
hipError_t launch_window_endpoint(hipStream_t st, const FastParams* d_fp, int model, int integ, int P, int64_t N, int64_t H, double dt,
                                  const double* X, const double* U, int carry_lag, const double* d_phi, double* d_lag,
                                  double* d_chunk, double* d_se, double* d_total, double* d_endpoints);
// The same over several recordings (bags) in row-aligned X and U.  d_tab = [wpre [nbags + 1] | off [nbags + 1]] (int64): the windows
// before each bag and its first row; nwin = wpre[nbags].  d_wrow [nwin] and d_wopen [chunks] are scratch for the window-to-row map,
// built by the first launch; d_target [nwin][nx] or nullptr: the rows the windows are scored against.  With carry_lag every bag
// starts from zero lag.  P = 0 writes d_target alone.  One launch more than launch_window_endpoint, whatever nbags and P are.
hipError_t launch_window_endpoint_ragged(hipStream_t st, const FastParams* d_fp, int model, int integ, int P, int64_t nbags,
                                         const int64_t* d_tab, int64_t nwin, int64_t H, double dt, const double* X, const double* U,
                                         int carry_lag, const double* d_phi, double* d_lag, double* d_chunk, int64_t* d_wrow,
                                         unsigned long long* d_wopen, double* d_se, double* d_total, double* d_endpoints,
                                         double* d_target);
// Finite-difference normal equations (rollout.hip): d_E [(m+1)][R], R = W nx; d_part fd_normal_blocks(R) x (m+1)(m+2)/2 doubles;
// d_out = [JtJ (m x m) | Jtr (m)].
int fd_normal_blocks(int64_t R);
hipError_t launch_fd_normal_eq(hipStream_t st, int nx, int m, int64_t R, const double* d_E, const double* d_target, const double* d_delta,
                               const double* d_weight, double* d_part, double* d_out);
hipError_t launch_fill_controls(hipStream_t st, int layout, int dist, int64_t B, int64_t T, int nu, uint64_t seed,
                                int64_t b0, int64_t T_total, const double* scale8, double* U);

int probe_xcd_round_robin(hipStream_t st);

// ---- EDMDc -----------------------------------------------------------------------------
// Lifted row layout (device native, "Z rows"): [rbf_0 .. rbf_{kp-1} | x_0..x_{n-1} u_0..u_{r-1} 0..]
// with kp = k rounded up to 16 and the tail block (n + r) rounded up to 16; width = kp + tailp.
struct EdmdcShape {
    int n, r, k;
    int kp;      // k padded to a multiple of 16
    int tailp;   // (n + r) padded to a multiple of 16
    int width;   // kp + tailp  (doubles per lifted row)
    int d, p;    // n + k, n + k + r
    int xplus;   // 1: the padding of the tail is wide enough for x_{t+1} (n + r + n <= tailp); lift_rows writes it there and the
                 //    Gram takes the x part of Y from the row's own last tile instead of from a 33rd Y tile of the next row
};
inline EdmdcShape edmdc_shape(int n, int r, int k) {
    EdmdcShape s;
    s.n = n; s.r = r; s.k = k;
    s.kp = (k + 15) / 16 * 16;
    s.tailp = (n + r + 15) / 16 * 16;
    s.width = s.kp + s.tailp;
    s.d = n + k; s.p = n + k + r;
    s.xplus = (n + r + n <= s.tailp) ? 1 : 0;
    return s;
}
// Reference-order lift Z[N][n+k] = [x, rbf]  (edmdc_lift C entry point)
hipError_t launch_lift_ref(hipStream_t st, int64_t N, int n, int k, double gamma, const double* X, const double* C, double* Z);
// multistep_rmse by linearity: se[w] = |X[w + H] - (RHt^T phi(x_w) + sum_t Gt[t]^T u_{w+t})|^2 for w < nw; RHt [n + k][n], Gt [H][r][n]; xhat [nw][n] optional
hipError_t launch_linear_windows(hipStream_t st, int64_t nw, int n, int r, int k, int64_t H, double gamma, const double* X, const double* U,
                                 const double* C, const double* RHt, const double* Gt, double* se, double* xhat);
// Device-native lifted rows for `rows` consecutive state rows starting at global row `row0`
// (bag structure: state row index = b * xs + t, t in [0, L]; input row = b * us + t, t < L).
// Rows >= total_rows (and gap rows t > L) are written as zeros with weight 0.
// pairflag != nullptr: ragged bags -- X / U hold the bags' rows one after the other (U row-aligned with X), pairflag[g] = 1 when rows
// (g, g + 1) belong to one bag (launch_bag_pairflags); pass xs > total_rows and L = xs - 1.
hipError_t launch_lift_rows_total(hipStream_t st, const EdmdcShape& s, double gamma, const double* C,
                                  int64_t row0, int64_t rows, int64_t total_rows, int64_t L, int64_t xs, int64_t us,
                                  const double* X, const double* U, double* Zrows, double* wrow, const unsigned char* pairflag = nullptr);
// pairflag[g] = 1 for every row g < total_rows that has a successor in its own bag: bag b = rows [offsets[b], offsets[b + 1])
hipError_t launch_bag_pairflags(hipStream_t st, int64_t nbags, const int64_t* d_offsets, int64_t total_rows, unsigned char* pairflag);
// Gram task table (device copy owned by the ctx) and sizes.
// partial: [ntasks][nslab][24 tiles][64 lanes][4] doubles.
// mode 0: tasks of G^T[G|Y]; mode 1: tasks of W^T Y (edmdc_pinv_apply)
size_t gram_partial_doubles(const EdmdcShape& s, int mode, int* ntasks_out, int* nslab_out);
size_t gram_task_bytes(const EdmdcShape& s, int mode);
hipError_t upload_gram_tasks(hipStream_t st, const EdmdcShape& s, int mode, void* d_tasks, size_t cap_bytes, int* ntasks);
// Gram of one chunk: pairs (row, row+1) for row in [0, npairs) of Zrows (4*ceil(npairs/4)+1 rows lifted),
// weight wrow[row]; accumulated into `partial` in place when `accumulate`.
// Arows: rows the A operand is cut from (== Zrows for the Gram; the rows of W = G P^T for edmdc_pinv_apply)
hipError_t launch_gram_chunk_tasks(hipStream_t st, const EdmdcShape& s, int ntasks, const void* d_tasks, int64_t npairs,
                                   const double* Arows, const double* Zrows, const double* wrow, double* partial, int accumulate);
// Wrows[rows][width] = Zrows . PdT  (PdT [width][width] = P^T in device feature order)
// (PdT needs 8 extra rows of allocation: the tuned kernel prefetches two K-steps past the last feature; simple = the round-2 kernel)
hipError_t launch_rows_times_pt(hipStream_t st, const EdmdcShape& s, int64_t rows, const double* Zrows, const double* PdT, double* Wrows,
                                int simple = 0);
void wrows_decomposition(const EdmdcShape& s, int* items_per_unit, int* tiles_wanted_per_unit);
int edmdc_dev_to_ref_feature(const EdmdcShape& s, int f);
// Sum partials over slabs (fixed order) and scatter into reference-order GtG [p][p], GtY [p][d].
hipError_t launch_gram_finish_tasks(hipStream_t st, const EdmdcShape& s, int ntasks, const void* d_tasks, const double* partial,
                                    int accumulate_out, double* GtG, double* GtY);

// ---- lifted propagation (propagate.hip) ---------------------------------------------------
struct PropShape {
    int n, r, k, d, p;
    int dpad;      // d padded to 48 (feature rows of Zt / columns of ABt)
    int ksteps;    // ceil(p / 4)
    int ppad;      // 4 * ksteps (rows of ABt)
    int64_t nw;    // windows (or simulated trajectories)
    int64_t nwp;   // nw padded to 128
    int zrows;     // rows of a Zt buffer: max(dpad, ppad) -- lifted state rows, then the r input rows of the current step
};
PropShape prop_shape(int n, int r, int k, int64_t nw);
hipError_t launch_lift_t(hipStream_t st, const PropShape& s, double gamma, int64_t xstride, const double* X, const double* C, double* Zt);
hipError_t launch_transpose(hipStream_t st, int64_t rows, int64_t cols, const double* src, int64_t lds_, double* dst, int64_t ldd);
hipError_t launch_set_input_rows(hipStream_t st, const PropShape& s, const double* U, int64_t ldu, double* Zt);
int64_t prop_window_blocks(const PropShape& s);
hipError_t launch_propagate(hipStream_t st, const PropShape& s, const double* ABt, const double* Zin, const double* Unext, int64_t ldu, double* Zout,
                            int64_t wb0 = 0, int64_t nwb = -1);
hipError_t launch_endpoint_se(hipStream_t st, const PropShape& s, int64_t xstride, const double* Xref, const double* Zt, double* se, double* xhat);
hipError_t launch_extract_state(hipStream_t st, const PropShape& s, int64_t T1, int64_t t, const double* Zt, double* Xp);
hipError_t launch_useq_t(hipStream_t st, const PropShape& s, int64_t T, const double* Us, double* Ust);
int window_scan_chunk();
// blocked scan of the windows' initial lag states (rollout.hip): x_{k+1} = Phi x_k + resp_k over nc lag banks of 3 states
// (6: the Fossen evaluator's wrench space, 8: the PINc evaluator's thruster space), for P candidates, in place.
// d_phi [P][18] = [Phi | Phi^window_scan_chunk()], d_rs [P][nwin][nc][3]: the responses on entry, the start states on exit;
// d_chunk [P][nchunks][nc][3]: scratch; d_s0 [nc][3] or nullptr (zero): the state before the first window, every candidate's
hipError_t launch_window_lag_scan(hipStream_t st, int nc, int P, int64_t nwin, const double* d_phi, double* d_rs, double* d_chunk,
                                  const double* d_s0);
// out[0] = the sum of v[0..n), a fixed-shape tree
hipError_t launch_sum(hipStream_t st, int64_t n, const double* v, double* out);

// ---- column statistics (colstats.hip) -------------------------------------------------------
// partial [colstats_blocks(N)][16]: per-block sums of x (squares = false) or of (x - d_shift)^2 (squares = true) per column
int colstats_blocks(int64_t N);
hipError_t launch_colstats(hipStream_t st, int64_t N, int n, const double* X, int64_t xstride, const double* d_shift, bool squares,
                           double* d_partial);

// copy by the shader cores, 16-byte words (both pointers 16-byte aligned, bytes a multiple of 16); src or dst may be pinned host memory
hipError_t launch_copy_bytes(hipStream_t st, void* dst, const void* src, size_t bytes);

// ---- k-means (kmeans.hip) ------------------------------------------------------------------
int kmeans_blocks(int64_t N, int n, int k, bool scalar_records);
int kmeans_epochs(int64_t N, int n, int k, bool scalar_records);
size_t kmeans_partial_words(int64_t N, int n, int k, bool scalar_records);      // u64 words of the E-step's partial tables
size_t kmeans_red_words(int n, int k);                                          // int64 words of the totals (+ 2 tail words)
bool kmeans_reads_through_perm(int n, int k, bool scalar_records);
hipError_t launch_kmeans_c2(hipStream_t st, int n, int k, const double* C, double* c2);
hipError_t launch_kmeans_range(hipStream_t st, int64_t N, int n, const double* X, int64_t xstride, const double* mean, unsigned long long* rng);
hipError_t launch_kmeans_scale(hipStream_t st, int n, const unsigned long long* rng, double* fix, double* prm);
// distance bounds of the sorted loop (kmeans.hip: kmeans_bounds_kernel): per-position bounds moved by the centres' shifts; the positions
// whose bounds fail go to `list` (tiles padded to whole waves with ~position), their number to nlist[0]
// nlist: [0] the list's entries (one-region form) | [KM_NL_TICKET] tickets drawn by the E-step | [KM_NL_FRONT], [KM_NL_BACK] entries of the two
// regions (two-region form; [0] stays 0) -- every counter in its own 64-byte line: atomics on one line are served one after the other
// (83 per microsecond, tools/attic/atomic_ticket_probe.hip), and 2 442 tiles reserving their piece of the list are 29 us of that
constexpr int KM_NL_TICKET = 16, KM_NL_FRONT = 32, KM_NL_BACK = 48;
struct KmBounds {
    float* ub = nullptr;            // [N] >= distance to the own centre
    float* lb = nullptr;            // [N] <= distance to every other centre
    const float* shiftc = nullptr;  // [k + kmeans_bounds_tail()] from launch_kmeans_average
    const float* mvd = nullptr;     // [k][4] from launch_kmeans_cdist: distances to the centres that moved most
    const float* rw2 = nullptr;     // [k] from launch_kmeans_cdist, or nullptr: squared radius beyond which a centre's samples make expensive passes
                                    //     (given: the list lies in two regions, the tiles with such samples in front; nlist[2] = their entries)
    int* list = nullptr;            // [kmeans_bounds_list_words(N)]
    int* nlist = nullptr;           // [64]: counters of the list and of the E-step's tickets, one per 64-byte line (kmeans.hip: KM_NL_*)
    double beta = -1.0;             // >= 0: the prefix of a pass that leaves bounds is cut at 2 (1 + beta) u (default KM_BND_BETA)
    bool use_list = false;          // the E-step visits the list only and its partials are CHANGES (launch_kmeans_mstep: delta)
};
size_t kmeans_bounds_list_words(int64_t N);
hipError_t launch_kmeans_bounds(hipStream_t st, int64_t N, int k, const int* labels, const KmBounds& b, const double* prm);
// E-step; Dc != nullptr selects the candidate-filtered form (Dc [k][k rounded up to 256] floats from launch_kmeans_cdist); prm [4], fix [32] from launch_kmeans_scale
hipError_t launch_kmeans_assign(hipStream_t st, int64_t N, int n, int k, const double* X, int64_t xstride, const double* mean,
                                const double* c2, int* labels, unsigned long long* partial, double* block_inertia, int* block_changed,
                                const float* Dc, const double* prm, const double* fix, float* d2out, bool scalar_records, const int* perm = nullptr,
                                const unsigned long long* Nk = nullptr, const float* Pf = nullptr, const KmBounds* bounds = nullptr);
// Dc [k][kp] (kp = k rounded up to 256); Nk (optional, kp <= 512): every row once more sorted, as keys (distance bits << 16 | centre index)
// Pf (optional, with Nk; n <= 13): the sorted rows once more as float pair records [k][kp / 2][32] for kmeans_assign_pk_kernel
struct KmMstepArgs;
hipError_t launch_kmeans_cdist(hipStream_t st, int n, int k, const double* c2, float* Dc, unsigned long long* Nk = nullptr, float* Pf = nullptr,
                               const float* shiftc = nullptr, float* mvd = nullptr, float* rw2 = nullptr, int pf_pairs = 0,
                               const KmMstepArgs* tail = nullptr);
int kmeans_bounds_tail();
int kmeans_lds_pf_pairs();          // pair records per row the LDS / DPP kernel's screening can reach (pf_pairs of launch_kmeans_cdist when it is Pf's only reader)
// E-step with packed-fp32 screening of the candidates (kmeans.hip, third form): labels, scores and member sums as the other kernels'
int kmeans_pk_blocks(int64_t N, int n, int k);
int kmeans_pk_epochs(int64_t N, int n, int k);
bool kmeans_pk_supported(int n, int k);
hipError_t launch_kmeans_assign_pk(hipStream_t st, int64_t N, int n, int k, const double* X, int64_t xstride, const double* mean, const double* c2,
                                   int* labels, unsigned long long* partial, double* block_inertia, int* block_changed, const double* prm,
                                   const double* fix, float* d2out, const int* perm, const unsigned long long* Nk, const float* Pf);
hipError_t launch_kmeans_average(hipStream_t st, int n, int k, const long long* red, const double* fix, const double* Cold, double* Cnew,
                                 double* c2, double* stats, double* prm, int mode, float* shiftc = nullptr, int* nlist = nullptr);
// the M-step as one launch (kmeans.hip: kmeans_mstep_kernel): phases 1 = sums, 2 = centres + tail (from `red`), 3 = both
struct KmMstepArgs {
    int nparts = 0, nblocks = 0, n = 0, k = 0;
    const unsigned long long* partial = nullptr;
    const double* block_inertia = nullptr;
    const int* block_changed = nullptr;
    long long* red = nullptr;
    long long* tot = nullptr;
    int delta = 0;
    int* nlist = nullptr;               // the counter of the bounds list (read when delta, zeroed for the next list)
    const double* fix = nullptr;
    const double* Cold = nullptr;
    double* Cnew = nullptr;
    double* Ct = nullptr;
    double* stats = nullptr;
    double* prm = nullptr;
    float* shiftc = nullptr;
    float* mvd = nullptr;
    double* scratch = nullptr;          // [kmeans_mstep_scratch_doubles(k)], zeroed once before the loop (its ticket word)
    double* hstats = nullptr;           // pinned, device-mapped [5] or nullptr: four statistics, then `seq`
    double seq = 0.0;
    bool tail_deferred = false;         // the one-block global part (sum of shifts, empty clusters, movers, the host's statistics) is not launched here:
                                        // the caller hands these arguments to the launch_kmeans_cdist that follows (`tail`), which runs it as one more block
};
size_t kmeans_mstep_scratch_doubles(int k);
hipError_t launch_kmeans_mstep(hipStream_t st, const KmMstepArgs& a, int phases);
hipError_t launch_kmeans_reloc_dist(hipStream_t st, int64_t N, int n, const double* X, int64_t xstride, const double* mean, const double* Cold,
                                    const int* labels, const int* perm, double* dist_row, int* lab_row);
// the inertia of the returned labels and centres by differences: partial [kmeans_inertia_blocks(N)], added by the host in block order
int kmeans_inertia_blocks(int64_t N);
hipError_t launch_kmeans_inertia(hipStream_t st, int64_t N, int n, int k, const double* X, int64_t xstride, const double* mean, const double* C,
                                 const int* labels, double* partial);


// width of the label field in the sort keys of the Lloyd loop's sample order (sortperm.hip); kmeans.hip checks its own limit against it
constexpr int KM_SORT_LABEL_BITS = 10;
constexpr int KM_SORT_LABEL_MAX = 1 << KM_SORT_LABEL_BITS;
// sample order of the Lloyd loop (sortperm.hip): sort by (label, distance to the centre), gather rows / labels / permutation
size_t kmeans_sort_temp_bytes(int64_t N);
hipError_t launch_kmeans_resort(hipStream_t st, int64_t N, const int* labels_old, int* labels_new, const int* perm_old, int* perm_new,
                                const float* d2, unsigned* keys_in, unsigned* keys_out, unsigned* vals_in, unsigned* vals_out, void* temp,
                                size_t temp_bytes, float* d2_new = nullptr, const float* ub_old = nullptr, float* ub_new = nullptr,
                                const float* lb_old = nullptr, float* lb_new = nullptr);
hipError_t launch_kmeans_unpermute(hipStream_t st, int64_t N, const int* perm, const int* labels_sorted, int* labels_out);

int kmeanspp_chunks(int64_t N);
size_t kmeanspp_sum_doubles(int64_t N);
size_t kmeanspp_state_bytes();
hipError_t launch_kmeanspp(hipStream_t st, int64_t N, int n, int k, int L, const double* X, int64_t xstride, const double* mean,
                           long long first, const double* u, double* Xt, double* xsq, double* closest, double* S,
                           void* state, double* C, long long* indices, float* Xf, void* rowbuf = nullptr);
// scratch of the seeding's row level (a ball, the largest closest and the sum of closest per row of 16 samples): bytes, 256-aligned pieces
size_t kmeanspp_row_bytes(int64_t N, int n);

size_t kmeanspp_shard_doubles(int world);
hipError_t launch_kmeanspp_sharded(hipStream_t st, int64_t N, int n, int k, int L, const double* X, int64_t xstride, const double* mean,
                                   long long first, const double* u, double* Xt, double* xsq, double* closest, double* S,
                                   void* state, double* C, long long* indices, float* Xf, int world, int rank, long long row0,
                                   double* shard, int (*exch)(void*, void*, int64_t, int), void* user, int* comm_failed, void* rowbuf = nullptr);

// ---- PINc residual network (pinc.hip) -------------------------------------------------------
// w: the packed fp32 weight blob (PINC_NPARAMS floats, state-dict order), p: the thruster map at this call's dt
constexpr int PINC_NPARAMS = 14541;
hipError_t launch_pinc_forward(hipStream_t st, const float* w, int64_t B, const float* z, float* x_next);
hipError_t launch_pinc_rollout(hipStream_t st, const float* w, const DevParams& p, int64_t B, int64_t T, double dt, const double* x0,
                               const double* U, double* lag_io, double* traj, int64_t stride, double* xT);
// d_lag [nwin][24] / d_chunk [chunks][24]: the arrays of launch_window_lag_scan (nc = 8, P = 1), used when carry_lag; d_lag_io [8][3]
// (nullptr = zero) is the lag before the first window and, with carry_lag, receives the lag after the last one; d_lag_starts
// [nwin][8][3] optional
hipError_t launch_pinc_window_endpoint(hipStream_t st, const float* w, const DevParams& p, int64_t N, int64_t H, double dt,
                                       const double* X, const double* U, int carry_lag, const double* d_phi, double* d_lag,
                                       double* d_chunk, double* d_lag_io, double* d_lag_starts, double* d_se, double* d_total);

// ---- PINc training (pinc_train.hip) ------------------------------------------------------------
constexpr int PINC_PART_STRIDE = PINC_NPARAMS + 3;    // one workgroup's partial: the gradient in blob order, then three loss sums
constexpr int PINC_TRAIN_MAX_K = 16;                  // rollout steps whose activations fit the LDS tape
struct PincAdam { double lr, beta1, beta2, eps, weight_decay, max_norm; };
int pinc_grad_parts(int B);                           // partials launch_pinc_grad writes for a minibatch of B rows
// one minibatch: Z [*][14], Y [*][9], U4 [*][4] fp32, row r of the batch = row perm[r] (perm nullptr: row r); K rollout steps from
// batch row 0 (0 = none, <= PINC_TRAIN_MAX_K and < B) -> part [pinc_grad_parts(B)][PINC_PART_STRIDE]
hipError_t launch_pinc_grad(hipStream_t st, const float* w, int B, const float* Z, const float* Y, const float* U4, const int* perm,
                            int K, int use_physics, float* part);
// fixed-order sum of the partials -> grad_out [PINC_NPARAMS], loss_out [3] = (mse, physics mean square, rollout), norm_out [1] (each
// optional); ad != nullptr: clip to ad->max_norm and take AdamW step number `step` (1-based) on w, m, v in place
hipError_t launch_pinc_reduce(hipStream_t st, int nparts, int stride, const float* part, int B, float* grad_out, float* loss_out,
                              float* norm_out, const PincAdam* ad, int64_t step, float* w, float* m, float* v);
// one map vehicle over N consecutive samples U [N][8] -> tau [N][6]; d_lag_io [8][3] in / out; d_phi = [Ad | Ad^window_scan_chunk()],
// d_lag [N][24], d_chunk [chunks][24]: the arrays of launch_window_lag_scan (nc = 8, P = 1)
hipError_t launch_thruster_stream(hipStream_t st, const DevParams& p, int64_t N, const double* U, const double* d_phi, double* d_lag,
                                  double* d_chunk, double* d_lag_io, double* tau);

}  // namespace brov
