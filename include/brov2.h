/*
 * brov2.h -- C ABI of libbrov2.so: MI355X (gfx950) batched BlueROV2 Fossen dynamics
 * rollouts and Koopman-EDMDc lift / Gram build.
 *
 * The reference (ViktorNfa/bluerov2_dynamics) is pure Python and has no FFI layer; its
 * boundary for this path is the Python object API that training scripts import.  Each
 * entry point below names the reference interface it stands behind (paths relative to the
 * reference checkout).  The Python classes in bluerov2_dynamics_amd/{fossen,Koopman}/ keep
 * the reference's names/signatures and call these functions through ctypes
 * (INTEGRATION.md shows the binding).
 *
 * Conventions
 *   - every array is IEEE fp64, C-contiguous; sizes are element counts, not bytes;
 *   - functions return BROV_OK (0) or a negative brov_status; brov_last_error(ctx) gives
 *     a message owned by the ctx.  Nothing aborts, NaN/inf propagate like in the reference;
 *   - a ctx is bound to one device, is not thread-safe, and launches on one HIP stream
 *     (brov_set_stream; default: the null stream);
 *   - "_dev" functions take DEVICE pointers and are asynchronous on the ctx stream;
 *     the others take HOST pointers, copy in/out and return when the result is on the host.
 *
 * Models (brov_model):
 *   BROV_THRUSTER_EULER  nx=12 [x y z phi theta psi u v w p q r], nu=8 thruster commands
 *                        in [-1,1], 8x3 thruster-lag state   (fossen/BlueROV2.py)
 *   BROV_WRENCH_EULER    nx=12, nu=6 body wrench, no lag       (fossen/BlueROV2_thrust.py)
 *   BROV_WRENCH_QUAT     nx=13 [x y z qw qx qy qz u v w p q r], nu=6; the quaternion is
 *                        re-normalised after every integrator step (fossen/BlueROV2_wrench.py,
 *                        training/train_tank_brov2_wrench_quat.py:258-263)
 */
#ifndef BROV2_H
#define BROV2_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BROV2_ABI_VERSION 1

#if defined(BROV2_BUILDING)
#define BROV_API __attribute__((visibility("default")))
#else
#define BROV_API
#endif

typedef struct brov_ctx brov_ctx;

typedef enum brov_status {
    BROV_OK = 0,
    BROV_ERR_ARG = -1,     /* bad argument (NULL, negative size, unknown enum) */
    BROV_ERR_HIP = -2,     /* a HIP runtime call failed (message has hipGetErrorString) */
    BROV_ERR_NOMEM = -3,   /* device or host allocation failed */
    BROV_ERR_NODEVICE = -4,/* no gfx950 device visible (no GPU at all, or a GPU of another architecture) */
    BROV_ERR_COMM = -5     /* RCCL missing or an RCCL call failed (brov_comm_last_error) */
} brov_status;

typedef enum brov_model {
    BROV_THRUSTER_EULER = 0, BROV_WRENCH_EULER = 1, BROV_WRENCH_QUAT = 2,
    /* learned double-integrator baseline of the comparison scripts (gains from brov_set_di_gains):
     * nx/nu = 12/8, 12/6, 13/6; rollouts and window errors only */
    BROV_DI_THRUSTER_EULER = 3, BROV_DI_WRENCH_EULER = 4, BROV_DI_WRENCH_QUAT = 5
} brov_model;
typedef enum brov_integrator { BROV_EULER = 0, BROV_RK4 = 1 } brov_integrator;
/* PER_CALL = the reference: the lag filters advance on every dynamics() call, i.e. 4x per RK4
 * step (training/train_tank_brov2_rk4.py:386-391 calling fossen/BlueROV2.py:258).
 * PER_STEP = lag advanced once per step, thrust frozen over the RK4 stages (not the reference). */
typedef enum brov_lag_mode { BROV_LAG_PER_CALL = 0, BROV_LAG_PER_STEP = 1 } brov_lag_mode;
/* BTU: U[B][T][nu], traj[B][T/stride+1][nx]  (what the reference's callers hold, row-major)
 * TUB: U[T][nu][B], traj[T/stride+1][nx][B]  (time-major struct-of-arrays, device native) */
/* TPB: as TUB with channel PAIRS interleaved -- U[T][ceil(nu/2)][B][2], traj[T/stride+1][ceil(nx/2)][B][2] (an odd
 *      channel count is padded with one unused element): 16-byte accesses per lane, the fastest rollout layout */
typedef enum brov_layout { BROV_LAYOUT_BTU = 0, BROV_LAYOUT_TUB = 1, BROV_LAYOUT_TPB = 2 } brov_layout;
typedef enum brov_dist { BROV_DIST_IID_UNIFORM = 0, BROV_DIST_AR1 = 1 } brov_dist;

/* Vehicle parameters; brov_default_params() fills the reference's values
 * (fossen/BlueROV2.py:79-140,172-232,245-257,476-480). Signs follow the reference's attributes. */
typedef struct brov_params {
    double rho, g, m, volume;
    double xb, yb, zb;          /* centre of buoyancy (CG at origin) */
    double Ix, Iy, Iz;
    double added_mass[6];       /* Xu_dot Yv_dot Zw_dot Kp_dot Mq_dot Nr_dot (negative) */
    double lin_damp[6];         /* Xu Yv Zw Kp Mq Nr (negative or -0.0) */
    double quad_damp[6];        /* Xu_abs ... Nr_abs (negative) */
    double current[3];          /* NED current speed, default 0 */
    double thr_r[8][3];         /* thruster positions (body) */
    double thr_dir[8][3];       /* thruster directions (body) */
    double thrust_poly[5];      /* F_cmd = c0 V + c1 V^3 + c2 V^5 + c3 V^7 + c4 V^9 */
    double lag_Ac[9], lag_Bc[3], lag_Cc[3]; /* continuous thruster lag (row-major) */
} brov_params;

/* ---- context ------------------------------------------------------------------------- */
BROV_API int brov_abi_version(void);
BROV_API int brov_create(int device_id, brov_ctx** out);
BROV_API void brov_destroy(brov_ctx* ctx);
BROV_API const char* brov_last_error(const brov_ctx* ctx);
/* 1 if a device whose hipDeviceProp_t.gcnArchName is `gcn_arch_name` can run this library ("gfx950[:features]"), else 0.
 * brov_create applies it to the selected device and returns BROV_ERR_NODEVICE otherwise.  Host only. */
BROV_API int brov_arch_is_supported(const char* gcn_arch_name);
BROV_API int brov_device_arch(const brov_ctx* ctx, char* buf, size_t cap);   /* gcnArchName of the ctx's device */
/* 1 if workgroups b and b+8 were seen to share an XCD when the ctx was created (the assumption behind the XCD-aware block
 * numbering of the Gram / propagation kernels; speed only), 0 if not, -1 if the probe could not run. */
BROV_API int brov_xcd_round_robin(const brov_ctx* ctx);
BROV_API int brov_set_stream(brov_ctx* ctx, void* hip_stream);     /* hipStream_t; NULL = null stream */
BROV_API int brov_sync(brov_ctx* ctx);                             /* hipStreamSynchronize(ctx stream) */
/* HIP-event timing of the kernels launched by the most recent call on this ctx
 * (sum over its launches, ms).  Enable first; reading waits for the stop event. */
BROV_API int brov_set_timing(brov_ctx* ctx, int enabled);
BROV_API int brov_last_kernel_ms(brov_ctx* ctx, float* ms);

/* ---- parameters  (replaces BlueROV2.__init__, fossen/BlueROV2.py:79-157) -------------- */
BROV_API void brov_default_params(brov_params* p);
BROV_API int brov_set_params(brov_ctx* ctx, const brov_params* p);
BROV_API int brov_get_params(const brov_ctx* ctx, brov_params* p);
/* Minv diagonal (6) and the 6x8 allocation matrix tau = T F  (fossen/BlueROV2.py:126,265-278).
 * Host only; p = NULL means the default parameters. */
BROV_API int brov_get_derived(const brov_params* p, double Minv6[6], double alloc6x8[48]);
/* ZOH discretisation of the thruster lag: replaces ThrusterLag._discretise
 * (fossen/BlueROV2.py:490-496 -> scipy.signal.cont2discrete(method="zoh")).  Host only. */
BROV_API int brov_discretise_lag(const brov_params* p, double dt, double Ad[9], double Bd[3]);

BROV_API int brov_model_nx(int model);
BROV_API int brov_model_nu(int model);

/* ---- device memory helpers (so that callers need no HIP/torch of their own) -----------
 * brov_free keeps blocks of up to 256 MB (1 GB in total per ctx) for the next brov_malloc of a similar size; brov_destroy releases them.
 * The copies are synchronous (done on return) and accept pageable host memory: between 64 KB and 16 MB they are staged through two
 * pinned blocks owned by the ctx instead of handing the caller's pages to the runtime. */
BROV_API int brov_malloc(brov_ctx* ctx, size_t bytes, void** dptr);
BROV_API int brov_free(brov_ctx* ctx, void* dptr);
BROV_API int brov_memcpy_h2d(brov_ctx* ctx, void* dst, const void* src, size_t bytes);
BROV_API int brov_memcpy_d2h(brov_ctx* ctx, void* dst, const void* src, size_t bytes);
/* device to device on the ctx stream, asynchronous like brov_memset (both ranges on the ctx's device; overlapping ranges:
 * BROV_ERR_ARG, nothing copied) */
BROV_API int brov_memcpy_d2d(brov_ctx* ctx, void* dst, const void* src, size_t bytes);
BROV_API int brov_memset(brov_ctx* ctx, void* dst, int value, size_t bytes);
/* Free and total bytes of the ctx's device (hipMemGetInfo): lets a caller without HIP / torch decide whether an optional buffer
 * (edmdc_lift_cache) fits. */
BROV_API int brov_mem_info(brov_ctx* ctx, size_t* free_bytes, size_t* total_bytes);
/* A list of host arrays into ONE device buffer -- what KoopmanEDMDc.fit_multi's np.vstack of its trajectory list becomes
 * (Koopman/koopmanEDMDc.py:125,140-142).  Bag b = bag_rows[b] rows of `cols` contiguous doubles at bag_ptrs[b]; it is written to
 * d_dst + dst_rows[b] * cols.  The destinations must ascend without overlap (holes are allowed; small ones are zero-filled, larger ones
 * left untouched).  Packed through two pinned staging blocks by a few host threads while the previous block is in flight; the data is
 * in place when the call returns. */
BROV_API int brov_upload_bags(brov_ctx* ctx, int64_t nbags, const double* const* bag_ptrs, const int64_t* bag_rows,
                              const int64_t* dst_rows, int cols, double* d_dst);

/* ---- Fossen RHS / rollouts ------------------------------------------------------------ */
/* Batched dynamics(): xdot[b] = f(x[b], u[b]).  Replaces BlueROV2.dynamics
 * (fossen/BlueROV2.py:357-400, BlueROV2_thrust.py:235-282, BlueROV2_wrench.py:322-367).
 * lag_io [B][8][3] is advanced one sample in place (thruster model; the reference's side
 * effect on self.thruster_lags); NULL = zero lag state, not returned. */
BROV_API int brov_rhs(brov_ctx* ctx, int model, int64_t B, const double* x, const double* u, double dt,
             double* lag_io, double* xdot);
/* Replaces BlueROV2.compute_thruster_forces (fossen/BlueROV2.py:265-278): tau [B][6]. */
BROV_API int brov_thruster_forces(brov_ctx* ctx, int64_t B, const double* u, double dt, double* lag_io, double* tau);

/* simulate_physics over a batch: training/train_tank_brov2_full_comparison.py:453-466 (Euler),
 * training/train_tank_brov2_rk4.py:375-396 (RK4), ..._wrench_quat.py:249-266 (quaternion).
 * x0 [B][nx]; U and traj per `layout`; lag_io [B][8][3] in/out or NULL (zero start);
 * traj holds every traj_stride-th state including x0 (T/stride+1 states) or is NULL;
 * xT [B][nx] (final state) or NULL. */
BROV_API int brov_rollout(brov_ctx* ctx, int model, int integrator, int lag_mode, int layout,
                 int64_t B, int64_t T, double dt, const double* x0, const double* U,
                 double* lag_io, double* traj, int64_t traj_stride, double* xT);
/* Gains of the double-integrator models: dv = u K_lin, dw = u K_ang with K_lin, K_ang [nu][3] row-major, nu = 8 or 6
 * (estimate_di_gains + simulate_double_integrator, training/train_tank_brov2_full_comparison.py:510-573,
 * RK4 form ..._rk4.py:461-525, wrench / quaternion forms ..._wrench_comp.py:293-341, ..._wrench_quat.py:324-372). */
BROV_API int brov_set_di_gains(brov_ctx* ctx, int nu, const double* K_lin, const double* K_ang);
/* How BROV_LAYOUT_BTU rollouts (stride 1 or no trajectory) move data: 0 = auto (LDS-staged tiles
 * for the memory-bound cases -- Euler, wrench models -- and lane-per-row accesses for the
 * instruction-bound thruster RK4 kernel; measured in DESIGN.md), 1 = always LDS-staged, 2 = never. */
BROV_API int brov_set_btu_staging(brov_ctx* ctx, int mode);
/* Which kernel runs the thruster-model rollouts: 0 = the two-wave kernel (thrust half and body half of a step on two waves that share
 * a SIMD; default), 1 = the whole step in one lane (the kernel of the wrench / double-integrator models; the independent second
 * implementation of the parity tests).  Same trajectories to rounding. */
BROV_API int brov_set_rollout_variant(brov_ctx* ctx, int variant);
BROV_API int brov_rollout_dev(brov_ctx* ctx, int model, int integrator, int lag_mode, int layout,
                     int64_t B, int64_t T, double dt, const double* d_x0, const double* d_U,
                     double* d_lag_io, double* d_traj, int64_t traj_stride, double* d_xT);

/* multistep_rmse_endpoint_physics: training/train_tank_brov2_full_comparison.py:469-487,
 * ..._rk4.py:399-417, ..._wrench_comp.py, ..._wrench_quat.py:279-297.
 * X [N][nx], U [N][nu]; windows k = 0..N-H-1 start at X[k], apply U[k..k+H-1], and are scored
 * against X[k+H].  carry_lag=1 is the reference: ONE vehicle object serves all windows, so the
 * thruster-lag state left by window k-1 is the initial lag state of window k.
 * se_total = sum_k |x_end - X[k+H]|^2 ; per_window [N-H] optional (NULL).
 * rmse = sqrt(se_total / ((N-H) * nx)). */
BROV_API int brov_window_endpoint_se(brov_ctx* ctx, int model, int integrator, int64_t N, int64_t H, double dt,
                            const double* X, const double* U, int carry_lag,
                            double* se_total, double* per_window);
BROV_API int brov_window_endpoint_se_dev(brov_ctx* ctx, int model, int integrator, int64_t N, int64_t H, double dt,
                                const double* d_X, const double* d_U, int carry_lag,
                                double* d_se_total, double* d_per_window /* [N-H], required */);

/* ---- parameter identification: the window evaluator over a population, finite-difference normal equations ----------
 * brov_window_endpoint_pop scores P parameter sets against one recording in one call: se[j] (and endpoints[j], the window end
 * states x_end, [P][N-H][nx], NULL = not wanted) are what brov_set_params(&params[j]) followed by brov_window_endpoint_se gives,
 * carried lag (carry_lag) and the four lag advances per RK4 step included.  The number of kernel launches does not depend on P
 * (the candidate is a grid dimension).  params is a HOST array in both forms; the ctx's own parameters (brov_set_params) are
 * neither read nor written.  Models: BROV_THRUSTER_EULER, BROV_WRENCH_EULER, BROV_WRENCH_QUAT (the double-integrator gains are
 * not brov_params: BROV_ERR_ARG); 1 <= P <= 65535.  N <= H: se[j] = 0, nothing else written.
 * rmse_j = sqrt(se[j] / ((N-H) * nx)).  se[j] is summed in a fixed order: the same bits from run to run. */
BROV_API int brov_window_endpoint_pop(brov_ctx* ctx, int model, int integrator, int64_t P, const brov_params* params /* [P], host */,
                             int64_t N, int64_t H, double dt, const double* X, const double* U, int carry_lag,
                             double* se /* [P] */, double* endpoints /* [P][N-H][nx], NULL ok */);
BROV_API int brov_window_endpoint_pop_dev(brov_ctx* ctx, int model, int integrator, int64_t P, const brov_params* params /* [P], host */,
                                 int64_t N, int64_t H, double dt, const double* d_X, const double* d_U, int carry_lag,
                                 double* d_se /* [P] */, double* d_endpoints /* [P][N-H][nx], NULL ok */);
/* The same over several recordings ("bags") that must not be joined: X [rows][nx] and U [rows][nu] hold the bags' rows one after the
 * other, row-aligned, and bag b is rows bag_offsets[b] .. bag_offsets[b+1]-1 (a HOST int64 array [nbags+1], bag_offsets[0] = 0,
 * non-decreasing, nbags >= 0: the contract of edmdc_gram_ragged).  Bag b of L_b rows has w_b = max(L_b - H, 0) windows; the windows
 * are numbered bag after bag, W = sum_b w_b.  Window k of bag b starts at row bag_offsets[b]+k, applies U rows ..+k .. ..+k+H-1 and is
 * scored against row bag_offsets[b]+k+H: no window reads a row of another bag (the last row of a bag's U is never read).  Empty
 * bags and bags of L_b <= H rows are allowed.  carry_lag=1 is a fresh vehicle per recording: the first window of every bag starts
 * from zero lag, and inside a bag window k starts from what window k-1 left.  The results are those of one
 * brov_window_endpoint_pop call per bag: se[j] = sum_b se_b[j], endpoints [P][W][nx] and per_window [P][W] the bags' arrays one
 * after the other; rmse_j = sqrt(se[j] / (W * nx)).  target [W][nx] (NULL = not wanted) receives the rows the windows are scored
 * against, X[row+H] in window order: the d_target of brov_fd_normal_eq_dev.  P = 0 with a target scores nothing and writes the
 * target alone (U is not read).  W = 0: se[j] = 0, nothing else written.  The number of kernel launches depends neither on nbags
 * nor on P; se[j] is summed in a fixed order.  Models and the range of P as in brov_window_endpoint_pop.  A bag list that breaks
 * the contract is refused on the host (BROV_ERR_ARG, brov_last_error names the rule) before anything is launched. */
BROV_API int brov_window_endpoint_pop_ragged(brov_ctx* ctx, int model, int integrator, int64_t P, const brov_params* params /* [P], host */,
                                    int64_t nbags, const int64_t* bag_offsets /* [nbags+1], host */, int64_t H, double dt,
                                    const double* X, const double* U, int carry_lag, double* se /* [P] */,
                                    double* endpoints /* [P][W][nx], NULL ok */, double* target /* [W][nx], NULL ok */);
BROV_API int brov_window_endpoint_pop_ragged_dev(brov_ctx* ctx, int model, int integrator, int64_t P, const brov_params* params /* [P], host */,
                                        int64_t nbags, const int64_t* bag_offsets /* [nbags+1], host */, int64_t H, double dt,
                                        const double* d_X, const double* d_U, int carry_lag, double* d_se /* [P] */,
                                        double* d_endpoints /* [P][W][nx], NULL ok */, double* d_target /* [W][nx], NULL ok */,
                                        double* d_per_window /* [P][W], NULL ok */);
/* brov_window_endpoint_se over the same bag list, on the ctx's own parameters: the P = 1 case of the kernels above, for all six
 * models (the double-integrator ones included, after brov_set_di_gains).  se_total = sum over the W windows of all bags;
 * per_window [W] optional in the host form, required in the _dev form.  W = 0: se_total = 0, nothing else written. */
BROV_API int brov_window_endpoint_se_ragged(brov_ctx* ctx, int model, int integrator, int64_t nbags,
                                   const int64_t* bag_offsets /* [nbags+1], host */, int64_t H, double dt, const double* X,
                                   const double* U, int carry_lag, double* se_total, double* per_window);
BROV_API int brov_window_endpoint_se_ragged_dev(brov_ctx* ctx, int model, int integrator, int64_t nbags,
                                       const int64_t* bag_offsets /* [nbags+1], host */, int64_t H, double dt, const double* d_X,
                                       const double* d_U, int carry_lag, double* d_se_total, double* d_per_window /* [W], required */);
/* Normal equations of a Gauss-Newton / Levenberg-Marquardt step from endpoints scored at base (row block 0) and at
 * base + delta_j e_j (row block j + 1), j = 0..m-1, 1 <= m <= 48, over W windows of nx coordinates:
 *     J[(k,i)][j] = w_i (E_{j+1}[k][i] - E_0[k][i]) / delta_j,    r[(k,i)] = w_i (E_0[k][i] - target[k][i]),
 *     JtJ = J^T J [m][m],  Jtr = J^T r [m].
 * d_endpoints [m+1][W][nx] and d_target [W][nx] (= X[H:]) are device arrays; delta [m] (finite, non-zero), weight [nx] (NULL = 1),
 * JtJ and Jtr are host arrays, valid on return.  Partial sums per block, added in index order, no atomics: the same bits from
 * run to run. */
BROV_API int brov_fd_normal_eq_dev(brov_ctx* ctx, int nx, int m, int64_t W, const double* d_endpoints, const double* d_target,
                          const double* delta_host, const double* weight_host, double* JtJ_host, double* Jtr_host);

/* ---- rollouts over a population of parameter sets, ensemble statistics ------------------------------------------------------
 * brov_rollout_pop is simulate_physics (training/train_tank_brov2_full_comparison.py:453-466, ..._rk4.py:375-396,
 * ..._wrench_quat.py:249-266) for P vehicles in one call: candidate j rolls B trajectories of T steps under params[j].  One
 * derivation pass on the host, one upload of the derived constants, one kernel launch, whatever P is (the candidate is a grid
 * dimension).  params is a HOST array in both forms; the ctx's own parameters (brov_set_params) are neither read nor written.
 * Layout BROV_LAYOUT_BTU only.  Inputs are shared by the candidates (inputs_per_candidate = 0: x0 [B][nx], U [B][T][nu], every
 * vehicle sees the same scenarios) or per candidate (inputs_per_candidate = 1: x0 [P][B][nx], U [P][B][T][nu]).  Outputs are always
 * per candidate and each may be NULL: traj [P][B][T/traj_stride+1][nx] (every traj_stride-th state including x0), xT [P][B][nx],
 * lag_io [P][B][8][3] in/out (thruster model; NULL = start from zero lag, no per-thruster bookkeeping).
 * The kernel always takes the general step (the one brov_rollout_dev takes for a vehicle with a current, xb / yb != 0, a dense
 * allocation matrix or a lag bank without observer form), so one kernel serves mixed populations.  Candidate j agrees with
 * brov_rollout_dev after brov_set_params(&params[j]) to rounding; it is not bit-equal to any of brov_rollout_dev's paths (the
 * specialised step, the two-wave kernel, the one-lane general kernel): those carry sin/cos of the attitude and the
 * acceleration-space lag from step to step, this kernel re-forms both from (x, lag_io) at every step so that a call can be resumed
 * exactly (last sentence below).
 * Models: BROV_THRUSTER_EULER, BROV_WRENCH_EULER, BROV_WRENCH_QUAT (the double-integrator gains are not brov_params:
 * BROV_ERR_ARG); both integrators and both lag modes; 0 <= P <= 65535, every candidate's mass matrix non-singular.  B = 0 or
 * P = 0: BROV_OK, nothing touched.  A call of T steps continued by a call from the returned xT and lag_io gives the bits of one
 * call over both spans. */
BROV_API int brov_rollout_pop(brov_ctx* ctx, int model, int integrator, int lag_mode, int64_t P, const brov_params* params /* [P], host */,
                     int inputs_per_candidate, int64_t B, int64_t T, double dt, const double* x0, const double* U,
                     double* lag_io, double* traj, int64_t traj_stride, double* xT);
BROV_API int brov_rollout_pop_dev(brov_ctx* ctx, int model, int integrator, int lag_mode, int64_t P, const brov_params* params /* [P], host */,
                         int inputs_per_candidate, int64_t B, int64_t T, double dt, const double* d_x0, const double* d_U,
                         double* d_lag_io, double* d_traj, int64_t traj_stride, double* d_xT);
/* Reduces a population of results to bands: d_vals [P][M] (for instance traj of brov_rollout_pop_dev, M = B rows nx) ->
 * d_out [4][M] = mean, sample standard deviation (divisor P - 1; 0 when P = 1), minimum, maximum over the P candidates.  Where any
 * candidate's value is not finite all four are NaN.  Summed in index order, no atomics: the same bits from run to run.  P >= 1. */
BROV_API int brov_ensemble_stats_dev(brov_ctx* ctx, int64_t P, int64_t M, const double* d_vals, double* d_out);

/* ---- closed-loop rollouts: a feedback law evaluated inside the rollout kernel -----------------------------------------------
 * brov_rollout_feedback is brov_rollout_pop with the control array replaced by a linear tracking law on the state, which never
 * leaves the kernel: candidate j rolls B trajectories of T steps under params[j], and at every step the command comes from the
 * state, a reference and the gains below.  One law serves the wrench models (nu = 6) and the thruster model (nu = 8).
 *
 * Ticks and hold.  The law is evaluated at the steps t = 0, hold, 2 hold, ... of a call (hold >= 1) and its command is held in
 * between (zero-order hold).  Under RK4 the command is constant over the four stages; the thruster lag advances per lag_mode
 * exactly as in brov_rollout_pop.
 * Tracking error e[12], from the state x at the start of the step and the reference row r, which has the layout of a state
 * (nx values):
 *     e[0:3]  = R(att)^T (r.p - x.p), the position error in the body frame, R the rotation matrix the model itself forms from x
 *               (the quaternion model normalises q for it, as its dynamics do);
 *     e[3:6]  = Euler models: r.att - x.att component-wise, wrapped to [-pi, pi] as d - 2 pi rint(d / (2 pi)) (round half to even:
 *               a difference of exactly an odd multiple of pi keeps the sign rint gives it);
 *               BROV_WRENCH_QUAT: q_e = conj(x.q) (x) r.q on the quaternions as stored, e = 2 s q_e.xyz with s = +1 when
 *               q_e.w >= 0 and -1 otherwise (the short way round);
 *     e[6:12] = r.nu - x.nu.
 * Command and integral state, at a tick:
 *     u = clip(u_ff[t] + K e + Ki z, u_min, u_max)            K [nu][12], Ki [nu][6], u_ff the feed-forward row of step t (NULL = 0)
 *     z <- clip(z + hold dt e[0:6], -z_max, z_max)            after the command is formed: the first tick uses the incoming z,
 *                                                             and anti-windup is the clamp.
 * Reference: ref_rows = 1 is a set-point (one row per trajectory), ref_rows = T uses row t at step t.
 * Metrics [4] per trajectory, accumulated at every step t = 0..T-1 on the state at the start of the step (the error is evaluated
 * at every step for this, whatever hold is): sum dt |e[0:3]|^2, sum dt |e[3:6]|^2, sum dt |u|^2 of the applied command, and the
 * number of steps at which at least one channel of the applied command equals its u_min or u_max.
 *
 * Arguments as brov_rollout_pop, except: u_ff [.][B][T][nu] is optional; fb is a HOST array of nfb records, nfb = 1 (one
 * controller for every vehicle: robustness) or nfb = P (candidate j under fb[j]: gain tuning); ref [.][B][ref_rows][nx];
 * inputs_per_candidate covers x0, u_ff and ref together (0: shared, leading dimension B; 1: leading dimensions [P][B]).  z_io
 * [P][B][6] in/out (NULL = start from zero, nothing returned).  Optional outputs u_applied [P][B][T][nu] and metrics [P][B][4].
 * Models, integrators, lag modes and the range of P are those of brov_rollout_pop (double-integrator models: BROV_ERR_ARG); B = 0
 * or P = 0: BROV_OK, nothing touched.  Refused on the host with BROV_ERR_ARG and a brov_last_error text naming the rule, before
 * anything is copied or launched: hold < 1, nfb not in {1, P}, ref_rows not in {1, T}, u_min > u_max (channels < nu), a negative
 * z_max, a NaN anywhere in fb, traj_stride < 1.  The ctx's own parameters are neither read nor written.
 * Deterministic (no atomics, every lane writes its own outputs): two calls give the same bits.  Resume: a call of T1 steps with
 * T1 a multiple of hold, continued by a call from the returned (xT, lag_io, z_io) with the remaining rows of u_ff / ref, gives the
 * bits of one call over both spans in traj, xT, lag_io, z_io and u_applied; the metrics of the two spans add up to those of the
 * one call to rounding only (the sums are split at T1). */
typedef struct brov_feedback {
    double K[8][12], Ki[8][6];      /* rows >= nu ignored */
    double u_min[8], u_max[8];      /* u_min <= u_max, may be +-inf */
    double z_max[6];                /* >= 0, may be inf */
    int32_t hold, _pad;             /* >= 1 */
} brov_feedback;
BROV_API int brov_rollout_feedback(brov_ctx* ctx, int model, int integrator, int lag_mode, int64_t P, const brov_params* params /* [P], host */,
                          int64_t nfb, const brov_feedback* fb /* [nfb], host */, int inputs_per_candidate, int64_t B, int64_t T,
                          double dt, const double* x0, const double* u_ff, const double* ref, int64_t ref_rows, double* lag_io,
                          double* z_io, double* traj, int64_t traj_stride, double* xT, double* u_applied, double* metrics);
BROV_API int brov_rollout_feedback_dev(brov_ctx* ctx, int model, int integrator, int lag_mode, int64_t P, const brov_params* params /* [P], host */,
                              int64_t nfb, const brov_feedback* fb /* [nfb], host */, int inputs_per_candidate, int64_t B, int64_t T,
                              double dt, const double* d_x0, const double* d_u_ff, const double* d_ref, int64_t ref_rows,
                              double* d_lag_io, double* d_z_io, double* d_traj, int64_t traj_stride, double* d_xT,
                              double* d_u_applied, double* d_metrics);

/* ---- state estimation: an unscented Kalman filter on the Fossen model ---------------------------------------------------------
 * brov_ukf_filter turns noisy, gappy recordings of the state into estimates with error bars, for P vehicles at once: candidate j
 * (params[j], a HOST array as in brov_rollout_pop) filters B recordings of T rows each, in one launch whatever P, B and T are.
 * info[0], the innovation log-likelihood, says which candidate explains a recording best.
 * Models BROV_THRUSTER_EULER and BROV_WRENCH_EULER (n = 12 states, 2 n + 1 = 25 sigma points); both integrators and both lag
 * modes.  The quaternion model (its mean lives on a manifold: brov_ukf_filter_quat below is its filter) and the double-integrator
 * models: BROV_ERR_ARG.  The thruster lag
 * depends on the commands only, never on the state, so all sigma points share one lag bank and the filter's state stays at 12.
 * The measurements are components of the state and R is diagonal, so the measurement update is a sequence of scalar Kalman
 * updates: exact, no unscented transform, no matrix inverse, and per-component dropouts come for free.
 *
 * Inputs, shared by the candidates: x0 [B][12]; P0 [B][12][12], of which the lower triangle is read and taken as symmetric;
 * U [B][T][nu]; Y [B][T][12], the measured state rows, where a NaN means "this component was not measured at this row";
 * lag_io [P][B][8][3] optional, in/out (thruster model; NULL = start from zero lag, nothing returned).
 * Record brov_ukf: q[12] the per-step process variances (>= 0, finite), r[12] the measurement variances (>= 0; +inf = never
 * measured), alpha, beta, kappa.  ukf is a HOST array of nrec records: nrec = 1 (one noise model for all candidates) or nrec = P
 * (candidate j under ukf[j]).  Derived, with n = 12:
 *     lambda = alpha^2 (n + kappa) - n,  c = sqrt(n + lambda),
 *     Wm_0 = lambda / (n + lambda),  Wc_0 = Wm_0 + 1 - alpha^2 + beta,  W_i = 1 / (2 (n + lambda))  for i = 1 .. 2 n.
 * A small alpha makes the centre weight huge (alpha = 1e-3: Wm_0 ~ -1.2e7) and costs digits in any arithmetic: in fp64 against
 * long double the filtered states then differ by ~2e-10 instead of ~1e-15.  That is a property of the method, not of this kernel;
 * alpha in [0.5, 1] is the tested range.
 *
 * For t = 0 .. T-1, starting from (x, P) = (x0, P0), which is the estimate of row 0 BEFORE its measurement:
 *   1. Update with row t.  For i = 0 .. 11 in this order, skipped when Y[t][i] is NaN or r[i] = +inf:
 *          v = Y[t][i] - x[i]; for i in {3, 4, 5} wrapped as d - 2 pi rint(d / (2 pi)), the rule of brov_rollout_feedback
 *          s = P[i][i] + r[i],  k = P[:, i] / s,  x += k v,  P[a][b] -= k[a] k[b] s for all a, b
 *          l -= (ln(2 pi s) + v^2 / s) / 2;  the normalised innovation is v / sqrt(s).
 *      The same expression serves both triangles, so P stays bit-symmetric; a later component sees the x and P the earlier ones
 *      left.  Outputs of row t: the filtered mean xf[t], pstd[t][i] = sqrt(P[i][i]), innov[t][i] (NaN where skipped).
 *   2. Predict with U[t].  P = L L^T (lower Cholesky); chi_0 = x, chi_i = x + c L[:, i-1], chi_{i+n} = x - c L[:, i-1] (i = 1 .. n).
 *      Every chi advances one step through the general step of brov_rollout_pop with the same lag bank, which advances once, exactly
 *      as that kernel advances it.  d_i = chi_i' - chi_0' with components 3 .. 5 wrapped;  m = sum_{i>=1} W_i d_i;  x = chi_0' + m
 *      (the attitude of x is not wrapped: it stays continuous);  e_i = d_i - m, e_0 = -m;
 *      P = Wc_0 e_0 e_0^T + sum_{i>=1} W_i e_i e_i^T + diag(q), every sum in index order.
 * After T steps (xT, PT) is the estimate of row T before its measurement, so a call continued from (xT, PT, lag_io) with the
 * remaining rows gives the bits of the unbroken call in every per-row output, in xT, PT and lag_io; l adds up to rounding.
 *
 * Outputs, per candidate, each may be NULL: xf, pstd, innov [P][B][T][12]; xT [P][B][12]; PT [P][B][12][12] (full, symmetric);
 * info [P][B][4] = l, the number of scalar updates applied, the first failed step (-1: none), the smallest Cholesky pivot
 * L[j][j] seen.
 * Failure is a numerical condition of one (candidate, recording), handled in the kernel: s <= 0 or not finite in stage 1 of row
 * t, a pivot argument <= 0 or not finite in stage 2, or a non-finite predicted mean.  The filter stops there for that problem
 * only: per-row outputs after the failing stage are NaN (stage 1: row t and later; stage 2: row t is kept, its update was
 * complete), xT and PT are NaN, info = (-inf, updates so far, t, smallest pivot so far), lag_io is left as it came.  The call
 * returns BROV_OK and no other problem is touched.
 * Refused on the host with BROV_ERR_ARG and a brov_last_error text naming the rule, before anything is copied or launched: a
 * model other than the two above, nrec not in {1, P}, alpha not finite or <= 0, n + lambda <= 0 or not finite, a negative or NaN
 * q or r, an infinite q, T < 1, P > 65535, a NULL params, ukf, x0, P0, U or Y, dt not finite and > 0, a singular mass matrix.
 * B = 0 or P = 0: BROV_OK, nothing touched.  The ctx's own parameters are neither read nor written.
 * Deterministic (no atomics, fixed summation orders): two calls give the same bits. */
typedef struct brov_ukf {
    double q[12];                   /* per-step process variance, >= 0 */
    double r[12];                   /* measurement variance, >= 0; +inf: never measured */
    double alpha, beta, kappa;      /* alpha > 0 and 12 + lambda > 0 */
} brov_ukf;
BROV_API int brov_ukf_filter(brov_ctx* ctx, int model, int integrator, int lag_mode, int64_t P, const brov_params* params /* [P], host */,
                    int64_t nrec, const brov_ukf* ukf /* [nrec], host */, int64_t B, int64_t T, double dt, const double* x0,
                    const double* P0, const double* U, const double* Y, double* lag_io, double* xf, double* pstd, double* innov,
                    double* xT, double* PT, double* info);
BROV_API int brov_ukf_filter_dev(brov_ctx* ctx, int model, int integrator, int lag_mode, int64_t P, const brov_params* params /* [P], host */,
                        int64_t nrec, const brov_ukf* ukf /* [nrec], host */, int64_t B, int64_t T, double dt, const double* d_x0,
                        const double* d_P0, const double* d_U, const double* d_Y, double* d_lag_io, double* d_xf, double* d_pstd,
                        double* d_innov, double* d_xT, double* d_PT, double* d_info);

/* ---- the filter on the quaternion model: a multiplicative UKF ------------------------------------------------------------------
 * brov_ukf_filter_quat is brov_ukf_filter for BROV_WRENCH_QUAT, the vehicle that flies through pitch = +-90 degrees: candidate j
 * filters B recordings of T rows, one launch.  Its arguments are brov_ukf_filter's without model, lag_mode and lag_io (this is the
 * wrench model).
 *
 * State and error state.  The state is x[13] = p[3], q[4] (w first, Hamilton product, as everywhere in the library), nu[6].  The
 * error state is delta[12] = dp[3], g[3], dnu[6].  P, q[12] and r[12] live in the error state; the record is brov_ukf, unchanged,
 * with n = 12 in lambda, c, Wc_0 and W_i.  The attitude chart is twice the Gibbs vector, applied on the right, i.e. in the body
 * frame, the side that brov_rollout_feedback's conj(q) (x) q_ref uses:
 *     dq(g) = (1, g / 2) / sqrt(1 + |g|^2 / 4)
 *     x [+] delta = (p + dp, q (x) dq(g), nu + dnu)
 *     a [-] b = (p_a - p_b, 2 e_v / e_w, nu_a - nu_b)  with e = conj(q_b) (x) q_a
 * The chart has no branch.  It is invariant to the sign and the norm of either quaternion, so a measured quaternion need not be
 * unit.  It leaves the finite numbers only at exactly half a turn, where e_w = 0.
 *
 * Inputs, shared by the candidates: x0 [B][13]; P0 [B][12][12] (lower triangle read); U [B][T][6]; Y [B][T][13].  The position and
 * velocity entries of Y are as in brov_ukf_filter: NaN means not measured.  The attitude of row t is measured only when none of
 * Y[t][3..6] is NaN.  r[3..5] are the variances of the attitude measurement in chart units, which is rad^2 at small angles.
 *
 * For t = 0 .. T-1, starting from (x, P) = (x0, P0):
 *   1. Update with row t.
 *      a. Form z[12] once, from x as the row found it: z[0..2] = Y[t][0..2] - p;  z[3..5] = 2 e_v / e_w with
 *         e = conj(q) (x) q_y;  z[6..11] = Y[t][7..12] - nu.
 *      b. If the attitude is measured and a z[3..5] is not finite, stage 1 of row t fails before any update of the row is applied
 *         (q_y = 0, or a measurement half a turn away).
 *      c. Start with d = 0.  For i = 0 .. 11 in order, skipping where z[i] is NaN (not measured) or r[i] = +inf:
 *             v = z[i] - d[i];  s = P[i][i] + r[i] (s <= 0 or not finite fails stage 1 as in brov_ukf_filter);  k = P[:, i] / s;
 *             d += k v;  P[a][b] -= k[a] k[b] s, the same expression for both triangles;
 *             l -= (ln(2 pi s) + v^2 / s) / 2;  innov[t][i] = v / sqrt(s).
 *      d. x = x [+] d.
 *      e. The outputs of the row: xf[t][13], pstd[t][12] and innov[t][12], NaN where skipped.
 *      For position and velocity this is brov_ukf_filter's update exactly.  For the attitude it is the multiplicative update with
 *      one reset per row.
 *   2. Predict with U[t].  P = L L^T with brov_ukf_filter's Cholesky and pivot rule;  chi_0 = x, chi_i = x [+] (c L[:, i-1]),
 *      chi_{i+12} = x [+] (-c L[:, i-1]).  Every chi advances one step through the general step of brov_rollout_pop for
 *      BROV_WRENCH_QUAT, which normalises q.  d_i = chi_i' [-] chi_0';  m = sum_{i>=1} W_i d_i;  x = chi_0' [+] m;
 *      P = Wc_0 m m^T + sum_{i>=1} W_i (d_i - m)(d_i - m)^T + diag(q).  Every sum runs in index order.  A non-finite entry of m or
 *      x fails stage 2, as the non-finite predicted mean does in brov_ukf_filter.
 * Neither is derived here: the prediction is not re-centred at the new mean (it is the usual first-order USQUE form), and P is not
 * transported between the tangent spaces at a reset.
 *
 * Outputs, per candidate, each may be NULL: xf [P][B][T][13]; pstd, innov [P][B][T][12]; xT [P][B][13]; PT [P][B][12][12],
 * bit-symmetric; info [P][B][4] as brov_ukf_filter.
 * Unchanged from brov_ukf_filter: the failure handling (the problem stops alone, NaN rows, info), the continuation property (a call
 * resumed from (xT, PT) gives the bits of the unbroken call), determinism, and every host-side refusal that applies, with the same
 * words.  x0's quaternion is used as it comes: negating it negates the quaternion of xf and xT and changes no other bit.
 * Its smoother is brov_ukf_smooth_quat further down (with brov_ukf_filter_tape_quat_dev and brov_ukf_rts_quat_dev).  Not covered:
 * brov_ukf_filter, brov_ukf_smooth, EM and output feedback keep refusing the quaternion model. */
BROV_API int brov_ukf_filter_quat(brov_ctx* ctx, int integrator, int64_t P, const brov_params* params /* [P], host */, int64_t nrec,
                         const brov_ukf* ukf /* [nrec], host */, int64_t B, int64_t T, double dt, const double* x0, const double* P0,
                         const double* U, const double* Y, double* xf, double* pstd, double* innov, double* xT, double* PT, double* info);
BROV_API int brov_ukf_filter_quat_dev(brov_ctx* ctx, int integrator, int64_t P, const brov_params* params /* [P], host */, int64_t nrec,
                             const brov_ukf* ukf /* [nrec], host */, int64_t B, int64_t T, double dt, const double* d_x0,
                             const double* d_P0, const double* d_U, const double* d_Y, double* d_xf, double* d_pstd, double* d_innov,
                             double* d_xT, double* d_PT, double* d_info);

/* ---- state estimation after the fact: the unscented Rauch-Tung-Striebel smoother over the filter ------------------------------
 * The filter estimates row t from rows 0 .. t.  For a recording that is complete the smoothed estimate E[x_t | all rows] is the
 * better one: smaller errors, honest error bars in the first rows, better values of a component that is never measured.  It is a
 * backward pass over what the forward pass leaves on a tape.
 *
 * Forward pass with a tape (brov_ukf_filter_tape_dev).  The filter is the law above, unchanged, bit for bit in every output and in
 * lag_io.  Step t (update with row t, then predict with U[t]) also records what the backward pass needs for the transition
 * t -> t + 1: tape [P][B][T][312], a record of 312 doubles for both models, triangles packed row by row (entry e = a (a + 1) / 2 + b
 * holds [a][b], b <= a):
 *       0 ..  77   Pf_t, the covariance after the update of row t, lower triangle
 *      78 ..  89   xp_{t+1}, the predicted mean (the x that stage 2 leaves)
 *      90 .. 167   Pp_{t+1}, the predicted covariance including diag(q), lower triangle
 *     168 .. 311   C_{t+1} [12][12] row-major, C[a][b] = cov(x_t[a], x_{t+1}[b])
 * In the notation of stage 2, C_{t+1} = sum_{i>=1} W_i (chi_i - x)(d_i - m)^T; chi_i - x = +- c L[:, i-1] and the m terms cancel, so
 *     C[a][b] = sum_{j=0..11} L[a][j] ((c W_i) (d_{j+1}[b] - d_{j+13}[b])),  summed in index order.
 * nrows [P][B], stored as doubles like info, is the number of rows whose update completed: T for a filter that did not fail, t for
 * a failure in stage 1 of row t, t + 1 for a failure in stage 2 of row t.  Of a transition that did not complete, xp, Pp and C are
 * NaN, and so are whole records of rows whose update did not complete; Pf_t is there whenever the update of row t was complete.
 * d_tape and d_nrows go together; with both NULL the call is brov_ukf_filter_dev.
 *
 * Backward pass (brov_ukf_rts_dev), per (candidate, recording), with n = nrows (clamped to 0 .. T, so -inf counts as 0 and +inf as
 * T; then the fraction is dropped; NaN counts as 0).  n = 0: every output of the
 * problem is NaN, sinfo included.  Otherwise it starts from (xs, Ps)_{n-1} = (xf, Pf)_{n-1}; if n = T and a terminal pair
 * (xs_T [P][B][12], Ps_T [P][B][12][12], lower triangle read) is given -- the smoothed estimate of row T from a later span -- it
 * starts from that pair and takes the transition T-1 -> T first.  Then for t = n-2 .. 0 (with a terminal pair from t = T-1):
 *     Pp_{t+1} = Lp Lp^T, the Cholesky factorisation and the pivot rule of the filter's stage 2;
 *     G = C_{t+1} Pp_{t+1}^-1 by two triangular solves per row of C (w Lp^T = C[a][:] forwards, G[a][:] Lp = w backwards), no
 *         explicit inverse;
 *     xs_t = xf_t + G (xs_{t+1} - xp_{t+1}).  This difference is NOT wrapped: xf, xp and xs live on the filter's continuous
 *         attitude branch (stage 2 never wraps the mean), so a yaw that has turned through pi needs nothing here;
 *     Ps_t = Pf_t + G (Ps_{t+1} - Pp_{t+1}) G^T, one expression for both triangles: Ps is bit-symmetric.
 * Outputs, per candidate, each may be NULL: xs, pstd_s [P][B][T][12] (pstd_s = sqrt of the diagonal of Ps); Ps [P][B][T][12][12],
 * full; Ps0 [P][B][12][12] = Ps of row 0, which with xs[0] is the terminal pair for an earlier span; sinfo [P][B][2] = the first
 * failed transition (-1: none), the smallest pivot Lp[j][j] of any factorisation (+inf when there was none).  Rows >= n are NaN.
 * Row n-1 (T-1 without a terminal pair) carries the bits of the filter: xs = xf, pstd_s = pstd.
 * Failure of transition t is a pivot argument <= 0 or not finite: xs, pstd_s and Ps of rows <= t are NaN, rows > t stay valid, Ps0
 * is NaN, no other problem is touched, and the call returns BROV_OK.
 * Splitting in time: filter span 1, then span 2 from (xT, PT, lag_io); smooth span 2; smooth span 1 with span 2's (xs[0], Ps0) as
 * its terminal pair: the bits of the unbroken call in xs, pstd_s and Ps.
 * Refused with BROV_ERR_ARG: negative sizes, P > 65535, T < 1, a NULL d_xf, d_tape or d_nrows, one terminal pointer without the
 * other.  P = 0 or B = 0: BROV_OK, nothing touched.
 *
 * brov_ukf_smooth[_dev] is both passes: the inputs of brov_ukf_filter, the filter's outputs and the smoother's.  The tape lives in a
 * buffer the ctx owns, and the tape itself never exceeds tape_bytes (0: the default of 2 GiB): the recordings are processed in
 * chunks, one filter launch and one backward launch per chunk, and a chunk is a whole number of blocks of 4 recordings.  Chunking
 * changes no bit.  The buffer holds the chunk's tape, its nrows (8 bytes per problem) and up to 512 bytes of alignment, so it is
 * that much larger than the tape.  It is allocated once every refusal below has passed, and the ctx keeps it for the next call: a
 * call that needs more, or less than half of what is held, frees it and allocates its own size, so that one call with a large
 * tape_bytes does not bind that memory for the life of the ctx.  brov_destroy frees it.
 * Refused on the host, before anything is copied, allocated or launched, with a text that names the function called: everything
 * brov_ukf_filter refuses, a negative tape_bytes, and a tape_bytes smaller than one block of recordings (P * 4 * T * 2496 bytes).
 * Deterministic (no atomics, fixed summation orders): two calls give the same bits.
 * Still missing: full Q and R; for the quaternion model (brov_ukf_smooth_quat below is its smoother) the EM fit and output feedback.
 *
 * ---- fitting q and r: the sufficient statistics of expectation-maximisation (EM) ------------------------------------------------
 * Every call above takes a record whose q[12] and r[12] are guesses.  brov_ukf_rts_em_dev and brov_ukf_smooth_em[_dev] are the
 * backward pass and the smooth calls, unchanged bit for bit in every output they share with them, which also sum what one EM
 * iteration needs.  Model: x_{t+1} = f(x_t, u_t) + w, w ~ N(0, Q), Q = diag(q); Y_t[i] = x_t[i] + v, v ~ N(0, r[i]).  The
 * filter predicts Pp = (sigma-point covariance) + Q.  Taking the sigma-point covariance as independent of w, conditioning on all
 * rows Y gives for the transition t -> t + 1
 *     E[w w^T | Y] = Q + Q Pp^-1 (Ps_{t+1} - Pp_{t+1} + d d^T) Pp^-1 Q,   d = xs_{t+1} - xp_{t+1},
 * in which everything is local to the transition.  For a linear model this IS the Shumway-Stoffer expression with the lag-one
 * smoothed covariance Ps_{t+1} G_t^T substituted, so no lag-one covariance has to be formed or stored (tests/test_ukf_em_cpu.py
 * checks the identity on a linear-Gaussian model to 1e-12).  Q is diagonal, so only the diagonal is needed.
 * Per (candidate, recording), with n = nrows and the walk of brov_ukf_rts_dev (terminal pair included), in the order of the
 * backward pass, last row first, with M = Ps_{t+1} - Pp_{t+1} and d as that pass has them:
 *     Sq[i]  the sum over every completed transition t of  q_i + q_i^2 (u^T M u + (u . d)^2),  where u solves Lp Lp^T u = e_i by
 *            the forward and the backward substitution of a gain row; the inner sums run in index order;
 *     nq     the number of transitions summed: n - 1, or n with a terminal pair;
 *     Sr[i]  the sum of  v^2 + Ps_t[i][i],  v = Y[t][i] - xs_t[i] (for i in {3, 4, 5} wrapped by the filter's rule), over the rows
 *            t < n where Y[t][i] is not NaN and r_i is finite; row n-1 without a terminal pair uses (xf, Pf)_{n-1}, as the
 *            smoother's outputs do;
 *     nr[i]  the number of terms of Sr[i].
 * Output em [P][B][37] = Sq[12] | Sr[12] | nr[12] | nq, the counts stored as doubles like info.  q_i = 0 gives Sq[i] = 0.0
 * exactly: EM cannot leave a zero, so a component fixed at q_i = 0 stays there.  n = 0, or a failed backward transition: 37 NaN
 * for that problem alone.  Y [B][T][12] is indexed by the recording and shared by the candidates; q and r come from the record of
 * candidate j (nrec = 1 or P).  Spans split in time add: the em of span 2 (no terminal pair) plus the em of span 1 (with span 2's
 * pair) equals that of the unbroken call up to rounding.  Deterministic: per-lane accumulators, no atomics.
 * The M-step is the host's (fossen/estimate.py: em_update), per candidate, pooled over its recordings whose filter and backward
 * pass both completed:  q_i <- max(sum Sq_i / sum nq, q_floor);  r_i <- max(sum Sr_i / sum nr_i, r_floor) where sum nr_i > 0,
 * otherwise r_i stays (+inf stays +inf).  x0 and P0 are not re-estimated.
 * brov_ukf_rts_em_dev: the arguments of brov_ukf_rts_dev, then nrec, ukf [nrec] (host), d_Y and d_em.  brov_ukf_smooth_em[_dev]:
 * the arguments of brov_ukf_smooth[_dev], then em; they run through the same chunks.  Every per-row output may be NULL: an EM
 * iteration asks for info, sinfo and em and then stores no rows.
 * Refused with BROV_ERR_ARG and a text naming the function, before any copy or launch: everything the plain calls refuse; a NULL
 * d_Y, ukf or em; nrec not in {1, P}; a negative, NaN or infinite q; a negative or NaN r.  P = 0 or B = 0: BROV_OK. */
BROV_API int brov_ukf_filter_tape_dev(brov_ctx* ctx, int model, int integrator, int lag_mode, int64_t P, const brov_params* params /* [P], host */,
                             int64_t nrec, const brov_ukf* ukf /* [nrec], host */, int64_t B, int64_t T, double dt, const double* d_x0,
                             const double* d_P0, const double* d_U, const double* d_Y, double* d_lag_io, double* d_xf, double* d_pstd,
                             double* d_innov, double* d_xT, double* d_PT, double* d_info, double* d_tape, double* d_nrows);
BROV_API int brov_ukf_rts_dev(brov_ctx* ctx, int64_t P, int64_t B, int64_t T, const double* d_xf, const double* d_tape, const double* d_nrows,
                     const double* d_xs_T, const double* d_Ps_T, double* d_xs, double* d_pstd_s, double* d_Ps, double* d_Ps0,
                     double* d_sinfo);
BROV_API int brov_ukf_smooth(brov_ctx* ctx, int model, int integrator, int lag_mode, int64_t P, const brov_params* params /* [P], host */,
                    int64_t nrec, const brov_ukf* ukf /* [nrec], host */, int64_t B, int64_t T, double dt, const double* x0,
                    const double* P0, const double* U, const double* Y, double* lag_io, double* xf, double* pstd, double* innov,
                    double* xT, double* PT, double* info, double* xs, double* pstd_s, double* Ps, double* Ps0, double* sinfo,
                    int64_t tape_bytes);
BROV_API int brov_ukf_smooth_dev(brov_ctx* ctx, int model, int integrator, int lag_mode, int64_t P, const brov_params* params /* [P], host */,
                        int64_t nrec, const brov_ukf* ukf /* [nrec], host */, int64_t B, int64_t T, double dt, const double* d_x0,
                        const double* d_P0, const double* d_U, const double* d_Y, double* d_lag_io, double* d_xf, double* d_pstd,
                        double* d_innov, double* d_xT, double* d_PT, double* d_info, double* d_xs, double* d_pstd_s, double* d_Ps,
                        double* d_Ps0, double* d_sinfo, int64_t tape_bytes);
BROV_API int brov_ukf_rts_em_dev(brov_ctx* ctx, int64_t P, int64_t B, int64_t T, const double* d_xf, const double* d_tape, const double* d_nrows,
                        const double* d_xs_T, const double* d_Ps_T, double* d_xs, double* d_pstd_s, double* d_Ps, double* d_Ps0,
                        double* d_sinfo, int64_t nrec, const brov_ukf* ukf /* [nrec], host */, const double* d_Y, double* d_em);
BROV_API int brov_ukf_smooth_em(brov_ctx* ctx, int model, int integrator, int lag_mode, int64_t P, const brov_params* params /* [P], host */,
                       int64_t nrec, const brov_ukf* ukf /* [nrec], host */, int64_t B, int64_t T, double dt, const double* x0,
                       const double* P0, const double* U, const double* Y, double* lag_io, double* xf, double* pstd, double* innov,
                       double* xT, double* PT, double* info, double* xs, double* pstd_s, double* Ps, double* Ps0, double* sinfo,
                       int64_t tape_bytes, double* em);
BROV_API int brov_ukf_smooth_em_dev(brov_ctx* ctx, int model, int integrator, int lag_mode, int64_t P, const brov_params* params /* [P], host */,
                           int64_t nrec, const brov_ukf* ukf /* [nrec], host */, int64_t B, int64_t T, double dt, const double* d_x0,
                           const double* d_P0, const double* d_U, const double* d_Y, double* d_lag_io, double* d_xf, double* d_pstd,
                           double* d_innov, double* d_xT, double* d_PT, double* d_info, double* d_xs, double* d_pstd_s, double* d_Ps,
                           double* d_Ps0, double* d_sinfo, int64_t tape_bytes, double* d_em);

/* ---- the smoother of the quaternion model ---------------------------------------------------------------------------------------
 * Notation as in brov_ukf_filter_quat: the state is 13 wide, the error state 12 wide, [+] and [-] are that filter's chart.  The
 * smoother is the first-order form, consistent with the filter it runs over: NO covariance is transported between the tangent
 * spaces at xf_t, xp_{t+1} and xs_{t+1}, as the filter transports none at a reset.
 *
 * Tape.  brov_ukf_filter_tape_quat_dev is brov_ukf_filter_quat_dev plus d_tape and d_nrows, given together or not at all; with both
 * NULL it is the plain call.  Every output of the plain call keeps its bits.  tape [P][B][T][313], a record of 313 doubles (2 504
 * bytes), triangles packed as in the tape above:
 *       0 ..  77   Pf_t, the covariance after the update of row t (in the error state at xf_t), lower triangle
 *      78 ..  90   xp_{t+1}, the 13-wide predicted mean chi_0' [+] m
 *      91 .. 168   Pp_{t+1}, the predicted covariance including diag(q), lower triangle
 *     169 .. 312   C_{t+1} [12][12] row-major
 * C_{t+1} = sum_{i>=1} W_i (chi_i [-] x)(d_i - m)^T.  chi_i [-] x = +- c L[:, i-1] by construction, so
 *     C[a][b] = sum_{j=0..11} L[a][j] ((c W_i) (d_{j+1}[b] - d_{j+13}[b])),  summed in index order:
 * the expression of the tape above on the quaternion filter's d.  nrows and the NaN rules for transitions that did not complete are
 * those of brov_ukf_filter_tape_dev.
 *
 * Backward pass.  brov_ukf_rts_quat_dev takes the arguments of brov_ukf_rts_dev; d_xf, d_xs and d_xs_T are 13 wide and the tape 313.
 * With n as there, it starts from (xs, Ps)_{n-1} = (xf, Pf)_{n-1}, or, with n = T and a terminal pair (xs_T [P][B][13], Ps_T
 * [P][B][12][12], lower triangle read), from that pair.  Per transition t:
 *     Pp_{t+1} = Lp Lp^T, the filter's Cholesky factorisation and pivot rule;
 *     G = C_{t+1} Pp_{t+1}^-1 by the two substitutions per row of C;
 *     delta = xs_{t+1} [-] xp_{t+1}, the attitude part through the chart, so it is blind to the sign and the norm of either
 *         quaternion.  A delta that is not finite (half a turn between the two, or a zero quaternion) fails transition t exactly
 *         like a bad pivot;
 *     xs_t = xf_t [+] (G delta): the smoothed quaternion keeps the sign and the norm of xf_t;
 *     Ps_t = Pf_t + G (Ps_{t+1} - Pp_{t+1}) G^T, one expression for both triangles: Ps is bit-symmetric.
 * Outputs, each may be NULL: xs [P][B][T][13]; pstd_s [P][B][T][12]; Ps [P][B][T][12][12]; Ps0 [P][B][12][12]; sinfo [P][B][2].  As in
 * brov_ukf_rts_dev: rows >= n are NaN and n = 0 leaves every output of the problem NaN, sinfo included; row n-1 (T-1 without a
 * terminal pair) carries the bits of the filter, xs = xf and pstd_s = pstd; a failed transition t leaves xs, pstd_s and Ps of rows
 * <= t and Ps0 NaN, rows > t valid and every other problem untouched, and the call returns BROV_OK; spans split in time chain
 * through (xT, PT) forwards and (xs[0], Ps0) backwards and give the bits of the unbroken call; the refusals are the same.
 * Negating x0's quaternion negates the quaternion of every xf and xs bit for bit and changes no other output; negating or scaling the
 * quaternion of xs_T changes no bit.
 *
 * brov_ukf_smooth_quat[_dev] is both passes: the inputs of brov_ukf_filter_quat, the filter's outputs, the smoother's outputs and
 * tape_bytes.  Chunking, the ctx-owned tape buffer (the one brov_ukf_smooth uses) and its keep / free rule are brov_ukf_smooth's;
 * refused is what brov_ukf_filter_quat refuses, a negative tape_bytes, and a tape_bytes smaller than one block of recordings
 * (P * 4 * T * 2504 bytes), before anything is copied, allocated or launched, with a text that names the function called. */
BROV_API int brov_ukf_filter_tape_quat_dev(brov_ctx* ctx, int integrator, int64_t P, const brov_params* params /* [P], host */, int64_t nrec,
                                  const brov_ukf* ukf /* [nrec], host */, int64_t B, int64_t T, double dt, const double* d_x0,
                                  const double* d_P0, const double* d_U, const double* d_Y, double* d_xf, double* d_pstd, double* d_innov,
                                  double* d_xT, double* d_PT, double* d_info, double* d_tape, double* d_nrows);
BROV_API int brov_ukf_rts_quat_dev(brov_ctx* ctx, int64_t P, int64_t B, int64_t T, const double* d_xf, const double* d_tape,
                          const double* d_nrows, const double* d_xs_T, const double* d_Ps_T, double* d_xs, double* d_pstd_s, double* d_Ps,
                          double* d_Ps0, double* d_sinfo);
BROV_API int brov_ukf_smooth_quat(brov_ctx* ctx, int integrator, int64_t P, const brov_params* params /* [P], host */, int64_t nrec,
                         const brov_ukf* ukf /* [nrec], host */, int64_t B, int64_t T, double dt, const double* x0, const double* P0,
                         const double* U, const double* Y, double* xf, double* pstd, double* innov, double* xT, double* PT, double* info,
                         double* xs, double* pstd_s, double* Ps, double* Ps0, double* sinfo, int64_t tape_bytes);
BROV_API int brov_ukf_smooth_quat_dev(brov_ctx* ctx, int integrator, int64_t P, const brov_params* params /* [P], host */, int64_t nrec,
                             const brov_ukf* ukf /* [nrec], host */, int64_t B, int64_t T, double dt, const double* d_x0,
                             const double* d_P0, const double* d_U, const double* d_Y, double* d_xf, double* d_pstd, double* d_innov,
                             double* d_xT, double* d_PT, double* d_info, double* d_xs, double* d_pstd_s, double* d_Ps, double* d_Ps0,
                             double* d_sinfo, int64_t tape_bytes);

/* ---- output-feedback closed loop: the filter inside the rollout kernel ----------------------------------------------------------
 * brov_rollout_feedback feeds the TRUE state back, and brov_ukf_filter runs over recordings whose commands are fixed.  A vehicle
 * never sees its true state: brov_output_feedback closes the loop through the estimate.  Candidate j pairs a filter model
 * params[j] with a plant plant[j] (nplant = P), or with the one plant plant[0] (nplant = 1: one true vehicle controlled through P
 * model draws); both are HOST arrays as in brov_rollout_pop.  Every candidate runs B closed loops of T steps, in one launch whatever
 * P, B and T are.  Models BROV_THRUSTER_EULER and BROV_WRENCH_EULER, both integrators, both lag modes, the range of P: those of
 * brov_ukf_filter.  fb [nfb] and ukf [nrec] are the records of brov_rollout_feedback and brov_ukf_filter with their rules (nfb and
 * nrec 1 or P).
 *
 * Inputs, shared by the candidates: x0_true [B][12], the plant's start; x0_est [B][12] and P0 [B][12][12] (lower triangle read),
 * the filter's start, the estimate of row 0 BEFORE its measurement; V [B][T][12], the measurement noise, where a NaN means "this
 * component is not measured at this row" (there is no random generator in the kernel: the caller draws V); W [B][T][12], an
 * optional process disturbance (NULL = none); u_ff [B][T][nu] optional (NULL = 0); ref [B][ref_rows][12], ref_rows 1 (a set-point)
 * or T.
 *
 * For t = 0 .. T-1, from (x_true, x, P, z) = (x0_true, x0_est, P0, z_io):
 *   1. Measure.  y = x_true + V[t] component-wise; y_out[t] = y (NaN exactly where V[t] is NaN).
 *   2. Update.  Stage 1 of brov_ukf_filter on (x, P) with the row y: the same order, wrap, skips and log-likelihood.  Outputs
 *      xf[t], pstd[t], innov[t].
 *   3. Command.  At a tick (t a multiple of hold, counted from the start of the call) the law of brov_rollout_feedback with the
 *      tracking error e taken from the ESTIMATE, e = e(xf[t], ref[t]):
 *          u = clip(u_ff[t] + K e + Ki z, u_min, u_max),   then   z <- clip(z + hold dt e[0:6], -z_max, z_max),
 *      in that kernel's order of operations.  Between ticks the command is held.  u_applied[t] = u.
 *   4. Plant.  x_true advances one step under u through the general step of brov_rollout_pop with the PLANT's parameters and the
 *      plant's own lag bank; with W, x_true += W[t] afterwards.  traj[t+1] = x_true (traj[0] = x0_true).
 *   5. Predict.  Stage 2 of brov_ukf_filter on (x, P) with the command u, under params[j], with the filter's own lag bank.
 * So the estimator is brov_ukf_filter on the rows (u_applied, y_out) and the plant is brov_rollout_pop on u_applied, bit for bit.
 *
 * Metrics [7] per (candidate, run).  Entries 0 .. 3 are the four of brov_rollout_feedback, evaluated at every step on the TRUE state
 * at the start of the step: sum dt |e[0:3]|^2 and sum dt |e[3:6]|^2 with e = e(x_true, ref[t]), sum dt |u|^2 of the applied command,
 * and the number of steps at which a channel of the applied command equals its u_min or u_max.  Entries 4 .. 6 are the estimation
 * error sum dt |xf[t] - x_true|^2 over the position (components 0 .. 2), the attitude (3 .. 5, each difference wrapped as in the
 * filter) and the velocity (6 .. 11), x_true at the start of step t.  info [4] is brov_ukf_filter's.
 *
 * Outputs, per candidate, each may be NULL: traj [P][B][T+1][12]; y_out, xf, pstd, innov [P][B][T][12]; u_applied [P][B][T][nu];
 * xT_true, xT [P][B][12]; PT [P][B][12][12]; metrics [P][B][7]; info [P][B][4].  In / out, per candidate: lag_est_io and
 * lag_plant_io [P][B][8][3] (thruster model; both or neither; NULL = both start from zero lag, nothing returned) and z_io [P][B][6]
 * (NULL = start from zero, nothing returned).
 * Checkpoint: (xT_true, xT, PT, lag_est_io, lag_plant_io, z_io).  A call of T1 steps, T1 a multiple of hold, continued by a call
 * from the checkpoint with the remaining rows of V, W, u_ff and ref gives the bits of the unbroken call in every per-row output
 * (traj: the second call's row 0 repeats the first call's last) and in the checkpoint; the metrics and info[0] of the two spans
 * add up to rounding, info[1] exactly.
 *
 * Failure is the filter's: a numerical condition of one (candidate, run), handled in the kernel, which stops that run alone; the
 * call returns BROV_OK and no other run is touched.  What was complete before the failing stage is kept, the rest is NaN:
 *   stage 1 of row t fails (s <= 0 or not finite):  kept  traj [0 .. t], y_out [0 .. t], xf, pstd, innov, u_applied [0 .. t-1];
 *                                                   NaN   traj [t+1 ..], y_out [t+1 ..], xf, pstd, innov, u_applied [t ..];
 *   stage 2 of row t fails (a pivot argument <= 0 or not finite, or a non-finite predicted mean; the command and the plant's
 *   step of row t are complete):                    kept  traj [0 .. t+1], y_out, xf, pstd, innov, u_applied [0 .. t];
 *                                                   NaN   traj [t+2 ..], y_out, xf, pstd, innov, u_applied [t+1 ..].
 * In both cases xT_true, xT, PT and all seven metrics are NaN, info = (-inf, updates so far, t, smallest pivot so far), and
 * lag_est_io, lag_plant_io and z_io are left as they came.
 *
 * Refused on the host with BROV_ERR_ARG and a brov_last_error text naming the rule, before anything is copied or launched: what
 * brov_rollout_feedback refuses of a record and of ref_rows (hold < 1, nfb not in {1, P}, ref_rows not in {1, T}, u_min > u_max,
 * a negative z_max, a NaN anywhere in fb), what brov_ukf_filter refuses (a model other than the two above, nrec not in {1, P}, the
 * rules of alpha, lambda, q and r, T < 1, P > 65535, dt not finite and > 0, a singular mass matrix of a model or of a plant), and:
 * nplant not in {1, P}; one of lag_est_io, lag_plant_io without the other; a NULL params, plant, fb, ukf, x0_true, x0_est, P0, V or
 * ref.  B = 0 or P = 0: BROV_OK, nothing touched.  The ctx's own parameters are neither read nor written.
 * Deterministic (no atomics, fixed summation orders, every run writes its own outputs): two calls give the same bits. */
BROV_API int brov_output_feedback(brov_ctx* ctx, int model, int integrator, int lag_mode, int64_t P, const brov_params* params /* [P], host */,
                         int64_t nplant, const brov_params* plant /* [nplant], host */, int64_t nfb, const brov_feedback* fb /* [nfb], host */,
                         int64_t nrec, const brov_ukf* ukf /* [nrec], host */, int64_t B, int64_t T, double dt, const double* x0_true,
                         const double* x0_est, const double* P0, const double* V, const double* W, const double* u_ff, const double* ref,
                         int64_t ref_rows, double* lag_est_io, double* lag_plant_io, double* z_io, double* traj, double* y_out,
                         double* u_applied, double* xf, double* pstd, double* innov, double* xT_true, double* xT, double* PT,
                         double* metrics, double* info);
BROV_API int brov_output_feedback_dev(brov_ctx* ctx, int model, int integrator, int lag_mode, int64_t P, const brov_params* params /* [P], host */,
                             int64_t nplant, const brov_params* plant /* [nplant], host */, int64_t nfb,
                             const brov_feedback* fb /* [nfb], host */, int64_t nrec, const brov_ukf* ukf /* [nrec], host */, int64_t B,
                             int64_t T, double dt, const double* d_x0_true, const double* d_x0_est, const double* d_P0, const double* d_V,
                             const double* d_W, const double* d_u_ff, const double* d_ref, int64_t ref_rows, double* d_lag_est_io,
                             double* d_lag_plant_io, double* d_z_io, double* d_traj, double* d_y_out, double* d_u_applied, double* d_xf,
                             double* d_pstd, double* d_innov, double* d_xT_true, double* d_xT, double* d_PT, double* d_metrics,
                             double* d_info);

/* ---- model-predictive control: one sampling-based (MPPI) update, sampled, rolled out and scored on the device ---------------------
 * brov_mppi_step performs one MPPI update for B independent problems (B vehicles, or B draws of a fit).  Problem b has a state
 * x [nx], for the thruster model optionally a start lag [8][3] (read only; NULL = zero), a reference, and a nominal knot sequence
 * U_nom [M][nu] with M = ceil(H / hold): step t of the horizon uses knot m(t) = t / hold (the last knot may cover fewer than hold
 * steps).
 *
 * Samples.  Sample 0 is the nominal itself (xi = 0).  For k >= 1 and sigma[j] > 0, xi[k][m][j] is read from the optional eps
 * [B][K][M][nu] (row k = 0 of eps is ignored, and so are the channels with sigma[j] = 0), or, with eps = NULL, drawn from the
 * library's counter-based stream: counter c = ((b K + k) M + m) nu + j, second stream s2 = seed ^ 0xA5A5A5A5A5A5A5A5,
 * xi = sqrt(-2 ln(1 - u1)) cos(2 pi u2) with u1, u2 the uniforms number 2c and 2c + 1 of s2 -- the normal of dist B of
 * brov_fill_controls_dev.
 * Sample command and rollout.
 *     v[k][m][j]     = clip(U_nom[m][j] + sigma[j] xi[k][m][j], u_min[j], u_max[j])        (a NaN xi stays a NaN)
 *     delta[k][m][j] = v[k][m][j] - U_nom[m][j]                                            the perturbation after the clamp
 * The rollout of sample k applies v[k][m(t)] at step t, H steps from x (and the lag), with the model, integrator and lag mode of
 * brov_rollout_pop (the general step, both integrators, both lag modes; the double-integrator models: BROV_ERR_ARG).
 * Cost.  e_t = the tracking error e[12] of brov_rollout_feedback on the state at the start of step t against reference row
 * ref_row0 + t:
 *     S_k = sum_{t<H} dt ( sum_i q[i] e_t[i]^2 + sum_j r[j] v[k][m(t)][j]^2 )
 *           + sum_i qf[i] e_H[i]^2                                                          the end state against row ref_row0 + H
 *           + gamma sum_m sum_{j: sigma[j] > 0} U_nom[m][j] delta[k][m][j] / sigma[j]^2     the importance term
 * Reference: ref [B][ref_total][nx].  ref_total = 1 is a set-point (ref_row0 must be 0); otherwise the call reads the rows
 * ref_row0 .. ref_row0 + H, which must lie inside ref_total.
 * Update.  A non-finite S_k is left out (weight 0) and counted.  beta = the minimum over the finite S_k,
 *     w_k = exp(-(S_k - beta) / lambda),   eta = sum_k w_k,
 *     U_new[m][j] = clip(U_nom[m][j] + sum_k w_k delta[k][m][j] / eta, u_min[j], u_max[j]).
 * shift = 0: U_nom <- U_new.  shift = 1: U_nom[m] <- U_new[m + 1], the last knot repeated (the plan of the next controller tick).
 * Outputs, each optional: u_apply [B][hold][nu] = U_new[0] in hold rows (what brov_rollout_pop_dev takes as U for the plant);
 * cost [B][K]; info [B][4] = S_0, beta, the effective sample size eta^2 / sum_k w_k^2, the number of non-finite samples.
 * A problem with no finite sample: its U_nom is left as it came (no shift), u_apply is the clamped first knot, info = (S_0, +inf,
 * 0, K); the call still returns BROV_OK.
 *
 * Arguments.  params is a HOST array of nparams sets, nparams = 1 (one planning model for every problem) or B (one per problem);
 * the ctx's own parameters are neither read nor written.  cfg is ONE host record.  U_nom [B][M][nu] is in / out.  1 <= B <= 65535,
 * 1 <= K <= 2^31, 1 <= H <= 2^31; B = 0: BROV_OK, nothing touched.  Refused on the host with BROV_ERR_ARG and a brov_last_error
 * text naming the rule, before anything is copied or launched: K < 1 or K > 2^31, H < 1 or H > 2^31, hold < 1, lambda <= 0, a
 * negative weight, sigma or gamma, u_min > u_max (channels < nu), a NaN anywhere in cfg, nparams not in {1, B}, a reference window
 * outside ref_total, B > 65535, a double-integrator model, a NULL params, cfg, x, ref or U_nom, a dt that is not finite and > 0, a
 * parameter set with a singular mass matrix.
 * Deterministic: no atomics, every sum in a fixed order -- two calls with the same arguments give the same bits in every output. */
typedef struct brov_mppi {
    double q[12], qf[12];           /* stage / terminal weights on the tracking error e[12] of brov_rollout_feedback, >= 0 */
    double r[8];                    /* weights on the command, >= 0; entries >= nu ignored */
    double sigma[8];                /* standard deviation of the perturbation per channel, >= 0 (0: channel not perturbed) */
    double u_min[8], u_max[8];      /* u_min <= u_max, may be +-inf */
    double lambda;                  /* temperature, > 0 */
    double gamma;                   /* weight of the importance term, >= 0 (the usual choice is lambda) */
    int32_t hold, _pad;             /* >= 1 */
} brov_mppi;
BROV_API int brov_mppi_step(brov_ctx* ctx, int model, int integrator, int lag_mode, int64_t B, int64_t nparams,
                   const brov_params* params /* [nparams], host */, const brov_mppi* cfg /* host */, int64_t K, int64_t H, double dt,
                   uint64_t seed, const double* x, const double* lag, const double* ref, int64_t ref_total, int64_t ref_row0,
                   const double* eps, double* U_nom, int shift, double* u_apply, double* cost, double* info);
BROV_API int brov_mppi_step_dev(brov_ctx* ctx, int model, int integrator, int lag_mode, int64_t B, int64_t nparams,
                       const brov_params* params /* [nparams], host */, const brov_mppi* cfg /* host */, int64_t K, int64_t H, double dt,
                       uint64_t seed, const double* d_x, const double* d_lag, const double* d_ref, int64_t ref_total, int64_t ref_row0,
                       const double* d_eps, double* d_U_nom, int shift, double* d_u_apply, double* d_cost, double* d_info);

/* ---- model-predictive control planned with a Koopman EDMDc model -------------------------------------------------------------------
 * edmdc_mppi_step performs one MPPI update for nb problems with an EDMDc model as the planning model: n in {12, 13} states,
 * r = nu in {6, 8} inputs, k >= 0 centres C [k][n], gamma, A [d][d], B [d][r] with d = n + k (what KoopmanEDMDc.fit returns).
 * Everything that does not concern the prediction is the law of brov_mppi_step, word for word: the brov_mppi record, the knots
 * (M = ceil(H / hold)), sample 0 is the nominal, the counter c = ((b K + k) M + m) nu + j on the second stream or the explicit eps
 * [nb][K][M][nu], the clamp that keeps a NaN and delta, the importance term, the treatment of non-finite costs, the soft-min,
 * shift, u_apply, cost and info, the no-finite-sample rule, and determinism.  The same seed gives the same v[k][m][j] as
 * brov_mppi_step does.
 * Prediction.  z_0 = phi(x) = [x, exp(-gamma (|x|^2 + |c_i|^2 - 2 x.c_i))], the lift as edmdc_lift computes it;
 * z_{t+1} = A z_t + B v[k][m(t)];  x_hat_t = z_t[0:n], with no re-lifting: KoopmanEDMDc.simulate applied to the sample's command
 * sequence.  The call evaluates this in the linear form
 *     x_hat_t = P[t] phi(x) + sum_{m : m hold < t} Gc[t][m] v[k][m]            (m ascending, then the channels ascending)
 * from two coefficient arrays that the caller passes, formed with E = the first n rows of the identity as
 *     P[0] = E,  P[t+1] = P[t] A                                               P [H+1][n][d]
 *     G[j] = P[j] B                                                            (n x r)
 *     Gc[t][m] = sum_{s : m(s) = m, s < t} G[t-1-s]   in ascending s           Gc [H+1][M][n][r], zero where m hold >= t
 * (m(s) = s / hold; entries with m hold >= t are never read).  A and B are required as the model the coefficients belong to; the
 * call itself reads P and Gc only.  The linear form agrees with the iterated recursion to rounding amplified by |E A^t|.
 * Cost.  e_t = the tracking error e[12] of brov_rollout_feedback on x_hat_t against reference row ref_row0 + t: n = 12 with the
 * Euler-angle error, n = 13 with the quaternion error on the predicted quaternion as it stands (x_hat is not normalised; the
 * rotation normalises its copy as the quaternion model does).  S_k is then brov_mppi_step's expression.  x [nb][n], ref
 * [nb][ref_total][n], U_nom [nb][M][nu] in / out.
 * One more optional output: pred [nb][K][H+1][n], the predicted states of every sample (row 0 = x); NULL = no stores.
 * Refused on the host with BROV_ERR_ARG and a brov_last_error text naming the rule, before anything is copied or launched: what
 * brov_mppi_step refuses of K, H, the record, the reference window, nb > 65535 and dt; n or r outside the sets above; k < 0 or
 * k > 1024; a NULL cfg, x, ref, U_nom, A, B, P or Gc; a NULL C with k > 0; a NaN gamma; M nu > 312 (a sample's commands live in
 * the 160 KB of LDS of one 64-lane block).  nb = 0: BROV_OK, nothing touched. */
BROV_API int edmdc_mppi_step(brov_ctx* ctx, int n, int r, int k, double gamma, const double* C, const double* A, const double* B,
                    const double* P, const double* Gc, int64_t nb, const brov_mppi* cfg /* host */, int64_t K, int64_t H, double dt,
                    uint64_t seed, const double* x, const double* ref, int64_t ref_total, int64_t ref_row0, const double* eps,
                    double* U_nom, int shift, double* u_apply, double* cost, double* info, double* pred);
BROV_API int edmdc_mppi_step_dev(brov_ctx* ctx, int n, int r, int k, double gamma, const double* d_C, const double* d_A, const double* d_B,
                        const double* d_P, const double* d_Gc, int64_t nb, const brov_mppi* cfg /* host */, int64_t K, int64_t H,
                        double dt, uint64_t seed, const double* d_x, const double* d_ref, int64_t ref_total, int64_t ref_row0,
                        const double* d_eps, double* d_U_nom, int shift, double* d_u_apply, double* d_cost, double* d_info,
                        double* d_pred);

/* ---- linear model-predictive control with a Koopman EDMDc model: a batched box-constrained QP ---------------------------------------
 * edmdc_lmpc_step solves, for nb problems, the convex QP that the EDMDc model makes of the tracking problem of edmdc_mppi_step: the
 * prediction is linear in the knots v [M][nu], the error is taken linear too, so the cost is a quadratic with ONE matrix Hq for
 * every problem and a vector g per problem.  The model arguments n, r = nu, k, gamma, C, A, B, P, Gc, the knots (M = ceil(H / hold),
 * Nv = M nu <= 312) and the reference window (ref_total, ref_row0; one row = a set-point) are those of edmdc_mppi_step.
 * Prediction.  x_hat_t = F[t] + sum_{m : m hold < t} Gc[t][m] v[m], F[t] = P[t] phi(x): the bits of edmdc_mppi_step's prediction.
 * Linear error.  e_t = rt_t - x_hat_t, plain component differences, where rt_t is reference row ref_row0 + t adjusted ONCE against the
 * measured state x (never against the prediction):
 *     n = 12: rt_t[i] = r_t[i] - 2 pi rint((r_t[i] - x[i]) / (2 pi)) for the angles i = 3, 4, 5; the other entries as they are
 *     n = 13: entries 3..6 of r_t times -1 when sum_i x[3+i] r_t[3+i] < 0 (the short way round); the other entries as they are
 * Objective.  brov_mppi_step's cost with this error and no importance term:
 *     J(v) = sum_{t<H} dt ( sum_i q[i] e_t[i]^2 + sum_j r[j] v[m(t)][j]^2 ) + sum_i qf[i] e_H[i]^2              i < n
 *          = 1/2 v' Hq v + g' v + c,   with w_t = dt, Q_t = q for t < H, w_H = 1, Q_H = qf, e0_t = F[t] - rt_t:
 *     Hq = 2 sum_t w_t Gc[t]' diag(Q_t) Gc[t] + 2 diag(dt r[j] steps(m))        steps(m) = the horizon steps knot m holds
 *     g  = 2 sum_t w_t Gc[t]' diag(Q_t) e0_t                                    (t ascending, then i ascending, one sum per column)
 *     c  = J(0)
 * Gc[t] is the n x Nv matrix [Gc[t][0] .. Gc[t][M-1]] (zero where m hold >= t).  Hq depends on the model, the record, H and dt only.
 * The caller passes W [Nv][Nv] = (Hq + rho I)^-1, symmetric, as it passes P and Gc; the call reads W as given and needs Hq nowhere.
 * Iteration.  Scaled ADMM from z = clip(U_nom, u_min, u_max) and y = y_io (NULL: 0):
 *     v+ = W (rho (z - y) - g)            (row i: the sum over j ascending of W[j][i] s_j)
 *     z+ = clip(v+ + y, u_min, u_max),    y+ = (y + v+) - z+
 *     r_prim = max |v+ - z+|,   r_dual = rho max |z+ - z|
 * A problem stops after the first iteration at which r_prim <= tol and r_dual <= tol (tol = 0: no test), or after `iters`; the
 * problems stop independently.  With iters = 0 there is no residual: both are reported as +inf.
 * In / out: U_nom [nb][M][nu] receives z; y_io [nb][M][nu] (optional) receives y; shift = 1 moves both one knot forward, the last knot
 * repeated.  Outputs, each optional: u_apply [nb][hold][nu] = the first knot of z (before the shift) in hold rows; pred [nb][H+1][n] =
 * x_hat under z; info [nb][6] = J(z), J(clip(U_nom)), r_prim, r_dual, the iterations done, the number of entries of z equal to a
 * limit.  J is evaluated from the prediction, never from W: a W that belongs to another record shows as a J that does not fall.
 * A problem whose g or c is not finite: U_nom and y_io are left as they came (no shift), u_apply is the clamped first knot, info =
 * (+inf, +inf, +inf, +inf, 0, 0), pred is NaN; the call still returns BROV_OK.
 * Refused on the host with BROV_ERR_ARG and a brov_last_error text naming the rule, before anything is copied or launched: what
 * edmdc_mppi_step refuses of n, r, k, H, M nu, nb, dt, gamma, the reference window and NULL arrays; a NULL W; hold < 1; iters outside
 * 0 .. 1 000 000; rho not finite and > 0; tol negative; a negative weight; u_min > u_max (channels < nu); a NaN anywhere in the
 * record.  nb = 0: BROV_OK, nothing touched.
 * Deterministic: no atomics, every sum in a fixed order -- two calls with the same arguments give the same bits in every output. */
typedef struct brov_lmpc {
    double q[13], qf[13];           /* stage / terminal weights on the linear error, >= 0; entry 12 ignored for n = 12 */
    double r[8];                    /* weights on the command, >= 0; entries >= nu ignored.  (q, qf, r) must make Hq positive definite */
    double u_min[8], u_max[8];      /* u_min <= u_max, may be +-inf */
    double rho;                     /* ADMM penalty, finite and > 0: the rho of W */
    double tol;                     /* >= 0; 0 = always `iters` iterations */
    int32_t hold, iters;            /* hold >= 1; 0 <= iters <= 1 000 000 */
} brov_lmpc;
BROV_API int edmdc_lmpc_step(brov_ctx* ctx, int n, int r, int k, double gamma, const double* C, const double* A, const double* B,
                    const double* P, const double* Gc, const double* W, int64_t nb, const brov_lmpc* cfg /* host */, int64_t H, double dt,
                    const double* x, const double* ref, int64_t ref_total, int64_t ref_row0, double* U_nom, double* y_io, int shift,
                    double* u_apply, double* pred, double* info);
BROV_API int edmdc_lmpc_step_dev(brov_ctx* ctx, int n, int r, int k, double gamma, const double* d_C, const double* d_A, const double* d_B,
                        const double* d_P, const double* d_Gc, const double* d_W, int64_t nb, const brov_lmpc* cfg /* host */, int64_t H,
                        double dt, const double* d_x, const double* d_ref, int64_t ref_total, int64_t ref_row0, double* d_U_nom,
                        double* d_y_io, int shift, double* d_u_apply, double* d_pred, double* d_info);
/* The LDS bytes of one block of the solver (four problems) at Nv = M nu variables, and in *w_in_lds (optional) whether W is staged
 * into them (1) or read from global memory (0): staged while two blocks fit the 160 KB of a compute unit together.  Needs no device.
 * -1 for nv outside 1 .. 312. */
BROV_API int edmdc_lmpc_block_lds(int64_t nv, int* w_in_lds);

/* ---- PINc residual network (inference) ----------------------------------------------------
 * The reference's PINcNet (training/train_tank_brov2_full_comparison.py:648-721) with the architecture of its shipped
 * checkpoint: z = [x9, u4, dt] (14) -> 4 x (Linear, AdaptiveSoftplus, LayerNorm(64)) -> Linear(64 -> 9), fp32.
 * x9 = [x y z cos(psi) sin(psi) u v w r]; u4 = tau[0,1,2,5] of the thruster map (compute_thruster_forces, fp64, stateful lag
 * [8][3] as in brov_thruster_forces, discretised at dt), rounded to fp32 with the rest of z.  12-D states follow
 * dataset12_to_9 / state9_to_12 (:612-646): phi, theta, p, q of a predicted state are 0, psi = atan2(sin, cos). */
/* The packed parameters: n = 14541 fp32 values in state-dict order (net.0.weight [64][14], net.0.bias, net.1.beta,
 * net.2.weight, net.2.bias, net.3.weight ... net.12.weight [9][64], net.12.bias), i.e. the checkpoint the script loads at
 * :948-952.  Copied to the device; every other brov_pinc_* call fails (BROV_ERR_ARG) until this one has succeeded. */
BROV_API int brov_pinc_set_weights(brov_ctx* ctx, const float* blob, int64_t n);
/* PINcNet.forward (:695-721): d_z [B][14] fp32 -> d_x_next [B][9] fp32. */
BROV_API int brov_pinc_forward_dev(brov_ctx* ctx, int64_t B, const float* d_z, float* d_x_next);
/* simulate_pinc (:838-863) for B trajectories: x0 [B][12], U [B][T][8]; lag_io [B][8][3] is each trajectory's map vehicle
 * (advanced in place; NULL = zero lag, not returned); traj [B][T/traj_stride+1][12] (row 0 = x0 unchanged; NULL = not stored),
 * xT [B][12] (optional). */
BROV_API int brov_pinc_rollout(brov_ctx* ctx, int64_t B, int64_t T, double dt, const double* x0, const double* U,
                      double* lag_io, double* traj, int64_t traj_stride, double* xT);
BROV_API int brov_pinc_rollout_dev(brov_ctx* ctx, int64_t B, int64_t T, double dt, const double* d_x0, const double* d_U,
                          double* d_lag_io, double* d_traj, int64_t traj_stride, double* d_xT);
/* multistep_rmse_endpoint_pinc (:866-890): windows k = 0..N-H-1 as in brov_window_endpoint_se, X [N][12], U [N-1][8] (window k reads
 * U[k .. k+H-1], so rows up to N-2 only; no row of U is read when H = 0).
 * lag_io [8][3] is the map vehicle's lag before the first window (NULL = zero).  carry_lag=1 is the reference: one vehicle serves
 * every window, window k starts from the lag window k-1 left, and lag_io receives the lag after the last window (the vehicle
 * carries it into the next call).  carry_lag=0: every window starts from lag_io, which is left unchanged.
 * se_total = sum_k |x_end - X[k+H]|^2 (12-D, fp64); per_window [N-H] and lag_starts [N-H][8][3] (each window's initial lag,
 * carry_lag=1 only) optional (NULL); the _dev form requires d_per_window. */
BROV_API int brov_pinc_window_endpoint_se(brov_ctx* ctx, int64_t N, int64_t H, double dt, const double* X, const double* U,
                                 int carry_lag, double* lag_io, double* se_total, double* per_window, double* lag_starts);
BROV_API int brov_pinc_window_endpoint_se_dev(brov_ctx* ctx, int64_t N, int64_t H, double dt, const double* d_X, const double* d_U,
                                     int carry_lag, double* d_lag_io, double* d_se_total, double* d_per_window,
                                     double* d_lag_starts);

/* ---- PINc residual network (training) -----------------------------------------------------
 * train_pinc's loop body (training/train_tank_brov2_full_comparison.py:790-835) in fp32.  A minibatch of B rows z [B][14],
 * y [B][9], u4 [B][4] (all fp32, what the reference's .float() makes of make_pinc_dataset's arrays) gives three loss terms
 *   loss[0] = mse(model(z), y)                                  mean over B*9
 *   loss[1] = physics_loss(model(z), u4)                         mean square of the 4-DOF right-hand side; a value only (no_grad)
 *   loss[2] = rollout_loss(model, z, K)                          K steps from batch row 0, step i scored against row i+1
 * with total = loss[0] + 0.5 loss[1] + loss[2], and the gradient of loss[0] + loss[2] over the 14541 parameters in blob order.
 * K must be < B and <= 16 (0 = no rollout term).  Sums run in a fixed order: the same inputs give the same bits. */
typedef struct brov_pinc_hyper {
    double lr, beta1, beta2, eps, weight_decay;   /* torch.optim.AdamW: 3e-3, 0.9, 0.999, 1e-8, 0.01 */
    double max_norm;                              /* clip_grad_norm_: 5.0 */
    int32_t batch, rollout_steps;                 /* 256, 10; each iteration uses K = min(rollout_steps, rows - 1) */
    int32_t use_physics, use_rollout;
} brov_pinc_hyper;
/* One minibatch, no update: d_weights [14541] fp32 (device) -> d_grad [14541] (unclipped), d_loss [3].  Asynchronous. */
BROV_API int brov_pinc_loss_grad_dev(brov_ctx* ctx, const float* d_weights, int64_t B, const float* d_z, const float* d_y,
                                     const float* d_u4, int K, int use_physics, float* d_grad, float* d_loss);
/* clip_grad_norm_(max_norm) on d_grad (which is left as given) then AdamW step number `step` (1-based) on d_w, d_m, d_v [14541]
 * in place; d_norm_out [1] (optional) receives the 2-norm before clipping.  Asynchronous. */
BROV_API int brov_pinc_adamw_step_dev(brov_ctx* ctx, float* d_w, float* d_m, float* d_v, const float* d_grad, int64_t step, double lr,
                                      double beta1, double beta2, double eps, double weight_decay, double max_norm, float* d_norm_out);
/* A training session owned by the ctx: begin copies blob [n = 14541] (host) to a device copy of its own with m = v = 0, step = 0;
 * the weights brov_pinc_set_weights gave the ctx are neither read nor written.  A second begin replaces the session. */
BROV_API int brov_pinc_train_begin(brov_ctx* ctx, const float* blob, int64_t n, const brov_pinc_hyper* hyper);
/* Optimiser state of a resumed run: m, v [14541] (host), step >= 0. */
BROV_API int brov_pinc_train_set_state(brov_ctx* ctx, const float* m, const float* v, int64_t step);
/* One epoch over d_Z [N][14], d_Y [N][9], d_U4 [N][4] (device, fp32) in the order d_perm [N] (device, int32, a permutation of
 * 0..N-1): queues all ceil(N / batch) iterations on the ctx stream and returns; iteration i writes its three loss terms to
 * d_loss_log[3 i ..].  The arrays must stay valid until the stream has been synchronised. */
BROV_API int brov_pinc_train_epoch_dev(brov_ctx* ctx, int64_t N, const float* d_Z, const float* d_Y, const float* d_U4,
                                       const int32_t* d_perm, float* d_loss_log);
/* Weights and optimiser state to the host (each optional): blob_out, m_out, v_out [14541], step_out [1].  Synchronises. */
BROV_API int brov_pinc_train_get(brov_ctx* ctx, float* blob_out, float* m_out, float* v_out, int64_t* step_out);
BROV_API int brov_pinc_train_end(brov_ctx* ctx);
/* make_pinc_dataset's loop over compute_thruster_forces (:732-735): ONE stateful vehicle fed U [N][8] in order -> tau [N][6];
 * lag_io [8][3] is its lag before the first sample and receives the lag after the last. */
BROV_API int brov_thruster_stream(brov_ctx* ctx, int64_t N, const double* U, double dt, double* lag_io, double* tau);
BROV_API int brov_thruster_stream_dev(brov_ctx* ctx, int64_t N, const double* d_U, double dt, double* d_lag_io, double* d_tau);

/* Synthetic control sequences on device (benchmarks):
 * counter-based splitmix64 stream, value for (trajectory b0+b, step t, channel j) independent
 * of layout and of how trajectories are sharded.  scale[nu] multiplies each channel (NULL = 1). */
BROV_API int brov_fill_controls_dev(brov_ctx* ctx, int layout, int dist, int64_t B, int64_t T, int nu,
                           uint64_t seed, int64_t b0, int64_t T_total, const double* scale_host,
                           double* d_U);

/* ---- Koopman EDMDc --------------------------------------------------------------------- */
/* phi(x) = [x, exp(-gamma(|x|^2 + |c|^2 - 2 x.c))]: KoopmanEDMDc._lift / _rbf_mat
 * (Koopman/koopmanEDMDc.py:41-48,221-236).  X [N][n], C [k][n] -> Z [N][n+k]. */
BROV_API int edmdc_lift(brov_ctx* ctx, int64_t N, int n, int k, double gamma, const double* X, const double* C, double* Z);

/* Normal-equation blocks of fit / fit_multi (Koopman/koopmanEDMDc.py:89-97,129-147):
 *   G = [phi(x_t), u_t], Y = phi(x_{t+1});  GtG [p][p] = G^T G, GtY [p][d] = G^T Y,
 *   d = n + k, p = d + r, feature order exactly the reference's ([x, rbf..., u]).
 * Data: nbags trajectories ("bags"); bag b holds states X[b*x_bag_stride + t], t = 0..L,
 * and inputs U[b*u_bag_stride + t], t = 0..L-1, i.e. L pairs per bag and no pair crosses
 * a bag.  fit(X,U) is nbags=1, L=N-1.  accumulate=1 adds to the GtG/GtY passed in.
 * The host forms of edmdc_gram*, edmdc_pinv_apply* and edmdc_kmeans_lloyd stage their arrays in the ctx's scratch arena like every
 * other host form: it only grows, so a context keeps the device bytes of its largest host call until brov_destroy. */
BROV_API int edmdc_gram(brov_ctx* ctx, int n, int r, int k, double gamma, const double* C,
               int64_t nbags, int64_t L, int64_t x_bag_stride, int64_t u_bag_stride,
               const double* X, const double* U, int accumulate, double* GtG, double* GtY);
BROV_API int edmdc_gram_dev(brov_ctx* ctx, int n, int r, int k, double gamma, const double* d_C,
                   int64_t nbags, int64_t L, int64_t x_bag_stride, int64_t u_bag_stride,
                   const double* d_X, const double* d_U, int accumulate, double* d_GtG, double* d_GtY);
/* The same normal-equation blocks for a RAGGED list of trajectories -- fit_multi(X_list, U_list), Koopman/koopmanEDMDc.py:113-152:
 * "Each (X, U) is a bag/rollout.  We never create cross-bag transitions"; a bag with fewer than 2 states contributes nothing (:131-132),
 * bag b contributes the pairs (X_b[t], U_b[t], X_b[t+1]), t = 0 .. len(X_b) - 2 (:133-138).
 * Data: the bags' rows one after the other.  X [rows][n] = np.vstack(X_list) (:125 -- also what the reference clusters for its centres),
 * U [rows][r] ROW-ALIGNED with X (U_b[t] next to X_b[t]; the row next to the last state of a bag is never read -- the reference drops it
 * with U[:-1]), bag b = rows bag_offsets[b] .. bag_offsets[b + 1] - 1, bag_offsets [nbags + 1] on the HOST in both forms (metadata: it is
 * validated there -- bag_offsets[0] = 0, non-decreasing -- and rows = bag_offsets[nbags]).  Empty bags and one-row bags are allowed.
 * One call lifts every state once, whatever the number of bags: no per-bag launch, allocation or copy. */
BROV_API int edmdc_gram_ragged(brov_ctx* ctx, int n, int r, int k, double gamma, const double* C,
                               int64_t nbags, const int64_t* bag_offsets, const double* X, const double* U,
                               int accumulate, double* GtG, double* GtY);
BROV_API int edmdc_gram_ragged_dev(brov_ctx* ctx, int n, int r, int k, double gamma, const double* d_C,
                                   int64_t nbags, const int64_t* bag_offsets, const double* d_X, const double* d_U,
                                   int accumulate, double* d_GtG, double* d_GtY /* NULL: G^T G alone */);
/* Rows lifted per chunk by edmdc_gram* (workspace = rows * padded_width * 8 bytes). */
BROV_API int edmdc_set_chunk_rows(brov_ctx* ctx, int64_t rows);

/* H-step propagation in lifted space + endpoint squared error: KoopmanEDMDc.multistep_rmse /
 * evaluate (Koopman/koopmanEDMDc.py:157-200).  X [N][n], U [N-1][r] or longer (only rows 0..N-2 are read, as in the
 * reference, which accepts len(U) == len(X) - 1), A [d][d], B [d][r];
 * se_total = sum over k < N-H and the n state coordinates of (X[k+H] - x_hat)^2;
 * rmse = sqrt(se_total / ((N-H) * n)).  xhat_end [N-H][n] optional (NULL). */
BROV_API int edmdc_multistep_se(brov_ctx* ctx, int n, int r, int k, double gamma, const double* C,
                       const double* A, const double* B, int64_t N, int64_t H,
                       const double* X, const double* U, double* se_total, double* xhat_end);
/* The same scores by linearity (opt-in; KoopmanEDMDc.multistep_rmse(..., method="linear")): the H-step prediction is
 *   x_hat[w] = (E A^H) phi(x_w) + sum_{t<H} (E A^(H-1-t) B) u_{w+t},   E = first n rows of the identity,
 * so the caller passes RHt [n+k][n] = (E A^H)^T and Gt [H][r][n] with Gt[t] = (E A^(H-1-t) B)^T (host, H products of n x d by d x d) and
 * the device evaluates every window in one pass -- no H-step recurrence.  Same outputs and argument rules as edmdc_multistep_se;
 * agrees with it to the rounding of the explicit powers of A (<= 1e-9 in the RMSE on the fixtures at H = 1 / 10 / 100). */
BROV_API int edmdc_multistep_se_linear(brov_ctx* ctx, int n, int r, int k, double gamma, const double* C,
                       const double* RHt, const double* Gt, int64_t N, int64_t H,
                       const double* X, const double* U, double* se_total, double* xhat_end);
/* KoopmanEDMDc.simulate (Koopman/koopmanEDMDc.py:202-216), batched over nb start states:
 * x0 [nb][n], U_seq [nb][T][r] -> X_pred [nb][T+1][n]. */
BROV_API int edmdc_simulate(brov_ctx* ctx, int n, int r, int k, double gamma, const double* C,
                   const double* A, const double* B, int64_t nb, int64_t T,
                   const double* x0, const double* U_seq, double* X_pred);

/* Lloyd iterations of k-means on device: the E/M loop of scikit-learn's KMeans(algorithm="lloyd") that
 * KoopmanEDMDc.fit / fit_multi run to place the RBF centres (Koopman/koopmanEDMDc.py:85,126).  The host layer
 * obtains the k-means++ initialisation from scikit-learn and passes it in C_io; the final centres come back
 * in C_io.  X [N][n] (row stride x_stride doubles), mean [n] = column means to subtract (NULL = none; centres
 * are then in the centred frame), stop when no label changes, when the summed squared centre shift is
 * <= tol_abs, or after max_iter iterations.  labels [N] int32 (host version: optional), inertia = sum of
 * squared distances of the samples to the centres of the returned labels, summed by differences (x - mean - c) in one pass of its own
 * after the loop: accurate relative to itself also where it is tiny against sum |x|^2 (0 when every sample is its own centre);
 * n_iter = iterations run.
 * Empty clusters follow scikit-learn 1.7.2 (sklearn/cluster/_k_means_common.pyx): `_relocate_empty_clusters_dense` moves
 * each of them to one of the n_empty samples farthest from their own centre (that sample leaves its cluster's sum), unless
 * all those distances are zero; `_average_centers` then gives a cluster that is still empty the row of the biggest cluster
 * (its mean, or -- in front of it in index order -- its member SUM, as the in-place loop of that function leaves it).
 * The member sums are exact integer sums of the samples in 2^-48 fixed point per coordinate range, so the centres are the
 * same bits from run to run, for every edmdc_set_kmeans_variant, and for any sharding over ranks. */
BROV_API int edmdc_kmeans_lloyd(brov_ctx* ctx, int64_t N, int n, int k, const double* X, const double* mean,
                                double* C_io, int max_iter, double tol_abs, int32_t* labels, double* inertia, int* n_iter);
BROV_API int edmdc_kmeans_lloyd_dev(brov_ctx* ctx, int64_t N, int n, int k, const double* d_X, int64_t x_stride,
                                    const double* mean_host, double* d_C_io, int max_iter, double tol_abs,
                                    int32_t* d_labels, double* inertia, int* n_iter);

/* Column means and (population) variances of d_X [N][n] (row stride x_stride doubles, n <= 16) into HOST arrays mean_host [n],
 * var_host [n] (either may be NULL): what scikit-learn's KMeans takes from `X.mean(axis=0)` and `np.var(X, axis=0)` before the loop
 * above (sklearn/cluster/_kmeans.py: centring and `_tolerance`; reached from Koopman/koopmanEDMDc.py:85,126) -- mean_host is
 * edmdc_kmeans_lloyd_dev's `mean_host`, tol * mean(var_host) its tol_abs.  Two passes over X, fixed summation order: the values
 * depend on (N, n, x_stride) only.  Synchronous (the results are on the host on return). */
BROV_API int edmdc_col_stats_dev(brov_ctx* ctx, int64_t N, int n, const double* d_X, int64_t x_stride, double* mean_host,
                                 double* var_host);

/* k-means++ seeding on device: scikit-learn 1.7.2 `_kmeans_plusplus` with unit sample weights, i.e. the initialisation
 * of the KMeans(n_clusters, n_init="auto", random_state=0) that KoopmanEDMDc.fit constructs
 * (Koopman/koopmanEDMDc.py:85,126).  The random numbers are the caller's, in the order scikit-learn draws them from
 * its RandomState: first_index = random_state.choice(N, p=uniform), then uniforms[(c-1)*n_trials + j] =
 * random_state.uniform(size=n_trials)[j] for centre c = 1..k-1, n_trials = 2 + int(log(k)).  d_X [N][n] (row stride
 * x_stride), mean_host [n] subtracted from every row (NULL = none).  Outputs: d_C [k][n] (centred frame, device),
 * indices_host [k] = rows of X chosen (optional).  Same candidates as scikit-learn unless a drawn value falls within
 * rounding (~1e-13 relative) of a running-sum boundary. */
BROV_API int edmdc_kmeanspp_dev(brov_ctx* ctx, int64_t N, int n, int k, const double* d_X, int64_t x_stride,
                                const double* mean_host, int64_t first_index, int n_trials, const double* uniforms_host,
                                double* d_C, int64_t* indices_host);

/* KoopmanEDMDc.fit evaluates M = pinv(G^T G + ridge I) @ G.T @ Y left to right, i.e. (P G^T) Y
 * (Koopman/koopmanEDMDc.py:97), whereas fit_multi forms P (G^T Y) (:147).  The two differ by the conditioning of the Gram
 * (1e-6 in the H = 100 RMSE at the class defaults k = 200, ridge = 1e-8).  This entry point reproduces fit()'s order on
 * the device: P [p][p] is the host's pinv of the regularised Gram (from edmdc_gram), rows W = G P^T are formed chunk by
 * chunk (fp64 MFMA) and M [p][d] = W^T Y is accumulated over the same pairs as edmdc_gram.  Data layout as edmdc_gram. */
BROV_API int edmdc_pinv_apply(brov_ctx* ctx, int n, int r, int k, double gamma, const double* C,
                              int64_t nbags, int64_t L, int64_t x_bag_stride, int64_t u_bag_stride,
                              const double* X, const double* U, const double* P, double* M);
BROV_API int edmdc_pinv_apply_dev(brov_ctx* ctx, int n, int r, int k, double gamma, const double* d_C,
                                  int64_t nbags, int64_t L, int64_t x_bag_stride, int64_t u_bag_stride,
                                  const double* d_X, const double* d_U, const double* P_host, double* d_M);

/* edmdc_pinv_apply for the ragged bag list of edmdc_gram_ragged (fit()'s product order over fit_multi's data: what a caller gets who
 * wants the better-conditioned association on a trajectory list). */
BROV_API int edmdc_pinv_apply_ragged(brov_ctx* ctx, int n, int r, int k, double gamma, const double* C,
                                     int64_t nbags, const int64_t* bag_offsets, const double* X, const double* U,
                                     const double* P, double* M);
BROV_API int edmdc_pinv_apply_ragged_dev(brov_ctx* ctx, int n, int r, int k, double gamma, const double* d_C,
                                         int64_t nbags, const int64_t* bag_offsets, const double* d_X, const double* d_U,
                                         const double* P_host, double* d_M);

/* Work decomposition of edmdc_gram / edmdc_gram_dev for a shape (no device work; for roofline accounting): the normal
 * equations G^T[G|Y] (Koopman/koopmanEDMDc.py:129-147) are computed as ntasks blocks of 4 x 6 tiles of 16 x 16 per slab of
 * rows, nslabs slabs per chunk; a task executes 24 x 16 x 16 x 2 = 12 288 flop per sample whether a tile is wanted or not. */
BROV_API int edmdc_gram_decomposition(int n, int r, int k, int* ntasks, int* nslabs);
/* The same for edmdc_gram_dev called with d_GtY = NULL: G^T G alone, the Gram pass of KoopmanEDMDc.fit (which never forms G^T Y,
 * Koopman/koopmanEDMDc.py:89-97). */
BROV_API int edmdc_gtg_decomposition(int n, int r, int k, int* ntasks, int* nslabs);
/* The same for edmdc_pinv_apply(_dev), fit()'s own product order (Koopman/koopmanEDMDc.py:97): the rows of W = G P^T are
 * formed per unit of 192 rows by `wrows_items_per_192_rows` blocks of 4 x 6 tiles (`wrows_tiles_wanted` of their tile products
 * are wanted; a tile product is 16 x 16 x 16 x 2 flop per 16 rows = 512 flop per row), and W^T Y is accumulated by `wty_tasks`
 * blocks of 4 x 6 tiles per slab of rows, `wty_slabs` slabs per chunk (12 288 flop per sample and task). */
BROV_API int edmdc_apply_decomposition(int n, int r, int k, int* wrows_items_per_192_rows, int* wrows_tiles_wanted, int* wty_tasks, int* wty_slabs);
/* Lifted-row cache for the fit() sequence edmdc_gram_dev -> (host pinv) -> edmdc_pinv_apply_dev.  The caller lends the ctx a
 * device buffer (16-byte aligned; rows x (padded width + 1) x 8 bytes plus 8 rows of padding per chunk: 45.7 GB for 1e7 states at
 * k = 512 -- what 288 GB of HBM are for).  The next edmdc_gram_dev whose lifted chunks fit lifts them straight into it, and an
 * edmdc_pinv_apply_dev with the SAME pointers, shape, gamma and bag layout reads them back instead of lifting again.  The caller
 * promises not to modify X, U or C between the two calls and keeps the buffer alive until it is withdrawn (d_buffer = NULL).
 * Any other edmdc_gram_dev call invalidates the cached rows. */
BROV_API int edmdc_lift_cache(brov_ctx* ctx, void* d_buffer, size_t bytes);
/* Which kernel forms the rows of W in edmdc_pinv_apply(_dev): 0 = the tuned one (default), 1 = the plain one-row-tile-per-wave
 * form (kept as an independent second implementation for the parity tests; BROV2_APPLY_SIMPLE=1 selects it at brov_create). */
BROV_API int edmdc_set_apply_variant(brov_ctx* ctx, int variant);
/* Lloyd's loop in edmdc_kmeans_lloyd(_dev) -- a mask of three bits; every setting gives the same labels and the same centres, bit for bit
 * (integer member sums), so the non-default ones are the independent second implementations the parity tests compare against:
 *   0      default: E-step with the per-wave candidate filter (triangle inequality over the centre-centre distances) on a sample order
 *          kept sorted by (label, distance to the centre) -- a permutation, re-sorted as labels move; candidates screened in packed fp32
 *          in the frame of the wave's reference centre, exact fp64 only for the certified pair; Hamerly-style distance bounds let an
 *          E-step visit only the samples whose label could change (sorted order: >= 2^18 samples, n <= 14, k <= 512, or k <= 1024 for
 *          n = 12 / 13; bounds and screening: n = 12 / 13, k <= 512; anything else falls back to the plainer forms by itself);
 *   + 1    full scan over all k centres in the caller's order: no filter, no sorting, no bounds;
 *   + 2    candidate filter in the caller's order (no sorted sample order, hence no screening and no bounds);   (1 + 2 is refused)
 *   + 4    distance bounds off: every E-step visits every sample.
 * A library built with -DBROV2_EXPERIMENTS=1 (tools/, A/B measurements; brov_experiments_build() = 1) accepts further bits that swap
 * single stages for their earlier forms (csrc/capi.hip: KMV_*) and reads its tuning knobs from the environment; the default build
 * refuses those bits and reads no environment variable except BROV2_QUIET (silences the one note brov_create may print about the XCD
 * placement probe) and BROV2_RCCL_LIBRARY (below).
 * Changelog: up to round 4 `+ 4` selected the scalar-record kernel and `+ 8 .. + 256` were accepted by every build; since round 5 the
 * bits mean what is listed above and a caller passing the old values to a default build gets BROV_ERR_ARG. */
BROV_API int edmdc_set_kmeans_variant(brov_ctx* ctx, int variant);
/* When the distance bounds take over: an E-step visits only the samples whose bounds fail once at most `rate` of all labels changed in
 * the iteration before (default 0.03; 1 = from the first sorted iteration on, 0 = never).  Speed only: labels and centres do not depend
 * on it (tests/test_gpu_parity.py::test_lloyd_distance_bounds_change_nothing runs both ends). */
BROV_API int edmdc_set_kmeans_bounds_rate(brov_ctx* ctx, double rate);
BROV_API int brov_experiments_build(void);                          /* 1 for a -DBROV2_EXPERIMENTS=1 library */
/* Which samples `_relocate_empty_clusters_dense` moves its empty clusters to is
 * `np.argpartition(distances, -n_empty)[:-n_empty-1:-1]` (sklearn/cluster/_k_means_common.pyx): the selection algorithm decides the
 * order of the n_empty largest (which empty cluster gets which row) and the winner among equal distances -- and NumPy has two of them:
 * its own introselect (numpy/_core/src/npysort/selection.cpp) wherever no SIMD kernel is dispatched, x86-simd-sort's argselect on x86
 * hosts with AVX-512 / AVX2, with different answers.  Without a callback (fn = NULL: plain-C callers) the library applies a restatement
 * of the FORMER -- NumPy's introselect, step for step, pinned by tests/golden/farselect.npz (np.argpartition with its dispatch
 * disabled) and exported as edmdc_far_select_numpy.  The Python layer installs a callback that calls np.argpartition on the host at hand,
 * so that the rows are scikit-learn's on that host whatever it dispatches.  distances [N] (host), rows of the caller's X -- in a sharded
 * run (edmdc_set_kmeans_shard) the distances of ALL ranks' rows in global row order, N = n_global; far_rows_out [n_empty]; return 0 on
 * success. */
typedef int (*brov_far_select_fn)(void* user, const double* distances, int64_t N, int n_empty, int64_t* far_rows_out);
BROV_API int edmdc_set_kmeans_far_select(brov_ctx* ctx, brov_far_select_fn fn, void* user);
/* The library's own rule, host only: far_rows_out[q] = np.argpartition(distances, -n_empty)[N - 1 - q] as NumPy's introselect leaves it
 * (NaN = farthest).  1 <= n_empty <= N. */
BROV_API int edmdc_far_select_numpy(const double* distances, int64_t N, int n_empty, int64_t* far_rows_out);
/* relocations of empty clusters during the last edmdc_kmeans_lloyd(_dev) call (iterations in which at least one took place) */
BROV_API int edmdc_kmeans_relocations(brov_ctx* ctx);
/* How the last edmdc_kmeans_lloyd(_dev) call ran (speed only; none of it changes a result): info[0] = iterations with a relocation,
 * info[1] = re-sorts of the sample order, info[2] = iteration of the first re-sort (0 = none), info[3] = E-steps that visited only the
 * samples whose distance bounds failed.  Ranks of a sharded run report the same numbers. */
BROV_API int edmdc_kmeans_loop_info(brov_ctx* ctx, int info[4]);
/* Sharded Lloyd: every rank calls edmdc_kmeans_lloyd_dev on its own rows with the same initial centres; `fn` is called on the
 * ctx stream's behalf with a DEVICE buffer that has to be combined over all ranks in place before work queued later on the ctx
 * stream reads it: op 0 = sum of `count` int64, op 1 = maximum of `count` uint64.  One call with op 1 (16 words) before the loop,
 * one with op 0 (2 k (n + 1) + 2 words, 53 KB at k = 512) per iteration.  Integer sums: every rank gets the same centres, and
 * they are the centres of the unsharded run bit for bit.  fn = NULL: single rank.  Return 0 on success. */
typedef int (*brov_allreduce_fn)(void* user, void* d_buf, int64_t count, int op);
BROV_API int edmdc_set_kmeans_allreduce(brov_ctx* ctx, brov_allreduce_fn fn, void* user);
/* This rank's place in a sharded k-means: ranks hold contiguous shards of the rows in rank order, row_offset = global index of this
 * rank's first row, n_global = rows over all ranks (defaults: rank 0 of 1).  With an exchange installed (edmdc_set_kmeans_allreduce
 * or edmdc_kmeans_use_comm):
 *   edmdc_kmeanspp_dev seeds over ALL rows -- first_index and the returned indices are global, k <= n_global, every rank passes the
 *     same first_index and uniforms (drawn for n_global rows) and ends with the same centres; two small exchanges per centre (the
 *     ranks' partial potentials, the rows of the next candidates);
 *   edmdc_kmeans_lloyd_dev relocates empty clusters to the farthest rows of the WHOLE set: the ranks' distances are put side by side in
 *     global row order (one all-reduce of n_global words; this path runs when a cluster runs empty, i.e. hardly ever) and every rank applies
 *     the same selection -- the callback of edmdc_set_kmeans_far_select when one is installed, the library's rule otherwise -- to the same
 *     array, then the owner of each chosen row sends its label and coordinates (one small exchange per row): the rows, and with them the
 *     centres, of the unsharded run under the same rule. */
BROV_API int edmdc_set_kmeans_shard(brov_ctx* ctx, int rank, int world, int64_t row_offset, int64_t n_global);

/* ---- multi-GPU: one process per GPU, RCCL over xGMI ----------------------------------------
 * Rollouts shard over trajectories with no communication; the sharded EDMDc fit has exactly one exchange: the sum over
 * ranks of the local [GtG | GtY] blocks (4.5 MB at k = 512), after which every rank solves the same p x p system.
 * librccl is bound with dlopen at first use (a copy already mapped by the process, e.g. PyTorch's, is reused; with
 * BROV2_RCCL_LIBRARY set that path is the ONLY candidate -- when it cannot be opened brov_comm_available() is 0 and the
 * brov_comm_* calls return BROV_ERR_COMM, the rest of the library keeps working).  Rank 0 calls brov_comm_unique_id and hands the 128 bytes to the other ranks out of band
 * (file, socket, MPI, torch.distributed store ...); every rank then calls brov_comm_init_rank (collective, blocks until
 * all nranks have joined).  A communicator is bound to one device and is independent of any brov_ctx. */
#define BROV_COMM_ID_BYTES 128
typedef struct brov_comm brov_comm;
BROV_API int brov_comm_available(void);                               /* 1 if librccl could be bound */
BROV_API int brov_comm_unique_id(unsigned char id[BROV_COMM_ID_BYTES]);
BROV_API int brov_comm_init_rank(int device_id, const unsigned char id[BROV_COMM_ID_BYTES], int nranks, int rank, brov_comm** out);
BROV_API void brov_comm_destroy(brov_comm* comm);
BROV_API int brov_comm_nranks(const brov_comm* comm);
BROV_API int brov_comm_rank(const brov_comm* comm);
BROV_API const char* brov_comm_last_error(const brov_comm* comm);
/* In-place sum over all ranks of d_GtG (n_gtg doubles) and d_GtY (n_gty doubles), issued as ONE grouped RCCL all-reduce on
 * `hip_stream` (hipStream_t, NULL = null stream; asynchronous: order later work on the same stream or synchronise it). */
BROV_API int edmdc_gram_allreduce_dev(brov_comm* comm, double* d_GtG, int64_t n_gtg, double* d_GtY, int64_t n_gty, void* hip_stream);
/* In-place all-reduce of `count` 64-bit words on `hip_stream` (asynchronous): op 0 = sum of int64, op 1 = maximum of uint64. */
BROV_API int brov_comm_allreduce_words(brov_comm* comm, void* d_buf, int64_t count, int op, void* hip_stream);
/* Sharded Lloyd without torch: edmdc_kmeans_lloyd_dev on this ctx exchanges its member sums through `comm` (RCCL on the ctx stream);
 * the same as edmdc_set_kmeans_allreduce with a callback that calls brov_comm_allreduce_words.  comm = NULL: single rank again. */
BROV_API int edmdc_kmeans_use_comm(brov_ctx* ctx, brov_comm* comm);

#ifdef __cplusplus
}
#endif
#endif /* BROV2_H */
