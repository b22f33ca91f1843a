// rollout.hip -- time-loop kernels: batched RHS, Euler/RK4 rollouts, sliding-window
// endpoint error with the reference's carried thruster-lag state.
//
// Mapping: one wavefront lane = one trajectory (or one evaluation window); all state lives in VGPRs, nothing in scratch.
// Vehicle constants sit in a small device buffer (FastParams) read through the constant address space, i.e. as scalar
// loads.  Two forms of the rollout:
//   rollout_pair_kernel  thruster model, time-major layouts (the benchmark): every step split over the two waves of a SIMD
//                        -- thrust half and body half, LDS hand-over (K1p below);
//   rollout_kernel       every model, every layout: the whole step in one lane, control rows prefetched one step ahead;
//                        256-thread workgroups = one wave per SIMD at BASELINE config 2.
// One RK4 step of the thruster model executes ~760 fp64 VALU instructions per 64 trajectories (brov2_fast.h).
#include "brov2_device.h"
#include "brov2_fast.h"
#include "brov2_kernels.h"
#include "brov2_rows.h"

namespace brov {

constexpr int TRIG_REFRESH = 64;   // steps between full sin/cos evaluations of the carried attitude trig (power of two)

#if BROV_CLOCK_STAMPS
// Diagnostic build only (tools/attic/clock_probe.py; never in the shipped library): the body wave of every workgroup stamps the
// shader clock (s_memtime) and the constant 100 MHz clock (s_memrealtime) around its time loop; the ratio is the clock the
// chip holds under this launch.  The stamps go to a buffer of their own, no output value is computed from them.
__device__ unsigned long long g_clock_stamps[4096][4];
extern "C" __attribute__((visibility("default"))) int brov_debug_clock_stamps(unsigned long long* host, int nblocks) {
    return (int)hipMemcpyFromSymbol(host, HIP_SYMBOL(g_clock_stamps), sizeof(unsigned long long) * 4 * nblocks, 0, hipMemcpyDeviceToHost);
}
#endif

// ---------------------------------------------------------------------------------------
// global <-> register movement for one row of NX/NU doubles (load_row / store_row: brov2_rows.h)
// ---------------------------------------------------------------------------------------
template <int N>
__device__ __forceinline__ void load_soa(const double* __restrict__ src, int64_t ld, double* r) {
#pragma unroll
    for (int i = 0; i < N; ++i) r[i] = src[i * ld];
}
template <int N>
__device__ __forceinline__ void store_soa(double* __restrict__ dst, int64_t ld, const double* r) {
#pragma unroll
    for (int i = 0; i < N; ++i) dst[i * ld] = r[i];
}
// paired struct-of-arrays: element pair i of lane b lives at base[(i * B + b) * 2 .. +1]; `p` points at pair 0 of this lane
template <int N>
__device__ __forceinline__ void load_pairs(const double* __restrict__ p, int64_t ld2, double* r) {
#pragma unroll
    for (int i = 0; i < (N + 1) / 2; ++i) {
        // streamed once: nontemporal (slc) accesses keep the rows out of each other's way in L2 (-1 % kernel time)
        typedef double v2d __attribute__((ext_vector_type(2)));
        const v2d w = __builtin_nontemporal_load(reinterpret_cast<const v2d*>(p + i * ld2));
        const double2 v = make_double2(w[0], w[1]);
        r[2 * i] = v.x;
        if (2 * i + 1 < N) r[2 * i + 1] = v.y;
    }
}
template <int N>
__device__ __forceinline__ void store_pairs(double* __restrict__ p, int64_t ld2, const double* r) {
#pragma unroll
    for (int i = 0; i < (N + 1) / 2; ++i) {
        typedef double v2d __attribute__((ext_vector_type(2)));
        v2d w; w[0] = r[2 * i]; w[1] = (2 * i + 1 < N) ? r[2 * i + 1] : 0.0;
        __builtin_nontemporal_store(w, reinterpret_cast<v2d*>(p + i * ld2));
    }
}

// ---------------------------------------------------------------------------------------
// one integrator step (training/train_tank_brov2_full_comparison.py:462-465 Euler,
// training/train_tank_brov2_rk4.py:385-394 RK4, ..._wrench_quat.py:258-263 renormalisation)
// ---------------------------------------------------------------------------------------
template <int MODEL, int INTEG, int LAGMODE>
__device__ __forceinline__ void integrate_step(const DevParams& p, double dt, double* x, const double* u, LagBank& lag) {
    constexpr int NX = Dims<MODEL>::NX;
    constexpr bool THR = (MODEL == MODEL_THRUSTER_EULER);
    double fcmd[8], F[8], tau[6];
    if constexpr (THR) {
#pragma unroll
        for (int i = 0; i < 8; ++i) fcmd[i] = thrust_poly(p, u[i]);
    } else {
#pragma unroll
        for (int i = 0; i < 6; ++i) tau[i] = u[i];
    }
    if constexpr (INTEG == INTEG_EULER) {
        double k[NX];
        if constexpr (THR) { lag.forces_after(p, 1, fcmd, F); allocate(p, F, tau); }
        rhs_state<MODEL>(p, x, tau, k);
#pragma unroll
        for (int i = 0; i < NX; ++i) x[i] = fma(dt, k[i], x[i]);
        if constexpr (THR) lag.advance(p, 1, fcmd);
    } else {
        double k[NX], acc[NX], xs[NX];
        const double h2 = 0.5 * dt;
        if constexpr (THR) { lag.forces_after(p, 1, fcmd, F); allocate(p, F, tau); }
        rhs_state<MODEL>(p, x, tau, k);
#pragma unroll
        for (int i = 0; i < NX; ++i) { acc[i] = k[i]; xs[i] = fma(h2, k[i], x[i]); }
        if constexpr (THR && LAGMODE == 0) { lag.forces_after(p, 2, fcmd, F); allocate(p, F, tau); }
        rhs_state<MODEL>(p, xs, tau, k);
#pragma unroll
        for (int i = 0; i < NX; ++i) { acc[i] = fma(2.0, k[i], acc[i]); xs[i] = fma(h2, k[i], x[i]); }
        if constexpr (THR && LAGMODE == 0) { lag.forces_after(p, 3, fcmd, F); allocate(p, F, tau); }
        rhs_state<MODEL>(p, xs, tau, k);
#pragma unroll
        for (int i = 0; i < NX; ++i) { acc[i] = fma(2.0, k[i], acc[i]); xs[i] = fma(dt, k[i], x[i]); }
        if constexpr (THR && LAGMODE == 0) { lag.forces_after(p, 4, fcmd, F); allocate(p, F, tau); }
        rhs_state<MODEL>(p, xs, tau, k);
        const double h6 = dt / 6.0;
#pragma unroll
        for (int i = 0; i < NX; ++i) x[i] = fma(h6, acc[i] + k[i], x[i]);
        if constexpr (THR) lag.advance(p, LAGMODE == 0 ? 4 : 1, fcmd);
    }
    if constexpr (MODEL == MODEL_WRENCH_QUAT) quat_normalize(x + 3);
}

// ---------------------------------------------------------------------------------------
// K2: batched dynamics() -- one RHS evaluation per row, lag advanced one sample
// ---------------------------------------------------------------------------------------
template <int MODEL>
__global__ void __launch_bounds__(256) rhs_kernel(DevParams p, int64_t B, const double* __restrict__ X,
                                                  const double* __restrict__ U, double* __restrict__ lag_io,
                                                  double* __restrict__ XD, unsigned long long* done, unsigned long long seq) {
    constexpr int NX = Dims<MODEL>::NX, NU = Dims<MODEL>::NU;
    const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    double x[NX], u[NU], xd[NX], tau[6];
    load_row<NX>(X + b * NX, x);
    load_row<NU>(U + b * NU, u);
    if constexpr (MODEL == MODEL_THRUSTER_EULER) {
        LagBank lag;
        if (lag_io) load_row<24>(lag_io + b * 24, &lag.x[0][0]);
        else {
#pragma unroll
            for (int i = 0; i < 24; ++i) (&lag.x[0][0])[i] = 0.0;
        }
        double fcmd[8], F[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) fcmd[i] = thrust_poly(p, u[i]);
        lag.forces_after(p, 1, fcmd, F);
        allocate(p, F, tau);
        lag.advance(p, 1, fcmd);
        if (lag_io) store_row<24>(lag_io + b * 24, &lag.x[0][0]);
    } else {
#pragma unroll
        for (int i = 0; i < 6; ++i) tau[i] = u[i];
    }
    rhs_state<MODEL>(p, x, tau, xd);
    store_row<NX>(XD + b * NX, xd);
    // per-call path (capi.hip: brov_rhs with a handful of vehicles): the results live in host memory and the host spins on
    // done[b] instead of synchronising the stream -- release at system scope, after the row's stores
    if (done) __hip_atomic_store(done + b, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

// compute_thruster_forces (fossen/BlueROV2.py:265-278), batched
__global__ void __launch_bounds__(256) thruster_forces_kernel(DevParams p, int64_t B, const double* __restrict__ U,
                                                              double* __restrict__ lag_io, double* __restrict__ TAU,
                                                              unsigned long long* done, unsigned long long seq) {
    const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    double u[8], fcmd[8], F[8], tau[6];
    LagBank lag;
    load_row<8>(U + b * 8, u);
    load_row<24>(lag_io + b * 24, &lag.x[0][0]);
#pragma unroll
    for (int i = 0; i < 8; ++i) fcmd[i] = thrust_poly(p, u[i]);
    lag.forces_after(p, 1, fcmd, F);
    allocate(p, F, tau);
    lag.advance(p, 1, fcmd);
    store_row<24>(lag_io + b * 24, &lag.x[0][0]);
    store_row<6>(TAU + b * 6, tau);
    if (done) __hip_atomic_store(done + b, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

// ---------------------------------------------------------------------------------------
// K1: rollout.  U / traj layouts: BTU = [B][T][nu] / [B][rows][nx]; TUB = [T][nu][B] / [rows][nx][B].
// ---------------------------------------------------------------------------------------
template <int MODEL, int INTEG, int LAYOUT, int LAGMODE, bool TRACK, bool GENERIC>
__global__ void __launch_bounds__(256) rollout_kernel(const FastParams* __restrict__ pg, int64_t B, int64_t T, double dt,
                                                      const double* __restrict__ X0, const double* __restrict__ U,
                                                      double* __restrict__ lag_io, double* __restrict__ traj,
                                                      int64_t stride, double* __restrict__ XT) {
    constexpr int NX = Dims<MODEL>::NX, NU = Dims<MODEL>::NU;
    __shared__ double2 qt[4];
    init_quadrant_table(qt);
    __syncthreads();
    const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const CFP p = as_constant(pg);
    HotConsts h;
    load_hot(p, h);
    double x[NX];
    load_row<NX>(X0 + b * NX, x);
    LagZ lz;
    double Xl[8][3];
    if constexpr (MODEL == MODEL_THRUSTER_EULER) {
        if constexpr (TRACK) {
            load_row<24>(lag_io + b * 24, &Xl[0][0]);
            lz.from_thrusters(p, Xl);
        } else {
            lz.zero();
        }
        if constexpr (!GENERIC) lz.to_observer(p);
    }
    const int64_t rows = traj ? T / stride + 1 : 0;
    double* tp = nullptr;       // next trajectory row of this lane
    int64_t tstep = 0;          // distance between rows
    constexpr int NXP = (NX + 1) / 2, NUP = (NU + 1) / 2;
    if (traj) {
        if constexpr (LAYOUT == LAYOUT_BTU) { tp = traj + b * rows * NX; tstep = NX; }
        else if constexpr (LAYOUT == LAYOUT_TUB) { tp = traj + b; tstep = (int64_t)NX * B; }
        else { tp = traj + 2 * b; tstep = (int64_t)NXP * 2 * B; }
    }
    auto store_state = [&]() {
        if constexpr (LAYOUT == LAYOUT_BTU) store_row<NX>(tp, x);
        else if constexpr (LAYOUT == LAYOUT_TUB) store_soa<NX>(tp, B, x);
        else store_pairs<NX>(tp, 2 * B, x);
        tp += tstep;
    };
    const double* up;
    int64_t ustep;
    if constexpr (LAYOUT == LAYOUT_BTU) { up = U + b * T * NU; ustep = NU; }
    else if constexpr (LAYOUT == LAYOUT_TUB) { up = U + b; ustep = (int64_t)NU * B; }
    else { up = U + 2 * b; ustep = (int64_t)NUP * 2 * B; }

    double un[NU];
    if (T > 0) {
        if constexpr (LAYOUT == LAYOUT_BTU) load_row<NU>(up, un);
        else if constexpr (LAYOUT == LAYOUT_TUB) load_soa<NU>(up, B, un);
        else load_pairs<NU>(up, 2 * B, un);
    }
    // (storing the previous state at the top of the iteration, before the prefetch, measured 2 % slower)
    if (traj) store_state();
    int64_t countdown = stride;
    Trig tcarry;           // sin/cos of the attitude angles, carried from step to step (integrate_fast)
#if BROV_CLOCK_STAMPS
    const unsigned long long st0 = __builtin_amdgcn_s_memtime(), sr0 = __builtin_amdgcn_s_memrealtime();
#endif
    for (int64_t t = 0; t < T; ++t) {
        double u[NU];
#pragma unroll
        for (int i = 0; i < NU; ++i) u[i] = un[i];
        // prefetch the next control row while this step computes -- unconditionally: the last step re-reads its own row
        // (never consumed), so `un` is defined by one load on every path and costs no copy between register files
        up += (t + 1 < T) ? ustep : 0;
        {
            if constexpr (LAYOUT == LAYOUT_BTU) load_row<NU>(up, un);
            else if constexpr (LAYOUT == LAYOUT_TUB) load_soa<NU>(up, B, un);
            else load_pairs<NU>(up, 2 * B, un);
        }
        step_fast<MODEL, INTEG, LAGMODE, TRACK, GENERIC>(h, p, dt, x, u, lz, Xl, qt, &tcarry, (t & (TRIG_REFRESH - 1)) == 0);
        if (traj && --countdown == 0) {
            countdown = stride;
            store_state();
        }
    }
#if BROV_CLOCK_STAMPS
    if (threadIdx.x == 0 && blockIdx.x < 4096) {
        g_clock_stamps[blockIdx.x][0] = st0; g_clock_stamps[blockIdx.x][1] = sr0;
        g_clock_stamps[blockIdx.x][2] = __builtin_amdgcn_s_memtime(); g_clock_stamps[blockIdx.x][3] = __builtin_amdgcn_s_memrealtime();
    }
#endif
    if (XT) store_row<NX>(XT + b * NX, x);
    if constexpr (MODEL == MODEL_THRUSTER_EULER && TRACK) store_row<24>(lag_io + b * 24, &Xl[0][0]);
}

// ---------------------------------------------------------------------------------------
// K1 over a population of vehicles: grid (ceil(B / blockDim.x), P), candidate j = blockIdx.y runs B trajectories under pg[j].
// A sibling of rollout_kernel<.., LAYOUT_BTU, .., GENERIC = true> rather than a flag on it (the listings of the existing
// instantiations stay as they are); the step itself is the shared step_fast.  The candidate is uniform per block, so
// as_constant(pg + blockIdx.y) keeps every constant a scalar load, as in window_endpoint_kernel, and the GENERIC step serves
// mixed populations (a current, xb / yb, a dense allocation, obs_bad) with one kernel.  (x, per-thruster lag) is the whole
// checkpoint: sin/cos of the attitude are evaluated in full at every step (no carry, as in window_endpoint_kernel) and with TRACK
// the acceleration-space bank is formed from the per-thruster state at every step, so T1 + T2 steps in two launches give the bits
// of T1 + T2 steps in one.  Candidate j therefore equals rollout_kernel<.., GENERIC = true> under pg[j] to rounding, not bit for bit.
// Inputs shared (per_candidate = 0: X0 [B][nx], U [B][T][nu], every vehicle sees the same scenarios) or per candidate
// (X0 [P][B][nx], U [P][B][T][nu]); outputs always per candidate: traj [P][B][T/stride+1][nx], XT [P][B][nx], lag_io [P][B][24]
// (TRACK).  Launched with 64- or 256-thread blocks.
// ---------------------------------------------------------------------------------------
template <int MODEL, int INTEG, int LAGMODE, bool TRACK>
__global__ void __launch_bounds__(256) rollout_pop_kernel(const FastParams* __restrict__ pg, int64_t B, int64_t T, double dt,
                                                          const double* __restrict__ X0, const double* __restrict__ U, int per_candidate,
                                                          double* __restrict__ lag_io, double* __restrict__ traj, int64_t stride,
                                                          double* __restrict__ XT) {
    constexpr int NX = Dims<MODEL>::NX, NU = Dims<MODEL>::NU;
    __shared__ double2 qt[4];
    init_quadrant_table(qt);
    __syncthreads();
    const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const int64_t row = (int64_t)blockIdx.y * B + b;          // trajectory b of candidate blockIdx.y in the per-candidate arrays
    const int64_t in = per_candidate ? row : b;               // its row in X0 and U
    const CFP p = as_constant(pg + blockIdx.y);
    HotConsts h;
    load_hot(p, h);
    double x[NX];
    load_row<NX>(X0 + in * NX, x);
    LagZ lz;
    double Xl[8][3];
    if constexpr (MODEL == MODEL_THRUSTER_EULER) {
        if constexpr (TRACK) load_row<24>(lag_io + row * 24, &Xl[0][0]);
        else lz.zero();
    }
    double* tp = traj ? traj + row * (T / stride + 1) * NX : nullptr;      // next trajectory row of this lane
    const double* up = U + in * T * NU;
    double un[NU];
    if (T > 0) load_row<NU>(up, un);
    if (traj) { store_row<NX>(tp, x); tp += NX; }
    int64_t countdown = stride;
    for (int64_t t = 0; t < T; ++t) {
        double u[NU];
#pragma unroll
        for (int i = 0; i < NU; ++i) u[i] = un[i];
        // the next control row, as in rollout_kernel: the last step re-reads its own row
        up += (t + 1 < T) ? NU : 0;
        load_row<NU>(up, un);
        // the per-thruster state is the lag state: the acceleration-space bank is formed from it at every step, not carried
        if constexpr (MODEL == MODEL_THRUSTER_EULER && TRACK) lz.from_thrusters(relaunder(p), Xl);
        step_fast<MODEL, INTEG, LAGMODE, TRACK, true>(h, p, dt, x, u, lz, Xl, qt);
        if (traj && --countdown == 0) {
            countdown = stride;
            store_row<NX>(tp, x);
            tp += NX;
        }
    }
    if (XT) store_row<NX>(XT + row * NX, x);
    if constexpr (MODEL == MODEL_THRUSTER_EULER && TRACK) store_row<24>(lag_io + row * 24, &Xl[0][0]);
}

// ---------------------------------------------------------------------------------------
// K1p: thruster-model rollouts with every step split over TWO waves of one SIMD (time-major layouts).
//
// A lone wave issues one instruction of any kind every ~4.3 clocks (tools/gen_ubench_valu.py: fp64 FMA, mul, add, s_mov,
// v_mov, s_nop all cost the same slot, dependent or not), and BASELINE config 2 has exactly one wave of trajectories per
// SIMD, so in rollout_kernel every scalar instruction, every register-file shuffle and every wait comes straight out of the
// fp64 issue stream.  With two waves on a SIMD the fp64 pipe is still one instruction per ~4.15 clocks in total, but scalar
// instructions, waits and half of the move traffic of one wave disappear behind the fp64 work of the other.  The thruster
// model's step splits cleanly into two such streams (brov2_fast.h):
//   THRUST wave (waves 4-7 of a 512-thread workgroup): control row -> thrust polynomial -> allocation -> lag bank ->
//       the four accelerations a_s = Minv tau_s the step's four dynamics() calls will see (quirk Q1); never sees the state.
//       ~200 fp64 instructions per step, holds the control prefetch and all allocation / lag constants.
//   BODY wave (waves 0-3): rigid-body right-hand sides + RK4 + trajectory stores; reads a_s, never sees a control.
//       ~590 fp64 instructions per step, no lag state, no controls: ~70 VGPRs fewer than the one-lane form, nothing spills.
// Wave w and wave w + 4 serve the same 64 trajectories and (workgroup waves are dealt round-robin over the four SIMDs) share
// a SIMD.  The thrust wave runs one step ahead through a two-slot LDS exchange (24 doubles per lane and step, 16-byte
// accesses, conflict-free), one workgroup barrier per step:
//       thrust: produce a(0);  for t: barrier; produce a(t+1) -> slot (t+1)&1
//       body  :                for t: barrier; consume a(t)   <- slot t&1, integrate, store
// Slot (t+1)&1 was last read during step t-1, i.e. before the barrier the body wave has just passed.  The barrier waits for
// LDS traffic only (s_waitcnt lgkmcnt(0)): trajectory stores and control loads stay in flight across it.
// ---------------------------------------------------------------------------------------
#ifndef BROV_PAIR_EXP
#define BROV_PAIR_EXP 0          // experiments (tools/build_variants.py): 1 body wave alone, 3 thrust wave alone, 4 pairwise LDS flags
#endif
#ifndef BROV_PAIR_RING
#define BROV_PAIR_RING 2         // exchange slots (the flag form can run the thrust wave further ahead)
#endif
#ifndef BROV_PAIR_STAGE
#define BROV_PAIR_STAGE 1        // LAYOUT_BTU: stored states go through LDS and leave in contiguous runs (0: six 16-byte stores per lane and step)
#endif
#ifndef BROV_PAIR_PRIO
#define BROV_PAIR_PRIO 0         // 1: s_setprio 3 for the body wave, 0 for the thrust wave
#endif
__device__ __forceinline__ void pair_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// LAYOUT_TPB streams (control rows in, states out) addressed in the saddr form: a wave-uniform 64-bit base in SGPRs that advances one
// row per step with SALU, plus a fixed 32-bit offset per lane and pair (lane's pair 0 + i x pair stride).  The 64-bit VGPR address
// arithmetic of the plain form costs one VALU slot per access and step.  The offsets must fit 32 bits: pair_saddr_fits(B), checked by
// the launcher, which takes rollout_kernel for larger batches.
__host__ __device__ constexpr bool pair_saddr_fits(int64_t B) { return B > 0 && B <= (int64_t)((0xFFFFFFFFull - 64 * 16) / (5 * 16)); }
// The offset passes through an empty asm at each access, in place (a loop-carried register, no copy): a 32-bit value the compiler
// cannot widen once outside the loop -- it would then add two 64-bit registers per access, the plain form's VALU slot.
__device__ __forceinline__ uint64_t lane_offset(unsigned& o) { asm volatile("" : "+v"(o)); return o; }
typedef __attribute__((address_space(1))) char* gptr_t;         // global address space: global_* (not flat_*) instructions
__device__ __forceinline__ gptr_t wave_uniform(const void* ptr) {
    const uint64_t a = reinterpret_cast<uint64_t>(ptr);
    return (gptr_t)(((uint64_t)(unsigned)__builtin_amdgcn_readfirstlane((int)(a >> 32)) << 32) |
                    (uint64_t)(unsigned)__builtin_amdgcn_readfirstlane((int)(a & 0xFFFFFFFFull)));
}

template <int INTEG, int LAYOUT, int LAGMODE, bool TRACK, bool GENERIC>
__global__ void __launch_bounds__(512) rollout_pair_kernel(const FastParams* __restrict__ pg, int64_t B, int64_t T, double dt,
                                                           const double* __restrict__ X0, const double* __restrict__ U,
                                                           double* __restrict__ lag_io, double* __restrict__ traj,
                                                           int64_t stride, double* __restrict__ XT) {
    // LAYOUT_BTU (the callers' layout, round 3): lane-per-row accesses -- the thrust wave reads its trajectory's 64-byte control
    // row with four 16-byte loads, the body wave writes its 96-byte state row with six 16-byte stores.  A wave-instruction then
    // touches 64 cache lines instead of 8, which costs address-pipeline cycles but no issue slots: the instruction counts are
    // those of the time-major layouts, and the thrust wave's loads fall into its slack.
    constexpr int MODEL = MODEL_THRUSTER_EULER;
    constexpr int NX = 12, NU = 8, NXP = 6, NUP = 4;
    constexpr int NS = (INTEG == INTEG_RK4) ? 4 : 1;          // dynamics() calls per step
    __shared__ double2 qt[4];
    __shared__ __attribute__((aligned(16))) double2 xch[BROV_PAIR_RING][4][NS * 3][64];     // [slot][pair][stage, channel pair][lane]
    // LAYOUT_BTU, every state stored (round 6): a body wave parks STG_S consecutive states of its 64 trajectories in LDS (row q = trajectory
    // q, STG_S x 96 bytes + 16 of padding: conflict-free both ways) and writes them out with lanes ALONG the trajectories -- a store
    // instruction then covers 1 KB in runs of STG_S x 96 contiguous bytes (11 cache lines) instead of one 16-byte piece in each of 64 lines
    constexpr bool STG = (LAYOUT == LAYOUT_BTU) && BROV_PAIR_STAGE;
    constexpr int STG_S = 2, STG_ROW = STG_S * NXP + 1, STG_PER = STG_S * NXP;               // double2 per parked row; pieces per trajectory and tile
    __shared__ __attribute__((aligned(16))) double2 stg[STG ? 4 * 64 * STG_ROW : 1];
#if BROV_PAIR_EXP == 4
    __shared__ int pflag[2][4];                               // [produced | consumed][pair]: steps done so far
    if (threadIdx.x < 8) (&pflag[0][0])[threadIdx.x] = 0;
#endif
    init_quadrant_table(qt);
    __syncthreads();
    const int wave = threadIdx.x >> 6, pair = wave & 3, lane = threadIdx.x & 63;
    const bool thrust = wave >= 4;                            // wave-uniform
#if BROV_PAIR_PRIO
    if (thrust) __builtin_amdgcn_s_setprio(0); else __builtin_amdgcn_s_setprio(3);
#endif
    const int64_t b_raw = (int64_t)blockIdx.x * 256 + pair * 64 + lane;
    const bool live = b_raw < B;
    const int64_t b = live ? b_raw : B - 1;                   // dead lanes shadow the last trajectory, never store
    const CFP p = as_constant(pg);
    HotConstsResident h;
    load_hot(p, h);

    if (thrust) {
        LagZ lz;
        double Xl[8][3];
        if constexpr (TRACK) { load_row<24>(lag_io + b * 24, &Xl[0][0]); lz.from_thrusters(p, Xl); }
        else lz.zero();
        if constexpr (!GENERIC) lz.to_observer(p);
        const double* up = nullptr;
        int64_t ustep;
        if constexpr (LAYOUT == LAYOUT_BTU) { up = U + b * T * NU; ustep = NU; }
        else if constexpr (LAYOUT == LAYOUT_TUB) { up = U + b; ustep = (int64_t)NU * B; }
        else ustep = (int64_t)NUP * 2 * B;
        // LAYOUT_TPB: wave-uniform row base + per-lane offsets (pair_saddr_fits)
        const int64_t bw_c = (int64_t)blockIdx.x * 256 + pair * 64 < B ? (int64_t)blockIdx.x * 256 + pair * 64 : B - 1;
        gptr_t ub = LAYOUT == LAYOUT_TPB ? wave_uniform(U + 2 * bw_c) : nullptr;
        unsigned uoff[NUP];
#pragma unroll
        for (int i = 0; i < NUP; ++i) uoff[i] = (unsigned)((b - bw_c) * 16 + (int64_t)i * 16 * B);
        double un[NU];                                        // the controls of the next step to produce
        int64_t tl = 0;                                       // step whose controls sit in `un`
        auto load_controls = [&]() {
            if constexpr (LAYOUT == LAYOUT_BTU) load_row<NU>(up, un);
            else if constexpr (LAYOUT == LAYOUT_TUB) load_soa<NU>(up, B, un);
            else {
                typedef double v2d __attribute__((ext_vector_type(2)));
#pragma unroll
                for (int i = 0; i < NUP; ++i) {
                    const v2d w = __builtin_nontemporal_load(reinterpret_cast<const __attribute__((address_space(1))) v2d*>(ub + lane_offset(uoff[i])));
                    un[2 * i] = w[0]; un[2 * i + 1] = w[1];
                }
            }
        };
        if (T > 0) load_controls();
        auto produce = [&](int slot) {
            double fcmd[8], acmd[6], a[6];
            const CFP pp = relaunder(p);
            command_accel<MODEL, !GENERIC>(pp, un, fcmd, acmd);
            // the row is consumed: prefetch the next one into the same registers (no copy of the row); it has the rest of this
            // step and the next barrier to land.  The last step re-reads its own row, unused.
            if constexpr (LAYOUT == LAYOUT_TPB) ub += (tl + 1 != T) ? ustep * 8 : 0;     // (tl < T: a scalar compare)
            else up += (tl + 1 != T) ? ustep : 0;
            ++tl;
            load_controls();
#pragma unroll
            for (int s = 1; s <= NS; ++s) {
                lag_stage_accel<LAGMODE, GENERIC>(h, pp, lz, s, acmd, a);
#pragma unroll
                for (int j = 0; j < 3; ++j) xch[slot][pair][(s - 1) * 3 + j][lane] = make_double2(a[2 * j], a[2 * j + 1]);
            }
            lag_step_advance<INTEG, LAGMODE, TRACK, GENERIC>(relaunder(p), lz, fcmd, acmd, Xl);
        };
#if BROV_PAIR_EXP == 1                                        // experiment: the body wave alone (results are garbage)
        for (int64_t t = 0; t < T; ++t) pair_barrier();
        (void)produce;
#elif BROV_PAIR_EXP == 4                                      // experiment: pairwise flags instead of the workgroup barrier
        {
            volatile int* prodf = &pflag[0][pair];
            volatile int* consf = &pflag[1][pair];
            int slot = 0;
            for (int64_t s = 0; s < T; ++s) {
                if (s >= BROV_PAIR_RING) {
                    const int need = (int)(s - BROV_PAIR_RING + 1);
                    int spins = 0;
                    while (*consf < need && ++spins < (1 << 22)) __builtin_amdgcn_s_sleep(1);
                }
                asm volatile("" ::: "memory");
                produce(slot);
                asm volatile("" ::: "memory");
                *prodf = (int)(s + 1);
                slot = (slot + 1 == BROV_PAIR_RING) ? 0 : slot + 1;
            }
        }
#else
        // T barriers, the body wave's count: produce a(t) behind barrier t - 1
        if (T > 0) produce(0);
        for (int64_t t = 1; t < T; ++t) {
            pair_barrier();
            produce((int)(t & 1));
        }
        if (T > 0) pair_barrier();
#endif
        if constexpr (TRACK) { if (live) store_row<24>(lag_io + b * 24, &Xl[0][0]); }
    } else {
        double x[NX];
        load_row<NX>(X0 + b * NX, x);
        double* tp = nullptr;
        int64_t tstep = 0;
        if (traj) {
            if constexpr (LAYOUT == LAYOUT_BTU) { tp = traj + b * (T / stride + 1) * NX; tstep = NX; }
            else if constexpr (LAYOUT == LAYOUT_TUB) { tp = traj + b; tstep = (int64_t)NX * B; }
            else tstep = (int64_t)NXP * 2 * B;
        }
        // LAYOUT_TPB: wave-uniform row base + per-lane offsets (pair_saddr_fits).  Dead lanes shadow trajectory B - 1 and store its
        // values, bit for bit what lane B - 1 stores, so the stores need no lane mask.
        const int64_t sw_c = (int64_t)blockIdx.x * 256 + pair * 64 < B ? (int64_t)blockIdx.x * 256 + pair * 64 : B - 1;
        gptr_t sb = LAYOUT == LAYOUT_TPB ? wave_uniform(traj + 2 * sw_c) : nullptr;
        unsigned soff[NXP];
#pragma unroll
        for (int i = 0; i < NXP; ++i) soff[i] = (unsigned)((b - sw_c) * 16 + (int64_t)i * 16 * B);
        // staged stores (LAYOUT_BTU, stride 1).  Write-out of a tile: STG_PER = 12 lanes per trajectory, five trajectories per instruction (lanes
        // 60-63 idle), 13 instructions for the wave's 64 trajectories -- lane l always handles piece l % 12 of trajectory 5 it + l / 12, so
        // its global offset and LDS index are one register each plus a wave-uniform term per instruction
        const bool staged = STG && traj != nullptr && stride == 1 && (uint64_t)(T + 1) * (NX * 8) * 64 < (1ull << 32);
        const int64_t bw = (int64_t)blockIdx.x * 256 + pair * 64;          // first trajectory of this wave
        constexpr int STG_TPI = 64 / STG_PER, STG_NI = (64 + STG_TPI - 1) / STG_TPI;       // trajectories per instruction, instructions per tile
        const int st_q = lane / STG_PER, st_c = lane - st_q * STG_PER;
        const unsigned st_rb = (unsigned)((T + 1) * (NX * 8));             // bytes of one trajectory
        const unsigned st_off = (unsigned)st_q * st_rb + (unsigned)st_c * 16u;
        const int st_lds = st_q * STG_ROW + st_c;
        const int st_live = (int)((B - bw) < 64 ? (B - bw) : 64);          // trajectories of this wave that exist (wave-uniform)
        int st_fill = 0;
        char* st_base = nullptr;                                          // wave-uniform: row `rows flushed so far` of the wave's first trajectory
        double2* const st_wave = stg + (STG ? pair * 64 * STG_ROW : 0);
        if constexpr (STG) {
            if (staged) {
                const uint64_t a = reinterpret_cast<uint64_t>(traj) + (uint64_t)bw * (uint64_t)st_rb;
                st_base = reinterpret_cast<char*>(((uint64_t)(unsigned)__builtin_amdgcn_readfirstlane((int)(a >> 32)) << 32) |
                                                  (uint64_t)(unsigned)__builtin_amdgcn_readfirstlane((int)(a & 0xFFFFFFFFull)));
            }
        }
        auto st_flush = [&](int ns) {
            if constexpr (STG) {
                __builtin_amdgcn_wave_barrier();
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                if (ns == STG_S) {
#pragma unroll
                    for (int it = 0; it < STG_NI; ++it) {
                        if (lane < STG_TPI * STG_PER && it * STG_TPI + st_q < st_live) {
                            const double2 v = st_wave[st_lds + it * STG_TPI * STG_ROW];
                            *reinterpret_cast<double2*>(st_base + (uint64_t)(it * STG_TPI) * st_rb + st_off) = v;
                        }
                    }
                } else {                                                  // the last, shorter tile of a trajectory with an odd number of rows
                    const int per = ns * NXP;
                    for (int i = lane; i < 64 * per; i += 64) {
                        const int q = i / per, c = i - q * per;
                        const double2 v = st_wave[q * STG_ROW + c];
                        if (q < st_live) *reinterpret_cast<double2*>(st_base + (uint64_t)q * st_rb + (uint64_t)c * 16u) = v;
                    }
                }
                st_base += (int64_t)ns * (NX * 8);
                st_fill = 0;
                __builtin_amdgcn_wave_barrier();
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            }
        };
        auto store_state = [&]() {
            if constexpr (STG) {
                if (staged) {
                    double2* row = st_wave + lane * STG_ROW + st_fill * NXP;
#pragma unroll
                    for (int j = 0; j < NXP; ++j) row[j] = make_double2(x[2 * j], x[2 * j + 1]);
                    if (++st_fill == STG_S) st_flush(STG_S);
                    return;
                }
            }
            if constexpr (LAYOUT == LAYOUT_TPB) {
                typedef double v2d __attribute__((ext_vector_type(2)));
#pragma unroll
                for (int i = 0; i < NXP; ++i) {
                    v2d w; w[0] = x[2 * i]; w[1] = x[2 * i + 1];
                    __builtin_nontemporal_store(w, reinterpret_cast<__attribute__((address_space(1))) v2d*>(sb + lane_offset(soff[i])));
                }
                sb += tstep * 8;
                return;
            }
            if (live) {
                if constexpr (LAYOUT == LAYOUT_BTU) store_row<NX>(tp, x);
                else if constexpr (LAYOUT == LAYOUT_TUB) store_soa<NX>(tp, B, x);
            }
            tp += tstep;
        };
        if (traj) store_state();
        int64_t countdown = stride;
        Trig tcarry;
#if BROV_CLOCK_STAMPS
        const unsigned long long st0 = __builtin_amdgcn_s_memtime(), sr0 = __builtin_amdgcn_s_memrealtime();
#endif
#if BROV_PAIR_EXP == 4
        volatile int* prodf = &pflag[0][pair];
        volatile int* consf = &pflag[1][pair];
        int seen = 0, slot = 0;
#endif
        for (int64_t t = 0; t < T; ++t) {
#if BROV_PAIR_EXP == 3                                        // experiment: the thrust wave alone
            pair_barrier();
            const double2* src = &xch[t & 1][pair][0][lane];
            if (T >= 0) continue;
#elif BROV_PAIR_EXP == 4
            {
                int spins = 0;
                while (seen < (int)(t + 1) && ++spins < (1 << 22)) { seen = *prodf; if (seen < (int)(t + 1)) __builtin_amdgcn_s_sleep(1); }
            }
            asm volatile("" ::: "memory");
            const double2* src = &xch[slot][pair][0][lane];
            slot = (slot + 1 == BROV_PAIR_RING) ? 0 : slot + 1;
#else
            pair_barrier();
            const double2* src = &xch[t & 1][pair][0][lane];
#endif
            integrate_fast<MODEL, INTEG, GENERIC>(h, p, dt, x, [&](int s, double* a) {
#pragma unroll
                for (int j = 0; j < 3; ++j) { const double2 v = src[((s - 1) * 3 + j) * 64]; a[2 * j] = v.x; a[2 * j + 1] = v.y; }
            }, qt, &tcarry, (t & (TRIG_REFRESH - 1)) == 0);
#if BROV_PAIR_EXP == 4
            asm volatile("" ::: "memory");
            *consf = (int)(t + 1);                            // LDS requests of one wave are served in order: after the step's reads
            seen = *prodf;                                    // asked for now, looked at when the next step begins
#endif
            if (traj && --countdown == 0) {
                countdown = stride;
                store_state();
            }
        }
#if BROV_CLOCK_STAMPS
        if (wave == 0 && lane == 0 && blockIdx.x < 4096) {
            g_clock_stamps[blockIdx.x][0] = st0; g_clock_stamps[blockIdx.x][1] = sr0;
            g_clock_stamps[blockIdx.x][2] = __builtin_amdgcn_s_memtime(); g_clock_stamps[blockIdx.x][3] = __builtin_amdgcn_s_memrealtime();
        }
#endif
        if constexpr (STG) { if (staged && st_fill > 0) st_flush(st_fill); }
        if (XT && live) store_row<NX>(XT + b * NX, x);
    }
}

// ---------------------------------------------------------------------------------------
// K1b: rollout for the caller layout BTU (U[B][T][nu], traj[B][T+1][nx]) with LDS staging.
//
// Per trajectory the controls / states of consecutive steps are contiguous in memory but lanes
// are T*nu*8 bytes apart, so a lane-per-row access touches 64 cache lines per instruction.  Here
// each wave moves TILE steps at a time through its own LDS region:
//   in : global_load_lds_dwordx4 (LDS-DMA, no VGPRs, asynchronous, double buffered): one
//        wave-instruction copies 1 KiB = the next TILE*nu*8 contiguous bytes of 64/CH trajectories.
//        The DMA writes LDS linearly (slot = i*64 + lane), so the bank-conflict-free image is
//        obtained by permuting which 16-byte chunk of its trajectory a lane fetches
//        (chunk = c ^ ((j>>1)&7) for nu = 8) and reading with the same permutation.
//   out: every lane parks its state row in a padded LDS row; after TILE steps the wave writes the
//        tile out with 16-byte stores whose lanes walk along the trajectory rows (TILE*nx*8
//        contiguous bytes per trajectory).
// Lane <-> trajectory, all state in VGPRs, exactly as rollout_kernel.
// ---------------------------------------------------------------------------------------
constexpr int BTU_TILE = 2;

template <int NU> __device__ __forceinline__ int in_swizzle(int d, int j) {
    if constexpr (NU == 8) return d ^ ((j >> 1) & 7);   // conflict-free for ds_read_b128 (checked exhaustively)
    else return d;                                       // nu = 6: 2-way at worst
}

template <int MODEL, int INTEG, int LAGMODE, bool TRACK, bool GENERIC>
__global__ void __launch_bounds__(256) rollout_btu_lds_kernel(const FastParams* __restrict__ pg, int64_t B, int64_t T, double dt,
                                                              const double* __restrict__ X0, const double* __restrict__ U,
                                                              double* __restrict__ lag_io, double* __restrict__ traj,
                                                              double* __restrict__ XT) {
    constexpr int NX = Dims<MODEL>::NX, NU = Dims<MODEL>::NU;
    constexpr int CH = BTU_TILE * NU / 2;                 // 16-byte chunks per trajectory per input tile
    constexpr int IN_SLOTS = 64 * CH;                     // per wave per buffer
    constexpr int ORS = BTU_TILE * NX + 2;                // padded output row (doubles)
    constexpr int OCB = (NX % 2 == 0) ? 2 : 1;            // doubles per output chunk (16 B when rows stay 16-B aligned)
    constexpr int OCPR = BTU_TILE * NX / OCB;             // output chunks per trajectory per tile
    __shared__ __attribute__((aligned(16))) double lds_in[4][2][IN_SLOTS * 2];
    __shared__ __attribute__((aligned(16))) double lds_out[4][64 * ORS];
    __shared__ double2 qt[4];
    init_quadrant_table(qt);
    __syncthreads();

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t b0w = (int64_t)blockIdx.x * 256 + wave * 64;     // first trajectory of this wave
    const int64_t b_raw = b0w + lane;
    const bool live = b_raw < B;
    const int64_t b = live ? b_raw : B - 1;                        // dead lanes shadow the last trajectory, never store
    const CFP p = as_constant(pg);
    HotConsts h;
    load_hot(p, h);
    double x[NX];
    load_row<NX>(X0 + b * NX, x);
    LagZ lz;
    double Xl[8][3];
    if constexpr (MODEL == MODEL_THRUSTER_EULER) {
        if constexpr (TRACK) { load_row<24>(lag_io + b * 24, &Xl[0][0]); lz.from_thrusters(p, Xl); }
        else lz.zero();
        if constexpr (!GENERIC) lz.to_observer(p);
    }
    if (traj && live) store_row<NX>(traj + b * (T + 1) * NX, x);

    // issue the LDS-DMA of input tile `k` into buffer k&1
    auto issue_tile = [&](int64_t k) {
        const int64_t t0 = k * BTU_TILE;
#pragma unroll
        for (int i = 0; i < CH; ++i) {
            const int g = i * 64 + lane;
            const int j = g / CH, c = g % CH;
            const int d = in_swizzle<NU>(c, j);                    // data chunk this lane fetches
            int64_t bj = b0w + j;
            if (bj >= B) bj = B - 1;
            int64_t t = t0 + (2 * d) / NU;
            if (t >= T) t = T - 1;                                 // stay inside the buffer; value is never used
            const double* src = U + (bj * T + t) * NU + (2 * d) % NU;
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                             (__attribute__((address_space(3))) void*)(&lds_in[wave][k & 1][i * 128]), 16, 0, 0);
        }
    };

    const int64_t ntiles = (T + BTU_TILE - 1) / BTU_TILE;
    Trig tcarry;
    if (ntiles > 0) issue_tile(0);
    for (int64_t k = 0; k < ntiles; ++k) {
        __syncthreads();                     // tile k has landed (vmcnt(0)); last tile's LDS reads are finished
        if (k + 1 < ntiles) issue_tile(k + 1);
        const double* ib = &lds_in[wave][k & 1][0];
        double* ob = &lds_out[wave][lane * ORS];
        const int64_t t0 = k * BTU_TILE;
#pragma unroll 1
        for (int s = 0; s < BTU_TILE; ++s) {
            if (t0 + s < T) {
                double u[NU];
#pragma unroll
                for (int cc = 0; cc < NU / 2; ++cc) {
                    const int d = s * (NU / 2) + cc;
                    const double2 v = *reinterpret_cast<const double2*>(ib + (lane * CH + in_swizzle<NU>(d, lane)) * 2);
                    u[2 * cc] = v.x; u[2 * cc + 1] = v.y;
                }
                step_fast<MODEL, INTEG, LAGMODE, TRACK, GENERIC>(h, p, dt, x, u, lz, Xl, qt, &tcarry, ((t0 + s) & (TRIG_REFRESH - 1)) == 0);
                if (traj) store_row<NX>(ob + s * NX, x);
            }
        }
        if (traj) {
            __syncthreads();                 // the wave's output tile is complete
            const double* ot = &lds_out[wave][0];
#pragma unroll
            for (int i = 0; i < (64 * OCPR + 63) / 64; ++i) {
                const int g = i * 64 + lane;
                const int j = g / OCPR, c = g % OCPR;
                const int64_t bj = b0w + j;
                const int64_t row = t0 + 1 + (c * OCB) / NX;       // trajectory row of this chunk
                if (j < 64 && bj < B && row <= T) {
                    double* dst = traj + (bj * (T + 1) + t0 + 1) * NX + c * OCB;
                    const double* sp = ot + j * ORS + c * OCB;
                    if constexpr (OCB == 2) *reinterpret_cast<double2*>(dst) = *reinterpret_cast<const double2*>(sp);
                    else *dst = *sp;
                }
            }
        }
    }
    if (XT && live) store_row<NX>(XT + b * NX, x);
    if constexpr (MODEL == MODEL_THRUSTER_EULER && TRACK) { if (live) store_row<24>(lag_io + b * 24, &Xl[0][0]); }
}

// ---------------------------------------------------------------------------------------
// K3: sliding-window endpoint error (multistep_rmse_endpoint_physics,
// training/train_tank_brov2_full_comparison.py:469-487) for P parameter sets at once; one set (the ctx's own) is P = 1.
// Quirk Q2: the reference uses ONE vehicle object for all windows, so window k starts from the lag state window k-1 left.
// The lag bank is LTI and driven by the commands only, so:
//   (A) zero-state response b_k of each window (parallel over windows),
//   (B) x_{k+1} = Phi x_k + b_k, Phi = Ad^(samples per window)  (blocked scan, below),
//   (C) every window is an independent lane starting from its own x_k.
// pg is a FastParams[P] array; the candidate is blockIdx.y (blockIdx.x where one block serves a candidate), uniform per block,
// so as_constant(pg + blockIdx.y) keeps every constant read a scalar load.  Candidate j computes what
// brov_set_params(params[j]) + brov_window_endpoint_se computes.  The matrices of (B) are per candidate because the
// acceleration-space lag folds in Minv T.  Per-candidate arrays are candidate-major: lag [P][nwin][18], chunk [P][nchunks][18],
// phi [P][18], se [P][nwin], endpoints [P][nwin][NX].
//
// Several recordings ("bags", RAGGED = true): X and U hold the bags' rows one after the other, the windows are numbered bag after
// bag, and no window reads a row of another bag.  One map, built once per call by window_map_kernel, serves (A), (B) and (C):
// wrow [nwin] = the row window w starts at, and wopen [chunks] = bit i of word c set when window 64 c + i is the first of its
// bag (one word per scan chunk).  A lane pays one map load; the lanes of a wave still read consecutive rows except at a join.
// With carry_lag every bag is a fresh vehicle: (B) becomes a segmented scan that restarts from zero at every bag opening.
// RAGGED = false is the one-recording code, unchanged: window k starts at row k.
// ---------------------------------------------------------------------------------------
constexpr int WSCAN_CHUNK = 64;     // windows per chunk of the blocked scan (B), below
static_assert(WSCAN_CHUNK == 64, "wopen packs one scan chunk per 64-bit word, filled by one wave's ballot");

// tab = [wpre [nbags + 1] | off [nbags + 1]]: windows before bag b, and its first row.  Bags without a window are skipped:
// window w belongs to the last bag b with wpre[b] <= w.
__global__ void __launch_bounds__(256) window_map_kernel(int64_t nbags, const int64_t* __restrict__ tab, int64_t nwin,
                                                         int64_t* __restrict__ wrow, unsigned long long* __restrict__ wopen) {
    const int64_t w = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t* wpre = tab;
    const int64_t* off = tab + nbags + 1;
    bool open = false;
    if (w < nwin) {
        int64_t lo = 0, hi = nbags;                 // wpre[lo] <= w < wpre[hi]: wpre[0] = 0, wpre[nbags] = nwin
        while (hi - lo > 1) {
            const int64_t mid = (lo + hi) >> 1;
            if (wpre[mid] <= w) lo = mid; else hi = mid;
        }
        open = w == wpre[lo];
        wrow[w] = off[lo] + (w - wpre[lo]);
    }
    const unsigned long long m = __ballot(open);    // a wave = 64 consecutive windows = one scan chunk
    if ((threadIdx.x & 63) == 0 && w < nwin) wopen[w >> 6] = m;
}

// target [nwin][nx] = X[wrow[w] + H]: the rows the windows are scored against, for a caller that wants them without a candidate
__global__ void __launch_bounds__(256) window_target_kernel(int64_t nwin, int64_t H, int nx, const double* __restrict__ X,
                                                            const int64_t* __restrict__ wrow, double* __restrict__ target) {
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= nwin * nx) return;
    const int64_t w = g / nx;
    target[g] = X[(wrow[w] + H) * nx + (g - w * nx)];
}

template <int NSUB, bool RAGGED>
__global__ void __launch_bounds__(256) window_lag_response_kernel(const FastParams* __restrict__ pg, int64_t nwin, int64_t H,
                                                                  const double* __restrict__ U, double* __restrict__ resp,
                                                                  const int64_t* __restrict__ wrow) {
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= nwin) return;
    const int64_t r0 = RAGGED ? wrow[k] : k;        // first row of window k
    LagZ lz;
    lz.zero();
    for (int64_t t = 0; t < H; ++t) {
        const CFP pp = relaunder(as_constant(pg + blockIdx.y));
        double u[8], fcmd[8], acmd[6];
        load_row<8>(U + (r0 + t) * 8, u);
        command_accel<MODEL_THRUSTER_EULER, false>(pp, u, fcmd, acmd);
        lz.advance(NSUB == 4 ? pp->A4 : pp->A1, NSUB == 4 ? pp->b4 : pp->b1, acmd);
    }
    store_row<18>(resp + ((int64_t)blockIdx.y * nwin + k) * 18, &lz.z[0][0]);
}

// start[k] = lag state at the beginning of window k:
//     x_{k+1} = Phi x_k + b_k,  Phi = Ad^(samples per window), the same matrix for every window.
// Blocked scan over chunks of WSCAN_CHUNK windows, one lane per (chunk, lag bank):
//   (1) chunk_end[c]   = the recurrence over chunk c from a zero state               (parallel over chunks)
//   (2) chunk_start[c] : S_{c+1} = Phi^CHUNK S_c + chunk_end[c]                      (sequential over nwin/CHUNK chunks)
//   (3) start[k]       = the recurrence over chunk c from chunk_start[c]             (parallel over chunks)
// A single sequential pass over all windows (the first version) paid one exposed global-memory latency per window:
// 11 ms for the reference's 45 723 windows, more than everything else in the evaluator together.
// NC lag banks of 3 states per window: 6 wrench components (the Fossen evaluator, acceleration space) or 8 thrusters (the PINc
// evaluator and the thruster stream, pinc.hip / pinc_train.hip, thruster space).  phi [P][18] = [Phi | Phi^WSCAN_CHUNK].
__device__ __forceinline__ void wscan_step(const double P[9], double& x0, double& x1, double& x2, double b0, double b1, double b2) {
    const double n0 = fma(P[2], x2, fma(P[1], x1, fma(P[0], x0, b0)));
    const double n1 = fma(P[5], x2, fma(P[4], x1, fma(P[3], x0, b1)));
    const double n2 = fma(P[8], x2, fma(P[7], x1, fma(P[6], x0, b2)));
    x0 = n0; x1 = n1; x2 = n2;
}

// phases 1 (store_start = 0: chunk_io[c] <- end state of chunk c from zero) and 3 (store_start = 1: the chunk's start states,
// beginning from chunk_io[c]) for candidate blockIdx.y.  In place: phase 3 writes each start state over the response it has just
// consumed, so rs [P][nwin][NC][3] holds the responses on entry and the start states on exit.
// SEG (several bags): the state returns to zero at every bag-opening window (wopen, see above), so phase 1 measures a chunk from
// its last opening and phase 3 gives a bag's first window a zero start, the chunk's first window included.
template <int NC, bool SEG>
__global__ void __launch_bounds__(256) window_lag_chunk_kernel(int64_t nwin, int64_t nchunks, const double* __restrict__ phi,
                                                              double* rs, double* __restrict__ chunk_io, int store_start,
                                                              const unsigned long long* __restrict__ wopen) {
    constexpr int W = NC * 3;
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t c = g / NC;
    const int i = (int)(g - c * NC);
    const int64_t k0 = c * WSCAN_CHUNK;
    if (k0 >= nwin) return;
    const int64_t j = blockIdx.y;
    double P[9];
#pragma unroll
    for (int q = 0; q < 9; ++q) P[q] = phi[j * 18 + q];
    double* ce = chunk_io + (j * nchunks + c) * W + i * 3;
    double x0 = 0.0, x1 = 0.0, x2 = 0.0;
    if (store_start) { x0 = ce[0]; x1 = ce[1]; x2 = ce[2]; }
    const int64_t k1 = k0 + WSCAN_CHUNK < nwin ? k0 + WSCAN_CHUNK : nwin;
    unsigned long long om = 0;
    if constexpr (SEG) om = wopen[c];
    for (int64_t k = k0; k < k1; ++k) {
        double* r = rs + (j * nwin + k) * W + i * 3;
        const double r0 = r[0], r1 = r[1], r2 = r[2];
        if constexpr (SEG) {
            if ((om >> (k - k0)) & 1) { x0 = 0.0; x1 = 0.0; x2 = 0.0; }
        }
        if (store_start) { r[0] = x0; r[1] = x1; r[2] = x2; }
        wscan_step(P, x0, x1, x2, r0, r1, r2);
    }
    if (!store_start) { ce[0] = x0; ce[1] = x1; ce[2] = x2; }
}

// phase 2, one block per candidate: in place, chunk_io[c] (end-from-zero) -> state at the beginning of chunk c.
// s0 [NC][3]: state before the first window, the same for every candidate (nullptr = zero, a fresh vehicle).
// SEG: a chunk that holds a bag opening hands on what phase 1 measured from that opening, S_{c+1} = chunk_end[c]; the state that
// entered the chunk ended with the previous bag.
template <int NC, bool SEG>
__global__ void __launch_bounds__(64) window_lag_scan_kernel(int64_t nchunks, const double* __restrict__ phi, double* __restrict__ chunk_io,
                                                             const double* __restrict__ s0, const unsigned long long* __restrict__ wopen) {
    constexpr int W = NC * 3;
    const int i = threadIdx.x;  // lag bank
    if (i >= NC) return;
    const int64_t j = blockIdx.x;
    double P[9];
#pragma unroll
    for (int q = 0; q < 9; ++q) P[q] = phi[j * 18 + 9 + q];
    double x0 = 0.0, x1 = 0.0, x2 = 0.0;
    if (s0) { x0 = s0[i * 3]; x1 = s0[i * 3 + 1]; x2 = s0[i * 3 + 2]; }
    double* e = chunk_io + j * nchunks * W + i * 3;
    double b0 = 0, b1 = 0, b2 = 0;
    unsigned long long bo = 0;
    if (nchunks > 0) { b0 = e[0]; b1 = e[1]; b2 = e[2]; if constexpr (SEG) bo = wopen[0]; }
    for (int64_t c = 0; c < nchunks; ++c) {
        const double c0 = b0, c1 = b1, c2 = b2;
        const unsigned long long co = bo;
        if (c + 1 < nchunks) {
            b0 = e[(c + 1) * W + 0]; b1 = e[(c + 1) * W + 1]; b2 = e[(c + 1) * W + 2];
            if constexpr (SEG) bo = wopen[c + 1];
        }
        e[c * W + 0] = x0; e[c * W + 1] = x1; e[c * W + 2] = x2;
        if (SEG && co) { x0 = c0; x1 = c1; x2 = c2; }
        else wscan_step(P, x0, x1, x2, c0, c1, c2);
    }
}

// RAGGED: window k starts at row wrow[k]; target [nwin][NX] (optional) receives the rows the windows are scored against, written
// by the lanes of candidate 0.
template <int MODEL, int INTEG, bool RAGGED>
__global__ void __launch_bounds__(256) window_endpoint_kernel(const FastParams* __restrict__ pg, int64_t nwin, int64_t H, double dt,
                                                              const double* __restrict__ X, const double* __restrict__ U,
                                                              const double* __restrict__ lag_start, double* __restrict__ se,
                                                              double* __restrict__ endpoints, const int64_t* __restrict__ wrow,
                                                              double* __restrict__ target) {
    constexpr int NX = Dims<MODEL>::NX, NU = Dims<MODEL>::NU;
    __shared__ double2 qt[4];
    init_quadrant_table(qt);
    __syncthreads();
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= nwin) return;
    const int64_t row = (int64_t)blockIdx.y * nwin + k;       // window k of candidate blockIdx.y
    const int64_t r0 = RAGGED ? wrow[k] : k;                  // its first row in X and U
    const CFP p = as_constant(pg + blockIdx.y);
    HotConsts h;
    load_hot(p, h);
    double x[NX];
    load_row<NX>(X + r0 * NX, x);
    LagZ lz;
    double Xl[8][3];
    if constexpr (MODEL == MODEL_THRUSTER_EULER) {
        if (lag_start) load_row<18>(lag_start + row * 18, &lz.z[0][0]);
        else lz.zero();
    }
    for (int64_t t = 0; t < H; ++t) {
        double u[NU];
        load_row<NU>(U + (r0 + t) * NU, u);  // lane k reads row k+t: coalesced across the wave (ragged: except at a join)
        // full sin/cos at every step (no carry): the evaluator's windows are short, and recorded wrench sequences drive the
        // open-loop models far off the data (RMSE ~ 20), where every ulp is amplified.  The GENERIC step (current / xb, yb
        // branches) whatever the candidates' flags say: one kernel serves mixed populations, and this is not the benchmark path
        step_fast<MODEL, INTEG, 0, false, true>(h, p, dt, x, u, lz, Xl, qt);
    }
    double ref[NX], e = 0.0;
    load_row<NX>(X + (r0 + H) * NX, ref);
#pragma unroll
    for (int i = 0; i < NX; ++i) { const double d = x[i] - ref[i]; e = fma(d, d, e); }
    se[row] = e;
    if (endpoints) store_row<NX>(endpoints + row * NX, x);   // lane k writes row k of its candidate
    if constexpr (RAGGED) {
        if (target && blockIdx.y == 0) store_row<NX>(target + k * NX, ref);
    }
}

// Deterministic sum of n doubles per candidate blockIdx.x: fixed-shape tree, one block each.  out[j] = sum of v[j][0..n).
__global__ void __launch_bounds__(1024) sum_kernel(int64_t n, const double* __restrict__ v, double* __restrict__ out) {
    __shared__ double sh[1024];
    const double* vj = v + (int64_t)blockIdx.x * n;
    double a = 0.0;
    for (int64_t i = threadIdx.x; i < n; i += 1024) a += vj[i];
    sh[threadIdx.x] = a;
    __syncthreads();
    for (int s = 512; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) sh[threadIdx.x] += sh[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[blockIdx.x] = sh[0];
}

// Ensemble statistics over a population: vals [P][M] -> out [4][M] = mean, sample standard deviation (divisor P - 1; 0 when
// P = 1), minimum, maximum over the P candidates.  One thread per element m, two passes over j = 0..P-1 in index order (lanes
// read consecutive m: coalesced), no atomics: the same bits from run to run.  A non-finite value of any candidate at m makes all
// four outputs at m NaN.
__global__ void __launch_bounds__(256) ensemble_stats_kernel(int64_t P, int64_t M, const double* __restrict__ vals,
                                                             double* __restrict__ out) {
    const int64_t m = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= M) return;
    const double* v = vals + m;
    double s = 0.0, lo = v[0], hi = lo;
    bool finite = true;
    for (int64_t j = 0; j < P; ++j) {
        const double a = v[j * M];
        finite = finite && isfinite(a);
        s += a;
        lo = a < lo ? a : lo;
        hi = a > hi ? a : hi;
    }
    double mean = s / (double)P;
    double q = 0.0;
    for (int64_t j = 0; j < P; ++j) {
        const double d = v[j * M] - mean;
        q = fma(d, d, q);
    }
    double sd = P > 1 ? sqrt(q / (double)(P - 1)) : 0.0;
    if (!finite) mean = sd = lo = hi = __builtin_nan("");
    out[m] = mean;
    out[M + m] = sd;
    out[2 * M + m] = lo;
    out[3 * M + m] = hi;
}

// ---------------------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------------------
hipError_t launch_sum(hipStream_t st, int64_t n, const double* v, double* out) {
    hipLaunchKernelGGL(sum_kernel, dim3(1), dim3(1024), 0, st, n, v, out);
    return hipGetLastError();
}
static inline unsigned nblk(int64_t n, int bs) { return (unsigned)((n + bs - 1) / bs); }

#define BROV_LAUNCH_CHECK() do { hipError_t e_ = hipGetLastError(); if (e_ != hipSuccess) return e_; } while (0)

template <int MODEL>
static hipError_t launch_rhs_m(hipStream_t st, const DevParams& p, int64_t B, const double* x, const double* u, double* lag, double* xd,
                               unsigned long long* done, unsigned long long seq) {
    hipLaunchKernelGGL(rhs_kernel<MODEL>, dim3(nblk(B, 256)), dim3(256), 0, st, p, B, x, u, lag, xd, done, seq);
    return hipGetLastError();
}
hipError_t launch_rhs(hipStream_t st, const DevParams& p, int model, int64_t B, const double* x, const double* u, double* lag, double* xd,
                      unsigned long long* done, unsigned long long seq) {
    if (B <= 0) return hipSuccess;
    switch (model) {
        case MODEL_THRUSTER_EULER: return launch_rhs_m<MODEL_THRUSTER_EULER>(st, p, B, x, u, lag, xd, done, seq);
        case MODEL_WRENCH_EULER: return launch_rhs_m<MODEL_WRENCH_EULER>(st, p, B, x, u, lag, xd, done, seq);
        default: return launch_rhs_m<MODEL_WRENCH_QUAT>(st, p, B, x, u, lag, xd, done, seq);
    }
}
hipError_t launch_thruster_forces(hipStream_t st, const DevParams& p, int64_t B, const double* u, double* lag, double* tau,
                                  unsigned long long* done, unsigned long long seq) {
    if (B <= 0) return hipSuccess;
    hipLaunchKernelGGL(thruster_forces_kernel, dim3(nblk(B, 256)), dim3(256), 0, st, p, B, u, lag, tau, done, seq);
    return hipGetLastError();
}

template <int MODEL, int INTEG, int LAYOUT, int LAGMODE, bool TRACK, bool GENERIC>
static hipError_t launch_rollout_g(hipStream_t st, const FastParams* p, int64_t B, int64_t T, double dt, const double* x0,
                                   const double* U, double* lag, double* traj, int64_t stride, double* xT, bool want_lds, bool want_pair) {
    if constexpr (MODEL == MODEL_THRUSTER_EULER) {
        // the caller layout BTU takes the two-wave kernel where the one-lane kernel would use lane-per-row accesses anyway
        // (RK4: instruction-bound); the memory-bound Euler case keeps its LDS-staged kernel
        const bool staged_btu = LAYOUT == LAYOUT_BTU && (!traj || stride == 1) && T > 0 && want_lds;
        if (want_pair && !staged_btu && (LAYOUT != LAYOUT_TPB || pair_saddr_fits(B))) {
            hipLaunchKernelGGL((rollout_pair_kernel<INTEG, LAYOUT, LAGMODE, TRACK, GENERIC>), dim3(nblk(B, 256)), dim3(512), 0, st,
                               p, B, T, dt, x0, U, lag, traj, stride, xT);
            return hipGetLastError();
        }
    }
    if (LAYOUT == LAYOUT_BTU && (!traj || stride == 1) && T > 0 && want_lds)
        hipLaunchKernelGGL((rollout_btu_lds_kernel<MODEL, INTEG, LAGMODE, TRACK, GENERIC>), dim3(nblk(B, 256)), dim3(256), 0, st,
                           p, B, T, dt, x0, U, lag, traj, xT);
    else
        hipLaunchKernelGGL((rollout_kernel<MODEL, INTEG, LAYOUT, LAGMODE, TRACK, GENERIC>), dim3(nblk(B, 256)), dim3(256), 0, st,
                           p, B, T, dt, x0, U, lag, traj, stride, xT);
    return hipGetLastError();
}
template <int MODEL, int INTEG, int LAYOUT, int LAGMODE>
static hipError_t launch_rollout_t(hipStream_t st, const FastParams* p, int64_t B, int64_t T, double dt, const double* x0,
                                   const double* U, double* lag, double* traj, int64_t stride, double* xT, int btu_staging) {
    // LDS staging pays where the kernel is memory-bound (Euler, wrench models); the thruster RK4 kernel is
    // instruction-issue bound at one wave per SIMD and loses 14 % to the staging instructions
    const bool want_lds = (btu_staging & 3) == 1 || ((btu_staging & 3) == 0 && (INTEG == INTEG_EULER || MODEL != MODEL_THRUSTER_EULER));
    const bool generic = (btu_staging & 4) != 0;      // bit 2: vehicle has a current or xb/yb != 0 (set by the C ABI layer)
    const bool want_pair = (btu_staging & 8) == 0;    // bit 3: keep every step in one lane (A/B runs; set by the C ABI layer)
    constexpr bool DI = model_is_di(MODEL);
    if (MODEL == MODEL_THRUSTER_EULER && lag) {
        if constexpr (MODEL == MODEL_THRUSTER_EULER) {
            return generic ? launch_rollout_g<MODEL, INTEG, LAYOUT, LAGMODE, true, true>(st, p, B, T, dt, x0, U, lag, traj, stride, xT, want_lds, want_pair)
                           : launch_rollout_g<MODEL, INTEG, LAYOUT, LAGMODE, true, false>(st, p, B, T, dt, x0, U, lag, traj, stride, xT, want_lds, want_pair);
        }
    }
    if (generic && !DI) return launch_rollout_g<MODEL, INTEG, LAYOUT, LAGMODE, false, true>(st, p, B, T, dt, x0, U, lag, traj, stride, xT, want_lds, want_pair);
    return launch_rollout_g<MODEL, INTEG, LAYOUT, LAGMODE, false, false>(st, p, B, T, dt, x0, U, lag, traj, stride, xT, want_lds, want_pair);
}
template <int MODEL, int INTEG, int LAYOUT>
static hipError_t launch_rollout_l(hipStream_t st, const FastParams* p, int lag_mode, int64_t B, int64_t T, double dt,
                                   const double* x0, const double* U, double* lag, double* traj, int64_t stride, double* xT, int btu_staging) {
    if constexpr (MODEL == MODEL_THRUSTER_EULER && INTEG == INTEG_RK4) {
        if (lag_mode == 1) return launch_rollout_t<MODEL, INTEG, LAYOUT, 1>(st, p, B, T, dt, x0, U, lag, traj, stride, xT, btu_staging);
    }
    return launch_rollout_t<MODEL, INTEG, LAYOUT, 0>(st, p, B, T, dt, x0, U, lag, traj, stride, xT, btu_staging);
}
template <int MODEL>
static hipError_t launch_rollout_m(hipStream_t st, const FastParams* p, int integ, int lag_mode, int layout, int64_t B, int64_t T,
                                   double dt, const double* x0, const double* U, double* lag, double* traj, int64_t stride, double* xT, int btu_staging) {
    if (integ == INTEG_EULER) {
        if (layout == LAYOUT_BTU) return launch_rollout_l<MODEL, INTEG_EULER, LAYOUT_BTU>(st, p, lag_mode, B, T, dt, x0, U, lag, traj, stride, xT, btu_staging);
        if (layout == LAYOUT_TUB) return launch_rollout_l<MODEL, INTEG_EULER, LAYOUT_TUB>(st, p, lag_mode, B, T, dt, x0, U, lag, traj, stride, xT, btu_staging);
        return launch_rollout_l<MODEL, INTEG_EULER, LAYOUT_TPB>(st, p, lag_mode, B, T, dt, x0, U, lag, traj, stride, xT, btu_staging);
    }
    if (layout == LAYOUT_BTU) return launch_rollout_l<MODEL, INTEG_RK4, LAYOUT_BTU>(st, p, lag_mode, B, T, dt, x0, U, lag, traj, stride, xT, btu_staging);
    if (layout == LAYOUT_TUB) return launch_rollout_l<MODEL, INTEG_RK4, LAYOUT_TUB>(st, p, lag_mode, B, T, dt, x0, U, lag, traj, stride, xT, btu_staging);
    return launch_rollout_l<MODEL, INTEG_RK4, LAYOUT_TPB>(st, p, lag_mode, B, T, dt, x0, U, lag, traj, stride, xT, btu_staging);
}
hipError_t launch_rollout(hipStream_t st, const FastParams* p, int model, int integ, int lag_mode, int layout, int64_t B, int64_t T,
                          double dt, const double* x0, const double* U, double* lag, double* traj, int64_t stride, double* xT, int btu_staging) {
    if (B <= 0) return hipSuccess;
    switch (model) {
        case MODEL_THRUSTER_EULER: return launch_rollout_m<MODEL_THRUSTER_EULER>(st, p, integ, lag_mode, layout, B, T, dt, x0, U, lag, traj, stride, xT, btu_staging);
        case MODEL_WRENCH_EULER: return launch_rollout_m<MODEL_WRENCH_EULER>(st, p, integ, lag_mode, layout, B, T, dt, x0, U, lag, traj, stride, xT, btu_staging);
        case MODEL_WRENCH_QUAT: return launch_rollout_m<MODEL_WRENCH_QUAT>(st, p, integ, lag_mode, layout, B, T, dt, x0, U, lag, traj, stride, xT, btu_staging);
        case MODEL_DI_THRUSTER_EULER: return launch_rollout_m<MODEL_DI_THRUSTER_EULER>(st, p, integ, lag_mode, layout, B, T, dt, x0, U, nullptr, traj, stride, xT, btu_staging);
        case MODEL_DI_WRENCH_EULER: return launch_rollout_m<MODEL_DI_WRENCH_EULER>(st, p, integ, lag_mode, layout, B, T, dt, x0, U, nullptr, traj, stride, xT, btu_staging);
        default: return launch_rollout_m<MODEL_DI_WRENCH_QUAT>(st, p, integ, lag_mode, layout, B, T, dt, x0, U, nullptr, traj, stride, xT, btu_staging);
    }
}

// The population rollout: one launch, grid (blocks of B, P).  64-lane blocks when B <= 64, so that many vehicles with one or a
// few trajectories each do not launch 256-lane blocks with one live lane.  lag (thruster model) selects TRACK.
template <int MODEL, int INTEG, int LAGMODE>
static hipError_t launch_rollout_pop_t(hipStream_t st, const FastParams* p, int P, int per_candidate, int64_t B, int64_t T, double dt,
                                       const double* x0, const double* U, double* lag, double* traj, int64_t stride, double* xT) {
    const int bs = B <= 64 ? 64 : 256;
    const dim3 grid(nblk(B, bs), (unsigned)P);
    if constexpr (MODEL == MODEL_THRUSTER_EULER) {
        if (lag) {
            hipLaunchKernelGGL((rollout_pop_kernel<MODEL, INTEG, LAGMODE, true>), grid, dim3(bs), 0, st, p, B, T, dt, x0, U, per_candidate,
                               lag, traj, stride, xT);
            return hipGetLastError();
        }
    }
    hipLaunchKernelGGL((rollout_pop_kernel<MODEL, INTEG, LAGMODE, false>), grid, dim3(bs), 0, st, p, B, T, dt, x0, U, per_candidate,
                       nullptr, traj, stride, xT);
    return hipGetLastError();
}
template <int MODEL>
static hipError_t launch_rollout_pop_m(hipStream_t st, const FastParams* p, int integ, int lag_mode, int P, int per_candidate, int64_t B,
                                       int64_t T, double dt, const double* x0, const double* U, double* lag, double* traj, int64_t stride,
                                       double* xT) {
    if (integ == INTEG_EULER) return launch_rollout_pop_t<MODEL, INTEG_EULER, 0>(st, p, P, per_candidate, B, T, dt, x0, U, lag, traj, stride, xT);
    if constexpr (MODEL == MODEL_THRUSTER_EULER) {
        if (lag_mode == 1) return launch_rollout_pop_t<MODEL, INTEG_RK4, 1>(st, p, P, per_candidate, B, T, dt, x0, U, lag, traj, stride, xT);
    }
    return launch_rollout_pop_t<MODEL, INTEG_RK4, 0>(st, p, P, per_candidate, B, T, dt, x0, U, lag, traj, stride, xT);
}
hipError_t launch_rollout_pop(hipStream_t st, const FastParams* p, int model, int integ, int lag_mode, int P, int per_candidate, int64_t B,
                              int64_t T, double dt, const double* x0, const double* U, double* lag, double* traj, int64_t stride,
                              double* xT) {
    if (B <= 0 || P <= 0) return hipSuccess;
    switch (model) {
        case MODEL_THRUSTER_EULER: return launch_rollout_pop_m<MODEL_THRUSTER_EULER>(st, p, integ, lag_mode, P, per_candidate, B, T, dt, x0, U, lag, traj, stride, xT);
        case MODEL_WRENCH_EULER: return launch_rollout_pop_m<MODEL_WRENCH_EULER>(st, p, integ, lag_mode, P, per_candidate, B, T, dt, x0, U, nullptr, traj, stride, xT);
        case MODEL_WRENCH_QUAT: return launch_rollout_pop_m<MODEL_WRENCH_QUAT>(st, p, integ, lag_mode, P, per_candidate, B, T, dt, x0, U, nullptr, traj, stride, xT);
        default: return hipErrorInvalidValue;     // the double-integrator gains are not per-candidate parameters
    }
}

hipError_t launch_ensemble_stats(hipStream_t st, int64_t P, int64_t M, const double* vals, double* out) {
    if (P <= 0 || M <= 0) return hipSuccess;
    hipLaunchKernelGGL(ensemble_stats_kernel, dim3(nblk(M, 256)), dim3(256), 0, st, P, M, vals, out);
    return hipGetLastError();
}

int window_scan_chunk() { return WSCAN_CHUNK; }

// d_wopen != nullptr: the segmented scan over several bags (SEG), from a zero state
template <int NC, bool SEG>
static hipError_t launch_window_lag_scan_n(hipStream_t st, int P, int64_t nwin, const double* d_phi, double* d_rs, double* d_chunk,
                                           const double* d_s0, const unsigned long long* d_wopen) {
    const int64_t nchunks = (nwin + WSCAN_CHUNK - 1) / WSCAN_CHUNK;
    const dim3 gc(nblk(nchunks * NC, 256), (unsigned)P);
    hipLaunchKernelGGL((window_lag_chunk_kernel<NC, SEG>), gc, dim3(256), 0, st, nwin, nchunks, d_phi, d_rs, d_chunk, 0, d_wopen);
    BROV_LAUNCH_CHECK();
    hipLaunchKernelGGL((window_lag_scan_kernel<NC, SEG>), dim3((unsigned)P), dim3(64), 0, st, nchunks, d_phi, d_chunk, d_s0, d_wopen);
    BROV_LAUNCH_CHECK();
    hipLaunchKernelGGL((window_lag_chunk_kernel<NC, SEG>), gc, dim3(256), 0, st, nwin, nchunks, d_phi, d_rs, d_chunk, 1, d_wopen);
    return hipGetLastError();
}
hipError_t launch_window_lag_scan(hipStream_t st, int nc, int P, int64_t nwin, const double* d_phi, double* d_rs, double* d_chunk,
                                  const double* d_s0) {
    if (nwin <= 0 || P <= 0) return hipSuccess;
    return nc == 6 ? launch_window_lag_scan_n<6, false>(st, P, nwin, d_phi, d_rs, d_chunk, d_s0, nullptr)
                   : launch_window_lag_scan_n<8, false>(st, P, nwin, d_phi, d_rs, d_chunk, d_s0, nullptr);
}

template <int MODEL, bool RAGGED>
static hipError_t launch_window_m(hipStream_t st, const FastParams* p, int integ, int P, int64_t nwin, int64_t H, double dt,
                                  const double* X, const double* U, const double* lag_start, double* se, double* endpoints,
                                  const int64_t* wrow, double* target) {
    const dim3 grid(nblk(nwin, 256), (unsigned)P);
    if (integ == INTEG_RK4)
        hipLaunchKernelGGL((window_endpoint_kernel<MODEL, INTEG_RK4, RAGGED>), grid, dim3(256), 0, st, p, nwin, H, dt, X, U, lag_start, se,
                           endpoints, wrow, target);
    else
        hipLaunchKernelGGL((window_endpoint_kernel<MODEL, INTEG_EULER, RAGGED>), grid, dim3(256), 0, st, p, nwin, H, dt, X, U, lag_start, se,
                           endpoints, wrow, target);
    return hipGetLastError();
}

// (A) and (B) for the thruster model with carried lag (d_lag: responses, then start states), (C), and the per-candidate totals.
// d_wrow / d_wopen: the map of the ragged form (RAGGED), built by the caller's launch of window_map_kernel.
template <bool RAGGED>
static hipError_t launch_window_stages(hipStream_t st, const FastParams* p, int model, int integ, int P, int64_t nwin, int64_t H, double dt,
                                       const double* X, const double* U, int carry_lag, const double* d_phi, double* d_lag,
                                       double* d_chunk, double* d_se, double* d_total, double* d_endpoints, const int64_t* d_wrow,
                                       const unsigned long long* d_wopen, double* d_target) {
    const double* lag_start = nullptr;
    if (model == MODEL_THRUSTER_EULER && carry_lag) {
        const dim3 gw(nblk(nwin, 256), (unsigned)P);
        if (integ == INTEG_RK4)
            hipLaunchKernelGGL((window_lag_response_kernel<4, RAGGED>), gw, dim3(256), 0, st, p, nwin, H, U, d_lag, d_wrow);
        else
            hipLaunchKernelGGL((window_lag_response_kernel<1, RAGGED>), gw, dim3(256), 0, st, p, nwin, H, U, d_lag, d_wrow);
        BROV_LAUNCH_CHECK();
        const hipError_t e = launch_window_lag_scan_n<6, RAGGED>(st, P, nwin, d_phi, d_lag, d_chunk, nullptr, d_wopen);
        if (e != hipSuccess) return e;
        lag_start = d_lag;
    }
    hipError_t e;
    switch (model) {
        case MODEL_THRUSTER_EULER: e = launch_window_m<MODEL_THRUSTER_EULER, RAGGED>(st, p, integ, P, nwin, H, dt, X, U, lag_start, d_se, d_endpoints, d_wrow, d_target); break;
        case MODEL_WRENCH_EULER: e = launch_window_m<MODEL_WRENCH_EULER, RAGGED>(st, p, integ, P, nwin, H, dt, X, U, lag_start, d_se, d_endpoints, d_wrow, d_target); break;
        case MODEL_WRENCH_QUAT: e = launch_window_m<MODEL_WRENCH_QUAT, RAGGED>(st, p, integ, P, nwin, H, dt, X, U, lag_start, d_se, d_endpoints, d_wrow, d_target); break;
        case MODEL_DI_THRUSTER_EULER: e = launch_window_m<MODEL_DI_THRUSTER_EULER, RAGGED>(st, p, integ, P, nwin, H, dt, X, U, lag_start, d_se, d_endpoints, d_wrow, d_target); break;
        case MODEL_DI_WRENCH_EULER: e = launch_window_m<MODEL_DI_WRENCH_EULER, RAGGED>(st, p, integ, P, nwin, H, dt, X, U, lag_start, d_se, d_endpoints, d_wrow, d_target); break;
        default: e = launch_window_m<MODEL_DI_WRENCH_QUAT, RAGGED>(st, p, integ, P, nwin, H, dt, X, U, lag_start, d_se, d_endpoints, d_wrow, d_target); break;
    }
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(sum_kernel, dim3((unsigned)P), dim3(1024), 0, st, nwin, d_se, d_total);
    return hipGetLastError();
}

// Six launches with carry_lag on the thruster model, two otherwise, whatever P is.
hipError_t launch_window_endpoint(hipStream_t st, const FastParams* p, int model, int integ, int P, int64_t N, int64_t H, double dt,
                                  const double* X, const double* U, int carry_lag, const double* d_phi, double* d_lag,
                                  double* d_chunk, double* d_se, double* d_total, double* d_endpoints) {
    const int64_t nwin = N - H;
    if (nwin <= 0 || P <= 0) return hipSuccess;
    return launch_window_stages<false>(st, p, model, integ, P, nwin, H, dt, X, U, carry_lag, d_phi, d_lag, d_chunk, d_se, d_total,
                                       d_endpoints, nullptr, nullptr, nullptr);
}

// The same over several bags: one launch more (the map), whatever P and the number of bags are.  P = 0: the map and d_target only.
hipError_t launch_window_endpoint_ragged(hipStream_t st, const FastParams* p, int model, int integ, int P, int64_t nbags,
                                         const int64_t* d_tab, int64_t nwin, int64_t H, double dt, const double* X, const double* U,
                                         int carry_lag, const double* d_phi, double* d_lag, double* d_chunk, int64_t* d_wrow,
                                         unsigned long long* d_wopen, double* d_se, double* d_total, double* d_endpoints,
                                         double* d_target) {
    if (nwin <= 0 || P < 0) return hipSuccess;
    hipLaunchKernelGGL(window_map_kernel, dim3(nblk(nwin, 256)), dim3(256), 0, st, nbags, d_tab, nwin, d_wrow, d_wopen);
    BROV_LAUNCH_CHECK();
    if (P == 0) {
        if (!d_target) return hipSuccess;
        const int nx = model_is_quat(model) ? 13 : 12;
        hipLaunchKernelGGL(window_target_kernel, dim3(nblk(nwin * nx, 256)), dim3(256), 0, st, nwin, H, nx, X, d_wrow, d_target);
        return hipGetLastError();
    }
    return launch_window_stages<true>(st, p, model, integ, P, nwin, H, dt, X, U, carry_lag, d_phi, d_lag, d_chunk, d_se, d_total,
                                      d_endpoints, d_wrow, d_wopen, d_target);
}

// ---------------------------------------------------------------------------------------
// Finite-difference normal equations of the identification loop.  E [(m+1)][R] holds the window endpoints of the base
// parameters (row block 0) and of base + delta_j e_j (row block j + 1), R = W nx values each.  With
//     J[r][j] = w_i (E_{j+1}[r] - E_0[r]) / delta_j,   res[r] = w_i (E_0[r] - target[r]),   i = r mod nx,
// every block forms A = [J | res] for tiles of FDN_TILE rows in LDS and adds the tile's share of the upper triangle of A^T A
// (thread q owns entries q, q + 256, ...) to its own partial, tile after tile in index order; fd_normal_reduce_kernel adds the
// blocks' partials in index order.  No atomics: the same bits from run to run.
// ---------------------------------------------------------------------------------------
constexpr int FDN_TILE = 64, FDN_MAX_M = 48, FDN_THREADS = 256;
constexpr int FDN_MAX_Q = ((FDN_MAX_M + 1) * (FDN_MAX_M + 2) / 2 + FDN_THREADS - 1) / FDN_THREADS;   // entries per thread: 5

// entry q of the packed upper triangle of an n x n matrix -> (a, b), a <= b, row-major
__host__ __device__ inline void fdn_unpack(int q, int n, int& a, int& b) {
    a = 0;
    while (q >= n - a) { q -= n - a; ++a; }
    b = a + q;
}

__global__ void __launch_bounds__(FDN_THREADS) fd_normal_partial_kernel(int nx, int m, int64_t R, const double* __restrict__ E,
                                                                        const double* __restrict__ target,
                                                                        const double* __restrict__ delta,
                                                                        const double* __restrict__ weight, double* __restrict__ part) {
    __shared__ double tile[FDN_MAX_M + 1][FDN_TILE + 1];     // [column of A][row of the tile]; + 1: columns on different banks
    const int n = m + 1, npair = n * (n + 1) / 2;
    int ia[FDN_MAX_Q], ib[FDN_MAX_Q];
    double acc[FDN_MAX_Q];
#pragma unroll
    for (int s = 0; s < FDN_MAX_Q; ++s) {
        const int q = (int)threadIdx.x + s * FDN_THREADS;
        ia[s] = 0; ib[s] = 0; acc[s] = 0.0;
        if (q < npair) fdn_unpack(q, n, ia[s], ib[s]);
    }
    const int64_t ntiles = (R + FDN_TILE - 1) / FDN_TILE;
    for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const int64_t r0 = t * FDN_TILE;
        for (int idx = threadIdx.x; idx < n * FDN_TILE; idx += FDN_THREADS) {
            const int col = idx / FDN_TILE, lr = idx - col * FDN_TILE;
            const int64_t r = r0 + lr;
            double v = 0.0;
            if (r < R) {
                const double w = weight[r % nx], e0 = E[r];
                v = col < m ? w * (E[(int64_t)(col + 1) * R + r] - e0) / delta[col] : w * (e0 - target[r]);
            }
            tile[col][lr] = v;
        }
        __syncthreads();
#pragma unroll
        for (int s = 0; s < FDN_MAX_Q; ++s) {
            if ((int)threadIdx.x + s * FDN_THREADS < npair) {
                double ts = 0.0;
                for (int lr = 0; lr < FDN_TILE; ++lr) ts = fma(tile[ia[s]][lr], tile[ib[s]][lr], ts);
                acc[s] += ts;
            }
        }
        __syncthreads();
    }
#pragma unroll
    for (int s = 0; s < FDN_MAX_Q; ++s) {
        const int q = (int)threadIdx.x + s * FDN_THREADS;
        if (q < npair) part[(int64_t)blockIdx.x * npair + q] = acc[s];
    }
}

// out = [JtJ (m x m, both triangles) | Jtr (m)]
__global__ void __launch_bounds__(FDN_THREADS) fd_normal_reduce_kernel(int m, int nblocks, const double* __restrict__ part, double* __restrict__ out) {
    const int n = m + 1, npair = n * (n + 1) / 2;
    const int q = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (q >= npair) return;
    double s = 0.0;
    for (int g = 0; g < nblocks; ++g) s += part[(int64_t)g * npair + q];
    int a, b;
    fdn_unpack(q, n, a, b);
    if (b < m) { out[a * m + b] = s; out[b * m + a] = s; }
    else if (a < m) out[m * m + a] = s;
}

int fd_normal_blocks(int64_t R) {
    const int64_t ntiles = (R + FDN_TILE - 1) / FDN_TILE;
    return (int)(ntiles < 1 ? 1 : (ntiles > 512 ? 512 : ntiles));
}

// d_part: fd_normal_blocks(R) x (m + 1)(m + 2) / 2 doubles; d_out: m m + m doubles
hipError_t launch_fd_normal_eq(hipStream_t st, int nx, int m, int64_t R, const double* d_E, const double* d_target, const double* d_delta,
                               const double* d_weight, double* d_part, double* d_out) {
    const int nb = fd_normal_blocks(R), npair = (m + 1) * (m + 2) / 2;
    hipLaunchKernelGGL(fd_normal_partial_kernel, dim3(nb), dim3(FDN_THREADS), 0, st, nx, m, R, d_E, d_target, d_delta, d_weight, d_part);
    BROV_LAUNCH_CHECK();
    hipLaunchKernelGGL(fd_normal_reduce_kernel, dim3(nblk(npair, FDN_THREADS)), dim3(FDN_THREADS), 0, st, m, nb, d_part, d_out);
    return hipGetLastError();
}

}  // namespace brov
