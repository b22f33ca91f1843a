// pinc.hip -- inference of the PINc residual network (training/train_tank_brov2_full_comparison.py:601-721, 838-890):
// forward, rollouts (simulate_pinc) and the sliding-window evaluator (multistep_rmse_endpoint_pinc).
//
// Network (the shipped checkpoint's architecture, fp32 as the reference runs it): z = [x9, u4, dt] (14)
//   -> 4 x (Linear -> AdaptiveSoftplus -> LayerNorm(64)) -> Linear(64 -> 9) = dx,
//   x_next = z[:9] + dx with dx's x/y rotated body -> world by the input yaw and (cos, sin) renormalised (PINcNet.forward).
// Thruster map between steps: compute_thruster_forces in fp64 with the vehicle's stateful lag (the LagBank arithmetic of
// brov2_device.h, bit for bit what brov_thruster_forces computes), u4 = tau[0, 1, 2, 5] rounded to fp32.
//
// Mapping: ONE wave64 per trajectory / window, lane j = hidden unit j (the hidden width is the wave width).  Lane j holds row j of
// every hidden weight matrix in VGPRs (14 + 3 x 64 floats) and, for j < 9, row j of the output layer (64); the input of a layer is
// broadcast from the lanes with v_readlane, so a GEMV is 64 readlanes + 64 FMAs per lane and needs no LDS.  LayerNorm's two sums
// are DPP row reductions plus four readlanes; every lane ends with the same bits, so the wave-uniform state (x9, the endpoint) is
// identical in all lanes.  The eight thruster-lag filters live one per lane (lane & 7) in fp64; their forces are gathered with
// readlanes and allocated in brov2_device.h's order.  Waves loop over trajectories (grid-stride), loading the weights once.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "brov2_kernels.h"

namespace brov {
namespace {

constexpr int PINC_IN = 14, PINC_H = 64, PINC_OUT = 9;
// offsets in the packed blob (state-dict order: net.0.weight, net.0.bias, net.1.beta, net.2.weight, net.2.bias, net.3.weight ...)
constexpr int L0_W = 0, L0_B = 896, L0_BETA = 960, L0_G = 961, L0_BE = 1025;
constexpr int HID_BASE = 1089, HID_STRIDE = 4289;                 // layers 1..3: W [64][64], b, beta, ln.weight, ln.bias
constexpr int HID_B = 4096, HID_BETA = 4160, HID_G = 4161, HID_BE = 4225;
constexpr int OUT_W = 13956, OUT_B = 14532;
static_assert(OUT_B + PINC_OUT == PINC_NPARAMS, "blob layout");
constexpr int PINC_MAX_WAVES = 2048;                               // grid-stride cap (2 rounds of one wave per SIMD)

__device__ __forceinline__ float bcast(float v, int lane) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), lane)); }
__device__ __forceinline__ double bcast64(double v, int lane) {
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), lane), __builtin_amdgcn_readlane(__double2loint(v), lane));
}
template <int CTRL> __device__ __forceinline__ float dpp(float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xF, 0xF, true));
}
// sum over the 64 lanes, the same bits in every lane: pairs, quads, half rows, rows (DPP), then the four row sums
__device__ __forceinline__ float wave_sum(float v) {
    v += dpp<0xB1>(v);     // quad_perm [1,0,3,2]
    v += dpp<0x4E>(v);     // quad_perm [2,3,0,1]
    v += dpp<0x141>(v);    // row_half_mirror
    v += dpp<0x140>(v);    // row_mirror
    return (bcast(v, 0) + bcast(v, 16)) + (bcast(v, 32) + bcast(v, 48));
}

struct PincNet {
    float w0[PINC_IN];
    float w[3][PINC_H];
    float wo[PINC_H];
    float b[4], beta_div[4], beta[4], g[4], be[4];
    float bo;

    __device__ __forceinline__ void load(const float* __restrict__ W, int j) {
#pragma unroll
        for (int i = 0; i < PINC_IN; ++i) w0[i] = W[L0_W + j * PINC_IN + i];
        b[0] = W[L0_B + j]; beta[0] = W[L0_BETA]; g[0] = W[L0_G + j]; be[0] = W[L0_BE + j];
#pragma unroll
        for (int l = 0; l < 3; ++l) {
            const float* Wl = W + HID_BASE + l * HID_STRIDE;
#pragma unroll
            for (int i = 0; i < PINC_H; ++i) w[l][i] = Wl[j * PINC_H + i];
            b[l + 1] = Wl[HID_B + j]; beta[l + 1] = Wl[HID_BETA]; g[l + 1] = Wl[HID_G + j]; be[l + 1] = Wl[HID_BE + j];
        }
        const int o = j < PINC_OUT ? j : 0;                        // lanes >= 9 compute a discarded copy of output 0
#pragma unroll
        for (int i = 0; i < PINC_H; ++i) wo[i] = W[OUT_W + o * PINC_H + i];
        bo = W[OUT_B + o];
#pragma unroll
        for (int l = 0; l < 4; ++l) beta_div[l] = beta[l] + 1e-12f;    // AdaptiveSoftplus divides by the fp32 sum beta + 1e-12
    }

    // AdaptiveSoftplus (F.softplus threshold 20) then LayerNorm(64, eps 1e-5, biased variance, affine)
    __device__ __forceinline__ float act_norm(float a, int l) const {
        const float y = beta[l] * a;
        const float s = (y > 20.0f ? y : log1pf(expf(y))) / beta_div[l];
        const float mean = wave_sum(s) * (1.0f / PINC_H);
        const float d = s - mean;
        const float var = wave_sum(d * d) * (1.0f / PINC_H);
        return fmaf(d * (1.0f / sqrtf(var + 1e-5f)), g[l], be[l]);
    }

    __device__ __forceinline__ float gemv(const float (&wr)[PINC_H], float bias, float h) const {
        float a = bias;
#pragma unroll
        for (int i = 0; i < PINC_H; ++i) a = fmaf(wr[i], bcast(h, i), a);
        return a;
    }

    // PINcNet.forward for one row z (wave-uniform) -> x_next (wave-uniform)
    __device__ __forceinline__ void forward(const float z[PINC_IN], float xn[PINC_OUT]) const {
        float a = b[0];
#pragma unroll
        for (int i = 0; i < PINC_IN; ++i) a = fmaf(w0[i], z[i], a);
        float h = act_norm(a, 0);
#pragma unroll
        for (int l = 0; l < 3; ++l) h = act_norm(gemv(w[l], b[l + 1], h), l + 1);
        const float dlane = gemv(wo, bo, h);
        float dx[PINC_OUT];
#pragma unroll
        for (int o = 0; o < PINC_OUT; ++o) dx[o] = bcast(dlane, o);
        const float c = z[3], s = z[4];
        xn[0] = (c * dx[0] - s * dx[1]) + z[0];
        xn[1] = (s * dx[0] + c * dx[1]) + z[1];
        xn[2] = z[2] + dx[2];
        const float cb = z[3] + dx[3], sb = z[4] + dx[4];
        const float nrm = fmaxf(sqrtf(cb * cb + sb * sb), 1e-6f);
        xn[3] = cb / nrm;
        xn[4] = sb / nrm;
#pragma unroll
        for (int o = 5; o < PINC_OUT; ++o) xn[o] = z[o] + dx[o];
    }
};

// compute_thruster_forces for one sample: lane t = lane & 7 owns thruster t's lag filter (x[3], fp64);
// returns u4 = tau[0, 1, 2, 5] (wave-uniform, fp64) and advances the filter
__device__ __forceinline__ void thruster_u4(const DevParams& p, double x[3], double u_t, double u4[4]) {
    const double fcmd = thrust_poly(p, u_t);
    const double Ft = fma(p.lag_c[0][2], x[2], fma(p.lag_c[0][1], x[1], fma(p.lag_c[0][0], x[0], p.lag_d[0] * fcmd)));
    const double* A = p.lag_A[0];
    const double* bb = p.lag_b[0];
    const double a0 = x[0], a1 = x[1], a2 = x[2];
    x[0] = fma(A[2], a2, fma(A[1], a1, fma(A[0], a0, bb[0] * fcmd)));
    x[1] = fma(A[5], a2, fma(A[4], a1, fma(A[3], a0, bb[1] * fcmd)));
    x[2] = fma(A[8], a2, fma(A[7], a1, fma(A[6], a0, bb[2] * fcmd)));
    double F[8], tau[6];
#pragma unroll
    for (int i = 0; i < 8; ++i) F[i] = bcast64(Ft, i);
    allocate(p, F, tau);
    u4[0] = tau[0]; u4[1] = tau[1]; u4[2] = tau[2]; u4[3] = tau[5];
}

// dataset12_to_9 (fp64) rounded to fp32 as the reference's z cast does
__device__ __forceinline__ void x12_to_x9(const double* __restrict__ x12, float x9[PINC_OUT]) {
    double s, c;
    sincos(x12[5], &s, &c);
    x9[0] = (float)x12[0]; x9[1] = (float)x12[1]; x9[2] = (float)x12[2];
    x9[3] = (float)c; x9[4] = (float)s;
    x9[5] = (float)x12[6]; x9[6] = (float)x12[7]; x9[7] = (float)x12[8]; x9[8] = (float)x12[11];
}

// state9_to_12 in fp64: phi, theta, p, q = 0, psi = atan2(s, c)
__device__ __forceinline__ void x9_to_x12(const float x9[PINC_OUT], double x12[12]) {
    x12[0] = x9[0]; x12[1] = x9[1]; x12[2] = x9[2];
    x12[3] = 0.0; x12[4] = 0.0; x12[5] = atan2((double)x9[4], (double)x9[3]);
    x12[6] = x9[5]; x12[7] = x9[6]; x12[8] = x9[7];
    x12[9] = 0.0; x12[10] = 0.0; x12[11] = x9[8];
}

// one simulate_pinc step: thruster map (advances the lag), z = [x9, u4, dt] in fp32, x9 <- PINcNet(z)
__device__ __forceinline__ void pinc_step(const PincNet& net, const DevParams& p, float dtf, double lag[3], double u_t, float x9[PINC_OUT]) {
    double u4[4];
    thruster_u4(p, lag, u_t, u4);
    float z[PINC_IN];
#pragma unroll
    for (int i = 0; i < PINC_OUT; ++i) z[i] = x9[i];
#pragma unroll
    for (int i = 0; i < 4; ++i) z[PINC_OUT + i] = (float)u4[i];
    z[13] = dtf;
    net.forward(z, x9);
}

__device__ __forceinline__ void store_x12(double* __restrict__ dst, const double x[12]) {
#pragma unroll
    for (int i = 0; i < 12; i += 2) *reinterpret_cast<double2*>(dst + i) = make_double2(x[i], x[i + 1]);
}

__global__ void __launch_bounds__(64) pinc_forward_kernel(const float* __restrict__ W, int64_t B, const float* __restrict__ Z,
                                                          float* __restrict__ Xn) {
    const int j = threadIdx.x;
    PincNet net;
    net.load(W, j);
    for (int64_t b = blockIdx.x; b < B; b += gridDim.x) {
        float z[PINC_IN], xn[PINC_OUT];
#pragma unroll
        for (int i = 0; i < PINC_IN; ++i) z[i] = Z[b * PINC_IN + i];
        net.forward(z, xn);
        if (j == 0) {
#pragma unroll
            for (int i = 0; i < PINC_OUT; ++i) Xn[b * PINC_OUT + i] = xn[i];
        }
    }
}

// x0 [B][12], U [B][T][8], lag_io [B][8][3] (nullptr: zero, not returned), traj [B][T/stride+1][12] (optional), xT [B][12] (optional)
__global__ void __launch_bounds__(64) pinc_rollout_kernel(const float* __restrict__ W, DevParams p, int64_t B, int64_t T, double dt,
                                                          const double* __restrict__ X0, const double* __restrict__ U,
                                                          double* __restrict__ lag_io, double* __restrict__ traj, int64_t stride,
                                                          double* __restrict__ XT) {
    const int j = threadIdx.x, t8 = j & 7;
    const int64_t rows = T / stride + 1;
    const float dtf = (float)dt;
    PincNet net;
    net.load(W, j);
    for (int64_t b = blockIdx.x; b < B; b += gridDim.x) {
        double lag[3] = {0.0, 0.0, 0.0};
        if (lag_io) { lag[0] = lag_io[b * 24 + t8 * 3]; lag[1] = lag_io[b * 24 + t8 * 3 + 1]; lag[2] = lag_io[b * 24 + t8 * 3 + 2]; }
        double x12[12];
#pragma unroll
        for (int i = 0; i < 12; ++i) x12[i] = X0[b * 12 + i];
        float x9[PINC_OUT];
        x12_to_x9(x12, x9);
        if (traj && j == 0) store_x12(traj + b * rows * 12, x12);      // row 0 = x0 unchanged
        for (int64_t t = 0; t < T; ++t) {
            pinc_step(net, p, dtf, lag, U[(b * T + t) * 8 + t8], x9);
            if ((traj && (t + 1) % stride == 0) || t + 1 == T) {
                x9_to_x12(x9, x12);
                if (traj && (t + 1) % stride == 0 && j == 0) store_x12(traj + (b * rows + (t + 1) / stride) * 12, x12);
            }
        }
        if (XT && j == 0) store_x12(XT + b * 12, x12);
        if (lag_io && j < 8) { lag_io[b * 24 + j * 3] = lag[0]; lag_io[b * 24 + j * 3 + 1] = lag[1]; lag_io[b * 24 + j * 3 + 2] = lag[2]; }
    }
}

// zero-state response of window k's lag over its H samples, thruster space: resp [nwin][8][3]; one lane per (window, thruster)
__global__ void __launch_bounds__(256) pinc_lag_response_kernel(DevParams p, int64_t nwin, int64_t H, const double* __restrict__ U,
                                                                double* __restrict__ resp) {
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t k = g >> 3;
    const int i = (int)(g & 7);
    if (k >= nwin) return;
    double x[3] = {0.0, 0.0, 0.0};
    const double* A = p.lag_A[0];
    const double* bb = p.lag_b[0];
    for (int64_t t = 0; t < H; ++t) {
        const double f = thrust_poly(p, U[(k + t) * 8 + i]);
        const double a0 = x[0], a1 = x[1], a2 = x[2];
        x[0] = fma(A[2], a2, fma(A[1], a1, fma(A[0], a0, bb[0] * f)));
        x[1] = fma(A[5], a2, fma(A[4], a1, fma(A[3], a0, bb[1] * f)));
        x[2] = fma(A[8], a2, fma(A[7], a1, fma(A[6], a0, bb[2] * f)));
    }
    resp[g * 3] = x[0]; resp[g * 3 + 1] = x[1]; resp[g * 3 + 2] = x[2];
}

// window k: x0 = X[k], U[k .. k+H-1], lag from lag_start[k] (carry) or lag0 (every window, nullptr = zero); se[k] = |x_end - X[k+H]|^2
// (fp64, 12-D).  lag_final [8][3]: the last window's lag afterwards (the vehicle after the evaluator), when given.
__global__ void __launch_bounds__(64) pinc_window_kernel(const float* __restrict__ W, DevParams p, int64_t nwin, int64_t H, double dt,
                                                         const double* __restrict__ X, const double* __restrict__ U,
                                                         const double* __restrict__ lag_start, const double* __restrict__ lag0,
                                                         double* __restrict__ lag_final, double* __restrict__ se) {
    const int j = threadIdx.x, t8 = j & 7;
    const float dtf = (float)dt;
    PincNet net;
    net.load(W, j);
    for (int64_t k = blockIdx.x; k < nwin; k += gridDim.x) {
        double lag[3] = {0.0, 0.0, 0.0};
        const double* ls = lag_start ? lag_start + k * 24 : lag0;
        if (ls) { lag[0] = ls[t8 * 3]; lag[1] = ls[t8 * 3 + 1]; lag[2] = ls[t8 * 3 + 2]; }
        double x12[12];
#pragma unroll
        for (int i = 0; i < 12; ++i) x12[i] = X[k * 12 + i];
        float x9[PINC_OUT];
        x12_to_x9(x12, x9);
        for (int64_t t = 0; t < H; ++t) pinc_step(net, p, dtf, lag, U[(k + t) * 8 + t8], x9);
        if (H > 0) x9_to_x12(x9, x12);
        double e = 0.0;
#pragma unroll
        for (int i = 0; i < 12; ++i) { const double d = x12[i] - X[(k + H) * 12 + i]; e = fma(d, d, e); }
        if (j == 0) se[k] = e;
        if (lag_final && k == nwin - 1 && j < 8) { lag_final[j * 3] = lag[0]; lag_final[j * 3 + 1] = lag[1]; lag_final[j * 3 + 2] = lag[2]; }
    }
}

inline unsigned waves_for(int64_t n) { return (unsigned)(n < PINC_MAX_WAVES ? n : PINC_MAX_WAVES); }

}  // namespace

hipError_t launch_pinc_forward(hipStream_t st, const float* w, int64_t B, const float* z, float* x_next) {
    if (B <= 0) return hipSuccess;
    hipLaunchKernelGGL(pinc_forward_kernel, dim3(waves_for(B)), dim3(64), 0, st, w, B, z, x_next);
    return hipGetLastError();
}

hipError_t launch_pinc_rollout(hipStream_t st, const float* w, const DevParams& p, int64_t B, int64_t T, double dt, const double* x0,
                               const double* U, double* lag_io, double* traj, int64_t stride, double* xT) {
    if (B <= 0) return hipSuccess;
    hipLaunchKernelGGL(pinc_rollout_kernel, dim3(waves_for(B)), dim3(64), 0, st, w, p, B, T, dt, x0, U, lag_io, traj, stride, xT);
    return hipGetLastError();
}

hipError_t launch_pinc_window_endpoint(hipStream_t st, const float* w, const DevParams& p, int64_t N, int64_t H, double dt,
                                       const double* X, const double* U, int carry_lag, const double* d_phi, double* d_lag,
                                       double* d_chunk, double* d_lag_io, double* d_lag_starts, double* d_se, double* d_total) {
    const int64_t nwin = N - H;
    if (nwin <= 0) return hipSuccess;
    const double* lag_start = nullptr;
    if (carry_lag) {
        hipLaunchKernelGGL(pinc_lag_response_kernel, dim3((unsigned)((nwin * 8 + 255) / 256)), dim3(256), 0, st, p, nwin, H, U, d_lag);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
        e = launch_window_lag_scan(st, 8, 1, nwin, d_phi, d_lag, d_chunk, d_lag_io);      // responses -> start states, in place
        if (e != hipSuccess) return e;
        lag_start = d_lag;
        if (d_lag_starts) {
            e = hipMemcpyAsync(d_lag_starts, d_lag, (size_t)nwin * 24 * sizeof(double), hipMemcpyDeviceToDevice, st);
            if (e != hipSuccess) return e;
        }
    }
    // the last window's lag goes to d_lag_io only after every window has read its start (the kernel reads d_lag_io as lag0 when
    // !carry_lag, and the vehicle's lag is not advanced then)
    hipLaunchKernelGGL(pinc_window_kernel, dim3(waves_for(nwin)), dim3(64), 0, st, w, p, nwin, H, dt, X, U, lag_start,
                       carry_lag ? nullptr : d_lag_io, carry_lag ? d_lag_io : nullptr, d_se);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return launch_sum(st, nwin, d_se, d_total);
}

}  // namespace brov
