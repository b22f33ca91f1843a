// pinc_train.hip -- training of the PINc residual network (training/train_tank_brov2_full_comparison.py:724-835): the loss of one
// minibatch with its gradient over all 22 tensors, clip_grad_norm_ + AdamW, and the thruster map of one stateful vehicle over a
// whole recording (make_pinc_dataset's loop).
//
// One training iteration is two launches on the ctx stream:
//   pinc_grad_kernel   one wave64 per workgroup, lane j = hidden unit j (the mapping of pinc.hip).  Workgroup 0 runs the serial
//                      K-step rollout chain forward and back (its activations on an LDS tape); workgroup p >= 1 takes the batch
//                      rows p-1, p-1+nb, ...  Every workgroup holds its weight-gradient rows in VGPRs (lane j owns row j of dW) and
//                      ends by storing them, with its loss sums, as one partial [PINC_PART_STRIDE].
//   pinc_adamw_kernel  one workgroup: sums the partials in index order (no atomics, so the same inputs give the same bits), forms
//                      the 2-norm, clips, applies AdamW to w / m / v in place and stores the three loss terms.
// The hidden weight matrices live in LDS with a row stride of 65 floats: the forward GEMV (lane j reads row j) and the backward one
// (lane i reads column i) are both free of bank conflicts; the layer input is broadcast from the lanes with v_readlane.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "brov2_kernels.h"

namespace brov {
namespace {

constexpr int IN = 14, H = 64, OUT = 9;
constexpr int L0_W = 0, L0_B = 896, L0_BETA = 960, L0_G = 961, L0_BE = 1025;
constexpr int HID_BASE = 1089, HID_STRIDE = 4289;
constexpr int HID_B = 4096, HID_BETA = 4160, HID_G = 4161, HID_BE = 4225;
constexpr int OUT_W = 13956, OUT_B = 14532;
static_assert(OUT_B + OUT == PINC_NPARAMS, "blob layout");
constexpr int WS = 65;                       // LDS row stride of a hidden weight matrix
constexpr int ROWS_PER_WAVE = 8;             // batch rows per workgroup before more workgroups are added
constexpr int MAX_BATCH_WAVES = 255;

__device__ __forceinline__ float bcast(float v, int lane) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), lane)); }
template <int CTRL> __device__ __forceinline__ float dpp(float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xF, 0xF, true));
}
// sum over the 64 lanes, the same bits in every lane (pinc.hip's reduction)
__device__ __forceinline__ float wave_sum(float v) {
    v += dpp<0xB1>(v);
    v += dpp<0x4E>(v);
    v += dpp<0x141>(v);
    v += dpp<0x140>(v);
    return (bcast(v, 0) + bcast(v, 16)) + (bcast(v, 32) + bcast(v, 48));
}

// what one step leaves for its backward pass: per lane the pre-activation and the normalised value of every layer (LDS), and the
// wave-uniform rest (every lane writes the same value to the same word and later reads back what it wrote itself)
struct Tape {
    float lane[4][2][H];
    float rstd[4];
    float z[IN];
    float dx[OUT];
    float xn[OUT];
};

struct Net {
    float w0[IN];            // row j of the first layer
    float woT[OUT];          // column j of the output layer
    float b[4], g[4], be[4], beta[4], bdiv[4];
    float bo[OUT];

    __device__ __forceinline__ void load(const float* __restrict__ W, int j) {
#pragma unroll
        for (int i = 0; i < IN; ++i) w0[i] = W[L0_W + j * IN + i];
        b[0] = W[L0_B + j]; beta[0] = W[L0_BETA]; g[0] = W[L0_G + j]; be[0] = W[L0_BE + j];
#pragma unroll
        for (int l = 0; l < 3; ++l) {
            const float* Wl = W + HID_BASE + l * HID_STRIDE;
            b[l + 1] = Wl[HID_B + j]; beta[l + 1] = Wl[HID_BETA]; g[l + 1] = Wl[HID_G + j]; be[l + 1] = Wl[HID_BE + j];
        }
#pragma unroll
        for (int o = 0; o < OUT; ++o) { woT[o] = W[OUT_W + o * H + j]; bo[o] = W[OUT_B + o]; }
#pragma unroll
        for (int l = 0; l < 4; ++l) bdiv[l] = beta[l] + 1e-12f;
    }
};

struct Grad {
    float dw0[IN];
    float dw[3][H];          // row j of the hidden layers' dW
    float dwoT[OUT];
    float db[4], dg[4], dbe[4], dbeta[4];
    float dbo[OUT];

    __device__ __forceinline__ void zero() {
#pragma unroll
        for (int i = 0; i < IN; ++i) dw0[i] = 0.0f;
#pragma unroll
        for (int l = 0; l < 3; ++l)
#pragma unroll
            for (int i = 0; i < H; ++i) dw[l][i] = 0.0f;
#pragma unroll
        for (int o = 0; o < OUT; ++o) { dwoT[o] = 0.0f; dbo[o] = 0.0f; }
#pragma unroll
        for (int l = 0; l < 4; ++l) { db[l] = 0.0f; dg[l] = 0.0f; dbe[l] = 0.0f; dbeta[l] = 0.0f; }
    }
};

// PINcNet.forward for one row (z wave-uniform), recorded on `t`
__device__ __forceinline__ void forward(const Net& n, const float* __restrict__ sW, int j, const float z[IN], Tape& t, float xn[OUT]) {
    float a = n.b[0];
#pragma unroll
    for (int i = 0; i < IN; ++i) a = fmaf(n.w0[i], z[i], a);
    float h = 0.0f;
#pragma unroll
    for (int l = 0; l < 4; ++l) {
        if (l > 0) {
            const float* row = sW + (l - 1) * H * WS + j * WS;
            a = n.b[l];
#pragma unroll
            for (int i = 0; i < H; ++i) a = fmaf(row[i], bcast(h, i), a);
        }
        const float y = n.beta[l] * a;
        const float s = (y > 20.0f ? y : log1pf(expf(y))) / n.bdiv[l];
        const float mean = wave_sum(s) * (1.0f / H);
        const float d = s - mean;
        const float var = wave_sum(d * d) * (1.0f / H);
        const float rstd = 1.0f / sqrtf(var + 1e-5f);
        const float xh = d * rstd;
        h = fmaf(xh, n.g[l], n.be[l]);
        t.lane[l][0][j] = a;
        t.lane[l][1][j] = xh;
        t.rstd[l] = rstd;
    }
    float dx[OUT];
#pragma unroll
    for (int o = 0; o < OUT; ++o) dx[o] = wave_sum(n.woT[o] * h) + n.bo[o];
    const float c = z[3], s = z[4];
    xn[0] = (c * dx[0] - s * dx[1]) + z[0];
    xn[1] = (s * dx[0] + c * dx[1]) + z[1];
    xn[2] = z[2] + dx[2];
    const float cb = z[3] + dx[3], sb = z[4] + dx[4];
    const float nrm = fmaxf(sqrtf(cb * cb + sb * sb), 1e-6f);
    xn[3] = cb / nrm;
    xn[4] = sb / nrm;
#pragma unroll
    for (int o = 5; o < OUT; ++o) xn[o] = z[o] + dx[o];
#pragma unroll
    for (int i = 0; i < IN; ++i) t.z[i] = z[i];
#pragma unroll
    for (int o = 0; o < OUT; ++o) { t.dx[o] = dx[o]; t.xn[o] = xn[o]; }
}

// backward of one recorded step: gx = dL/dx_next (wave-uniform); accumulates into G; with WANT_DZ, dz[0..8] = dL/d(input state)
template <bool WANT_DZ>
__device__ __forceinline__ void backward(const Net& n, const float* __restrict__ sW, int j, const Tape& t, const float gx[OUT], Grad& G,
                                         float dz[OUT]) {
    float z[IN], dx[OUT];
#pragma unroll
    for (int i = 0; i < IN; ++i) z[i] = t.z[i];
#pragma unroll
    for (int o = 0; o < OUT; ++o) dx[o] = t.dx[o];
    const float c = z[3], s = z[4];
    // the renormalisation of (cos, sin): n = max(|(cb, sb)|, 1e-6); no derivative through n where the clamp is active
    const float cb = c + dx[3], sb = s + dx[4];
    const float r = sqrtf(cb * cb + sb * sb);
    const float nrm = fmaxf(r, 1e-6f);
    float dcb = gx[3] / nrm, dsb = gx[4] / nrm;
    if (r >= 1e-6f) {
        const float dn = -(gx[3] * cb + gx[4] * sb) / (nrm * nrm);      // dL/dn
        dcb = fmaf(dn, cb / r, dcb);
        dsb = fmaf(dn, sb / r, dsb);
    }
    float ddx[OUT];
    ddx[0] = gx[0] * c + gx[1] * s;
    ddx[1] = gx[1] * c - gx[0] * s;
    ddx[2] = gx[2];
    ddx[3] = dcb;
    ddx[4] = dsb;
#pragma unroll
    for (int o = 5; o < OUT; ++o) ddx[o] = gx[o];
    if (WANT_DZ) {
        dz[0] = gx[0]; dz[1] = gx[1]; dz[2] = gx[2];
        dz[3] = (gx[0] * dx[0] + gx[1] * dx[1]) + dcb;
        dz[4] = (gx[1] * dx[0] - gx[0] * dx[1]) + dsb;
#pragma unroll
        for (int o = 5; o < OUT; ++o) dz[o] = gx[o];
    }
    // output layer
    const float h4 = fmaf(t.lane[3][1][j], n.g[3], n.be[3]);
    float dh = 0.0f;
#pragma unroll
    for (int o = 0; o < OUT; ++o) {
        G.dwoT[o] = fmaf(ddx[o], h4, G.dwoT[o]);
        G.dbo[o] += ddx[o];
        dh = fmaf(n.woT[o], ddx[o], dh);
    }
#pragma unroll
    for (int l = 3; l >= 0; --l) {
        const float a = t.lane[l][0][j], xh = t.lane[l][1][j], rstd = t.rstd[l];
        // LayerNorm
        G.dg[l] = fmaf(dh, xh, G.dg[l]);
        G.dbe[l] += dh;
        const float dxh = dh * n.g[l];
        const float m1 = wave_sum(dxh) * (1.0f / H);
        const float m2 = wave_sum(dxh * xh) * (1.0f / H);
        const float ds = rstd * ((dxh - m1) - xh * m2);
        // AdaptiveSoftplus: s = softplus(beta a) / (beta + 1e-12)
        // d/dbeta = (sig a - softplus(y) / bdiv) / bdiv = (sig y - softplus(y)) / bdiv^2 where bdiv == beta in fp32 (always, unless
        // |beta| < 1e-5).  sig y and softplus(y) nearly cancel for large |y|; with u = exp(-|y|) their difference is
        // -(|y| u / (1 + u) + log1p(u)) for either sign of y, a sum of two terms of one sign.
        const float y = n.beta[l] * a;
        float sig = 1.0f, q = 0.0f, sp = y;
        if (!(y > 20.0f)) {
            const float u = expf(-fabsf(y)), r = u / (u + 1.0f), lu = log1pf(u);
            sig = y > 0.0f ? 1.0f - r : r;
            sp = y > 0.0f ? y + lu : lu;
            q = -fmaf(fabsf(y), r, lu);
        }
        const float da = ds * (sig * n.beta[l] / n.bdiv[l]);
        const float dsdbeta = n.bdiv[l] == n.beta[l] ? q / (n.bdiv[l] * n.bdiv[l]) : (sig * a - sp / n.bdiv[l]) / n.bdiv[l];
        G.dbeta[l] = fmaf(ds, dsdbeta, G.dbeta[l]);
        G.db[l] += da;
        if (l > 0) {
            const float hin = fmaf(t.lane[l - 1][1][j], n.g[l - 1], n.be[l - 1]);
            const float* col = sW + (l - 1) * H * WS + j;
            float acc = 0.0f;
#pragma unroll
            for (int i = 0; i < H; ++i) {
                G.dw[l - 1][i] = fmaf(da, bcast(hin, i), G.dw[l - 1][i]);
                acc = fmaf(col[i * WS], bcast(da, i), acc);
            }
            dh = acc;
        } else {
#pragma unroll
            for (int i = 0; i < IN; ++i) G.dw0[i] = fmaf(da, z[i], G.dw0[i]);
            if (WANT_DZ) {
#pragma unroll
                for (int i = 0; i < OUT; ++i) dz[i] += wave_sum(n.w0[i] * da);
            }
        }
    }
}

// sum of squares of the 4-DOF right-hand side (fossen/bluerov_torch.py with fossen/parameters.py) at x9 under u4, fp32
__device__ __forceinline__ float physics_sq(const float x[OUT], const float u4[4]) {
    constexpr double m = 11.4, g = 9.82, F_bouy = 1026 * 0.0115 * g;
    constexpr double X_ud = -2.6, Y_vd = -18.5, Z_wd = -13.3, N_rd = -0.28, I_zz = 0.245;
    constexpr double X_u = -0.09, Y_v = -0.26, Z_w = -0.19, N_r = -4.64;
    constexpr double X_uc = -34.96, Y_vc = -103.25, Z_wc = -74.23, N_rc = -0.43;
    const float c = x[3], s = x[4], u = x[5], v = x[6], w = x[7], r = x[8];
    float d[OUT];
    d[0] = c * u - s * v;
    d[1] = s * u + c * v;
    d[2] = w;
    d[3] = -s * r;
    d[4] = c * r;
    d[5] = (float)(1 / (m - X_ud)) * ((u4[0] + ((float)(m - Y_vd) * v) * r) + ((float)X_u + (float)X_uc * fabsf(u)) * u);
    d[6] = (float)(1 / (m - Y_vd)) * ((u4[1] - ((float)(m - X_ud) * u) * r) + ((float)Y_v + (float)Y_vc * fabsf(v)) * v);
    d[7] = (float)(1 / (m - Z_wd)) * (((u4[2] + ((float)Z_w + (float)Z_wc * fabsf(w)) * w) + (float)(m * g)) - (float)F_bouy);
    d[8] = (float)(1 / (I_zz - N_rd)) * ((u4[3] - ((float)(X_ud - Y_vd) * u) * v) + ((float)N_r + (float)N_rc * fabsf(r)) * r);
    float e = 0.0f;
#pragma unroll
    for (int o = 0; o < OUT; ++o) e = fmaf(d[o], d[o], e);
    return e;
}

// Z [*][14], Y [*][9], U4 [*][4] fp32; minibatch row r is row perm[r] of them (perm == nullptr: row r).  K rollout steps (0 = none).
// part [gridDim.x][PINC_PART_STRIDE]: the workgroup's gradient in blob order, then [sum of squared one-step errors, sum of squared
// right-hand sides, rollout loss].
__global__ void __launch_bounds__(64) pinc_grad_kernel(const float* __restrict__ W, int B, const float* __restrict__ Z,
                                                       const float* __restrict__ Y, const float* __restrict__ U4,
                                                       const int* __restrict__ perm, int K, int use_physics, float* __restrict__ part) {
    __shared__ float sW[3 * H * WS];
    __shared__ Tape tape[PINC_TRAIN_MAX_K];
    const int j = threadIdx.x;
    for (int l = 0; l < 3; ++l) {
        const float* Wl = W + HID_BASE + l * HID_STRIDE;
        for (int e = j; e < H * H; e += 64) sW[l * H * WS + (e >> 6) * WS + (e & 63)] = Wl[e];
    }
    Net net;
    net.load(W, j);
    Grad G;
    G.zero();
    __syncthreads();
    float mse = 0.0f, phys = 0.0f, roll = 0.0f;
    if (blockIdx.x == 0) {
        if (K > 0) {
            const int64_t r0 = perm ? perm[0] : 0;
            float z[IN], xn[OUT];
#pragma unroll
            for (int i = 0; i < OUT; ++i) z[i] = Z[r0 * IN + i];
            z[13] = Z[r0 * IN + 13];
            const float scale = 2.0f / (float)(OUT * K);
            for (int k = 0; k < K; ++k) {
                const int64_t rk = perm ? perm[k] : k;
#pragma unroll
                for (int i = 0; i < 4; ++i) z[OUT + i] = Z[rk * IN + OUT + i];
                forward(net, sW, j, z, tape[k], xn);
#pragma unroll
                for (int i = 0; i < OUT; ++i) z[i] = xn[i];
            }
            float carry[OUT];
#pragma unroll
            for (int i = 0; i < OUT; ++i) carry[i] = 0.0f;
            for (int k = K - 1; k >= 0; --k) {
                const int64_t rt = perm ? perm[k + 1] : k + 1;
                float gx[OUT], e = 0.0f;
#pragma unroll
                for (int i = 0; i < OUT; ++i) {
                    const float d = tape[k].xn[i] - Z[rt * IN + i];
                    e = fmaf(d, d, e);
                    gx[i] = fmaf(d, scale, carry[i]);
                }
                roll += e * (1.0f / OUT);
                backward<true>(net, sW, j, tape[k], gx, G, carry);
            }
            roll /= (float)K;
        }
    } else {
        const int nb = gridDim.x - 1;
        const float scale = 2.0f / ((float)B * (float)OUT);
        for (int r = blockIdx.x - 1; r < B; r += nb) {
            const int64_t row = perm ? perm[r] : r;
            float z[IN], xn[OUT], gx[OUT], dz[OUT];
#pragma unroll
            for (int i = 0; i < IN; ++i) z[i] = Z[row * IN + i];
            forward(net, sW, j, z, tape[0], xn);
#pragma unroll
            for (int i = 0; i < OUT; ++i) {
                const float d = xn[i] - Y[row * OUT + i];
                mse = fmaf(d, d, mse);
                gx[i] = d * scale;
            }
            if (use_physics) {
                float u4[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) u4[i] = U4[row * 4 + i];
                phys += physics_sq(xn, u4);
            }
            backward<false>(net, sW, j, tape[0], gx, G, dz);
        }
    }
    // the partial, in blob order
    float* P = part + (size_t)blockIdx.x * PINC_PART_STRIDE;
#pragma unroll
    for (int i = 0; i < IN; ++i) P[L0_W + j * IN + i] = G.dw0[i];
#pragma unroll
    for (int l = 0; l < 4; ++l) {
        const int base = l == 0 ? 0 : HID_BASE + (l - 1) * HID_STRIDE;
        P[base + (l == 0 ? L0_B : HID_B) + j] = G.db[l];
        P[base + (l == 0 ? L0_G : HID_G) + j] = G.dg[l];
        P[base + (l == 0 ? L0_BE : HID_BE) + j] = G.dbe[l];
        const float dbeta = wave_sum(G.dbeta[l]);
        if (j == 0) P[base + (l == 0 ? L0_BETA : HID_BETA)] = dbeta;
    }
#pragma unroll
    for (int l = 0; l < 3; ++l)
#pragma unroll
        for (int i = 0; i < H; ++i) P[HID_BASE + l * HID_STRIDE + j * H + i] = G.dw[l][i];
#pragma unroll
    for (int o = 0; o < OUT; ++o) P[OUT_W + o * H + j] = G.dwoT[o];
    if (j == 0) {
#pragma unroll
        for (int o = 0; o < OUT; ++o) P[OUT_B + o] = G.dbo[o];
        P[PINC_NPARAMS] = mse;
        P[PINC_NPARAMS + 1] = phys;
        P[PINC_NPARAMS + 2] = roll;
    }
}

struct AdamArgs {
    float decay;         // 1 - lr * weight_decay
    float one_m_b1, b2, one_m_b2;
    float step_size;     // lr / (1 - beta1^t)
    float bc2_sqrt;      // sqrt(1 - beta2^t)
    float eps, max_norm;
};

// g = sum over the nparts partials (index order); grad_out (optional) receives g unclipped; loss_out (optional) [3]; norm_out
// (optional) the 2-norm of g.  update: clip_grad_norm_(max_norm) then torch.optim.AdamW's step on w, m, v in place.
__global__ void __launch_bounds__(1024) pinc_adamw_kernel(int nparts, int stride, const float* __restrict__ part, int B,
                                                          float* __restrict__ grad_out, float* __restrict__ loss_out,
                                                          float* __restrict__ norm_out, int update, AdamArgs a, float* __restrict__ w,
                                                          float* __restrict__ m, float* __restrict__ v) {
    constexpr int PER = (PINC_NPARAMS + 1023) / 1024;
    __shared__ double sh[1024];
    const int tid = threadIdx.x;
    float g[PER];
    double ss = 0.0;
#pragma unroll
    for (int k = 0; k < PER; ++k) {
        const int e = tid + k * 1024;
        float s = 0.0f;
        if (e < PINC_NPARAMS) {
            for (int p = 0; p < nparts; ++p) s += part[(size_t)p * stride + e];
            if (grad_out) grad_out[e] = s;
        }
        g[k] = s;
        ss = fma((double)s, (double)s, ss);
    }
    sh[tid] = ss;
    __syncthreads();
    for (int s = 512; s > 0; s >>= 1) {
        if (tid < s) sh[tid] += sh[tid + s];
        __syncthreads();
    }
    const float norm = (float)sqrt(sh[0]);
    if (tid == 0) {
        if (norm_out) norm_out[0] = norm;
        if (loss_out) {
            double e = 0.0, ph = 0.0;
            for (int p = 1; p < nparts; ++p) { e += part[(size_t)p * stride + PINC_NPARAMS]; ph += part[(size_t)p * stride + PINC_NPARAMS + 1]; }
            const double cnt = (double)B * OUT;
            loss_out[0] = (float)(e / cnt);
            loss_out[1] = (float)(ph / cnt);
            loss_out[2] = part[PINC_NPARAMS + 2];
        }
    }
    if (!update) return;
    const float coef = fminf(a.max_norm / (norm + 1e-6f), 1.0f);
#pragma unroll
    for (int k = 0; k < PER; ++k) {
        const int e = tid + k * 1024;
        if (e >= PINC_NPARAMS) continue;
        const float gc = g[k] * coef;
        float p = w[e] * a.decay;
        float mm = m[e];
        mm = fmaf(gc - mm, a.one_m_b1, mm);
        const float vv = fmaf(a.one_m_b2 * gc, gc, v[e] * a.b2);
        const float denom = sqrtf(vv) / a.bc2_sqrt + a.eps;
        p = p - a.step_size * (mm / denom);
        w[e] = p; m[e] = mm; v[e] = vv;
    }
}

// ---- the thruster map of one vehicle over N consecutive samples ----
// resp[k][i] = Bd * F_cmd(U[k][i]): the lag recurrence x_{k+1} = Ad x_k + resp[k] of thruster i
__global__ void __launch_bounds__(256) stream_resp_kernel(DevParams p, int64_t N, const double* __restrict__ U, double* __restrict__ resp) {
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= N * 8) return;
    const double f = thrust_poly(p, U[g]);
    resp[g * 3] = p.lag_b[0][0] * f; resp[g * 3 + 1] = p.lag_b[0][1] * f; resp[g * 3 + 2] = p.lag_b[0][2] * f;
}

// start [N][8][3]: the lag before each sample -> tau [N][6]; the lag after the last sample goes to lag_io
__global__ void __launch_bounds__(256) stream_tau_kernel(DevParams p, int64_t N, const double* __restrict__ U, const double* __restrict__ start,
                                                         double* __restrict__ tau, double* __restrict__ lag_io) {
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= N) return;
    const double* A = p.lag_A[0];
    const double* bb = p.lag_b[0];
    double F[8], t6[6];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const double* x = start + (k * 8 + i) * 3;
        const double a0 = x[0], a1 = x[1], a2 = x[2];
        const double f = thrust_poly(p, U[k * 8 + i]);
        F[i] = fma(p.lag_c[0][2], a2, fma(p.lag_c[0][1], a1, fma(p.lag_c[0][0], a0, p.lag_d[0] * f)));
        if (k == N - 1) {
            lag_io[i * 3] = fma(A[2], a2, fma(A[1], a1, fma(A[0], a0, bb[0] * f)));
            lag_io[i * 3 + 1] = fma(A[5], a2, fma(A[4], a1, fma(A[3], a0, bb[1] * f)));
            lag_io[i * 3 + 2] = fma(A[8], a2, fma(A[7], a1, fma(A[6], a0, bb[2] * f)));
        }
    }
    allocate(p, F, t6);
#pragma unroll
    for (int i = 0; i < 6; ++i) tau[k * 6 + i] = t6[i];
}

}  // namespace

int pinc_grad_parts(int B) {
    int nb = (B + ROWS_PER_WAVE - 1) / ROWS_PER_WAVE;
    if (nb > MAX_BATCH_WAVES) nb = MAX_BATCH_WAVES;
    if (nb < 1) nb = 1;
    return nb + 1;
}

hipError_t launch_pinc_grad(hipStream_t st, const float* w, int B, const float* Z, const float* Y, const float* U4, const int* perm,
                            int K, int use_physics, float* part) {
    hipLaunchKernelGGL(pinc_grad_kernel, dim3(pinc_grad_parts(B)), dim3(64), 0, st, w, B, Z, Y, U4, perm, K, use_physics, part);
    return hipGetLastError();
}

hipError_t launch_pinc_reduce(hipStream_t st, int nparts, int stride, const float* part, int B, float* grad_out, float* loss_out,
                              float* norm_out, const PincAdam* ad, int64_t step, float* w, float* m, float* v) {
    AdamArgs a = {};
    if (ad) {
        const double bc1 = 1.0 - pow(ad->beta1, (double)step), bc2 = 1.0 - pow(ad->beta2, (double)step);
        a.decay = (float)(1.0 - ad->lr * ad->weight_decay);
        a.one_m_b1 = (float)(1.0 - ad->beta1);
        a.b2 = (float)ad->beta2;
        a.one_m_b2 = (float)(1.0 - ad->beta2);
        a.step_size = (float)(ad->lr / bc1);
        a.bc2_sqrt = (float)sqrt(bc2);
        a.eps = (float)ad->eps;
        a.max_norm = (float)ad->max_norm;
    }
    hipLaunchKernelGGL(pinc_adamw_kernel, dim3(1), dim3(1024), 0, st, nparts, stride, part, B, grad_out, loss_out, norm_out, ad ? 1 : 0, a,
                       w, m, v);
    return hipGetLastError();
}

hipError_t launch_thruster_stream(hipStream_t st, const DevParams& p, int64_t N, const double* U, const double* d_phi, double* d_lag,
                                  double* d_chunk, double* d_lag_io, double* tau) {
    if (N <= 0) return hipSuccess;
    hipLaunchKernelGGL(stream_resp_kernel, dim3((unsigned)((N * 8 + 255) / 256)), dim3(256), 0, st, p, N, U, d_lag);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    e = launch_window_lag_scan(st, 8, 1, N, d_phi, d_lag, d_chunk, d_lag_io);      // responses -> start states, in place
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(stream_tau_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, st, p, N, U, d_lag, tau, d_lag_io);
    return hipGetLastError();
}

}  // namespace brov
