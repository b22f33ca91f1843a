// brov2_lift.h -- the RBF lift of one state row against one or several centres (Koopman/koopmanEDMDc.py:41-48, the expanded distance
// form), shared by edmdc.hip and koopman_mppi.hip: the same code, so the same bits wherever a state is lifted
#pragma once
#include <hip/hip_runtime.h>

namespace brov {

constexpr int LIFT_NMAX = 16;   // max state dimension held in registers per centre

// exp(x): k = rint(x / ln 2), r = x - k ln2 (two-constant Cody-Waite), degree-13 Taylor on |r| <= ln2/2
// (truncation 4e-18), scaled by 2^k with v_ldexp_f64 (underflows to 0 like exp, NaN propagates).
// ~20 instructions against ~35 for the OCML routine; <= 1 ulp on the range the RBF lift uses (x <= ~0).
__device__ __forceinline__ double exp_fast(double x) {
    const double kf = rint(x * 1.44269504088896338700e+00);
    double r = fma(-kf, 6.93147180369123816490e-01, x);      // ln2_hi
    r = fma(-kf, 1.90821492927058770002e-10, r);             // ln2_lo
    double p = fma(r, 1.6059043836821614599e-10, 2.0876756987868098979e-09);   // 1/13!, 1/12!
    p = fma(r, p, 2.5052108385441718775e-08);    // 1/11!
    p = fma(r, p, 2.7557319223985890653e-07);    // 1/10!
    p = fma(r, p, 2.7557319223985892511e-06);    // 1/9!
    p = fma(r, p, 2.4801587301587301566e-05);    // 1/8!
    p = fma(r, p, 1.9841269841269841253e-04);    // 1/7!
    p = fma(r, p, 1.3888888888888889419e-03);    // 1/6!
    p = fma(r, p, 8.3333333333333332177e-03);    // 1/5!
    p = fma(r, p, 4.1666666666666664354e-02);    // 1/4!
    p = fma(r, p, 1.6666666666666665741e-01);    // 1/3!
    p = fma(r, p, 0.5);
    p = fma(r, p, 1.0);
    p = fma(r, p, 1.0);
    double kc = fmin(fmax(kf, -2200.0), 2200.0);             // keep the int conversion in range; ldexp saturates
    return ldexp(p, (int)kc);
}

// rbf value for the centre held by this lane, state row read through wave-uniform (scalar) loads.
// NS > 0: compile-time state dimension (straight-line code, merged scalar loads); NS = 0: runtime n.
// x2 = |x|^2 is the same for every lane; it is computed once per row and shared by the NC centres of a lane.
template <int NS, int NC>
__device__ __forceinline__ void rbf_row(int n, double gamma, const double* __restrict__ xrow, const double (*c)[LIFT_NMAX],
                                        const double* c2, double* out) {
    double x2 = 0.0, dot[NC];
#pragma unroll
    for (int q = 0; q < NC; ++q) dot[q] = 0.0;
    if constexpr (NS > 0) {
        double xr[NS];
#pragma unroll
        for (int j = 0; j < NS; ++j) xr[j] = xrow[j];
#pragma unroll
        for (int j = 0; j < NS; ++j) {
            x2 = fma(xr[j], xr[j], x2);
#pragma unroll
            for (int q = 0; q < NC; ++q) dot[q] = fma(xr[j], c[q][j], dot[q]);
        }
    } else {
#pragma unroll
        for (int j = 0; j < LIFT_NMAX; ++j) {
            if (j < n) {
                const double xj = xrow[j];
                x2 = fma(xj, xj, x2);
#pragma unroll
                for (int q = 0; q < NC; ++q) dot[q] = fma(xj, c[q][j], dot[q]);
            }
        }
    }
#pragma unroll
    for (int q = 0; q < NC; ++q) out[q] = exp_fast(-gamma * ((x2 + c2[q]) - 2.0 * dot[q]));   // Koopman/koopmanEDMDc.py:46-48
}
template <int NS>
__device__ __forceinline__ double rbf_one(int n, double gamma, const double* __restrict__ xrow, const double* c, double c2) {
    double o;
    rbf_row<NS, 1>(n, gamma, xrow, reinterpret_cast<const double (*)[LIFT_NMAX]>(c), &c2, &o);
    return o;
}

}  // namespace brov
