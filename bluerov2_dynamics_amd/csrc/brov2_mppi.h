// brov2_mppi.h -- what the cost kernels of the model-predictive update share (mppi.hip: the Fossen models, koopman_mppi.hip: an EDMDc
// model): the record and arrays behind the constant address space, and the command of a sample (include/brov2.h: brov_mppi_step)
#pragma once
#include "brov2_kernels.h"
#include "brov2_stream.h"

namespace brov {

typedef const MppiRec __attribute__((address_space(4)))* CMR;
typedef const double __attribute__((address_space(4)))* CDP;
__device__ __forceinline__ CMR as_constant_mr(const MppiRec* g) { return (CMR)(unsigned long long)g; }
__device__ __forceinline__ CDP as_constant_d(const double* g) { return (CDP)(unsigned long long)g; }
// make the compiler re-issue the scalar loads behind the pointer here (relaunder in brov2_fast.h)
__device__ __forceinline__ CMR relaunder_mr(CMR f) {
    asm volatile("" : "+s"(f));
    return f;
}
__device__ __forceinline__ CDP relaunder_d(CDP f) {
    asm volatile("" : "+s"(f));
    return f;
}

// a clamp that lets a NaN through (fmin / fmax would return the limit): a NaN perturbation must reach the cost
__device__ __forceinline__ double clip_keep_nan(double v, double lo, double hi) {
    v = v < lo ? lo : v;
    return v > hi ? hi : v;
}

// The command of sample k at one (knot, channel): clip(U + sigma xi, lo, hi) with xi = 0 for the nominal sample (k = 0) and for an
// unperturbed channel (sigma = 0; neither eps nor the stream is touched), else eps[c] or the normal number c of the second stream.
// c = ((b K + k) M + m) nu + j is both the index into eps and the counter.  Both kernels call this: the same bits in both.
__device__ __forceinline__ double mppi_command(double U, double sg, double lo, double hi, const double* __restrict__ eps, uint64_t s2,
                                               uint64_t c, bool nominal) {
    double xi = 0.0;
    if (sg > 0.0) {                     // wave-uniform
        const double n = eps ? eps[c] : box_muller(uniform01_at(s2, 2ull * c), uniform01_at(s2, 2ull * c + 1ull));
        xi = nominal ? 0.0 : n;
    }
    return clip_keep_nan(fma(sg, xi, U), lo, hi);
}

}  // namespace brov
