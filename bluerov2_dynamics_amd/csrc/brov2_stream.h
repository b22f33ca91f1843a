// brov2_stream.h -- the counter-based splitmix64 stream and the Box-Muller normal of dist B (controls.hip holds the layout of the
// counters of the control fills, mppi.hip that of its perturbations)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace brov {

__device__ __forceinline__ uint64_t splitmix64_at(uint64_t seed, uint64_t counter) {
    uint64_t z = seed + (counter + 1ull) * 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
__device__ __forceinline__ double uniform01_at(uint64_t seed, uint64_t counter) {
    return (double)(splitmix64_at(seed, counter) >> 11) * 0x1.0p-53;
}

// Box-Muller normal of dist B from two uniforms of the counter stream: sqrt(-2 ln(1 - u1)) cos(2 pi u2) (oracle/controls.py).  1 - u1 is exact
// (u1 is a multiple of 2^-53 below 1), so log(1 - u1) is the oracle's log1p(-u1) to an ulp, and cospi(2 u2) is cos(2 pi u2) without the
// rounding of the product 2 pi u2 and without the large-argument branch of cos: the values agree with the NumPy oracle to ~6e-15 absolute
// (tested at 1e-12) for 0.7 of the instructions (round 6: the fill kernels are bound by fp64 VALU issue, profiles/r06_cfg4_pmc_summary.json).
__device__ __forceinline__ double box_muller(double u1, double u2) {
    return sqrt(-2.0 * log(1.0 - u1)) * cospi(2.0 * u2);
}

}  // namespace brov
