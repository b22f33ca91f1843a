// brov2_rows.h -- global <-> register movement for one row of NX/NU doubles (shared by rollout.hip and feedback.hip)
#pragma once
#include <hip/hip_runtime.h>

namespace brov {

template <int N>
__device__ __forceinline__ void load_row(const double* __restrict__ src, double* r) {
    if constexpr (N % 2 == 0) {
        const double2* s2 = reinterpret_cast<const double2*>(src);
#pragma unroll
        for (int i = 0; i < N / 2; ++i) { double2 v = s2[i]; r[2 * i] = v.x; r[2 * i + 1] = v.y; }
    } else {
#pragma unroll
        for (int i = 0; i < N; ++i) r[i] = src[i];
    }
}
template <int N>
__device__ __forceinline__ void store_row(double* __restrict__ dst, const double* r) {
    if constexpr (N % 2 == 0) {
        double2* d2 = reinterpret_cast<double2*>(dst);
#pragma unroll
        for (int i = 0; i < N / 2; ++i) d2[i] = make_double2(r[2 * i], r[2 * i + 1]);
    } else {
#pragma unroll
        for (int i = 0; i < N; ++i) dst[i] = r[i];
    }
}

}  // namespace brov
