// brov2_ukf.h -- the wave's LDS image and the cross-lane helpers of the unscented Kalman filter kernels: shared by ukf.hip (the
// filter, its tape variant and the backward pass), ukf_feedback.hip (the filter inside the closed loop) and ukf_quat.hip (the filter
// of the quaternion model).  ukf.hip's head comment describes the layout and the synchronisation they serve.
#pragma once
#include "brov2_device.h"
#include "brov2_kernels.h"

namespace brov {

constexpr int UKF_WAVES = 4;            // recordings (waves) per block
constexpr int UKF_LD = 13;              // row stride of the LDS matrices, in doubles
constexpr int UKF_NS = 25;              // sigma points of the 12-state model

struct UkfLds {
    double D[UKF_NS][UKF_LD];           // deviations of the propagated points from point 0 (attitude wrapped)
    double P[12][UKF_LD];               // covariance, both triangles
    double L[12][UKF_LD];               // its lower Cholesky factor
    double x[12], m[12], c0[12], k[12]; // mean, mean deviation, propagated point 0, gain column
};

// the image of the quaternion-model filter (ukf_quat.hip): D, P, L, m and k live in the 12-component error state, the mean and the
// propagated point 0 in the 13-component state; d is the error-state correction that the updates of a row add up
struct UkfQuatLds {
    double D[UKF_NS][UKF_LD];
    double P[12][UKF_LD];
    double L[12][UKF_LD];
    double x[13], c0[13];
    double d[12], m[12], k[12];
};

typedef const UkfRec __attribute__((address_space(4)))* CUK;
__device__ __forceinline__ CUK as_constant_uk(const UkfRec* g) { return (CUK)(unsigned long long)g; }

// LDS written by some lanes of a wave is read by others: order the two
__device__ __forceinline__ void ukf_wave_sync() {
    __builtin_amdgcn_wave_barrier();
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
}
// keeps the image reads of the EM term (ukf_em_term) from mixing with those of the phases around it, which would cost more registers
// than a lane has
__device__ __forceinline__ void ukf_fence() { asm volatile("" ::: "memory"); }
// the value of lane l (a constant) / of the first lane, as a wave-uniform scalar
__device__ __forceinline__ double ukf_lane(double v, int l) {
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), l), __builtin_amdgcn_readlane(__double2loint(v), l));
}
__device__ __forceinline__ double ukf_uniform(double v) {
    return __hiloint2double(__builtin_amdgcn_readfirstlane(__double2hiint(v)), __builtin_amdgcn_readfirstlane(__double2loint(v)));
}
__device__ __forceinline__ double ukf_wrap(double d) {      // the rule of the feedback law (brov2_error.h)
    return fma(-6.28318530717958647692e+00, rint(d * 1.59154943091895335769e-01), d);
}
// entry e of the lower triangle, row by row: e = a (a + 1) / 2 + b, b <= a
__device__ __forceinline__ void ukf_entry(int e, int& a, int& b) {
    a = 0;
    while ((a + 1) * (a + 2) / 2 <= e) ++a;
    b = e - a * (a + 1) / 2;
}

}  // namespace brov
