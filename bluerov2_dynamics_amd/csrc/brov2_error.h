// brov2_error.h -- the tracking error e[12] of the closed-loop laws (include/brov2.h: brov_rollout_feedback), shared by
// feedback.hip and mppi.hip
#pragma once
#include "brov2_device.h"
#include "brov2_fast.h"

namespace brov {

// e[12] of the law: body-frame position error R^T (p_ref - p) with the model's R, attitude error (Euler angles: the difference
// wrapped by arithmetic; quaternion: twice the vector part of conj(q) q_ref, signed to the short way round), velocity error.
template <int MODEL>
__device__ __forceinline__ void tracking_error(const double* x, const double* r, const double2* qt, double e[12]) {
    constexpr int NV = Dims<MODEL>::NV;
    double R[9];
    if constexpr (model_is_quat(MODEL)) {
        double q[4] = {x[3], x[4], x[5], x[6]};
        quat_normalize(q);                                    // R as rhs_fast_quat forms it
        const double qw = q[0], qx = q[1], qy = q[2], qz = q[3];
        R[0] = 1.0 - 2.0 * fma(qy, qy, qz * qz); R[1] = 2.0 * fma(qx, qy, -(qz * qw));    R[2] = 2.0 * fma(qx, qz, qy * qw);
        R[3] = 2.0 * fma(qx, qy, qz * qw);       R[4] = 1.0 - 2.0 * fma(qx, qx, qz * qz); R[5] = 2.0 * fma(qy, qz, -(qx * qw));
        R[6] = 2.0 * fma(qx, qz, -(qy * qw));    R[7] = 2.0 * fma(qy, qz, qx * qw);       R[8] = 1.0 - 2.0 * fma(qx, qx, qy * qy);
        // q_e = conj(q) (x) q_ref on the quaternions as stored
        const double sw = x[3], sx = x[4], sy = x[5], sz = x[6], rw = r[3], rx = r[4], ry = r[5], rz = r[6];
        const double we = fma(sz, rz, fma(sy, ry, fma(sx, rx, sw * rw)));
        const double vx = fma(sw, rx, -(rw * sx)) - fma(sy, rz, -(sz * ry));
        const double vy = fma(sw, ry, -(rw * sy)) - fma(sz, rx, -(sx * rz));
        const double vz = fma(sw, rz, -(rw * sz)) - fma(sx, ry, -(sy * rx));
        const double s = we >= 0.0 ? 2.0 : -2.0;
        e[3] = s * vx; e[4] = s * vy; e[5] = s * vz;
    } else {
        Trig t;
        trig_full(x + 3, t, qt);                              // R as rhs_fast_euler<GENERIC> forms it
        const double ss = t.sth * t.sphi, sc = t.sth * t.cphi;
        R[0] = t.cpsi * t.cth; R[1] = fma(t.cpsi, ss, -(t.spsi * t.cphi)); R[2] = fma(t.cpsi, sc, t.spsi * t.sphi);
        R[3] = t.spsi * t.cth; R[4] = fma(t.spsi, ss, t.cpsi * t.cphi);    R[5] = fma(t.spsi, sc, -(t.cpsi * t.sphi));
        R[6] = -t.sth;         R[7] = t.cth * t.sphi;                      R[8] = t.cth * t.cphi;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const double d = r[3 + i] - x[3 + i];
            e[3 + i] = fma(-6.28318530717958647692e+00, rint(d * 1.59154943091895335769e-01), d);
        }
    }
    const double d0 = r[0] - x[0], d1 = r[1] - x[1], d2 = r[2] - x[2];
#pragma unroll
    for (int i = 0; i < 3; ++i) e[i] = fma(R[6 + i], d2, fma(R[3 + i], d1, R[i] * d0));
#pragma unroll
    for (int i = 0; i < 6; ++i) e[6 + i] = r[NV + i] - x[NV + i];
}

}  // namespace brov
