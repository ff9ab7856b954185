// The motion of a sensor during one sweep, in float64, for the host and the device alike: the simulator's cull
// writes its column table with it (lidar_sim.hip), the deskew entry point derives its kernel arguments with it (deskew.hip).
//
//   D = P0^-1 P1 = (R_D, t_D), w = Log(R_D) = angle * k with |k| = 1 and angle < pi;  D(s) = (Exp(s w), s t_D).
//
// All matrices row-major.  Every operation rounds once (the build has contraction off).
#pragma once
#include <math.h>

struct SweepMotion {
    double k[3];     // unit axis of R_D; (0,0,0) when R_D has no antisymmetric part (the identity)
    double angle;    // in [0, pi)
    double t[3];     // t_D
};

// D = P0^-1 P1 of two 4x4 sensor-to-world poses, as rotation (9) and translation (3).  R_D[i][j] = sum_k R0[k][i] R1[k][j]
// in this order: with P1 == P0 the sum for [i][j] and for [j][i] are the same products in the same order, so R_D is EXACTLY
// symmetric, sweep_log gives angle 0 and every D(s) is exactly the identity.
__host__ __device__ inline void sweep_delta(const double *P0, const double *P1, double *R, double *t) {
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) R[3 * i + j] = (P0[i] * P1[j] + P0[4 + i] * P1[4 + j]) + P0[8 + i] * P1[8 + j];
    const double dx = P1[3] - P0[3], dy = P1[7] - P0[7], dz = P1[11] - P0[11];
    for (int i = 0; i < 3; ++i) t[i] = (P0[i] * dx + P0[4 + i] * dy) + P0[8 + i] * dz;
}

// Log of a rotation from its antisymmetric part v = sin(angle) k and its trace: atan2 keeps a tiny angle (|v| ~ 1e-9) as
// exact as |v| itself, and v == 0 is answered without a division.  A half turn (v == 0, trace -1) has no unique axis and
// lies outside the model; it reads as the identity.
__host__ __device__ inline void sweep_log(const double *R, double *k, double *angle) {
    const double vx = 0.5 * (R[7] - R[5]), vy = 0.5 * (R[2] - R[6]), vz = 0.5 * (R[3] - R[1]);
    const double n = sqrt((vx * vx + vy * vy) + vz * vz);
    if (n == 0.0) {
        k[0] = k[1] = k[2] = 0.0, *angle = 0.0;
        return;
    }
    k[0] = vx / n, k[1] = vy / n, k[2] = vz / n;
    *angle = atan2(n, 0.5 * (((R[0] + R[4]) + R[8]) - 1.0));
}

__host__ __device__ inline SweepMotion sweep_motion(const double *P0, const double *P1) {
    SweepMotion m;
    double R[9];
    sweep_delta(P0, P1, R, m.t);
    sweep_log(R, m.k, &m.angle);
    return m;
}

// Exp(s w) by Rodrigues' formula, 1 - cos a written as 2 sin^2(a / 2): I + sin a K + (1 - cos a) (k k^T - |k|^2 I)
__host__ __device__ inline void sweep_exp(const SweepMotion &m, double s, double *R) {
    const double a = s * m.angle, sn = sin(a), h = sin(0.5 * a), v = 2.0 * h * h;
    const double x = m.k[0], y = m.k[1], z = m.k[2], kk = (x * x + y * y) + z * z;
    R[0] = 1.0 + v * (x * x - kk), R[1] = v * (x * y) - sn * z, R[2] = v * (x * z) + sn * y;
    R[3] = v * (x * y) + sn * z, R[4] = 1.0 + v * (y * y - kk), R[5] = v * (y * z) - sn * x;
    R[6] = v * (x * z) - sn * y, R[7] = v * (y * z) + sn * x, R[8] = 1.0 + v * (z * z - kk);
}
