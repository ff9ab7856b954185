// Deskew: remove the distortion a moving sensor leaves in one sweep.  A point p measured at sweep fraction s
// in the sensor's frame AT THAT TIME becomes D(s_ref)^-1 D(s) p, the same point in the sensor's frame at the reference time,
// with D(s) = (Exp(s w), s t_D) the constant-rate motion between the start and the end of the sweep (sweep_motion.h).
//
// One launch, in place, one lane per row like dpm_points_affine; rows at and past the count are neither read nor written.
// The host derives axis, angle, t_D and D(s_ref)^-1 in float64 and passes them by value; the kernel works in float32:
// Rodrigues' formula with 1 - cos a = 2 sin^2(a / 2), the translation, the reference inverse.  No counterpart in the
// reference (it assumes compensated scans): pinned to this project's float64 restatement (tests/lidar_sweep_restated.py).
#include "dpm_common.h"
#include "sweep_motion.h"

namespace {

constexpr float INV_TWO_PI = 0.15915494309189535f;

struct DeskewArgs {
    float k[3], angle, t[3];   // the motion: unit axis, angle, t_D
    float Ri[9], ti[3];        // D(s_ref)^-1
};

__global__ __launch_bounds__(256) void deskew_kernel(float *__restrict__ xyz, const int32_t *__restrict__ idx,
                                                     const int32_t *__restrict__ count, int cap, int mode,
                                                     const float *__restrict__ times, int n_times, int A, const DeskewArgs m) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= max(0, min(*count, cap))) return;
    float *p = xyz + 3 * (size_t)i;
    const float x = p[0], y = p[1], z = p[2];
    float s;
    if (mode == 0) {          // the column the row's ray belongs to: idx survives sampling and shuffles
        int c = idx[i] % A;
        c = c < 0 ? c + A : c;
        s = (float)c / (float)A;
    } else if (mode == 1) {   // the point's own azimuth: raw frames only
        float u = atan2f(y, x) * INV_TWO_PI;
        u = u < 0.f ? u + 1.f : u;
        if (A > 0) {
            const float c = rintf(u * (float)A);
            s = (c >= (float)A ? 0.f : c) / (float)A;
        } else
            s = u >= 1.f ? 0.f : u;
    } else {                  // explicit fractions by original row; a row whose index lies outside the table stays as it is
        const int j = idx[i];
        if (j < 0 || j >= n_times) return;
        s = times[j];
    }
    const float a = s * m.angle, sn = sinf(a), h = sinf(0.5f * a), v = 2.f * h * h;
    const float cx = m.k[1] * z - m.k[2] * y, cy = m.k[2] * x - m.k[0] * z, cz = m.k[0] * y - m.k[1] * x;     // k x p
    const float ex = m.k[1] * cz - m.k[2] * cy, ey = m.k[2] * cx - m.k[0] * cz, ez = m.k[0] * cy - m.k[1] * cx;   // k x (k x p)
    const float qx = (x + (sn * cx + v * ex)) + s * m.t[0];
    const float qy = (y + (sn * cy + v * ey)) + s * m.t[1];
    const float qz = (z + (sn * cz + v * ez)) + s * m.t[2];
    p[0] = ((m.Ri[0] * qx + m.Ri[1] * qy) + m.Ri[2] * qz) + m.ti[0];
    p[1] = ((m.Ri[3] * qx + m.Ri[4] * qy) + m.Ri[5] * qz) + m.ti[1];
    p[2] = ((m.Ri[6] * qx + m.Ri[7] * qy) + m.Ri[8] * qz) + m.ti[2];
}

}  // namespace

extern "C" int dpm_points_deskew(float *xyz, const int32_t *idx, const int32_t *count, int capacity, int time_mode,
                                 const float *times, int n_times, int azimuth_steps, const double *motion, double s_ref,
                                 dpm_stream_t stream) {
    DPM_CHECK_ARG(xyz && count && motion && capacity >= 1 && time_mode >= 0 && time_mode <= 2);
    DPM_CHECK_ARG(time_mode == 1 || idx != nullptr);
    DPM_CHECK_ARG(time_mode == 0 ? azimuth_steps >= 1 : azimuth_steps >= 0);
    DPM_CHECK_ARG(azimuth_steps <= (1 << 24) && (time_mode != 2 || (times != nullptr && n_times >= 1)));
    DPM_CHECK_ARG(s_ref >= 0.0 && s_ref <= 1.0);   // also refuses NaN
    for (int i = 0; i < 12; ++i) DPM_CHECK_ARG(isfinite(motion[i]));
    // `motion` is HOST memory: D row-major.  D(s) D(s_ref)^-1 of the identity is the identity for every s: nothing to do, and
    // the rows keep their bytes (the arithmetic below would turn a -0 into +0)
    static const double EYE[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    bool identity = true;
    for (int i = 0; i < 12; ++i) identity = identity && motion[i] == EYE[i];
    if (identity) return DPM_OK;
    const SweepMotion mo = sweep_motion(EYE, motion);
    double E[9];
    sweep_exp(mo, s_ref, E);
    DeskewArgs a;
    for (int i = 0; i < 3; ++i) a.k[i] = (float)mo.k[i], a.t[i] = (float)mo.t[i];
    a.angle = (float)mo.angle;
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) a.Ri[3 * i + j] = (float)E[3 * j + i];
        a.ti[i] = (float)(0.0 - s_ref * ((E[i] * mo.t[0] + E[3 + i] * mo.t[1]) + E[6 + i] * mo.t[2]));
    }
    hipLaunchKernelGGL(deskew_kernel, dim3(dpm_cdiv(capacity, 256)), dim3(256), 0, (hipStream_t)stream, xyz, idx, count, capacity,
                       time_mode, times, n_times, azimuth_steps, a);
    return dpm_launch_status();
}
