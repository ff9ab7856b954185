// A spinning-LiDAR simulator: a procedural scene (ground plane, oriented boxes, capped vertical cylinders) ray-cast from F
// sensor poses.  No counterpart in the reference: pinned to this project's own restatement (tests/lidar_sim_restated.py).
// THREE launches for a batch of F frames, whatever F is, no host synchronisation, nothing but stream-ordered kernels:
//
//   dpm_lidar_cull  one block per frame.  Every primitive is moved into the frame of the sensor in FLOAT64 and rounded to
//                   float32 once: a record holds the sensor's origin in the primitive's own coordinates, the three rows that
//                   turn a sensor-frame direction into those coordinates, and the extents.  So the cast works with numbers
//                   no larger than max_range + the primitive's size, however far from the world's origin the scene lies.
//                   Primitives whose bounding sphere reaches the max_range ball are kept, in ascending index (a block scan).
//   dpm_lidar_cast  one lane per ray; the frame's kept records pass through LDS in tiles of TILE, every lane reads the same
//                   record (an LDS broadcast).  Slab test for the box; for the cylinder the side interval from the
//                   perpendicular distance of the axis to the ray (no b^2 - a c) cut with the slab of the two caps.
//   dpm_lidar_emit  range noise, drop, xyz = t * dir, intensity / label, and the ordered compaction into the frame layout of
//                   augment.hip in ONE launch: every block counts the keep flags of the whole frame (the part before its
//                   chunk is its offset, the total is the count), then writes its chunk like ingest.hip does.
//
// Sweep motion, still three launches: dpm_lidar_cull_sweep takes a start and an end pose per frame, keeps what
// the max_range ball enlarged by the sensor's travel reaches, and writes the frame's column table (Exp(s_c w) and s_c t_D per
// azimuth column, float64 rounded once); dpm_lidar_cast_sweep turns every ray by its column's entry and moves its origin.
// Both are the MOVING instantiation of the kernels below; the static one compiles to the code it was before the template.
//
// Arithmetic: + - * / sqrt, each rounded once (the build has contraction off; there is no fmaf here), so a float32 numpy
// restatement that follows the order of operations gives the same bits.  No atomics.
#include <math.h>

#include "block_scan.h"
#include "sweep_motion.h"

namespace {

constexpr int REC = 16;     // floats per kept record: o(3) u(3) v(3) w(3) h(3) id
constexpr int PRM = 10;     // doubles per scene primitive: c(3) h(3) cos sin sphere_dz sphere_radius
constexpr int TILE = 64;    // records per LDS tile of the cast
constexpr int CH = 4096;    // rays per compaction block of the emit
constexpr int KIND_SHIFT = 30;
constexpr int COL = 12;     // floats per column of a sweep table: Exp(s_c w) row-major (9), s_c t_D (3)

// ---- cull: grid (F), 256 threads.  MOVING: poses = the start poses, poses1 = the end poses, A columns, table (F,A,COL)
template <bool MOVING>
__global__ __launch_bounds__(256) void lidar_cull_kernel(const double *__restrict__ prims, const int32_t *__restrict__ kind, int P,
                                                         const double *__restrict__ ground, const double *__restrict__ poses,
                                                         double max_range, int max_kept, float *__restrict__ kept,
                                                         float *__restrict__ plane, int32_t *__restrict__ status,
                                                         const double *__restrict__ poses1, int A, float *__restrict__ table) {
    __shared__ int s_w[4];
    const int f = blockIdx.x, t = threadIdx.x;
    const double *M = poses + 16 * (size_t)f;
    if constexpr (MOVING) {
        // every thread derives the frame's motion itself (a few dozen float64 operations); the reach grows by the travel
        const SweepMotion mo = sweep_motion(M, poses1 + 16 * (size_t)f);
        max_range += sqrt((mo.t[0] * mo.t[0] + mo.t[1] * mo.t[1]) + mo.t[2] * mo.t[2]);
        float *col = table + (size_t)f * A * COL;
        for (int c = t; c < A; c += 256) {
            const double sc = (double)c / (double)A;
            double E[9];
            sweep_exp(mo, sc, E);
#pragma unroll
            for (int i = 0; i < 9; ++i) col[(size_t)c * COL + i] = (float)E[i];
#pragma unroll
            for (int i = 0; i < 3; ++i) col[(size_t)c * COL + 9 + i] = (float)(sc * mo.t[i]);
        }
    }
    const double R00 = M[0], R01 = M[1], R02 = M[2], tx = M[3];
    const double R10 = M[4], R11 = M[5], R12 = M[6], ty = M[7];
    const double R20 = M[8], R21 = M[9], R22 = M[10], tz = M[11];
    float *out = kept + (size_t)f * max_kept * REC;
    int base = 0;
    for (int p0 = 0; p0 < P; p0 += 256) {
        const int p = p0 + t;
        bool keep = false;
        double ex = 0, ey = 0, ez = 0, c = 1, s = 0, ha = 0, hb = 0, hc = 0;
        if (p < P) {
            const double *q = prims + (size_t)PRM * p;
            ex = tx - q[0], ey = ty - q[1], ez = tz - q[2];
            ha = q[3], hb = q[4], hc = q[5], c = q[6], s = q[7];
            const double sz = ez - q[8], reach = max_range + q[9];
            keep = (ex * ex + ey * ey) + sz * sz <= reach * reach;
        }
        const int pos = block_scan_exclusive((int)keep, s_w, base);
        base += s_w[0] + s_w[1] + s_w[2] + s_w[3];
        __syncthreads();
        if (keep && pos < max_kept) {
            float *r = out + (size_t)pos * REC;
            // the sensor's origin in the primitive's coordinates (a turn by -yaw about z)
            r[0] = (float)(c * ex + s * ey);
            r[1] = (float)(c * ey - s * ex);
            r[2] = (float)ez;
            // rows that take a sensor-frame direction d to the primitive's coordinates: Rz(-yaw) R
            r[3] = (float)(c * R00 + s * R10), r[4] = (float)(c * R01 + s * R11), r[5] = (float)(c * R02 + s * R12);
            r[6] = (float)(c * R10 - s * R00), r[7] = (float)(c * R11 - s * R01), r[8] = (float)(c * R12 - s * R02);
            r[9] = (float)R20, r[10] = (float)R21, r[11] = (float)R22;
            r[12] = (float)ha, r[13] = (float)hb, r[14] = (float)hc;
            r[15] = __int_as_float(p | (kind[p] << KIND_SHIFT));
        }
    }
    if (t == 0) {
        status[2 * f] = base;
        status[2 * f + 1] = base > max_kept;
        const bool has = ground[1] != 0.0;
        float *g = plane + 4 * (size_t)f;
        g[0] = has ? (float)R20 : 0.f, g[1] = has ? (float)R21 : 0.f, g[2] = has ? (float)R22 : 0.f;
        g[3] = has ? (float)(ground[0] - tz) : 0.f;
    }
}

// one axis of a slab [lo, hi] seen from o along dd: the parameter interval [tn, tf]; false = the ray misses the slab
__device__ __forceinline__ bool slab(float o, float dd, float lo, float hi, float &tn, float &tf) {
    if (dd == 0.f) {
        tn = -INFINITY, tf = INFINITY;
        return !(o < lo || o > hi);
    }
    const float t1 = (lo - o) / dd, t2 = (hi - o) / dd;
    tn = t1 < t2 ? t1 : t2;
    tf = t1 < t2 ? t2 : t1;
    return true;
}

// ---- cast: grid (ceil(rays / 256), F), 256 threads, one lane per ray.  MOVING: ray r belongs to column r % A of the table
template <bool MOVING>
__global__ __launch_bounds__(256) void lidar_cast_kernel(const float *__restrict__ kept, const float *__restrict__ plane,
                                                         const int32_t *__restrict__ status, int max_kept, int P,
                                                         const float *__restrict__ dirs, int rays, float min_range,
                                                         float max_range, float *__restrict__ range, int32_t *__restrict__ prim,
                                                         float *__restrict__ cos_inc, const float *__restrict__ table, int A) {
    __shared__ float s_rec[TILE * REC];
    const int f = blockIdx.y;
    const int r = blockIdx.x * 256 + threadIdx.x;
    const bool live = r < rays;
    float d0 = live ? dirs[3 * (size_t)r] : 1.f, d1 = live ? dirs[3 * (size_t)r + 1] : 0.f,
          d2 = live ? dirs[3 * (size_t)r + 2] : 0.f;
    float o0 = 0.f, o1 = 0.f, o2 = 0.f;   // MOVING: the sensor's origin at the ray's time, in the frame of the start pose
    if constexpr (MOVING) {
        if (live) {   // the ray's direction in the frame of the start pose: d' = R_c d
            const float *e = table + ((size_t)f * A + r % A) * COL;
            const float x = d0, y = d1, z = d2;
            d0 = (e[0] * x + e[1] * y) + e[2] * z;
            d1 = (e[3] * x + e[4] * y) + e[5] * z;
            d2 = (e[6] * x + e[7] * y) + e[8] * z;
            o0 = e[9], o1 = e[10], o2 = e[11];
        }
    }
    const int n = max(0, min(status[2 * f], max_kept));
    const float *rec = kept + (size_t)f * max_kept * REC;
    float best = INFINITY, bcos = 0.f;
    int bid = -1;
    for (int k0 = 0; k0 < n; k0 += TILE) {
        const int m = min(TILE, n - k0);
        __syncthreads();
        for (int i = threadIdx.x; i < m * REC; i += 256) s_rec[i] = rec[(size_t)k0 * REC + i];
        __syncthreads();
        for (int k = 0; k < m; ++k) {
            const float *q = s_rec + k * REC;
            // MOVING: the moved origin in the primitive's coordinates, q.o + U o_c
            const float ox = MOVING ? q[0] + ((q[3] * o0 + q[4] * o1) + q[5] * o2) : q[0];
            const float oy = MOVING ? q[1] + ((q[6] * o0 + q[7] * o1) + q[8] * o2) : q[1];
            const float oz = MOVING ? q[2] + ((q[9] * o0 + q[10] * o1) + q[11] * o2) : q[2];
            const float dx = (q[3] * d0 + q[4] * d1) + q[5] * d2;
            const float dy = (q[6] * d0 + q[7] * d1) + q[8] * d2;
            const float dz = (q[9] * d0 + q[10] * d1) + q[11] * d2;
            const int id = __float_as_int(q[15]);
            float enter, exit_, cen, cex;
            bool hit;
            if ((id >> KIND_SHIFT) == 0) {   // box, half extents q[12..14]
                float nx, fx, ny, fy, nz, fz;
                hit = slab(ox, dx, -q[12], q[12], nx, fx);
                hit = slab(oy, dy, -q[13], q[13], ny, fy) && hit;
                hit = slab(oz, dz, -q[14], q[14], nz, fz) && hit;
                enter = nx, cen = fabsf(dx);
                if (ny > enter) enter = ny, cen = fabsf(dy);
                if (nz > enter) enter = nz, cen = fabsf(dz);
                exit_ = fx, cex = fabsf(dx);
                if (fy < exit_) exit_ = fy, cex = fabsf(dy);
                if (fz < exit_) exit_ = fz, cex = fabsf(dz);
            } else {                         // cylinder, radius q[12], height q[13], base at the origin
                const float rad = q[12];
                const float a = dx * dx + dy * dy;
                float ns, fs, cs, nz, fz;
                if (a == 0.f) {
                    hit = ox * ox + oy * oy <= rad * rad;
                    ns = -INFINITY, fs = INFINITY, cs = 0.f;
                } else {
                    const float cr = fabsf(ox * dy - oy * dx);   // distance of the axis to the ray, times sqrt(a)
                    const float qa = rad * sqrtf(a);
                    const float disc = (qa - cr) * (qa + cr);
                    hit = disc >= 0.f;
                    const float sd = sqrtf(hit ? disc : 0.f);
                    const float half = sd / a;
                    const float tm = (0.f - (ox * dx + oy * dy)) / a;
                    ns = tm - half, fs = tm + half, cs = sd / rad;
                }
                hit = slab(oz, dz, 0.f, q[13], nz, fz) && hit;
                enter = ns, cen = cs;
                if (nz > enter) enter = nz, cen = fabsf(dz);
                exit_ = fs, cex = cs;
                if (fz < exit_) exit_ = fz, cex = fabsf(dz);
            }
            hit = hit && enter <= exit_ && exit_ > 0.f;
            const float t = enter > 0.f ? enter : exit_;
            const float c = enter > 0.f ? cen : cex;
            if (hit && t < best) best = t, bcos = c, bid = id & ((1 << KIND_SHIFT) - 1);
        }
    }
    {   // the ground last: it takes a tie from nobody
        const float *g = plane + 4 * (size_t)f;
        const float den = (g[0] * d0 + g[1] * d1) + g[2] * d2;
        if (den != 0.f) {
            const float t = (MOVING ? g[3] - ((g[0] * o0 + g[1] * o1) + g[2] * o2) : g[3]) / den;
            if (t > 0.f && t < best) best = t, bcos = fabsf(den), bid = P;
        }
    }
    if (!live) return;
    const bool ret = bid >= 0 && !(best < min_range) && !(best > max_range);
    const size_t o = (size_t)f * rays + r;
    range[o] = ret ? best : 0.f;
    prim[o] = ret ? bid : -1;
    cos_inc[o] = ret ? bcos : 0.f;
}

// ---- emit: grid (ceil(rays / CH), F), 256 threads
__device__ __forceinline__ bool returns(const int32_t *__restrict__ prim, const float *__restrict__ u, float drop, size_t o) {
    return prim[o] >= 0 && (u == nullptr || u[o] >= drop);
}

__global__ __launch_bounds__(256) void lidar_emit_kernel(const float *__restrict__ range, const int32_t *__restrict__ prim,
                                                         const float *__restrict__ cos_inc, const float *__restrict__ dirs,
                                                         int rays, const float *__restrict__ noise, const float *__restrict__ u,
                                                         float drop, const float *__restrict__ albedo,
                                                         const int32_t *__restrict__ class_id, int P, float *__restrict__ xyz,
                                                         int32_t *__restrict__ idx, int32_t *__restrict__ count,
                                                         float *__restrict__ intensity, int32_t *__restrict__ label) {
    __shared__ int s_a[4], s_b[4], s_w[4];
    const int f = blockIdx.y, t = threadIdx.x, lane = t & 63, w = t >> 6;
    const size_t fo = (size_t)f * rays;
    const int c0 = blockIdx.x * CH;
    // the keep flags of the whole frame: those before this chunk are its offset, all of them the frame's count
    int before = 0, total = 0;
    for (int r = t; r < rays; r += 256) {
        const int k = returns(prim, u, drop, fo + r);
        total += k;
        before += r < c0 ? k : 0;
    }
    before = wave_sum(before), total = wave_sum(total);
    if (lane == 0) s_a[w] = before, s_b[w] = total;
    // thread t owns CH / 256 CONSECUTIVE rays so that the block-level order is the ray order
    bool keep[CH / 256];
    int cnt = 0;
#pragma unroll
    for (int k = 0; k < CH / 256; ++k) {
        const int r = c0 + t * (CH / 256) + k;
        keep[k] = r < rays && returns(prim, u, drop, fo + r);
        cnt += keep[k];
    }
    int pos = block_scan_exclusive(cnt, s_w);   // its barrier also publishes s_a / s_b
    const int n = s_b[0] + s_b[1] + s_b[2] + s_b[3];
    pos += s_a[0] + s_a[1] + s_a[2] + s_a[3];
    float *ox = xyz + 3 * fo;
    int32_t *oi = idx + fo;
#pragma unroll
    for (int k = 0; k < CH / 256; ++k) {
        const int r = c0 + t * (CH / 256) + k;
        if (r >= rays) break;
        const int id = prim[fo + r];
        const bool hit = id >= 0 && id <= P;
        intensity[fo + r] = hit ? albedo[id] * cos_inc[fo + r] : 0.f;
        label[fo + r] = hit ? class_id[id] : -1;
        if (!keep[k]) continue;
        const float tt = noise != nullptr ? range[fo + r] + noise[fo + r] : range[fo + r];
        if (pos < rays) {
            ox[3 * (size_t)pos] = tt * dirs[3 * (size_t)r];
            ox[3 * (size_t)pos + 1] = tt * dirs[3 * (size_t)r + 1];
            ox[3 * (size_t)pos + 2] = tt * dirs[3 * (size_t)r + 2];
            oi[pos] = r;
        }
        ++pos;
    }
    // rows at and past the count of this block's OUTPUT range: zero (survivors land below the count, never here)
    for (int k = t; k < CH; k += 256) {
        const int j = c0 + k;
        if (j >= rays) break;
        if (j >= n) ox[3 * (size_t)j] = 0.f, ox[3 * (size_t)j + 1] = 0.f, ox[3 * (size_t)j + 2] = 0.f, oi[j] = 0;
    }
    if (blockIdx.x == 0 && t == 0) count[f] = n;
}

}  // namespace

extern "C" int dpm_lidar_cull(const double *prims, const int32_t *kind, int P, const double *ground, const double *poses, int F,
                              double max_range, int max_kept, float *kept, float *plane, int32_t *status, dpm_stream_t stream) {
    DPM_CHECK_ARG(P >= 0 && P < (1 << KIND_SHIFT) && (P == 0 || (prims && kind)));
    DPM_CHECK_ARG(ground && poses && kept && plane && status);
    DPM_CHECK_ARG(F >= 1 && F <= 65535 && max_kept >= 1 && max_range > 0.0);
    hipLaunchKernelGGL(lidar_cull_kernel<false>, dim3(F), dim3(256), 0, (hipStream_t)stream, prims, kind, P, ground, poses,
                       max_range, max_kept, kept, plane, status, (const double *)nullptr, 0, (float *)nullptr);
    return dpm_launch_status();
}

extern "C" int dpm_lidar_cull_sweep(const double *prims, const int32_t *kind, int P, const double *ground, const double *poses0,
                                    const double *poses1, int F, int azimuth_steps, double max_range, int max_kept, float *kept,
                                    float *plane, int32_t *status, float *table, dpm_stream_t stream) {
    DPM_CHECK_ARG(P >= 0 && P < (1 << KIND_SHIFT) && (P == 0 || (prims && kind)));
    DPM_CHECK_ARG(ground && poses0 && poses1 && kept && plane && status && table);
    DPM_CHECK_ARG(F >= 1 && F <= 65535 && max_kept >= 1 && max_range > 0.0 && azimuth_steps >= 1 && azimuth_steps <= (1 << 24));
    hipLaunchKernelGGL(lidar_cull_kernel<true>, dim3(F), dim3(256), 0, (hipStream_t)stream, prims, kind, P, ground, poses0,
                       max_range, max_kept, kept, plane, status, poses1, azimuth_steps, table);
    return dpm_launch_status();
}

extern "C" int dpm_lidar_cast(const float *kept, const float *plane, const int32_t *status, int max_kept, int P,
                              const float *dirs, int rays, int F, double min_range, double max_range, float *range,
                              int32_t *prim, float *cos_inc, dpm_stream_t stream) {
    DPM_CHECK_ARG(kept && plane && status && dirs && range && prim && cos_inc);
    DPM_CHECK_ARG(P >= 0 && P < (1 << KIND_SHIFT) && max_kept >= 1 && rays >= 1 && rays <= (1 << 24) && F >= 1 && F <= 65535);
    DPM_CHECK_ARG(min_range >= 0.0 && max_range > min_range);
    hipLaunchKernelGGL(lidar_cast_kernel<false>, dim3(dpm_cdiv(rays, 256), F), dim3(256), 0, (hipStream_t)stream, kept, plane,
                       status, max_kept, P, dirs, rays, (float)min_range, (float)max_range, range, prim, cos_inc,
                       (const float *)nullptr, 0);
    return dpm_launch_status();
}

extern "C" int dpm_lidar_cast_sweep(const float *kept, const float *plane, const int32_t *status, int max_kept, int P,
                                    const float *dirs, int rays, int F, const float *table, int azimuth_steps, double min_range,
                                    double max_range, float *range, int32_t *prim, float *cos_inc, dpm_stream_t stream) {
    DPM_CHECK_ARG(kept && plane && status && dirs && table && range && prim && cos_inc);
    DPM_CHECK_ARG(P >= 0 && P < (1 << KIND_SHIFT) && max_kept >= 1 && rays >= 1 && rays <= (1 << 24) && F >= 1 && F <= 65535);
    DPM_CHECK_ARG(azimuth_steps >= 1 && rays % azimuth_steps == 0 && min_range >= 0.0 && max_range > min_range);
    hipLaunchKernelGGL(lidar_cast_kernel<true>, dim3(dpm_cdiv(rays, 256), F), dim3(256), 0, (hipStream_t)stream, kept, plane,
                       status, max_kept, P, dirs, rays, (float)min_range, (float)max_range, range, prim, cos_inc, table,
                       azimuth_steps);
    return dpm_launch_status();
}

extern "C" int dpm_lidar_emit(const float *range, const int32_t *prim, const float *cos_inc, const float *dirs, int rays, int F,
                              const float *noise, const float *u, double drop_prob, const float *albedo,
                              const int32_t *class_id, int P, float *xyz, int32_t *idx, int32_t *count, float *intensity,
                              int32_t *label, dpm_stream_t stream) {
    DPM_CHECK_ARG(range && prim && cos_inc && dirs && albedo && class_id && xyz && idx && count && intensity && label);
    DPM_CHECK_ARG(P >= 0 && P < (1 << KIND_SHIFT) && rays >= 1 && rays <= (1 << 24) && F >= 1 && F <= 65535);
    DPM_CHECK_ARG(drop_prob >= 0.0 && drop_prob <= 1.0);
    hipLaunchKernelGGL(lidar_emit_kernel, dim3(dpm_cdiv(rays, CH), F), dim3(256), 0, (hipStream_t)stream, range, prim, cos_inc,
                       dirs, rays, noise, u, (float)drop_prob, albedo, class_id, P, xyz, idx, count, intensity, label);
    return dpm_launch_status();
}
