// The map assembly of the registration training step (reference pipeline/modules/model_pipeline.py:62-104 with
// _get_accurate_RT, :199-272): B x S encoded frames become a source map of S1 frames and a target map of S - S1 frames, every
// frame's key points moved into its map's first frame, (B,S,C,N) interleaved into (B,C,S*N).  The reference walks the frames in
// Python (per frame one upload, one 4x4 inverse, a handful of 3x3 products); here it is three launches without a host round
// trip: the poses (one thread per frame), the assembly, and the assembly's backward.
//
// Rounding order (the build has -ffp-contract=off, every fusion below is written out):
//   scaled point       p = coor * (float)coor_scale                                   one rounding, as `coor * scale` in torch
//   moved point        q_i = fmaf(r_i2, p_z, fmaf(r_i1, p_y, r_i0 * p_x)) + t_i       the product first, then `+ T` as its own
//                      rounding: the reference's `R @ coor + T` is a matmul whose result is stored and an addition
//   4x4 / 3x3 products c_ij = fmaf(a_i3, b_3j, ... fmaf(a_i1, b_1j, a_i0 * b_0j))     k ascending
//   4x4 inverse        Gauss-Jordan on [A | I], partial pivoting, IEEE division; a singular calib gives Inf / NaN
// The first frame of a map is not multiplied by an identity: it is `p` and nothing else.  Feature rows and masks are copies.
// The backward is a gather (one reader per output element): exact, and the same bytes on every run.
#include <algorithm>

#include "dpm_common.h"

namespace {

constexpr int MAX_FRAMES = 65535;   // frames ride in gridDim.y

// c = a b, 4x4 row-major
__device__ void mul4(const float *a, const float *b, float *c) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float acc = a[4 * i] * b[j];
#pragma unroll
            for (int k = 1; k < 4; ++k) acc = fmaf(a[4 * i + k], b[4 * k + j], acc);
            c[4 * i + j] = acc;
        }
}

// inv = a^-1 (4x4 row-major): Gauss-Jordan with partial pivoting.  Every index is a compile-time constant after unrolling
// (the pivot row is brought up by conditional swaps), so both matrices stay in registers.
__device__ void invert4(const float *a_in, float *inv) {
    float a[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) a[i] = a_in[i], inv[i] = (i % 5 == 0) ? 1.f : 0.f;
#pragma unroll
    for (int col = 0; col < 4; ++col) {
        int p = col;
        float best = fabsf(a[4 * col + col]);
#pragma unroll
        for (int r = col + 1; r < 4; ++r) {
            const float v = fabsf(a[4 * r + col]);
            if (v > best) best = v, p = r;
        }
#pragma unroll
        for (int r = col + 1; r < 4; ++r)
            if (r == p) {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    float t = a[4 * col + j];
                    a[4 * col + j] = a[4 * r + j], a[4 * r + j] = t;
                    t = inv[4 * col + j];
                    inv[4 * col + j] = inv[4 * r + j], inv[4 * r + j] = t;
                }
            }
        const float d = a[4 * col + col];
#pragma unroll
        for (int j = 0; j < 4; ++j) a[4 * col + j] = a[4 * col + j] / d, inv[4 * col + j] = inv[4 * col + j] / d;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            if (r == col) continue;
            const float m = a[4 * r + col];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                a[4 * r + j] = fmaf(-m, a[4 * col + j], a[4 * r + j]);
                inv[4 * r + j] = fmaf(-m, inv[4 * col + j], inv[4 * r + j]);
            }
        }
    }
}

// entry e < F: frame (b, s) into its map's first frame; entry F + b: source-first into target-first.  out = [R | T], 3x4.
__global__ __launch_bounds__(64) void map_poses_kernel(const float *__restrict__ R, const float *__restrict__ T,
                                                        const float *__restrict__ calib, const float *__restrict__ icp,
                                                        const uint8_t *__restrict__ has_icp, int B, int S, int S1,
                                                        float *__restrict__ rel, float *__restrict__ gt) {
    const int F = B * S, e = blockIdx.x * 64 + threadIdx.x;
    if (e >= F + B) return;
    int src, dst;
    float *out;
    if (e < F) {
        const int b = e / S, s = e - b * S, first = s < S1 ? 0 : S1;
        src = e, dst = b * S + first, out = rel + 12 * (size_t)e;
        if (s == first) {
#pragma unroll
            for (int i = 0; i < 12; ++i) out[i] = (i % 5 == 0) ? 1.f : 0.f;
            return;
        }
    } else {
        const int b = e - F;
        src = b * S, dst = b * S + S1, out = gt + 12 * (size_t)b;
    }
    if (has_icp[e]) {   // d_calib @ icp @ inverse(s_calib), rows [:3]
        float sc[16], dc[16], pose[16], inv[16], t[16], m[16];
#pragma unroll
        for (int i = 0; i < 16; ++i)
            sc[i] = calib[16 * (size_t)src + i], dc[i] = calib[16 * (size_t)dst + i], pose[i] = icp[16 * (size_t)e + i];
        invert4(sc, inv);
        mul4(dc, pose, t);
        mul4(t, inv, m);
#pragma unroll
        for (int i = 0; i < 12; ++i) out[i] = m[i];
    } else {            // rt_global_to_relative: Rc^T Ro, Rc^T (To - Tc)
        float rc[9], ro[9], d[3];
#pragma unroll
        for (int i = 0; i < 9; ++i) rc[i] = R[9 * (size_t)dst + i], ro[i] = R[9 * (size_t)src + i];
#pragma unroll
        for (int k = 0; k < 3; ++k) d[k] = T[3 * (size_t)src + k] - T[3 * (size_t)dst + k];
#pragma unroll
        for (int i = 0; i < 3; ++i) {
#pragma unroll
            for (int j = 0; j < 3; ++j) out[4 * i + j] = fmaf(rc[6 + i], ro[6 + j], fmaf(rc[3 + i], ro[3 + j], rc[i] * ro[j]));
            out[4 * i + 3] = fmaf(rc[6 + i], d[2], fmaf(rc[3 + i], d[1], rc[i] * d[0]));
        }
    }
}

__device__ __forceinline__ void move3(const float *__restrict__ rt, float x, float y, float z, float &ox, float &oy, float &oz) {
    ox = fmaf(rt[2], z, fmaf(rt[1], y, rt[0] * x)) + rt[3];
    oy = fmaf(rt[6], z, fmaf(rt[5], y, rt[4] * x)) + rt[7];
    oz = fmaf(rt[10], z, fmaf(rt[9], y, rt[8] * x)) + rt[11];
}

// Row copy between the frame layout (F, C, N) and the map layout (B, rows, Sx*N): element (c, n) of frame (b, s) is
// element (c, sp*N + n) of map b, sp = the frame's place in its map.  TO_MAP: frame -> map (forward), else map -> frame.
// VEC: N % 4 == 0 and every base 16-byte aligned, so each row start is and no float4 straddles a row.
template <bool VEC, bool TO_MAP>
__device__ __forceinline__ void copy_rows(const float *__restrict__ in, float *__restrict__ out, int C, int N, size_t L,
                                          unsigned nblk) {
    const unsigned total = (unsigned)C * N / (VEC ? 4 : 1);   // shape_ok: C * N < 2^31
    for (unsigned i = blockIdx.x * 256 + threadIdx.x; i < total; i += nblk * 256) {
        const unsigned e = VEC ? i * 4 : i;
        const unsigned c = e / N, n = e - c * N;
        const size_t frame_at = (size_t)e, map_at = (size_t)c * L + (size_t)n;
        if (VEC) {
            if (TO_MAP) *reinterpret_cast<float4 *>(out + map_at) = *reinterpret_cast<const float4 *>(in + frame_at);
            else
                *reinterpret_cast<float4 *>(out + frame_at) =
                    in ? *reinterpret_cast<const float4 *>(in + map_at) : make_float4(0.f, 0.f, 0.f, 0.f);
        } else {
            if (TO_MAP) out[map_at] = in[frame_at];
            else out[frame_at] = in ? in[map_at] : 0.f;
        }
    }
}

// grid (nfb + ncb, F): the first nfb blocks of a frame copy its feature rows, the other ncb its points, mask and global coordinates
template <bool VEC>
__global__ __launch_bounds__(256) void map_assemble_fwd_kernel(
    const float *__restrict__ coor, const float *__restrict__ fea, const uint8_t *__restrict__ mask, const float *__restrict__ rel,
    const float *__restrict__ gt, int S, int S1, int N, int C, float scale, unsigned nfb, float *__restrict__ src_desc,
    float *__restrict__ dst_desc, uint8_t *__restrict__ src_mask, uint8_t *__restrict__ dst_mask, float *__restrict__ src_global,
    float *__restrict__ dst_global) {
    const int f = blockIdx.y, b = f / S, s = f - b * S;
    const bool is_src = s < S1;
    const int sp = is_src ? s : s - S1;
    const size_t L = (size_t)(is_src ? S1 : S - S1) * N, at = (size_t)sp * N;
    float *desc = (is_src ? src_desc : dst_desc) + (size_t)b * (C + 3) * L + at;
    if (blockIdx.x < nfb) {
        copy_rows<VEC, true>(fea + (size_t)f * C * N, desc, C, N, L, nfb);
        return;
    }
    const int n = (blockIdx.x - nfb) * 256 + threadIdx.x;
    if (n >= N) return;
    const float *p = coor + (size_t)f * 3 * N + n;
    float x = p[0] * scale, y = p[N] * scale, z = p[2 * (size_t)N] * scale;
    if (sp != 0) move3(rel + 12 * (size_t)f, x, y, z, x, y, z);
    float *xyz = desc + (size_t)C * L + n;
    xyz[0] = x, xyz[L] = y, xyz[2 * L] = z;
    (is_src ? src_mask : dst_mask)[(size_t)b * L + at + n] = mask[(size_t)f * N + n];
    float *g = (is_src ? src_global : dst_global) + (size_t)b * 3 * L + at + n;
    if (is_src) move3(gt + 12 * (size_t)b, x, y, z, x, y, z);
    g[0] = x, g[L] = y, g[2 * L] = z;
}

template <bool VEC>
__global__ __launch_bounds__(256) void map_assemble_bwd_kernel(const float *__restrict__ d_src, const float *__restrict__ d_dst,
                                                               int S, int S1, int N, int C, float *__restrict__ dfea) {
    const int f = blockIdx.y, b = f / S, s = f - b * S;
    const bool is_src = s < S1;
    const int sp = is_src ? s : s - S1;
    const size_t L = (size_t)(is_src ? S1 : S - S1) * N;
    const float *d = is_src ? d_src : d_dst;
    copy_rows<VEC, false>(d ? d + (size_t)b * (C + 3) * L + (size_t)sp * N : nullptr, dfea + (size_t)f * C * N, C, N, L, gridDim.x);
}

inline bool shape_ok(int B, int S, int S1, int N, int C) {
    return B >= 1 && S >= 2 && S1 >= 1 && S1 < S && N >= 1 && C >= 1 && (long long)B * S <= MAX_FRAMES &&
           (long long)(C + 3) * S * N < (1ll << 31);
}
inline bool aligned16(const void *p) { return (((uintptr_t)p) & 15) == 0; }
inline unsigned copy_blocks(int C, int N, bool vec) {
    const long long units = (long long)C * N / (vec ? 4 : 1);
    return (unsigned)std::min<long long>(std::max<long long>((units + 255) / 256, 1), 256);
}

}  // namespace

extern "C" int dpm_map_poses(const float *R, const float *T, const float *calib, const float *icp, const uint8_t *has_icp, int B,
                             int S, int S1, float *rel, float *gt, dpm_stream_t stream) {
    DPM_CHECK_ARG(R && T && calib && icp && has_icp && rel && gt);
    DPM_CHECK_ARG(B >= 1 && S >= 2 && S1 >= 1 && S1 < S && (long long)B * S <= MAX_FRAMES);
    map_poses_kernel<<<dpm_cdiv((long long)B * S + B, 64), 64, 0, (hipStream_t)stream>>>(R, T, calib, icp, has_icp, B, S, S1, rel, gt);
    return dpm_launch_status();
}

extern "C" int dpm_map_assemble_fwd(const float *coor, const float *fea, const uint8_t *mask, const float *rel, const float *gt,
                                    int B, int S, int S1, int N, int C, double coor_scale, float *src_desc, float *dst_desc,
                                    uint8_t *src_mask, uint8_t *dst_mask, float *src_global, float *dst_global,
                                    dpm_stream_t stream) {
    DPM_CHECK_ARG(coor && fea && mask && rel && gt && src_desc && dst_desc && src_mask && dst_mask && src_global && dst_global);
    DPM_CHECK_ARG(shape_ok(B, S, S1, N, C));
    const bool vec = (N & 3) == 0 && aligned16(fea) && aligned16(src_desc) && aligned16(dst_desc);
    const unsigned nfb = copy_blocks(C, N, vec);
    const dim3 grid(nfb + dpm_cdiv(N, 256), B * S);
    auto kernel = vec ? map_assemble_fwd_kernel<true> : map_assemble_fwd_kernel<false>;
    kernel<<<grid, 256, 0, (hipStream_t)stream>>>(coor, fea, mask, rel, gt, S, S1, N, C, (float)coor_scale, nfb, src_desc, dst_desc,
                                                  src_mask, dst_mask, src_global, dst_global);
    return dpm_launch_status();
}

extern "C" int dpm_map_assemble_bwd(const float *d_src_desc, const float *d_dst_desc, int B, int S, int S1, int N, int C, float *dfea,
                                    dpm_stream_t stream) {
    DPM_CHECK_ARG(dfea);
    DPM_CHECK_ARG(shape_ok(B, S, S1, N, C));
    const bool vec = (N & 3) == 0 && aligned16(dfea) && aligned16(d_src_desc) && aligned16(d_dst_desc);
    const dim3 grid(copy_blocks(C, N, vec), B * S);
    auto kernel = vec ? map_assemble_bwd_kernel<true> : map_assemble_bwd_kernel<false>;
    kernel<<<grid, 256, 0, (hipStream_t)stream>>>(d_src_desc, d_dst_desc, S, S1, N, C, dfea);
    return dpm_launch_status();
}
