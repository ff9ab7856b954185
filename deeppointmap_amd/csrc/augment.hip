// The training transforms on the GPU: GroundFilter, VoxelSample 'first' / 'center', the mask transforms
// (DistanceSample, RandomDrop, RandomShield), the point-wise maps (RandomRT, RandomPosJitter, CoordinatesNormalization,
// VerticalCorrect), the index transforms (RandomShuffle, RandomSample, FarthestPointSample) and the packing of S frames
// into the batch (reference dataloader/transforms.py:69-98, 174-227, 300-356, 375-474, 477-564; dataloader/body.py:155-161).
//
// ONE RULE: a frame is a fixed-capacity buffer plus a count that lives in device memory --
//   xyz (cap,3) fp32, orig_idx (cap,) int32, count (1,) int32.
// Every entry point takes the count as a device pointer, sizes its grid by the capacity and writes the new count to
// device memory, so a whole chain over a whole batch runs without the host knowing any intermediate length.  Rows at and
// past the count are never read: whatever they hold (NaN included) reaches no output and no statistic.
//
// Selections are stable, ordered compactions in the count / scan / write split of preprocess.hip: a block counts the
// survivors of its 4096-item chunk, ONE workgroup scans the block counts, a block writes its survivors at its offset.
// No kernel waits on another workgroup; the only atomics are integer atomics (the ground filter's cell table on
// order-preserving images of z, the voxel grid's minima), which are associative: two runs give identical bytes.
#include "block_scan.h"
#include "workspace.h"
#include <algorithm>

namespace {

constexpr int CH = 4096;          // items per compaction block
constexpr int MAX_WEDGES = 16;    // RandomShield: wedges per call (configs use max_num <= 4)
constexpr int PACK_MAX = 64;      // frames per pack launch (pointer table travels in the kernel arguments)
constexpr int NONE = 0x7fffffff;

__device__ __forceinline__ int frame_count(const int *count, int cap) { return max(0, min(*count, cap)); }

// torch.norm(xyz, p=2, dim=1) on the CPU: the fma chain of preprocess.hip's keep_point (pinned there against 400 000 points)
__device__ __forceinline__ float norm3(float x, float y, float z) { return sqrtf(fmaf(z, z, fmaf(y, y, x * x))); }

__device__ __forceinline__ unsigned ordered(float f) {  // as voxel_map.hip: unsigned order == float order
    const unsigned u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float unordered(unsigned o) { return __uint_as_float((o & 0x80000000u) ? (o ^ 0x80000000u) : ~o); }

// ---------------------------------------------------------------------------------------------------------------
// The compaction, over a functor K:  K::n() = size of the domain (read from device memory),  K::src(c) = the source
// row that item c of the domain keeps, or -1.  Output row p holds xyz[src], idx_in[src] (or src itself).
// ---------------------------------------------------------------------------------------------------------------
template <class K>
__global__ __launch_bounds__(256) void sel_count_kernel(const K keep, int *__restrict__ bcount) {
    __shared__ int s[4];
    const long long n = keep.n(), c0 = (long long)blockIdx.x * CH;
    if (c0 >= n) return;
    int cnt = 0;
    for (int k = threadIdx.x; k < CH; k += 256) {
        const long long c = c0 + k;
        if (c < n && keep.src(c) >= 0) ++cnt;
    }
    const int total = block_total<4>(cnt, s);
    if (threadIdx.x == 0) bcount[blockIdx.x] = total;
}

template <class K>
__global__ __launch_bounds__(1024) void sel_scan_kernel(const K keep, int *__restrict__ bcount, int max_blocks,
                                                        int32_t *__restrict__ n_out) {
    __shared__ int wsum[16];
    const int nblk = (int)min((long long)max_blocks, (keep.n() + CH - 1) / CH);
    const int run = block_scan_runs(bcount, nblk, (max_blocks + 1023) / 1024, wsum);
    if (threadIdx.x == 1023) *n_out = run;
}

template <class K>
__global__ __launch_bounds__(256) void sel_write_kernel(const K keep, const int *__restrict__ boff,
                                                        const float *__restrict__ xyz, const int32_t *__restrict__ idx_in,
                                                        float *__restrict__ out_xyz, int32_t *__restrict__ out_idx, int out_cap) {
    __shared__ int s_w[4];
    const long long n = keep.n(), c0 = (long long)blockIdx.x * CH;
    if (c0 >= n) return;
    // thread t owns 16 CONSECUTIVE items so that the block-level order equals the domain's order
    const int t = threadIdx.x;
    int src[CH / 256], cnt = 0;
#pragma unroll
    for (int k = 0; k < CH / 256; ++k) {
        const long long c = c0 + (long long)t * (CH / 256) + k;
        src[k] = c < n ? keep.src(c) : -1;
        cnt += src[k] >= 0;
    }
    int pos = block_scan_exclusive(cnt, s_w, boff[blockIdx.x]);
#pragma unroll
    for (int k = 0; k < CH / 256; ++k) {
        const int g = src[k];
        if (g < 0) continue;
        if (pos < out_cap) {
            out_xyz[3 * (size_t)pos] = xyz[3 * (size_t)g], out_xyz[3 * (size_t)pos + 1] = xyz[3 * (size_t)g + 1];
            out_xyz[3 * (size_t)pos + 2] = xyz[3 * (size_t)g + 2];
            if (out_idx) out_idx[pos] = idx_in ? idx_in[g] : g;
        }
        ++pos;
    }
}

template <class K>
int compact(const K &keep, int max_blocks, int *bcount, const float *xyz, const int32_t *idx_in, float *out_xyz,
            int32_t *out_idx, int out_cap, int32_t *n_out, hipStream_t st) {
    hipLaunchKernelGGL(sel_count_kernel<K>, dim3(max_blocks), dim3(256), 0, st, keep, bcount);
    hipLaunchKernelGGL(sel_scan_kernel<K>, dim3(1), dim3(1024), 0, st, keep, bcount, max_blocks, n_out);
    hipLaunchKernelGGL(sel_write_kernel<K>, dim3(max_blocks), dim3(256), 0, st, keep, bcount, xyz, idx_in, out_xyz, out_idx,
                       out_cap);
    return dpm_launch_status();
}

// ---------------------------------------------------------------------------------------------------------------
// GroundFilter: a dense img_len x img_width table of (count, ordered zmin, ordered zmax, lowest position)
// ---------------------------------------------------------------------------------------------------------------
struct GroundKeep {
    const float *xyz;
    const int *count;
    int cap, L, W, preserve, identity;
    float gw, hl, hw, gh;
    const unsigned *table;
    __device__ long long n() const { return frame_count(count, cap); }
    // int32(x / grid_width + img_len / 2) in float32, truncated towards zero: (-1, 0) lands in row 0 (transforms.py:191-194)
    __device__ int cell(int i) const {
        const float x = xyz[3 * (size_t)i], y = xyz[3 * (size_t)i + 1];
        const float fr = x / gw + hl, fc = y / gw + hw;
        if (!(fr > -1.f && fr < (float)L && fc > -1.f && fc < (float)W)) return -1;   // also NaN
        return (int)fr * W + (int)fc;
    }
    __device__ int src(long long c) const {
        const int i = (int)c;
        if (identity) return i;
        const int g = cell(i);
        if (g < 0) return -1;
        const unsigned *t = table + 4 * (size_t)g;
        if (t[0] < 3u) return -1;
        if (unordered(t[2]) - unordered(t[1]) > gh) return i;
        return (preserve && t[3] == (unsigned)i) ? i : -1;
    }
};

__global__ __launch_bounds__(256) void ground_fill_kernel(unsigned *__restrict__ table, int ncell) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c < ncell) {
        uint4 v;
        v.x = 0u, v.y = 0xffffffffu, v.z = 0u, v.w = 0xffffffffu;
        reinterpret_cast<uint4 *>(table)[c] = v;
    }
}

__global__ __launch_bounds__(256) void ground_mark_kernel(const GroundKeep k, unsigned *__restrict__ table) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= k.n()) return;
    const int g = k.cell(i);
    if (g < 0) return;
    unsigned *t = table + 4 * (size_t)g;
    const unsigned z = ordered(k.xyz[3 * (size_t)i + 2]);
    atomicAdd(&t[0], 1u);
    atomicMin(&t[1], z);
    atomicMax(&t[2], z);
    atomicMin(&t[3], (unsigned)i);
}

// ---------------------------------------------------------------------------------------------------------------
// VoxelSample 'first' / 'center'
// ---------------------------------------------------------------------------------------------------------------
struct VoxHdr {
    float lo[3], hi[3];
    int X, Y, Z;
    long long ncell;
    int n_out, overflow;   // adjacent: copied out as status[2]
};

struct VoxelKeep {
    const VoxHdr *hdr;
    const int *grid;
    __device__ long long n() const { return hdr->overflow ? 0 : hdr->ncell; }
    __device__ int src(long long c) const {
        const int g = grid[c];
        return g == NONE ? -1 : g;
    }
};

__global__ __launch_bounds__(1024) void vox_bbox_kernel(const float *__restrict__ xyz, const int *__restrict__ count, int cap,
                                                        float vs, long long max_cells, VoxHdr *__restrict__ hdr) {
    __shared__ float red[6][16];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int N = frame_count(count, cap);
    float lo[3] = {__builtin_inff(), __builtin_inff(), __builtin_inff()}, hi[3] = {-lo[0], -lo[0], -lo[0]};
    for (int i = t; i < N; i += 1024)
        for (int a = 0; a < 3; ++a) {
            const float v = xyz[(size_t)i * 3 + a];
            lo[a] = fminf(lo[a], v), hi[a] = fmaxf(hi[a], v);
        }
    for (int a = 0; a < 3; ++a) {
        lo[a] = -wave_max_dpp(-lo[a]), hi[a] = wave_max_dpp(hi[a]);
        if (lane == 0) red[a][w] = lo[a], red[3 + a][w] = hi[a];
    }
    __syncthreads();
    if (t == 0) {
        for (int a = 0; a < 3; ++a) {
            for (int k = 0; k < 16; ++k) lo[a] = fminf(lo[a], red[a][k]), hi[a] = fmaxf(hi[a], red[3 + a][k]);
            hdr->lo[a] = lo[a], hdr->hi[a] = hi[a];
        }
        hdr->n_out = 0;
        if (N == 0) {   // an empty frame stays empty
            hdr->X = hdr->Y = hdr->Z = 0, hdr->ncell = 0, hdr->overflow = 0;
            return;
        }
        const int X = (int)((hi[0] - lo[0]) / vs) + 1, Y = (int)((hi[1] - lo[1]) / vs) + 1, Z = (int)((hi[2] - lo[2]) / vs) + 1;
        hdr->X = X, hdr->Y = Y, hdr->Z = Z;
        hdr->ncell = (long long)X * Y * Z;
        // X, Y, Z >= 1 for finite coordinates; a non-finite one makes a term <= 0 or the product huge
        hdr->overflow = (X < 1 || Y < 1 || Z < 1 || hdr->ncell > max_cells || hdr->ncell > 0x7fffffffLL) ? 1 : 0;
    }
}

__global__ __launch_bounds__(256) void vox_fill_kernel(const VoxHdr *__restrict__ hdr, int *__restrict__ grid,
                                                       unsigned long long *__restrict__ dist) {
    if (hdr->overflow) return;
    const long long n = hdr->ncell;
    for (long long c = (long long)blockIdx.x * 256 + threadIdx.x; c < n; c += (long long)gridDim.x * 256) {
        grid[c] = NONE;
        if (dist) dist[c] = ~0ull;
    }
}

// pass 0: 'first' -> atomicMin(position); 'center' -> atomicMin(bits of the fp64 centre distance)
// pass 1: 'center' -> the points that hold their voxel's minimum distance race for the lowest position
__global__ __launch_bounds__(256) void vox_mark_kernel(const float *__restrict__ xyz, const int *__restrict__ count, int cap,
                                                       float vs, double vsd, int center, int pass,
                                                       const VoxHdr *__restrict__ hdr, int *__restrict__ grid,
                                                       unsigned long long *__restrict__ dist) {
    if (hdr->overflow) return;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= frame_count(count, cap)) return;
    const float *p = xyz + (size_t)i * 3;
    const float r0 = p[0] - hdr->lo[0], r1 = p[1] - hdr->lo[1], r2 = p[2] - hdr->lo[2];
    const int vx = (int)(r0 / vs), vy = (int)(r1 / vs), vz = (int)(r2 / vs);
    if (vx < 0 || vy < 0 || vz < 0 || vx >= hdr->X || vy >= hdr->Y || vz >= hdr->Z) return;   // NaN coordinates
    const int id = vx + vy * hdr->X + vz * hdr->X * hdr->Y;
    if (!center) {
        atomicMin(&grid[id], i);
        return;
    }
    // np.sum((relative_xyz - voxel_xyz * voxel_size - voxel_size / 2) ** 2, axis=-1): int32 * python float promotes to
    // float64, so the distance is fp64 of the fp32 relative coordinate against the DOUBLE voxel size (transforms.py:344)
    const double half = vsd / 2;
    const double d0 = ((double)r0 - (double)vx * vsd) - half, d1 = ((double)r1 - (double)vy * vsd) - half,
                 d2 = ((double)r2 - (double)vz * vsd) - half;
    const double d = (d0 * d0 + d1 * d1) + d2 * d2;
    const unsigned long long bits = (unsigned long long)__double_as_longlong(d);   // d >= 0: bit order == value order
    if (pass == 0)
        atomicMin(&dist[id], bits);
    else if (dist[id] == bits)
        atomicMin(&grid[id], i);
}

// ---------------------------------------------------------------------------------------------------------------
// mask transforms
// ---------------------------------------------------------------------------------------------------------------
struct MaskKeep {
    const float *xyz;
    const int *count;
    int cap, use_dist, nw;
    float dmin, dmax, ratio;
    const float *u;
    float w[MAX_WEDGES][4];   // start, end (already - 360 when the wedge wraps), wraps, distance threshold
    __device__ long long n() const { return frame_count(count, cap); }
    __device__ int src(long long c) const {
        const int i = (int)c;
        const float x = xyz[3 * (size_t)i], y = xyz[3 * (size_t)i + 1], z = xyz[3 * (size_t)i + 2];
        const float d = norm3(x, y, z);
        if (use_dist && !(dmin <= d && d <= dmax)) return -1;
        if (u && !(u[i] >= ratio)) return -1;
        if (nw > 0) {
            const float az = atan2f(y, x) * 180.f / 3.14159265358979323846f;   // transforms.py:453
            for (int k = 0; k < nw; ++k) {
                const bool in = w[k][2] != 0.f ? (az >= w[k][0] || az <= w[k][1]) : (az >= w[k][0] && az <= w[k][1]);
                if (in && d >= w[k][3]) return -1;
            }
        }
        return i;
    }
};

// ---------------------------------------------------------------------------------------------------------------
// point-wise maps, in place on the first count rows
// ---------------------------------------------------------------------------------------------------------------
struct AffineArgs {
    float m[12];        // mode 0: R (row-major 9) then T (3);  mode 2: m[0] = ratio
    double sn, cs;      // mode 3: sin / cos of the correction angle
};

__global__ __launch_bounds__(256) void affine_kernel(float *__restrict__ xyz, const int *__restrict__ count, int cap, int mode,
                                                     const AffineArgs a, const float *__restrict__ jitter) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= frame_count(count, cap)) return;
    float *p = xyz + 3 * (size_t)i;
    const float x = p[0], y = p[1], z = p[2];
    if (mode == 0) {          // R_aug x + T_aug (transforms.py:529)
        p[0] = fmaf(a.m[2], z, fmaf(a.m[1], y, a.m[0] * x)) + a.m[9];
        p[1] = fmaf(a.m[5], z, fmaf(a.m[4], y, a.m[3] * x)) + a.m[10];
        p[2] = fmaf(a.m[8], z, fmaf(a.m[7], y, a.m[6] * x)) + a.m[11];
    } else if (mode == 1) {   // xyz += jitter (transforms.py:563)
        p[0] = x + jitter[3 * (size_t)i], p[1] = y + jitter[3 * (size_t)i + 1], p[2] = z + jitter[3 * (size_t)i + 2];
    } else if (mode == 2) {   // xyz /= ratio: a true division (transforms.py:406)
        p[0] = x / a.m[0], p[1] = y / a.m[0], p[2] = z / a.m[0];
    } else {                  // VerticalCorrect (transforms.py:311-317): Rodrigues about k = normalize(x cross z) = (y, -x, 0) / |.|
        const double nx = (double)y, ny = -(double)x, nrm = sqrt(nx * nx + ny * ny);
        const double ka = nx / nrm, kb = ny / nrm, oc = 1.0 - a.cs;   // on the z axis: 0 / 0 = NaN, as in the reference
        // R = I + sin K + (1 - cos) K^2 in fp64, rounded to fp32 before it multiplies the point
        const float r00 = (float)(1.0 + oc * (ka * ka - 1.0)), r01 = (float)(oc * ka * kb), r02 = (float)(a.sn * kb);
        const float r10 = r01, r11 = (float)(1.0 + oc * (kb * kb - 1.0)), r12 = (float)(-a.sn * ka);
        const float r20 = (float)(-a.sn * kb), r21 = (float)(a.sn * ka), r22 = (float)a.cs;
        p[0] = fmaf(r02, z, fmaf(r01, y, r00 * x));
        p[1] = fmaf(r12, z, fmaf(r11, y, r10 * x));
        p[2] = fmaf(r22, z, fmaf(r21, y, r20 * x));
    }
}

// ---------------------------------------------------------------------------------------------------------------
// index transforms: out[j] = in[sel[j]]
// ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void gather_kernel(const float *__restrict__ xyz, const int32_t *__restrict__ idx_in,
                                                     const int *__restrict__ count, int cap, const int32_t *__restrict__ sel,
                                                     int n_sel, int limit, float *__restrict__ out_xyz,
                                                     int32_t *__restrict__ out_idx, int32_t *__restrict__ out_count) {
    const int n_in = frame_count(count, cap);
    const bool same = limit >= 0 && n_in <= limit;   // RandomSample / FarthestPointSample leave a short frame untouched
    const int n_out = same ? n_in : min(min(limit < 0 ? n_in : limit, n_sel), cap);
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j == 0) *out_count = n_out;
    if (j >= n_out) return;
    int s = same ? j : sel[j];
    const bool ok = s >= 0 && s < n_in;               // an index outside the frame gives a zero row and index -1
    out_xyz[3 * (size_t)j] = ok ? xyz[3 * (size_t)s] : 0.f;
    out_xyz[3 * (size_t)j + 1] = ok ? xyz[3 * (size_t)s + 1] : 0.f;
    out_xyz[3 * (size_t)j + 2] = ok ? xyz[3 * (size_t)s + 2] : 0.f;
    if (out_idx) out_idx[j] = ok ? (idx_in ? idx_in[s] : s) : -1;
}

// ---------------------------------------------------------------------------------------------------------------
// ToTensor(padding_to) + map_collate_fn for S frames
// ---------------------------------------------------------------------------------------------------------------
struct PackArgs {
    const float *xyz[PACK_MAX];
    const int *count[PACK_MAX];
    int cap[PACK_MAX];
};

__global__ __launch_bounds__(256) void pack_kernel(const PackArgs a, int s0, int P, float *__restrict__ points,
                                                   unsigned char *__restrict__ padding, int32_t *__restrict__ status) {
    const int s = blockIdx.y, j = blockIdx.x * 256 + threadIdx.x;
    const int n = frame_count(a.count[s], a.cap[s]);
    if (j == 0) status[2 * (size_t)(s0 + s)] = n, status[2 * (size_t)(s0 + s) + 1] = n > P;
    if (j >= P) return;
    const bool live = j < n && n <= P;   // a frame longer than padding_to writes nothing but its overflow flag
    const float *p = a.xyz[s] + 3 * (size_t)j;
    float *o = points + (size_t)(s0 + s) * 3 * P + j;
    o[0] = live ? p[0] : 0.f, o[(size_t)P] = live ? p[1] : 0.f, o[2 * (size_t)P] = live ? p[2] : 0.f;
    padding[(size_t)(s0 + s) * P + j] = j >= n;
}

// One buffer serves the three selections in turn, each with a layout of its own from the aligned base on.
struct GroundWs { unsigned *table; int *bcount; };   // 16 bytes a cell, then the block counts
GroundWs ground_layout(WsCursor &c, int capacity, long long ncell) {
    GroundWs w;
    w.table = c.take<unsigned>(4 * (size_t)ncell);
    w.bcount = c.take<int>((size_t)dpm_cdiv(capacity, CH));
    return w;
}
struct VoxelWs {
    VoxHdr *hdr;
    unsigned long long *dist;   // 8 + 4 bytes a cell
    int *grid, *bcount;
};
VoxelWs voxel_layout(WsCursor &c, long long max_cells) {
    VoxelWs w;
    w.hdr = c.take<VoxHdr>(1);
    c.align256();
    w.dist = c.take<unsigned long long>((size_t)max_cells);
    w.grid = c.take<int>((size_t)max_cells);
    w.bcount = c.take<int>((size_t)(max_cells / CH + 1));
    return w;
}
int *mask_layout(WsCursor &c, int capacity) { return c.take<int>((size_t)dpm_cdiv(capacity, CH)); }

}  // namespace

extern "C" size_t dpm_augment_workspace_bytes(int capacity, long long cells) {
    // header + the ground table (16 bytes a cell) or the voxel grids (12 bytes a cell) + the block counts of either domain:
    // a bound on the three layouts above rather than the largest of them, kept to the byte (callers size one buffer for the
    // whole chain by it).  The one size that is a formula of its own; the layouts are measured next to it so that a slice
    // added to one of them cannot outgrow it unnoticed.
    if (capacity < 0 || cells < 0) return 0;
    WsCursor ground(nullptr), voxel(nullptr), mask(nullptr);
    ground_layout(ground, capacity, cells), voxel_layout(voxel, cells), mask_layout(mask, capacity);
    const size_t bound = 1024 + 16 * (size_t)cells + sizeof(int) * ((size_t)cells / CH + (size_t)capacity / CH + 4);
    return std::max(bound, std::max(ground.bytes(), std::max(voxel.bytes(), mask.bytes())));
}

extern "C" int dpm_ground_filter(const float *xyz, const int32_t *idx_in, const int32_t *count, int capacity, int img_len,
                                 int img_width, double grid_width, double ground_height, int preserve_sparse_ground,
                                 float *out_xyz, int32_t *out_idx, int32_t *out_count, void *workspace, dpm_stream_t stream) {
    DPM_CHECK_ARG(xyz && count && out_xyz && out_count && workspace && capacity >= 1 && img_len >= 1 && img_width >= 1);
    DPM_CHECK_ARG(grid_width > 0.0 && (long long)img_len * img_width <= (1 << 26) && out_xyz != xyz && out_count != count);
    hipStream_t st = (hipStream_t)stream;
    const int ncell = img_len * img_width, max_blocks = (int)dpm_cdiv(capacity, CH);
    WsCursor c(workspace);
    const auto [table, bcount] = ground_layout(c, capacity, ncell);
    GroundKeep k;
    k.xyz = xyz, k.count = count, k.cap = capacity, k.L = img_len, k.W = img_width, k.preserve = preserve_sparse_ground != 0;
    k.identity = !(ground_height > 0.0);   // transforms.py:186
    k.gw = (float)grid_width, k.hl = (float)(img_len / 2.0), k.hw = (float)(img_width / 2.0), k.gh = (float)ground_height;
    k.table = table;
    if (!k.identity) {
        hipLaunchKernelGGL(ground_fill_kernel, dim3(dpm_cdiv(ncell, 256)), dim3(256), 0, st, table, ncell);
        hipLaunchKernelGGL(ground_mark_kernel, dim3(dpm_cdiv(capacity, 256)), dim3(256), 0, st, k, table);
    }
    return compact(k, max_blocks, bcount, xyz, idx_in, out_xyz, out_idx, capacity, out_count, st);
}

extern "C" int dpm_voxel_select(const float *xyz, const int32_t *idx_in, const int32_t *count, int capacity, double voxel_size,
                                int retention, long long max_cells, float *out_xyz, int32_t *out_idx, int32_t *status,
                                void *workspace, dpm_stream_t stream) {
    DPM_CHECK_ARG(xyz && count && out_xyz && status && workspace && capacity >= 1 && voxel_size > 0.0);
    DPM_CHECK_ARG(max_cells >= CH && max_cells <= 0x7fffffffLL && (retention == 0 || retention == 1) && out_xyz != xyz);
    hipStream_t st = (hipStream_t)stream;
    WsCursor c(workspace);
    const auto [hdr, dist, grid, bcount] = voxel_layout(c, max_cells);
    const int max_blocks = (int)(max_cells / CH + 1);
    const float vs = (float)voxel_size;
    hipLaunchKernelGGL(vox_bbox_kernel, dim3(1), dim3(1024), 0, st, xyz, count, capacity, vs, max_cells, hdr);
    hipLaunchKernelGGL(vox_fill_kernel, dim3(2048), dim3(256), 0, st, hdr, grid, retention ? dist : nullptr);
    for (int pass = 0; pass <= retention; ++pass)
        hipLaunchKernelGGL(vox_mark_kernel, dim3(dpm_cdiv(capacity, 256)), dim3(256), 0, st, xyz, count, capacity, vs, voxel_size,
                           retention, pass, hdr, grid, dist);
    VoxelKeep k;
    k.hdr = hdr, k.grid = grid;
    const int rc = compact(k, max_blocks, bcount, xyz, idx_in, out_xyz, out_idx, capacity, &hdr->n_out, st);
    if (rc != DPM_OK) return rc;
    // status = [n_out, overflow]: two ints copied device-to-device; status[0] serves as the frame's new count
    hipError_t e = hipMemcpyAsync(status, &hdr->n_out, 2 * sizeof(int), hipMemcpyDeviceToDevice, st);
    if (e != hipSuccess) return (int)e;
    return dpm_launch_status();
}

extern "C" int dpm_mask_select(const float *xyz, const int32_t *idx_in, const int32_t *count, int capacity, int use_distance,
                               double min_dis, double max_dis, const float *u, double drop_ratio, const float *wedges,
                               int n_wedges, float *out_xyz, int32_t *out_idx, int32_t *out_count, void *workspace,
                               dpm_stream_t stream) {
    DPM_CHECK_ARG(xyz && count && out_xyz && out_count && workspace && capacity >= 1 && out_xyz != xyz && out_count != count);
    DPM_CHECK_ARG(n_wedges >= 0 && (n_wedges == 0 || wedges));
    if (n_wedges > MAX_WEDGES) return DPM_EUNSUPPORTED;
    MaskKeep k;
    k.xyz = xyz, k.count = count, k.cap = capacity, k.use_dist = use_distance != 0, k.nw = n_wedges;
    k.dmin = (float)min_dis, k.dmax = (float)max_dis, k.ratio = (float)drop_ratio, k.u = u;
    for (int i = 0; i < MAX_WEDGES; ++i)
        for (int j = 0; j < 4; ++j) k.w[i][j] = i < n_wedges ? wedges[4 * i + j] : 0.f;   // `wedges` is HOST memory
    WsCursor c(workspace);
    return compact(k, (int)dpm_cdiv(capacity, CH), mask_layout(c, capacity), xyz, idx_in, out_xyz, out_idx, capacity, out_count,
                   (hipStream_t)stream);
}

extern "C" int dpm_points_affine(float *xyz, const int32_t *count, int capacity, int mode, const double *params,
                                 const float *jitter, dpm_stream_t stream) {
    DPM_CHECK_ARG(xyz && count && capacity >= 1 && mode >= 0 && mode <= 3);
    DPM_CHECK_ARG(mode == 1 ? jitter != nullptr : params != nullptr);
    AffineArgs a = {};
    if (mode == 0)
        for (int i = 0; i < 12; ++i) a.m[i] = (float)params[i];
    else if (mode == 2) {
        DPM_CHECK_ARG(params[0] != 0.0);
        a.m[0] = (float)params[0];
    } else if (mode == 3)
        a.sn = params[0], a.cs = params[1];
    hipLaunchKernelGGL(affine_kernel, dim3(dpm_cdiv(capacity, 256)), dim3(256), 0, (hipStream_t)stream, xyz, count, capacity, mode,
                       a, jitter);
    return dpm_launch_status();
}

extern "C" int dpm_gather_points(const float *xyz, const int32_t *idx_in, const int32_t *count, int capacity,
                                 const int32_t *sel, int n_sel, int limit, float *out_xyz, int32_t *out_idx,
                                 int32_t *out_count, dpm_stream_t stream) {
    DPM_CHECK_ARG(xyz && count && sel && out_xyz && out_count && capacity >= 1 && n_sel >= 0 && out_xyz != xyz);
    DPM_CHECK_ARG(out_count != count);
    hipLaunchKernelGGL(gather_kernel, dim3(dpm_cdiv(capacity, 256)), dim3(256), 0, (hipStream_t)stream, xyz, idx_in, count,
                       capacity, sel, n_sel, limit, out_xyz, out_idx, out_count);
    return dpm_launch_status();
}

extern "C" int dpm_pack_frames(const float *const *xyz, const int32_t *const *counts, const int32_t *capacities, int S,
                               int padding_to, float *points, unsigned char *padding, int32_t *status,
                               dpm_stream_t stream) {
    DPM_CHECK_ARG(xyz && counts && capacities && S >= 1 && padding_to >= 1 && points && padding && status);
    for (int s = 0; s < S; ++s) DPM_CHECK_ARG(xyz[s] && counts[s] && capacities[s] >= 1);
    for (int s0 = 0; s0 < S; s0 += PACK_MAX) {
        PackArgs a = {};
        const int n = S - s0 < PACK_MAX ? S - s0 : PACK_MAX;
        for (int s = 0; s < n; ++s) a.xyz[s] = xyz[s0 + s], a.count[s] = counts[s0 + s], a.cap[s] = capacities[s0 + s];
        hipLaunchKernelGGL(pack_kernel, dim3(dpm_cdiv(padding_to, 256), n), dim3(256), 0, (hipStream_t)stream, a, s0, padding_to,
                           points, padding, status);
    }
    return dpm_launch_status();
}
