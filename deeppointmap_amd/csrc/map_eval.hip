// Map evaluation: how far a point-cloud map lies from the surfaces it should lie on.  No counterpart in the reference: pinned
// to this project's own restatement (tests/map_eval_restated.py) and to constructed cases with known answers.
//
//   dpm_scene_distance  per map point the unsigned distance to the nearest surface of a simulator scene (ground plane,
//                       oriented boxes, capped vertical cylinders: deeppointmap_amd/lidar_sim.py) and that surface's id.
//                       One lane per point; the records pass through LDS in tiles of TILE, every lane reads the same
//                       record (an LDS broadcast).  P x M evaluations, no culling, no grid.
//   dpm_cloud_nn        exact truncated nearest neighbour from a query cloud to a target cloud.  The target is counting-
//                       sorted into a uniform 3-D grid once per call (setup, count, scan, scatter: the shape of csrc/icp.hip)
//                       with a cell edge of at least max_dist, four lanes per query scan the 3 x 3 x 3 cells around it.
//   dpm_distance_stats  a distance array -> a small fp64 table (counts, sums, maximum, counts under thresholds) per class
//                       and in total, in two launches with every order of summation fixed.
//
// Clouds are (3,M) fp32 channel-first.  Every point is shifted ONCE, q = (float)((double)p - origin), origin three doubles by
// value; everything after that is fp32 on numbers no larger than the map's extent (the reasoning of the cull's change of frame
// in csrc/lidar_sim.hip).  Arithmetic: + - * / sqrt, each rounded once (the build has contraction off; there is no fmaf here),
// so a float32 numpy restatement that follows the stated order of operations gives the same bits.  No floating-point atomics:
// two runs give identical bytes.  The integer atomics of the grid build decide the order inside a cell, and the (distance bits,
// index) key makes the result independent of it.
#include <math.h>

#include "block_scan.h"
#include "cell_grid.h"
#include "workspace.h"

namespace {

constexpr int REC = 12;       // floats per scene record: c - origin (3), cos, sin, extents (3), kind as bits, padding (3)
constexpr int TILE = 64;      // records per LDS tile
constexpr int GMAX = 128;     // grid cells per axis (upper bound) of the neighbour search
constexpr int SCH = 4096;     // least points per block of the statistics
constexpr int SBLK = 1024;    // most blocks of the statistics
constexpr int SCOL = 5;       // columns before the thresholds

__device__ __forceinline__ float shifted(float p, double o) { return (float)((double)p - o); }
__device__ __forceinline__ bool finite_f(float v) { return fabsf(v) < INFINITY; }   // false for Inf and NaN
__device__ __forceinline__ float fmax_(float a, float b) { return a > b ? a : b; }
__device__ __forceinline__ float fmin_(float a, float b) { return a < b ? a : b; }

// ---- scene distance: grid (ceil(M / 256)), 256 threads, one lane per point.
// Order of operations, per point and record, with q the shifted point, c the record's centre and d = q - c (per axis):
//   box       lx = cos*dx + sin*dy, ly = cos*dy - sin*dx, lz = dz; a_k = |l_k| - h_k, o_k = max(a_k, 0);
//             dist = |sqrt((ox*ox + oy*oy) + oz*oz) + min(max(ax, max(ay, az)), 0)|
//   cylinder  a0 = sqrt(dx*dx + dy*dy) - r, a1 = |dz| - hh, o_k = max(a_k, 0);
//             dist = |sqrt(o0*o0 + o1*o1) + min(max(a0, a1), 0)|
//   ground    |qz - z0'|
// Records in ascending index, a strictly smaller distance wins, the ground last.
__global__ __launch_bounds__(256) void scene_distance_kernel(const float *__restrict__ pts, int M, const float *__restrict__ recs,
                                                             int P, float ground, int has_ground, double ox, double oy, double oz,
                                                             float *__restrict__ dist, int32_t *__restrict__ surf) {
    __shared__ float s_rec[TILE * REC];
    const int i = blockIdx.x * 256 + threadIdx.x;
    const bool live = i < M;
    const float qx = live ? shifted(pts[i], ox) : 0.f, qy = live ? shifted(pts[(size_t)M + i], oy) : 0.f,
                qz = live ? shifted(pts[2 * (size_t)M + i], oz) : 0.f;
    float best = INFINITY;
    int bid = -1;
    for (int k0 = 0; k0 < P; k0 += TILE) {
        const int m = min(TILE, P - k0);
        __syncthreads();
        for (int j = threadIdx.x; j < m * REC; j += 256) s_rec[j] = recs[(size_t)k0 * REC + j];
        __syncthreads();
        for (int k = 0; k < m; ++k) {
            const float *r = s_rec + k * REC;
            const float dx = qx - r[0], dy = qy - r[1], dz = qz - r[2];
            float d;
            if (__float_as_int(r[8]) == 0) {   // box, half extents r[5..7]
                const float lx = r[3] * dx + r[4] * dy, ly = r[3] * dy - r[4] * dx;
                const float ax = fabsf(lx) - r[5], ay = fabsf(ly) - r[6], az = fabsf(dz) - r[7];
                const float px = fmax_(ax, 0.f), py = fmax_(ay, 0.f), pz = fmax_(az, 0.f);
                d = fabsf(sqrtf((px * px + py * py) + pz * pz) + fmin_(fmax_(ax, fmax_(ay, az)), 0.f));
            } else {                           // cylinder about its middle: radius r[5], half height r[6]
                const float a0 = sqrtf(dx * dx + dy * dy) - r[5], a1 = fabsf(dz) - r[6];
                const float p0 = fmax_(a0, 0.f), p1 = fmax_(a1, 0.f);
                d = fabsf(sqrtf(p0 * p0 + p1 * p1) + fmin_(fmax_(a0, a1), 0.f));
            }
            if (d < best) best = d, bid = k0 + k;
        }
    }
    if (has_ground) {   // the ground last: it takes a tie from nobody
        const float d = fabsf(qz - ground);
        if (d < best) best = d, bid = P;
    }
    if (!live) return;
    const bool ok = finite_f(qx) && finite_f(qy) && finite_f(qz);
    dist[i] = ok ? best : INFINITY;
    surf[i] = ok ? bid : -1;
}

// ---- cloud nearest neighbour
struct NnHdr {   // start of the workspace (256 bytes reserved)
    float lox, loy, loz, inv_cs;
    int gx, gy, gz, ncell;
};

struct NnArgs {
    const float *qry, *tgt;   // (3,Nq), (3,Nt)
    int Nq, Nt;
    double ox, oy, oz;
    char *ws;
};

__device__ __forceinline__ NnHdr *nn_hdr(const NnArgs &a) { return (NnHdr *)a.ws; }
// cell c holds sorted[cells[c] .. cells[c + 1])   (ncell + 1 entries)
__device__ __forceinline__ int *nn_cells(const NnArgs &a) { return (int *)(a.ws + 256); }
__device__ __forceinline__ float4 *nn_sorted(const NnArgs &a) {
    return (float4 *)(a.ws + 256 + sizeof(int) * ((size_t)GMAX * GMAX * GMAX + 4));
}

// One workgroup: the bounds of the shifted targets with finite coordinates, the grid header, the cell counters zeroed.
// Cell edge = max(1.001 max_dist, extent / (GMAX - 1)): past GMAX cells per axis the edge grows, the search stays exact.
__global__ __launch_bounds__(1024) void nn_setup_kernel(NnArgs A, float radius) {
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int i = t; i < A.Nt; i += 1024) {
        const float x = shifted(A.tgt[i], A.ox), y = shifted(A.tgt[(size_t)A.Nt + i], A.oy),
                    z = shifted(A.tgt[2 * (size_t)A.Nt + i], A.oz);
        if (!(finite_f(x) && finite_f(y) && finite_f(z))) continue;
        lo[0] = fminf(lo[0], x), hi[0] = fmaxf(hi[0], x), lo[1] = fminf(lo[1], y), hi[1] = fmaxf(hi[1], y);
        lo[2] = fminf(lo[2], z), hi[2] = fmaxf(hi[2], z);
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) lo[k] = wave_min(lo[k]), hi[k] = wave_max(hi[k]);
    __shared__ float red[6][16];
    __shared__ int s_ncell;
    if (lane == 0)
        for (int k = 0; k < 3; ++k) red[k][w] = lo[k], red[3 + k][w] = hi[k];
    __syncthreads();
    if (t == 0) {
        for (int j = 1; j < 16; ++j)
            for (int k = 0; k < 3; ++k) lo[k] = fminf(lo[k], red[k][j]), hi[k] = fmaxf(hi[k], red[3 + k][j]);
        NnHdr *hdr = nn_hdr(A);
        int g[3] = {1, 1, 1};
        float cs = radius * 1.001f;
        const bool usable = hi[0] >= lo[0] && hi[1] >= lo[1] && hi[2] >= lo[2];   // at least one finite target
        if (usable) {
            const float ext = fmaxf(fmaxf(hi[0] - lo[0], hi[1] - lo[1]), hi[2] - lo[2]);
            cs = fmaxf(cs, ext / (float)(GMAX - 1));
            if (!(cs < INFINITY)) cs = 3e38f;   // an extent beyond float: one cell
            for (int k = 0; k < 3; ++k) g[k] = min(GMAX, (int)fminf((hi[k] - lo[k]) / cs, (float)GMAX) + 1);
        } else {
            lo[0] = lo[1] = lo[2] = 0.f;
        }
        hdr->lox = lo[0], hdr->loy = lo[1], hdr->loz = lo[2], hdr->inv_cs = 1.0f / cs;
        hdr->gx = g[0], hdr->gy = g[1], hdr->gz = g[2], hdr->ncell = g[0] * g[1] * g[2];
        s_ncell = g[0] * g[1] * g[2];
    }
    __syncthreads();
    int *cells = nn_cells(A);
    for (int c = t; c <= s_ncell; c += 1024) cells[c] = 0;
}

// the two passes of the counting sort around nn_scan_kernel (grid_count_or_place of cell_grid.h).
// A target with a non-finite coordinate is in no cell: it is nobody's neighbour.
template <bool PLACE>
__global__ __launch_bounds__(256) void nn_grid_kernel(NnArgs A) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= A.Nt) return;
    const NnHdr *hdr = nn_hdr(A);
    const float x = shifted(A.tgt[i], A.ox), y = shifted(A.tgt[(size_t)A.Nt + i], A.oy),
                z = shifted(A.tgt[2 * (size_t)A.Nt + i], A.oz);
    if (!(finite_f(x) && finite_f(y) && finite_f(z))) return;
    const int c = (cell_coord(z, hdr->loz, hdr->inv_cs, hdr->gz) * hdr->gy + cell_coord(y, hdr->loy, hdr->inv_cs, hdr->gy)) * hdr->gx +
                  cell_coord(x, hdr->lox, hdr->inv_cs, hdr->gx);
    grid_count_or_place<PLACE>(nn_cells(A), nn_sorted(A), A.Nt, c, x, y, z, i);
}

// exclusive prefix sum of cells[1 .. ncell] in place, one workgroup (thread t owns a contiguous run of cells)
__global__ __launch_bounds__(1024) void nn_scan_kernel(NnArgs A) {
    __shared__ int wsum[16];
    const int ncell = nn_hdr(A)->ncell;
    block_scan_runs(nn_cells(A) + 1, ncell, (ncell + 1023) / 1024, wsum);
}

// grid (ceil(Nq / 64)), 256 threads: four lanes per query.  d2 = (dx*dx + dy*dy) + dz*dz on the shifted coordinates; the
// winner is the smallest (d2 bits, original index) key among the targets of the 3 x 3 x 3 cells, accepted when
// d2 <= r2 = (float)(max_dist * max_dist); dist = sqrt(d2).
__global__ __launch_bounds__(256) void nn_search_kernel(NnArgs A, float r2, float *__restrict__ dist, int32_t *__restrict__ idx) {
    const NnHdr *hdr = nn_hdr(A);
    const int *cells = nn_cells(A);
    const float4 *sorted = nn_sorted(A);
    const int gx = hdr->gx, gy = hdr->gy, gz = hdr->gz;
    const float inv_cs = hdr->inv_cs;
    const int i = blockIdx.x * 64 + (threadIdx.x >> 2), ql = threadIdx.x & 3;   // uniform inside a quad
    if (i >= A.Nq) return;
    const float qx = shifted(A.qry[i], A.ox), qy = shifted(A.qry[(size_t)A.Nq + i], A.oy),
                qz = shifted(A.qry[2 * (size_t)A.Nq + i], A.oz);
    const float flx = floorf((qx - hdr->lox) * inv_cs), fly = floorf((qy - hdr->loy) * inv_cs),
                flz = floorf((qz - hdr->loz) * inv_cs);
    // fminf / fmaxf drop a NaN: such a query looks at cells it has no business in and finds NaN distances there = no hit
    const int cx = (int)fmaxf(fminf(flx, 1e6f), -1e6f), cy = (int)fmaxf(fminf(fly, 1e6f), -1e6f),
              cz = (int)fmaxf(fminf(flz, 1e6f), -1e6f);
    const int xa = min(max(cx - 1, 0), gx), xb = min(max(cx + 2, 0), gx);
    unsigned long long best = ~0ull;
    // a row's cells xa .. xb-1 are one range of `sorted`; the range ends of all nine rows are requested before the first is used
    int rlo[9], rhi[9];
#pragma unroll
    for (int r = 0; r < 9; ++r) {
        const int yy = cy - 1 + r % 3, zz = cz - 1 + r / 3;
        const bool in = yy >= 0 && yy < gy && zz >= 0 && zz < gz && xa < xb;
        const int row = (min(max(zz, 0), gz - 1) * gy + min(max(yy, 0), gy - 1)) * gx;
        rlo[r] = in ? cells[row + xa] : 0, rhi[r] = in ? cells[row + xb] : 0;
    }
#pragma unroll
    for (int r = 0; r < 9; ++r) quad_scan_range(sorted, max(rlo[r], 0), min(rhi[r], A.Nt), ql, qx, qy, qz, best);
    best = quad_min_key(best);
    if (ql != 0) return;
    const float d2 = __uint_as_float((unsigned)(best >> 32));
    const bool hit = best != ~0ull && d2 <= r2;   // a NaN distance is no hit
    dist[i] = hit ? sqrtf(d2) : INFINITY;
    idx[i] = hit ? (int)(unsigned)best : -1;
}

size_t nn_bytes(int Nt) {
    return 256 + sizeof(int) * ((size_t)GMAX * GMAX * GMAX + 4) + sizeof(float4) * (size_t)(Nt > 0 ? Nt : 0) + 256;
}

// ---- distance statistics
struct StatThr {
    float v[DPM_STATS_MAX_THRESHOLDS];
};

int stat_blocks(int M) { return M <= SCH ? 1 : (int)(dpm_cdiv(M, SCH) < (unsigned)SBLK ? dpm_cdiv(M, SCH) : SBLK); }

// grid (blocks, C + 1), 256 threads.  Block b of row c walks the contiguous chunk [b * chunk, (b + 1) * chunk) of the points,
// lane t the indices first + t, first + t + 256, ... in ascending order, and keeps fp64 sums of the points of class c (row C:
// of every point).  The lanes of a wave are added by the xor butterfly 32, 16, ... 1, the four waves as (w0 + w1) + (w2 + w3);
// one partial row per block.  Σd adds (double)d, Σd² adds (double)d * (double)d (exact).
__global__ __launch_bounds__(256) void stats_partial_kernel(const float *__restrict__ dist, int M, int chunk,
                                                            const int32_t *__restrict__ surf, const int32_t *__restrict__ class_id,
                                                            int P1, int C, StatThr thr, int T, float max_dist,
                                                            double *__restrict__ partial) {
    constexpr int NC = SCOL + DPM_STATS_MAX_THRESHOLDS;
    const int row = blockIdx.y, t = threadIdx.x, lane = t & 63, w = t >> 6, cols = SCOL + T;
    const long long first = (long long)blockIdx.x * chunk;
    const long long last = first + chunk < (long long)M ? first + chunk : (long long)M;
    double s[NC];
#pragma unroll
    for (int k = 0; k < NC; ++k) s[k] = 0.0;
    for (long long i = first + t; i < last; i += 256) {
        if (row < C) {
            const int sf = surf[i];
            if (sf < 0 || sf >= P1 || class_id[sf] != row) continue;
        }
        const float d = dist[i];
        const bool matched = finite_f(d) && d <= max_dist;
        if (!matched) {
            s[1] += 1.0;
            continue;
        }
        const double dd = (double)d;
        s[0] += 1.0, s[2] += dd, s[3] += dd * dd, s[4] = dd > s[4] ? dd : s[4];
#pragma unroll
        for (int k = 0; k < DPM_STATS_MAX_THRESHOLDS; ++k)
            if (k < T && d <= thr.v[k]) s[SCOL + k] += 1.0;
    }
    __shared__ double sred[4][NC];
#pragma unroll
    for (int k = 0; k < NC; ++k) {
        const double v = k == 4 ? wave_max(s[k]) : wave_sum(s[k]);
        if (lane == 0) sred[w][k] = v;
    }
    __syncthreads();
    if (t < cols) {
        const double a = sred[0][t], b = sred[1][t], c = sred[2][t], d = sred[3][t];
        const double ab = t == 4 ? (a > b ? a : b) : a + b, cd = t == 4 ? (c > d ? c : d) : c + d;
        partial[((size_t)blockIdx.x * (C + 1) + row) * cols + t] = t == 4 ? (ab > cd ? ab : cd) : ab + cd;
    }
}

// one block: entry e of the (C + 1, 5 + T) table = the partials of blocks 0, 1, ... added (column 4: compared) in that order
__global__ __launch_bounds__(256) void stats_final_kernel(const double *__restrict__ partial, int blocks, int entries, int cols,
                                                          double *__restrict__ out) {
    for (int e = threadIdx.x; e < entries; e += 256) {
        const bool is_max = e % cols == 4;
        double v = 0.0;
        for (int b = 0; b < blocks; ++b) {
            const double p = partial[(size_t)b * entries + e];
            v = is_max ? (p > v ? p : v) : v + p;
        }
        out[e] = v;
    }
}

}  // namespace

extern "C" int dpm_scene_distance(const float *points, int M, const float *records, int P, double ground, int has_ground,
                                  double origin_x, double origin_y, double origin_z, float *dist, int32_t *surf,
                                  dpm_stream_t stream) {
    DPM_CHECK_ARG(M >= 0 && P >= 0 && (P == 0 || records) && (M == 0 || points));
    DPM_CHECK_ARG(dist && surf);
    if (M == 0) return DPM_OK;
    hipLaunchKernelGGL(scene_distance_kernel, dim3(dpm_cdiv(M, 256)), dim3(256), 0, (hipStream_t)stream, points, M, records, P,
                       (float)ground, has_ground != 0, origin_x, origin_y, origin_z, dist, surf);
    return dpm_launch_status();
}

extern "C" size_t dpm_cloud_nn_workspace_bytes(int Nq, int Nt) {
    if (Nq < 0 || Nt < 0) return 0;
    return nn_bytes(Nt);
}

extern "C" int dpm_cloud_nn(const float *query, int Nq, const float *target, int Nt, double max_dist, double origin_x,
                            double origin_y, double origin_z, float *dist, int32_t *idx, void *workspace, dpm_stream_t stream) {
    DPM_CHECK_ARG(Nq >= 0 && Nt >= 0 && (Nq == 0 || query) && (Nt == 0 || target));
    DPM_CHECK_ARG(dist && idx && workspace);
    DPM_CHECK_ARG(max_dist > 0.0 && max_dist < 1e18);
    if (Nq == 0) return DPM_OK;
    hipStream_t st = (hipStream_t)stream;
    NnArgs A{};
    A.qry = query, A.tgt = target, A.Nq = Nq, A.Nt = Nt, A.ox = origin_x, A.oy = origin_y, A.oz = origin_z;
    A.ws = (char *)ws_align256((uintptr_t)workspace);
    hipLaunchKernelGGL(nn_setup_kernel, dim3(1), dim3(1024), 0, st, A, (float)max_dist);
    if (Nt > 0) {
        hipLaunchKernelGGL(nn_grid_kernel<false>, dim3(dpm_cdiv(Nt, 256)), dim3(256), 0, st, A);
        hipLaunchKernelGGL(nn_scan_kernel, dim3(1), dim3(1024), 0, st, A);
        hipLaunchKernelGGL(nn_grid_kernel<true>, dim3(dpm_cdiv(Nt, 256)), dim3(256), 0, st, A);
    }
    hipLaunchKernelGGL(nn_search_kernel, dim3(dpm_cdiv(Nq, 64)), dim3(256), 0, st, A, (float)(max_dist * max_dist), dist, idx);
    return dpm_launch_status();
}

// the blocks' partials: one row of SCOL + T columns per block and class (and one for all classes)
static double *stats_layout(WsCursor &c, int M, int C, int T) { return c.take<double>((size_t)stat_blocks(M) * (C + 1) * (SCOL + T)); }

extern "C" size_t dpm_distance_stats_workspace_bytes(int M, int C, int T) {
    if (M < 0 || C < 0 || C > DPM_STATS_MAX_CLASSES || T < 0 || T > DPM_STATS_MAX_THRESHOLDS) return 0;
    WsCursor c(nullptr);
    stats_layout(c, M, C, T);
    return c.bytes();
}

extern "C" int dpm_distance_stats(const float *dist, int M, const int32_t *surf, const int32_t *class_id, int n_surf, int C,
                                  const float *thresholds, int T, double max_dist, double *out, void *workspace,
                                  dpm_stream_t stream) {
    DPM_CHECK_ARG(M >= 0 && (M == 0 || dist) && out && workspace);
    DPM_CHECK_ARG(T >= 0 && T <= DPM_STATS_MAX_THRESHOLDS && (T == 0 || thresholds));
    DPM_CHECK_ARG(C >= 0 && C <= DPM_STATS_MAX_CLASSES && n_surf >= 0 && (C == 0 || (surf && class_id && n_surf >= 1)));
    DPM_CHECK_ARG(max_dist > 0.0);
    StatThr thr{};
    for (int k = 0; k < T; ++k) thr.v[k] = thresholds[k];
    hipStream_t st = (hipStream_t)stream;
    WsCursor c(workspace);
    double *partial = stats_layout(c, M, C, T);
    const int blocks = stat_blocks(M), chunk = M == 0 ? 1 : (int)dpm_cdiv(M, blocks), cols = SCOL + T;
    hipLaunchKernelGGL(stats_partial_kernel, dim3(blocks, C + 1), dim3(256), 0, st, dist, M, chunk, surf, class_id, n_surf, C, thr,
                       T, (float)max_dist, partial);
    hipLaunchKernelGGL(stats_final_kernel, dim3(1), dim3(256), 0, st, partial, blocks, (C + 1) * cols, cols, out);
    return dpm_launch_status();
}
