// Scan Context (Kim & Kim, IROS 2018) place descriptors and the exhaustive search over a database of them (DESIGN §7k;
// deeppointmap_amd/loop_closure.py is the caller).  No counterpart in the reference, which recognises places with its learned
// loop head only: pinned to this project's own numpy restatement (tests/scan_context_restated.py) and to constructed cases.
//
// BUILD (three launches: clear, bin, finish; no host synchronisation, capturable).  A descriptor is a polar grid of rings x
// sectors cells around the sensor; a cell holds the greatest height h = z + z_offset > 0 of its points.  No transcendental
// runs on the device: the host passes the squared ring edges and (cos, sin) of the sector boundaries as fp32 tables, and a
// point's ring and sector are COUNTS of the table entries it has passed, so rounding can never leave a point without a cell
// or put it in two.  h is non-negative, so an integer atomicMax on its bits orders like the float: no floating-point atomic,
// the same bytes whatever the arrival order.  The finish pass normalises every column (sequential fp32, rings ascending) and
// writes the 64-bit occupancy mask.
//
// SEARCH (two launches).  All sectors shifted cosine sums of a pair are the wrapped diagonals of the Gram matrix Aq^T Ac of
// the two normalised descriptors: one 64 x 64 x rings product on v_mfma_f32_32x32x2_f32 with operands padded with zeros (a
// k-ordered fp32 fma chain per element, rings ascending: a fixed order).  One wave owns one pair at a time: the query's
// operand stays in registers, the candidate's is read from global memory in the operand layout (lane = column, coalesced),
// the next pair's while this pair's diagonals are added; the Gram tile goes to the wave's own LDS image (wave-private, so a
// wavefront-scope fence orders it, not a workgroup barrier) and lane s adds diagonal s with j ascending.  The pair's result is the
// smallest key (bits of d, s) of a wave reduction; the wave keeps the K smallest keys (bits of d, row) it has seen, one per
// lane; the block's four lists are merged by rank and written as ONE partial list per block, and a second launch (one wave a
// query) selects the K smallest of a query's partial lists.  Keys of real candidates are distinct (the row is part of the
// key), so selection is exact and the bytes do not depend on how rows were dealt to blocks.  Nothing of size (Q, D) or
// (Q, D, sectors) is ever stored.
//
// LDS image of a wave: 64 rows of SC_LD = 72 floats.  The accumulator registers of a 32x32 tile hold (row 8g + 4h + i,
// column lane & 31) for lane half h: with rows 72 floats apart the two halves of a store land 4 * 72 = 288 = 32 (mod 64) banks
// apart and a store is conflict free; a diagonal read takes at most `sectors` <= 64 consecutive floats of one row.
#include "dpm_common.h"
#include "workspace.h"

#include <cmath>

namespace {

constexpr int SC_MAX_RINGS = 32, SC_MAX_SECTORS = 64, SC_MAX_K = 8;
constexpr int SC_LD = 72;                  // floats between rows of a wave's Gram image
constexpr int SC_WAVES = 4;                // waves (= pairs in flight) a search block
constexpr unsigned long long SC_PAD = ~0ull;   // key of "no candidate": above every real key (bits of d <= bits of 1.0f)

struct ScTables {
    float ring_e2[SC_MAX_RINGS];           // e_1 .. e_rings
    float sec_c[SC_MAX_SECTORS / 2], sec_s[SC_MAX_SECTORS / 2];   // (cos, sin) of 2 pi m / sectors, m = 1 .. sectors/2 - 1 at [m - 1]
    float min_r2, z_offset;
};

// one lane per point.  Frame f reads point i's coordinate c at xyz[f * fstride + i * pstride + c * cstride].
// A sweep's rows come beam by beam and column by column, so the rows of a block fall into a handful of cells, and the whole
// descriptor is 4.8 KB: atomics on it from every block would queue on one or two L2 channels.  Each block therefore takes
// the maxima in an LDS copy of the grid first and sends only its non-zero cells on -- and of those only the ones a plain
// read does not already show beaten (a cell only grows, so such a read can be stale but never wrong).
__global__ __launch_bounds__(256) void sc_bin_kernel(const float *__restrict__ xyz, const int32_t *__restrict__ counts, int cap,
                                                     long long fstride, int pstride, int cstride, int rings, int sectors,
                                                     unsigned *__restrict__ raw, const ScTables t) {
    __shared__ unsigned cells[SC_MAX_RINGS * SC_MAX_SECTORS];
    const int f = blockIdx.y, cells_n = rings * sectors;
    const int i = blockIdx.x * 256 + threadIdx.x;
    const int n = max(0, min(counts[f], cap));
    if (blockIdx.x * 256 >= n) return;   // block-uniform
    for (int c = threadIdx.x; c < cells_n; c += 256) cells[c] = 0u;
    __syncthreads();
    if (i < n) {
        const float *p = xyz + f * fstride + (long long)i * pstride;
        float x = p[0], y = p[cstride], z = p[2 * (long long)cstride];
        const float r2 = x * x + y * y, h = z + t.z_offset;
        if (isfinite(x) && isfinite(y) && isfinite(z) && r2 != 0.f && r2 >= t.min_r2 && r2 < t.ring_e2[rings - 1] && h > 0.f) {
            int ring = 0;
            for (int m = 0; m < rings - 1; ++m) ring += r2 >= t.ring_e2[m] ? 1 : 0;
            const int half = (y > 0.f || (y == 0.f && x > 0.f)) ? 0 : 1;
            if (half) x = -x, y = -y;
            int k = 0;
            for (int m = 0; m < sectors / 2 - 1; ++m) k += t.sec_c[m] * y - t.sec_s[m] * x >= 0.f ? 1 : 0;
            atomicMax(&cells[ring * sectors + half * (sectors / 2) + k], __float_as_uint(h));
        }
    }
    __syncthreads();
    unsigned *out = raw + (size_t)f * cells_n;
    for (int c = threadIdx.x; c < cells_n; c += 256) {
        const unsigned v = cells[c];
        if (v != 0u && __builtin_nontemporal_load(out + c) < v) atomicMax(out + c, v);
    }
}

// one wave per frame, lane j = column j
__global__ __launch_bounds__(64) void sc_finish_kernel(const float *__restrict__ raw, float *__restrict__ norm,
                                                       unsigned long long *__restrict__ mask, int rings, int sectors) {
    const int f = blockIdx.x, j = threadIdx.x;
    const float *r = raw + (size_t)f * rings * sectors;
    float *o = norm + (size_t)f * rings * sectors;
    float n2 = 0.f;
    if (j < sectors)
        for (int m = 0; m < rings; ++m) n2 = n2 + r[m * sectors + j] * r[m * sectors + j];
    const float n = sqrtf(n2);
    if (j < sectors)
        for (int m = 0; m < rings; ++m) o[m * sectors + j] = n > 0.f ? r[m * sectors + j] / n : 0.f;
    const unsigned long long b = __ballot(j < sectors && n > 0.f);
    if (j == 0) mask[f] = b;
}

using f32x16 = __attribute__((ext_vector_type(16))) float;

__device__ __forceinline__ unsigned long long shfl_up_u64(unsigned long long v) {
    const unsigned lo = __shfl_up((unsigned)v, 1, 64), hi = __shfl_up((unsigned)(v >> 32), 1, 64);
    return ((unsigned long long)hi << 32) | lo;
}

// lane i < K holds the wave's i-th smallest key and its shift; `key` and `shift` are wave-uniform
__device__ __forceinline__ void sc_insert(unsigned long long &lkey, int &lshift, unsigned long long key, int shift, int K) {
    const int lane = lane_id();
    const int pos = __popcll(__ballot(lane < K && lkey < key));   // keys are distinct: the list is strictly ascending
    if (pos >= K) return;
    const unsigned long long up = shfl_up_u64(lkey);
    const int ups = __shfl_up(lshift, 1, 64);
    if (lane == pos) lkey = key, lshift = shift;
    else if (lane > pos) lkey = up, lshift = ups;
}

// a wave's own LDS image needs no s_barrier between its stores and its loads: the LDS serves one wave's operations in
// order.  What is needed is that the compiler keeps the order and waits for the stores: a wavefront-scope fence.
__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// a candidate's operand: B[k = ring][j = column]; lane holds (ring 2 step + (lane >> 5), column 32 t + (lane & 31)), zero
// outside the descriptor.  Branch-free, so that the loads of a pair issue together.
template <int NT, int STEPS>
__device__ __forceinline__ void sc_load_operand(float (&b)[NT][STEPS], const float *__restrict__ d, int rings, int sectors, int col, int kh) {
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int s = 0; s < STEPS; ++s) {
            const int r = 2 * s + kh, j = 32 * t + col;
            const bool in = r < rings && j < sectors;
            const float v = d[in ? r * sectors + j : 0];
            b[t][s] = in ? v : 0.f;
        }
}

// grid (blocks of `rpb` database rows, Q).  NT = ceil(sectors / 32): tiles per side of the Gram matrix; STEPS >= ceil(rings / 2):
// k-steps of two rings each (the steps past the descriptor multiply zeros: 8, 12 or 16 are instantiated).
template <int NT, int STEPS>
__global__ __launch_bounds__(64 * SC_WAVES) void sc_search_kernel(const float *__restrict__ qn, const unsigned long long *__restrict__ qm,
                                                                  const float *__restrict__ dn, const unsigned long long *__restrict__ dm,
                                                                  int D, const int32_t *__restrict__ limit, int rings, int sectors,
                                                                  int K, int rpb, unsigned long long *__restrict__ part_key,
                                                                  int32_t *__restrict__ part_shift) {
    __shared__ float gram[SC_WAVES][64 * SC_LD];
    __shared__ unsigned long long mkey[SC_WAVES * SC_MAX_K];
    __shared__ int mshift[SC_WAVES * SC_MAX_K];
    const int q = blockIdx.y, wave = threadIdx.x >> 6, lane = lane_id();
    const int lim = max(0, min(limit[q], D));
    const int row0 = blockIdx.x * rpb, row1 = min(row0 + rpb, lim);
    const int per = rings * sectors;
    const int col = lane & 31, kh = lane >> 5;
    unsigned long long lkey = SC_PAD;
    int lshift = -1;
    if (row0 + wave < row1) {   // wave-uniform; a wave's rows are row0 + wave, + SC_WAVES, ..
        float a[NT][STEPS], b[NT][STEPS];
        sc_load_operand<NT, STEPS>(a, qn + (size_t)q * per, rings, sectors, col, kh);   // the query's: A[i = column][k = ring], the same lane map
        const unsigned long long mq = qm[q];
        const unsigned long long all = sectors == 64 ? ~0ull : (1ull << sectors) - 1ull;
        float *g = gram[wave];
        sc_load_operand<NT, STEPS>(b, dn + (size_t)(row0 + wave) * per, rings, sectors, col, kh);
        for (int c = row0 + wave; c < row1; c += SC_WAVES) {
            unsigned long long mc = dm[c] & all;
            f32x16 acc[NT][NT];
#pragma unroll
            for (int ti = 0; ti < NT; ++ti)
#pragma unroll
                for (int tj = 0; tj < NT; ++tj)
#pragma unroll
                    for (int e = 0; e < 16; ++e) acc[ti][tj][e] = 0.f;
#pragma unroll
            for (int s = 0; s < STEPS; ++s)
#pragma unroll
                for (int ti = 0; ti < NT; ++ti)
#pragma unroll
                    for (int tj = 0; tj < NT; ++tj)
                        acc[ti][tj] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[ti][s], b[tj][s], acc[ti][tj], 0, 0, 0);
            // the next pair's operand is on its way while this pair's diagonals are added (the last pair reloads itself)
            sc_load_operand<NT, STEPS>(b, dn + (size_t)min(c + SC_WAVES, row1 - 1) * per, rings, sectors, col, kh);
#pragma unroll
            for (int ti = 0; ti < NT; ++ti)
#pragma unroll
                for (int tj = 0; tj < NT; ++tj)
#pragma unroll
                    for (int e = 0; e < 16; ++e)
                        g[(32 * ti + (e & 3) + 8 * (e >> 2) + 4 * kh) * SC_LD + 32 * tj + col] = acc[ti][tj][e];
            wave_lds_sync();
            // lane s: S(s) = sum_j G[j][(j + s) % sectors], j ascending
            float S = 0.f;
            if (lane < sectors) {
                int cc = lane;
#pragma unroll 4
                for (int j = 0; j < sectors; ++j) {
                    S = S + g[j * SC_LD + cc];
                    cc = cc + 1 == sectors ? 0 : cc + 1;
                }
            }
            wave_lds_sync();   // the next pair's stores stay behind these loads
            const int sh = lane < sectors ? lane : 0;
            const unsigned long long rot = sh == 0 ? mc : ((mc >> sh) | (mc << (sectors - sh))) & all;   // bit j = mc[(j + s) % sectors]
            const int used = __popcll(mq & rot);
            const float d = used ? fmaxf(1.f - S / (float)used, 0.f) : 1.f;
            unsigned long long key = lane < sectors ? ((unsigned long long)__float_as_uint(d) << 32) | (unsigned)lane : SC_PAD;
            key = wave_min(key);
            sc_insert(lkey, lshift, (key & 0xFFFFFFFF00000000ull) | (unsigned)c, (int)(key & 0xFFFFFFFFu), K);
        }
    }
    // the block's four lists -> one, by rank (real keys are distinct; pads are ranked by their slot)
    if (lane < K) mkey[wave * K + lane] = lkey, mshift[wave * K + lane] = lshift;
    __syncthreads();
    if (wave == 0) {
        const int n = SC_WAVES * K;
        unsigned long long mine = SC_PAD;
        int ms = -1, rank = 0;
        if (lane < n) {
            mine = mkey[lane], ms = mshift[lane];
            for (int o = 0; o < n; ++o) rank += (mkey[o] < mine || (mkey[o] == mine && o < lane)) ? 1 : 0;
            if (rank < K) {
                const size_t at = ((size_t)q * gridDim.x + blockIdx.x) * K + rank;
                part_key[at] = mine, part_shift[at] = ms;
            }
        }
    }
}

// one wave per query: the K smallest keys of its nblk * K partial entries, ascending; K rounds of "smallest key above the last"
__global__ __launch_bounds__(64) void sc_merge_kernel(const unsigned long long *__restrict__ part_key, const int32_t *__restrict__ part_shift,
                                                      int nblk, int K, float *__restrict__ dist, int32_t *__restrict__ row,
                                                      int32_t *__restrict__ shift) {
    const int q = blockIdx.x, lane = threadIdx.x;
    const size_t n = (size_t)nblk * K;
    const unsigned long long *pk = part_key + (size_t)q * n;
    const int32_t *ps = part_shift + (size_t)q * n;
    unsigned long long last = 0;
    bool first = true;
    for (int k = 0; k < K; ++k) {
        unsigned long long best = SC_PAD;
        for (size_t i = lane; i < n; i += 64) {
            const unsigned long long v = pk[i];
            if ((first || v > last) && v < best) best = v;
        }
        best = wave_min(best);
        if (best == SC_PAD) {   // fewer than K candidates: (inf, -1, -1) from here on
            if (lane == 0)
                for (int kk = k; kk < K; ++kk) dist[q * K + kk] = __uint_as_float(0x7F800000u), row[q * K + kk] = -1, shift[q * K + kk] = -1;
            return;
        }
        for (size_t i = lane; i < n; i += 64)
            if (pk[i] == best) dist[q * K + k] = __uint_as_float((unsigned)(best >> 32)), row[q * K + k] = (int)(best & 0xFFFFFFFFu), shift[q * K + k] = ps[i];
        last = best, first = false;
    }
}

int sc_check(int rings, int sectors) {
    return rings >= 1 && rings <= SC_MAX_RINGS && sectors >= 4 && sectors <= SC_MAX_SECTORS && (sectors & 1) == 0;
}

// database rows a search block takes: a power of two in [SC_WAVES, 256], sized so that about a thousand blocks exist
int sc_rows_per_block(int Q, int D) {
    int rpb = SC_WAVES;
    while (rpb < 256 && (long long)Q * dpm_cdiv(D, rpb) > 1024) rpb *= 2;
    return rpb;
}

int sc_build(const float *xyz, const int32_t *counts, int F, int cap, long long fstride, int pstride, int cstride, int rings,
             int sectors, double max_range, double min_range, double z_offset, const float *ring_e2, const float *sector_cs,
             float *raw, float *norm, unsigned long long *mask, hipStream_t stream) {
    DPM_CHECK_ARG(counts && raw && norm && mask && ring_e2 && sector_cs && F >= 1 && cap >= 0 && (cap == 0 || xyz));
    DPM_CHECK_ARG(sc_check(rings, sectors));
    DPM_CHECK_ARG(min_range >= 0.0 && min_range <= max_range && std::isfinite(max_range) && std::isfinite(z_offset));
    ScTables t = {};
    for (int m = 0; m < rings; ++m) t.ring_e2[m] = ring_e2[m];
    for (int m = 0; m < sectors / 2 - 1; ++m) t.sec_c[m] = sector_cs[2 * m], t.sec_s[m] = sector_cs[2 * m + 1];
    t.min_r2 = (float)(min_range * min_range);
    t.z_offset = (float)z_offset;
    const hipError_t e = hipMemsetAsync(raw, 0, sizeof(float) * (size_t)F * rings * sectors, stream);
    if (e != hipSuccess) return (int)e;
    if (cap > 0)
        hipLaunchKernelGGL(sc_bin_kernel, dim3(dpm_cdiv(cap, 256), F), dim3(256), 0, stream, xyz, counts, cap, fstride, pstride,
                           cstride, rings, sectors, (unsigned *)raw, t);
    hipLaunchKernelGGL(sc_finish_kernel, dim3(F), dim3(64), 0, stream, raw, norm, mask, rings, sectors);
    return dpm_launch_status();
}

}  // namespace

extern "C" int dpm_scan_context_build(const float *xyz, const int32_t *count, int cap, int rings, int sectors, double max_range,
                                      double min_range, double z_offset, const float *ring_e2, const float *sector_cs, float *raw,
                                      float *norm, unsigned long long *mask, dpm_stream_t stream) {
    return sc_build(xyz, count, 1, cap, 0, 3, 1, rings, sectors, max_range, min_range, z_offset, ring_e2, sector_cs, raw, norm, mask,
                    (hipStream_t)stream);
}

extern "C" int dpm_scan_context_build_batched(const float *pcd, const int32_t *lengths, int F, int N, int rings, int sectors,
                                              double max_range, double min_range, double z_offset, const float *ring_e2,
                                              const float *sector_cs, float *raw, float *norm, unsigned long long *mask,
                                              dpm_stream_t stream) {
    DPM_CHECK_ARG(F >= 1 && F <= 65535);
    return sc_build(pcd, lengths, F, N, 3ll * N, 1, N, rings, sectors, max_range, min_range, z_offset, ring_e2, sector_cs, raw, norm,
                    mask, (hipStream_t)stream);
}

struct SearchWs {   // the blocks' K best per query: packed (distance, row) keys, then the shifts
    unsigned long long *part_key;
    int32_t *part_shift;
};
// from the caller's pointer on (no base rounding, no allowance)
static SearchWs search_layout(WsCursor &c, int Q, int D, int K) {
    const size_t n = (size_t)Q * dpm_cdiv(D, sc_rows_per_block(Q, D)) * K;
    SearchWs w;
    w.part_key = c.take<unsigned long long>(n);
    w.part_shift = c.take<int32_t>(n);
    return w;
}

extern "C" size_t dpm_scan_context_search_workspace_bytes(int Q, int D, int K) {
    if (Q < 1 || D < 1 || K < 1 || K > SC_MAX_K) return 0;
    WsCursor c(nullptr, false);
    search_layout(c, Q, D, K);
    return c.bytes();
}

extern "C" int dpm_scan_context_search(const float *q_norm, const unsigned long long *q_mask, int Q, const float *db_norm,
                                       const unsigned long long *db_mask, int D, const int32_t *limit, int rings, int sectors,
                                       int K, float *dist, int32_t *row, int32_t *shift, void *workspace, dpm_stream_t stream) {
    DPM_CHECK_ARG(q_norm && q_mask && db_norm && db_mask && limit && dist && row && shift && workspace);
    DPM_CHECK_ARG(Q >= 1 && Q <= 65535 && D >= 1 && K >= 1 && K <= SC_MAX_K && sc_check(rings, sectors));
    const int rpb = sc_rows_per_block(Q, D), nblk = (int)dpm_cdiv(D, rpb);
    WsCursor c(workspace, false);
    const auto [part_key, part_shift] = search_layout(c, Q, D, K);
    const dim3 grid(nblk, Q), block(64 * SC_WAVES);
#define SC_LAUNCH(NT, STEPS)                                                                                                       \
    hipLaunchKernelGGL((sc_search_kernel<NT, STEPS>), grid, block, 0, (hipStream_t)stream, q_norm, q_mask, db_norm, db_mask, D, limit, \
                       rings, sectors, K, rpb, part_key, part_shift)
    if (sectors <= 32) {
        if (rings <= 16) SC_LAUNCH(1, 8);
        else if (rings <= 24) SC_LAUNCH(1, 12);
        else SC_LAUNCH(1, 16);
    } else {
        if (rings <= 16) SC_LAUNCH(2, 8);
        else if (rings <= 24) SC_LAUNCH(2, 12);
        else SC_LAUNCH(2, 16);
    }
#undef SC_LAUNCH
    hipLaunchKernelGGL(sc_merge_kernel, dim3(Q), dim3(64), 0, (hipStream_t)stream, part_key, part_shift, nblk, K, dist, row, shift);
    return dpm_launch_status();
}
