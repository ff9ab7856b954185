// The end-of-run global map (reference ResultLogger.draw_trajectory, system/modules/recoder.py:167-190): every scan's
// cloud moved by its SE3_pred, the union voxel-down-sampled at `vs` (open3d PointCloud::VoxelDownSample).
//
// Semantics, restated from open3d:  min_b = (min over all points) - vs/2 per axis;  voxel index = floor((p - min_b) / vs)
// in fp64 from the fp32 transformed point;  output = mean of each voxel's points.  Output order here is the order of
// first appearance in the concatenation (scan order, then point order) -- open3d's is unordered_map order, unspecified.
//
// Five calls over one workspace (dpm_voxel_map_workspace_bytes(N), N = total points), bounds and insert may be repeated over
// batches of scans so that host-resident clouds can be streamed through a bounded staging buffer:
//   init    clears the header and the hash table;
//   bounds  min / max of the transformed points (fp32 min / max is exact, so atomics on an order-preserving integer image
//           give the same bits in any order) and the number of non-finite coordinates;  the caller reads the header back,
//           refuses non-finite input and extents the key packing cannot hold, and computes min_b;
//   insert  transforms again (the same fp32 arithmetic: the same bits), packs the voxel index into a 63-bit key
//           (3 x 21 bits) and accumulates per voxel, in an open-addressing hash table: the point count (u32), the
//           64-bit fixed-point sums of the offsets from the voxel's lower corner (2^-32 m resolution) and the smallest
//           global point index (atomicMin).  Integer atomics are associative: the table does not depend on arrival order.
//   finish  marks every voxel's first point in a bitmask over the N points and prefix-counts it: a voxel's rank in the
//           output is the number of first points before its own, i.e. the order of first appearance;
//   emit    writes centroid (corner + sum / count, in fp64, rounded once to fp32) and count at that rank.
//
// Contention: LiDAR points arrive in scan order, so neighbouring points share voxels.  Each wave walks a contiguous range
// of WAVE_PTS points, 64 at a time; equal keys in consecutive lanes are merged by a segmented scan in registers, and the
// run that reaches lane 63 is carried into the next 64 points instead of being flushed.  Only run tails touch HBM: one
// probe (atomicCAS when the slot is new) + count + three sums + first = 5 atomics (+ the CAS) per run, not per point.
// The header counts runs and CAS attempts, so that callers can report atomics per point.
//
// Fixed-point bound: a voxel's offset sum is < count * (vs + ulp) * 2^32 and count <= N, so N * (vs * 2^32 + 2) < 2^62
// (checked by the caller before the first call) keeps every int64 sum far from wrapping.  Accuracy: each offset is
// rounded to 2^-33 m, so a centroid is within 1.2e-10 m of the fp64 mean before its fp32 rounding.
//
// Memory: header 256 B + per slot 40 B (key 8, sums 24, first 4, count 4) with N + N/4 (+64) slots, + N/4 bytes of
// bitmask / prefix: <= 51 B per input point (+ 8 KB).
#include "block_scan.h"
#include "workspace.h"

namespace {

constexpr int VM_BLOCK = 256;
constexpr int WAVE_PTS = 1024;                 // points per wave (16 iterations of 64)
constexpr unsigned long long EMPTY = ~0ull;    // keys use 63 bits: never equal to EMPTY
constexpr double FIX_SCALE = 4294967296.0;     // 2^32 fixed-point steps per metre
constexpr int CHUNK_WORDS = 1024;              // bitmask words per prefix block (256 threads x 4)

struct Layout {
    long long cap, W, NCH;
    size_t off_keys, off_sums, off_first, off_cnt, off_bits, off_wpre, off_chunks, total;
};

__host__ __device__ inline Layout vm_layout(long long N) {
    Layout L;
    L.cap = ((N + N / 4 + 63) / 64) * 64 + 64;
    L.W = (N + 31) / 32;
    L.NCH = (L.W + CHUNK_WORDS - 1) / CHUNK_WORDS;
    size_t o = 256;
    L.off_keys = o;   o += (size_t)L.cap * 8;
    L.off_sums = o;   o += (size_t)L.cap * 24;
    L.off_first = o;  o += (size_t)L.cap * 4;
    L.off_cnt = o;    o += (size_t)L.cap * 4;
    L.off_bits = o;   o += (size_t)L.W * 4;
    L.off_wpre = o;   o += (size_t)L.W * 4;
    L.off_chunks = o; o += (size_t)(L.NCH + 1) * 4;
    L.total = ws_align256(o);
    return L;
}

// header (unsigned words): [0..2] min, [3..5] max (order-preserving images of fp32), [6] non-finite coordinates,
// [7] keys out of range, [8] M; 64-bit words at byte 64: runs flushed, CAS attempts
struct Header {
    unsigned mn[3], mx[3], nonfinite, badkey, M, pad[7];
    unsigned long long runs, cas;
};

__device__ __forceinline__ unsigned ordered(float f) {
    const unsigned u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__device__ __forceinline__ void xform(const float *__restrict__ P, float x, float y, float z, float w[3]) {
    // as dpm_map_tile: k-ordered fma chain, then the translation
#pragma unroll
    for (int a = 0; a < 3; ++a) w[a] = fmaf(P[3 * a + 2], z, fmaf(P[3 * a + 1], y, P[3 * a] * x)) + P[9 + a];
}

// scan of global point gi (local to this batch): offsets (n_scans + 1) prefix sums
__device__ __forceinline__ int scan_of(const long long *__restrict__ offsets, int n_scans, long long gi) {
    int lo = 0, hi = n_scans - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (offsets[mid] <= gi) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

__global__ __launch_bounds__(VM_BLOCK) void vm_init_kernel(unsigned char *__restrict__ ws, long long N) {
    const Layout L = vm_layout(N);
    const long long tid = (long long)blockIdx.x * VM_BLOCK + threadIdx.x, stride = (long long)gridDim.x * VM_BLOCK;
    if (tid < 64) {
        unsigned *h = reinterpret_cast<unsigned *>(ws);
        h[tid] = tid < 3 ? 0xFFFFFFFFu : 0u;
    }
    unsigned long long *keys = reinterpret_cast<unsigned long long *>(ws + L.off_keys);
    long long *sums = reinterpret_cast<long long *>(ws + L.off_sums);
    unsigned *first = reinterpret_cast<unsigned *>(ws + L.off_first), *cnt = reinterpret_cast<unsigned *>(ws + L.off_cnt);
    for (long long i = tid; i < L.cap; i += stride) {
        keys[i] = EMPTY;
        sums[i] = 0, sums[L.cap + i] = 0, sums[2 * L.cap + i] = 0;
        first[i] = 0xFFFFFFFFu, cnt[i] = 0u;
    }
    unsigned *bits = reinterpret_cast<unsigned *>(ws + L.off_bits);
    for (long long i = tid; i < L.W; i += stride) bits[i] = 0u;
}

// one wave per WAVE_PTS consecutive points of the batch
__global__ __launch_bounds__(VM_BLOCK) void vm_bounds_kernel(const float *const *__restrict__ clouds,
                                                             const long long *__restrict__ offsets,
                                                             const float *__restrict__ poses, int n_scans,
                                                             unsigned char *__restrict__ ws) {
    const long long n = offsets[n_scans];
    const long long g0 = ((long long)blockIdx.x * (VM_BLOCK / 64) + (threadIdx.x >> 6)) * WAVE_PTS;
    float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
    unsigned bad = 0;
    if (g0 < n) {
        const long long g1 = min(n, g0 + WAVE_PTS);
        int s = scan_of(offsets, n_scans, g0);
        for (long long gi = g0 + lane_id(); gi < g1; gi += 64) {
            while (gi >= offsets[s + 1]) ++s;
            const long long j = gi - offsets[s], Ni = offsets[s + 1] - offsets[s];
            const float *c = clouds[s];
            float w[3];
            xform(poses + (size_t)s * 12, c[j], c[Ni + j], c[2 * Ni + j], w);
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                if (!isfinite(w[a])) {
                    ++bad;
                } else {
                    mn[a] = fminf(mn[a], w[a]);
                    mx[a] = fmaxf(mx[a], w[a]);
                }
            }
        }
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) mn[a] = wave_min(mn[a]), mx[a] = wave_max(mx[a]);
    bad = wave_sum(bad);
    if (lane_id() == 0 && g0 < n) {
        Header *h = reinterpret_cast<Header *>(ws);
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            if (mn[a] <= mx[a]) {   // the wave saw a finite value on this axis
                atomicMin(&h->mn[a], ordered(mn[a]));
                atomicMax(&h->mx[a], ordered(mx[a]));
            }
        }
        if (bad) atomicAdd(&h->nonfinite, bad);
    }
}

struct Run {
    unsigned long long key;
    long long q[3];
    unsigned cnt, first;
};

// one lane adds a run to its voxel's slot.  cap > N >= number of distinct keys: the probe always ends.
__device__ __forceinline__ void flush(const Run &r, const Layout &L, unsigned char *__restrict__ ws, unsigned &cas) {
    unsigned long long *keys = reinterpret_cast<unsigned long long *>(ws + L.off_keys);
    unsigned long long *sums = reinterpret_cast<unsigned long long *>(ws + L.off_sums);
    unsigned *first = reinterpret_cast<unsigned *>(ws + L.off_first), *cnt = reinterpret_cast<unsigned *>(ws + L.off_cnt);
    long long slot = (long long)(mix64(r.key) % (unsigned long long)L.cap);
    while (true) {
        const unsigned long long k = __hip_atomic_load(&keys[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (k == r.key) break;
        if (k == EMPTY) {
            ++cas;
            const unsigned long long prev = atomicCAS(&keys[slot], EMPTY, r.key);
            if (prev == EMPTY || prev == r.key) break;
        }
        slot = slot + 1 == L.cap ? 0 : slot + 1;
    }
    atomicAdd(&cnt[slot], r.cnt);
#pragma unroll
    for (int a = 0; a < 3; ++a) atomicAdd(&sums[a * L.cap + slot], (unsigned long long)r.q[a]);
    atomicMin(&first[slot], r.first);
}

__device__ __forceinline__ unsigned long long shfl_up_u64(unsigned long long v, int d) {
    return (unsigned long long)__shfl_up((long long)v, d, 64);
}

__global__ __launch_bounds__(VM_BLOCK) void vm_insert_kernel(const float *const *__restrict__ clouds,
                                                             const long long *__restrict__ offsets,
                                                             const float *__restrict__ poses, int n_scans,
                                                             long long base, long long N, double mbx, double mby,
                                                             double mbz, double vs, unsigned char *__restrict__ ws) {
    const Layout L = vm_layout(N);
    const long long n = offsets[n_scans];
    const long long g0 = ((long long)blockIdx.x * (VM_BLOCK / 64) + (threadIdx.x >> 6)) * WAVE_PTS;
    if (g0 >= n) return;   // whole waves leave together
    const long long g1 = min(n, g0 + WAVE_PTS);
    const int lane = lane_id();
    const double mb[3] = {mbx, mby, mbz};
    int s = scan_of(offsets, n_scans, g0);
    Run carry;
    carry.key = EMPTY, carry.cnt = 0;
    unsigned runs = 0, cas = 0, badkey = 0;
    for (long long c0 = g0; c0 < g1; c0 += 64) {
        const long long gi = c0 + lane;
        Run r;
        r.key = EMPTY, r.cnt = 0, r.q[0] = r.q[1] = r.q[2] = 0;
        if (gi < g1) {
            while (gi >= offsets[s + 1]) ++s;
            const long long j = gi - offsets[s], Ni = offsets[s + 1] - offsets[s];
            const float *c = clouds[s];
            float w[3];
            xform(poses + (size_t)s * 12, c[j], c[Ni + j], c[2 * Ni + j], w);
            unsigned long long key = 0;
            bool ok = true;
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                const double p = (double)w[a];
                const double fi = floor((p - mb[a]) / vs);
                ok = ok && fi >= 0.0 && fi < 2097152.0;   // also false for NaN
                const long long i = ok ? (long long)fi : 0;
                key |= (unsigned long long)i << (21 * a);
                r.q[a] = __double2ll_rn((p - (mb[a] + (double)i * vs)) * FIX_SCALE);
            }
            if (ok) {
                r.key = key, r.cnt = 1u, r.first = (unsigned)(base + gi);
            } else {
                ++badkey;
                r.q[0] = r.q[1] = r.q[2] = 0;
            }
        }
        // runs of equal keys in consecutive lanes: head flags, the head position by a max-scan, then a segmented sum
        const unsigned long long kup = shfl_up_u64(r.key, 1);
        const bool head = lane == 0 || kup != r.key;
        int start = head ? lane : 0;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) start = max(start, __shfl_up(start, d, 64));
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const long long u0 = __shfl_up(r.q[0], d, 64), u1 = __shfl_up(r.q[1], d, 64), u2 = __shfl_up(r.q[2], d, 64);
            const unsigned uc = __shfl_up(r.cnt, d, 64);
            if (lane - d >= start) r.q[0] += u0, r.q[1] += u1, r.q[2] += u2, r.cnt += uc;
        }
        const bool next_head = __shfl_down((int)head, 1, 64) != 0;
        const bool tail = lane == 63 || next_head;
        if (r.cnt) r.first = (unsigned)(base + gi) - r.cnt + 1u;   // the run's lanes hold consecutive indices
        // the carried run continues into lane 0's run, or is flushed now
        if (carry.key != EMPTY) {
            const unsigned long long k0 = __shfl(r.key, 0, 64);
            if (k0 == carry.key) {
                if (start == 0 && tail) {   // the tail of the first run takes the carry
                    r.q[0] += carry.q[0], r.q[1] += carry.q[1], r.q[2] += carry.q[2];
                    r.cnt += carry.cnt, r.first = carry.first;
                }
            } else if (lane == 0) {
                flush(carry, L, ws, cas);
                ++runs;
            }
        }
        // the run ending at lane 63 becomes the carry (it may continue in the next 64 points); other tails flush
        if (tail && lane != 63 && r.key != EMPTY) {
            flush(r, L, ws, cas);
            ++runs;
        }
        carry.key = (unsigned long long)__shfl((long long)r.key, 63, 64);
        carry.q[0] = __shfl(r.q[0], 63, 64), carry.q[1] = __shfl(r.q[1], 63, 64), carry.q[2] = __shfl(r.q[2], 63, 64);
        carry.cnt = __shfl(r.cnt, 63, 64), carry.first = __shfl(r.first, 63, 64);
    }
    if (carry.key != EMPTY && lane == 0) {
        flush(carry, L, ws, cas);
        ++runs;
    }
    runs = wave_sum(runs), cas = wave_sum(cas), badkey = wave_sum(badkey);
    if (lane == 0) {
        Header *h = reinterpret_cast<Header *>(ws);
        atomicAdd(&h->runs, (unsigned long long)runs);
        atomicAdd(&h->cas, (unsigned long long)cas);
        if (badkey) atomicAdd(&h->badkey, badkey);
    }
}

// every occupied slot sets the bit of its first point
__global__ __launch_bounds__(VM_BLOCK) void vm_mark_kernel(unsigned char *__restrict__ ws, long long N) {
    const Layout L = vm_layout(N);
    const unsigned long long *keys = reinterpret_cast<const unsigned long long *>(ws + L.off_keys);
    const unsigned *first = reinterpret_cast<const unsigned *>(ws + L.off_first);
    unsigned *bits = reinterpret_cast<unsigned *>(ws + L.off_bits);
    for (long long i = (long long)blockIdx.x * VM_BLOCK + threadIdx.x; i < L.cap; i += (long long)gridDim.x * VM_BLOCK) {
        if (keys[i] != EMPTY) {
            const unsigned f = first[i];
            if ((long long)f < N) atomicOr(&bits[f >> 5], 1u << (f & 31));
        }
    }
}

// exclusive block scan of one value per thread (256 threads); returns the block total through *total
__device__ __forceinline__ unsigned block_excl_scan(unsigned v, unsigned *lds /* 4 */, unsigned *total) {
    const int lane = lane_id(), wave = threadIdx.x >> 6;
    const unsigned x = wave_scan_inclusive(v);
    if (lane == 63) lds[wave] = x;
    __syncthreads();
    unsigned before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < VM_BLOCK / 64; ++w) {
        before += w < wave ? lds[w] : 0u;
        all += lds[w];
    }
    __syncthreads();
    *total = all;
    return before + x - v;
}

// bits set per chunk of CHUNK_WORDS words (scanned by vm_chunk_scan_kernel, spread per word by vm_word_prefix_kernel)
__global__ __launch_bounds__(VM_BLOCK) void vm_chunk_count_kernel(unsigned char *__restrict__ ws, long long N) {
    const Layout L = vm_layout(N);
    const unsigned *bits = reinterpret_cast<const unsigned *>(ws + L.off_bits);
    unsigned *chunks = reinterpret_cast<unsigned *>(ws + L.off_chunks);
    __shared__ unsigned lds[VM_BLOCK / 64];
    const long long w0 = (long long)blockIdx.x * CHUNK_WORDS + threadIdx.x * 4;
    unsigned c = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (w0 + k < L.W) c += __popc(bits[w0 + k]);
    unsigned total;
    block_excl_scan(c, lds, &total);
    if (threadIdx.x == 0) chunks[blockIdx.x] = total;
}

// one block: exclusive scan of the chunk counts in place; M = the total
__global__ __launch_bounds__(VM_BLOCK) void vm_chunk_scan_kernel(unsigned char *__restrict__ ws, long long N) {
    const Layout L = vm_layout(N);
    unsigned *chunks = reinterpret_cast<unsigned *>(ws + L.off_chunks);
    __shared__ unsigned lds[VM_BLOCK / 64];
    unsigned running = 0;
    for (long long b = 0; b < L.NCH; b += VM_BLOCK) {
        const long long i = b + threadIdx.x;
        const unsigned v = i < L.NCH ? chunks[i] : 0u;
        unsigned total;
        const unsigned ex = block_excl_scan(v, lds, &total);
        if (i < L.NCH) chunks[i] = running + ex;
        running += total;
    }
    if (threadIdx.x == 0) reinterpret_cast<Header *>(ws)->M = running;
}

__global__ __launch_bounds__(VM_BLOCK) void vm_word_prefix_kernel(unsigned char *__restrict__ ws, long long N) {
    const Layout L = vm_layout(N);
    const unsigned *bits = reinterpret_cast<const unsigned *>(ws + L.off_bits);
    const unsigned *chunks = reinterpret_cast<const unsigned *>(ws + L.off_chunks);
    unsigned *wpre = reinterpret_cast<unsigned *>(ws + L.off_wpre);
    __shared__ unsigned lds[VM_BLOCK / 64];
    const long long w0 = (long long)blockIdx.x * CHUNK_WORDS + threadIdx.x * 4;
    unsigned c[4], sum = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        c[k] = w0 + k < L.W ? __popc(bits[w0 + k]) : 0u;
        sum += c[k];
    }
    unsigned total;
    unsigned run = chunks[blockIdx.x] + block_excl_scan(sum, lds, &total);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (w0 + k < L.W) wpre[w0 + k] = run;
        run += c[k];
    }
}

__global__ __launch_bounds__(VM_BLOCK) void vm_emit_kernel(const unsigned char *__restrict__ ws, long long N, double mbx,
                                                           double mby, double mbz, double vs, float *__restrict__ out,
                                                           int32_t *__restrict__ counts, int M) {
    const Layout L = vm_layout(N);
    const unsigned long long *keys = reinterpret_cast<const unsigned long long *>(ws + L.off_keys);
    const long long *sums = reinterpret_cast<const long long *>(ws + L.off_sums);
    const unsigned *first = reinterpret_cast<const unsigned *>(ws + L.off_first);
    const unsigned *cnt = reinterpret_cast<const unsigned *>(ws + L.off_cnt);
    const unsigned *bits = reinterpret_cast<const unsigned *>(ws + L.off_bits);
    const unsigned *wpre = reinterpret_cast<const unsigned *>(ws + L.off_wpre);
    const double mb[3] = {mbx, mby, mbz};
    for (long long i = (long long)blockIdx.x * VM_BLOCK + threadIdx.x; i < L.cap; i += (long long)gridDim.x * VM_BLOCK) {
        const unsigned long long key = keys[i];
        if (key == EMPTY) continue;
        const unsigned f = first[i];
        if ((long long)f >= N) continue;
        const unsigned rank = wpre[f >> 5] + __popc(bits[f >> 5] & ((1u << (f & 31)) - 1u));
        if (rank >= (unsigned)M) continue;   // cannot happen when M is the finish() total; keeps the stores in bounds
        const double n = (double)cnt[i];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const double corner = mb[a] + (double)((key >> (21 * a)) & 0x1FFFFFull) * vs;
            out[(size_t)a * M + rank] = (float)(corner + (double)sums[(size_t)a * L.cap + i] / FIX_SCALE / n);
        }
        counts[rank] = (int32_t)cnt[i];
    }
}

inline unsigned grid_for(long long items) {
    const long long b = (items + VM_BLOCK - 1) / VM_BLOCK;
    return (unsigned)(b < 1 ? 1 : b > 8192 ? 8192 : b);
}

}  // namespace

extern "C" size_t dpm_voxel_map_workspace_bytes(long long n_points) {
    if (n_points < 1 || n_points > 0x7FFFFFFFll) return 0;
    return vm_layout(n_points).total;
}

extern "C" int dpm_voxel_map_init(long long n_points, void *workspace, dpm_stream_t stream) {
    DPM_CHECK_ARG(workspace && n_points >= 1 && n_points <= 0x7FFFFFFFll);
    hipLaunchKernelGGL(vm_init_kernel, dim3(grid_for(vm_layout(n_points).cap)), dim3(VM_BLOCK), 0, (hipStream_t)stream,
                       (unsigned char *)workspace, n_points);
    return dpm_launch_status();
}

extern "C" int dpm_voxel_map_bounds(const float *const *clouds, const long long *offsets, const float *poses, int n_scans,
                                    long long n_batch, void *workspace, dpm_stream_t stream) {
    DPM_CHECK_ARG(clouds && offsets && poses && workspace && n_scans >= 1 && n_batch >= 0);
    if (n_batch == 0) return DPM_OK;
    const long long waves = (n_batch + WAVE_PTS - 1) / WAVE_PTS;
    hipLaunchKernelGGL(vm_bounds_kernel, dim3(dpm_cdiv(waves, VM_BLOCK / 64)), dim3(VM_BLOCK), 0, (hipStream_t)stream,
                       clouds, offsets, poses, n_scans, (unsigned char *)workspace);
    return dpm_launch_status();
}

extern "C" int dpm_voxel_map_insert(const float *const *clouds, const long long *offsets, const float *poses, int n_scans,
                                    long long n_batch, long long base, long long n_points, double min_x, double min_y,
                                    double min_z, double voxel_size, void *workspace, dpm_stream_t stream) {
    DPM_CHECK_ARG(clouds && offsets && poses && workspace && n_scans >= 1 && n_batch >= 0 && base >= 0 &&
                  base + n_batch <= n_points && n_points <= 0x7FFFFFFFll && voxel_size > 0.0);
    if (n_batch == 0) return DPM_OK;
    const long long waves = (n_batch + WAVE_PTS - 1) / WAVE_PTS;
    hipLaunchKernelGGL(vm_insert_kernel, dim3(dpm_cdiv(waves, VM_BLOCK / 64)), dim3(VM_BLOCK), 0, (hipStream_t)stream,
                       clouds, offsets, poses, n_scans, base, n_points, min_x, min_y, min_z, voxel_size,
                       (unsigned char *)workspace);
    return dpm_launch_status();
}

extern "C" int dpm_voxel_map_finish(long long n_points, void *workspace, dpm_stream_t stream) {
    DPM_CHECK_ARG(workspace && n_points >= 1 && n_points <= 0x7FFFFFFFll);
    const Layout L = vm_layout(n_points);
    unsigned char *ws = (unsigned char *)workspace;
    hipLaunchKernelGGL(vm_mark_kernel, dim3(grid_for(L.cap)), dim3(VM_BLOCK), 0, (hipStream_t)stream, ws, n_points);
    hipLaunchKernelGGL(vm_chunk_count_kernel, dim3((unsigned)L.NCH), dim3(VM_BLOCK), 0, (hipStream_t)stream, ws, n_points);
    hipLaunchKernelGGL(vm_chunk_scan_kernel, dim3(1), dim3(VM_BLOCK), 0, (hipStream_t)stream, ws, n_points);
    hipLaunchKernelGGL(vm_word_prefix_kernel, dim3((unsigned)L.NCH), dim3(VM_BLOCK), 0, (hipStream_t)stream, ws, n_points);
    return dpm_launch_status();
}

extern "C" int dpm_voxel_map_emit(const void *workspace, long long n_points, double min_x, double min_y, double min_z,
                                  double voxel_size, float *centroids, int32_t *counts, int M, dpm_stream_t stream) {
    DPM_CHECK_ARG(workspace && centroids && counts && n_points >= 1 && n_points <= 0x7FFFFFFFll && M >= 1 &&
                  M <= n_points && voxel_size > 0.0);
    hipLaunchKernelGGL(vm_emit_kernel, dim3(grid_for(vm_layout(n_points).cap)), dim3(VM_BLOCK), 0, (hipStream_t)stream,
                       (const unsigned char *)workspace, n_points, min_x, min_y, min_z, voxel_size, centroids, counts, M);
    return dpm_launch_status();
}
