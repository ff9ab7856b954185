// Batched frame ingest: the device side of "F scan files arrive" (reference dataloader/heads/bin.py:16-17,
// dataloader/transforms.py PointCloud.__init__).  The loader packs the raw records of a whole batch into ONE pinned staging
// block; dpm_ingest_frames issues ONE asynchronous copy of that block and THREE launches, whatever F is, and leaves F frames
// of common capacity in the layout of augment.hip: xyz (F,cap,3), idx (F,cap), count (F,).
//
// The staging block, as 32-bit words:
//   header  F x 4 int64  = (offset of the frame's first record in floats from the start of the block, rows, stride in floats,
//                           drop_nan)
//   records frame after frame, `rows` records of `stride` floats each; the first three floats of a record are x, y, z.
// drop_nan = 1 drops a record when one of its first three floats is NaN (bin.py:16-17: the intensity column of a .bin record is
// not looked at); drop_nan = 0 keeps every record.
//
// The kept records' x, y, z are moved AS BITS (32-bit integer loads and stores, the NaN test is a compare on the bits): NaN
// payloads, -0.0 and denormals arrive unchanged.  The compaction is the stable count / scan / write split of augment.hip with
// the frame as the grid's second dimension; the write pass also zeroes the rows at and past the count and writes idx[j] = j,
// so each frame equals PointCloud(filtered array, capacity=cap) byte for byte.  No atomics at all: two runs give identical
// bytes.  Every header field is checked on the host BEFORE anything is queued (a row count above the capacity is DPM_EINVAL),
// and the kernels clamp what they read from the device copy of the header all the same.
#include "block_scan.h"

namespace {

constexpr int CH = 4096;   // records per compaction block (ops.INGEST_CHUNK; the entry point refuses any other `chunk`)

struct Frame {
    const uint32_t *rec;
    int rows, stride, drop;
};

__device__ __forceinline__ Frame frame_of(const long long *__restrict__ hdr, const uint32_t *__restrict__ block,
                                          long long block_words, int f, int cap) {
    const long long off = hdr[4 * f], rows = hdr[4 * f + 1], stride = hdr[4 * f + 2];
    Frame fr;
    const bool ok = off >= 0 && rows >= 0 && rows <= cap && stride >= 3 && off + rows * stride <= block_words;
    fr.rec = block + (ok ? off : 0);
    fr.rows = ok ? (int)rows : 0;
    fr.stride = ok ? (int)stride : 3;
    fr.drop = hdr[4 * f + 3] != 0;
    return fr;
}

__device__ __forceinline__ bool nan_bits(uint32_t u) { return (u & 0x7fffffffu) > 0x7f800000u; }

__device__ __forceinline__ bool keeps(const Frame &fr, int r) {
    if (!fr.drop) return true;
    const uint32_t *p = fr.rec + (size_t)r * fr.stride;
    return !(nan_bits(p[0]) || nan_bits(p[1]) || nan_bits(p[2]));
}

// grid (nblk, F): the survivors of every CH-record chunk
__global__ __launch_bounds__(256) void ingest_count_kernel(const long long *__restrict__ hdr, const uint32_t *__restrict__ block,
                                                           long long block_words, int cap, int nblk, int *__restrict__ bcount) {
    __shared__ int s[4];
    const int f = blockIdx.y;
    const Frame fr = frame_of(hdr, block, block_words, f, cap);
    const long long c0 = (long long)blockIdx.x * CH;
    int cnt = 0;
    for (int k = threadIdx.x; k < CH; k += 256) {
        const long long c = c0 + k;
        if (c < fr.rows && keeps(fr, (int)c)) ++cnt;
    }
    const int total = block_total<4>(cnt, s);
    if (threadIdx.x == 0) bcount[(size_t)f * nblk + blockIdx.x] = total;
}

// grid (F), one wave: exclusive scan of a frame's chunk counts in place, the total is the frame's count
__global__ __launch_bounds__(64) void ingest_scan_kernel(int nblk, int *__restrict__ bcount, int32_t *__restrict__ count) {
    int *bc = bcount + (size_t)blockIdx.x * nblk;
    const int lane = threadIdx.x;
    int carry = 0;
    for (int b0 = 0; b0 < nblk; b0 += 64) {
        const int b = b0 + lane;
        const int v = b < nblk ? bc[b] : 0;
        const int inc = wave_scan_inclusive(v);
        if (b < nblk) bc[b] = carry + inc - v;
        carry += __shfl(inc, 63, 64);
    }
    if (lane == 0) count[blockIdx.x] = carry;
}

// grid (nblk, F): block b writes the survivors of chunk b at its offset, then idx[j] = j and the zero rows at and past the
// count for the OUTPUT rows j of [b * CH, (b + 1) * CH).  Survivors land below the count, the fill at and above it: the two
// never touch the same row.
__global__ __launch_bounds__(256) void ingest_write_kernel(const long long *__restrict__ hdr, const uint32_t *__restrict__ block,
                                                           long long block_words, int cap, int nblk,
                                                           const int *__restrict__ boff, const int32_t *__restrict__ count,
                                                           uint32_t *__restrict__ xyz, int32_t *__restrict__ idx) {
    __shared__ int s_w[4];
    const int f = blockIdx.y;
    const Frame fr = frame_of(hdr, block, block_words, f, cap);
    uint32_t *ox = xyz + 3 * (size_t)f * cap;
    int32_t *oi = idx + (size_t)f * cap;
    const long long c0 = (long long)blockIdx.x * CH;
    // thread t owns 16 CONSECUTIVE records so that the block-level order equals the input order
    const int t = threadIdx.x;
    bool keep[CH / 256];
    int cnt = 0;
#pragma unroll
    for (int k = 0; k < CH / 256; ++k) {
        const long long c = c0 + (long long)t * (CH / 256) + k;
        keep[k] = c < fr.rows && keeps(fr, (int)c);
        cnt += keep[k];
    }
    int pos = block_scan_exclusive(cnt, s_w, boff[(size_t)f * nblk + blockIdx.x]);
#pragma unroll
    for (int k = 0; k < CH / 256; ++k) {
        if (!keep[k]) continue;
        const uint32_t *p = fr.rec + (size_t)(c0 + (long long)t * (CH / 256) + k) * fr.stride;
        if (pos < cap) ox[3 * (size_t)pos] = p[0], ox[3 * (size_t)pos + 1] = p[1], ox[3 * (size_t)pos + 2] = p[2];
        ++pos;
    }
    const int n = max(0, min(count[f], cap));
    for (int k = t; k < CH; k += 256) {
        const long long j = c0 + k;
        if (j >= cap) break;
        oi[j] = (int32_t)j;
        if (j >= n) ox[3 * (size_t)j] = 0u, ox[3 * (size_t)j + 1] = 0u, ox[3 * (size_t)j + 2] = 0u;
    }
}

}  // namespace

extern "C" int dpm_ingest_frames(const void *staging_host, void *staging_dev, long long staging_bytes, int F, int capacity,
                                 int chunk, float *xyz, int32_t *idx, int32_t *count, void *workspace, dpm_stream_t stream) {
    DPM_CHECK_ARG(staging_host && staging_dev && xyz && idx && count && workspace);
    DPM_CHECK_ARG(chunk == CH && F >= 1 && F <= 65535 && capacity >= 1);
    DPM_CHECK_ARG(staging_bytes >= 32LL * F && staging_bytes % 4 == 0);
    const long long words = staging_bytes / 4;
    const long long *hdr = (const long long *)staging_host;
    for (int f = 0; f < F; ++f) {
        const long long off = hdr[4 * f], rows = hdr[4 * f + 1], stride = hdr[4 * f + 2], drop = hdr[4 * f + 3];
        DPM_CHECK_ARG(rows >= 0 && rows <= capacity);       // the host knows every row count from the file size
        DPM_CHECK_ARG(stride >= 3 && stride <= (1 << 20) && (drop == 0 || drop == 1));
        DPM_CHECK_ARG(off >= 8LL * F && off <= words && rows * stride <= words - off);
    }
    const int nblk = (int)dpm_cdiv(capacity, CH);
    hipStream_t st = (hipStream_t)stream;
    const hipError_t e = hipMemcpyAsync(staging_dev, staging_host, (size_t)staging_bytes, hipMemcpyHostToDevice, st);
    if (e != hipSuccess) return (int)e;
    const long long *dh = (const long long *)staging_dev;
    const uint32_t *db = (const uint32_t *)staging_dev;
    int *bcount = (int *)workspace;
    hipLaunchKernelGGL(ingest_count_kernel, dim3(nblk, F), dim3(256), 0, st, dh, db, words, capacity, nblk, bcount);
    hipLaunchKernelGGL(ingest_scan_kernel, dim3(F), dim3(64), 0, st, nblk, bcount, count);
    hipLaunchKernelGGL(ingest_write_kernel, dim3(nblk, F), dim3(256), 0, st, dh, db, words, capacity, nblk, bcount, count,
                       (uint32_t *)xyz, idx);
    return dpm_launch_status();
}
