// Prefix sums over the threads of a workgroup: what every ordered compaction (count / scan / write) and every counting sort
// of csrc/ is built from.  Integer sums only, so the result never depends on the order the hardware adds in.
#pragma once
#include "dpm_common.h"

// inclusive prefix sum of v over the lanes of the calling wave
__device__ __forceinline__ int wave_scan_inclusive(int v) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int o = __shfl_up(v, off, 64);
        if (lane >= off) v += o;
    }
    return v;
}

// base + the sum of v over the threads before the caller (exclusive), across the blockDim.x / 64 waves of the workgroup.
// wsum: LDS, one entry per wave.  CONTAINS A __syncthreads(): every thread of the workgroup calls it, and a second call on
// the same wsum needs a barrier of the caller's in between.  Afterwards wsum[k] is the total of wave k.
__device__ __forceinline__ int block_scan_exclusive(int v, int *wsum, int base = 0) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int inc = wave_scan_inclusive(v);
    if (lane == 63) wsum[w] = inc;
    __syncthreads();
    int run = base + inc - v;
    for (int k = 0; k < w; ++k) run += wsum[k];
    return run;
}

// exclusive prefix sum of c[0 .. n) in place (global memory) by ONE workgroup: thread t owns [t * per, (t + 1) * per) cut to
// [0, n), so per * blockDim.x >= n.  Returns the sum up to the end of the caller's run: in the last thread, the total.
// Contains the barrier of block_scan_exclusive.
__device__ __forceinline__ int block_scan_runs(int *c, int n, int per, int *wsum) {
    const int a = min((int)threadIdx.x * per, n), b = min(a + per, n);
    int sum = 0;
    for (int k = a; k < b; ++k) sum += c[k];
    int run = block_scan_exclusive(sum, wsum);
    for (int k = a; k < b; ++k) {
        const int v = c[k];
        c[k] = run, run += v;
    }
    return run;
}
