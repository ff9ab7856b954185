// Prefix sums, totals and bounds over the threads of a workgroup: what every ordered compaction (count / scan / write), every
// counting sort and every grid header of csrc/ is built from.  Integer sums, minima and maxima only, so the result never
// depends on the order the hardware combines in.
#pragma once
#include "dpm_common.h"

// inclusive prefix sum of v (int or unsigned) over the lanes of the calling wave
template <typename T>
__device__ __forceinline__ T wave_scan_inclusive(T v) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const T o = __shfl_up(v, off, 64);
        if (lane >= off) v += o;
    }
    return v;
}

// base + the sum of v over the threads before the caller (exclusive), across the blockDim.x / 64 waves of the workgroup.
// wsum: LDS, one entry per wave.  CONTAINS A __syncthreads(): every thread of the workgroup calls it, and a second call on
// the same wsum needs a barrier of the caller's in between.  Afterwards wsum[k] is the total of wave k.
template <typename T>
__device__ __forceinline__ T block_scan_exclusive(T v, T *wsum, T base = 0) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const T inc = wave_scan_inclusive(v);
    if (lane == 63) wsum[w] = inc;
    __syncthreads();
    T run = base + inc - v;
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

// the sum of v over a workgroup of NW waves, in every thread.  s: LDS, NW entries.  CONTAINS A __syncthreads(), like the scan.
template <int NW>
__device__ __forceinline__ int block_total(int v, int *s) {
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = v;
    __syncthreads();
    int total = s[0];
#pragma unroll
    for (int k = 1; k < NW; ++k) total += s[k];
    return total;
}

// xy bounds over a workgroup of NW waves, in two halves with the CALLER'S __syncthreads() between them, so that other LDS
// work of the caller's (a histogram to clear) goes under the same barrier.  red: LDS, rows 0 .. 3 of NW entries.
// box_put: every thread; each wave's bounds into red, and into the arguments of all its lanes.
// box_get: after the barrier, in the threads that need the result: folds the waves from `from` on into the arguments
// (thread 0 alone may leave out its own wave: from = 1).
template <int NW>
__device__ __forceinline__ void box_put(float &lox, float &loy, float &hix, float &hiy, float (*red)[NW]) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {   // the four butterflies step by step together: four shuffles in flight
        lox = fminf(lox, __shfl_xor(lox, off, 64)), loy = fminf(loy, __shfl_xor(loy, off, 64));
        hix = fmaxf(hix, __shfl_xor(hix, off, 64)), hiy = fmaxf(hiy, __shfl_xor(hiy, off, 64));
    }
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) red[0][w] = lox, red[1][w] = loy, red[2][w] = hix, red[3][w] = hiy;
}
template <int NW>
__device__ __forceinline__ void box_get(float &lox, float &loy, float &hix, float &hiy, const float (*red)[NW], int from = 0) {
    for (int k = from; k < NW; ++k) {
        lox = fminf(lox, red[0][k]), loy = fminf(loy, red[1][k]);
        hix = fmaxf(hix, red[2][k]), hiy = fmaxf(hiy, red[3][k]);
    }
}
