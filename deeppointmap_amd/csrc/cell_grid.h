// The counting-sorted uniform grid of the nearest-neighbour searches (infomat.hip, icp.hip, map_eval.hip): cell c holds
// sorted[cells[c] .. cells[c + 1]), a sorted entry is (x, y, z, original index as bits), and a query's winner is the smallest
// (distance bits, original index) key, which does not depend on the order of the points inside a cell.
#pragma once
#include "dpm_common.h"

__device__ __forceinline__ int cell_coord(float v, float lo, float inv_cs, int g) {
    return min(max((int)floorf((v - lo) * inv_cs), 0), g - 1);
}

// Grid (nblk, n_pairs) -> (block within the pair, pair) such that ALL blocks of one pair run on the SAME XCD.
// Workgroups are dealt round-robin to the 8 XCDs by linear id and every XCD has a private 4 MB L2; with the
// plain mapping each L2 sees the grids of all pairs at once (64 x 1 MB: every candidate load misses to the
// fabric -- 4.8 GB per launch measured), with this one it holds the one or two pairs it is working on.
// Which workgroup computes a (pair, block) partial changes nothing about the partial.
__device__ __forceinline__ void pair_block(int &blk, int &pair) {
    const int nblk = gridDim.x, npair = gridDim.y;
    if (npair % 8 == 0) {
        const unsigned L = blockIdx.y * nblk + blockIdx.x;
        const unsigned xcd = L & 7, slot = L >> 3;
        pair = (int)((slot / nblk) * 8 + xcd), blk = (int)(slot % nblk);
    } else {
        pair = blockIdx.y, blk = blockIdx.x;
    }
}

// One point of the counting sort.  PLACE = false: points per cell into cells[c + 1]; PLACE = true (after the exclusive scan of
// cells[1 ..], when cells[c + 1] is the start of cell c): the point to its cell's next free slot, which leaves cells[c + 1] at
// the cell's end = the start of cell c + 1.  A slot outside [0, cap) -- counters that are not this pass's -- is not written.
template <bool PLACE>
__device__ __forceinline__ void grid_count_or_place(int *cells, float4 *sorted, int cap, int c, float x, float y, float z, int i) {
    const int pos = atomicAdd(cells + 1 + c, 1);
    if (PLACE && pos >= 0 && pos < cap) sorted[pos] = make_float4(x, y, z, __int_as_float(i));
}

// (distance bits, original index): for distances >= 0 the unsigned order of the key is the order of (distance, index)
__device__ __forceinline__ unsigned long long nn_key(float d2, float idx_bits) {
    return ((unsigned long long)__float_as_uint(d2) << 32) | (unsigned)__float_as_int(idx_bits);
}

// lane ql of a quad takes candidates lo + ql, lo + ql + 4, ... of sorted[lo .. hi); d2 = (dx*dx + dy*dy) + dz*dz
__device__ __forceinline__ void quad_scan_range(const float4 *sorted, int lo, int hi, int ql, float qx, float qy, float qz,
                                                unsigned long long &best) {
    for (int p = lo + ql; p < hi; p += 4) {
        const float4 t = sorted[p];
        const float dx = qx - t.x, dy = qy - t.y, dz = qz - t.z;
        const unsigned long long key = nn_key((dx * dx + dy * dy) + dz * dz, t.w);
        best = key < best ? key : best;
    }
}

// the smallest key of the quad's four lanes, in all four
__device__ __forceinline__ unsigned long long quad_min_key(unsigned long long best) {
#pragma unroll
    for (int off = 1; off <= 2; off <<= 1) {
        const unsigned long long o = (unsigned long long)__shfl_xor((long long)best, off, 64);
        best = o < best ? o : best;
    }
    return best;
}
