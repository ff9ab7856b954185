// The voxel keys and the open-addressing table shared by csrc/local_map.hip and csrc/tsdf_map.hip: one voxel is one 3 x 21-bit
// key (the coordinate floor(p / v) per axis, biased by 2^20), a table is cap_vox slots (a power of two) of 64-bit keys with
// linear probing from mix64(key) and the empty key ~0.  Both maps cut space with exactly these functions, so a point lies in
// the same voxel of either.
#pragma once
#include "dpm_common.h"

constexpr unsigned long long EMPTY = ~0ull;

// voxel coordinate (biased by 2^20) and sub-cell coordinate of one axis; 0 when the 21 bits cannot hold it (or NaN)
__device__ __forceinline__ int axis_cell(float p, float v, int s, int &vox, int &sub) {
    const float f = __fdiv_rn(p, v), fl = floorf(f);
    if (!(fl >= -1048576.f && fl < 1048576.f)) return 0;
    vox = (int)fl + 1048576;
    sub = min((int)((f - fl) * (float)s), s - 1);
    return 1;
}

__device__ __forceinline__ unsigned long long pack_key(int x, int y, int z) {
    return (unsigned long long)x | ((unsigned long long)y << 21) | ((unsigned long long)z << 42);
}

__device__ __forceinline__ int key_axis(unsigned long long key, int a) { return (int)((key >> (21 * a)) & 0x1FFFFF); }

// the centre of a held voxel, per axis c = ((float)index + 0.5f) * v
__device__ __forceinline__ void voxel_centre(unsigned long long key, float v, float c[3]) {
#pragma unroll
    for (int a = 0; a < 3; ++a) c[a] = ((float)(key_axis(key, a) - 1048576) + 0.5f) * v;
}

// The tile of voxel `key`: the cube of 2^b voxels per axis that share key_axis(key, a) >> b (the BIASED index, so tiles are cut
// at multiples of 2^b voxels from the low end of the 21 bits, and 2^20 is such a multiple for every b <= 20); the host names it
// pack_key(x >> b, y >> b, z >> b).  Its centre, per axis c = ((float)(first index of the tile, unbiased) + 0.5f * (float)2^b) * v,
// every operation rounded once.
__device__ __forceinline__ void tile_centre(unsigned long long key, int b, float v, float c[3]) {
#pragma unroll
    for (int a = 0; a < 3; ++a) c[a] = ((float)(((key_axis(key, a) >> b) << b) - 1048576) + 0.5f * (float)(1 << b)) * v;
}

// a tile is NEAR a pose when its centre lies within sqrt(r2) of the pose's map-frame translation (ox, oy, oz the map's origin):
// csrc/local_map.hip's voxel_within on the tile's centre
__device__ __forceinline__ bool tile_near(unsigned long long key, int b, float v, const double *pose, double ox, double oy, double oz,
                                          float r2) {
    const float tx = (float)(pose[3] - ox), ty = (float)(pose[7] - oy), tz = (float)(pose[11] - oz);
    float c[3];
    tile_centre(key, b, v, c);
    const float dx = c[0] - tx, dy = c[1] - ty, dz = c[2] - tz;
    return (dx * dx + dy * dy) + dz * dz <= r2;
}

// slot of `key` in a table nobody is writing, or -1
__device__ __forceinline__ int find_slot(const unsigned long long *keys, int cap_vox, unsigned long long key) {
    int slot = (int)(mix64(key) & (unsigned long long)(cap_vox - 1));
    for (int probe = 0; probe < cap_vox; ++probe) {
        const unsigned long long k = keys[slot];
        if (k == key) return slot;
        if (k == EMPTY) return -1;
        slot = (slot + 1) & (cap_vox - 1);
    }
    return -1;
}

// slot of `key`, claimed if new, in a table other lanes are claiming in; -1 when no slot is free
__device__ __forceinline__ int claim_slot(unsigned long long *keys, int cap_vox, unsigned long long key) {
    int slot = (int)(mix64(key) & (unsigned long long)(cap_vox - 1));
    for (int probe = 0; probe < cap_vox; ++probe) {
        unsigned long long k = __hip_atomic_load(&keys[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (k == EMPTY) k = atomicCAS(&keys[slot], EMPTY, key);
        if (k == EMPTY || k == key) return slot;
        slot = (slot + 1) & (cap_vox - 1);
    }
    return -1;
}

// ---- what the entry points of both maps refuse, on the host
// a table: the caller's buffer (16-byte aligned) of cap_vox slots, a power of two in [2, 2^24]
inline bool table_ok(const void *map, int cap_vox) {
    return map && ((uintptr_t)map & 15) == 0 && cap_vox >= 2 && cap_vox <= (1 << 24) && (cap_vox & (cap_vox - 1)) == 0;
}

inline bool voxel_ok(double voxel) { return voxel > 0.0 && voxel < 1e18 && (float)voxel > 0.f; }

inline bool origin_ok(const double *origin) {
    if (!origin) return false;
    for (int a = 0; a < 3; ++a)
        if (!(origin[a] > -1e300 && origin[a] < 1e300)) return false;
    return true;
}
