// A truncated signed distance field (TSDF) over hashed voxels, and a surface from it (deeppointmap_amd/tsdf.py is the caller).
// The reference has no counterpart: its map is a cloud of points.  DESIGN §7l is the definition.
//
// Map: one buffer of 256 + 20 cap_vox bytes.  A 256-byte header (word 0: samples that found no slot, word 1: samples outside
// the 21-bit key range, word 2: rows of the plane form without a usable normal), then an open-addressing table of cap_vox slots (csrc/voxel_hash.h: the keys, the probing and the
// cutting of space are csrc/local_map.hip's) as three arrays: key u64, sum int64, count u32.  The map frame and the pose
// handling are the local map's too: a float64 `origin` on the host, a pose of 16 doubles in device memory entering as (float)R
// and (float)(t - origin) (gn_load_pose), a point as gn_xform's fma chain.
//
//   integrate  one lane per row, one launch.  Per row that passes the local map's range gate on the SENSOR-frame point, in fp32,
//              every operation rounded once (the build has -ffp-contract=off; the division is __fdiv_rn, the square root sqrtf,
//              which this build expands to the correctly rounded sequence -- __fsqrt_rn is the bare 1-ulp instruction here):
//                  r = sqrt((x*x + y*y) + z*z),  q = the row in the map frame,  o = the pose's map-frame translation,
//                  u = (q - o) / r per axis.
//              For k = -n .. n ascending (n = ceil(tau / h), formed on the host): t = r + (float)k * h; the sample is skipped
//              unless t > 0; p = o + u * t per axis; the voxel of p per axis by axis_cell (a sample outside the 21 bits adds one
//              to header word 1 and is skipped); a sample whose key equals the key of this ray's previous keyed sample is skipped.
//              With c the voxel's centre and e = q - c:  s = (ux*ex + uy*ey) + uz*ez clamped to [-(float)tau, (float)tau]:
//              positive on the sensor's side of the return.  fixed = (long long)rintf(s * 2^24) (round half to even; |fixed| <=
//              2^30 since tau <= 64).  The slot is found or claimed (atomicCAS on the key), then sum += fixed and count += 1 by
//              integer atomics (equal keys of a wave merged first: integrate_ray).  No free slot: header word 0 counts the sample.
//              Integer atomics only, and integer addition commutes: what a key leads to is the same whatever the order of rows,
//              frames or launches.  Slot positions are not, and nothing reads them.
//   frames     the same rule over a list of stored frames: blockIdx.y the list entry, x over the P columns of a channel-major
//              store (capacity,3,P), as dpm_local_map_insert_frames reads it.  Frame and list are the two sources of
//              csrc/scan_source.h: integrate and carve are one kernel each, ts_integrate_kernel<PLANE, Src>, ts_carve_kernel<Src>.
//   planes     integrate / frames with the distance to the TANGENT PLANE at the return in place of the distance along the ray
//              (wrong by about d tan(incidence) for a centre d beside a slanted ray), weighted by the cosine of the incidence.
//              A normal per row in the SENSOR frame, unit length expected, not renormalised, either sign: (cap,3) beside xyz, or
//              a store (capacity,P,3).  Gate, r, q, o, u, the samples, the voxels, header word 1 and the skip are the rule above.
//              Per row, once: n_m[a] = fma(R[a][2], nz, fma(R[a][1], ny, R[a][0] * nx)) (gn_xform's chain without t);
//              a0 = (n_m.x*u.x + n_m.y*u.y) + n_m.z*u.z; m = a0 >= 0 ? n_m : -n_m (away from the sensor, as u); a = |a0|;
//              wq = (int)rintf(a * 256.f).  The row is USABLE when wq >= 1 and a >= (float)cos_min (a zero or NaN normal fails by
//              comparison); a row that passed the range gate and is not usable adds one to header word 2 and offers nothing.
//              Per kept sample: s = (m.x*ex + m.y*ey) + m.z*ez clamped to [-tau, tau], fixed = rintf(s * 2^24), sum += wq *
//              fixed, count += wq.  D = sum / (count * 2^24) is the weighted mean; a full-weight sample counts 256.  With |n| <=
//              1: wq * |fixed| <= 2^38, and a count wraps after 2^24 full-weight samples of one voxel.
//   carve      lookups only (find_slot; no slot is claimed, the key set stays).  Per row that passes the range gate, for k = 1,
//              2, ... while t = (float)k * h < r - (float)margin: the voxel of o + u * t (outside the 21 bits: skipped silently);
//              skipped when its key equals the key of this ray's previous keyed sample; if the table holds the key: sum += weight
//              * rintf(tau * 2^24), count += weight ("free, at the truncation distance").  weight in [1, 65535] count units;
//              max_range / step <= 65536.  A function of (the map before, the set of frames); meant to run after the
//              integrations, and a later integrate adds to what is there.
//   export     (key, sum, count) of every occupied slot in arrival order + their number; Python sorts.
//   evict      one lane per slot, into a second cleared table: the voxels of tiles NEAR a pose (2^b voxels per axis, the tile's
//              centre within the radius: csrc/voxel_hash.h) are kept, the others listed for the host -- or kept when the list
//              is full.  absorb: one lane per record, sum += s and count += c by integrate's atomics.  Integer addition: a
//              voxel split between table and host adds back to the same bytes ("rolling the map").
//
// Field: D(slot) = (float)((double)sum / ((double)count * 2^24)).  A voxel is QUALIFIED when count >= min_count (>= 1).
//   surface    one lane per slot.  For a qualified voxel k0 and an axis a with k1 = k0 + e_a qualified and (D0 < 0) != (D1 < 0):
//              f = D0 / (D0 - D1), the position is k0's centre with f * v added on axis a.  grad(k)_b from the qualified
//              neighbours of k on axis b: both: D(k + e_b) - D(k - e_b); only +: 2 (D(k + e_b) - D(k)); only -: 2 (D(k) -
//              D(k - e_b)); neither: 0.  The normal is g = grad(k0) + grad(k1), divided per axis by sqrt((gx*gx + gy*gy) + gz*gz)
//              where that is > 0, else (0, 0, 0); it points to free space (D grows towards the sensor).
//   mesh       marching tetrahedra, one lane per slot.  The cell anchored at a voxel centre is meshed only when its 8 corner
//              voxels are qualified.  Corner number m = dx | dy << 1 | dz << 2.  The six tetrahedra of the Kuhn decomposition
//              round the diagonal 0 - 7, one per permutation (a, b, c) of the axes in lexicographic order: corners 0, 1 << a,
//              1 << a | 1 << b, 7.  Every edge of them runs from a corner p to a corner q that contains p's bits, so a vertex is
//              named (key of p, direction): q ^ p = 1, 2, 4 (axes) -> 0, 1, 2; 3, 5, 6 (face diagonals) -> 3, 4, 5; 7 (the body
//              diagonal) -> 6.  The faces of neighbouring cells carry the same diagonals.  A vertex exists where (Dp < 0) !=
//              (Dq < 0): f = Dp / (Dp - Dq), the position is p's centre with f * v added on every axis of q ^ p.  One negative
//              or one non-negative corner gives a triangle, two and two a quadrilateral cut into two triangles; they are wound
//              so that the normal (b - a) x (c - a) points to the positive side.  A corner with D == 0 counts as positive, and
//              the triangles of zero area it makes are kept.
//   indexed    the same mesh with the weld done here: a vertex (key of p, direction) is (slot of p << 3) | direction, a 7-bit mask
//              per slot says which exist, a scan over the masks' popcounts numbers them; faces are index triples, a vertex carries
//              surface's normal of its edge.  Six launches, integer atomics only ("the indexed mesh" below).
//   tiles      surface and the indexed mesh given a sorted list of tile keys emit only what is anchored at a voxel of one of those
//              tiles, and read whatever that needs: single-tile calls partition the result ("Meshing beyond the table").
//   raycast    one lane per ray, grid y the pose, lookups only: the field (below) at t_k = t0 + (float)k * h along o + u * t, the
//              first sign change between two valued samples in a row -> range, the unit gradient in the sensor frame, a flag
//              (MISS 0, HIT 1, BACK 2).  blocks: the set of 8 x 8 x 8 blocks that hold a qualified voxel, one lane per slot;
//              the marcher skips the lookups of a sample whose base voxel lies in a block the set does not hold.
#include "block_scan.h"
#include "gn_one.h"
#include "scan_source.h"
#include "voxel_hash.h"
#include "workspace.h"

namespace {

constexpr int TS_BLOCK = 256;
constexpr float FIX_ONE = 16777216.f;   // 2^24: |s| <= 64 m leaves 2^32 samples of headroom in the int64 sum
constexpr int MAX_STEPS = 4096;         // n = ceil(tau / h) at most

struct TsdfHdr {   // 256 bytes
    unsigned overflow, outside, unusable, pad[61];
};

struct Tsdf {
    unsigned char *base;
    int cap_vox;
    float v;
    double ox, oy, oz;
    __host__ __device__ unsigned long long *keys() const { return (unsigned long long *)(base + 256); }
    __host__ __device__ long long *sum() const { return (long long *)(keys() + cap_vox); }
    __host__ __device__ unsigned *count() const { return (unsigned *)(sum() + cap_vox); }
    __host__ __device__ TsdfHdr *hdr() const { return (TsdfHdr *)base; }
};

struct Rays {
    float lo2, hi2, tau, h;
    int n;
};

__global__ __launch_bounds__(TS_BLOCK) void ts_clear_kernel(Tsdf M) {
    const size_t tid = (size_t)blockIdx.x * TS_BLOCK + threadIdx.x, stride = (size_t)gridDim.x * TS_BLOCK;
    if (tid < 64) ((unsigned *)M.base)[tid] = 0u;
    for (size_t i = tid; i < (size_t)M.cap_vox; i += stride) M.keys()[i] = EMPTY, M.sum()[i] = 0, M.count()[i] = 0u;
}

// One return (x, y, z) in the sensor frame under pose P: the samples of its ray.  Neighbouring rows of a sweep are neighbouring
// columns of one beam and fall into the same voxel at the same k, so equal keys are merged inside a wave before the atomics:
// every lane of the wave walks the samples together (row = false: a lane without a return), runs of neighbouring lanes with one
// key are summed by a segmented suffix sum over (count << 40) + fixed (|fixed| <= 2^30, 64 lanes), and the first lane of a run
// adds the run's sum and count.  The same integers reach the table as with one pair of atomics a sample, which timed 2.4 times
// slower on an HDL64E frame (profiles/tsdf_bench.md).  The callers keep the wave together: no lane returns before this.
// PLANE: the distance to the tangent plane at the return instead of the distance along the ray.  (nx, ny, nz) is the return's
// normal in the sensor frame; the row gate, the weight wq and the direction m are formed once a row, before the samples.  A run
// is summed in two words, sum (wq * fixed, at most 64 * 2^38) and count (wq): a packed word would tie the rule to |n| <= 1.
template <bool PLANE>
__device__ __forceinline__ void integrate_ray(const Tsdf &M, const GnPose32 &P, bool row, float x, float y, float z,
                                              const Rays &R, float nx = 0.f, float ny = 0.f, float nz = 0.f,
                                              float cos_min = 0.f) {
    const int lane = threadIdx.x & 63;
    const float r2 = (x * x + y * y) + z * z;
    bool live = row && r2 >= R.lo2 && r2 <= R.hi2;
    const float r = sqrtf(r2);
    float q[3], u[3];
    gn_xform(P, x, y, z, q);
#pragma unroll
    for (int a = 0; a < 3; ++a) u[a] = __fdiv_rn(q[a] - P.t[a], r);
    float m[3] = {0.f, 0.f, 0.f};
    unsigned wq = 0u;
    if constexpr (PLANE) {
        float nm[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) nm[a] = fmaf(P.R[3 * a + 2], nz, fmaf(P.R[3 * a + 1], ny, P.R[3 * a] * nx));
        const float a0 = (nm[0] * u[0] + nm[1] * u[1]) + nm[2] * u[2], aa = fabsf(a0), wf = rintf(aa * 256.f);
        const bool usable = wf >= 1.f && aa >= cos_min;   // a NaN fails both
        if (live && !usable) atomicAdd(&M.hdr()->unusable, 1u);
        live = live && usable;
        wq = live ? (unsigned)wf : 0u;
#pragma unroll
        for (int a = 0; a < 3; ++a) m[a] = a0 >= 0.f ? nm[a] : -nm[a];
    }
    const float *d = PLANE ? m : u;
    unsigned long long prev = EMPTY;
    for (int k = -R.n; k <= R.n; ++k) {
        const float t = r + (float)k * R.h;
        bool valid = live && t > 0.f;
        int vox[3] = {0, 0, 0}, sub;
        int inside = 1;
#pragma unroll
        for (int a = 0; a < 3; ++a) inside &= axis_cell(P.t[a] + u[a] * t, M.v, 1, vox[a], sub);
        if (valid && !inside) atomicAdd(&M.hdr()->outside, 1u);
        valid = valid && inside;
        unsigned long long key = valid ? pack_key(vox[0], vox[1], vox[2]) : EMPTY;
        if (valid && key == prev) valid = false, key = EMPTY;
        else if (valid) prev = key;
        float c[3];
        voxel_centre(key, M.v, c);
        const float ex = q[0] - c[0], ey = q[1] - c[1], ez = q[2] - c[2];
        const float s = fminf(fmaxf((d[0] * ex + d[1] * ey) + d[2] * ez, -R.tau), R.tau);
        long long acc = valid ? (PLANE ? (long long)wq * (long long)rintf(s * FIX_ONE) : (1ll << 40) + (long long)rintf(s * FIX_ONE)) : 0ll;
        const unsigned long long before = __shfl_up(key, 1, 64);
        const bool head = lane == 0 || before != key;
        const unsigned long long heads = __ballot(head || !valid);
        const unsigned long long above = lane == 63 ? 0ull : heads >> (lane + 1);
        const int end = above ? lane + __ffsll((long long)above) : 64;
        if constexpr (PLANE) {
            unsigned cnt = valid ? wq : 0u;
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) {
                const long long other = __shfl_down(acc, off, 64);
                const unsigned others = __shfl_down(cnt, off, 64);
                if (lane + off < end) acc += other, cnt += others;
            }
            if (valid && head) {
                const int slot = claim_slot(M.keys(), M.cap_vox, key);
                if (slot < 0) {
                    atomicAdd(&M.hdr()->overflow, cnt);
                } else {
                    atomicAdd((unsigned long long *)&M.sum()[slot], (unsigned long long)acc);
                    atomicAdd(&M.count()[slot], cnt);
                }
            }
        } else {
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) {
                const long long other = __shfl_down(acc, off, 64);
                if (lane + off < end) acc += other;
            }
            if (valid && head) {
                const long long cnt = (acc + (1ll << 39)) >> 40, total = acc - (cnt << 40);
                const int slot = claim_slot(M.keys(), M.cap_vox, key);
                if (slot < 0) {
                    atomicAdd(&M.hdr()->overflow, (unsigned)cnt);
                } else {
                    atomicAdd((unsigned long long *)&M.sum()[slot], (unsigned long long)total);
                    atomicAdd(&M.count()[slot], (unsigned)cnt);
                }
            }
        }
    }
}

// The rows of a source (csrc/scan_source.h), one lane each.  Two properties every source keeps: a lane without a row (i >= n) does
// NOT leave -- it calls integrate_ray with row = false, because the wave walks the samples together for the segmented sum -- and
// only the WHOLE BLOCK may leave, on a list entry outside the store.  PLANE: normals is the side array beside the source, (cap,3)
// beside xyz or a store (capacity,P,3) beside the frame store.
template <bool PLANE, typename Src>
__global__ __launch_bounds__(TS_BLOCK) void ts_integrate_kernel(Tsdf M, Src S, const float *normals, Rays R, float cos_min) {
    SourceRows o;
    if (!S.open(o)) return;
    const int i = blockIdx.x * TS_BLOCK + threadIdx.x;
    const bool row = i < o.n;
    const GnPose32 P = gn_load_pose(o.pose, M.ox, M.oy, M.oz);
    float x = 0.f, y = 0.f, z = 0.f, nx = 0.f, ny = 0.f, nz = 0.f;
    if (row) {
        S.point(o, i, x, y, z);
        if constexpr (PLANE) {
            const float *nr = normals + 3 * S.side(o, i);
            nx = nr[0], ny = nr[1], nz = nr[2];
        }
    }
    integrate_ray<PLANE>(M, P, row, x, y, z, R, nx, ny, nz, cos_min);
}

// ---------------------------------------------------------------------------------------------------------- free-space carving
// One return: every voxel its ray crosses before `margin` short of the return, IF THE TABLE HOLDS IT, is told "free, at the
// truncation distance".  Lookups only (find_slot: nobody writes a key while a carve runs), so the key set stays and what a key
// receives depends on the key set and the frames alone, not on their order.  A lane on its own, leaving when its ray ends: the
// form that merges equal keys of a wave before the lookup, as integrate_ray does, was built and timed 1.14 times slower on an
// HDL64E frame and 1.21 times slower on 50 stored frames (profiles/tsdf_bench.md).  Supposed, not measured: lookups of one key by
// neighbouring lanes are one cache line, few lookups hit, and the merged wave walks to its longest ray.
// The loop ends: t = (float)k * h grows without bound and lim <= r <= sqrt(hi2) is finite (k <= max_range / step + 1 <= 65537).
struct Carve {
    long long add;     // weight * rintf(tau * 2^24)
    unsigned weight;
    float margin;
};

__device__ __forceinline__ void carve_ray(const Tsdf &M, const GnPose32 &P, float x, float y, float z, const Rays &R,
                                          const Carve &C) {
    const float r2 = (x * x + y * y) + z * z;
    if (!(r2 >= R.lo2 && r2 <= R.hi2)) return;
    const float r = sqrtf(r2), lim = r - C.margin;
    float q[3], u[3];
    gn_xform(P, x, y, z, q);
#pragma unroll
    for (int a = 0; a < 3; ++a) u[a] = __fdiv_rn(q[a] - P.t[a], r);
    unsigned long long prev = EMPTY;
    for (int k = 1;; ++k) {
        const float t = (float)k * R.h;
        if (!(t < lim)) break;
        int vox[3] = {0, 0, 0}, sub;
        int inside = 1;
#pragma unroll
        for (int a = 0; a < 3; ++a) inside &= axis_cell(P.t[a] + u[a] * t, M.v, 1, vox[a], sub);
        if (!inside) continue;
        const unsigned long long key = pack_key(vox[0], vox[1], vox[2]);
        if (key == prev) continue;
        prev = key;
        const int slot = find_slot(M.keys(), M.cap_vox, key);
        if (slot < 0) continue;
        atomicAdd((unsigned long long *)&M.sum()[slot], (unsigned long long)C.add);
        atomicAdd(&M.count()[slot], C.weight);
    }
}

// a lane leaves on its own: past the rows of its frame, or with its list entry
template <typename Src>
__global__ __launch_bounds__(TS_BLOCK) void ts_carve_kernel(Tsdf M, Src S, Rays R, Carve C) {
    SourceRows o;
    if (!S.open(o)) return;
    const int i = blockIdx.x * TS_BLOCK + threadIdx.x;
    if (i >= o.n) return;
    const GnPose32 P = gn_load_pose(o.pose, M.ox, M.oy, M.oz);
    float x, y, z;
    S.point(o, i, x, y, z);
    carve_ray(M, P, x, y, z, R, C);
}

__global__ __launch_bounds__(TS_BLOCK) void ts_export_kernel(Tsdf M, unsigned long long *keys, long long *sums, uint32_t *counts,
                                                             int32_t *count, int max_out) {
    const int slot = blockIdx.x * TS_BLOCK + threadIdx.x;
    if (slot >= M.cap_vox) return;
    const unsigned long long key = M.keys()[slot];
    if (key == EMPTY) return;
    const int pos = atomicAdd(count, 1);
    if (pos < 0 || pos >= max_out) return;
    keys[pos] = key, sums[pos] = M.sum()[slot], counts[pos] = M.count()[slot];
}

// ------------------------------------------------------------------------------------------------------------ rolling the map
// Nothing can be deleted from a table whose empty key ends a probe, so a map is rolled by REBUILDING it: evict moves the voxels of
// the tiles (csrc/voxel_hash.h) near a pose into a second, cleared table and lists the others for the host; absorb adds listed
// records back.  A voxel is (key, int64 sum, uint32 count) and every write is an integer add, so a voxel's content split between
// the table and the host adds back to the same bytes.
struct EvictOut {
    unsigned long long *keys;
    long long *sums;
    uint32_t *counts;
    int32_t *count;
    int max_out;
};

// dst cleared, src's three counters carried over, the list's counter zeroed
__global__ __launch_bounds__(TS_BLOCK) void ts_evict_clear_kernel(Tsdf S, Tsdf D, int32_t *count) {
    const size_t tid = (size_t)blockIdx.x * TS_BLOCK + threadIdx.x, stride = (size_t)gridDim.x * TS_BLOCK;
    if (tid < 64) ((unsigned *)D.base)[tid] = tid < 3 ? ((const unsigned *)S.base)[tid] : 0u;
    if (tid == 0) count[0] = 0;
    for (size_t i = tid; i < (size_t)D.cap_vox; i += stride) D.keys()[i] = EMPTY, D.sum()[i] = 0, D.count()[i] = 0u;
}

// One lane per slot of src.  A lane past the table or on an empty slot does NOT leave before the ballot: the far voxels of a wave
// take their list positions with one atomic (the first far lane adds their number, every far lane adds its rank among them), as
// integrate_ray keeps the wave together for its sums.  A far voxel whose position is at or past max_out stays: it is claimed in
// dst like a near one, so nothing is dropped.  Keys are unique in src, so the values are stored plainly.
__global__ __launch_bounds__(TS_BLOCK) void ts_evict_kernel(Tsdf S, Tsdf D, const double *pose, float r2, int b, EvictOut O) {
    const int slot = blockIdx.x * TS_BLOCK + threadIdx.x, lane = threadIdx.x & 63;
    const unsigned long long key = slot < S.cap_vox ? S.keys()[slot] : EMPTY;
    const bool held = key != EMPTY;
    const bool far = held && !tile_near(key, b, S.v, pose, S.ox, S.oy, S.oz, r2);
    const unsigned long long wants = __ballot(far);
    int base = 0;
    const int first = wants ? __ffsll((long long)wants) - 1 : 0;
    if (far && lane == first) base = atomicAdd(O.count, (int)__popcll(wants));
    base = __shfl(base, first, 64);
    if (!held) return;
    const long long sum = S.sum()[slot];
    const unsigned count = S.count()[slot];
    if (far) {
        const int pos = base + (int)__popcll(wants & ((1ull << lane) - 1ull));
        if (pos >= 0 && pos < O.max_out) {
            O.keys[pos] = key, O.sums[pos] = sum, O.counts[pos] = count;
            return;
        }
    }
    const int to = claim_slot(D.keys(), D.cap_vox, key);   // never full: no more keys than src holds
    if (to < 0) {
        atomicAdd(&D.hdr()->overflow, 1u);
        return;
    }
    D.sum()[to] = sum, D.count()[to] = count;
}

// One lane per record: the slot found or claimed, then the integer atomics of integrate, so equal keys in the list and keys the
// table holds add, in any order to the same bytes.  A key with bit 63 set cannot be a voxel (EMPTY is one): header word 1.
__global__ __launch_bounds__(TS_BLOCK) void ts_absorb_kernel(Tsdf M, const unsigned long long *keys, const long long *sums,
                                                             const uint32_t *counts, int n) {
    const int i = blockIdx.x * TS_BLOCK + threadIdx.x;
    if (i >= n) return;
    const unsigned long long key = keys[i];
    if (key >> 63) {
        atomicAdd(&M.hdr()->outside, 1u);
        return;
    }
    const unsigned count = counts[i];
    if (count == 0u) return;
    const int slot = claim_slot(M.keys(), M.cap_vox, key);
    if (slot < 0) {
        atomicAdd(&M.hdr()->overflow, 1u);
        return;
    }
    atomicAdd((unsigned long long *)&M.sum()[slot], (unsigned long long)sums[i]);
    atomicAdd(&M.count()[slot], count);
}

// ------------------------------------------------------------------------------------------------------------------ the field
// D of a slot; false when the slot is none (-1) or its voxel is not qualified
__device__ __forceinline__ bool slot_value(const Tsdf &M, int slot, unsigned min_count, float &D) {
    if (slot < 0) return false;
    const unsigned n = M.count()[slot];
    if (n < min_count) return false;
    D = (float)__ddiv_rn((double)M.sum()[slot], (double)n * 16777216.0);
    return true;
}

// D of the voxel with (biased) coordinates (x, y, z); false outside the 21 bits, without a slot or when not qualified
__device__ __forceinline__ bool voxel_value(const Tsdf &M, int x, int y, int z, unsigned min_count, float &D) {
    if ((unsigned)x > 0x1FFFFFu || (unsigned)y > 0x1FFFFFu || (unsigned)z > 0x1FFFFFu) return false;
    return slot_value(M, find_slot(M.keys(), M.cap_vox, pack_key(x, y, z)), min_count, D);
}

// g += grad(k) of the qualified voxel k = (x[0], x[1], x[2]) with value D
__device__ __forceinline__ void add_grad(const Tsdf &M, const int x[3], float D, unsigned min_count, float g[3]) {
#pragma unroll
    for (int b = 0; b < 3; ++b) {
        float Dp = 0.f, Dm = 0.f;
        const bool hp = voxel_value(M, x[0] + (b == 0), x[1] + (b == 1), x[2] + (b == 2), min_count, Dp);
        const bool hm = voxel_value(M, x[0] - (b == 0), x[1] - (b == 1), x[2] - (b == 2), min_count, Dm);
        g[b] += hp && hm ? Dp - Dm : hp ? 2.f * (Dp - D) : hm ? 2.f * (D - Dm) : 0.f;
    }
}

// the normal of a crossing between the qualified voxels x0 and x1: g = grad(x0) + grad(x1) divided per axis by its length, or zeros
__device__ __forceinline__ void edge_normal(const Tsdf &M, const int x0[3], float D0, const int x1[3], float D1, unsigned min_count,
                                            float n[3]) {
    float g0[3] = {0.f, 0.f, 0.f}, g1[3] = {0.f, 0.f, 0.f};
    add_grad(M, x0, D0, min_count, g0);
    add_grad(M, x1, D1, min_count, g1);
    const float gx = g0[0] + g1[0], gy = g0[1] + g1[1], gz = g0[2] + g1[2];
    const float len = sqrtf((gx * gx + gy * gy) + gz * gz);
    const bool unit = len > 0.f;
    n[0] = unit ? __fdiv_rn(gx, len) : 0.f;
    n[1] = unit ? __fdiv_rn(gy, len) : 0.f;
    n[2] = unit ? __fdiv_rn(gz, len) : 0.f;
}

// Ownership by tiles (csrc/voxel_hash.h): an extraction that is given a sorted list of n tile keys emits only what is anchored at
// a voxel k0 whose tile, pack_key(x >> b, y >> b, z >> b), is in the list; n == 0: everything.  A list of up to OWN_LDS keys is
// staged in LDS by own_stage, which EVERY thread of the block calls before any leaves (it holds a barrier); a longer one is
// searched where it lies.
constexpr int OWN_LDS = 1024;

struct Owners {
    const unsigned long long *tiles;
    int n, b;
};

__device__ __forceinline__ const unsigned long long *own_stage(const Owners &O, unsigned long long *lds) {
    if (O.n == 0 || O.n > OWN_LDS) return O.tiles;
    for (int i = threadIdx.x; i < O.n; i += TS_BLOCK) lds[i] = O.tiles[i];
    __syncthreads();
    return lds;
}

__device__ __forceinline__ bool owned(const Owners &O, const unsigned long long *list, unsigned long long k0) {
    if (O.n == 0) return true;
    const unsigned long long t = pack_key(key_axis(k0, 0) >> O.b, key_axis(k0, 1) >> O.b, key_axis(k0, 2) >> O.b);
    int lo = 0, hi = O.n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (list[mid] < t) lo = mid + 1;
        else hi = mid;
    }
    return lo < O.n && list[lo] == t;
}

// An edge runs from a voxel p to the voxel q = p + d, d = dx | dy << 1 | dz << 2 not 0.  Its direction code, and d of a code:
// 1, 2, 4 (the axes) <-> 0, 1, 2; 3, 5, 6 (the face diagonals) <-> 3, 4, 5; 7 (the body diagonal) <-> 6.
__host__ __device__ constexpr int edge_dir(int d) { return (0x65423100 >> (4 * d)) & 7; }
__host__ __device__ constexpr int dir_edge(int dir) { return (0x7653421 >> (4 * dir)) & 7; }
constexpr bool dirs_invert(int d = 7) { return d == 0 || (dir_edge(edge_dir(d)) == d && edge_dir(d) < 7 && dirs_invert(d - 1)); }
static_assert(dirs_invert() && edge_dir(4) == 2 && edge_dir(3) == 3 && edge_dir(7) == 6, "edge_dir and dir_edge invert each other");

// the point of the edge p - q where the field changes sign: f = Dp / (Dp - Dq), p's centre c with f * v added on every axis of d
__device__ __forceinline__ void edge_point(const float c[3], int d, float Dp, float Dq, float v, float *xyz) {
    const float f = __fdiv_rn(Dp, Dp - Dq);
#pragma unroll
    for (int b = 0; b < 3; ++b) xyz[b] = (d >> b) & 1 ? c[b] + f * v : c[b];
}

// the records of the qualified voxel k0 with value D0: one per axis whose neighbour k1 is qualified with the other sign
__device__ __forceinline__ void put_crossings(const Tsdf &M, unsigned min_count, unsigned long long k0, float D0,
                                              unsigned long long *keys, int32_t *axes, float *xyz, float *normals, int32_t *count,
                                              int max_out) {
    const int x0[3] = {key_axis(k0, 0), key_axis(k0, 1), key_axis(k0, 2)};
    float c[3];
    voxel_centre(k0, M.v, c);
    for (int a = 0; a < 3; ++a) {
        const int x1[3] = {x0[0] + (a == 0), x0[1] + (a == 1), x0[2] + (a == 2)};
        float D1;
        if (!voxel_value(M, x1[0], x1[1], x1[2], min_count, D1) || (D0 < 0.f) == (D1 < 0.f)) continue;
        const int pos = atomicAdd(count, 1);
        if (pos < 0 || pos >= max_out) continue;
        float n[3];
        edge_normal(M, x0, D0, x1, D1, min_count, n);   // every read before the first write
        keys[pos] = k0, axes[pos] = a;
        edge_point(c, 1 << a, D0, D1, M.v, &xyz[3 * (size_t)pos]);
#pragma unroll
        for (int b = 0; b < 3; ++b) normals[3 * (size_t)pos + b] = n[b];
    }
}

__global__ __launch_bounds__(TS_BLOCK) void ts_surface_kernel(Tsdf M, unsigned min_count, unsigned long long *keys, int32_t *axes,
                                                              float *xyz, float *normals, int32_t *count, int max_out) {
    const int slot = blockIdx.x * TS_BLOCK + threadIdx.x;
    if (slot >= M.cap_vox) return;
    const unsigned long long k0 = M.keys()[slot];
    float D0;
    if (k0 == EMPTY || !slot_value(M, slot, min_count, D0)) return;
    put_crossings(M, min_count, k0, D0, keys, axes, xyz, normals, count, max_out);
}

// ts_surface_kernel's records, in its order, of the owned voxels
__global__ __launch_bounds__(TS_BLOCK) void ts_surface_tiles_kernel(Tsdf M, unsigned min_count, Owners W, unsigned long long *keys,
                                                                    int32_t *axes, float *xyz, float *normals, int32_t *count,
                                                                    int max_out) {
    __shared__ unsigned long long own[OWN_LDS];
    const unsigned long long *list = own_stage(W, own);
    const int slot = blockIdx.x * TS_BLOCK + threadIdx.x;
    if (slot >= M.cap_vox) return;
    const unsigned long long k0 = M.keys()[slot];
    float D0;
    if (k0 == EMPTY || !slot_value(M, slot, min_count, D0) || !owned(W, list, k0)) return;
    put_crossings(M, min_count, k0, D0, keys, axes, xyz, normals, count, max_out);
}

// ------------------------------------------------------------------------------------------------------- marching tetrahedra
struct MeshOut {
    unsigned long long *vkeys;   // (max_out,3)
    int32_t *vdirs;              // (max_out,3)
    float *xyz;                  // (max_out,3,3)
    int32_t *count;
    int max_out;
};

struct Cell {
    int x[3];
    float D[8], v;
};

// vertex j of triangle `pos`: on the edge between corners m[i0] and m[i1] of a tetrahedron whose corners are nested, m[0] c m[1] ...
__device__ __forceinline__ void put_vertex(const MeshOut &O, const Cell &C, const int m[4], int i0, int i1, int pos, int j) {
    const int p = m[min(i0, i1)], q = m[max(i0, i1)], d = q ^ p;
    const unsigned long long key = pack_key(C.x[0] + (p & 1), C.x[1] + ((p >> 1) & 1), C.x[2] + (p >> 2));
    float c[3];
    voxel_centre(key, C.v, c);
    const size_t at = 3 * (size_t)pos + j;
    O.vkeys[at] = key;
    O.vdirs[at] = edge_dir(d);
    edge_point(c, d, C.D[p], C.D[q], C.v, &O.xyz[3 * at]);
}

// the triangle on the edges (a0,a1), (b0,b1), (c0,c1); flip: the last two change places
__device__ __forceinline__ void put_triangle(const MeshOut &O, const Cell &C, const int m[4], int a0, int a1, int b0, int b1,
                                             int c0, int c1, bool flip) {
    const int pos = atomicAdd(O.count, 1);
    if (pos < 0 || pos >= O.max_out) return;
    put_vertex(O, C, m, a0, a1, pos, 0);
    put_vertex(O, C, m, flip ? c0 : b0, flip ? c1 : b1, pos, 1);
    put_vertex(O, C, m, flip ? b0 : c0, flip ? b1 : c1, pos, 2);
}

// The triangles of a cell whose corner m has bit m of `neg` set when D[m] < 0, each handed to emit(m, a0, a1, b0, b1, c0, c1, flip):
// put_triangle's arguments, m the four nested corners of the tetrahedron it lies in.
template <typename Emit>
__device__ __forceinline__ void march_cell(int neg, Emit emit) {
    for (int t = 0; t < 6; ++t) {
        // the t-th permutation (a, b, c) of the axes in lexicographic order; odd ones give a left-handed tetrahedron
        const int a = t >> 1, b = (0x489 >> (2 * t)) & 3;   // b = 1, 2, 0, 2, 0, 1
        const bool odd = (0x26 >> t) & 1;                    // t = 1, 2, 5
        const int m[4] = {0, 1 << a, (1 << a) | (1 << b), 7};
        int nm = 0;
        for (int i = 0; i < 4; ++i) nm |= ((neg >> m[i]) & 1) << i;
        const int cnt = __popc(nm);
        if (cnt == 0 || cnt == 4) continue;
        if (cnt != 2) {
            // corner A alone on its side; (A, B, C, D) with B < C < D is an even permutation when A is even
            const int A = __ffs(cnt == 1 ? nm : (~nm & 15)) - 1;
            const int B = A == 0 ? 1 : 0, Cc = A <= 1 ? 2 : 1, Dd = A == 3 ? 2 : 3;
            emit(m, A, B, A, Cc, A, Dd, ((A & 1) != 0) ^ odd ^ (cnt == 3));
        } else {
            // A < B negative, Cc < Dd positive; the parity of (A, B, Cc, Dd) is that of its inversions
            const int A = __ffs(nm) - 1, B = 31 - __clz(nm), pm = ~nm & 15, Cc = __ffs(pm) - 1, Dd = 31 - __clz(pm);
            const int inv = (A > Cc) + (A > Dd) + (B > Cc) + (B > Dd);
            const bool swap = ((inv & 1) != 0) ^ odd;
            const int P = swap ? Dd : Cc, Q = swap ? Cc : Dd;
            emit(m, A, P, A, Q, B, Q, false);
            emit(m, A, P, B, Q, B, P, false);
        }
    }
}

// The cell anchored at the qualified voxel k0 of `slot`, D[0] its value: D and the slot of every corner, bit m of neg set when
// D[m] < 0.  false at the first corner that lies outside the 21 bits, has no slot or is not qualified.
__device__ __forceinline__ bool load_cell(const Tsdf &M, unsigned min_count, int slot, unsigned long long k0, float D[8], int at[8],
                                          int &neg) {
    at[0] = slot;
    neg = D[0] < 0.f;
    for (int m = 1; m < 8; ++m) {
        const int x = key_axis(k0, 0) + (m & 1), y = key_axis(k0, 1) + ((m >> 1) & 1), z = key_axis(k0, 2) + (m >> 2);
        if ((unsigned)x > 0x1FFFFFu || (unsigned)y > 0x1FFFFFu || (unsigned)z > 0x1FFFFFu) return false;
        at[m] = find_slot(M.keys(), M.cap_vox, pack_key(x, y, z));
        if (!slot_value(M, at[m], min_count, D[m])) return false;
        neg |= (D[m] < 0.f) << m;
    }
    return true;
}

__global__ __launch_bounds__(TS_BLOCK) void ts_mesh_kernel(Tsdf M, unsigned min_count, MeshOut O) {
    const int slot = blockIdx.x * TS_BLOCK + threadIdx.x;
    if (slot >= M.cap_vox) return;
    const unsigned long long k0 = M.keys()[slot];
    Cell C;
    C.v = M.v;
    int at[8], neg;
    if (k0 == EMPTY || !slot_value(M, slot, min_count, C.D[0])) return;
    if (!load_cell(M, min_count, slot, k0, C.D, at, neg) || neg == 0 || neg == 255) return;
    for (int a = 0; a < 3; ++a) C.x[a] = key_axis(k0, a);
    march_cell(neg, [&](const int m[4], int a0, int a1, int b0, int b1, int c0, int c1, bool flip) {
        put_triangle(O, C, m, a0, a1, b0, b1, c0, c1, flip);
    });
}

// ---------------------------------------------------------------------------------------------------------- the indexed mesh
// The same cells and triangles with the weld done here: a vertex is named (key of p, direction) and p is a slot of this table, so
// (slot << 3) | direction is a vertex id that needs no sorting of names.  Six launches, integer atomics only:
//   clear     the mask words and the two counts
//   cells     ts_mesh_kernel's walk over the cells whose base voxel is owned: a triangle takes its position by atomicAdd and is
//             written as three ids; every id sets bit `direction` of its slot's byte of the mask (atomicOr on the 32-bit word)
//   count     the popcounts of the masks summed per block of 256 slots
//   scan      one block: the exclusive scan of those sums in place, and V, their total
//   vertices  one lane per slot: the block's sum + the scan inside the block is the slot's first vertex index; per used
//             direction, ascending, the name, put_vertex's position and ts_surface_kernel's normal of the edge p - q
//   remap     one lane per written id: first[slot] + the used directions below it
// Which index a vertex gets follows the slots, and the slots follow the order of arrival: the caller sorts by name.
struct MeshIdx {
    unsigned *mask;          // cap_vox bytes in 32-bit words: byte s = the used directions of slot s
    int32_t *first;          // (cap_vox,) the first vertex index of slot s
    int32_t *block_first;    // (cap_vox / 256 rounded up,)
    int32_t *counts;         // V, F
    unsigned long long *vkeys;
    int32_t *vdirs;
    float *xyz, *normals;
    int32_t *faces;          // (max_f,3)
    int max_v, max_f;
};

constexpr int SCAN_BLOCK = 1024;

__device__ __forceinline__ unsigned slot_mask(const MeshIdx &X, int slot) { return ((const unsigned char *)X.mask)[slot]; }

__global__ __launch_bounds__(TS_BLOCK) void ts_mesh_clear_kernel(MeshIdx X, int words) {
    const size_t tid = (size_t)blockIdx.x * TS_BLOCK + threadIdx.x, stride = (size_t)gridDim.x * TS_BLOCK;
    if (tid < 2) X.counts[tid] = 0;
    for (size_t i = tid; i < (size_t)words; i += stride) X.mask[i] = 0u;
}

__global__ __launch_bounds__(TS_BLOCK) void ts_mesh_cells_kernel(Tsdf M, unsigned min_count, Owners W, MeshIdx X) {
    __shared__ unsigned long long own[OWN_LDS];
    const unsigned long long *list = own_stage(W, own);
    const int slot = blockIdx.x * TS_BLOCK + threadIdx.x;
    if (slot >= M.cap_vox) return;
    const unsigned long long k0 = M.keys()[slot];
    float D[8];
    int at[8], neg;
    if (k0 == EMPTY || !slot_value(M, slot, min_count, D[0]) || !owned(W, list, k0)) return;
    if (!load_cell(M, min_count, slot, k0, D, at, neg) || neg == 0 || neg == 255) return;
    march_cell(neg, [&](const int m[4], int a0, int a1, int b0, int b1, int c0, int c1, bool flip) {
        const int e[3][2] = {{a0, a1}, {flip ? c0 : b0, flip ? c1 : b1}, {flip ? b0 : c0, flip ? b1 : c1}};
        const int pos = atomicAdd(&X.counts[1], 1);
        const bool room = pos >= 0 && pos < X.max_f;
        for (int j = 0; j < 3; ++j) {
            const int p = m[min(e[j][0], e[j][1])], dir = edge_dir(m[max(e[j][0], e[j][1])] ^ p), s = at[p];
            atomicOr(&X.mask[s >> 2], (1u << dir) << (8 * (s & 3)));   // also without room: V is counted in full
            if (room) X.faces[3 * (size_t)pos + j] = (s << 3) | dir;
        }
    });
}

__global__ __launch_bounds__(TS_BLOCK) void ts_mesh_count_kernel(int cap_vox, MeshIdx X) {
    __shared__ int part[TS_BLOCK / 64];
    const int slot = blockIdx.x * TS_BLOCK + threadIdx.x;
    const int total = block_total<TS_BLOCK / 64>(slot < cap_vox ? __popc(slot_mask(X, slot)) : 0, part);
    if (threadIdx.x == 0) X.block_first[blockIdx.x] = total;
}

__global__ __launch_bounds__(SCAN_BLOCK) void ts_mesh_scan_kernel(int blocks, int per, MeshIdx X) {
    __shared__ int wsum[SCAN_BLOCK / 64];
    const int total = block_scan_runs(X.block_first, blocks, per, wsum);
    if (threadIdx.x == SCAN_BLOCK - 1) X.counts[0] = total;
}

__global__ __launch_bounds__(TS_BLOCK) void ts_mesh_vertices_kernel(Tsdf M, unsigned min_count, MeshIdx X) {
    __shared__ int wsum[TS_BLOCK / 64];
    const int slot = blockIdx.x * TS_BLOCK + threadIdx.x;
    const unsigned mask = slot < M.cap_vox ? slot_mask(X, slot) : 0u;
    int idx = block_scan_exclusive((int)__popc(mask), wsum, (int)X.block_first[blockIdx.x]);
    if (slot >= M.cap_vox) return;
    X.first[slot] = idx;
    if (mask == 0u) return;
    const unsigned long long key = M.keys()[slot];
    float Dp = 0.f, c[3];
    slot_value(M, slot, min_count, Dp);      // a marked slot is a qualified corner of a meshed cell, and so is every q below
    voxel_centre(key, M.v, c);
    const int x0[3] = {key_axis(key, 0), key_axis(key, 1), key_axis(key, 2)};
    for (int dir = 0; dir < 7; ++dir) {
        if (!((mask >> dir) & 1u)) continue;
        const int at = idx++;
        if (at >= X.max_v) continue;
        const int d = dir_edge(dir);
        const int x1[3] = {x0[0] + (d & 1), x0[1] + ((d >> 1) & 1), x0[2] + (d >> 2)};
        float Dq = 0.f, n[3];
        voxel_value(M, x1[0], x1[1], x1[2], min_count, Dq);
        edge_normal(M, x0, Dp, x1, Dq, min_count, n);
        X.vkeys[at] = key, X.vdirs[at] = dir;
        edge_point(c, d, Dp, Dq, M.v, &X.xyz[3 * (size_t)at]);
#pragma unroll
        for (int b = 0; b < 3; ++b) X.normals[3 * (size_t)at + b] = n[b];
    }
}

__global__ __launch_bounds__(TS_BLOCK) void ts_mesh_remap_kernel(MeshIdx X) {
    const size_t i = (size_t)blockIdx.x * TS_BLOCK + threadIdx.x;
    if (i >= 3 * (size_t)min(max(X.counts[1], 0), X.max_f)) return;
    const int id = X.faces[i], s = id >> 3;
    X.faces[i] = X.first[s] + (int)__popc(slot_mask(X, s) & ((1u << (id & 7)) - 1u));
}

// ------------------------------------------------------------------------------------------- the field at a point, registration
// The trilinear interpolant of D between the 8 voxel centres round q (map frame) and its exact gradient inside that cell, in
// fp32, every operation rounded once, no fmaf: include/dpm_hip.h (dpm_tsdf_sample) is the rule and tests/tsdf_register_restated.py
// equals it bit for bit.  false -- the point HAS NO VALUE -- when the cell leaves the 21 bits (a NaN fails the comparison) or one
// of the 8 corners is not qualified: a missing corner is never read as 0.  Lookups only.
__device__ __forceinline__ bool field_at(const Tsdf &M, const float q[3], unsigned min_count, float &d, float grad[3], float &n2) {
    float f[3], fl[3];
    bool valid = true;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float g = __fdiv_rn(q[a], M.v) - 0.5f;
        fl[a] = floorf(g);
        valid = valid && fl[a] >= -1048576.f && fl[a] < 1048575.f;   // fl and fl + 1 fit the 21 bits
        f[a] = g - fl[a];
    }
    if (!valid) return false;
    const int i0[3] = {(int)fl[0] + 1048576, (int)fl[1] + 1048576, (int)fl[2] + 1048576};
    float D[2][2][2];
#pragma unroll
    for (int m = 0; m < 8; ++m)
        if (!voxel_value(M, i0[0] + (m & 1), i0[1] + ((m >> 1) & 1), i0[2] + (m >> 2), min_count, D[m & 1][(m >> 1) & 1][m >> 2])) return false;
    float e[2][2], c[2][2], mm[2], b[2], t[2];
#pragma unroll
    for (int dy = 0; dy < 2; ++dy)
#pragma unroll
        for (int dz = 0; dz < 2; ++dz) {
            e[dy][dz] = D[1][dy][dz] - D[0][dy][dz];
            c[dy][dz] = D[0][dy][dz] + f[0] * e[dy][dz];
        }
#pragma unroll
    for (int dz = 0; dz < 2; ++dz) {
        mm[dz] = c[1][dz] - c[0][dz];
        b[dz] = c[0][dz] + f[1] * mm[dz];
        t[dz] = e[0][dz] + f[1] * (e[1][dz] - e[0][dz]);
    }
    const float hz = b[1] - b[0];
    d = b[0] + f[2] * hz;
    const float hy = mm[0] + f[2] * (mm[1] - mm[0]);
    const float hx = t[0] + f[2] * (t[1] - t[0]);
    grad[0] = __fdiv_rn(hx, M.v), grad[1] = __fdiv_rn(hy, M.v), grad[2] = __fdiv_rn(hz, M.v);
    n2 = (grad[0] * grad[0] + grad[1] * grad[1]) + grad[2] * grad[2];
    return true;
}

__global__ __launch_bounds__(TS_BLOCK) void ts_sample_kernel(Tsdf M, const float *xyz, const int32_t *count, int cap,
                                                             const double *pose, unsigned min_count, float *d, float *grad,
                                                             int32_t *flag) {
    const int i = blockIdx.x * TS_BLOCK + threadIdx.x;
    if (i >= cap) return;
    float dv = 0.f, g[3] = {0.f, 0.f, 0.f}, n2;
    int fl = -1;
    if (i < min(max(count[0], 0), cap)) {
        const GnPose32 P = gn_load_pose(pose, M.ox, M.oy, M.oz);
        float q[3];
        gn_xform(P, xyz[3 * (size_t)i], xyz[3 * (size_t)i + 1], xyz[3 * (size_t)i + 2], q);
        fl = field_at(M, q, min_count, dv, g, n2) ? 1 : 0;
        if (!fl) dv = 0.f, g[0] = g[1] = g[2] = 0.f;
    }
    d[i] = dv, flag[i] = fl;
    grad[3 * (size_t)i] = g[0], grad[3 * (size_t)i + 1] = g[1], grad[3 * (size_t)i + 2] = g[2];
}

// Scan-to-field registration: csrc/gn_one.h's driver, as csrc/local_map.hip's register_impl, with the field in place of the search.
struct TsRegArgs {   // the accumulate kernel's arguments; hdr and partial are csrc/gn_one.h's
    Tsdf M;
    const float *xyz;
    const int32_t *count;
    int cap;
    unsigned min_count;
    float grad_min2;
    GnOneHdr *hdr;
    double *partial;
    double *pose;
    float *fitness, *rmse;
    int32_t *iterations, *status;
    int32_t *dbg_flag;      // (cap,) or NULL: 1 the row was given, 0 it was not, -1 past the count
    double *dbg_system;     // (GN_NSUM,) or NULL
};

// One lane per row, 256 rows a block: 8 find_slot probes and the sum / count loads of the corners they find, then the row into
// the lane's own 29 fp64 sums.  Every lane may hold a row, so the butterfly runs all six offsets (gn_block_reduce<1>; the default
// stops at 4 for kernels whose rows sit in lane 0 of a quad), then the four waves in the fixed tree.
__global__ __launch_bounds__(TS_BLOCK) void ts_reg_accumulate_kernel(TsRegArgs A, float max_dist, double kappa) {
    if (A.hdr->done) return;
    const int blk = blockIdx.x, i = blk * TS_BLOCK + threadIdx.x, n1 = A.hdr->n1;
    double s[GN_NSUM];
#pragma unroll
    for (int k = 0; k < GN_NSUM; ++k) s[k] = 0.0;
    if (i < n1) {
        const GnPose32 P = gn_load_pose(A.pose, A.M.ox, A.M.oy, A.M.oz);
        float q[3], d, g[3], n2;
        gn_xform(P, A.xyz[3 * (size_t)i], A.xyz[3 * (size_t)i + 1], A.xyz[3 * (size_t)i + 2], q);
        // a NaN fails every comparison; n2 < FLT_MAX: finite
        const bool row = field_at(A.M, q, A.min_count, d, g, n2) && fabsf(d) <= max_dist && n2 >= A.grad_min2 && n2 <= 3.402823466e38f;
        if (A.dbg_flag) A.dbg_flag[i] = row ? 1 : 0;
        if (row) {
            const double p[3] = {q[0], q[1], q[2]}, gd[3] = {g[0], g[1], g[2]};
            s[27] += 1.0;
            gn_field_row(s, p, gd, (double)d, kappa);
        }
    } else if (i < A.cap && A.dbg_flag) {
        A.dbg_flag[i] = -1;
    }
    gn_block_reduce<1>(s, A.partial, blk);
}

// ------------------------------------------------------------------------------------------------------- ray-casting the field
// The occupied-block set: the keys (x >> 3, y >> 3, z >> 3) of the 8 x 8 x 8 blocks that hold a voxel qualified at min_count, in a
// second open-addressing set of cap_blocks slots behind a 256-byte header (word 0: claims that found no room).  Integer
// compare-and-swap only, so membership is a function of the table's content and min_count alone.  A block key has 3 x 18 bits
// and is never EMPTY.
struct BlockSet {
    unsigned char *base;     // nullptr: the plain form of the marcher
    int cap;
    __host__ __device__ unsigned long long *keys() const { return (unsigned long long *)(base + 256); }
};

__device__ __forceinline__ unsigned long long block_key(int x, int y, int z) { return pack_key(x >> 3, y >> 3, z >> 3); }

__global__ __launch_bounds__(TS_BLOCK) void ts_blocks_clear_kernel(BlockSet B) {
    const size_t tid = (size_t)blockIdx.x * TS_BLOCK + threadIdx.x, stride = (size_t)gridDim.x * TS_BLOCK;
    if (tid < 64) ((unsigned *)B.base)[tid] = 0u;
    for (size_t i = tid; i < (size_t)B.cap; i += stride) B.keys()[i] = EMPTY;
}

// one lane per slot of the table; the voxels of one block sit in unrelated slots, so nothing is merged before the claim
__global__ __launch_bounds__(TS_BLOCK) void ts_blocks_kernel(Tsdf M, unsigned min_count, BlockSet B) {
    const int slot = blockIdx.x * TS_BLOCK + threadIdx.x;
    if (slot >= M.cap_vox) return;
    const unsigned long long key = M.keys()[slot];
    if (key == EMPTY || M.count()[slot] < min_count) return;
    if (claim_slot(B.keys(), B.cap, block_key(key_axis(key, 0), key_axis(key, 1), key_axis(key, 2))) < 0)
        atomicAdd((unsigned *)B.base, 1u);
}

// The marcher: one lane per ray, grid y the pose; neighbouring lanes are neighbouring columns of one beam.  Sample k lies at
// t_k = t0 + (float)k * h, p_k = o + u * t_k; its value and gradient are field_at's, and the ray ends at the first pair of valued
// samples k - 1, k whose signs (d > 0) differ (include/dpm_hip.h is the rule; tests/tsdf_raycast_restated.py equals it bit for bit).
// SKIP: a sample whose base voxel i0 -- field_at's own, formed by the same three operations -- lies in a block the set does not
// hold cannot have a value (its corner (0,0,0) is not qualified), so field_at is not run for it.  The block's answer stays in two
// registers while consecutive samples stay inside the block (16 samples at half-voxel steps along an axis): empty space costs
// one probe of the set per block entered and none in between.  No sample is stepped over: every k forms its own p_k and i0, so
// the bytes are those of the plain form.
struct Cast {
    float t0, h;
    int K;
    unsigned min_count;
};

template <bool SKIP>
__global__ __launch_bounds__(TS_BLOCK) void ts_raycast_kernel(Tsdf M, BlockSet B, const double *poses, const float *dirs, int R,
                                                              Cast C, float *range, float *normals, int32_t *flag) {
    const int r = blockIdx.x * TS_BLOCK + threadIdx.x, f = blockIdx.y;
    if (r >= R) return;
    const GnPose32 P = gn_load_pose(poses + 16 * (size_t)f, M.ox, M.oy, M.oz);
    const float dx = dirs[3 * (size_t)r], dy = dirs[3 * (size_t)r + 1], dz = dirs[3 * (size_t)r + 2];
    float u[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) u[a] = fmaf(P.R[3 * a + 2], dz, fmaf(P.R[3 * a + 1], dy, P.R[3 * a] * dx));
    bool prev = false;
    float dp = 0.f, gp[3] = {0.f, 0.f, 0.f};
    unsigned long long held = EMPTY;      // the block of the last valid base voxel, and whether the set holds it
    bool present = false;
    int out = 0;
    float rg = 0.f, n[3] = {0.f, 0.f, 0.f};
    for (int k = 0; k < C.K; ++k) {
        const float t = C.t0 + (float)k * C.h;
        const float p[3] = {P.t[0] + u[0] * t, P.t[1] + u[1] * t, P.t[2] + u[2] * t};
        bool may = true;
        if constexpr (SKIP) {
            float fl[3];
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                fl[a] = floorf(__fdiv_rn(p[a], M.v) - 0.5f);
                may = may && fl[a] >= -1048576.f && fl[a] < 1048575.f;   // a NaN fails: no cell, no value
            }
            if (may) {
                const unsigned long long bk = block_key((int)fl[0] + 1048576, (int)fl[1] + 1048576, (int)fl[2] + 1048576);
                if (bk != held) held = bk, present = find_slot(B.keys(), B.cap, bk) >= 0;
                may = present;
            }
        }
        float d = 0.f, g[3] = {0.f, 0.f, 0.f}, n2;
        const bool has = may && field_at(M, p, C.min_count, d, g, n2);
        if (has && prev && (dp > 0.f) != (d > 0.f)) {
            const float fr = __fdiv_rn(dp, dp - d);
            rg = (C.t0 + (float)(k - 1) * C.h) + fr * C.h;
            out = dp > 0.f ? 1 : 2;
            float gm[3];
#pragma unroll
            for (int a = 0; a < 3; ++a) gm[a] = gp[a] + fr * (g[a] - gp[a]);
            const float len = sqrtf((gm[0] * gm[0] + gm[1] * gm[1]) + gm[2] * gm[2]);
            if (len > 0.f && len <= 3.402823466e38f) {   // a NaN fails
#pragma unroll
                for (int a = 0; a < 3; ++a) gm[a] = __fdiv_rn(gm[a], len);
#pragma unroll
                for (int j = 0; j < 3; ++j) n[j] = (P.R[j] * gm[0] + P.R[3 + j] * gm[1]) + P.R[6 + j] * gm[2];   // R^T: sensor frame
            }
            break;
        }
        prev = has;
        if (has) dp = d, gp[0] = g[0], gp[1] = g[1], gp[2] = g[2];
    }
    const size_t at = (size_t)f * R + r;
    range[at] = rg, flag[at] = out;
    normals[3 * at] = n[0], normals[3 * at + 1] = n[1], normals[3 * at + 2] = n[2];
}

inline Tsdf make_tsdf(const void *map, int cap_vox, double voxel, const double *origin) {
    Tsdf M;
    M.base = (unsigned char *)map, M.cap_vox = cap_vox, M.v = (float)voxel;
    M.ox = origin ? origin[0] : 0.0, M.oy = origin ? origin[1] : 0.0, M.oz = origin ? origin[2] : 0.0;
    return M;
}

// the gate and the samples of a ray from the host's doubles; false when they are refused
inline bool make_rays(double min_range, double max_range, double truncation, double step, Rays &R) {
    if (!range_ok(min_range, max_range)) return false;
    if (!(truncation > 0.0 && truncation <= 64.0 && step > 0.0 && (float)step > 0.f && (float)truncation > 0.f)) return false;
    const double n = ceil(truncation / step);
    if (!(n <= (double)MAX_STEPS)) return false;
    R.lo2 = (float)(min_range * min_range), R.hi2 = (float)(max_range * max_range);
    R.tau = (float)truncation, R.h = (float)step, R.n = (int)n;
    return true;
}

inline bool cos_ok(double cos_min) { return cos_min >= 0.0 && cos_min <= 1.0; }

// the carve's constants from the host's arguments; false when they are refused
inline bool make_carve(const Rays &R, double max_range, double step, int weight, double margin, Carve &C) {
    if (!(weight >= 1 && weight <= 65535 && margin >= 0.0 && margin < 1e18 && max_range / step <= 65536.0)) return false;
    C.add = (long long)weight * (long long)rintf(R.tau * FIX_ONE), C.weight = (unsigned)weight, C.margin = (float)margin;
    return true;
}

// the map of an entry point that places points in it
inline bool field_ok(const void *map, int cap_vox, double voxel, const double *origin) {
    return table_ok(map, cap_vox) && voxel_ok(voxel) && origin_ok(origin);
}

// the two fusion operations over a source of F entries: one launch, one lane per row
template <bool PLANE, typename Src>
int integrate_over(const Tsdf &M, const Src &S, int F, const float *normals, const Rays &R, double cos_min, dpm_stream_t stream) {
    return source_launch(S, F, TS_BLOCK, [&](dim3 grid) {
        hipLaunchKernelGGL((ts_integrate_kernel<PLANE, Src>), grid, dim3(TS_BLOCK), 0, (hipStream_t)stream, M, S, normals, R,
                           (float)cos_min);
    });
}

template <typename Src>
int carve_over(const Tsdf &M, const Src &S, int F, const Rays &R, const Carve &C, dpm_stream_t stream) {
    return source_launch(S, F, TS_BLOCK, [&](dim3 grid) {
        hipLaunchKernelGGL(ts_carve_kernel<Src>, grid, dim3(TS_BLOCK), 0, (hipStream_t)stream, M, S, R, C);
    });
}

}  // namespace

extern "C" size_t dpm_tsdf_bytes(int cap_vox) {
    if (!table_ok((const void *)16, cap_vox)) return 0;
    return 256 + (size_t)cap_vox * 20;
}

extern "C" int dpm_tsdf_init(void *map, int cap_vox, dpm_stream_t stream) {
    DPM_CHECK_ARG(table_ok(map, cap_vox));
    const unsigned g = dpm_cdiv(cap_vox, TS_BLOCK);
    hipLaunchKernelGGL(ts_clear_kernel, dim3(g > 8192 ? 8192 : g), dim3(TS_BLOCK), 0, (hipStream_t)stream,
                       make_tsdf(map, cap_vox, 1.0, nullptr));
    return dpm_launch_status();
}

extern "C" int dpm_tsdf_integrate(void *map, int cap_vox, double voxel, const double *origin, const float *xyz,
                                  const int32_t *count, int cap, const double *pose, double min_range, double max_range,
                                  double truncation, double step, dpm_stream_t stream) {
    Rays R;
    DPM_CHECK_ARG(field_ok(map, cap_vox, voxel, origin) && make_rays(min_range, max_range, truncation, step, R));
    const Tsdf M = make_tsdf(map, cap_vox, voxel, origin);
    return integrate_over<false>(M, OneFrame{xyz, count, cap, pose}, 1, nullptr, R, 0.0, stream);
}

extern "C" int dpm_tsdf_integrate_frames(void *map, int cap_vox, double voxel, const double *origin, const float *store,
                                         const int32_t *lengths, int capacity, int P, const int32_t *frames,
                                         const double *poses, int F, double min_range, double max_range, double truncation,
                                         double step, dpm_stream_t stream) {
    Rays R;
    DPM_CHECK_ARG(field_ok(map, cap_vox, voxel, origin) && make_rays(min_range, max_range, truncation, step, R));
    const Tsdf M = make_tsdf(map, cap_vox, voxel, origin);
    return integrate_over<false>(M, StoredFrames{store, lengths, capacity, P, frames, poses}, F, nullptr, R, 0.0, stream);
}

extern "C" int dpm_tsdf_integrate_planes(void *map, int cap_vox, double voxel, const double *origin, const float *xyz,
                                         const float *normals, const int32_t *count, int cap, const double *pose, double min_range,
                                         double max_range, double truncation, double step, double cos_min, dpm_stream_t stream) {
    Rays R;
    DPM_CHECK_ARG(field_ok(map, cap_vox, voxel, origin) && make_rays(min_range, max_range, truncation, step, R));
    DPM_CHECK_ARG(normals && cos_ok(cos_min));
    const Tsdf M = make_tsdf(map, cap_vox, voxel, origin);
    return integrate_over<true>(M, OneFrame{xyz, count, cap, pose}, 1, normals, R, cos_min, stream);
}

extern "C" int dpm_tsdf_integrate_planes_frames(void *map, int cap_vox, double voxel, const double *origin, const float *store,
                                                const float *normals, const int32_t *lengths, int capacity, int P,
                                                const int32_t *frames, const double *poses, int F, double min_range,
                                                double max_range, double truncation, double step, double cos_min,
                                                dpm_stream_t stream) {
    Rays R;
    DPM_CHECK_ARG(field_ok(map, cap_vox, voxel, origin) && make_rays(min_range, max_range, truncation, step, R));
    DPM_CHECK_ARG((F == 0 || normals) && cos_ok(cos_min));   // an empty list may come with null pointers
    const Tsdf M = make_tsdf(map, cap_vox, voxel, origin);
    return integrate_over<true>(M, StoredFrames{store, lengths, capacity, P, frames, poses}, F, normals, R, cos_min, stream);
}

extern "C" int dpm_tsdf_carve(void *map, int cap_vox, double voxel, const double *origin, const float *xyz, const int32_t *count,
                              int cap, const double *pose, double min_range, double max_range, double truncation, double step,
                              int weight, double margin, dpm_stream_t stream) {
    Rays R;
    Carve C;
    DPM_CHECK_ARG(field_ok(map, cap_vox, voxel, origin) && make_rays(min_range, max_range, truncation, step, R) &&
                  make_carve(R, max_range, step, weight, margin, C));
    const Tsdf M = make_tsdf(map, cap_vox, voxel, origin);
    return carve_over(M, OneFrame{xyz, count, cap, pose}, 1, R, C, stream);
}

extern "C" int dpm_tsdf_carve_frames(void *map, int cap_vox, double voxel, const double *origin, const float *store,
                                     const int32_t *lengths, int capacity, int P, const int32_t *frames, const double *poses, int F,
                                     double min_range, double max_range, double truncation, double step, int weight, double margin,
                                     dpm_stream_t stream) {
    Rays R;
    Carve C;
    DPM_CHECK_ARG(field_ok(map, cap_vox, voxel, origin) && make_rays(min_range, max_range, truncation, step, R) &&
                  make_carve(R, max_range, step, weight, margin, C));
    const Tsdf M = make_tsdf(map, cap_vox, voxel, origin);
    return carve_over(M, StoredFrames{store, lengths, capacity, P, frames, poses}, F, R, C, stream);
}

extern "C" int dpm_tsdf_export(const void *map, int cap_vox, unsigned long long *keys, long long *sums, uint32_t *counts,
                               int32_t *count, int max_out, dpm_stream_t stream) {
    DPM_CHECK_ARG(table_ok(map, cap_vox) && count && max_out >= 0);
    DPM_CHECK_ARG(max_out == 0 || (keys && sums && counts));
    hipLaunchKernelGGL(ts_export_kernel, dim3(dpm_cdiv(cap_vox, TS_BLOCK)), dim3(TS_BLOCK), 0, (hipStream_t)stream,
                       make_tsdf(map, cap_vox, 1.0, nullptr), keys, sums, counts, count, max_out);
    return dpm_launch_status();
}

extern "C" int dpm_tsdf_evict(const void *src, void *dst, int cap_vox, double voxel, const double *origin, const double *pose,
                              double radius, int tile_bits, unsigned long long *keys_out, long long *sums_out,
                              uint32_t *counts_out, int32_t *count_out, int max_out, dpm_stream_t stream) {
    DPM_CHECK_ARG(field_ok(src, cap_vox, voxel, origin) && table_ok(dst, cap_vox) && src != dst);
    DPM_CHECK_ARG(pose && radius >= 0.0 && radius < 1e18 && tile_bits >= 3 && tile_bits <= 10 && count_out && max_out >= 0);
    DPM_CHECK_ARG(max_out == 0 || (keys_out && sums_out && counts_out));
    const Tsdf S = make_tsdf(src, cap_vox, voxel, origin), D = make_tsdf(dst, cap_vox, voxel, origin);
    const EvictOut O{keys_out, sums_out, counts_out, count_out, max_out};
    const unsigned g = dpm_cdiv(cap_vox, TS_BLOCK);
    hipLaunchKernelGGL(ts_evict_clear_kernel, dim3(g > 8192 ? 8192 : g), dim3(TS_BLOCK), 0, (hipStream_t)stream, S, D, count_out);
    hipLaunchKernelGGL(ts_evict_kernel, dim3(g), dim3(TS_BLOCK), 0, (hipStream_t)stream, S, D, pose, (float)(radius * radius),
                       tile_bits, O);
    return dpm_launch_status();
}

extern "C" int dpm_tsdf_absorb(void *map, int cap_vox, const unsigned long long *keys, const long long *sums,
                               const uint32_t *counts, int n, dpm_stream_t stream) {
    DPM_CHECK_ARG(table_ok(map, cap_vox) && n >= 0);
    if (n == 0) return DPM_OK;   // nothing to read: the lists may be null
    DPM_CHECK_ARG(keys && sums && counts);
    hipLaunchKernelGGL(ts_absorb_kernel, dim3(dpm_cdiv(n, TS_BLOCK)), dim3(TS_BLOCK), 0, (hipStream_t)stream,
                       make_tsdf(map, cap_vox, 1.0, nullptr), keys, sums, counts, n);
    return dpm_launch_status();
}

// what surface and mesh are given: a table, a voxel size, a qualifying count, a counter and room for max_out >= 0 records
static bool extract_ok(const void *map, int cap_vox, double voxel, int min_count, const int32_t *count, int max_out) {
    return table_ok(map, cap_vox) && voxel_ok(voxel) && min_count >= 1 && count && max_out >= 0;
}

// the owner list of an entry point: nothing (everything is owned), or n sorted tile keys on the device
static bool owners_ok(int tile_bits, const unsigned long long *tiles, int n_tiles) {
    return n_tiles >= 0 && (n_tiles == 0 || (tiles && tile_bits >= 3 && tile_bits <= 10));
}

// both surface entry points; W: the owners of the tiles form, or null
static int surface_launch(const void *map, int cap_vox, double voxel, int min_count, const Owners *W, unsigned long long *keys,
                          int32_t *axes, float *xyz, float *normals, int32_t *count, int max_out, dpm_stream_t stream) {
    DPM_CHECK_ARG(extract_ok(map, cap_vox, voxel, min_count, count, max_out) && (max_out == 0 || (keys && axes && xyz && normals)));
    const Tsdf M = make_tsdf(map, cap_vox, voxel, nullptr);
    const dim3 grid(dpm_cdiv(cap_vox, TS_BLOCK)), block(TS_BLOCK);
    if (W)
        hipLaunchKernelGGL(ts_surface_tiles_kernel, grid, block, 0, (hipStream_t)stream, M, (unsigned)min_count, *W, keys, axes, xyz,
                           normals, count, max_out);
    else
        hipLaunchKernelGGL(ts_surface_kernel, grid, block, 0, (hipStream_t)stream, M, (unsigned)min_count, keys, axes, xyz, normals,
                           count, max_out);
    return dpm_launch_status();
}

extern "C" int dpm_tsdf_surface(const void *map, int cap_vox, double voxel, int min_count, unsigned long long *keys,
                                int32_t *axes, float *xyz, float *normals, int32_t *count, int max_out, dpm_stream_t stream) {
    return surface_launch(map, cap_vox, voxel, min_count, nullptr, keys, axes, xyz, normals, count, max_out, stream);
}

extern "C" int dpm_tsdf_mesh(const void *map, int cap_vox, double voxel, int min_count, unsigned long long *vertex_keys,
                             int32_t *vertex_dirs, float *xyz, int32_t *count, int max_out, dpm_stream_t stream) {
    DPM_CHECK_ARG(extract_ok(map, cap_vox, voxel, min_count, count, max_out) && (max_out == 0 || (vertex_keys && vertex_dirs && xyz)));
    const MeshOut O{vertex_keys, vertex_dirs, xyz, count, max_out};
    hipLaunchKernelGGL(ts_mesh_kernel, dim3(dpm_cdiv(cap_vox, TS_BLOCK)), dim3(TS_BLOCK), 0, (hipStream_t)stream,
                       make_tsdf(map, cap_vox, voxel, nullptr), (unsigned)min_count, O);
    return dpm_launch_status();
}

extern "C" int dpm_tsdf_surface_tiles(const void *map, int cap_vox, double voxel, int min_count, int tile_bits,
                                      const unsigned long long *tiles, int n_tiles, unsigned long long *keys, int32_t *axes,
                                      float *xyz, float *normals, int32_t *count, int max_out, dpm_stream_t stream) {
    DPM_CHECK_ARG(owners_ok(tile_bits, tiles, n_tiles));
    const Owners W{n_tiles ? tiles : nullptr, n_tiles, tile_bits};
    return surface_launch(map, cap_vox, voxel, min_count, &W, keys, axes, xyz, normals, count, max_out, stream);
}

// the indexed mesh's workspace: the mask bytes, a first index per slot, a sum per block of slots
static void mesh_indexed_layout(WsCursor &c, int cap_vox, MeshIdx &X) {
    X.mask = c.take256<unsigned>(dpm_cdiv(cap_vox, 4));
    X.first = c.take256<int32_t>((size_t)cap_vox);
    X.block_first = c.take256<int32_t>(dpm_cdiv(cap_vox, TS_BLOCK));
}

extern "C" size_t dpm_tsdf_mesh_indexed_bytes(int cap_vox) {
    if (!table_ok((const void *)16, cap_vox)) return 0;
    WsCursor c(nullptr);
    MeshIdx X;
    mesh_indexed_layout(c, cap_vox, X);
    return c.bytes();
}

extern "C" int dpm_tsdf_mesh_indexed(const void *map, int cap_vox, double voxel, int min_count, int tile_bits,
                                     const unsigned long long *tiles, int n_tiles, unsigned long long *vertex_keys,
                                     int32_t *vertex_dirs, float *xyz, float *normals, int32_t *faces, int32_t *counts, int max_v,
                                     int max_f, void *workspace, dpm_stream_t stream) {
    DPM_CHECK_ARG(table_ok(map, cap_vox) && voxel_ok(voxel) && min_count >= 1 && counts && workspace);
    DPM_CHECK_ARG(owners_ok(tile_bits, tiles, n_tiles) && max_v >= 0 && max_f >= 0 && max_f <= 0x7FFFFFFF / 3);
    DPM_CHECK_ARG((max_v == 0 || (vertex_keys && vertex_dirs && xyz && normals)) && (max_f == 0 || faces));
    hipStream_t st = (hipStream_t)stream;
    const Tsdf M = make_tsdf(map, cap_vox, voxel, nullptr);
    const Owners W{n_tiles ? tiles : nullptr, n_tiles, tile_bits};
    MeshIdx X{};
    WsCursor c(workspace);
    mesh_indexed_layout(c, cap_vox, X);
    X.counts = counts, X.vkeys = vertex_keys, X.vdirs = vertex_dirs, X.xyz = xyz, X.normals = normals, X.faces = faces;
    X.max_v = max_v, X.max_f = max_f;
    const unsigned g = dpm_cdiv(cap_vox, TS_BLOCK), words = dpm_cdiv(cap_vox, 4), gw = dpm_cdiv(words, TS_BLOCK);
    hipLaunchKernelGGL(ts_mesh_clear_kernel, dim3(gw > 8192 ? 8192 : gw), dim3(TS_BLOCK), 0, st, X, (int)words);
    hipLaunchKernelGGL(ts_mesh_cells_kernel, dim3(g), dim3(TS_BLOCK), 0, st, M, (unsigned)min_count, W, X);
    hipLaunchKernelGGL(ts_mesh_count_kernel, dim3(g), dim3(TS_BLOCK), 0, st, cap_vox, X);
    hipLaunchKernelGGL(ts_mesh_scan_kernel, dim3(1), dim3(SCAN_BLOCK), 0, st, (int)g, (int)dpm_cdiv(g, SCAN_BLOCK), X);
    hipLaunchKernelGGL(ts_mesh_vertices_kernel, dim3(g), dim3(TS_BLOCK), 0, st, M, (unsigned)min_count, X);
    if (max_f > 0)   // a counting call wrote no id
        hipLaunchKernelGGL(ts_mesh_remap_kernel, dim3(dpm_cdiv(3 * (size_t)max_f, TS_BLOCK)), dim3(TS_BLOCK), 0, st, X);
    return dpm_launch_status();
}

extern "C" int dpm_tsdf_sample(const void *map, int cap_vox, double voxel, const double *origin, const float *xyz,
                               const int32_t *count, int cap, const double *pose, int min_count, float *d, float *grad,
                               int32_t *flag, dpm_stream_t stream) {
    DPM_CHECK_ARG(table_ok(map, cap_vox) && voxel_ok(voxel) && origin_ok(origin));
    DPM_CHECK_ARG(count && pose && cap >= 0 && min_count >= 1);
    if (cap == 0) return DPM_OK;   // nothing to read or write: the row pointers may be null
    DPM_CHECK_ARG(xyz && d && grad && flag);
    hipLaunchKernelGGL(ts_sample_kernel, dim3(dpm_cdiv(cap, TS_BLOCK)), dim3(TS_BLOCK), 0, (hipStream_t)stream,
                       make_tsdf(map, cap_vox, voxel, origin), xyz, count, cap, pose, (unsigned)min_count, d, grad, flag);
    return dpm_launch_status();
}

extern "C" size_t dpm_tsdf_register_scratch_bytes(int cap) {
    if (cap < 1) return 0;
    WsCursor c(nullptr);
    GnOneHdr *hdr;
    double *partial;
    gn_one_layout(c, cap, hdr, partial);
    return c.bytes();
}

extern "C" int dpm_tsdf_register(const void *map, int cap_vox, double voxel, const double *origin, double truncation,
                                 int min_count, double grad_min, const float *xyz, const int32_t *count, int cap,
                                 const double *init_pose, const double *stage_max_dist, const int32_t *stage_max_iter,
                                 int n_stages, double kernel_scale, double tol_rot, double tol_trans, double *pose,
                                 float *fitness, float *rmse, int32_t *iterations, int32_t *status, int32_t *debug_flag,
                                 double *debug_system, void *workspace, dpm_stream_t stream) {
    DPM_CHECK_ARG(table_ok(map, cap_vox) && voxel_ok(voxel) && origin_ok(origin));
    DPM_CHECK_ARG(truncation > 0.0 && truncation <= 64.0 && min_count >= 1 && grad_min >= 0.0 && grad_min < 1e18);
    DPM_CHECK_ARG(xyz && count && init_pose && stage_max_dist && stage_max_iter && workspace && cap >= 1);
    DPM_CHECK_ARG(pose && fitness && rmse && iterations && status && pose != init_pose);
    DPM_CHECK_ARG(n_stages >= 1 && n_stages <= 16 && tol_rot >= 0.0 && tol_trans >= 0.0 && kernel_scale >= 0.0 && kernel_scale < 1e18);
    for (int s = 0; s < n_stages; ++s)   // beyond the clamp the field is flat
        DPM_CHECK_ARG(stage_max_dist[s] > 0.0 && stage_max_dist[s] <= truncation && stage_max_iter[s] >= 0);
    hipStream_t st = (hipStream_t)stream;
    TsRegArgs A{};
    A.M = make_tsdf(map, cap_vox, voxel, origin);
    A.xyz = xyz, A.count = count, A.cap = cap, A.min_count = (unsigned)min_count, A.grad_min2 = (float)(grad_min * grad_min);
    WsCursor c(workspace);
    gn_one_layout(c, cap, A.hdr, A.partial);
    A.pose = pose, A.fitness = fitness, A.rmse = rmse, A.iterations = iterations, A.status = status;
    A.dbg_flag = debug_flag, A.dbg_system = debug_system;
    const double kappa = kernel_scale * kernel_scale;
    const GnOne G{A.hdr, A.partial, pose, fitness, rmse, iterations, status, debug_system, count, cap, A.M.ox, A.M.oy, A.M.oz};
    return gn_one_run(G, init_pose, stage_max_iter, n_stages, tol_rot, tol_trans, st, [&](int s) {
        hipLaunchKernelGGL(ts_reg_accumulate_kernel, dim3(dpm_cdiv(cap, TS_BLOCK)), dim3(TS_BLOCK), 0, st, A,
                           (float)stage_max_dist[s], kappa);
    });
}

// a block set: the caller's buffer of dpm_tsdf_blocks_bytes(cap_blocks) bytes, under the table's own limits
extern "C" size_t dpm_tsdf_blocks_bytes(int cap_blocks) {
    if (!table_ok((const void *)16, cap_blocks)) return 0;
    return 256 + (size_t)cap_blocks * 8;
}

extern "C" int dpm_tsdf_blocks(const void *map, int cap_vox, int min_count, void *blocks, int cap_blocks, dpm_stream_t stream) {
    DPM_CHECK_ARG(table_ok(map, cap_vox) && table_ok(blocks, cap_blocks) && min_count >= 1);
    const BlockSet B{(unsigned char *)blocks, cap_blocks};
    const unsigned g = dpm_cdiv(cap_blocks, TS_BLOCK);
    hipLaunchKernelGGL(ts_blocks_clear_kernel, dim3(g > 8192 ? 8192 : g), dim3(TS_BLOCK), 0, (hipStream_t)stream, B);
    hipLaunchKernelGGL(ts_blocks_kernel, dim3(dpm_cdiv(cap_vox, TS_BLOCK)), dim3(TS_BLOCK), 0, (hipStream_t)stream,
                       make_tsdf(map, cap_vox, 1.0, nullptr), (unsigned)min_count, B);
    return dpm_launch_status();
}

extern "C" int dpm_tsdf_raycast(const void *map, int cap_vox, double voxel, const double *origin, const void *blocks,
                                int cap_blocks, const double *poses, int F, const float *dirs, int R, double min_range,
                                double max_range, double step, int min_count, float *range, float *normals, int32_t *flag,
                                dpm_stream_t stream) {
    DPM_CHECK_ARG(table_ok(map, cap_vox) && voxel_ok(voxel) && origin_ok(origin));
    DPM_CHECK_ARG(!blocks || table_ok(blocks, cap_blocks));
    DPM_CHECK_ARG(step > 0.0 && range_ok(min_range, max_range));
    const double samples = floor((max_range - min_range) / step) + 1.0;
    DPM_CHECK_ARG(samples <= 65536.0 && min_count >= 1 && F >= 0 && F <= 65535 && R >= 0);
    if (F == 0 || R == 0) return DPM_OK;   // nothing to read or write: the pointers may be null
    DPM_CHECK_ARG(poses && dirs && range && normals && flag);
    const Tsdf M = make_tsdf(map, cap_vox, voxel, origin);
    const BlockSet B{(unsigned char *)blocks, blocks ? cap_blocks : 0};
    const Cast C{(float)min_range, (float)step, (int)samples, (unsigned)min_count};
    const dim3 grid(dpm_cdiv(R, TS_BLOCK), F);
    if (blocks)
        hipLaunchKernelGGL(ts_raycast_kernel<true>, grid, dim3(TS_BLOCK), 0, (hipStream_t)stream, M, B, poses, dirs, R, C, range,
                           normals, flag);
    else
        hipLaunchKernelGGL(ts_raycast_kernel<false>, grid, dim3(TS_BLOCK), 0, (hipStream_t)stream, M, B, poses, dirs, R, C, range,
                           normals, flag);
    return dpm_launch_status();
}
