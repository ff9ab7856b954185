// The rolling local map of the geometric odometry (deeppointmap_amd/odometry.py) and the registration of a scan against it.
// The reference has no counterpart: it estimates poses with its learned pipeline only.
//
// Map: an open-addressing table of cap_vox slots (a power of two, linear probing, empty key ~0) keyed by the voxel
// coordinate floor(p / v) per axis, 3 x 21 bits biased by 2^20 as in csrc/voxel_map.hip.  p is the fp32 point in the MAP
// frame: world minus a float64 `origin` fixed when the map is made; a pose enters as R -> (float)R and
// t -> (float)(t - origin), the difference formed in fp64 and rounded once (csrc/map_eval.hip's shift).  A voxel has
// S = s^3 sub-cells, s in {1, 2, 3}; sub-cell (a, b, c) -> (c * s + b) * s + a.  Per axis, in fp32:
//     f = p / v (correctly rounded division),  voxel = floor(f),  sub = min((int)((f - voxel) * s), s - 1).
// Each sub-cell holds at most one point: an owner word (stamp << 32) | row and a float4 (x, y, z, 0).
//
// RULE: a sub-cell belongs to the point with the smallest owner word ever offered to it.  The stamp counts frames, so an
// older frame is never displaced, and within a frame the smaller row (the frame's `idx`, the ORIGINAL row number, which
// survives sampling and shuffles) wins: "at most S points a voxel, first come first kept" with "first" defined.  Only
// integer atomics: the content reachable by key is a function of the inserted points alone.  Slot positions are not (two
// voxels racing for one probe chain), and nothing reads them.
//
//   claim    per valid row: range gate on the SENSOR-frame point, r2 = (x*x + y*y) + z*z, kept when
//            (float)(min_range^2) <= r2 <= (float)(max_range^2) (a NaN fails);  transform
//            q = fma(R2, z, fma(R1, y, R0 * x)) + t, the arithmetic of the registration search;  a coordinate outside the
//            21 bits is dropped and counted (header word 1);  find or claim the voxel (atomicCAS on the key);  atomicMin on
//            the sub-cell's owner word.  No free slot within cap_vox probes: header word 0 (overflow) counts the point,
//            and the map is defined only while that word is 0.
//   commit   the same arithmetic (the same bits), a read-only probe, and the coordinates written where the owner word is
//            the point's own.  A launch boundary lies between the atomics and these plain stores.
//   prune    the other half of the double buffer is cleared, then every voxel whose centre c = ((float)voxel + 0.5f) * v
//            has (dx*dx + dy*dy) + dz*dz <= (float)(radius^2) from the pose's translation is claimed there and its S
//            sub-cells are copied.  A voxel is one key: the copy has one writer.
//   export   (key, sub-cell, owner, xyz) of every occupied sub-cell in arrival order + their number; Python sorts.
//   frames   (dpm_local_map_insert_frames) claim and commit over a LIST of stored frames in two launches, blockIdx.y the list
//            entry, x over the P columns of a channel-major store (capacity,3,P): entry f offers column i of row frames[f]
//            under poses[f] by the claim's rule, owner word (stamps[f] << 32) | i.  With a centre, a row is offered only when
//            its voxel passes prune's test around it: the content is that of the inserts, in any order, followed by the
//            prune, and the voxels the prune would drop never ask for a slot.  `outside` counts before the filter, `overflow`
//            after it.  One frame and the list are the two sources of csrc/scan_source.h; what claim and commit do with a
//            row is written once, insert_row<COMMIT>, under lm_insert_kernel and lm_insert_frames_kernel.
//
// Registration: per iteration two launches, no host synchronisation, capturable on one stream.
//   accumulate: four lanes per query, queries in ROW order.  The query is moved by the device pose rounded to fp32; lane l
//               of the quad probes neighbours n = l, l + 4, ... of the 27 voxels around it (n = ((dz+1) * 3 + (dy+1)) * 3 +
//               (dx+1)) read-only and scans their occupied sub-cells; the winner is the smallest 64-bit key
//               (distance bits, n * 32 + sub-cell): ties are broken by geometry alone.  A hit needs d2 <= (float)(max_dist^2);
//               max_dist <= v (checked on the host), so in exact arithmetic no nearer point lies outside the 27 voxels.
//               Lane 0 adds the point-to-point rows, weighted w = (kappa / (kappa + e.e))^2 (Geman-McClure, kappa =
//               kernel_scale^2, 0 = unweighted), to the 29 fp64 sums of csrc/gn_solve.h: H and g weighted, the match count
//               and the squared residuals not.  One partial per block.
//   solve:      (csrc/gn_one.h, the driver shared with csrc/tsdf_map.hip) one wave adds the partials in block order; the step
//               is taken on the pose in the map frame (where the rows were formed) and shifted back; a step not taken leaves
//               the pose's bytes alone.
// The search pose is csrc/gn_solve.h's; the rows, the reduction, the solve and the start values are shared with csrc/icp.hip there.
//
// Voxel planes (dpm_local_map_planes): a cache derived from the map, one float4 (normal, w) and one count per SLOT of the
// current half, in caller-owned buffers.  One launch, four lanes a slot.  The centre of a held voxel is
// c = ((float)index + 0.5f) * v per axis; every occupied sub-cell point p of the 27 voxels around it with d = p - c (fp32) and
// (dx*dx + dy*dy) + dz*dz <= (float)(plane_radius^2) is a member (plane_radius <= 1.5 v: the ball lies inside the 27 voxels).
// Lane l adds the ten cumulants of d (n, 3 first, 6 second moments) in fp64 over the neighbours n = l, l + 4, ... ascending,
// sub-cells ascending; the four lanes are added as (l0 + l1) + (l2 + l3).  So a voxel's plane is a function of the map's
// content alone.  Lane 0 forms the scatter matrix n * S_ab - S_a * S_b (the covariance times n^2: exactly zero where the
// points' coordinates are, which a quotient by n would not keep), runs the cyclic Jacobi of csrc/sym3_jacobi.h in
// fp64 and orders the eigenvalues ascending, the smaller axis first among equals.  The normal is
// the unit eigenvector of the smallest, rounded to fp32, its sign such that the component of largest magnitude (of the fp32
// values; the first axis among equals) is positive; w = (float)(max(l0, 0) / l1).  Fewer than 3 members, or a line, l1 <= 1e-8 l2
// (which includes l1 <= 0; see LINE_RATIO): (0, 0, 0, -1).  An empty slot: (0, 0, 0, -1) and count 0.
//
// Plane rows (dpm_local_map_register_planes): lm_accumulate_kernel<true>.  Search, tie-break and key as above; the matched
// point's voxel (its slot) gives a row only when counts >= min_points and 0 <= w <= (float)max_ratio:
// e = (nx*ex + ny*ey) + nz*ez, J = (p x n, n) -- gn_plane_row, the batched ICP's too -- weighted (kappa / (kappa + e*e))^2.
// A match whose voxel has no such plane contributes nothing and is not counted.
#include "cell_grid.h"
#include "gn_one.h"
#include "scan_source.h"
#include "sym3_jacobi.h"
#include "voxel_hash.h"

namespace {

constexpr int LM_BLOCK = 256;

struct MapHdr {   // 256 bytes
    unsigned overflow, outside, pad[62];
};

struct Map {
    unsigned char *base;
    int cap_vox, s, S, half;
    float v;
    double ox, oy, oz;
    __host__ __device__ size_t half_bytes() const { return (size_t)cap_vox * 8 + (size_t)cap_vox * S * 24; }
    __host__ __device__ unsigned long long *keys(int h) const { return (unsigned long long *)(base + 256 + (size_t)h * half_bytes()); }
    __host__ __device__ unsigned long long *owner(int h) const { return keys(h) + cap_vox; }
    __host__ __device__ float4 *pts(int h) const { return (float4 *)(owner(h) + (size_t)cap_vox * S); }
    __host__ __device__ MapHdr *hdr() const { return (MapHdr *)base; }
};

// Lane ql of a quad visits the neighbours n = ql, ql + 4, ... (n = ((dz+1) * 3 + (dy+1)) * 3 + (dx+1)) of the 27 voxels around
// (vx, vy, vz) and offers every occupied sub-cell, ascending, to f(n, slot, c, point).  own_slot >= 0: the slot of n = 13, if known.
template <typename Fn>
__device__ __forceinline__ void quad_visit27(const unsigned long long *keys, const unsigned long long *owner, const float4 *pts,
                                             int cap_vox, int S, int vx, int vy, int vz, int ql, int own_slot, Fn f) {
    for (int n = ql; n < 27; n += 4) {
        const int x = vx + n % 3 - 1, y = vy + (n / 3) % 3 - 1, z = vz + n / 9 - 1;
        if ((unsigned)x > 0x1FFFFFu || (unsigned)y > 0x1FFFFFu || (unsigned)z > 0x1FFFFFu) continue;
        const int slot = n == 13 && own_slot >= 0 ? own_slot : find_slot(keys, cap_vox, pack_key(x, y, z));
        if (slot < 0) continue;
        for (int c = 0; c < S; ++c) {
            if (owner[(size_t)slot * S + c] == EMPTY) continue;
            f(n, slot, c, pts[(size_t)slot * S + c]);
        }
    }
}

__global__ __launch_bounds__(LM_BLOCK) void lm_clear_kernel(Map M, int h, bool header) {
    const size_t tid = (size_t)blockIdx.x * LM_BLOCK + threadIdx.x, stride = (size_t)gridDim.x * LM_BLOCK;
    if (header && tid < 64) ((unsigned *)M.base)[tid] = 0u;
    unsigned long long *w = M.keys(h);   // the keys and the owner words are one run of cap_vox * (1 + S) words of ~0
    const size_t n = (size_t)M.cap_vox * (size_t)(1 + M.S);
    for (size_t i = tid; i < n; i += stride) w[i] = EMPTY;
}

// prune's test: the centre of voxel `key` lies within sqrt(r2) of the pose's map-frame translation
__device__ __forceinline__ bool voxel_within(const Map &M, unsigned long long key, const double *pose, float r2) {
    const float tx = (float)(pose[3] - M.ox), ty = (float)(pose[7] - M.oy), tz = (float)(pose[11] - M.oz);
    float c[3];
    voxel_centre(key, M.v, c);
    const float dx = c[0] - tx, dy = c[1] - ty, dz = c[2] - tz;
    return (dx * dx + dy * dy) + dz * dz <= r2;
}

struct Frame {   // one frame as the insert and accumulate kernels take it (their code depends on this layout)
    const float *xyz;        // (cap,3)
    const int32_t *idx;      // (cap,) original row numbers
    const int32_t *count;    // (1,)
    int cap;
};

// what claim and commit compute alike for the sensor-frame point (x, y, z); false when it offers nothing
__device__ __forceinline__ bool row_cell(const Map &M, const GnPose32 &P, float x, float y, float z, float lo2, float hi2,
                                         unsigned long long &key, int &sub, float q[3], bool &outside) {
    const float r2 = (x * x + y * y) + z * z;
    outside = false;
    if (!(r2 >= lo2 && r2 <= hi2)) return false;
    gn_xform(P, x, y, z, q);
    int vx, vy, vz, sx, sy, sz;
    if (!(axis_cell(q[0], M.v, M.s, vx, sx) & axis_cell(q[1], M.v, M.s, vy, sy) & axis_cell(q[2], M.v, M.s, vz, sz))) {
        outside = true;
        return false;
    }
    key = pack_key(vx, vy, vz), sub = (sz * M.s + sy) * M.s + sx;
    return true;
}

// What the local map adds to a source of rows (csrc/scan_source.h): the owner word of row i and the filter of a rebuild.
// One frame: stamped `stamp`, the low half its ORIGINAL row number idx[i]; no filter, so that test folds away.
struct FrameOwner {
    const int32_t *idx;   // (cap,)
    unsigned stamp;
    __device__ __forceinline__ unsigned long long word(int i) const { return ((unsigned long long)stamp << 32) | (unsigned)idx[i]; }
    __device__ __forceinline__ const double *centre() const { return nullptr; }
};

// Entry f of a list: stamped stamps[f], the low half the column i; with a centre, a row is offered only when its voxel passes
// prune's test around it.
struct StoredRows {
    StoredFrames rows;
    const uint32_t *stamps;    // (F,)
    const double *centre_;     // (16,) or NULL: no filter
    __device__ __forceinline__ unsigned long long word(int i) const {
        return ((unsigned long long)stamps[blockIdx.y] << 32) | (unsigned)i;
    }
    __device__ __forceinline__ const double *centre() const { return centre_; }
};

// Claim (!COMMIT) or commit of row i of `rows`, opened as o, owned as W says: what both insert kernels do with a row.
template <bool COMMIT, typename Src, typename Owner>
__device__ __forceinline__ void insert_row(const Map &M, const Src &rows, const SourceRows &o, int i, const Owner &W, float lo2,
                                           float hi2, float r2) {
    const GnPose32 P = gn_load_pose(o.pose, M.ox, M.oy, M.oz);
    float x, y, z;
    rows.point(o, i, x, y, z);
    unsigned long long key;
    int sub;
    float q[3];
    bool outside;
    if (!row_cell(M, P, x, y, z, lo2, hi2, key, sub, q, outside)) {
        if (!COMMIT && outside) atomicAdd(&M.hdr()->outside, 1u);
        return;
    }
    if (W.centre() && !voxel_within(M, key, W.centre(), r2)) return;   // `outside` counts before the filter, `overflow` after it
    const unsigned long long word = W.word(i);
    if (!COMMIT) {
        const int slot = claim_slot(M.keys(M.half), M.cap_vox, key);
        if (slot < 0) {
            atomicAdd(&M.hdr()->overflow, 1u);
            return;
        }
        atomicMin(&M.owner(M.half)[(size_t)slot * M.S + sub], word);
    } else {
        const int slot = find_slot(M.keys(M.half), M.cap_vox, key);
        if (slot < 0) return;   // counted as overflow by claim
        const size_t c = (size_t)slot * M.S + sub;
        if (M.owner(M.half)[c] == word) M.pts(M.half)[c] = make_float4(q[0], q[1], q[2], 0.f);
    }
}

// One frame.  The kernel's arguments are the parent form's, in its order, and not the source as one struct: with the pose and the
// stamp inside the source the claim was slower on small frames (profiles/scan_source_isa.md).  The rows are read through OneFrame.
template <bool COMMIT>
__global__ __launch_bounds__(LM_BLOCK) void lm_insert_kernel(Map M, Frame F, const double *pose, unsigned stamp, float lo2,
                                                             float hi2) {
    const OneFrame S{F.xyz, F.count, F.cap, pose};
    SourceRows o;
    const int i = blockIdx.x * LM_BLOCK + threadIdx.x;
    if (!S.open(o) || i >= o.n) return;
    insert_row<COMMIT>(M, S, o, i, FrameOwner{F.idx, stamp}, lo2, hi2, 0.f);
}

// A list of stored frames.  Hundreds of entries offer points to the same sub-cells; reading the owner word first and skipping an
// offer it already beats gave the same bytes and no time (profiles/local_map_rebuild_bench.md), so every offer is one atomicMin.
template <bool COMMIT>
__global__ __launch_bounds__(LM_BLOCK) void lm_insert_frames_kernel(Map M, StoredRows L, float lo2, float hi2, float r2) {
    SourceRows o;
    const int i = blockIdx.x * LM_BLOCK + threadIdx.x;
    if (!L.rows.open(o) || i >= o.n) return;   // one test, not two returns: the form that was timed (profiles/scan_source_isa.md)
    insert_row<COMMIT>(M, L.rows, o, i, L, lo2, hi2, r2);
}

// one thread per slot of the current half; survivors move to the other half (cleared before this launch)
__global__ __launch_bounds__(LM_BLOCK) void lm_prune_kernel(Map M, const double *pose, float r2) {
    const int slot = blockIdx.x * LM_BLOCK + threadIdx.x;
    if (slot >= M.cap_vox) return;
    const unsigned long long key = M.keys(M.half)[slot];
    if (key == EMPTY) return;
    if (!voxel_within(M, key, pose, r2)) return;
    const int to = claim_slot(M.keys(1 - M.half), M.cap_vox, key);   // never full: no more keys than the old half held
    if (to < 0) {
        atomicAdd(&M.hdr()->overflow, 1u);
        return;
    }
    const unsigned long long *ow = M.owner(M.half) + (size_t)slot * M.S;
    const float4 *pt = M.pts(M.half) + (size_t)slot * M.S;
    unsigned long long *ow2 = M.owner(1 - M.half) + (size_t)to * M.S;
    float4 *pt2 = M.pts(1 - M.half) + (size_t)to * M.S;
    for (int c = 0; c < M.S; ++c) {
        const unsigned long long o = ow[c];
        if (o == EMPTY) continue;
        ow2[c] = o, pt2[c] = pt[c];
    }
}

__global__ __launch_bounds__(LM_BLOCK) void lm_export_kernel(Map M, unsigned long long *keys, int32_t *sub,
                                                             unsigned long long *owner, float *xyz, int32_t *count,
                                                             int max_out) {
    const size_t n = (size_t)M.cap_vox * M.S;
    for (size_t c = (size_t)blockIdx.x * LM_BLOCK + threadIdx.x; c < n; c += (size_t)gridDim.x * LM_BLOCK) {
        const unsigned long long o = M.owner(M.half)[c];
        if (o == EMPTY) continue;
        const unsigned long long key = M.keys(M.half)[c / M.S];
        if (key == EMPTY) continue;
        const int pos = atomicAdd(count, 1);
        if (pos < 0 || pos >= max_out) continue;
        const float4 p = M.pts(M.half)[c];
        keys[pos] = key, sub[pos] = (int32_t)(c % M.S), owner[pos] = o;
        xyz[3 * (size_t)pos] = p.x, xyz[3 * (size_t)pos + 1] = p.y, xyz[3 * (size_t)pos + 2] = p.z;
    }
}

// ------------------------------------------------------------------------------------------------------------- voxel planes
// A point set whose middle eigenvalue is at most this fraction of its largest is a LINE: it has no plane.  In exact arithmetic
// that is l1 = 0 (a ring of a spinning sensor on a flat wall), but the map's coordinates are fp32: a line a metre long comes
// back 2^-24 |p| thick, l1 / l2 near 1e-11 at |p| = 50 m instead of 0, and the eigenvector of l0 is then whatever that rounding
// left.  1e-8 is a thickness of 1e-4 of the length: 16 times the rounding of a coordinate at 100 m over one metre, and a
// hundredth of what a sensor with 1 cm of range noise draws.
constexpr double LINE_RATIO = 1e-8;

// four lanes per slot of the current half, 64 slots a block
__global__ __launch_bounds__(LM_BLOCK) void lm_planes_kernel(Map M, float r2, float4 *planes, int32_t *counts) {
    const int slot = blockIdx.x * (LM_BLOCK / 4) + (threadIdx.x >> 2), ql = threadIdx.x & 3;   // uniform inside a quad
    if (slot >= M.cap_vox) return;
    const unsigned long long *keys = M.keys(M.half), *owner = M.owner(M.half);
    const float4 *pts = M.pts(M.half);
    const unsigned long long key = keys[slot];
    if (key == EMPTY) {
        if (ql == 0) planes[slot] = make_float4(0.f, 0.f, 0.f, -1.f), counts[slot] = 0;
        return;
    }
    float ctr[3];
    voxel_centre(key, M.v, ctr);
    double m[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};  // n, x, y, z, xx, xy, xz, yy, yz, zz
    quad_visit27(keys, owner, pts, M.cap_vox, M.S, key_axis(key, 0), key_axis(key, 1), key_axis(key, 2), ql, slot,
                 [&](int, int, int, const float4 &t) {
        const float dx = t.x - ctr[0], dy = t.y - ctr[1], dz = t.z - ctr[2];
        if (!((dx * dx + dy * dy) + dz * dz <= r2)) return;
        const double X = dx, Y = dy, Z = dz;
        m[0] += 1.0, m[1] += X, m[2] += Y, m[3] += Z;
        m[4] += X * X, m[5] += X * Y, m[6] += X * Z, m[7] += Y * Y, m[8] += Y * Z, m[9] += Z * Z;
    });
#pragma unroll
    for (int k = 0; k < 10; ++k) {   // (l0 + l1) + (l2 + l3)
        m[k] += __shfl_xor(m[k], 1, 64);
        m[k] += __shfl_xor(m[k], 2, 64);
    }
    if (ql != 0) return;
    float4 out = make_float4(0.f, 0.f, 0.f, -1.f);
    const double n = m[0];
    if (n >= 3.0) {
        double A[3][3] = {{n * m[4] - m[1] * m[1], n * m[5] - m[1] * m[2], n * m[6] - m[1] * m[3]},
                          {0, n * m[7] - m[2] * m[2], n * m[8] - m[2] * m[3]},
                          {0, 0, n * m[9] - m[3] * m[3]}};
        A[1][0] = A[0][1], A[2][0] = A[0][2], A[2][1] = A[1][2];
        double V[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
        sym3_jacobi(A, V);
        // ascending, the smaller axis first among equals: e0 the smallest, e1 the smaller of the other two
        int e0 = 0;
        if (A[1][1] < A[e0][e0]) e0 = 1;
        if (A[2][2] < A[e0][e0]) e0 = 2;
        const int ea = e0 == 0 ? 1 : 0, eb = e0 == 2 ? 1 : 2;
        const int e1 = A[eb][eb] < A[ea][ea] ? eb : ea;
        const double l0 = A[e0][e0], l1 = A[e1][e1], l2 = A[3 - e0 - e1][3 - e0 - e1];
        const double vx_ = V[0][e0], vy_ = V[1][e0], vz_ = V[2][e0], nr = sqrt(vx_ * vx_ + vy_ * vy_ + vz_ * vz_);
        if (l1 > LINE_RATIO * l2 && nr > 0.0) {   // also false for l1 <= 0 and for a NaN
            float nx = (float)(vx_ / nr), ny = (float)(vy_ / nr), nz = (float)(vz_ / nr);
            const float ax = fabsf(nx), ay = fabsf(ny), az = fabsf(nz);
            const float lead = (ax >= ay && ax >= az) ? nx : (ay >= az ? ny : nz);
            const float sg = lead < 0.f ? -1.f : 1.f;
            out = make_float4(sg * nx + 0.f, sg * ny + 0.f, sg * nz + 0.f, (float)((l0 > 0.0 ? l0 : 0.0) / l1));   // + 0: no -0
        }
    }
    planes[slot] = out, counts[slot] = (int32_t)n;
}

// ------------------------------------------------------------------------------------------------------------ registration
struct RegArgs {   // the accumulate kernels' arguments; hdr and partial are csrc/gn_one.h's
    Map M;
    Frame F;
    GnOneHdr *hdr;
    double *partial;
    double *pose;
    float *fitness, *rmse;
    int32_t *iterations, *status;
    long long *dbg_key;     // (cap,) or NULL
    int32_t *dbg_sub;       // (cap,) or NULL
    double *dbg_system;     // (GN_NSUM,) or NULL
};

// the plane cache of the current half and the gate a voxel's plane passes to give a row (all unused when !PLANE)
struct PlaneArgs {
    const float4 *planes;
    const int32_t *counts;
    int min_points;
    float max_ratio;
};

template <bool PLANE>
__global__ __launch_bounds__(LM_BLOCK) void lm_accumulate_kernel(RegArgs A, float r2, double kappa, PlaneArgs PA) {
    if (A.hdr->done) return;
    const Map &M = A.M;
    const int blk = blockIdx.x, n1 = A.hdr->n1, cap = A.F.cap;
    const GnPose32 P = gn_load_pose(A.pose, M.ox, M.oy, M.oz);
    const unsigned long long *keys = M.keys(M.half), *owner = M.owner(M.half);
    const float4 *pts = M.pts(M.half);
    const int quad = threadIdx.x >> 2, ql = threadIdx.x & 3;
    double s[GN_NSUM];
#pragma unroll
    for (int k = 0; k < GN_NSUM; ++k) s[k] = 0.0;
    for (int j = 0; j < 4; ++j) {
        const int i = blk * 256 + j * 64 + quad;   // uniform inside a quad
        if (i >= n1) {
            if (i < cap && ql == 0) {
                if (A.dbg_key) A.dbg_key[i] = -1;
                if (A.dbg_sub) A.dbg_sub[i] = -1;
            }
            continue;
        }
        float q[3];
        gn_xform(P, A.F.xyz[3 * (size_t)i], A.F.xyz[3 * (size_t)i + 1], A.F.xyz[3 * (size_t)i + 2], q);
        int vx, vy, vz, sx, sy, sz;
        const bool inside = axis_cell(q[0], M.v, M.s, vx, sx) & axis_cell(q[1], M.v, M.s, vy, sy) & axis_cell(q[2], M.v, M.s, vz, sz);
        unsigned long long best = ~0ull;
        int best_slot = -1;
        if (inside)
            quad_visit27(keys, owner, pts, M.cap_vox, M.S, vx, vy, vz, ql, -1, [&](int n, int slot, int c, const float4 &t) {
                const float dx = q[0] - t.x, dy = q[1] - t.y, dz = q[2] - t.z;
                const unsigned long long key =
                    ((unsigned long long)__float_as_uint((dx * dx + dy * dy) + dz * dz) << 32) | (unsigned)(n * 32 + c);
                if (key < best) best = key, best_slot = slot;
            });
        const unsigned long long mine = best;
        best = quad_min_key(best);
        bool hit = best != ~0ull &&__uint_as_float((unsigned)(best >> 32)) <= r2;   // a NaN distance is no hit
        // the winner's slot, from the lane that found it (keys of different lanes differ in n)
        int win_slot = mine == best ? best_slot : -1;
        win_slot = max(win_slot, __shfl_xor(win_slot, 1, 64));
        win_slot = max(win_slot, __shfl_xor(win_slot, 2, 64));
        if (ql != 0) continue;
        const int c = (int)((unsigned)best & 31u);
        float4 pl = make_float4(0.f, 0.f, 0.f, -1.f);
        if (PLANE && hit) {   // the matched point's voxel gives a row only with a plane that passes the gate
            pl = PA.planes[win_slot];
            hit = PA.counts[win_slot] >= PA.min_points && pl.w >= 0.f && pl.w <= PA.max_ratio;
        }
        if (A.dbg_key) A.dbg_key[i] = hit ? (long long)keys[win_slot] : -1;
        if (A.dbg_sub) A.dbg_sub[i] = hit ? c : -1;
        if (!hit) continue;
        const float4 t = pts[(size_t)win_slot * M.S + c];
        const double p[3] = {q[0], q[1], q[2]};
        const double e[3] = {p[0] - (double)t.x, p[1] - (double)t.y, p[2] - (double)t.z};
        s[27] += 1.0;
        if (PLANE) {
            const double n[3] = {pl.x, pl.y, pl.z};
            gn_plane_row(s, p, n, e, kappa);
        } else {
            gn_point_rows(s, p, e, gn_weight(kappa, (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]));
        }
    }
    // gn_block_reduce written out: through it the point-row kernel timed 3 to 4 % slower (profiles/gn_shared_isa.md)
    __shared__ double sred[4][GN_NSUM];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < GN_NSUM; ++k) {
        double v = s[k];
#pragma unroll
        for (int off = 32; off >= 4; off >>= 1) v += __shfl_xor(v, off, 64);   // lanes 1..3 of a quad hold zeros
        if (lane == 0) sred[wv][k] = v;
    }
    __syncthreads();
    if (threadIdx.x < GN_NSUM)
        A.partial[(size_t)blk * GN_NSUM_PAD + threadIdx.x] =
            (sred[0][threadIdx.x] + sred[1][threadIdx.x]) + (sred[2][threadIdx.x] + sred[3][threadIdx.x]);
}

inline unsigned grid_for(size_t items) {
    const size_t b = (items + LM_BLOCK - 1) / LM_BLOCK;
    return (unsigned)(b < 1 ? 1 : b > 8192 ? 8192 : b);
}

inline bool map_ok(const void *map, int cap_vox, int subdiv) { return table_ok(map, cap_vox) && subdiv >= 1 && subdiv <= 3; }

inline Map make_map(void *map, int cap_vox, int subdiv, int half, double voxel, const double *origin) {
    Map M;
    M.base = (unsigned char *)map, M.cap_vox = cap_vox, M.s = subdiv, M.S = subdiv * subdiv * subdiv, M.half = half;
    M.v = (float)voxel;
    M.ox = origin ? origin[0] : 0.0, M.oy = origin ? origin[1] : 0.0, M.oz = origin ? origin[2] : 0.0;
    return M;
}

inline bool geometry_ok(int half, double voxel, const double *origin) {
    return (half == 0 || half == 1) && voxel_ok(voxel) && origin_ok(origin);
}

}  // namespace

extern "C" size_t dpm_local_map_bytes(int cap_vox, int subdiv) {
    if (!map_ok((const void *)16, cap_vox, subdiv)) return 0;
    return 256 + 2 * make_map(nullptr, cap_vox, subdiv, 0, 1.0, nullptr).half_bytes();
}

extern "C" int dpm_local_map_init(void *map, int cap_vox, int subdiv, dpm_stream_t stream) {
    DPM_CHECK_ARG(map_ok(map, cap_vox, subdiv));
    const Map M = make_map(map, cap_vox, subdiv, 0, 1.0, nullptr);
    const unsigned g = grid_for((size_t)cap_vox * (size_t)(1 + M.S));
    hipLaunchKernelGGL(lm_clear_kernel, dim3(g), dim3(LM_BLOCK), 0, (hipStream_t)stream, M, 0, true);
    hipLaunchKernelGGL(lm_clear_kernel, dim3(g), dim3(LM_BLOCK), 0, (hipStream_t)stream, M, 1, false);
    return dpm_launch_status();
}

extern "C" int dpm_local_map_insert(void *map, int cap_vox, int subdiv, int half, double voxel, const double *origin,
                                    const float *xyz, const int32_t *idx, const int32_t *count, int cap,
                                    const double *pose, unsigned stamp, double min_range, double max_range,
                                    dpm_stream_t stream) {
    DPM_CHECK_ARG(map_ok(map, cap_vox, subdiv) && geometry_ok(half, voxel, origin));
    DPM_CHECK_ARG(idx && stamp < 0xFFFFFFFFu && range_ok(min_range, max_range));
    const Map M = make_map(map, cap_vox, subdiv, half, voxel, origin);
    const Frame F{xyz, idx, count, cap};
    const float lo2 = (float)(min_range * min_range), hi2 = (float)(max_range * max_range);
    return source_launch(OneFrame{xyz, count, cap, pose}, 1, LM_BLOCK, [&](dim3 grid) {
        hipLaunchKernelGGL(lm_insert_kernel<false>, grid, dim3(LM_BLOCK), 0, (hipStream_t)stream, M, F, pose, stamp, lo2, hi2);
        hipLaunchKernelGGL(lm_insert_kernel<true>, grid, dim3(LM_BLOCK), 0, (hipStream_t)stream, M, F, pose, stamp, lo2, hi2);
    });
}

extern "C" int dpm_local_map_prune(void *map, int cap_vox, int subdiv, int half, double voxel, const double *origin,
                                   const double *pose, double radius, dpm_stream_t stream) {
    DPM_CHECK_ARG(map_ok(map, cap_vox, subdiv) && geometry_ok(half, voxel, origin));
    DPM_CHECK_ARG(pose && radius >= 0.0 && radius < 1e18);
    const Map M = make_map(map, cap_vox, subdiv, half, voxel, origin);
    hipLaunchKernelGGL(lm_clear_kernel, dim3(grid_for((size_t)cap_vox * (size_t)(1 + M.S))), dim3(LM_BLOCK), 0,
                       (hipStream_t)stream, M, 1 - half, false);
    hipLaunchKernelGGL(lm_prune_kernel, dim3(dpm_cdiv(cap_vox, LM_BLOCK)), dim3(LM_BLOCK), 0, (hipStream_t)stream, M, pose,
                       (float)(radius * radius));
    return dpm_launch_status();
}

extern "C" int dpm_local_map_insert_frames(void *map, int cap_vox, int subdiv, int half, double voxel, const double *origin,
                                           const float *store, const int32_t *lengths, int capacity, int P,
                                           const int32_t *frames, const double *poses, const uint32_t *stamps, int F,
                                           const double *centre, double radius, double min_range, double max_range,
                                           dpm_stream_t stream) {
    DPM_CHECK_ARG(map_ok(map, cap_vox, subdiv) && geometry_ok(half, voxel, origin));
    DPM_CHECK_ARG(range_ok(min_range, max_range) && (!centre || (radius >= 0.0 && radius < 1e18)));
    DPM_CHECK_ARG(F == 0 || stamps);   // an empty list may come with null pointers
    const Map M = make_map(map, cap_vox, subdiv, half, voxel, origin);
    const StoredRows L{{store, lengths, capacity, P, frames, poses}, stamps, centre};
    const float lo2 = (float)(min_range * min_range), hi2 = (float)(max_range * max_range);
    const float r2 = centre ? (float)(radius * radius) : 0.f;
    return source_launch(L.rows, F, LM_BLOCK, [&](dim3 grid) {
        hipLaunchKernelGGL(lm_insert_frames_kernel<false>, grid, dim3(LM_BLOCK), 0, (hipStream_t)stream, M, L, lo2, hi2, r2);
        hipLaunchKernelGGL(lm_insert_frames_kernel<true>, grid, dim3(LM_BLOCK), 0, (hipStream_t)stream, M, L, lo2, hi2, r2);
    });
}

namespace {

// both registrations: PA = nullptr is point-to-point
int register_impl(const PlaneArgs *PA, const void *map, int cap_vox, int subdiv, int half, double voxel, const double *origin,
                  const float *xyz, const int32_t *count, int cap, const double *init_pose, const double *stage_max_dist,
                  const int32_t *stage_max_iter, int n_stages, double kernel_scale, double tol_rot, double tol_trans,
                  double *pose, float *fitness, float *rmse, int32_t *iterations, int32_t *status, long long *debug_key,
                  int32_t *debug_sub, double *debug_system, void *workspace, dpm_stream_t stream) {
    DPM_CHECK_ARG(map_ok(map, cap_vox, subdiv) && geometry_ok(half, voxel, origin));
    DPM_CHECK_ARG(xyz && count && init_pose && stage_max_dist && stage_max_iter && workspace && cap >= 1);
    DPM_CHECK_ARG(pose && fitness && rmse && iterations && status && pose != init_pose);
    DPM_CHECK_ARG(n_stages >= 1 && n_stages <= 16 && tol_rot >= 0.0 && tol_trans >= 0.0 && kernel_scale >= 0.0 && kernel_scale < 1e18);
    for (int s = 0; s < n_stages; ++s)
        DPM_CHECK_ARG(stage_max_dist[s] > 0.0 && stage_max_dist[s] <= (double)(float)voxel && stage_max_iter[s] >= 0);
    hipStream_t st = (hipStream_t)stream;
    RegArgs A{};
    A.M = make_map((void *)map, cap_vox, subdiv, half, voxel, origin);
    A.F = Frame{xyz, nullptr, count, cap};
    WsCursor c(workspace);
    gn_one_layout(c, cap, A.hdr, A.partial);
    A.pose = pose, A.fitness = fitness, A.rmse = rmse, A.iterations = iterations, A.status = status;
    A.dbg_key = debug_key, A.dbg_sub = debug_sub, A.dbg_system = debug_system;
    const double kappa = kernel_scale * kernel_scale;
    const PlaneArgs none{nullptr, nullptr, 0, 0.f};
    const GnOne G{A.hdr, A.partial, pose, fitness, rmse, iterations, status, debug_system, count, cap, A.M.ox, A.M.oy, A.M.oz};
    return gn_one_run(G, init_pose, stage_max_iter, n_stages, tol_rot, tol_trans, st, [&](int s) {
        const float r2 = (float)(stage_max_dist[s] * stage_max_dist[s]);
        if (PA) hipLaunchKernelGGL(lm_accumulate_kernel<true>, dim3(dpm_cdiv(cap, 256)), dim3(LM_BLOCK), 0, st, A, r2, kappa, *PA);
        else hipLaunchKernelGGL(lm_accumulate_kernel<false>, dim3(dpm_cdiv(cap, 256)), dim3(LM_BLOCK), 0, st, A, r2, kappa, none);
    });
}

}  // namespace

extern "C" int dpm_local_map_register(const void *map, int cap_vox, int subdiv, int half, double voxel, const double *origin,
                                      const float *xyz, const int32_t *count, int cap, const double *init_pose,
                                      const double *stage_max_dist, const int32_t *stage_max_iter, int n_stages,
                                      double kernel_scale, double tol_rot, double tol_trans, double *pose, float *fitness,
                                      float *rmse, int32_t *iterations, int32_t *status, long long *debug_key,
                                      int32_t *debug_sub, double *debug_system, void *workspace, dpm_stream_t stream) {
    return register_impl(nullptr, map, cap_vox, subdiv, half, voxel, origin, xyz, count, cap, init_pose, stage_max_dist,
                         stage_max_iter, n_stages, kernel_scale, tol_rot, tol_trans, pose, fitness, rmse, iterations, status,
                         debug_key, debug_sub, debug_system, workspace, stream);
}

extern "C" int dpm_local_map_planes(const void *map, int cap_vox, int subdiv, int half, double voxel, const double *origin,
                                    double plane_radius, float *planes, int32_t *counts, dpm_stream_t stream) {
    DPM_CHECK_ARG(map_ok(map, cap_vox, subdiv) && geometry_ok(half, voxel, origin));
    DPM_CHECK_ARG(planes && counts && ((uintptr_t)planes & 15) == 0);
    DPM_CHECK_ARG(plane_radius > 0.0 && plane_radius <= 1.5 * (double)(float)voxel);
    const Map M = make_map((void *)map, cap_vox, subdiv, half, voxel, origin);
    hipLaunchKernelGGL(lm_planes_kernel, dim3(dpm_cdiv(cap_vox, LM_BLOCK / 4)), dim3(LM_BLOCK), 0, (hipStream_t)stream, M,
                       (float)(plane_radius * plane_radius), (float4 *)planes, counts);
    return dpm_launch_status();
}

extern "C" int dpm_local_map_register_planes(const void *map, int cap_vox, int subdiv, int half, double voxel,
                                             const double *origin, const float *planes, const int32_t *counts, int min_points,
                                             double max_ratio, const float *xyz, const int32_t *count, int cap,
                                             const double *init_pose, const double *stage_max_dist,
                                             const int32_t *stage_max_iter, int n_stages, double kernel_scale, double tol_rot,
                                             double tol_trans, double *pose, float *fitness, float *rmse, int32_t *iterations,
                                             int32_t *status, long long *debug_key, int32_t *debug_sub, double *debug_system,
                                             void *workspace, dpm_stream_t stream) {
    DPM_CHECK_ARG(planes && counts && ((uintptr_t)planes & 15) == 0 && min_points >= 0 && max_ratio >= 0.0 && max_ratio < 1e18);
    const PlaneArgs PA{(const float4 *)planes, counts, min_points, (float)max_ratio};
    return register_impl(&PA, map, cap_vox, subdiv, half, voxel, origin, xyz, count, cap, init_pose, stage_max_dist,
                         stage_max_iter, n_stages, kernel_scale, tol_rot, tol_trans, pose, fitness, rmse, iterations, status,
                         debug_key, debug_sub, debug_system, workspace, stream);
}

extern "C" int dpm_local_map_export(const void *map, int cap_vox, int subdiv, int half, unsigned long long *keys,
                                    int32_t *sub, unsigned long long *owner, float *xyz, int32_t *count, int max_out,
                                    dpm_stream_t stream) {
    DPM_CHECK_ARG(map_ok(map, cap_vox, subdiv) && (half == 0 || half == 1) && count && max_out >= 0);
    DPM_CHECK_ARG(max_out == 0 || (keys && sub && owner && xyz));
    const Map M = make_map((void *)map, cap_vox, subdiv, half, 1.0, nullptr);
    hipLaunchKernelGGL(lm_export_kernel, dim3(grid_for((size_t)cap_vox * M.S)), dim3(LM_BLOCK), 0, (hipStream_t)stream, M, keys,
                       sub, owner, xyz, count, max_out);
    return dpm_launch_status();
}
