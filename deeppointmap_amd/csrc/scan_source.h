// Where the hashed maps (csrc/local_map.hip, csrc/tsdf_map.hip) take their rows from: ONE FRAME as the filters leave it, or a LIST
// OF STORED FRAMES.  Both are plain kernel arguments with one device interface, so a fusion kernel is written once over `Src`:
//   open(o)      block-uniform: the clamped length o.n and the pose o.pose of this block's frame; false when the list entry
//                (blockIdx.y) names a row outside the store, and then nothing of that row may be read: the whole block leaves
//   point(o, i)  the sensor-frame coordinates of row i < o.n
//   side(o, i)   the flat index of row i in a per-row side array (normals)
// and one host interface, what an entry point asks before it launches (source_launch).  The layouts differ, row-major against
// channel-major, so one frame is NOT a list of one.
#pragma once
#include "dpm_common.h"

struct SourceRows {   // what open() yields
    int row, n;       // the store's row (0 for one frame), rows to read
    const double *pose;
};

struct OneFrame {
    const float *xyz;        // (cap,3)
    const int32_t *count;    // (1,) on the device, clamped to [0, cap]
    int cap;
    const double *pose;      // (16,)

    __device__ __forceinline__ bool open(SourceRows &o) const {
        o.row = 0, o.n = min(max(count[0], 0), cap), o.pose = pose;
        return true;
    }
    __device__ __forceinline__ void point(const SourceRows &, int i, float &x, float &y, float &z) const {
        const float *p = xyz + 3 * (size_t)i;
        x = p[0], y = p[1], z = p[2];
    }
    __device__ __forceinline__ size_t side(const SourceRows &, int i) const { return (size_t)i; }

    bool ok(int) const { return xyz && count && pose && cap >= 0; }   // null pointers are refused at cap == 0 too
    bool empty(int) const { return cap == 0; }
    dim3 grid(int block, int) const { return dim3(dpm_cdiv(cap, block)); }
};

// F rows of a channel-major store (capacity,3,P)
inline bool frame_list_ok(int capacity, int P, int F) {
    return capacity >= 1 && P >= 1 && (size_t)capacity * 3 * (size_t)P < ((size_t)1 << 40) && F >= 0 && F <= 65535;
}

struct StoredFrames {   // entry f: row frames[f] of the store under poses[f]
    const float *store;        // (capacity,3,P)
    const int32_t *lengths;    // (capacity,)
    int capacity, P;
    const int32_t *frames;     // (F,) rows of the store
    const double *poses;       // (F,16)

    __device__ __forceinline__ bool open(SourceRows &o) const {
        const int f = blockIdx.y;
        o.row = frames[f];
        if ((unsigned)o.row >= (unsigned)capacity) return false;   // never read out of bounds
        o.n = min(max(lengths[o.row], 0), P), o.pose = poses + 16 * (size_t)f;
        return true;
    }
    __device__ __forceinline__ void point(const SourceRows &o, int i, float &x, float &y, float &z) const {
        const float *p = store + (size_t)o.row * 3 * P + i;
        x = p[0], y = p[P], z = p[2 * (size_t)P];
    }
    __device__ __forceinline__ size_t side(const SourceRows &o, int i) const { return (size_t)o.row * P + i; }

    // an empty list may come with null pointers
    bool ok(int F) const { return frame_list_ok(capacity, P, F) && (F == 0 || (store && lengths && frames && poses)); }
    bool empty(int F) const { return F == 0; }
    dim3 grid(int block, int F) const { return dim3(dpm_cdiv(P, block), F); }
};

// The tail of an entry point over a source of F entries (1 for a frame), after its own checks: refuse the source, return on an
// empty one, else launch(grid) with one lane per row.  The arrays an operation reads beside the source are its own to check.
template <typename Src, typename Launch>
inline int source_launch(const Src &S, int F, int block, Launch launch) {
    DPM_CHECK_ARG(S.ok(F));
    if (S.empty(F)) return DPM_OK;
    launch(S.grid(block, F));
    return dpm_launch_status();
}

// the range gate of a row, on the host
inline bool range_ok(double min_range, double max_range) { return min_range >= 0.0 && max_range >= min_range && max_range < 1e18; }
