// The driver of a SINGLE Gauss-Newton problem against a map with an origin, written once for csrc/local_map.hip (a scan against
// the rolling map) and csrc/tsdf_map.hip (a scan against the field); csrc/gn_one.hip holds its kernels.  The caller keeps its
// argument checks and its accumulate kernel, which reads hdr->done / hdr->n1 and writes one partial of GN_NSUM_PAD doubles per
// block of 256 rows; everything else of a registration is here: the start values, the stages, the sum of the partials, the step
// of csrc/gn_solve.h taken in the map frame, the stop rule and the statuses.  csrc/icp.hip's batched driver indexes by pair and
// stays its own.
#pragma once
#include <functional>

#include "gn_solve.h"
#include "workspace.h"

struct GnOneHdr {   // start of the workspace (256 bytes), then one partial of GN_NSUM_PAD doubles per block
    int done, n1;
};

struct GnOne {
    GnOneHdr *hdr;
    double *partial;
    double *pose;
    float *fitness, *rmse;
    int32_t *iterations, *status;
    double *dbg_system;       // (GN_NSUM,) or NULL
    const int32_t *count;     // (1,) the frame's rows, clamped to [0, cap]
    int cap;
    double ox, oy, oz;        // the map's origin
};

// the workspace: the header in a 256-byte slice of its own, then the accumulate blocks' partials (512 + 256 bytes per 256 points
// of capacity: the size the callers compute)
inline void gn_one_layout(WsCursor &c, int cap, GnOneHdr *&hdr, double *&partial) {
    static_assert(sizeof(GnOneHdr) <= 256, "the header has a 256-byte slice");
    hdr = c.take256<GnOneHdr>(1);
    partial = c.take<double>((size_t)dpm_cdiv(cap, 256) * GN_NSUM_PAD);
}

// The staged loop (csrc/gn_one.hip): init, then per stage the stage kernel (after the first) and per iteration accumulate(stage),
// the caller's launch of its own kernel, followed by solve.  No host synchronisation, one stream: capturable in a graph.
// Hidden: nothing is added to the library's symbols.
__attribute__((visibility("hidden"))) int gn_one_run(const GnOne &G, const double *init, const int32_t *stage_max_iter, int n_stages,
                                                     double tol_rot, double tol_trans, hipStream_t stream,
                                                     const std::function<void(int)> &accumulate);
