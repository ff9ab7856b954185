// The kernels of the single-problem Gauss-Newton driver (csrc/gn_one.h) and the loop that launches them: one thread sets a
// problem to its start values, one re-arms it for the next stage, one wave adds the accumulate blocks' partials in block order
// and takes the step.  Defined here and not in the header: the library links separately compiled objects, and a kernel has one
// code object.
#include "gn_one.h"

namespace {

__global__ void gn_one_init_kernel(GnOne G, const double *init) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    gn_init_problem(0, init, G.pose, G.fitness, G.rmse, G.iterations, G.status);
    G.hdr->done = 0, G.hdr->n1 = min(max(G.count[0], 0), G.cap);
    gn_zero_system(0, G.dbg_system);
}

__global__ void gn_one_stage_kernel(GnOne G) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    G.hdr->done = 0;
    *G.status = DPM_ICP_MAX_ITER;
}

__global__ __launch_bounds__(64) void gn_one_solve_kernel(GnOne G, double tol_rot, double tol_trans) {
    const int lane = threadIdx.x;
    if (G.hdr->done) return;
    __shared__ double S[GN_NSUM_PAD];
    gn_sum_partials(G.partial, (G.cap + 255) / 256, S, G.dbg_system, 0);
    if (lane != 0) return;
    // the rows were formed in the map frame, so the step acts on the pose there; a step that was not taken leaves the
    // world pose's bytes alone
    double local[12];
    for (int k = 0; k < 12; ++k) local[k] = G.pose[k];
    local[3] -= G.ox, local[7] -= G.oy, local[11] -= G.oz;
    const int before = G.iterations[0];
    gn_solve_step(S, G.hdr->n1, local, G.fitness, G.rmse, G.iterations, G.status, 0, &G.hdr->done, tol_rot, tol_trans);
    if (G.iterations[0] == before) return;
    local[3] += G.ox, local[7] += G.oy, local[11] += G.oz;
    for (int k = 0; k < 12; ++k) G.pose[k] = local[k];
}

}  // namespace

int gn_one_run(const GnOne &G, const double *init, const int32_t *stage_max_iter, int n_stages, double tol_rot, double tol_trans,
               hipStream_t stream, const std::function<void(int)> &accumulate) {
    hipLaunchKernelGGL(gn_one_init_kernel, dim3(1), dim3(64), 0, stream, G, init);
    for (int s = 0; s < n_stages; ++s) {
        if (s > 0) hipLaunchKernelGGL(gn_one_stage_kernel, dim3(1), dim3(64), 0, stream, G);
        for (int it = 0; it < stage_max_iter[s]; ++it) {
            accumulate(s);
            hipLaunchKernelGGL(gn_one_solve_kernel, dim3(1), dim3(64), 0, stream, G, tol_rot, tol_trans);
        }
    }
    return dpm_launch_status();
}
