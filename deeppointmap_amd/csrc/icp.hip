// Batched ICP: refines the relative pose of P scan pairs at once.  Stands in for the offline third-party ICP that made the
// reference's per-scene refined_SE3.pkl (read by pipeline/modules/model_pipeline.py:199-282 through get_SE3_from_dict; no
// file of the reference writes it).
//
// Target side, once per call: every pair's target scan is counting-sorted into a pose-independent 2-D xy grid -- the layout
// of csrc/infomat.hip (cell edge half the radius and 5x5 cells, or one radius and 3x3 cells when that needs more than GMAX
// cells per axis), built here by a pass of its own (setup, count, scan, scatter) that honours the per-frame point counts.
// The order of the points inside a cell depends on scheduling (integer atomics); nothing downstream depends on it.
//
// Per iteration, two launches for all pairs together and no host synchronisation:
//   accumulate: four lanes per source point scan the cells around the transformed point; the winner is the smallest
//               (distance bits, original index) key, as in nn1_match_kernel.  Lane 0 of the quad adds the match's
//               Gauss-Newton rows (unweighted) to the 29 fp64 running sums.  Queries are walked in INDEX order and every
//               block leaves one partial.
//   solve:      one wave per pair adds the partials in block order, takes the step and sets the pair's `done` flag; blocks
//               of a done pair return at once.
// The rows, the reduction, the solve and the step x = (w, v), which moves a transformed point p' to p' + w x p' + v, are
// csrc/gn_solve.h, shared with csrc/local_map.hip.
#include "block_scan.h"
#include "cell_grid.h"
#include "gn_solve.h"
#include "workspace.h"

namespace {

constexpr int GMAX = 512;   // grid cells per axis (upper bound)

struct IcpHdr {   // start of every pair's workspace slice (256 bytes reserved)
    float lox, loy, inv_cs;
    int gx, gy, ncell, H;
    int n1, n2;        // valid points of the source / target frame
    int fs, fd;        // frame indices, clamped into [0, F)
    int done;
};

struct IcpArgs {
    const float *pcd;          // (F,3,N)
    const float *normals;      // (F,N,3) or NULL (point metric)
    const int32_t *lengths, *src, *dst;
    int F, N, n_pairs;
    char *ws;
    size_t ws_stride;
    double *pose;              // (P,16)
    float *fitness, *rmse;
    int32_t *iterations, *status;
    int32_t *dbg_match;        // (P,N) or NULL
    double *dbg_system;        // (P,GN_NSUM) or NULL
};

__device__ __forceinline__ IcpHdr *hdr_of(const IcpArgs &a, int p) { return (IcpHdr *)(a.ws + (size_t)p * a.ws_stride); }
// cell c holds sorted[cells[c] .. cells[c + 1])   (ncell + 1 entries)
__device__ __forceinline__ int *cells_of(const IcpArgs &a, int p) { return (int *)(a.ws + (size_t)p * a.ws_stride + 256); }
__device__ __forceinline__ float4 *sorted_of(const IcpArgs &a, int p) {
    return (float4 *)(a.ws + (size_t)p * a.ws_stride + 256 + sizeof(int) * (size_t)(GMAX * GMAX + 4));
}
__device__ __forceinline__ double *partial_of(const IcpArgs &a, int p) { return (double *)(sorted_of(a, p) + a.N); }

// One workgroup per pair: frame indices and counts, the target's xy bounds, the grid header, and the cell counters zeroed.
__global__ __launch_bounds__(1024) void icp_setup_kernel(IcpArgs A, float radius) {
    const int pair = blockIdx.x, t = threadIdx.x;
    IcpHdr *hdr = hdr_of(A, pair);
    const int fs = min(max(A.src[pair], 0), A.F - 1), fd = min(max(A.dst[pair], 0), A.F - 1);
    const int n1 = min(max(A.lengths[fs], 0), A.N), n2 = min(max(A.lengths[fd], 0), A.N);
    const float *p2 = A.pcd + (size_t)fd * 3 * A.N;
    float lox = __builtin_inff(), loy = lox, hix = -lox, hiy = -lox;
    for (int i = t; i < n2; i += 1024) {
        const float x = p2[i], y = p2[(size_t)A.N + i];
        lox = fminf(lox, x), hix = fmaxf(hix, x), loy = fminf(loy, y), hiy = fmaxf(hiy, y);
    }
    __shared__ float red[4][16];
    __shared__ int s_ncell;
    box_put(lox, loy, hix, hiy, red);
    __syncthreads();
    if (t == 0) {
        box_get(lox, loy, hix, hiy, red, 1);
        // an empty target, or one with a non-finite coordinate (its bounds are no numbers to divide by): one empty-handed cell
        const bool usable = n2 > 0 && hix - lox < 3e38f && hiy - loy < 3e38f && hix - lox >= 0.f && hiy - loy >= 0.f;
        int gx = 1, gy = 1, H = 1;
        float cs = radius;
        if (usable) {
            const float ext = fmaxf(fmaxf(hix - lox, hiy - loy), 1e-6f);
            cs = fmaxf(radius * 0.5005f, ext / (float)(GMAX - 1)), H = 2;
            if (cs >= radius) cs = fmaxf(radius, ext / (float)(GMAX - 1)), H = 1;
            gx = min(GMAX, (int)((hix - lox) / cs) + 1), gy = min(GMAX, (int)((hiy - loy) / cs) + 1);
        } else {
            lox = 0.f, loy = 0.f;
        }
        hdr->lox = lox, hdr->loy = loy, hdr->inv_cs = 1.0f / cs, hdr->gx = gx, hdr->gy = gy, hdr->ncell = gx * gy, hdr->H = H;
        hdr->n1 = n1, hdr->n2 = usable ? n2 : 0, hdr->fs = fs, hdr->fd = fd, hdr->done = 0;
        s_ncell = gx * gy;
    }
    __syncthreads();
    int *cells = cells_of(A, pair);
    for (int c = t; c <= s_ncell; c += 1024) cells[c] = 0;
}

// the two passes of the counting sort around icp_scan_kernel (grid_count_or_place of cell_grid.h)
template <bool PLACE>
__global__ __launch_bounds__(256) void icp_grid_kernel(IcpArgs A) {
    const int pair = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    const IcpHdr *hdr = hdr_of(A, pair);
    if (i >= hdr->n2) return;
    const float *p2 = A.pcd + (size_t)hdr->fd * 3 * A.N;
    const float x = p2[i], y = p2[(size_t)A.N + i];
    const int c = cell_coord(y, hdr->loy, hdr->inv_cs, hdr->gy) * hdr->gx + cell_coord(x, hdr->lox, hdr->inv_cs, hdr->gx);
    grid_count_or_place<PLACE>(cells_of(A, pair), sorted_of(A, pair), A.N, c, x, y, PLACE ? p2[2 * (size_t)A.N + i] : 0.f, i);
}

// exclusive prefix sum of cells[1 .. ncell] in place, one workgroup per pair (thread t owns a contiguous run of cells)
__global__ __launch_bounds__(1024) void icp_scan_kernel(IcpArgs A) {
    __shared__ int wsum[16];
    const int pair = blockIdx.x, ncell = hdr_of(A, pair)->ncell;
    block_scan_runs(cells_of(A, pair) + 1, ncell, (ncell + 1023) / 1024, wsum);
}

// pose <- init, the per-pair results to their start values
__global__ void icp_init_kernel(IcpArgs A, const double *init) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= A.n_pairs) return;
    gn_init_problem(p, init, A.pose, A.fitness, A.rmse, A.iterations, A.status);
    gn_zero_system(p, A.dbg_system);
}

// a new stage of the schedule: every pair runs again from where it stands
__global__ void icp_stage_kernel(IcpArgs A) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= A.n_pairs) return;
    hdr_of(A, p)->done = 0;
    A.status[p] = DPM_ICP_MAX_ITER;
}

template <int PLANE>
__global__ __launch_bounds__(256) void icp_accumulate_kernel(IcpArgs A, float r2) {
    int pair, blk;
    pair_block(blk, pair);
    const IcpHdr *hdr = hdr_of(A, pair);
    if (hdr->done) return;
    const int N = A.N, n1 = hdr->n1;
    const float *p1 = A.pcd + (size_t)hdr->fs * 3 * N;
    const float *p2 = A.pcd + (size_t)hdr->fd * 3 * N;
    const float *nrm = PLANE ? A.normals + (size_t)hdr->fd * 3 * N : nullptr;
    const int *cells = cells_of(A, pair);
    const float4 *sorted = sorted_of(A, pair);
    const int gx = hdr->gx, gy = hdr->gy, H = hdr->H;
    const float inv_cs = hdr->inv_cs, lox = hdr->lox, loy = hdr->loy;
    // The search runs in fp32, like the information matrix's: gn_load_pose / gn_xform with no origin, written out because
    // through them the point kernel timed above this form in both runs (profiles/gn_shared_isa.md).
    const double *pose = A.pose + (size_t)pair * 16;
    float Rt[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) Rt[k] = (float)pose[k];
    const int quad = threadIdx.x >> 2, ql = threadIdx.x & 3;
    double s[GN_NSUM];
#pragma unroll
    for (int k = 0; k < GN_NSUM; ++k) s[k] = 0.0;
    for (int j = 0; j < 4; ++j) {
        const int i = blk * 256 + j * 64 + quad;   // uniform inside a quad
        if (i >= n1) {
            if (i < N && A.dbg_match && ql == 0) A.dbg_match[(size_t)pair * N + i] = -1;
            continue;
        }
        const float x = p1[i], y = p1[(size_t)N + i], z = p1[2 * (size_t)N + i];
        const float q[3] = {fmaf(Rt[2], z, fmaf(Rt[1], y, Rt[0] * x)) + Rt[3], fmaf(Rt[6], z, fmaf(Rt[5], y, Rt[4] * x)) + Rt[7],
                            fmaf(Rt[10], z, fmaf(Rt[9], y, Rt[8] * x)) + Rt[11]};
        const float flx = floorf((q[0] - lox) * inv_cs), fly = floorf((q[1] - loy) * inv_cs);
        const int cx = (int)fmaxf(fminf(flx, 1e6f), -1e6f), cy = (int)fmaxf(fminf(fly, 1e6f), -1e6f);
        const int xa = min(max(cx - H, 0), gx), xb = min(max(cx + H + 1, 0), gx);
        unsigned long long best = ~0ull;
        // a row's cells xa .. xb-1 are one range of `sorted`; the range ends of all rows are requested before the first is used
        int rlo[5], rhi[5];
#pragma unroll
        for (int r = 0; r < 5; ++r) {
            const int yy = cy - H + r;
            const bool in = r <= 2 * H && yy >= 0 && yy < gy;
            const int yc = min(max(yy, 0), gy - 1);
            rlo[r] = in ? cells[yc * gx + xa] : 0, rhi[r] = in ? cells[yc * gx + xb] : 0;
        }
#pragma unroll
        for (int r = 0; r < 5; ++r) quad_scan_range(sorted, rlo[r], rhi[r], ql, q[0], q[1], q[2], best);
        best = quad_min_key(best);
        const bool hit = best != ~0ull && __uint_as_float((unsigned)(best >> 32)) <= r2;   // a NaN distance is no hit
        const int win = hit ? (int)(unsigned)best : -1;
        if (ql != 0) continue;
        if (A.dbg_match) A.dbg_match[(size_t)pair * N + i] = win;
        if (!hit) continue;
        const double p[3] = {q[0], q[1], q[2]};
        const double e[3] = {p[0] - (double)p2[win], p[1] - (double)p2[(size_t)N + win], p[2] - (double)p2[2 * (size_t)N + win]};
        s[27] += 1.0;
        if (PLANE) {
            const double n[3] = {nrm[3 * (size_t)win], nrm[3 * (size_t)win + 1], nrm[3 * (size_t)win + 2]};
            gn_plane_row(s, p, n, e, 0.0);
        } else {
            gn_point_rows(s, p, e, 1.0);
        }
    }
    gn_block_reduce(s, partial_of(A, pair), blk);
}

__global__ __launch_bounds__(64) void icp_solve_kernel(IcpArgs A, double tol_rot, double tol_trans) {
    const int pair = blockIdx.x, lane = threadIdx.x;
    IcpHdr *hdr = hdr_of(A, pair);
    if (hdr->done) return;
    __shared__ double S[GN_NSUM_PAD];
    gn_sum_partials(partial_of(A, pair), (A.N + 255) / 256, S, A.dbg_system, pair);
    if (lane != 0) return;
    gn_solve_step(S, hdr->n1, A.pose + (size_t)pair * 16, A.fitness, A.rmse, A.iterations, A.status, pair, &hdr->done, tol_rot, tol_trans);
}

size_t slice_bytes(int N) {
    const size_t b = 256 + sizeof(int) * (size_t)(GMAX * GMAX + 4) + sizeof(float4) * (size_t)N +
                     sizeof(double) * GN_NSUM_PAD * (size_t)dpm_cdiv(N, 256);
    return ws_align256(b);
}

}  // namespace

extern "C" size_t dpm_icp_workspace_bytes(int n_pairs, int N) {
    if (n_pairs < 1 || N < 1) return 0;
    return 256 + (size_t)n_pairs * slice_bytes(N);
}

extern "C" int dpm_icp_refine_batched(const float *pcd, int F, int N, const int32_t *lengths, const float *normals,
                                      const int32_t *src_frame, const int32_t *dst_frame, int n_pairs,
                                      const double *init_pose, int metric, const double *stage_max_dist,
                                      const int32_t *stage_max_iter, int n_stages, double tol_rot, double tol_trans,
                                      double *pose, float *fitness, float *rmse, int32_t *iterations, int32_t *status,
                                      int32_t *debug_match, double *debug_system, void *workspace, dpm_stream_t stream) {
    DPM_CHECK_ARG(pcd && lengths && src_frame && dst_frame && init_pose && stage_max_dist && stage_max_iter && workspace);
    DPM_CHECK_ARG(pose && fitness && rmse && iterations && status && pose != init_pose);
    DPM_CHECK_ARG(F >= 1 && N >= 1 && n_pairs >= 1 && n_stages >= 1 && n_stages <= 16 && tol_rot >= 0.0 && tol_trans >= 0.0);
    DPM_CHECK_ARG(metric == DPM_ICP_POINT || metric == DPM_ICP_PLANE);
    DPM_CHECK_ARG(metric == DPM_ICP_POINT || normals);
    if ((long long)n_pairs * N > 0x7fffffffLL || n_pairs > 65535) return DPM_EUNSUPPORTED;
    double rmax = 0.0;
    for (int s = 0; s < n_stages; ++s) {
        DPM_CHECK_ARG(stage_max_dist[s] > 0.0 && stage_max_dist[s] < 1e18 && stage_max_iter[s] >= 0);
        rmax = stage_max_dist[s] > rmax ? stage_max_dist[s] : rmax;
    }
    hipStream_t st = (hipStream_t)stream;
    IcpArgs A{};
    A.pcd = pcd, A.normals = normals, A.lengths = lengths, A.src = src_frame, A.dst = dst_frame;
    A.F = F, A.N = N, A.n_pairs = n_pairs;
    A.ws = (char *)ws_align256((uintptr_t)workspace), A.ws_stride = slice_bytes(N);
    A.pose = pose, A.fitness = fitness, A.rmse = rmse, A.iterations = iterations, A.status = status;
    A.dbg_match = debug_match, A.dbg_system = debug_system;
    const dim3 per_point(dpm_cdiv(N, 256), n_pairs);
    // the grids serve every stage: cells sized for the largest radius of the schedule
    hipLaunchKernelGGL(icp_init_kernel, dim3(dpm_cdiv(n_pairs, 64)), dim3(64), 0, st, A, init_pose);
    hipLaunchKernelGGL(icp_setup_kernel, dim3(n_pairs), dim3(1024), 0, st, A, (float)rmax);
    hipLaunchKernelGGL(icp_grid_kernel<false>, per_point, dim3(256), 0, st, A);
    hipLaunchKernelGGL(icp_scan_kernel, dim3(n_pairs), dim3(1024), 0, st, A);
    hipLaunchKernelGGL(icp_grid_kernel<true>, per_point, dim3(256), 0, st, A);
    for (int s = 0; s < n_stages; ++s) {
        const float r2 = (float)(stage_max_dist[s] * stage_max_dist[s]);
        if (s > 0) hipLaunchKernelGGL(icp_stage_kernel, dim3(dpm_cdiv(n_pairs, 64)), dim3(64), 0, st, A);
        for (int it = 0; it < stage_max_iter[s]; ++it) {
            if (metric == DPM_ICP_PLANE) hipLaunchKernelGGL(icp_accumulate_kernel<1>, per_point, dim3(256), 0, st, A, r2);
            else hipLaunchKernelGGL(icp_accumulate_kernel<0>, per_point, dim3(256), 0, st, A, r2);
            hipLaunchKernelGGL(icp_solve_kernel, dim3(n_pairs), dim3(64), 0, st, A, tol_rot, tol_trans);
        }
    }
    return dpm_launch_status();
}
