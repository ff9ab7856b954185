// The Gauss-Newton step of the registrations (icp.hip: batched scan pairs; local_map.hip: a scan against the rolling map;
// tsdf_map.hip: a scan against the field), written once.  The accumulate kernels keep their searches; what follows the match is
// here, and its order of operations is part of the contract (the tests compare bytes and fp64 floors).  The kernels that run
// it are icp.hip's own for a batch of pairs and gn_one.hip's (the driver of gn_one.h) for the two single scans against a map:
//   the search pose: the fp64 pose minus an origin, rounded to fp32, and q = fma(R2, z, fma(R1, y, R0 * x)) + t;
//   the rows of a match into the 29 fp64 sums S = [H upper triangle row-major (21), g (6), matches, sum of squared residuals]:
//     H and g weighted (Geman-McClure), the count (the caller's s[27] += 1.0) and the squared residuals not;
//   the block reduction, lanes then waves in a fixed tree, and the solve kernels' sum of the blocks' partials in block order:
//     the sums do not depend on scheduling, no floating-point atomics;
//   gn_solve_step, run by ONE lane on S: fitness and rmse, H x = -g by Cholesky with a pivot test, the step x = (w, v) composed
//     onto the pose as pose <- [exp(w) | v] o pose (Rodrigues rotation, the translation taken as it is), the stop rule and the
//     status.  No match: NO_MATCH; a system that cannot be solved, or a step / pose that is no number: SINGULAR -- both leave
//     the pose at its last good value and set *done;
//   the start values of a problem.
#pragma once
#include "dpm_common.h"

constexpr int GN_NSUM = 29, GN_NSUM_PAD = 32;
constexpr double GN_PIV_EPS = 1e-9;  // a Cholesky pivot below GN_PIV_EPS * (largest diagonal entry of its 3x3 block) is singular

// the fp32 pose the searches run with: 9 rotation entries row-major, then the translation minus the origin, the difference
// formed in fp64 and rounded once.  (icp_accumulate_kernel writes the same arithmetic out, with no origin.)
struct GnPose32 {
    float R[9], t[3];
};

__device__ __forceinline__ GnPose32 gn_load_pose(const double *pose, double ox, double oy, double oz) {
    GnPose32 P;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) P.R[3 * i + j] = (float)pose[4 * i + j];
    P.t[0] = (float)(pose[3] - ox), P.t[1] = (float)(pose[7] - oy), P.t[2] = (float)(pose[11] - oz);
    return P;
}

__device__ __forceinline__ void gn_xform(const GnPose32 &P, float x, float y, float z, float q[3]) {
#pragma unroll
    for (int a = 0; a < 3; ++a) q[a] = fmaf(P.R[3 * a + 2], z, fmaf(P.R[3 * a + 1], y, P.R[3 * a] * x)) + P.t[a];
}

// one row J (6) with residual e and weight w: H += w J^T J, g += w J^T e, squared residuals += e e  (w = 1.0 folds away)
__device__ __forceinline__ void gn_add_row(double (&s)[GN_NSUM], const double (&J)[6], double e, double w) {
    int k = 0;
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        const double wj = w * J[i];
#pragma unroll
        for (int j = i; j < 6; ++j) s[k] = fma(wj, J[j], s[k]), ++k;
        s[21 + i] = fma(wj, e, s[21 + i]);
    }
    s[28] = fma(e, e, s[28]);
}

// Geman-McClure weight of a match with squared residual E; kappa = kernel_scale^2, 0: unweighted
__device__ __forceinline__ double gn_weight(double kappa, double E) {
    if (!(kappa > 0.0)) return 1.0;
    const double r = kappa / (kappa + E);
    return r * r;
}

// point-to-point: the three rows of the moved point p with residual e = p - target
__device__ __forceinline__ void gn_point_rows(double (&s)[GN_NSUM], const double (&p)[3], const double (&e)[3], double w) {
    const double Jx[6] = {0.0, p[2], -p[1], 1.0, 0.0, 0.0}, Jy[6] = {-p[2], 0.0, p[0], 0.0, 1.0, 0.0},
                 Jz[6] = {p[1], -p[0], 0.0, 0.0, 0.0, 1.0};
    gn_add_row(s, Jx, e[0], w), gn_add_row(s, Jy, e[1], w), gn_add_row(s, Jz, e[2], w);
}

// point-to-plane: the row J = (p x n, n) with residual n . e, weighted by that residual
__device__ __forceinline__ void gn_plane_row(double (&s)[GN_NSUM], const double (&p)[3], const double (&n)[3],
                                             const double (&e)[3], double kappa) {
    const double r = (n[0] * e[0] + n[1] * e[1]) + n[2] * e[2];
    const double J[6] = {p[1] * n[2] - p[2] * n[1], p[2] * n[0] - p[0] * n[2], p[0] * n[1] - p[1] * n[0], n[0], n[1], n[2]};
    gn_add_row(s, J, r, gn_weight(kappa, r * r));
}

// a row on a scalar field: the residual e is the field's value at the moved point p and J = (p x g, g) with g its gradient
// there, in gn_plane_row's component order; weighted by that residual.  g is taken as it is: no normalisation.
__device__ __forceinline__ void gn_field_row(double (&s)[GN_NSUM], const double (&p)[3], const double (&g)[3], double e,
                                             double kappa) {
    const double J[6] = {p[1] * g[2] - p[2] * g[1], p[2] * g[0] - p[0] * g[2], p[0] * g[1] - p[1] * g[0], g[0], g[1], g[2]};
    gn_add_row(s, J, e, gn_weight(kappa, e * e));
}

// the sums of a block of 256 threads -> partial[blk * GN_NSUM_PAD + k]; all threads call it.  LOW is the butterfly's lowest
// offset: 4 where lanes 1..3 of a quad hold zeros (the rows sit in lane 0), 1 where every lane may hold a row
template <int LOW = 4>
__device__ __forceinline__ void gn_block_reduce(const double (&s)[GN_NSUM], double *partial, int blk) {
    __shared__ double sred[4][GN_NSUM];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < GN_NSUM; ++k) {
        double v = s[k];
#pragma unroll
        for (int off = 32; off >= LOW; off >>= 1) v += __shfl_xor(v, off, 64);
        if (lane == 0) sred[w][k] = v;
    }
    __syncthreads();
    if (threadIdx.x < GN_NSUM)
        partial[(size_t)blk * GN_NSUM_PAD + threadIdx.x] =
            (sred[0][threadIdx.x] + sred[1][threadIdx.x]) + (sred[2][threadIdx.x] + sred[3][threadIdx.x]);
}

// the head of a solve kernel (one wave): S (in LDS) = the partials of blocks 0 .. nblk-1 added in that order, and row k of dbg_system
__device__ __forceinline__ void gn_sum_partials(const double *partial, int nblk, double *S, double *dbg_system, size_t k) {
    const int lane = threadIdx.x;
    if (lane < GN_NSUM) {
        double v = 0.0;
        for (int b = 0; b < nblk; ++b) v += partial[(size_t)b * GN_NSUM_PAD + lane];
        S[lane] = v;
        if (dbg_system) dbg_system[k * GN_NSUM + lane] = v;
    }
    __syncthreads();
}

// problem k of a batch to its start values: pose <- init with the last row 0 0 0 1, the results; gn_zero_system: its debug row
__device__ __forceinline__ void gn_init_problem(size_t k, const double *init, double *pose, float *fitness, float *rmse,
                                                int32_t *iterations, int32_t *status) {
    for (int i = 0; i < 12; ++i) pose[k * 16 + i] = init[k * 16 + i];
    pose[k * 16 + 12] = 0.0, pose[k * 16 + 13] = 0.0, pose[k * 16 + 14] = 0.0, pose[k * 16 + 15] = 1.0;
    fitness[k] = 0.f, rmse[k] = 0.f, iterations[k] = 0, status[k] = DPM_ICP_MAX_ITER;
}

__device__ __forceinline__ void gn_zero_system(size_t k, double *dbg_system) {
    if (dbg_system)
        for (int i = 0; i < GN_NSUM; ++i) dbg_system[k * GN_NSUM + i] = 0.0;
}

__device__ __forceinline__ bool finite_d(double v) { return fabs(v) < 1e300; }   // false for Inf and NaN

// fitness / rmse / iterations / status are the arrays of a batch and k the problem's place in them
__device__ __forceinline__ void gn_solve_step(const double *S, int n_src, double *pose, float *fitness, float *rmse,
                                              int32_t *iterations, int32_t *status, int k_out, int *done, double tol_rot,
                                              double tol_trans) {
    const double cnt = S[27], rss = S[28];
    if (!(cnt >= 1.0)) {
        fitness[k_out] = 0.f, rmse[k_out] = 0.f, status[k_out] = DPM_ICP_NO_MATCH, *done = 1;
        return;
    }
    fitness[k_out] = (float)(cnt / (double)max(n_src, 1));
    const double ms = rss / cnt;
    rmse[k_out] = finite_d(ms) && ms >= 0.0 ? (float)sqrt(ms) : 0.f;
    double Hm[6][6], L[6][6], g[6];
    {
        int k = 0;
        for (int i = 0; i < 6; ++i)
            for (int j = i; j < 6; ++j) Hm[i][j] = Hm[j][i] = S[k++];
        for (int i = 0; i < 6; ++i) g[i] = S[21 + i];
    }
    bool ok = cnt >= 6.0;
    for (int k = 0; k < GN_NSUM && ok; ++k) ok = finite_d(S[k]);
    const double bm[2] = {fmax(fmax(Hm[0][0], Hm[1][1]), Hm[2][2]), fmax(fmax(Hm[3][3], Hm[4][4]), Hm[5][5])};
    for (int k = 0; k < 6 && ok; ++k) {
        double d = Hm[k][k];
        for (int m = 0; m < k; ++m) d -= L[k][m] * L[k][m];
        if (!(d > GN_PIV_EPS * bm[k / 3])) {
            ok = false;
            break;
        }
        L[k][k] = sqrt(d);
        for (int i = k + 1; i < 6; ++i) {
            double v = Hm[i][k];
            for (int m = 0; m < k; ++m) v -= L[i][m] * L[k][m];
            L[i][k] = v / L[k][k];
        }
    }
    double x[6];
    if (ok) {
        double yv[6];
        for (int i = 0; i < 6; ++i) {   // L y = -g
            double v = -g[i];
            for (int m = 0; m < i; ++m) v -= L[i][m] * yv[m];
            yv[i] = v / L[i][i];
        }
        for (int i = 5; i >= 0; --i) {  // L^T x = y
            double v = yv[i];
            for (int m = i + 1; m < 6; ++m) v -= L[m][i] * x[m];
            x[i] = v / L[i][i];
        }
        for (int i = 0; i < 6; ++i) ok = ok && finite_d(x[i]);
    }
    if (!ok) {   // the pose stays at its last good value
        status[k_out] = DPM_ICP_SINGULAR, *done = 1;
        return;
    }
    const double th2 = (x[0] * x[0] + x[1] * x[1]) + x[2] * x[2], th = sqrt(th2);
    double a, b;   // exp(w) = I + a K + b K^2
    if (th < 1e-8) a = 1.0, b = 0.5;
    else a = sin(th) / th, b = (1.0 - cos(th)) / th2;
    const double K[3][3] = {{0.0, -x[2], x[1]}, {x[2], 0.0, -x[0]}, {-x[1], x[0], 0.0}};
    double E[3][3];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            double k2 = 0.0;
            for (int m = 0; m < 3; ++m) k2 += K[i][m] * K[m][j];
            E[i][j] = (i == j ? 1.0 : 0.0) + a * K[i][j] + b * k2;
        }
    double out[12];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 4; ++j) {
            double v = 0.0;
            for (int m = 0; m < 3; ++m) v += E[i][m] * pose[m * 4 + j];
            out[i * 4 + j] = j == 3 ? v + x[3 + i] : v;
        }
    for (int k = 0; k < 12; ++k) ok = ok && finite_d(out[k]);
    if (!ok) {
        status[k_out] = DPM_ICP_SINGULAR, *done = 1;
        return;
    }
    for (int k = 0; k < 12; ++k) pose[k] = out[k];
    iterations[k_out] += 1;
    const double tr = sqrt((x[3] * x[3] + x[4] * x[4]) + x[5] * x[5]);
    if (th < tol_rot && tr < tol_trans) status[k_out] = DPM_ICP_CONVERGED, *done = 1;
}
