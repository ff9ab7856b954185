// The Gauss-Newton step of the registration kernels (icp.hip, local_map.hip), run by ONE lane on the 29 summed values
// S = [H upper triangle row-major (21), g (6), matches, sum of squared residuals]:  fitness and rmse, H x = -g by Cholesky
// with a pivot test, the step x = (w, v) composed onto the pose as pose <- [exp(w) | v] o pose (Rodrigues rotation, the
// translation taken as it is), the stop rule and the status.  No match: NO_MATCH; a system that cannot be solved, or a
// step / pose that is no number: SINGULAR -- both leave the pose at its last good value and set *done.  Everything fp64.
#pragma once
#include "dpm_common.h"

constexpr int GN_NSUM = 29;
constexpr double GN_PIV_EPS = 1e-9;  // a Cholesky pivot below GN_PIV_EPS * (largest diagonal entry of its 3x3 block) is singular

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
