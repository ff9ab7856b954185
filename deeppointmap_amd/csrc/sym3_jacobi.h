// Cyclic Jacobi of a symmetric 3 x 3 matrix in fp64, at most 12 sweeps: A becomes diagonal (the eigenvalues, in no order), the
// columns of V -- the identity on entry -- the eigenvectors.  Used by the point normals (knn.hip) and the voxel planes
// (local_map.hip); what they do with the eigenpairs is theirs.
#pragma once
#include "dpm_common.h"

__device__ __forceinline__ void sym3_jacobi(double (&A)[3][3], double (&V)[3][3]) {
    for (int sweep = 0; sweep < 12; ++sweep) {
        const double off = fabs(A[0][1]) + fabs(A[0][2]) + fabs(A[1][2]);
        if (off <= 1e-300 || off <= 1e-18 * (fabs(A[0][0]) + fabs(A[1][1]) + fabs(A[2][2]))) break;
        for (int p = 0; p < 2; ++p)
            for (int r = p + 1; r < 3; ++r) {
                if (A[p][r] == 0.0) continue;
                const double theta = (A[r][r] - A[p][p]) / (2.0 * A[p][r]);
                const double t = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                const double cs_ = 1.0 / sqrt(t * t + 1.0), sn = t * cs_;
                for (int k = 0; k < 3; ++k) {  // A <- A J
                    const double akp = A[k][p], akr = A[k][r];
                    A[k][p] = cs_ * akp - sn * akr, A[k][r] = sn * akp + cs_ * akr;
                }
                for (int k = 0; k < 3; ++k) {  // A <- J^T A,  V <- V J
                    const double apk = A[p][k], ark = A[r][k];
                    A[p][k] = cs_ * apk - sn * ark, A[r][k] = sn * apk + cs_ * ark;
                    const double vkp = V[k][p], vkr = V[k][r];
                    V[k][p] = cs_ * vkp - sn * vkr, V[k][r] = sn * vkp + cs_ * vkr;
                }
            }
    }
}
