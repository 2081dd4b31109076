// Eigen-decomposition of a symmetric 3x3 matrix by cyclic Jacobi in fp64: the one routine behind the kNN-PCA normals
// (knn_normals.hip: smallest_eigvec) and the moving-least-squares frames (mls.hip).
#pragma once
#include "common.h"

// On return the diagonal of a holds the eigenvalues (in no particular order) and column j of v the unit eigenvector of a[j][j].
__device__ __forceinline__ void jacobi_eig3(double a[3][3], double v[3][3]) {
    v[0][0] = 1; v[0][1] = 0; v[0][2] = 0;
    v[1][0] = 0; v[1][1] = 1; v[1][2] = 0;
    v[2][0] = 0; v[2][1] = 0; v[2][2] = 1;
    for (int sweep = 0; sweep < 12; ++sweep) {
        const double off = fabs(a[0][1]) + fabs(a[0][2]) + fabs(a[1][2]);
        if (off < 1e-30) break;
        for (int p = 0; p < 2; ++p)
            for (int q = p + 1; q < 3; ++q) {
                if (fabs(a[p][q]) < 1e-300) continue;
                const double theta = (a[q][q] - a[p][p]) / (2.0 * a[p][q]);
                const double t = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                const double cs = 1.0 / sqrt(t * t + 1.0), sn = t * cs;
                for (int k = 0; k < 3; ++k) {
                    const double akp = a[k][p], akq = a[k][q];
                    a[k][p] = cs * akp - sn * akq;
                    a[k][q] = sn * akp + cs * akq;
                }
                for (int k = 0; k < 3; ++k) {
                    const double apk = a[p][k], aqk = a[q][k];
                    a[p][k] = cs * apk - sn * aqk;
                    a[q][k] = sn * apk + cs * aqk;
                }
                for (int k = 0; k < 3; ++k) {
                    const double vkp = v[k][p], vkq = v[k][q];
                    v[k][p] = cs * vkp - sn * vkq;
                    v[k][q] = sn * vkp + cs * vkq;
                }
            }
    }
}
