// svd3.h — the fp64 3x3 "Kabsch rotation" R = V diag(1, 1, det(V U^T)) U^T of S = U diag(s) V^T as a device function, shared by
// kabsch.hip (one thread per cross-covariance of the weighted-Kabsch fit) and rigid_icp.hip (one fit per ICP iteration), and the
// symmetric eigen-solve of ground_plane.hip (ogc_sym_eig3, at the end) on the same Jacobi rotation.
//
// Cyclic Jacobi eigen-solve of S^T S (six sweeps; three reach machine precision for 3x3), U recovered column by column
// (with Gram-Schmidt completion for vanishing singular values), and the product formed from the two leading singular pairs
// and their cross products, which makes it independent of the sign conventions of the third pair: for det(V U^T) < 0 this is
// the SVD solution with the last row of V^T negated.  The arithmetic and its order are pinned: kabsch_rotation_kernel's
// output bits are watched by tests.
#pragma once
#include "ogc_common.h"

namespace {

__device__ inline void jacobi_rot(double (&A)[3][3], double (&V)[3][3], int p, int q) {
    if (A[p][q] == 0.0) return;
    const double theta = (A[q][q] - A[p][p]) / (2.0 * A[p][q]);
    const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
    const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
    for (int k = 0; k < 3; ++k) { // A <- A J
        const double akp = A[k][p], akq = A[k][q];
        A[k][p] = c * akp - s * akq;
        A[k][q] = s * akp + c * akq;
    }
    for (int k = 0; k < 3; ++k) { // A <- J^T A
        const double apk = A[p][k], aqk = A[q][k];
        A[p][k] = c * apk - s * aqk;
        A[q][k] = s * apk + c * aqk;
    }
    for (int k = 0; k < 3; ++k) { // V <- V J
        const double vkp = V[k][p], vkq = V[k][q];
        V[k][p] = c * vkp - s * vkq;
        V[k][q] = s * vkp + c * vkq;
    }
}

__device__ inline void cross3(const double (&a)[3], const double (&b)[3], double (&o)[3]) {
    o[0] = a[1] * b[2] - a[2] * b[1];
    o[1] = a[2] * b[0] - a[0] * b[2];
    o[2] = a[0] * b[1] - a[1] * b[0];
}

// S scaled to max |entry| = 1 by the caller (finite, not all zero).  false: rank 0, R untouched (cannot happen for such an S).
__device__ inline bool ogc_kabsch3(const double (&S)[3][3], double (&R)[3][3]) {
    // A = S^T S, eigen-decomposition A = V diag(l) V^T
    double A[3][3], V[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) A[r][c] = S[0][r] * S[0][c] + S[1][r] * S[1][c] + S[2][r] * S[2][c];
    for (int sweep = 0; sweep < 6; ++sweep) {
        jacobi_rot(A, V, 0, 1);
        jacobi_rot(A, V, 0, 2);
        jacobi_rot(A, V, 1, 2);
    }
    // sort eigenpairs descending
    int ord[3] = {0, 1, 2};
    for (int a = 0; a < 2; ++a)
        for (int b = a + 1; b < 3; ++b)
            if (A[ord[b]][ord[b]] > A[ord[a]][ord[a]]) { const int t = ord[a]; ord[a] = ord[b]; ord[b] = t; }
    double Vs[3][3], sig[3];
    for (int j = 0; j < 3; ++j) {
        sig[j] = sqrt(fmax(A[ord[j]][ord[j]], 0.0));
        for (int r = 0; r < 3; ++r) Vs[r][j] = V[r][ord[j]];
    }
    // make V a proper basis (det +1) — the reflection is handled by the diag(1,1,det) factor below, which only
    // depends on det(V) det(U), so flipping a V column together with the matching U column changes nothing.
    double U[3][3];
    const double tiny = 1e-12 * fmax(sig[0], 1e-300);
    int rank = 0;
    for (int j = 0; j < 3; ++j) {
        double u[3];
        for (int r = 0; r < 3; ++r) u[r] = S[r][0] * Vs[0][j] + S[r][1] * Vs[1][j] + S[r][2] * Vs[2][j];
        if (sig[j] > tiny) {
            // re-orthogonalise against previous columns (guards tiny sigma ratios), then normalise
            for (int p = 0; p < j; ++p) {
                const double dp = u[0] * U[0][p] + u[1] * U[1][p] + u[2] * U[2][p];
                for (int r = 0; r < 3; ++r) u[r] -= dp * U[r][p];
            }
            const double nrm = sqrt(u[0] * u[0] + u[1] * u[1] + u[2] * u[2]);
            if (nrm > tiny) {
                for (int r = 0; r < 3; ++r) U[r][j] = u[r] / nrm;
                rank = j + 1;
                continue;
            }
        }
        break;
    }
    if (rank == 0) return false;
    if (rank == 1) { // pick any unit vector orthogonal to U[:,0]
        double a[3] = {U[0][0], U[1][0], U[2][0]}, e[3] = {0, 0, 0}, o[3];
        const int m = fabs(a[0]) <= fabs(a[1]) && fabs(a[0]) <= fabs(a[2]) ? 0 : (fabs(a[1]) <= fabs(a[2]) ? 1 : 2);
        e[m] = 1.0;
        cross3(a, e, o);
        const double nrm = sqrt(o[0] * o[0] + o[1] * o[1] + o[2] * o[2]);
        for (int r = 0; r < 3; ++r) U[r][1] = o[r] / nrm;
        rank = 2;
    }
    {   // third columns: with d = det(V U^T) the product V diag(1,1,d) U^T equals
        // v1 u1^T + v2 u2^T + (v1 x v2)(u1 x u2)^T  — independent of the sign conventions of v3 / u3.
        double v1[3] = {Vs[0][0], Vs[1][0], Vs[2][0]}, v2[3] = {Vs[0][1], Vs[1][1], Vs[2][1]}, v3[3];
        double u1[3] = {U[0][0], U[1][0], U[2][0]}, u2[3] = {U[0][1], U[1][1], U[2][1]}, u3[3];
        cross3(v1, v2, v3);
        cross3(u1, u2, u3);
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c) R[r][c] = v1[r] * u1[c] + v2[r] * u2[c] + v3[r] * u3[c];
    }
    return true;
}

template <int A, int B> // eigenpair B in front of eigenpair A when its eigenvalue is larger
__device__ inline void eig_order(double (&lam)[3], double (&V)[3][3]) {
    if (lam[B] > lam[A]) {
        const double t = lam[A]; lam[A] = lam[B]; lam[B] = t;
        for (int r = 0; r < 3; ++r) { const double v = V[r][A]; V[r][A] = V[r][B]; V[r][B] = v; }
    }
}

// Eigen-decomposition of a symmetric S (finite; the caller scales it to max |entry| = 1): eigenvalues descending in lam, the
// matching unit eigenvectors in the columns of V.  The same six cyclic Jacobi sweeps as above (ground_plane.hip: the plane
// normal is column 2).  An exactly zero off-diagonal entry is left alone, so a scatter with exact zero rows keeps exact zero
// eigenvalues.
__device__ inline void ogc_sym_eig3(const double (&S)[3][3], double (&lam)[3], double (&V)[3][3]) {
    double A[3][3], W[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) A[r][c] = S[r][c];
    for (int sweep = 0; sweep < 6; ++sweep) {
        jacobi_rot(A, W, 0, 1);
        jacobi_rot(A, W, 0, 2);
        jacobi_rot(A, W, 1, 2);
    }
    for (int j = 0; j < 3; ++j) {
        lam[j] = A[j][j];
        for (int r = 0; r < 3; ++r) V[r][j] = W[r][j];
    }
    // sorted with constant indices only: an array indexed through a run-time permutation leaves the registers
    eig_order<0, 1>(lam, V);
    eig_order<0, 2>(lam, V);
    eig_order<1, 2>(lam, V);
}

} // namespace
