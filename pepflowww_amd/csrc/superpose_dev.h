// fp64 superposition helpers shared by superpose.hip (one wave per pair) and tm_score.hip (one lane per seed): the wave all-reduce,
// the one-sided Jacobi SVD of a 3x3 matrix and the Kabsch rotation built on it.
#pragma once
#include <hip/hip_runtime.h>

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);    // commutative pairs: every lane ends with the same bits
    return v;
}

// one-sided Jacobi SVD of a 3x3 matrix: A <- A V with orthogonal columns (A V = U Sigma), V accumulated; columns sorted by norm
__device__ inline void svd3_jacobi(double A[3][3], double V[3][3], double sig[3]) {
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) V[i][j] = i == j ? 1.0 : 0.0;
    for (int sweep = 0; sweep < 20; ++sweep) {
        bool rotated = false;
#pragma unroll
        for (int pq = 0; pq < 3; ++pq) {
            const int p = pq == 2 ? 1 : 0, q = pq == 0 ? 1 : 2;
            double al = 0.0, be = 0.0, ga = 0.0;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                al += A[k][p] * A[k][p];
                be += A[k][q] * A[k][q];
                ga += A[k][p] * A[k][q];
            }
            if (ga == 0.0 || fabs(ga) <= 1e-15 * sqrt(al * be)) continue;
            rotated = true;
            const double zeta = (be - al) / (2.0 * ga);
            const double t = (zeta >= 0.0 ? 1.0 : -1.0) / (fabs(zeta) + hypot(1.0, zeta));
            const double c = 1.0 / sqrt(1.0 + t * t), s = c * t;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const double ap = A[k][p], aq = A[k][q];
                A[k][p] = c * ap - s * aq;
                A[k][q] = s * ap + c * aq;
                const double vp = V[k][p], vq = V[k][q];
                V[k][p] = c * vp - s * vq;
                V[k][q] = s * vp + c * vq;
            }
        }
        if (!rotated) break;
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) sig[k] = sqrt(A[0][k] * A[0][k] + A[1][k] * A[1][k] + A[2][k] * A[2][k]);
    auto swapcol = [&](int p, int q) {
        const double t = sig[p]; sig[p] = sig[q]; sig[q] = t;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            double u = A[k][p]; A[k][p] = A[k][q]; A[k][q] = u;
            u = V[k][p]; V[k][p] = V[k][q]; V[k][q] = u;
        }
    };
    if (sig[0] < sig[1]) swapcol(0, 1);
    if (sig[0] < sig[2]) swapcol(0, 2);
    if (sig[1] < sig[2]) swapcol(1, 2);
}

// The rotation R that maximises tr(R S) for the centred cross terms S = X^T Y (y ~ R x), and that optimum lam.  Returns true where
// S has numerical rank < 2 (s2 <= 1e-6 s1): the rotation is not unique, R = identity, lam stays exact.
// S = U Sigma V^T.  The minimiser of sum |r x - y|^2 over O(3) maximises tr(r S): r = V U^T; over SO(3) the third singular
// pair carries sign(det S).  U is completed as a proper frame (u3 = u1 x u2), V made proper; then S = U diag(s1, s2, s3') V^T
// with s3' = u3 . (S v3) signed, and the optimum of tr(r S) is s1 + s2 + s3' (proper) or s1 + s2 + |s3'| (reflection allowed).
__device__ __forceinline__ bool kabsch_rotation(const double S[3][3], bool allow_reflection, double R[3][3], double& lam) {
    double A[3][3], V[3][3], sig[3];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) A[r][c] = S[r][c];
    svd3_jacobi(A, V, sig);
    const bool degenerate = !(sig[0] > 0.0) || sig[1] <= 1e-6 * sig[0];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) R[r][c] = r == c ? 1.0 : 0.0;
    if (degenerate) {
        lam = sig[0] + sig[1] + sig[2];                             // rank <= 1: every sign choice reaches the same optimum
    } else {
        double U[3][3];
#pragma unroll
        for (int k = 0; k < 3; ++k) U[k][0] = A[k][0] / sig[0];
        const double d01 = U[0][0] * A[0][1] + U[1][0] * A[1][1] + U[2][0] * A[2][1];
        double w[3], wn = 0.0;
#pragma unroll
        for (int k = 0; k < 3; ++k) { w[k] = A[k][1] - d01 * U[k][0]; wn += w[k] * w[k]; }
        wn = sqrt(wn);
#pragma unroll
        for (int k = 0; k < 3; ++k) U[k][1] = w[k] / wn;
        U[0][2] = U[1][0] * U[2][1] - U[2][0] * U[1][1];
        U[1][2] = U[2][0] * U[0][1] - U[0][0] * U[2][1];
        U[2][2] = U[0][0] * U[1][1] - U[1][0] * U[0][1];
        double s3 = U[0][2] * A[0][2] + U[1][2] * A[1][2] + U[2][2] * A[2][2];
        const double detV = V[0][0] * (V[1][1] * V[2][2] - V[1][2] * V[2][1]) - V[0][1] * (V[1][0] * V[2][2] - V[1][2] * V[2][0]) +
                            V[0][2] * (V[1][0] * V[2][1] - V[1][1] * V[2][0]);
        if (detV < 0.0) {
#pragma unroll
            for (int k = 0; k < 3; ++k) V[k][2] = -V[k][2];
            s3 = -s3;
        }
        lam = sig[0] + sig[1] + s3;
        const double d = (allow_reflection && s3 < 0.0) ? -1.0 : 1.0;
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int c = 0; c < 3; ++c) R[r][c] = V[r][0] * U[c][0] + V[r][1] * U[c][1] + d * V[r][2] * U[c][2];
    }
    return degenerate;
}
