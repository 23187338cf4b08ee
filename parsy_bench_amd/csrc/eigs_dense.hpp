// The small dense work of parsy_eigs_device (eigs.hpp), on the host in plain C++: a cyclic Jacobi eigensolver for the
// projected matrix (order <= 128), and the Cholesky factor and triangular inverse of a block's Gram matrix (order <= 16)
// with the rule that drops a dependent column.  No LAPACK, no device, nothing of the plan: tests/eigs_dense_check.cpp
// includes this header alone.  Every loop runs in a fixed order, so the same input gives the same bits.
#pragma once
#include <algorithm>
#include <cmath>
#include <numeric>
#include <vector>

namespace parsy {

constexpr int kEigsMaxBasis = 128;   // largest basis: the order of the Jacobi solver's matrix
constexpr int kEigsMaxBlock = 16;    // largest block: the order of a Gram matrix that is factored
// A column of a block whose pivot, in the Gram matrix scaled to unit diagonal, falls below this is dropped: the pivot is
// the squared sine of the column's angle to the ones before it, and below sqrt(u) = 2^-26.5 a second pass of
// Cholesky-QR no longer restores orthogonality to working precision (Yamamoto et al., ETNA 44, 2015: CholeskyQR2 needs
// kappa(T) <~ u^-1/2).
constexpr double kEigsDropPivot = 0x1p-26;
constexpr int kEigsJacobiSweeps = 60;

// Eigen-decomposition G = S diag(theta) S' of the symmetric G (order m, column-major, leading dimension m; both
// triangles are read, G is destroyed): theta ascending, S (m x m, column-major) orthogonal.  Cyclic Jacobi by rows with
// the rotation of Golub & Van Loan's sym.schur2; an entry is rotated away while it is above u ||G||_F / m, so the
// off-diagonal part ends below u ||G||_F.  Returns the sweeps taken, -1 when kEigsJacobiSweeps did not suffice (or G
// holds a NaN).
inline int eigs_jacobi(int m, double* G, double* theta, double* S) {
    for (int j = 0; j < m; ++j)
        for (int i = 0; i < m; ++i) S[(size_t)j * m + i] = i == j ? 1.0 : 0.0;
    double fro = 0.0;
    for (int e = 0; e < m * m; ++e) fro += G[e] * G[e];
    if (!(fro == fro)) return -1;
    const double small = 0x1p-53 * std::sqrt(fro) / std::max(m, 1);
    int sweeps = 0;
    for (;; ++sweeps) {
        bool rotated = false;
        if (sweeps == kEigsJacobiSweeps) return -1;
        for (int p = 0; p < m - 1; ++p)
            for (int q = p + 1; q < m; ++q) {
                const double gpq = G[(size_t)q * m + p];
                if (!(std::fabs(gpq) > small)) continue;
                rotated = true;
                const double tau = (G[(size_t)q * m + q] - G[(size_t)p * m + p]) / (2.0 * gpq);
                const double t = (tau >= 0.0 ? 1.0 : -1.0) / (std::fabs(tau) + std::sqrt(1.0 + tau * tau));
                const double c = 1.0 / std::sqrt(1.0 + t * t), s = t * c;
                G[(size_t)p * m + p] -= t * gpq;
                G[(size_t)q * m + q] += t * gpq;
                G[(size_t)q * m + p] = G[(size_t)p * m + q] = 0.0;
                for (int r = 0; r < m; ++r) {
                    if (r != p && r != q) {
                        const double grp = G[(size_t)p * m + r], grq = G[(size_t)q * m + r];
                        G[(size_t)p * m + r] = G[(size_t)r * m + p] = c * grp - s * grq;
                        G[(size_t)q * m + r] = G[(size_t)r * m + q] = s * grp + c * grq;
                    }
                    const double srp = S[(size_t)p * m + r], srq = S[(size_t)q * m + r];
                    S[(size_t)p * m + r] = c * srp - s * srq;
                    S[(size_t)q * m + r] = s * srp + c * srq;
                }
            }
        if (!rotated) break;
    }
    // ascending, equal values in the order Jacobi left them
    std::vector<int> order((size_t)m);
    std::iota(order.begin(), order.end(), 0);
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return G[(size_t)a * m + a] < G[(size_t)b * m + b]; });
    std::vector<double> sorted((size_t)m * m);
    for (int j = 0; j < m; ++j) {
        theta[j] = G[(size_t)order[(size_t)j] * m + order[(size_t)j]];
        std::copy(S + (size_t)order[(size_t)j] * m, S + (size_t)order[(size_t)j] * m + m, sorted.begin() + (size_t)j * m);
    }
    std::copy(sorted.begin(), sorted.end(), S);
    return sweeps;
}

enum EigsCholResult { kEigsCholOk = 0, kEigsCholNotSpd = -2 };

// S[:, :c] <- S[:, :c] R^-1 with R'R = S[:, :c]' W S[:, :c] (Cholesky): the first c columns of S (m x m, column-major)
// come out orthonormal in the inner product of W (m x m, symmetric, column-major, both triangles read).  W = V'MV of a
// basis whose M-orthonormality has drifted by rounding -- every restart multiplies V by a computed S -- so R = I + O(the
// drift) and the columns move by that much: V S[:, :c] is M-orthonormal again to the accuracy of W.
inline int eigs_w_orthonormalise(int m, int c, const double* W, double* S) {
    std::vector<double> WS((size_t)m * c), R((size_t)c * c, 0.0);
    for (int j = 0; j < c; ++j)
        for (int i = 0; i < m; ++i) {
            double v = 0.0;
            for (int t = 0; t < m; ++t) v += W[(size_t)t * m + i] * S[(size_t)j * m + t];
            WS[(size_t)j * m + i] = v;
        }
    for (int j = 0; j < c; ++j)
        for (int i = 0; i <= j; ++i) {
            double v = 0.0;
            for (int t = 0; t < m; ++t) v += S[(size_t)i * m + t] * WS[(size_t)j * m + t];
            for (int t = 0; t < i; ++t) v -= R[(size_t)i * c + t] * R[(size_t)j * c + t];   // (R[t, i] is R[i * c + t])
            if (i < j) {
                R[(size_t)j * c + i] = v / R[(size_t)i * c + i];
            } else {
                if (!(v > 0.0)) return kEigsCholNotSpd;
                R[(size_t)j * c + j] = std::sqrt(v);
            }
        }
    for (int j = 0; j < c; ++j)
        for (int r = 0; r < m; ++r) {
            double x = S[(size_t)j * m + r];
            for (int i = 0; i < j; ++i) x -= S[(size_t)i * m + r] * R[(size_t)j * c + i];
            S[(size_t)j * m + r] = x / R[(size_t)j * c + j];
        }
    return kEigsCholOk;
}

// One pass of Cholesky-QR on the Gram matrix G = T' M T of a block T of b columns (column-major, leading dimension b;
// the lower triangle is read): C (b x *kept, column-major, leading dimension b) with T C M-orthonormal to the accuracy
// of the pass.  scaled (the first pass): G is scaled to unit diagonal first and a column whose pivot falls below
// kEigsDropPivot is dropped -- it gets no column of C and a zero row -- and counted in *dropped; a diagonal entry that
// is not positive, or a pivot below -kEigsDropPivot, says that M is not positive definite.  Otherwise (the second pass)
// every pivot must be positive.
inline int eigs_chol_rinv(int b, const double* G, bool scaled, double* C, int* kept, int* dropped) {
    double scale[kEigsMaxBlock], R[kEigsMaxBlock * kEigsMaxBlock], Ri[kEigsMaxBlock * kEigsMaxBlock];
    int keep[kEigsMaxBlock], nk = 0;
    *kept = 0;
    for (int j = 0; j < b; ++j) {
        const double d = G[(size_t)j * b + j];
        if (scaled && !(d > 0.0)) return kEigsCholNotSpd;
        scale[j] = scaled ? 1.0 / std::sqrt(d) : 1.0;
    }
    auto g = [&](int i, int j) { return G[(size_t)std::min(i, j) * b + std::max(i, j)] * scale[i] * scale[j]; };
    // R (upper, nk x nk over the kept columns, leading dimension kEigsMaxBlock) column by column
    for (int j = 0; j < b; ++j) {
        double col[kEigsMaxBlock], piv = scaled ? 1.0 : g(j, j);
        for (int a = 0; a < nk; ++a) {
            double v = g(keep[a], j);
            for (int c = 0; c < a; ++c) v -= R[a * kEigsMaxBlock + c] * col[c];
            col[a] = v / R[a * kEigsMaxBlock + a];
        }
        for (int a = 0; a < nk; ++a) piv -= col[a] * col[a];
        if (scaled) {
            if (!(piv >= -kEigsDropPivot)) return kEigsCholNotSpd;
            if (piv < kEigsDropPivot) {
                *dropped += 1;
                continue;
            }
        } else if (!(piv > 0.0)) {
            return kEigsCholNotSpd;
        }
        for (int a = 0; a < nk; ++a) R[nk * kEigsMaxBlock + a] = col[a];   // column nk of R, rows 0 .. nk - 1
        R[nk * kEigsMaxBlock + nk] = std::sqrt(piv);
        keep[nk++] = j;
    }
    // Ri = R^-1 (upper), column by column: R Ri = I
    for (int j = 0; j < nk; ++j)
        for (int i = nk - 1; i >= 0; --i) {
            double v = i == j ? 1.0 : 0.0;
            for (int c = i + 1; c <= j; ++c) v -= R[c * kEigsMaxBlock + i] * Ri[j * kEigsMaxBlock + c];
            Ri[j * kEigsMaxBlock + i] = i > j ? 0.0 : v / R[i * kEigsMaxBlock + i];
        }
    for (int j = 0; j < nk; ++j) {
        for (int i = 0; i < b; ++i) C[(size_t)j * b + i] = 0.0;
        for (int a = 0; a <= j; ++a) C[(size_t)j * b + keep[a]] = scale[keep[a]] * Ri[j * kEigsMaxBlock + a];
    }
    *kept = nk;
    return kEigsCholOk;
}

}  // namespace parsy
