// The small dense helpers of the eigensolver (csrc/eigs_dense.hpp) on their own, under the host sanitizers
// (tests/test_eigs_host.py builds and runs this file).
//
// Jacobi: for G = S Theta S' computed with unit roundoff u = 2^-53, a rotation perturbs the two rows and columns it
// touches by a relative 6 u at most (Golub & Van Loan, Matrix Computations 4th ed., section 5.1.10: a computed Givens
// update is that of an exactly orthogonal matrix up to O(u)), an entry of S is touched m - 1 times per sweep, and the
// loop stops with the off-diagonal part below u ||G||_F.  Errors add at worst linearly, so with s sweeps
//     ||S'S - I||_F       <= 8 (s + 1) m u sqrt(m)   and   ||G S - S Theta||_F <= 8 (s + 1) m u ||G||_F
// are the bounds checked here (section 8.5.5 of the same book states the m u ||G|| form of the result).
// Cholesky-QR: C' G C = I up to cond(G) u for the kept columns; a pivot that is not positive is reported.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "eigs_dense.hpp"

namespace {

int failures = 0;
const double u = 0x1p-53;

void expect(bool ok, const char* what, double got, double bound) {
    if (!ok) {
        std::printf("FAIL %s: %.3e against %.3e\n", what, got, bound);
        failures += 1;
    }
}

double rnd(unsigned long long* st) {   // uniform in (-1, 1), a fixed sequence
    *st = *st * 6364136223846793005ull + 1442695040888963407ull;
    return (double)((*st >> 11) & ((1ull << 52) - 1)) / (double)(1ull << 51) - 1.0;
}

void check_jacobi(const char* name, int m, const std::vector<double>& G0) {
    std::vector<double> G(G0), theta((size_t)m), S((size_t)m * m);
    const int sweeps = parsy::eigs_jacobi(m, G.data(), theta.data(), S.data());
    expect(sweeps >= 0, name, sweeps, 0);
    if (sweeps < 0) return;
    double fro = 0, res = 0, orth = 0;
    for (double v : G0) fro += v * v;
    fro = std::sqrt(fro);
    for (int j = 0; j < m; ++j)
        for (int i = 0; i < m; ++i) {
            long double gs = 0, ss = 0;
            for (int k = 0; k < m; ++k) {
                gs += (long double)G0[(size_t)k * m + i] * S[(size_t)j * m + k];
                ss += (long double)S[(size_t)i * m + k] * S[(size_t)j * m + k];
            }
            const double r = (double)(gs - (long double)S[(size_t)j * m + i] * theta[(size_t)j]);
            const double o = (double)(ss - (i == j ? 1.0L : 0.0L));
            res += r * r, orth += o * o;
        }
    res = std::sqrt(res), orth = std::sqrt(orth);
    const double c = 8.0 * (sweeps + 1) * m * u;
    expect(res <= c * fro, name, res, c * fro);
    expect(orth <= c * std::sqrt((double)m), name, orth, c * std::sqrt((double)m));
    for (int j = 1; j < m; ++j) expect(theta[(size_t)j - 1] <= theta[(size_t)j], name, theta[(size_t)j - 1], theta[(size_t)j]);
    std::printf("jacobi %-12s m=%3d sweeps=%2d residual/bound=%.3f orthogonality/bound=%.3f\n", name, m, sweeps,
                fro > 0 ? res / (c * fro) : 0.0, orth / (c * std::sqrt((double)m)));
}

std::vector<double> random_symmetric(int m, unsigned long long seed) {
    std::vector<double> G((size_t)m * m);
    for (int j = 0; j < m; ++j)
        for (int i = 0; i <= j; ++i) G[(size_t)j * m + i] = G[(size_t)i * m + j] = rnd(&seed);
    return G;
}

// I + v v': the eigenvalue 1 repeated m - 1 times
std::vector<double> repeated(int m, unsigned long long seed) {
    std::vector<double> v((size_t)m), G((size_t)m * m);
    for (double& x : v) x = rnd(&seed);
    for (int j = 0; j < m; ++j)
        for (int i = 0; i < m; ++i) G[(size_t)j * m + i] = (i == j ? 1.0 : 0.0) + v[(size_t)i] * v[(size_t)j];
    return G;
}

// the Gram matrix T'T of b columns of length len
std::vector<double> gram(const std::vector<double>& T, int len, int b) {
    std::vector<double> G((size_t)b * b);
    for (int j = 0; j < b; ++j)
        for (int i = 0; i < b; ++i) {
            double s = 0;
            for (int k = 0; k < len; ++k) s += T[(size_t)i * len + k] * T[(size_t)j * len + k];
            G[(size_t)j * b + i] = s;
        }
    return G;
}

void check_cholesky() {
    unsigned long long seed = 77;
    const int len = 40, b = 16;
    std::vector<double> T((size_t)len * b);
    for (double& x : T) x = rnd(&seed);
    for (int scaled = 0; scaled < 2; ++scaled) {
        if (scaled)   // (the unit diagonal takes this out)
            for (int k = 0; k < len; ++k) T[(size_t)5 * len + k] *= 1e6;
        const std::vector<double> G = gram(T, len, b);
        std::vector<double> C((size_t)b * b);
        int kept = 0, dropped = 0;
        const int rc = parsy::eigs_chol_rinv(b, G.data(), scaled != 0, C.data(), &kept, &dropped);
        expect(rc == 0 && kept == b && dropped == 0, "cholesky: full rank", kept, b);
        double worst = 0;
        for (int j = 0; j < kept; ++j)
            for (int i = 0; i < kept; ++i) {
                long double s = 0;
                for (int a = 0; a < b; ++a)
                    for (int c = 0; c < b; ++c) s += (long double)C[(size_t)i * b + a] * G[(size_t)c * b + a] * C[(size_t)j * b + c];
                worst = std::fmax(worst, std::fabs((double)(s - (i == j ? 1.0L : 0.0L))));
            }
        // cond(G) of 16 random columns of length 40 is below 1e3 (in the unit-diagonal scaling where one column is large)
        const double bound = 1e3 * b * u;
        expect(worst <= bound, "cholesky: C'GC - I", worst, bound);
        std::printf("cholesky scaled=%d |C'GC - I|max=%.3e bound %.3e\n", scaled, worst, bound);
    }
    {   // a copy of column 0 in column 2 and a zero-angle pair: the copy is dropped, the rest stays
        std::vector<double> T3((size_t)len * 4);
        for (double& x : T3) x = rnd(&seed);
        for (int k = 0; k < len; ++k) T3[(size_t)2 * len + k] = T3[(size_t)k];
        const std::vector<double> G = gram(T3, len, 4);
        std::vector<double> C(16);
        int kept = 0, dropped = 0;
        const int rc = parsy::eigs_chol_rinv(4, G.data(), true, C.data(), &kept, &dropped);
        expect(rc == 0 && kept == 3 && dropped == 1, "cholesky: a dependent column is dropped", kept, 3);
        for (int j = 0; j < kept; ++j) expect(C[(size_t)j * 4 + 2] == 0.0, "cholesky: the dropped column's row is zero", C[(size_t)j * 4 + 2], 0);
    }
    {   // not positive definite: a non-positive pivot is reported in both forms, and so is a non-positive diagonal
        const double G[4] = {1.0, 2.0, 2.0, 1.0}, Gd[4] = {1.0, 0.0, 0.0, -1.0};
        double C[4];
        int kept = 0, dropped = 0;
        expect(parsy::eigs_chol_rinv(2, G, false, C, &kept, &dropped) == parsy::kEigsCholNotSpd, "cholesky: pivot <= 0", 0, 0);
        expect(parsy::eigs_chol_rinv(2, G, true, C, &kept, &dropped) == parsy::kEigsCholNotSpd, "cholesky: scaled pivot < 0", 0, 0);
        expect(parsy::eigs_chol_rinv(2, Gd, true, C, &kept, &dropped) == parsy::kEigsCholNotSpd, "cholesky: diagonal <= 0", 0, 0);
        expect(dropped == 0, "cholesky: nothing dropped on the way", dropped, 0);
    }
}

}  // namespace

int main() {
    check_jacobi("order 1", 1, {3.5});
    check_jacobi("swap", 2, {0.0, 1.0, 1.0, 0.0});
    check_jacobi("twice 2", 2, {2.0, 0.0, 0.0, 2.0});
    check_jacobi("random", 17, random_symmetric(17, 1));
    check_jacobi("repeated", 17, repeated(17, 2));
    check_jacobi("random", 128, random_symmetric(128, 3));
    check_jacobi("repeated", 128, repeated(128, 4));
    check_jacobi("zero", 17, std::vector<double>(17 * 17, 0.0));
    {
        std::vector<double> G = random_symmetric(5, 9), theta(5), S(25);
        G[7] = std::nan("");
        expect(parsy::eigs_jacobi(5, G.data(), theta.data(), S.data()) == -1, "jacobi: NaN is reported", 0, 0);
    }
    {   // squaring up: the first 17 columns of a computed S against W = I + 1e-9 E (a drifted V'MV) come out W-orthonormal
        // to the rounding of the products, (m + c) u per entry at worst
        const int m = 40, c = 17;
        std::vector<double> G = random_symmetric(m, 11), W = random_symmetric(m, 12), theta((size_t)m), S((size_t)m * m);
        expect(parsy::eigs_jacobi(m, G.data(), theta.data(), S.data()) >= 0, "square: jacobi", 0, 0);
        for (int j = 0; j < m; ++j)
            for (int i = 0; i < m; ++i) W[(size_t)j * m + i] = (i == j ? 1.0 : 0.0) + 1e-9 * W[(size_t)j * m + i];
        expect(parsy::eigs_w_orthonormalise(m, c, W.data(), S.data()) == 0, "square: positive definite", 0, 0);
        double worst = 0;
        for (int j = 0; j < c; ++j)
            for (int i = 0; i < c; ++i) {
                long double s = 0;
                for (int a = 0; a < m; ++a)
                    for (int b = 0; b < m; ++b) s += (long double)S[(size_t)i * m + a] * W[(size_t)b * m + a] * S[(size_t)j * m + b];
                worst = std::fmax(worst, std::fabs((double)(s - (i == j ? 1.0L : 0.0L))));
            }
        expect(worst <= (m + c) * u, "square: S'WS - I", worst, (m + c) * u);
        std::printf("square |S'WS - I|max=%.3e bound %.3e\n", worst, (m + c) * u);
        W[0] = -1.0;
        std::vector<double> S1((size_t)m * m, 0.0);
        for (int j = 0; j < m; ++j) S1[(size_t)j * m + j] = 1.0;
        expect(parsy::eigs_w_orthonormalise(m, c, W.data(), S1.data()) == parsy::kEigsCholNotSpd, "square: not SPD", 0, 0);
    }
    check_cholesky();
    if (failures) return std::printf("eigs_dense: %d failures\n", failures), 1;
    std::printf("eigs_dense: all checks passed\n");
    return 0;
}
