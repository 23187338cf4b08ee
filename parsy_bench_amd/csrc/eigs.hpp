// The smallest eigenpairs of A v = lambda M v on the device, through the factor (parsy_eigs_device): a block Davidson
// iteration with (L L')^-1 as preconditioner and a thick restart, everything in the factor's ordering.  This header is
// the host loop; the kernels and their launches are eigs_kernels.hip, the small dense work eigs_dense.hpp, the state
// EigsState (feature_states.hpp).
//
// V (n x m, M-orthonormal), A V and M V live side by side in EigsState::basis.  An iteration:
//   Ritz     G = V'(A V) (k_eigs_gram), symmetrised and diagonalised on the host (Jacobi): theta ascending, S;
//            R = (A V) S - (M V) S Theta and Y = V S in blocks of 16 columns (k_eigs_rotate), eta per pair
//            (k_eigs_colmax, k_eigs_eta) -- from the kept products;
//   stop     the first k pairs at eta <= tol: they are formed afresh, Y = V S, A Y and M Y by new products, and the eta of
//            those is what is returned.  A pair the fresh products put above tol sends the call back into the loop, which
//            asks for half the tolerance from there on;
//   restart  when m + block > max_basis: V <- V S[:, :keep], keep = min(m, k + block), written into the slab of A V (a
//            rotation is never in place here: k_eigs_rotate's Z and X are different memory) and the slabs swap; A V and
//            M V of the kept columns are new products, never rotated ones;
//   expand   sources = the first `block` unconverged pairs of the k wanted, filled up with the Ritz pairs beyond k;
//            T = (L L')^-1 (A y - theta M y), one many-right-hand-side solve pair (residual form: the factor may be a
//            stale one, it sets the speed and not the answer);
//   orthogonalise  twice T -= V ((M V)' T), then two passes of Cholesky-QR in the M inner product, the first on the Gram
//            matrix scaled to unit diagonal with the drop rule of eigs_dense.hpp; T, A T and M T join the basis.
//
// Before V S leaves the basis -- at a restart, and as the returned Y -- the columns of S that are used are made
// orthonormal in the inner product of V'(M V), so the rounding of the rotations does not add up over the restarts.
//
// The stream is waited for four times per iteration, each time for a small matrix the host works on: G (m x m), the
// eta of the wanted pairs (k doubles), and the Gram matrix of the block in each of the two Cholesky-QR passes
// (<= 16 x 16); once more at a restart and before the returned pairs are formed (V'(M V), m x m).  The status of the solves rides along with each.  Nothing else is read back; the basis never leaves the
// device.  Every sum here runs in a fixed order and there is no atomic: given the same solve results the same inputs give
// the same bits (the plan's many-right-hand-side solves are bitwise reproducible on some plans only).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <limits>
#include <string>

#include "eigs_dense.hpp"
#include "errors.hpp"
#include "executor.hpp"
#include "feature_states.hpp"
#include "hip_check.hpp"
#include "plan_util.hpp"
#include "refine.hpp"

namespace parsy {

constexpr int kEigsBlocks = 3;   // scratch blocks of n x 16: T / Y, its product or R, the other operand of a rotation

// Where the small matrices live in EigsState::dense (doubles)
struct EigsDense {
    static constexpr int64_t kSq = (int64_t)kEigsMaxBasis * kEigsMaxBasis;
    static constexpr int64_t g = 0;                // a Gram kernel's result: V'(A V), (M V)' T or T' M T
    static constexpr int64_t s = kSq;              // S (m x m)
    static constexpr int64_t st = 2 * kSq;         // - S Theta (m x m)
    static constexpr int64_t sel = 3 * kSq;        // the sources' columns of S and of - S Theta (m x block each)
    static constexpr int64_t c1 = sel + 2 * kEigsMaxBasis * kEigsMaxBlock;   // the two passes' T <- T C
    static constexpr int64_t c2 = c1 + kEigsMaxBlock * kEigsMaxBlock;
    static constexpr int64_t theta = c2 + kEigsMaxBlock * kEigsMaxBlock;
    static constexpr int64_t eta = theta + kEigsMaxBasis;
    static constexpr int64_t norms = eta + kEigsMaxBasis;                   // ||A||_inf, ||M||_inf
    static constexpr int64_t size = norms + 2;
};

// ---- eigs_kernels.hip ----
// the state with room for a basis of max_basis columns (with_m: a slab for M V too); 0 or -1
int eigs_ensure(parsy_plan* pl, int max_basis, bool with_m);
// C (p x q, leading dimension ldc, device) = X' Y for X n x p, Y n x q (leading dimension n)
int eigs_gram_enqueue(parsy_plan* pl, const double* X, int p, const double* Y, int q, double* C, int ldc, hipStream_t stream);
// Z (n x q) = beta Z + alpha X C for X n x p (p may be 0), C p x q (device, leading dimension ldc), q <= 16; Z is not X
int eigs_rotate_enqueue(parsy_plan* pl, double* Z, double beta, double alpha, const double* X, int p, const double* C, int ldc,
                        int q, hipStream_t stream);
// Y = A X for the gathered values vf (n x ncols, leading dimension n)
int eigs_product_enqueue(parsy_plan* pl, const double* vf, const double* X, double* Y, int ncols, hipStream_t stream);
// *out (device) = the largest absolute row sum of the gathered values vf; vf null: 1 (the identity's)
int eigs_norm_enqueue(parsy_plan* pl, const double* vf, double* out, hipStream_t stream);
// eta[c] = max |ay - theta[c] my| / ((norms[0] + |theta[c]| norms[1]) max |y|) of ncols <= 16 columns; my null: the
// residual is ay itself
int eigs_eta_enqueue(parsy_plan* pl, const double* ay, const double* my, const double* y, int ncols, const double* theta,
                     const double* norms, double* eta, hipStream_t stream);

namespace eigs_detail {

struct Run {
    parsy_plan* pl;
    EigsState& E;
    const char* who;
    const double* d_L;
    hipStream_t stream;
    int n, k, block, max_basis;
    bool with_m;
    double *V, *AV, *MV;          // the slabs (MV == V without an M)
    double* W[kEigsBlocks];
    double* D;                    // EigsState::dense
    int m = 0;                    // columns of the basis
    int iteration = 0;

    const double* vf_m() const { return with_m ? E.vf_m.data() : nullptr; }
    // Y = M X, or Y = X itself without an M: returns where M X is
    const double* times_m(const double* X, double* Y, int ncols, int* rc) {
        if (!with_m) return X;
        if (eigs_product_enqueue(pl, E.vf_m.data(), X, Y, ncols, stream) != 0) *rc = -1;
        return Y;
    }
    // host <- device behind everything enqueued so far, with the status of the solves
    int read_back(double* host, const double* dev, int64_t count) {
        int ctl[2] = {0, 0};
        PARSY_HIP(hipMemcpyAsync(host, dev, (size_t)count * 8, hipMemcpyDeviceToHost, stream));
        PARSY_HIP(hipMemcpyAsync(ctl, E.ctl.data(), sizeof(ctl), hipMemcpyDeviceToHost, stream));
        PARSY_HIP(hipStreamSynchronize(stream));
        if (ctl[1] < 0)
            return set_last_error(std::string(who) + ": a hand-off wait inside a chain launch timed out; nothing was returned"),
                   -1;
        return 0;
    }
    int upload(int64_t where, const std::vector<double>& h, int64_t count) {
        PARSY_HIP(hipMemcpyAsync(D + where, h.data(), (size_t)count * 8, hipMemcpyHostToDevice, stream));
        return 0;
    }

    // h_s and h_st (= - S Theta) for the basis as it stands, and their device copies
    int upload_rotation() {
        E.h_st.resize((size_t)m * m);
        for (int j = 0; j < m; ++j)
            for (int i = 0; i < m; ++i) E.h_st[(size_t)j * m + i] = -E.h_s[(size_t)j * m + i] * E.h_theta[(size_t)j];
        if (upload(EigsDense::s, E.h_s, (int64_t)m * m) != 0 || upload(EigsDense::st, E.h_st, (int64_t)m * m) != 0 ||
            upload(EigsDense::theta, E.h_theta, m) != 0)
            return -1;
        return 0;
    }

    // The first `cols` columns of S made orthonormal in the inner product of W = V'(M V) (eigs_w_orthonormalise), before
    // V S leaves the basis -- into a restart or out to the caller: the rounding of the rotations does not add up from
    // restart to restart, and Y is M-orthonormal to the accuracy of one Gram product.  One more wait.
    int square_rotation(int cols) {
        if (eigs_gram_enqueue(pl, V, m, MV, m, D + EigsDense::g, m, stream) != 0) return -1;
        E.h_g.resize((size_t)m * m);
        if (read_back(E.h_g.data(), D + EigsDense::g, (int64_t)m * m) != 0) return -1;
        for (int j = 0; j < m; ++j)
            for (int i = 0; i < j; ++i)
                E.h_g[(size_t)j * m + i] = E.h_g[(size_t)i * m + j] = 0.5 * (E.h_g[(size_t)j * m + i] + E.h_g[(size_t)i * m + j]);
        if (eigs_w_orthonormalise(m, cols, E.h_g.data(), E.h_s.data()) != kEigsCholOk)
            return set_last_error(std::string(who) + ": V'MV of iteration " + std::to_string(iteration) +
                                  " is not positive definite: M is not SPD"),
                   -2;
        return upload_rotation();
    }

    // theta, S of the basis and the eta of its first min(k, m) pairs from the kept products (E.h_eta)
    int ritz() {
        if (eigs_gram_enqueue(pl, V, m, AV, m, D + EigsDense::g, m, stream) != 0) return -1;
        E.h_g.resize((size_t)m * m);
        if (read_back(E.h_g.data(), D + EigsDense::g, (int64_t)m * m) != 0) return -1;
        for (int j = 0; j < m; ++j)
            for (int i = 0; i < j; ++i)
                E.h_g[(size_t)j * m + i] = E.h_g[(size_t)i * m + j] = 0.5 * (E.h_g[(size_t)j * m + i] + E.h_g[(size_t)i * m + j]);
        E.h_s.resize((size_t)m * m);
        E.h_theta.resize((size_t)m);
        if (eigs_jacobi(m, E.h_g.data(), E.h_theta.data(), E.h_s.data()) < 0)
            return set_last_error(std::string(who) + ": the projected matrix of iteration " + std::to_string(iteration) +
                                  " could not be diagonalised (not finite)"),
                   -1;
        if (upload_rotation() != 0) return -1;
        const int kk = std::min(k, m);
        for (int c0 = 0; c0 < kk; c0 += kEigsMaxBlock) {
            const int nc = std::min(kEigsMaxBlock, kk - c0);
            const double *Sc = D + EigsDense::s + (int64_t)c0 * m, *STc = D + EigsDense::st + (int64_t)c0 * m;
            if (eigs_rotate_enqueue(pl, W[0], 0.0, 1.0, V, m, Sc, m, nc, stream) != 0 ||
                eigs_rotate_enqueue(pl, W[1], 0.0, 1.0, AV, m, Sc, m, nc, stream) != 0 ||
                eigs_rotate_enqueue(pl, W[1], 1.0, 1.0, MV, m, STc, m, nc, stream) != 0 ||
                eigs_eta_enqueue(pl, W[1], nullptr, W[0], nc, D + EigsDense::theta + c0, D + EigsDense::norms,
                                 D + EigsDense::eta + c0, stream) != 0)
                return -1;
        }
        E.h_eta.resize((size_t)kk);
        return read_back(E.h_eta.data(), D + EigsDense::eta, kk);
    }

    // the eta of the first min(k, m) Ritz pairs from fresh products of Y = V S (fresh[])
    int fresh_eta(double* fresh) {
        const int kk = std::min(k, m);
        const int rc = square_rotation(kk);
        if (rc != 0) return rc;
        for (int c0 = 0; c0 < kk; c0 += kEigsMaxBlock) {
            const int nc = std::min(kEigsMaxBlock, kk - c0);
            int rc = 0;
            if (eigs_rotate_enqueue(pl, W[0], 0.0, 1.0, V, m, D + EigsDense::s + (int64_t)c0 * m, m, nc, stream) != 0 ||
                eigs_product_enqueue(pl, E.vf_a.data(), W[0], W[1], nc, stream) != 0)
                return -1;
            const double* my = times_m(W[0], W[2], nc, &rc);
            if (rc != 0 || eigs_eta_enqueue(pl, W[1], my, W[0], nc, D + EigsDense::theta + c0, D + EigsDense::norms,
                                            D + EigsDense::eta + c0, stream) != 0)
                return -1;
        }
        return read_back(fresh, D + EigsDense::eta, kk);
    }

    // Y = V S once more (the same bits) out through the ordering; zero columns where the basis has no pair
    int scatter_out(const int* perm, double* d_y, int ldy) {
        const int kk = std::min(k, m);
        for (int c0 = 0; c0 < k; c0 += kEigsMaxBlock) {
            const int nc = std::min(kEigsMaxBlock, k - c0), have = std::max(0, std::min(nc, kk - c0));
            if (have < nc) PARSY_HIP(hipMemsetAsync(W[0], 0, (size_t)n * nc * 8, stream));
            if (have > 0 &&
                eigs_rotate_enqueue(pl, W[0], 0.0, 1.0, V, m, D + EigsDense::s + (int64_t)c0 * m, m, have, stream) != 0)
                return -1;
            enqueue_perm_scatter(perm, W[0], 1.0, 0.0, d_y + (int64_t)c0 * ldy, ldy, n, nc, stream);
        }
        PARSY_HIP(hipGetLastError());
        PARSY_HIP(hipStreamSynchronize(stream));
        return 0;
    }

    // T (nb columns in W[0]) made M-orthonormal against V and in itself; what is left joins the basis with its products.
    // *added: the columns that did.  0, -1, or -2 (M is not positive definite)
    int orthonormalise_and_append(int nb, int* added) {
        *added = 0;
        double *T = W[0], *T2 = W[2];
        for (int pass = 0; pass < 2 && m > 0; ++pass)
            if (eigs_gram_enqueue(pl, MV, m, T, nb, D + EigsDense::g, m, stream) != 0 ||
                eigs_rotate_enqueue(pl, T, 1.0, -1.0, V, m, D + EigsDense::g, m, nb, stream) != 0)
                return -1;
        for (int pass = 0; pass < 2; ++pass) {
            int rc = 0, kept = 0;
            const double* MT = times_m(T, W[1], nb, &rc);
            if (rc != 0 || eigs_gram_enqueue(pl, T, nb, MT, nb, D + EigsDense::g, nb, stream) != 0) return -1;
            E.h_g.resize((size_t)nb * nb);
            if (read_back(E.h_g.data(), D + EigsDense::g, (int64_t)nb * nb) != 0) return -1;
            for (int j = 0; j < nb; ++j)   // (the lower triangle is what the factorization reads)
                for (int i = j + 1; i < nb; ++i)
                    E.h_g[(size_t)j * nb + i] = 0.5 * (E.h_g[(size_t)j * nb + i] + E.h_g[(size_t)i * nb + j]);
            std::vector<double>& C = pass == 0 ? E.h_c1 : E.h_c2;
            C.assign((size_t)kEigsMaxBlock * kEigsMaxBlock, 0.0);
            if (eigs_chol_rinv(nb, E.h_g.data(), pass == 0, C.data(), &kept, &E.dropped) != kEigsCholOk)
                return set_last_error(std::string(who) + ": the Gram matrix of the block of iteration " +
                                      std::to_string(iteration) + " is not positive definite: M is not SPD"),
                       -2;
            if (kept == 0) return 0;
            const int64_t where = pass == 0 ? EigsDense::c1 : EigsDense::c2;
            if (upload(where, C, (int64_t)nb * kept) != 0) return -1;
            // the last pass writes into the basis
            double* Z = pass == 0 ? T2 : V + (int64_t)m * n;
            if (eigs_rotate_enqueue(pl, Z, 0.0, 1.0, T, nb, D + where, nb, kept, stream) != 0) return -1;
            std::swap(T, T2);
            nb = kept;
        }
        const double* Tn = V + (int64_t)m * n;
        if (eigs_product_enqueue(pl, E.vf_a.data(), Tn, AV + (int64_t)m * n, nb, stream) != 0) return -1;
        if (with_m && eigs_product_enqueue(pl, E.vf_m.data(), Tn, MV + (int64_t)m * n, nb, stream) != 0) return -1;
        m += nb;
        *added = nb;
        return 0;
    }

    // V <- V S[:, :keep] through the slab of A V, then new products of the kept columns
    int restart(int keep) {
        const int rc = square_rotation(keep);
        if (rc != 0) return rc;
        for (int c0 = 0; c0 < keep; c0 += kEigsMaxBlock) {
            const int nc = std::min(kEigsMaxBlock, keep - c0);
            if (eigs_rotate_enqueue(pl, AV + (int64_t)c0 * n, 0.0, 1.0, V, m, D + EigsDense::s + (int64_t)c0 * m, m, nc,
                                    stream) != 0)
                return -1;
        }
        if (with_m) std::swap(V, AV);
        else std::swap(V, AV), MV = V;
        m = keep;
        if (eigs_product_enqueue(pl, E.vf_a.data(), V, AV, m, stream) != 0) return -1;
        if (with_m && eigs_product_enqueue(pl, E.vf_m.data(), V, MV, m, stream) != 0) return -1;
        // the kept columns are the Ritz vectors themselves now
        E.h_s.assign((size_t)m * m, 0.0);
        for (int j = 0; j < m; ++j) E.h_s[(size_t)j * m + j] = 1.0;
        E.h_theta.resize((size_t)m);
        return upload_rotation();
    }

    // the sources' residuals (A V) s - theta (M V) s into W[0]; returns their number
    int residuals_of_sources(double inner_tol, int* count) {
        const int kk = std::min(k, (int)E.h_eta.size());
        int src[kEigsMaxBlock], ns = 0;
        for (int i = 0; i < kk && ns < block; ++i)
            if (m < k || !(E.h_eta[(size_t)i] <= inner_tol)) src[ns++] = i;
        for (int i = k; i < m && ns < block; ++i) src[ns++] = i;
        std::vector<double>& sel = E.h_c1;   // (free here: its last upload lies behind a wait)
        sel.resize((size_t)2 * m * ns);
        for (int c = 0; c < ns; ++c)
            for (int i = 0; i < m; ++i) {
                sel[(size_t)c * m + i] = E.h_s[(size_t)src[c] * m + i];
                sel[(size_t)(ns + c) * m + i] = E.h_st[(size_t)src[c] * m + i];
            }
        *count = ns;
        if (ns == 0) return 0;
        if (upload(EigsDense::sel, sel, (int64_t)2 * m * ns) != 0 ||
            eigs_rotate_enqueue(pl, W[0], 0.0, 1.0, AV, m, D + EigsDense::sel, m, ns, stream) != 0 ||
            eigs_rotate_enqueue(pl, W[0], 1.0, 1.0, MV, m, D + EigsDense::sel + (int64_t)m * ns, m, ns, stream) != 0)
            return -1;
        return 0;
    }
};

}  // namespace eigs_detail

// parsy_eigs_device behind the null checks of the C ABI
inline int plan_eigs(parsy_plan* pl, const double* d_values, const double* d_mvalues, const double* d_L, int k,
                     const double* d_x0, int ldx0, int block, double tol, int max_basis, int max_iter, double* lambda,
                     double* d_y, int ldy, double* resid, int32_t* nconv, hipStream_t stream) {
    const char* who = "parsy_eigs_device";
    if (check_plan(pl, who, kNeedsIdle) != 0) return -1;
    const int n = pl->S.n;
    auto refuse = [&](const std::string& what) { return set_last_error(std::string(who) + ": " + what), -1; };
    if (k < 1 || block < 1 || block > kEigsMaxBlock) return refuse("need k >= 1 and 1 <= block <= 16");
    if (max_basis < 0 || max_basis > kEigsMaxBasis || max_basis > n)
        return refuse("need max_basis <= 128 and <= n (0: the default)");
    const int64_t floor_basis = (int64_t)k + 2 * (int64_t)block;
    const int mb = max_basis != 0 ? max_basis
                                  : (int)std::min<int64_t>(std::max<int64_t>(3 * (int64_t)k, (int64_t)k + 4 * block),
                                                           std::min(n, kEigsMaxBasis));
    if (mb < floor_basis) return refuse("need max_basis >= k + 2 block (the default is clipped to min(n, 128))");
    if (max_iter < 1) return refuse("need max_iter >= 1");
    if (ldx0 < n || ldy < n) return refuse("need leading dimensions >= n");
    if (refine_ensure_pattern(pl) != 0) return -1;
    if (!(tol >= (double)(pl->refine->max_row + 1) * 0x1p-52))
        return refuse("tol is below (max_row + 1) 2^-52, which an FP64 residual cannot show");
    const int* perm = nullptr;
    const bool with_m = d_mvalues != nullptr;
    if (plan_perm_device(pl, &perm) != 0 || eigs_ensure(pl, mb, with_m) != 0) return -1;
    EigsState& E = *pl->eigs;
    E.iterations = E.restarts = E.nconv = E.basis_cols = E.dropped = 0;
    E.solve_columns = 0;
    const int64_t slab = (int64_t)n * mb, blk = (int64_t)n * kEigsMaxBlock;
    eigs_detail::Run r{pl, E, who, d_L, stream, n, k, block, mb, with_m,
                       E.basis.data(), E.basis.data() + slab, with_m ? E.basis.data() + 2 * slab : E.basis.data(),
                       {E.blocks.data(), E.blocks.data() + blk, E.blocks.data() + 2 * blk}, E.dense.data()};
    double* const D = r.D;
    PARSY_HIP(hipMemsetAsync(E.ctl.data(), 0, 2 * sizeof(int), stream));
    if (refine_gather_values(pl, d_values, E.vf_a.data(), stream) != 0 ||
        (with_m && refine_gather_values(pl, d_mvalues, E.vf_m.data(), stream) != 0) ||
        eigs_norm_enqueue(pl, E.vf_a.data(), D + EigsDense::norms, stream) != 0 ||
        eigs_norm_enqueue(pl, r.vf_m(), D + EigsDense::norms + 1, stream) != 0)
        return -1;
    // start: the block in the factor's ordering, M-orthonormal
    enqueue_perm_gather(perm, d_x0, ldx0, r.W[0], nullptr, n, block, stream);
    PARSY_HIP(hipGetLastError());
    int added = 0;
    int rc = r.orthonormalise_and_append(block, &added);
    if (rc != 0) return rc;
    if (added == 0) return refuse("the start block has no column that is independent in the M inner product");
    double inner_tol = tol;
    std::vector<double> fresh;
    int kk = 0;
    for (;;) {
        if (r.ritz() != 0) return -1;
        kk = std::min(k, r.m);
        bool done = r.m >= k;
        for (int i = 0; i < kk && done; ++i) done = E.h_eta[(size_t)i] <= inner_tol;
        const bool last = E.iterations >= max_iter;
        if (done || last) {
            fresh.assign((size_t)kk, 0.0);
            rc = r.fresh_eta(fresh.data());
            if (rc != 0) return rc;
            bool held = true;
            for (int i = 0; i < kk; ++i) held = held && fresh[(size_t)i] <= tol;
            if (!done || held || last) break;
            inner_tol *= 0.5;
            continue;
        }
        E.iterations += 1;
        r.iteration = E.iterations;
        if (r.m + block > mb) {
            rc = r.restart(std::min(r.m, k + block));
            if (rc != 0) return rc;
            E.restarts += 1;
        }
        int ns = 0;
        if (r.residuals_of_sources(inner_tol, &ns) != 0) return -1;
        added = 0;
        if (ns > 0) {
            if (refine_solve_enqueue(pl, d_L, r.W[0], ns, E.ctl.data(), stream) != 0) return -1;
            E.solve_columns += ns;
            rc = r.orthonormalise_and_append(ns, &added);
            if (rc != 0) return rc;
        }
        if (added == 0) {   // every column was dropped: the basis cannot grow, the call ends as it stands
            if (r.ritz() != 0) return -1;
            kk = std::min(k, r.m);
            fresh.assign((size_t)kk, 0.0);
            rc = r.fresh_eta(fresh.data());
            if (rc != 0) return rc;
            break;
        }
    }
    if (r.scatter_out(perm, d_y, ldy) != 0) return -1;
    int nc = 0;
    for (int i = 0; i < k; ++i) {
        lambda[i] = i < kk ? E.h_theta[(size_t)i] : std::numeric_limits<double>::quiet_NaN();
        resid[i] = i < kk ? fresh[(size_t)i] : std::numeric_limits<double>::infinity();
        nc += resid[i] <= tol ? 1 : 0;
    }
    *nconv = E.nconv = nc;
    E.basis_cols = r.m;
    return 0;
}

}  // namespace parsy
