// Stand-alone driver of csrc/reach.cpp over hand-made supernodal etrees (tests/test_sparse_solve_host.py compiles it with
// reach.cpp alone, as host C++ under the address and undefined-behaviour sanitizers, and runs it): closures, pieces, steps,
// launch lists, gather lists and refusals.  No device, nothing of the plan.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <set>
#include <string>
#include <vector>

#include "reach.hpp"

namespace parsy {
static std::string g_error;
void set_last_error(const std::string& msg) { g_error = msg; }
const std::string& last_error() { return g_error; }
}  // namespace parsy

using namespace parsy;

static int g_checks = 0;
#define REQUIRE(cond)                                                              \
    do {                                                                           \
        ++g_checks;                                                                \
        if (!(cond)) {                                                             \
            std::printf("reach_check: line %d: %s failed\n", __LINE__, #cond);      \
            std::exit(1);                                                          \
        }                                                                          \
    } while (0)

// A schedule with these widths and parents (children before parents): the row list of a supernode is its own columns and
// every column of every ancestor, so every row below it belongs to an ancestor.
static Schedule make(const std::vector<int>& widths, const std::vector<int>& parent) {
    Schedule S;
    S.nsuper = (int)widths.size();
    S.sparent = parent;
    S.sn.resize(widths.size());
    int c = 0;
    for (size_t s = 0; s < widths.size(); ++s) S.sn[s].c0 = c, S.sn[s].w = widths[s], c += widths[s];
    S.n = c;
    int64_t px = 0;
    for (int s = 0; s < S.nsuper; ++s) {
        SnDesc& D = S.sn[(size_t)s];
        D.pi = (int64_t)S.rows.size();
        D.px = px;
        for (int a = s; a >= 0; a = parent[(size_t)a])
            for (int j = 0; j < S.sn[(size_t)a].w; ++j) S.rows.push_back(S.sn[(size_t)a].c0 + j);
        D.r = (int32_t)((int64_t)S.rows.size() - D.pi);
        D.ld = D.r;
        px += (int64_t)D.r * D.w;
    }
    S.xsize = px, S.ssize = (int64_t)S.rows.size();
    return S;
}

static std::vector<int32_t> closure(const Schedule& S, const std::vector<int>& rows) {
    std::set<int32_t> out;
    for (int row : rows) {
        int s = 0;
        while (S.sn[(size_t)s].c0 + S.sn[(size_t)s].w <= row) ++s;
        for (; s >= 0; s = S.sparent[(size_t)s]) out.insert(s);
    }
    return std::vector<int32_t>(out.begin(), out.end());
}

static int step_of(const SparsePass& P, const Schedule& S, int sn, int c0) {
    for (int t = 0; t < P.steps(); ++t)
        for (int i = P.step_first[(size_t)t]; i < P.step_first[(size_t)t + 1]; ++i)
            if (P.pieces[(size_t)i].px == S.sn[(size_t)sn].px && P.pieces[(size_t)i].c0 == c0) return t;
    return -1;
}

static void one(const Schedule& S, const std::vector<int>& inv, const std::vector<int>& bp, const std::vector<int>& bi,
                const std::vector<int>* xi, ReachIndex& I) {
    const int nrhs = (int)bp.size() - 1;
    REQUIRE(reach_build(S, inv, "reach_check", nrhs, bp.data(), bi.empty() ? nullptr : bi.data(), xi ? (int)xi->size() : 0,
                        xi ? xi->data() : nullptr, I) == 0);
    REQUIRE(reach_check(S, I) == 0);
    auto at = [&](int row) { return inv.empty() ? row : inv[(size_t)row]; };
    std::vector<int> brows, xrows;
    for (int row : bi) brows.push_back(at(row));
    if (xi) for (int row : *xi) xrows.push_back(at(row));
    else for (int row = 0; row < S.n; ++row) xrows.push_back(row);
    REQUIRE(I.fwd.sn == closure(S, brows));
    REQUIRE(I.bwd.sn == closure(S, xrows));
    REQUIRE(I.nx == (int)xrows.size() && (int)I.xcomp.size() == I.nx && I.bcol.size() == bi.size());
    // the compact numbering: the selected rows and B's rows land on their own columns
    int64_t widths = 0, entries = 0;
    std::vector<int32_t> both;
    std::set_union(I.fwd.sn.begin(), I.fwd.sn.end(), I.bwd.sn.begin(), I.bwd.sn.end(), std::back_inserter(both));
    for (int32_t s : both) widths += S.sn[(size_t)s].w, entries += S.sn[(size_t)s].r;
    REQUIRE(I.ncomp == widths && I.nent == entries && (int64_t)I.cmap.size() == entries);
    REQUIRE(reach_kernels(I, 0) == reach_kernels(I, 1) + reach_kernels(I, 2) - 3);
}

int main() {
    ReachIndex I;
    {   // a chain of three: every reach ends at the root; the wide root takes three pieces
        const Schedule S = make({2, 1, 2 * kSparsePiece + 1}, {1, 2, -1});
        one(S, {}, {0, 1}, {0}, nullptr, I);
        REQUIRE(I.fwd.sn.size() == 3 && I.fwd.pieces.size() == 5 && I.fwd.steps() == 5);
        REQUIRE(step_of(I.fwd, S, 2, 0) == 2 && step_of(I.fwd, S, 2, kSparsePiece) == 3 && step_of(I.fwd, S, 2, 2 * kSparsePiece) == 4);
        REQUIRE(I.fwd.pieces.back().nc == 1 && I.fwd.work_first[5] == I.fwd.work_first[4]);   // the last piece has no row below
        REQUIRE(I.fwd.entries == S.xsize - (int64_t)(2 * kSparsePiece + 1) * kSparsePiece - 1);   // (all but the strict upper triangles)
        const std::vector<int> xi = {S.n - 1};
        one(S, {}, {0, 1, 1}, {3}, &xi, I);   // B in the root, an empty second column
        REQUIRE(I.fwd.sn.size() == 1 && I.bwd.sn.size() == 1 && I.fwd.steps() == 3 && I.nrhs == 2);
        REQUIRE(I.ncomp == 2 * kSparsePiece + 1 && I.xcomp[0] == 2 * kSparsePiece);
        REQUIRE(reach_kernels(I, 1) == 3 + 3 + 2 && reach_kernels(I, 2) == 3 + 3 + 2 && reach_kernels(I, 0) == 3 + 2 * 5);
        one(S, {}, {0, 0}, {}, &xi, I);       // no entry at all
        REQUIRE(I.fwd.sn.empty() && I.fwd.steps() == 0 && I.gpos.empty() && reach_kernels(I, 1) == 3);
    }
    {   // two subtrees under one root, one of them two deep; under an ordering
        const Schedule S = make({3, 2, 4, 1, 257, 5}, {2, 2, 5, 4, 5, -1});
        std::vector<int> inv((size_t)S.n);
        for (int i = 0; i < S.n; ++i) inv[(size_t)i] = (i * 7 + 3) % S.n;   // (7 and n = 272 are coprime)
        std::vector<int> perm((size_t)S.n);
        for (int i = 0; i < S.n; ++i) perm[(size_t)inv[(size_t)i]] = i;
        std::vector<int> bi = {perm[0], perm[9]};   // supernodes 0 and 3
        std::sort(bi.begin(), bi.end());
        const std::vector<int> xi = {perm[4], perm[1]};   // supernodes 1 and 0, not ascending
        one(S, inv, {0, 2}, bi, &xi, I);
        REQUIRE((I.fwd.sn == std::vector<int32_t>{0, 2, 3, 4, 5}) && (I.bwd.sn == std::vector<int32_t>{0, 1, 2, 5}));
        REQUIRE(step_of(I.fwd, S, 0, 0) == 0 && step_of(I.fwd, S, 3, 0) == 0 && step_of(I.fwd, S, 2, 0) == 1);
        REQUIRE(step_of(I.fwd, S, 4, 0) == 1 && step_of(I.fwd, S, 4, kSparsePiece) == 2 && step_of(I.fwd, S, 5, 0) == 3);
        REQUIRE(step_of(I.bwd, S, 5, 0) == 2 && step_of(I.bwd, S, 1, 0) == 0 && I.bwd.steps() == 3);
        REQUIRE(I.xcomp[0] == 3 + 1 && I.xcomp[1] == 1);   // rows 4 and 1 of the factor's ordering in the compact numbering
        // supernode 1 is in K alone: its columns carry no gather list and its entries are not F's
        REQUIRE(I.colmask[3] == 2 && I.colmask[0] == 3 && I.gptr[4] == I.gptr[3] && I.entmask[(size_t)S.sn[0].r] == 0);
        // the first column of the root (compact 3 + 2 + 4 + 1 + 257) is below supernodes 0, 2, 3 and 4 of F
        REQUIRE(I.gptr[268] - I.gptr[267] == 4);
        one(S, inv, {0, 2}, bi, nullptr, I);
        REQUIRE((int)I.bwd.sn.size() == S.nsuper && I.bwd.entries + 3 + 1 + 6 + 0 + 257 * 128 + 10 == S.xsize);
    }
    {   // a forest: two roots, the second a single column
        const Schedule S = make({2, 3, 1}, {1, -1, -1});
        const std::vector<int> xi = {5};
        one(S, {}, {0, 1}, {0}, &xi, I);
        REQUIRE((I.fwd.sn == std::vector<int32_t>{0, 1}) && (I.bwd.sn == std::vector<int32_t>{2}) && I.ncomp == 6);
        REQUIRE(I.bwd.work.empty() && I.npart == 0 && reach_kernels(I, 2) == 3 + 1);
    }
    {   // the refusals
        const Schedule S = make({2, 2}, {1, -1});
        const int bp[] = {0, 2}, up[] = {1, 2}, down[] = {0, 2, 1}, bi[] = {1, 3}, same[] = {2, 2}, wide[] = {1, 4}, xi[] = {0, 0}, far[] = {-1};
        REQUIRE(reach_build(S, {}, "who", 0, bp, bi, 0, nullptr, I) == -1 && last_error() == "who: need nrhs >= 1");
        REQUIRE(reach_build(S, {}, "who", 1, nullptr, bi, 0, nullptr, I) == -1 && last_error() == "who: null argument");
        REQUIRE(reach_build(S, {}, "who", 1, bp, nullptr, 0, nullptr, I) == -1 && last_error() == "who: null argument");
        REQUIRE(reach_build(S, {}, "who", 1, up, bi, 0, nullptr, I) == -1 && last_error().find("start at 0") != std::string::npos);
        REQUIRE(reach_build(S, {}, "who", 2, down, bi, 0, nullptr, I) == -1 && last_error().find("decreases") != std::string::npos);
        REQUIRE(reach_build(S, {}, "who", 1, bp, same, 0, nullptr, I) == -1 && last_error().find("unsorted or repeated") != std::string::npos);
        REQUIRE(reach_build(S, {}, "who", 1, bp, wide, 0, nullptr, I) == -1 && last_error().find("out of range") != std::string::npos);
        REQUIRE(reach_build(S, {}, "who", 1, bp, bi, 2, xi, I) == -1 && last_error().find("repeated in the selected rows") != std::string::npos);
        REQUIRE(reach_build(S, {}, "who", 1, bp, bi, 0, xi, I) == -1 && last_error().find("nx >= 1") != std::string::npos);
        REQUIRE(reach_build(S, {}, "who", 1, bp, bi, 1, far, I) == -1 && last_error().find("out of range") != std::string::npos);
        REQUIRE(I.cmap.empty() && I.fwd.sn.empty());
        // a row list that leaves the etree is reported, not followed
        Schedule broken = make({1, 1, 1}, {2, 2, -1});
        broken.rows[(size_t)broken.sn[0].pi + 1] = 1;   // supernode 0 claims a row of its sibling
        const int one_bp[] = {0, 1}, zero[] = {0};
        REQUIRE(reach_build(broken, {}, "who", 1, one_bp, zero, 1, zero, I) == -1 && last_error().find("disagree") != std::string::npos);
    }
    std::printf("reach_check: %d checks, all sound\n", g_checks);
    return 0;
}
