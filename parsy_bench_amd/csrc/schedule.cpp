// Host-side construction of the device schedule (see schedule.hpp).
#include "schedule.hpp"

#include <array>
#include <cstdio>
#include <map>
#include <algorithm>
#include <queue>
#include <set>
#include <climits>
#include <cmath>
#include <cstdlib>
#include <cstdint>
#include <functional>
#include <stdexcept>
#include <string>

namespace parsy {

static inline int ceil_div(int a, int b) { return (a + b - 1) / b; }

static int env_int(const char* name, int dflt) {
    const char* v = std::getenv(name);
    if (!v || !*v) return dflt;
    return std::atoi(v);
}

// Subtrees of the etree that consist of eligible supernodes only and cost at most `cap`, as large as
// possible: subtree[s] = its subtree (numbered from the last root down) or -1.  `parent` must be a
// postordered forest (parent[s] > s); otherwise no subtree is formed.
// slots (optional): per supernode (columns, rows below); a subtree's columns plus the rows below its root must not
// exceed slot_cap (the LDS slots of the solves' subtree kernels for many right-hand sides).
static int find_subtrees(const std::vector<int>& parent, const std::vector<uint8_t>& eligible,
                         const std::vector<double>& cost, double cap, std::vector<int32_t>& subtree,
                         const std::vector<std::pair<int32_t, int32_t>>* slots = nullptr, int64_t slot_cap = 0) {
    const int ns = (int)parent.size();
    subtree.assign(ns, -1);
    std::vector<uint8_t> whole(eligible);  // the supernode and everything below it is eligible
    std::vector<double> sub(cost);
    std::vector<int64_t> cols(slots ? ns : 0);
    for (int s = 0; s < ns && slots; ++s) cols[s] = (*slots)[s].first;
    for (int s = 0; s < ns; ++s) {
        const int p = parent[s];
        if (p < 0) continue;
        if (p <= s) return 0;
        if (!whole[s]) whole[p] = 0;
        sub[p] += sub[s];
        if (slots) cols[p] += cols[s];
    }
    int count = 0;
    for (int s = ns - 1; s >= 0; --s) {
        const int p = parent[s];
        if (p >= 0 && subtree[p] >= 0) subtree[s] = subtree[p];
        else if (whole[s] && sub[s] <= cap && (!slots || cols[s] + (*slots)[s].second <= slot_cap)) subtree[s] = count++;
    }
    return count;
}

namespace {

// ---- The knobs of build_schedule: environment variables for diagnostics and tests.  read_build_knobs reads every one of
// them once, at the top of every build_schedule call -- nothing is kept from one plan to the next (the tests change the
// environment between two plans).  `_set`: that the variable is set at all matters, not only its value.
struct BuildKnobs {
    bool big_mink_set;       // PARSY_BIG_MINK: updates from descendants at least this wide go through the BIG launches (>= 1).
    int big_mink;            //   Set: whatever the size of the job; unset: kBigMinK from kBigAutoFlops update flops on, else never
    bool piece_width_set;    // PARSY_PIECE_WIDTH: columns of a piece of a very wide supernode (0: never split).
    int piece_width;         //   Set: whatever the size of the job; unset: kPieceWidth from kPieceAutoFlops update flops on, else 0
    int push_group;          // PARSY_PUSH_GROUP (kPushGroup, >= 1): pieces whose updates of the pieces further right are merged
    bool split_chunks_set;   // PARSY_SPLIT_CHUNKS (kSplitChunks): early wave streams longer than this many 16-wide chunks are cut
    int split_chunks;        //   into parts.  Set: this one rule on every level; unset: levels of few tiles cut finer (kSplitFew*)
    int split_target;        // PARSY_SPLIT_TARGET (kSplitTarget, >= 1): ... into parts of about this length
    int split_max;           // PARSY_SPLIT_MAX (kSplitMaxParts, >= 1): ... at most this many
    bool subtrees_set;       // PARSY_SUBTREES (kSubtreesPerCu): subtrees aimed at per compute unit (0: none).  Set: always cut, and
    int subtrees_per_cu;     //   the factorization aims at the same number; unset: only where there are enough eligible supernodes
    int chol_subtrees_per_cu;   // PARSY_CHOL_SUBTREES (kCholSubtreesPerCu, >= 1): the factorization's aim where PARSY_SUBTREES is unset
    int super_r, super_c;    // PARSY_BIG_SUPER=RxC | R (1..64 each): one super-tile edge for every BIG launch; 0 (unset): per launch
    int64_t super_min_tasks; // PARSY_BIG_SUPER_MIN (kBigSuperMinTasks): launches of at least this many single-tile tasks ...
    double super_max_fill;   // PARSY_BIG_SUPER_FILL (percent; kBigSuperMaxFill): ... whose windows are filled less than this ...
    int super_hi;            // PARSY_BIG_SUPER_HI (2; 1..8): ... take super-tiles of this edge
    int dense_mode;          // PARSY_BIG_DENSE (1): 0 = never k_chol_dense, 1 = by share, 2 = wherever there is a dense entry,
                             //   3 = as 2 but never a launch's ragged entries too, 4 = every entry of every launch (tests)
    double dense_min_share;  // PARSY_DENSE_MIN_SHARE (percent; kDenseMinShare): share of a launch's products that must be dense
    double dense_all_share;  // PARSY_DENSE_ALL_SHARE (percent; kDenseAllShare): ragged share up to which k_chol_dense takes it too
    int dense_fill_min;      // PARSY_DENSE_FILL (percent of 128 x 128; kDenseMinFill), in entries: windows this full count as dense
    bool dense_strips;       // PARSY_DENSE_STRIPS (1): 0 = no strips ride with the dense blocks
    bool big_recut_set;      // PARSY_BIG_RECUT: 0 = every BIG update is cut on the target's tile grid; 1 = domains of one row set
    int big_recut;           //   in their own row order; 2 = the other domains in intervals too; 3 = as 2 without the tail guard
                             //   (tests, tools).  Set: whatever the size of the job; unset: 2 from kPieceAutoFlops update flops
                             //   on where PARSY_BIG_SUPER is unset too, else 1 (find_conflict_domains)
};

BuildKnobs read_build_knobs() {
    auto percent = [](const char* name, double dflt) { return env_int(name, (int)(dflt * 100 + 0.5)); };
    BuildKnobs K{};
    K.big_mink_set = std::getenv("PARSY_BIG_MINK") != nullptr;
    K.big_mink = std::max(1, env_int("PARSY_BIG_MINK", kBigMinK));
    K.piece_width_set = std::getenv("PARSY_PIECE_WIDTH") != nullptr;
    K.piece_width = env_int("PARSY_PIECE_WIDTH", kPieceWidth);
    K.push_group = std::max(1, env_int("PARSY_PUSH_GROUP", kPushGroup));
    K.split_chunks_set = std::getenv("PARSY_SPLIT_CHUNKS") != nullptr;
    K.split_chunks = env_int("PARSY_SPLIT_CHUNKS", kSplitChunks);
    K.split_target = std::max(1, env_int("PARSY_SPLIT_TARGET", kSplitTarget));
    K.split_max = std::max(1, env_int("PARSY_SPLIT_MAX", kSplitMaxParts));
    K.subtrees_set = std::getenv("PARSY_SUBTREES") != nullptr;
    K.subtrees_per_cu = env_int("PARSY_SUBTREES", kSubtreesPerCu);
    K.chol_subtrees_per_cu = std::max(1, env_int("PARSY_CHOL_SUBTREES", kCholSubtreesPerCu));
    if (const char* e = std::getenv("PARSY_BIG_SUPER")) {
        int a = 0, b = 0;
        const int got = std::sscanf(e, "%dx%d", &a, &b);
        if (got >= 1 && a >= 1 && a <= 64) {
            K.super_r = a;
            K.super_c = (got == 2 && b >= 1 && b <= 64) ? b : a;
        }
    }
    K.super_min_tasks = env_int("PARSY_BIG_SUPER_MIN", kBigSuperMinTasks);
    K.super_max_fill = percent("PARSY_BIG_SUPER_FILL", kBigSuperMaxFill) / 100.0;
    K.super_hi = std::max(1, std::min(8, env_int("PARSY_BIG_SUPER_HI", 2)));
    K.dense_mode = env_int("PARSY_BIG_DENSE", 1);
    K.dense_min_share = percent("PARSY_DENSE_MIN_SHARE", kDenseMinShare) / 100.0;
    K.dense_all_share = percent("PARSY_DENSE_ALL_SHARE", kDenseAllShare) / 100.0;
    K.dense_fill_min = percent("PARSY_DENSE_FILL", kDenseMinFill) * kBigTile * kBigTile / 100;
    K.dense_strips = env_int("PARSY_DENSE_STRIPS", 1) != 0;
    K.big_recut_set = std::getenv("PARSY_BIG_RECUT") != nullptr;
    K.big_recut = std::max(0, std::min(3, env_int("PARSY_BIG_RECUT", 2)));
    return K;
}

// launch id << 40 | global tile index; window: 0 = a task of the tile cut, else domain << 32 | column window << 16 | row window
// of a re-cut domain (launch_tile then names the piece's first tile)
struct BigKeyed { int64_t launch_tile, window; WaveEntry e; int16_t sr, sc; };

// What the passes of build_schedule hand to each other and is not part of the Schedule.
struct BuildState {
    BuildKnobs knobs;
    int compute_units = 0;
    std::vector<int> tree;                  // the supernodal etree (Schedule::sparent)
    std::vector<int64_t> uptr, urel;        // update lists of the supernodes: [uptr[t], uptr[t + 1]) of (descendant usn, its rows
    std::vector<int> usn, ulb, uub;         // lb .. ub inside the target's columns, offset urel into relpos of row lb)
    std::vector<int8_t> launch_super;       // per BIG launch (source level * 2 + push): edge of its tasks' super-tiles
    std::vector<int64_t> level_tiles;       // 64 x 64 tiles of the tiled pieces per level of the Cholesky view
    std::vector<int64_t> big_tile0;         // first 128 x 128 tile index of every tiled piece
    std::vector<int32_t> upd_domain;        // per update: 0 = cut on the target's tile grid; else the re-cut conflict domain it is a
                                            //   member of = 1 + (the domain's first update - the target's first update),
                                            //   + kIntervalDomain where it is cut in intervals of the target's positions
    std::vector<int64_t> upd_bounds;        // per update of an interval domain: where its domain's intervals start in `bounds`
    std::vector<int32_t> bounds;            // per interval domain: the count, then the first position of every interval, ascending
    std::vector<BigKeyed> bigk;            // the BIG entries as they are found, keyed by (launch, tile)
};

// A run of an update's rows that falls into one window of the target's rows.
struct RowRun { int32_t win, first, len; };

// Row of target piece T's panel that row k (counted from lb) of update U lands on.
inline int rel_at(const Schedule& S, const SnDesc& T, const UpdDesc& U, int k) {
    return U.rel < 0 ? k : S.relpos[(size_t)U.rel + k] - T.rbias;
}

// The rows [0, U.m) of update U into piece T, cut into runs per window of `window` rows of T's panel.
void row_runs(const Schedule& S, const SnDesc& T, const UpdDesc& U, int window, std::vector<RowRun>& out) {
    out.clear();
    for (int k = 0; k < U.m;) {
        const int win = rel_at(S, T, U, k) / window;
        int k1 = k + 1;
        while (k1 < U.m && rel_at(S, T, U, k1) / window == win) ++k1;
        out.push_back(RowRun{win, k, k1 - k});
        k = k1;
    }
}

// Updates that go through the BIG launches: wide descendants, and EVERY update of a split supernode's
// pieces (what little reaches those from narrow descendants would otherwise be a TILES launch per
// piece, in between the PUSH launches of the side stream).
inline bool is_big(const Schedule& S, const UpdDesc& U, int target_piece) {
    const int real = S.csn_real[target_piece];
    return U.rel < 0 || U.K >= S.big_min_k || S.piece0[real + 1] - S.piece0[real] > 1;
}

// BIG launch of an update from a source on level lev_s into a target on level lev_t: NEXT(lev_s) | PUSH(lev_s)
inline int64_t big_launch_of(int lev_s, int lev_t) { return (int64_t)lev_s * 2 + (lev_s == lev_t - 1 ? 0 : 1); }

// The pairs (i, j), i >= j, of the block of rows [ia, ia + mi) x [ja, ja + nj) of a source: a block that straddles the
// diagonal has fewer than mi * nj
double block_pairs(int ia, int mi, int ja, int nj) {
    double pairs = 0;
    for (int jj = ja; jj < ja + nj; ++jj) pairs += std::max(0, ia + mi - std::max(ia, jj));
    return pairs;
}

// Reads P, lC, A2p.  Fills the pattern's sizes, S.rows and the supernode descriptors S.sn (checking the panel layout),
// max_width / max_rows, nnzL, flops_stored, n_dslots.
void describe_supernodes(const PatternRef& P, const size_t* lC, const int* A2p, Schedule& S) {
    const int n = P.n, ns = P.nsuper;
    S.n = n;
    S.nsuper = ns;
    S.solve_only = (A2p == nullptr);
    S.nnzA = A2p ? A2p[n] : 0;
    S.rows.assign(P.s, P.s + P.i_ptr[n]);
    S.ssize = (int64_t)P.i_ptr[n];
    S.xsize = (int64_t)lC[n];
    S.sn.resize(ns);
    for (int t = 0; t < ns; ++t) {
        SnDesc& d = S.sn[t];
        d.c0 = P.super[t];
        d.w = P.super[t + 1] - P.super[t];
        d.r = (int)(P.i_ptr[P.super[t + 1]] - P.i_ptr[P.super[t]]);
        d.ld = d.r;
        d.rbias = 0;
        d.px = (int64_t)lC[d.c0];
        d.pi = (int64_t)P.i_ptr[d.c0];
        d.a0 = A2p ? A2p[d.c0] : 0;
        d.a1 = A2p ? A2p[P.super[t + 1]] : 0;
        d.upd0 = 0;
        d.nupd = 0;
        d.dslot = -1;
        d.tflag0 = -1;
        if (d.w <= 0 || d.r < d.w) throw std::runtime_error("schedule: malformed supernode");
        if ((int64_t)d.w * d.r > 0x7fffffffLL)
            throw std::runtime_error("schedule: a single panel exceeds 2^31 entries");
        for (int col = d.c0; col < d.c0 + d.w; ++col)
            if (lC[col + 1] - lC[col] != (size_t)d.r || P.i_ptr[col] != P.i_ptr[d.c0])
                throw std::runtime_error("schedule: lC / Li_ptr are not a column-major panel layout");
        S.max_width = std::max(S.max_width, d.w);
        S.max_rows = std::max(S.max_rows, d.r);
        S.nnzL += (int64_t)d.w * d.r - (int64_t)d.w * (d.w - 1) / 2;
        for (int k = 0; k < d.w; ++k) S.flops_stored += (double)(d.r - k) * (double)(d.r - k);
        for (int k = 0; k < d.w; ++k)
            if (S.rows[d.pi + k] != d.c0 + k)
                throw std::runtime_error("schedule: supernode rows do not start with its own columns");
        // solve: one scratch slot (inverse diagonal block) per block column of the wide supernodes
        if (d.w > kTile) {
            d.dslot = (int32_t)S.n_dslots;
            S.n_dslots += ceil_div(d.w, kTile);
        }
    }
}

// Reads P, lC, A2p / A2i, S.sn, S.rows.  Fills the update lists of the supernodes (B.uptr / usn / ulb / uub), the relative
// indices S.relpos with B.urel, the A scatter map S.a_dst, update_flops and reread_bytes.
void list_updates(const PatternRef& P, const size_t* lC, const int* A2p, const int* A2i, Schedule& S, BuildState& B) {
    const int n = P.n, ns = P.nsuper;
    B.uptr.assign(ns + 1, 0);
    if (!S.solve_only) build_update_lists(P, B.uptr, B.usn, B.ulb, B.uub);
    B.urel.assign(B.usn.size(), 0);  // per (target, descendant): offset into relpos of row lb
    S.a_dst.assign((size_t)S.nnzA, 0);
    std::vector<int> map(n, -1), stamp(n, -1);
    for (int t = 0; t < ns; ++t) {
        const SnDesc& T = S.sn[t];
        for (int k = 0; k < T.r; ++k) {
            const int row = S.rows[T.pi + k];
            map[row] = k;
            stamp[row] = t;
        }
        for (int col = T.c0; !S.solve_only && col < T.c0 + T.w; ++col)
            for (int q = A2p[col]; q < A2p[col + 1]; ++q) {
                const int row = A2i[q];
                if (stamp[row] != t) throw std::runtime_error("schedule: A entry outside the pattern of L");
                S.a_dst[q] = (int64_t)lC[col] + map[row];
            }
        for (int64_t u = B.uptr[t]; u < B.uptr[t + 1]; ++u) {
            const SnDesc& D = S.sn[B.usn[u]];
            B.urel[u] = (int64_t)S.relpos.size();
            for (int k = B.ulb[u]; k < D.r; ++k) {
                const int row = S.rows[D.pi + k];
                if (stamp[row] != t)
                    throw std::runtime_error("schedule: descendant row missing from the target's pattern");
                S.relpos.push_back(map[row]);
            }
            const double K = D.w, m = D.r - B.ulb[u], n1 = B.uub[u] - B.ulb[u] + 1;
            S.update_flops += K * n1 * (n1 + 1) + 2.0 * K * (m - n1) * n1;
            S.reread_bytes += 8.0 * K * m;
        }
    }
    if (S.relpos.size() > 0x7fffffffULL) throw std::runtime_error("schedule: relative index array exceeds int32");
}

// Reads update_flops and the knobs.  Fills the sizes chosen by the job: big_min_k, piece_width, push_group.
// Which form the updates take follows the size of the job (measured on MI355X, 27-point grids with
// nested dissection): below about 1e11 update flops a factorization is a chain of latencies and the
// wave streams inside the chain launches are the shortest path; above it the LDS-staged BIG launches
// win (56^3 grid: 11.8 vs 13.1 ms); cutting the very wide supernodes into pieces pays from about 2e12
// (96^3 grid: 163 vs 174 ms).  PARSY_BIG_MINK / PARSY_PIECE_WIDTH override (diagnostics, tests).
void choose_sizes(Schedule& S, const BuildKnobs& K) {
    S.big_min_k = S.update_flops >= kBigAutoFlops ? kBigMinK : INT_MAX;
    S.piece_width = S.update_flops >= kPieceAutoFlops ? kPieceWidth : 0;
    if (K.big_mink_set) S.big_min_k = K.big_mink;
    if (K.piece_width_set) S.piece_width = K.piece_width;
    if (S.piece_width > 0) S.piece_width = ceil_div(std::max(S.piece_width, kBigTile), kBigTile) * kBigTile;
    if (S.piece_width < S.big_min_k) S.piece_width = 0;  // the pieces update each other through the BIG launches
    S.push_group = K.push_group;
}

// Reads P.sparent, S.sn, piece_width.  Fills the etree and its level sets (sparent, levelPtr / levelSet, nlevels; B.tree)
// and the Cholesky view: the pieces of the very wide supernodes (csn, piece0, csn_real) and their levels (clevelPtr /
// clevelSet, cnlevels, level_of).
void cut_pieces(const PatternRef& P, Schedule& S, BuildState& B) {
    const int ns = S.nsuper;
    B.tree.assign(P.sparent, P.sparent + ns);
    S.sparent = B.tree;
    level_sets(B.tree, S.levelPtr, S.levelSet);
    S.nlevels = (int)S.levelPtr.size() - 1;

    S.piece0.assign(ns + 1, 0);
    for (int t = 0; t < ns; ++t) {
        const SnDesc& T = S.sn[t];
        S.piece0[t] = (int32_t)S.csn.size();
        int np = 1;
        const int pw = S.piece_width;
        if (!S.solve_only && pw > 0 && T.w > pw + pw / 2) {
            np = ceil_div(T.w, pw);
            if (T.w - (np - 1) * pw < pw / 2) --np;  // a short remainder stays with the last piece
        }
        for (int j = 0; j < np; ++j) {
            const int off = j * pw;
            SnDesc c = T;
            c.c0 = T.c0 + off;
            c.w = (j == np - 1) ? T.w - off : pw;
            c.r = T.r - off;
            c.ld = T.r;
            c.rbias = off;
            c.px = T.px + (int64_t)off * T.r + off;
            c.pi = T.pi + off;
            c.dslot = -1;
            S.csn.push_back(c);
            S.csn_real.push_back(t);
        }
    }
    const int nc = (int)S.csn.size();
    S.piece0[ns] = nc;
    {
        std::vector<int> ctree(nc, -1);
        for (int t = 0; t < ns; ++t)
            for (int p = S.piece0[t]; p < S.piece0[t + 1]; ++p)
                ctree[p] = (p + 1 < S.piece0[t + 1]) ? p + 1 : (B.tree[t] >= 0 ? S.piece0[B.tree[t]] : -1);
        level_sets(ctree, S.clevelPtr, S.clevelSet);
    }
    S.cnlevels = (int)S.clevelPtr.size() - 1;
    S.level_of.assign(nc, 0);
    for (int l = 0; l < S.cnlevels; ++l)
        for (int q = S.clevelPtr[l]; q < S.clevelPtr[l + 1]; ++q) S.level_of[S.clevelSet[q]] = l;
}

// Reads the update lists (B), S.sn, the pieces, push_group.  Fills the update descriptors per piece (upd, upd_src, and
// upd0 / nupd of every piece): the supernode's descendants restricted to the piece's columns (reference order), then the
// pieces to its left (identity row map).
void describe_updates(Schedule& S, const BuildState& B) {
    const int ns = S.nsuper;
    for (int t = 0; t < ns && !S.solve_only; ++t) {
        const SnDesc& T = S.sn[t];
        for (int p = S.piece0[t]; p < S.piece0[t + 1]; ++p) {
            SnDesc& C = S.csn[p];
            C.upd0 = (int64_t)S.upd.size();
            const int col_lo = C.c0, col_hi = C.c0 + C.w;
            for (int64_t u = B.uptr[t]; u < B.uptr[t + 1]; ++u) {
                const SnDesc& D = S.sn[B.usn[u]];
                int lb = B.ulb[u], ub = B.uub[u];
                if (S.piece0[t + 1] - S.piece0[t] > 1) {
                    while (lb <= ub && S.rows[D.pi + lb] < col_lo) ++lb;
                    while (ub >= lb && S.rows[D.pi + ub] >= col_hi) --ub;
                    if (lb > ub) continue;
                }
                UpdDesc U;
                U.src = D.px + lb;
                U.ld = D.r;
                U.K = D.w;
                U.m = D.r - lb;
                U.n1 = ub - lb + 1;
                U.rel = B.urel[u] + (lb - B.ulb[u]);
                S.upd.push_back(U);
                S.upd_src.push_back(S.piece0[B.usn[u] + 1] - 1);
            }
            // the pieces to the left: the one right before this piece by itself (it is applied by the NEXT
            // launch of its level), the earlier ones in aligned groups of push_group pieces -- adjacent
            // columns of the same panel, one update with the summed width, due when the group's last
            // piece is complete (a group is cut short where this piece's turn comes first)
            const int j = p - S.piece0[t];
            for (int g0 = 0; g0 < j; ) {
                int g1 = (g0 == j - 1) ? j : std::min(j - 1, (g0 / S.push_group + 1) * S.push_group);
                const SnDesc& Q0 = S.csn[S.piece0[t] + g0];
                int K = 0;
                for (int q = g0; q < g1; ++q) K += S.csn[S.piece0[t] + q].w;
                UpdDesc U;
                U.src = T.px + (int64_t)Q0.rbias * T.r + C.rbias;
                U.ld = T.r;
                U.K = K;
                U.m = C.r;
                U.n1 = C.w;
                U.rel = -1;
                S.upd.push_back(U);
                S.upd_src.push_back(S.piece0[t] + g1 - 1);
                g0 = g1;
            }
            C.nupd = (int)((int64_t)S.upd.size() - C.upd0);
        }
    }
}

// Reads the etree (B.tree), S.sn, the pieces and their updates, the knobs, B.compute_units.  Fills the subtrees walked by
// one workgroup each (see schedule.hpp): chol_ / solve_ / bsolve_subtree, chol_cost / solve_cost and the three counts.
// Cost in flop equivalents: what the
// SMALL kernel executes plus a fixed amount per supernode and update (the small ones are latency);
// solves: panel entries.  The cap aims at kSubtreesPerCu subtrees per compute unit.
// A workgroup walks the supernodes of its subtree one after the other, siblings included, which level
// launches would run side by side: that only pays when the bottom of the etree saturates the device anyway
// (measured on MI355X: 45 000 narrow supernodes: factor -3 %, backward solve -7 %, forward solve -3 %;
// 1 300 .. 3 300 of them: +1 .. +9 % with subtrees), so by default subtrees are cut only where the
// eligible supernodes number at least kSubtreeMinPerSlot per subtree aimed at.
// PARSY_SUBTREES=k: always cut, aiming at k subtrees per compute unit (0: never; diagnostics, tests).
void cut_subtrees(Schedule& S, const BuildState& B) {
    const int ns = S.nsuper;
    const bool forced = B.knobs.subtrees_set;
    const int per_cu = B.knobs.subtrees_per_cu;
    if (per_cu > 0) {
        const int cus = B.compute_units > 0 ? B.compute_units : 256;
        std::vector<uint8_t> elig(ns, 0);
        auto cut = [&](std::vector<double>& cost, double min_cost, std::vector<int32_t>& subtree,
                       const std::vector<std::pair<int32_t, int32_t>>* slots = nullptr, int64_t min_members = -1, int aim_per_cu = 0) {
            double total = 0;
            int64_t members = 0;
            {   // everything that could be in a subtree at all
                std::vector<int32_t> all;
                find_subtrees(B.tree, elig, cost, 1e300, all, slots, kSubMaxSlots);
                for (int t = 0; t < ns; ++t)
                    if (all[t] >= 0) {
                        total += cost[t];
                        ++members;
                    }
            }
            if (!forced && members < (min_members >= 0 ? min_members : (int64_t)kSubtreeMinPerSlot * per_cu * cus)) return 0;
            return find_subtrees(B.tree, elig, cost, std::max(min_cost, total / ((double)(aim_per_cu > 0 ? aim_per_cu : per_cu) * cus)), subtree, slots,
                                 kSubMaxSlots);
        };
        if (!S.solve_only) {
            S.chol_cost.assign(ns, 0.0);
            for (int t = 0; t < ns; ++t) {
                const SnDesc& C = S.csn[S.piece0[t]];
                elig[t] = S.piece0[t + 1] - S.piece0[t] == 1 && is_small(C);
                double c = 5e4 + (double)C.w * C.r * C.r;
                for (int64_t u = C.upd0; u < C.upd0 + C.nupd && elig[t]; ++u)
                    c += 1e4 + 2.0 * S.upd[u].K * (double)S.upd[u].m * S.upd[u].n1;
                S.chol_cost[t] = c;
            }
            // (the factorization's subtrees aim at more, smaller ones than the threshold above counts with: a workgroup
            // keeps a whole panel in LDS, one or two per compute unit, and the launch runs alone on the device -- Flan-class
            // 3.8 -> 2.9 ms with 64 per unit, 3.2 with 128: profiles/r05_dense_thresholds.txt.  PARSY_CHOL_SUBTREES)
            S.n_chol_subtrees = cut(S.chol_cost, kSubtreeMinCost, S.chol_subtree, nullptr, -1, forced ? 0 : B.knobs.chol_subtrees_per_cu);
        }
        S.solve_cost.assign(ns, 0.0);
        // solves: the subtrees of TINY supernodes (one wave walks one: the wave-per-supernode solve kernel)
        std::vector<std::pair<int32_t, int32_t>> slots((size_t)ns);
        for (int t = 0; t < ns; ++t) {
            elig[t] = S.sn[t].w <= kTinyWidth;
            S.solve_cost[t] = 2e3 + (double)S.sn[t].w * S.sn[t].r;
            slots[(size_t)t] = {S.sn[t].w, S.sn[t].r - S.sn[t].w};
        }
        // (the solves cut subtrees from far fewer supernodes on than the factorization: tools/gate_sweep.py, round 5 -- grids of
        // 3 400 .. 9 000 supernodes: forward solve -12 .. -23 %, 8 right-hand sides up to -44 %; 750 .. 1 450: +-8 %)
        S.n_solve_subtrees = cut(S.solve_cost, kSubtreeMinCost / 16, S.solve_subtree, &slots, kSolveSubtreeMinMembers);
        // (the backward solve walks the same subtrees from their roots down)
        S.bsolve_subtree = S.solve_subtree;
        S.n_bsolve_subtrees = S.n_solve_subtrees;
    }
    if (S.chol_subtree.empty()) S.chol_subtree.assign(ns, -1);
    if (S.solve_subtree.empty()) S.solve_subtree.assign(ns, -1);
    if (S.bsolve_subtree.empty()) S.bsolve_subtree.assign(ns, -1);
}

// Reads the pieces, their updates and levels, the knobs.  Fills B.launch_super and big_super_r / _c.
// Edge of a BIG task's super-tile in 128 x 128 tiles, rows x columns, per launch (source level, kind).  A launch
// with many tasks whose 128 x 128 windows are mostly ragged (a 128-row window of the target holds about 64 rows of
// a typical source) takes 2 x 2 super-tiles -- a source's rows inside the larger windows are cut into FULL
// 128 x 128 blocks in its own row order: a quarter fewer chunks for the same products -- the others (pushes
// between the pieces of a separator: full windows anyway; launches of few tasks: they end with their longest
// task) stay with single tiles.  Measured per launch on the Flan-class input (tools/big_launches.py): early levels
// 10.7 -> 7.8 ms, the big pushes 37 -> 34 ms, launches below ~12 000 tasks 3-10 % slower with super-tiles.
// PARSY_BIG_SUPER=RxC (or R) forces one size everywhere (diagnostics, tests).
void choose_super_tiles(Schedule& S, BuildState& B) {
    const BuildKnobs& K = B.knobs;
    const int nc = (int)S.csn.size();
    B.launch_super.assign((size_t)2 * std::max(S.cnlevels, 1), 1);
    if (K.super_r == 0 && !S.solve_only) {
        std::vector<int64_t> ltasks(B.launch_super.size(), 0);
        std::vector<double> lfrag(B.launch_super.size(), 0.0), lchunks(B.launch_super.size(), 0.0);
        std::vector<int64_t> keys;
        std::vector<RowRun> runs;
        for (int t = 0; t < nc; ++t) {
            const SnDesc& T = S.csn[t];
            if (is_small(T)) continue;
            const int lev_t = S.level_of[t], nbr128 = ceil_div(T.r, kBigTile);
            keys.clear();
            for (int64_t u = T.upd0; u < T.upd0 + T.nupd; ++u) {
                const UpdDesc& U = S.upd[u];
                if (!is_big(S, U, t)) continue;
                const int64_t launch = big_launch_of(S.level_of[S.upd_src[u]], lev_t);
                row_runs(S, T, U, kBigTile, runs);
                const double chunks = ceil_div(U.K, 16);
                for (const RowRun& gc : runs) {
                    if (gc.first >= U.n1) break;
                    const int nj = std::min(gc.len, U.n1 - gc.first);
                    for (const RowRun& gr : runs) {
                        if (gr.win < gc.win) continue;
                        keys.push_back((launch << 40) | ((int64_t)gc.win * nbr128 + gr.win));
                        lfrag[(size_t)launch] += chunks * ceil_div(gr.len, 16) * ceil_div(nj, 16);
                        lchunks[(size_t)launch] += chunks;
                    }
                }
            }
            std::sort(keys.begin(), keys.end());
            keys.erase(std::unique(keys.begin(), keys.end()), keys.end());
            for (int64_t k : keys) ltasks[(size_t)(k >> 40)]++;
        }
        for (size_t l = 0; l < B.launch_super.size(); ++l)
            if (ltasks[l] >= K.super_min_tasks && lfrag[l] < K.super_max_fill * 64.0 * lchunks[l]) B.launch_super[l] = (int8_t)K.super_hi;
    }
    S.big_super_r = K.super_r;
    S.big_super_c = K.super_c;
}

// Reads one tiled piece t and its updates that are not BIG.  Fills its wave streams (wave_entries, wave_ptr, sn_wp0[t]).
// Every (target, descendant) update is cut along the 32-row windows of the target's tiles:
// the descendant rows that fall into row window I32 times those (among its first n1 rows)
// that fall into column window J32 are one WaveEntry of sub-tile (I32, J32), I32 >= J32.
// Lists keep the reference's update order, so the sum order per entry of L is fixed.
// Updates from wide descendants (is_big) do not enter these lists: the BIG entries.
void piece_wave_streams(Schedule& S, int t, std::vector<RowRun>& runs, std::vector<int64_t>& cursor) {
    const SnDesc& T = S.csn[t];
    const int nbc = ceil_div(T.w, kTile), nbr = ceil_div(T.r, kTile), lev_t = S.level_of[t];
    // key of a list: ((J * nbr + I) * 2 + phase) * 4 + wave
    const size_t nkeys = (size_t)nbc * nbr * 8;
    auto for_each_entry = [&](auto&& fn) {
        for (int64_t u = T.upd0; u < T.upd0 + T.nupd; ++u) {
            const UpdDesc& U = S.upd[u];
            if (is_big(S, U, t)) continue;
            // early: the descendant is complete before the level below the target even starts
            const int phase = (S.level_of[S.upd_src[u]] <= lev_t - 2) ? 0 : 1;
            row_runs(S, T, U, kSub, runs);
            for (const RowRun& gc : runs) {
                if (gc.first >= U.n1) break;
                const int nj = std::min(gc.len, U.n1 - gc.first);
                for (const RowRun& gr : runs) {
                    if (gr.win < gc.win) continue;
                    const int I = gr.win / 2, J = gc.win / 2;
                    const size_t key = (((size_t)J * nbr + I) * 2 + phase) * 4 + (gr.win & 1) * 2 + (gc.win & 1);
                    fn(key, U, gr.first, gr.len, gc.first, nj);
                }
            }
        }
    };
    cursor.assign(nkeys + 1, 0);
    for_each_entry([&](size_t key, const UpdDesc&, int, int, int, int) { cursor[key + 1]++; });
    const int64_t base = (int64_t)S.wave_entries.size();
    for (size_t k = 0; k < nkeys; ++k) cursor[k + 1] += cursor[k];
    S.sn_wp0[t] = (int64_t)S.wave_ptr.size();
    for (size_t k = 0; k <= nkeys; ++k) S.wave_ptr.push_back(base + cursor[k]);
    S.wave_entries.resize((size_t)(base + cursor[nkeys]));
    for_each_entry([&](size_t key, const UpdDesc& U, int ia, int mi, int ja, int nj) {
        S.wave_entries[(size_t)(base + cursor[key]++)] =
            WaveEntry{U.src, (int32_t)U.rel, U.ld, U.K, ia, ja, mi | (nj << 8)};
    });
}

// Reads one tiled piece t's wave streams, B.level_tiles, the split knobs.  Fills the weight of its tiles (tile_w, sn_tw0[t])
// = 16-wide k chunks of a tile's longest wave stream, and the splits of its long early streams (tile_split, split_desc,
// split_ranges, n_split_doubles).
void piece_tile_weights(Schedule& S, const BuildState& B, int t) {
    const BuildKnobs& K = B.knobs;
    const SnDesc& T = S.csn[t];
    const int nbc = ceil_div(T.w, kTile), nbr = ceil_div(T.r, kTile), lev_t = S.level_of[t];
    S.sn_tw0[t] = (int64_t)S.tile_w.size();
    S.tile_w.resize(S.tile_w.size() + (size_t)nbc * nbr * 2, 0);
    S.tile_split.resize(S.tile_w.size() / 2, -1);
    int32_t* tw = &S.tile_w[S.sn_tw0[t]];
    int64_t* tsplit = &S.tile_split[S.sn_tw0[t] / 2];
    const int64_t* wp = &S.wave_ptr[S.sn_wp0[t]];
    for (size_t tp = 0; tp < (size_t)nbc * nbr * 2; ++tp) {
        int64_t wchunks[4];
        for (int q = 0; q < 4; ++q) {
            int64_t chunks = 0;
            for (int64_t e = wp[tp * 4 + q]; e < wp[tp * 4 + q + 1]; ++e)
                chunks += ceil_div(S.wave_entries[(size_t)e].K, 16);
            wchunks[q] = chunks;
            tw[tp] = std::max<int32_t>(tw[tp], (int32_t)std::min<int64_t>(chunks, INT32_MAX));
        }
        // A launch ends with its longest wave stream: long EARLY streams are cut into parts that
        // separate workgroups apply to partial tiles (summed, in a fixed order, when the chain
        // launch loads the tile).  Every wave's list is cut where its own chunk count reaches p/nparts.
        // (PARSY_SPLIT_CHUNKS set: one rule for every level -- diagnostics)
        const bool few = B.level_tiles[(size_t)lev_t] <= kSplitFewTiles && !K.split_chunks_set;
        if ((tp & 1) == 0 && tw[tp] > (few ? kSplitFewChunks : K.split_chunks)) {
            const int nparts = few ? std::min<int>(kSplitFewMaxParts, ceil_div(tw[tp], kSplitFewTarget))
                                   : std::min<int>(K.split_max, ceil_div(tw[tp], K.split_target));
            Schedule::SplitDesc sd{(int64_t)S.split_ranges.size(), S.n_split_doubles, nparts, 0};
            S.n_split_doubles += (int64_t)(nparts - 1) * kTile * kTile;
            S.split_ranges.resize(S.split_ranges.size() + (size_t)nparts * 8, 0);
            int64_t* rg = &S.split_ranges[(size_t)sd.ranges];
            for (int q = 0; q < 4; ++q) {
                int64_t e = wp[tp * 4 + q], done = 0;
                for (int part = 0; part < nparts; ++part) {
                    rg[part * 8 + 2 * q] = e;
                    const int64_t goal = wchunks[q] * (part + 1) / nparts;
                    while (e < wp[tp * 4 + q + 1] && (part == nparts - 1 || done < goal))
                        done += ceil_div(S.wave_entries[(size_t)e++].K, 16);
                    rg[part * 8 + 2 * q + 1] = e;
                }
            }
            tsplit[tp / 2] = (int64_t)S.split_desc.size();
            S.split_desc.push_back(sd);
        }
    }
}

// Reads the pieces, their updates and levels.  Fills, per tiled piece: the tile flags (tflag0, n_tflags), inner_flops, the wave
// streams, the tile weights and the splits (the two functions above); n_small / n_big; B.level_tiles.
void build_wave_streams(Schedule& S, BuildState& B) {
    const int nc = (int)S.csn.size();
    S.sn_wp0.assign(nc, -1);
    S.sn_tw0.assign(nc, -1);
    // tiles per level: a level with few of them leaves the device empty while its longest early stream runs (ex15-class:
    // 2 - 12 workgroups for 47 - 76 us per level, the critical path of the upper half of the tree) -- there the streams
    // are cut finer (kSplitFew*)
    B.level_tiles.assign((size_t)std::max(S.cnlevels, 1), 0);
    if (S.solve_only) return;
    for (int t = 0; t < nc; ++t)
        if (!is_small(S.csn[t])) {
            const int nbc = ceil_div(S.csn[t].w, kTile), nbr = ceil_div(S.csn[t].r, kTile);
            B.level_tiles[(size_t)S.level_of[t]] += (int64_t)nbc * nbr - (int64_t)nbc * (nbc - 1) / 2;
        }
    std::vector<RowRun> runs;
    std::vector<int64_t> cursor;
    for (int t = 0; t < nc; ++t) {
        SnDesc& T = S.csn[t];
        if (is_small(T)) {
            S.n_small++;
            continue;
        }
        S.n_big++;
        const int nbc = ceil_div(T.w, kTile), nbr = ceil_div(T.r, kTile);
        if (S.n_tflags + (int64_t)nbc * nbr > 0x7fffffffLL) throw std::runtime_error("schedule: too many tiles");
        T.tflag0 = (int32_t)S.n_tflags;
        S.n_tflags += (int64_t)nbc * nbr;
        for (int jb = 1; jb < nbc; ++jb) {
            const double K = (double)jb * kTile, wb = std::min(kTile, T.w - jb * kTile);
            S.inner_flops += K * wb * (wb + 1) + 2.0 * K * (double)(T.r - jb * kTile - wb) * wb;
        }
        piece_wave_streams(S, t, runs, cursor);
        piece_tile_weights(S, B, t);
    }
}

// The blocks of update U into piece T under the TILE cut, a task per super-tile of sr x sc 128 x 128 tiles of the target:
// fn(row window, column window, ia, mi, ja, nj).
// The source's rows inside the super-tile's row window (a run of its panel rows) times its rows inside the column window
// are cut into 128 x 128 blocks IN THE SOURCE'S ROW ORDER -- full blocks but for the last of a run -- one entry each:
// a 128-row window of the target holds only about 64 rows of a typical source (a face of a sub-box on a
// separator plane), so per-tile windows were two-thirds ragged (tools/big_stats.py).
template <class Fn>
void tile_cut_blocks(const Schedule& S, const SnDesc& T, const UpdDesc& U, int sr, int sc, std::vector<RowRun>& runs,
                     std::vector<RowRun>& cruns, Fn&& fn) {
    row_runs(S, T, U, kBigTile * sr, runs);
    if (sc == sr) cruns = runs;
    else row_runs(S, T, U, kBigTile * sc, cruns);
    for (const RowRun& gc : cruns) {
        if (gc.first >= U.n1) break;
        const int njt = std::min(gc.len, U.n1 - gc.first);
        for (const RowRun& gr : runs) {
            // (the target's rows ascend with the source's: a window strictly above the diagonal holds nothing)
            if ((int64_t)(gr.win + 1) * sr * kBigTile - 1 < (int64_t)gc.win * sc * kBigTile) continue;
            for (int cb = 0; cb < njt; cb += kBigTile)
                for (int rb = 0; rb < gr.len; rb += kBigTile) {
                    const int mi = std::min(kBigTile, gr.len - rb), nj = std::min(kBigTile, njt - cb);
                    const int ia = gr.first + rb, ja = gc.first + cb;
                    if (ia + mi - 1 < ja) continue;   // block strictly above the diagonal
                    fn(gr.win, gc.win, ia, mi, ja, nj);
                }
        }
    }
}

// The blocks of update U under the RE-CUT of a conflict domain whose members all have U's rows (find_conflict_domains): the
// domain's index is then the source's own row order, cut into windows of kBigTile consecutive positions; a task is one
// (row window, column window), a block is one 128 x 128 square of the source's rows x its first n1 rows:
// fn(row window, column window, ia, mi, ja, nj, rides).
// A remainder of <= kStripMax rows (columns) right behind (beside) a full block goes to that block's task where strips
// ride with dense blocks (`strips`): the strip pairing of build_big_tasks looks for it there.  The corner of two
// remainders stays a task of its own: it rides with nothing, and a second entry would double its neighbour's length.
template <class Fn>
void recut_blocks(const UpdDesc& U, bool strips, Fn&& fn) {
    strips = strips && U.K >= kDenseChunk;
    for (int ja = 0; ja < U.n1; ja += kBigTile)
        for (int ia = ja; ia < U.m; ia += kBigTile) {   // (ia < ja: strictly above the diagonal)
            const int mi = std::min(kBigTile, U.m - ia), nj = std::min(kBigTile, U.n1 - ja);
            const bool row_strip = strips && mi <= kStripMax && nj == kBigTile && ia >= ja + kBigTile;
            const bool col_strip = strips && !row_strip && nj <= kStripMax && mi == kBigTile && ja >= kBigTile;
            fn(ia / kBigTile - row_strip, ja / kBigTile - col_strip, ia, mi, ja, nj, row_strip || col_strip);
        }
}

// Issued work of one block at the measured rates, in ns (the decision of find_conflict_domains):
// k_chol_dense multiplies the whole 128 x 128 block per 8-wide k chunk whatever the window holds, a strip that rides with
// a full block costs an eighth of that, k_chol_big pays a fixed part per 16-wide chunk and a part per 16 x 16 fragment.
int64_t issued_ns(const BuildKnobs& K, int mi, int nj, int k, bool rides) {
    if (rides) return (int64_t)ceil_div(k, kDenseChunk) * kIssueStripNs;
    const bool dense = K.dense_mode != 0 && k >= kDenseChunk && (K.dense_mode == 4 || mi * nj >= K.dense_fill_min);
    if (dense) return (int64_t)ceil_div(k, kDenseChunk) * kIssueDenseNs;
    return (int64_t)ceil_div(k, 16) * (kIssueRaggedNs + (int64_t)kIssueFragmentNs * ceil_div(mi, 16) * ceil_div(nj, 16));
}

// The INTERVAL cut of a conflict domain whose members' rows differ (find_conflict_domains): where its intervals start.
// The members' rows are swept by their position in T's panel, all members merged.  An interval starts at position 0, at
// T.w -- so that the column intervals are exactly the intervals below T.w -- and at the first position where some member
// would receive row kBigTile + 1 of the current interval.  Every member then has at most kBigTile rows in an interval,
// consecutive in its own panel because positions ascend with its own row order: two faces of 64 rows each per 128 target
// rows grow an interval to 256 target rows that holds one full block of each.
void interval_bounds(const Schedule& S, const SnDesc& T, const std::vector<const UpdDesc*>& members,
                     std::vector<std::pair<int32_t, int32_t>>& rows, std::vector<int32_t>& count, std::vector<int32_t>& bounds) {
    rows.clear();
    for (size_t q = 0; q < members.size(); ++q)
        for (int k = 0; k < members[q]->m; ++k) rows.push_back({rel_at(S, T, *members[q], k), (int32_t)q});
    std::sort(rows.begin(), rows.end());
    count.assign(members.size(), 0);
    bounds.assign(1, 0);
    for (size_t a = 0, b; a < rows.size(); a = b) {
        const int32_t pos = rows[a].first;
        for (b = a; b < rows.size() && rows[b].first == pos; ++b) {}
        int32_t start = 0;
        if (pos >= T.w && bounds.back() < T.w) start = T.w;
        for (size_t c = a; c < b && !start; ++c)
            if (count[(size_t)rows[c].second] == kBigTile) start = pos;
        if (start) {
            bounds.push_back(start);
            std::fill(count.begin(), count.end(), 0);
        }
        for (size_t c = a; c < b; ++c) ++count[(size_t)rows[c].second];
    }
}

// The blocks of update U under the INTERVAL cut of its domain, whose nb intervals start at bounds[0 .. nb):
// fn(row interval, column interval, ia, mi, ja, nj) -- the member's run of rows in the one times its run in the other,
// both in its own row numbering.  A block strictly above the diagonal is dropped as tile_cut_blocks drops it, one that
// straddles it is kept whole.
template <class Fn>
void interval_blocks(const Schedule& S, const SnDesc& T, const UpdDesc& U, const int32_t* bounds, int nb, std::vector<RowRun>& runs,
                     Fn&& fn) {
    runs.clear();
    int w = 0;
    for (int k = 0; k < U.m;) {
        const int pos = rel_at(S, T, U, k);
        while (w + 1 < nb && bounds[w + 1] <= pos) ++w;
        int k1 = k + 1;
        while (k1 < U.m && (w + 1 >= nb || rel_at(S, T, U, k1) < bounds[w + 1])) ++k1;
        if (k1 - k > kBigTile) throw std::runtime_error("schedule: an interval holds more than a block of one update's rows");
        runs.push_back(RowRun{w, k, k1 - k});
        k = k1;
    }
    for (const RowRun& gc : runs) {
        if (gc.first >= U.n1) break;
        const int nj = std::min(gc.len, U.n1 - gc.first);
        for (const RowRun& gr : runs) {
            if (gr.win < gc.win || gr.first + gr.len - 1 < gc.first) continue;   // block strictly above the diagonal
            fn(gr.win, gc.win, gr.first, gr.len, gc.first, nj);
        }
    }
}

// Reads the pieces, their updates and levels, B.launch_super, the knobs.  Fills B.upd_domain, B.upd_bounds, B.bounds.
// CONFLICT DOMAINS. The tile grid exists to fix the order of sums: an entry (r, c) of L is written by source A only
// if both r and c are rows of A, so two sources of one launch meet on a target piece only if they share a row that is
// one of the piece's columns.  Per BIG launch and target piece -- over all sources, whatever is active, so that every
// rank of a distributed run decides alike -- the sources that share a column (transitively) are one domain; different
// domains write disjoint entries even inside one tile.  A domain whose members all have the SAME rows in the piece (a
// single source; the two sides of a separator plane) is cut in the members' own row order instead of on the grid
// (recut_blocks): windows of 128 positions are full but for the last, where a 128-row window of the target held about 64
// rows.  Taken only where it issues less work (issued_ns), a function of the pattern and the knobs alone; every other
// domain keeps the tile cut.  PARSY_BIG_RECUT=0: the tile cut everywhere.
// A domain whose members' rows DIFFER (the faces of neighbouring sub-boxes, chained through shared columns) is cut in
// intervals of the target's positions (interval_bounds, interval_blocks) where that issues less than the tile cut AND the
// TAIL GUARD holds: its longest interval task issues no more than the larger of its longest task under the tile cut and
// the launch's work under the tile cut / kIssueSlots.  An interval task holds a block of every member, so it is longer
// than a tile's; with tasks dealt heaviest first, one below the per-slot average cannot be what ends a launch, and one no
// longer than the tile cut's longest ends it no later (forcing 4 x 4 super-tiles lost 19 ms of dense time to long last
// tasks).  PARSY_BIG_RECUT=1: never; 3: without the guard.
void find_conflict_domains(Schedule& S, BuildState& B) {
    const BuildKnobs& K = B.knobs;
    const int nc = (int)S.csn.size();
    B.upd_domain.assign(S.upd.size(), 0);
    B.upd_bounds.assign(S.upd.size(), -1);
    B.bounds.clear();
    // The interval cut is the default from the size on at which it was measured (Flan-class: the multi-source launches
    // of a job whose supernodes are cut into pieces run for milliseconds each); smaller jobs, and plans whose BIG launches
    // exist only because a diagnostic knob forces them, keep the cut of domains of one row set unless the knob says otherwise;
    // so does a plan with one super-tile shape forced on every launch (PARSY_BIG_SUPER: a diagnostic of the tile cut).
    const int recut = K.big_recut_set || (S.update_flops >= kPieceAutoFlops && !K.super_r) ? K.big_recut : 1;
    if (S.solve_only || !recut) return;
    std::vector<RowRun> runs, cruns;
    auto super_of = [&](int64_t launch) {
        return std::pair<int, int>{K.super_r ? K.super_r : B.launch_super[(size_t)launch], K.super_r ? K.super_c : B.launch_super[(size_t)launch]};
    };
    // the tail guard's per-slot average: every launch's issued work under the tile cut, over all targets
    std::vector<int64_t> launch_tile_ns(B.launch_super.size(), 0);
    if (recut == 2)
        for (int t = 0; t < nc; ++t) {
            const SnDesc& T = S.csn[t];
            if (is_small(T)) continue;
            for (int64_t u = T.upd0; u < T.upd0 + T.nupd; ++u) {
                const UpdDesc& U = S.upd[u];
                if (!is_big(S, U, t)) continue;
                const int64_t launch = big_launch_of(S.level_of[S.upd_src[u]], S.level_of[t]);
                const auto [sr, sc] = super_of(launch);
                int64_t ns = 0;
                tile_cut_blocks(S, T, U, sr, sc, runs, cruns, [&](int, int, int, int mi, int, int nj) { ns += issued_ns(K, mi, nj, U.K, false); });
                launch_tile_ns[(size_t)launch] += ns;
            }
        }
    std::vector<const UpdDesc*> member_upd;
    std::vector<std::pair<int32_t, int32_t>> sweep_rows;
    std::vector<int32_t> sweep_count, ivals;
    std::map<std::pair<int, int>, int64_t> tile_task, ival_task;   // issued ns of the domain's entries per task of either cut
    std::set<std::array<int, 4>> full_blocks;                      // (row window, column window, ia, ja) of a member's full blocks
    // (the strips count as riding wherever k_chol_dense is used, whatever PARSY_DENSE_STRIPS says: that knob changes the strips
    // of a plan, not the cut of its interval domains)
    const bool strips = K.dense_mode != 0;
    auto longest = [](const std::map<std::pair<int, int>, int64_t>& m) {
        int64_t v = 0;
        for (const auto& kv : m) v = std::max(v, kv.second);
        return v;
    };
    std::vector<std::pair<int64_t, int64_t>> big;   // (launch, update) of one piece's BIG updates
    std::vector<int64_t> owner;                     // per column of the piece: launch << 32 | first member that names it
    std::vector<int32_t> root;                      // union-find over the members of one launch, the smallest index on top
    std::vector<std::pair<int32_t, int32_t>> members;   // (domain, member), sorted
    auto find = [&](int32_t x) {
        while (root[(size_t)x] != x) x = root[(size_t)x] = root[(size_t)root[(size_t)x]];
        return x;
    };
    for (int t = 0; t < nc; ++t) {
        const SnDesc& T = S.csn[t];
        if (is_small(T)) continue;
        big.clear();
        for (int64_t u = T.upd0; u < T.upd0 + T.nupd; ++u)
            if (is_big(S, S.upd[u], t)) big.push_back({big_launch_of(S.level_of[S.upd_src[u]], S.level_of[t]), u});
        std::stable_sort(big.begin(), big.end(), [](const auto& a, const auto& b) { return a.first < b.first; });
        owner.assign((size_t)T.w, -1);
        for (size_t i = 0; i < big.size();) {
            size_t j = i;
            while (j < big.size() && big[j].first == big[i].first) ++j;
            const int64_t launch = big[i].first;
            const int32_t nm = (int32_t)(j - i);
            root.resize((size_t)nm);
            for (int32_t q = 0; q < nm; ++q) {
                root[(size_t)q] = q;
                const UpdDesc& U = S.upd[big[i + q].second];
                for (int k = 0; k < U.n1; ++k) {
                    const int c = rel_at(S, T, U, k);
                    if (c < 0 || c >= T.w) throw std::runtime_error("schedule: a column row of an update lies outside its target");
                    int64_t& o = owner[(size_t)c];
                    if (o < 0 || (o >> 32) != launch) {
                        o = (launch << 32) | q;
                        continue;
                    }
                    const int32_t a = find(q), b = find((int32_t)(o & 0xffffffff));
                    if (a < b) root[(size_t)b] = a;
                    else root[(size_t)a] = b;
                }
            }
            const auto [sr, sc] = super_of(launch);
            members.clear();
            for (int32_t q = 0; q < nm; ++q) members.push_back({find(q), q});
            std::sort(members.begin(), members.end());
            for (size_t d0 = 0, d1; d0 < members.size(); d0 = d1) {
                const int32_t q = members[d0].first;   // (= its first member: the smallest index is on top)
                for (d1 = d0; d1 < members.size() && members[d1].first == q; ++d1) {}
                // every member with q's rows?
                const UpdDesc& U0 = S.upd[big[i + q].second];
                bool same = true;
                for (size_t d = d0 + 1; d < d1 && same; ++d) {
                    const UpdDesc& U = S.upd[big[i + members[d].second].second];
                    same = U.m == U0.m && U.n1 == U0.n1;
                    for (int k = 0; k < U.m && same; ++k) same = rel_at(S, T, U, k) == rel_at(S, T, U0, k);
                }
                const int64_t first = big[i + q].second - T.upd0;
                if (first >= kIntervalDomain - 1) throw std::runtime_error("schedule: too many updates of one piece");
                if (!same) {
                    if (recut < 2) continue;
                    // rows differ: intervals of the target's positions, or the tile cut
                    member_upd.clear();
                    for (size_t d = d0; d < d1; ++d) member_upd.push_back(&S.upd[big[i + members[d].second].second]);
                    interval_bounds(S, T, member_upd, sweep_rows, sweep_count, ivals);
                    if (ivals.size() >= 0xffff) throw std::runtime_error("schedule: too many intervals of one conflict domain");
                    tile_task.clear();
                    ival_task.clear();
                    int64_t tile_ns = 0, ival_ns = 0;
                    for (const UpdDesc* U : member_upd) {
                        // (under the tile cut a remainder right behind or beside a full block of its task rides with it
                        // as a strip -- build_big_tasks; the full block comes first in the task's runs)
                        full_blocks.clear();
                        tile_cut_blocks(S, T, *U, sr, sc, runs, cruns, [&](int wr, int wc, int ia, int mi, int ja, int nj) {
                            const bool row_strip = mi <= kStripMax && nj == kBigTile, col_strip = nj <= kStripMax && mi == kBigTile;
                            if (mi == kBigTile && nj == kBigTile) full_blocks.insert({wr, wc, ia, ja});
                            const bool rides = strips && U->K >= kDenseChunk && (row_strip || col_strip) &&
                                               full_blocks.count({wr, wc, ia - (row_strip ? kBigTile : 0), ja - (col_strip ? kBigTile : 0)}) != 0;
                            const int64_t ns = issued_ns(K, mi, nj, U->K, rides);
                            tile_ns += ns;
                            tile_task[{wr, wc}] += ns;
                        });
                        interval_blocks(S, T, *U, ivals.data(), (int)ivals.size(), runs, [&](int wr, int wc, int, int mi, int, int nj) {
                            const int64_t ns = issued_ns(K, mi, nj, U->K, false);
                            ival_ns += ns;
                            ival_task[{wr, wc}] += ns;
                        });
                    }
                    if (ival_ns >= tile_ns) continue;
                    if (recut == 2 &&
                        longest(ival_task) > std::max(longest(tile_task), launch_tile_ns[(size_t)launch] / kIssueSlots))
                        continue;
                    const int64_t at = (int64_t)B.bounds.size();
                    B.bounds.push_back((int32_t)ivals.size());
                    B.bounds.insert(B.bounds.end(), ivals.begin(), ivals.end());
                    for (size_t d = d0; d < d1; ++d) {
                        const size_t u = (size_t)big[i + members[d].second].second;
                        B.upd_domain[u] = kIntervalDomain + (int32_t)first + 1;
                        B.upd_bounds[u] = at;
                    }
                    continue;
                }
                int64_t tile_ns = 0, recut_ns = 0;
                for (size_t d = d0; d < d1; ++d) {
                    const UpdDesc& U = S.upd[big[i + members[d].second].second];
                    tile_cut_blocks(S, T, U, sr, sc, runs, cruns, [&](int, int, int, int mi, int, int nj) {
                        tile_ns += issued_ns(K, mi, nj, U.K, false);
                    });
                    recut_blocks(U, K.dense_strips && K.dense_mode != 0, [&](int, int, int, int mi, int, int nj, bool rides) {
                        recut_ns += issued_ns(K, mi, nj, U.K, rides);
                    });
                }
                if (recut_ns >= tile_ns) continue;
                for (size_t d = d0; d < d1; ++d) B.upd_domain[(size_t)big[i + members[d].second].second] = (int32_t)first + 1;
            }
            i = j;
        }
    }
}

// Reads the pieces, their updates and levels, B.launch_super, B.upd_domain.  Fills the BIG entries as they are found, keyed
// by (launch, tile) or (launch, piece, domain, window): B.bigk, B.big_tile0; big_flops and tile_update_flops (the updates
// that are not BIG).
// BIG: the wide descendants, cut along the 128-row windows of the target's panel
void collect_big_entries(Schedule& S, BuildState& B) {
    const int nc = (int)S.csn.size();
    const int env_sr = B.knobs.super_r, env_sc = B.knobs.super_c;
    B.big_tile0.assign((size_t)nc + 1, 0);
    std::vector<RowRun> runs, cruns;
    for (int t = 0; t < nc; ++t) {
        const SnDesc& T = S.csn[t];
        B.big_tile0[t + 1] = B.big_tile0[t];
        if (S.solve_only || is_small(T)) continue;
        const int lev_t = S.level_of[t];
        const int nbr128 = ceil_div(T.r, kBigTile), nbc128 = ceil_div(T.w, kBigTile);
        B.big_tile0[t + 1] = B.big_tile0[t] + (int64_t)nbr128 * nbc128;
        for (int64_t u = T.upd0; u < T.upd0 + T.nupd; ++u) {
            const UpdDesc& U = S.upd[u];
            const double f = (double)U.K * U.n1 * (U.n1 + 1) + 2.0 * U.K * (double)(U.m - U.n1) * U.n1;
            if (!is_big(S, U, t)) {
                S.tile_update_flops += f;
                continue;
            }
            S.big_flops += f;
            const int lev_s = S.level_of[S.upd_src[u]];
            if (lev_s >= lev_t) throw std::runtime_error("schedule: an update source is not below its target");
            const int64_t launch = big_launch_of(lev_s, lev_t);
            const int sr = env_sr ? env_sr : B.launch_super[(size_t)launch], sc = env_sr ? env_sc : B.launch_super[(size_t)launch];
            auto entry = [&](int ia, int mi, int ja, int nj) {
                return WaveEntry{U.src, (int32_t)std::max<int64_t>(U.rel, 0), U.ld, U.K, ia, ja, mi | (nj << 8) | ((U.rel < 0) << 16)};
            };
            const int64_t domain = B.upd_domain[(size_t)u];
            if (domain >= kIntervalDomain) {
                // an interval domain: a task owns one (row interval, column interval) of the target's positions
                const int32_t* iv = &B.bounds[(size_t)B.upd_bounds[(size_t)u]];
                interval_blocks(S, T, U, iv + 1, iv[0], runs, [&](int wr, int wc, int ia, int mi, int ja, int nj) {
                    B.bigk.push_back(BigKeyed{(launch << 40) | B.big_tile0[t], (domain << 32) | ((int64_t)wc << 16) | wr,
                                              entry(ia, mi, ja, nj), 1, 1});
                });
                continue;
            }
            if (domain) {
                // a re-cut domain: a task owns one (row window, column window) of the members' own row order
                if (U.m / kBigTile >= 0xffff) throw std::runtime_error("schedule: too many windows of one update");
                recut_blocks(U, B.knobs.dense_strips && B.knobs.dense_mode != 0, [&](int wr, int wc, int ia, int mi, int ja, int nj, bool) {
                    B.bigk.push_back(BigKeyed{(launch << 40) | B.big_tile0[t], (domain << 32) | ((int64_t)wc << 16) | wr,
                                              entry(ia, mi, ja, nj), 1, 1});
                });
                continue;
            }
            // A task owns a SUPER-TILE of sr x sc 128 x 128 tiles of the target (tile_cut_blocks).  The blocks of one
            // source touch different entries of L; the sources stay in update order.
            tile_cut_blocks(S, T, U, sr, sc, runs, cruns, [&](int wr, int wc, int ia, int mi, int ja, int nj) {
                const int64_t tile = B.big_tile0[t] + (int64_t)wc * sc * nbr128 + (int64_t)wr * sr;
                B.bigk.push_back(BigKeyed{(launch << 40) | tile, 0, entry(ia, mi, ja, nj), (int16_t)sr, (int16_t)sc});
            });
        }
    }
}

// Reads B.bigk (sorted by launch) and the dense knobs.  Returns per launch: 0 = k_chol_big only; 1 = full blocks to
// k_chol_dense, the rest to k_chol_big; 2 = everything to
// k_chol_dense (it multiplies a ragged window as a whole block and drops what the window does not have) --
// where the ragged rest is so small (the last, partial row block of the pushes between a separator's pieces: a
// handful of tasks) that a launch of its own would cost more than the wasted products: measured 0.07 - 0.1 ms
// per such launch, 110 of them per Flan-class factorization.
// Dense entries: full 128 x 128 blocks of the source's rows (on or below the target's diagonal; a block that
// straddles it -- the diagonal blocks of the pushes between a separator's pieces -- is multiplied whole and its
// upper part dropped when the tile is updated: 1.4 % more products there, and no ragged launch of a few hundred
// diagonal blocks behind every such push).  A launch hands them to k_chol_dense when
// they carry at least kDenseMinShare of its products; decided per launch over ALL targets, so that the order of
// sums does not depend on which pieces a rank owns.
std::vector<uint8_t> dense_share_per_launch(const BuildState& B) {
    const BuildKnobs& K = B.knobs;
    std::vector<double> lprod(B.launch_super.size(), 0.0), ldense(B.launch_super.size(), 0.0);
    for (const BigKeyed& b : B.bigk) {
        const WaveEntry& E = b.e;
        const size_t l = (size_t)(b.launch_tile >> 40);
        const double products = (double)ceil_div(E.K, 4) * ceil_div(entry_rows(E), 16) * ceil_div(entry_cols(E), 16);
        lprod[l] += products;
        if (entry_rows(E) == kBigTile && entry_cols(E) == kBigTile && E.K >= kDenseChunk) ldense[l] += products;
    }
    std::vector<uint8_t> launch_dense(B.launch_super.size(), 0);
    for (size_t l = 0; l < launch_dense.size(); ++l) {
        if (K.dense_mode == 4) {   // (tests: every entry of every launch through k_chol_dense, ragged windows and all)
            launch_dense[l] = lprod[l] > 0 ? 2 : 0;
            continue;
        }
        if (K.dense_mode == 0 || ldense[l] <= 0) continue;
        if (K.dense_mode >= 2 || ldense[l] >= K.dense_min_share * lprod[l]) launch_dense[l] = 1;
        if (launch_dense[l] && lprod[l] - ldense[l] <= K.dense_all_share * lprod[l] && K.dense_mode != 3) launch_dense[l] = 2;
    }
    return launch_dense;
}

// Reads B.bigk, B.big_tile0, the dense knobs.  Fills the BIG tasks, one per (launch, tile), entries in update order (stable
// sort): big_entries, big_all, dense_flops, n_dense_entries, n_strip_entries.
void build_big_tasks(Schedule& S, BuildState& B) {
    std::vector<BigKeyed>& bigk = B.bigk;
    if (bigk.empty()) return;
    const int nc = (int)S.csn.size();
    std::stable_sort(bigk.begin(), bigk.end(),
                     [](const BigKeyed& a, const BigKeyed& b) {
                         return a.launch_tile != b.launch_tile ? a.launch_tile < b.launch_tile : a.window < b.window;
                     });
    const std::vector<uint8_t> launch_dense = dense_share_per_launch(B);
    // mode 1: full blocks, and windows filled well enough that a whole-block product beats the ragged kernel's rate
    const int fill_min = B.knobs.dense_fill_min;
    auto is_dense = [fill_min](const WaveEntry& E, int mode) {
        if (mode == 2) return E.K >= kDenseChunk;
        return mode == 1 && E.K >= kDenseChunk && entry_rows(E) * entry_cols(E) >= fill_min;
    };
    S.big_entries.resize(bigk.size());
    std::map<std::pair<int64_t, int64_t>, size_t> strip_of;   // (source, ia << 32 | ja) of a task's full dense blocks
    std::vector<uint8_t> absorbed;
    int t = 0;
    for (size_t i = 0; i < bigk.size();) {
        size_t j = i;
        while (j < bigk.size() && bigk[j].launch_tile == bigk[i].launch_tile && bigk[j].window == bigk[i].window) ++j;
        const int64_t launch = bigk[i].launch_tile >> 40, tile = bigk[i].launch_tile & ((1LL << 40) - 1);
        // dense entries first, each part in update order
        size_t at = i;
        int64_t weight = 0, dweight = 0, dchunks = 0;
        const int lmode = launch_dense[(size_t)launch];
        // (A task of a re-cut domain holds a remainder only beside its full block -- recut_blocks -- so there it rides
        // with the block also in a launch that hands k_chol_dense everything: as an entry of its own it would be
        // multiplied as a whole block and double the task's length.)
        // (An interval domain's task holds one block per member: as a task of the tile cut.)
        const bool strips_ride = bigk[i].window != 0 && (bigk[i].window >> 32) < kIntervalDomain && lmode == 2 && B.knobs.dense_strips;
        auto dense_here = [&](const WaveEntry& E) {
            if (!is_dense(E, lmode)) return false;
            const int mi = entry_rows(E), nj = entry_cols(E);
            return !(strips_ride && ((mi <= kStripMax && nj == kBigTile) || (nj <= kStripMax && mi == kBigTile)));
        };
        if (lmode)
            for (size_t q = i; q < j; ++q) {
                const WaveEntry& E = bigk[q].e;
                if (!dense_here(E)) continue;
                S.big_entries[at++] = E;
                dchunks += ceil_div(E.K, kDenseChunk);
                dweight += ceil_div(E.K, 16) + 2;
                S.dense_flops += 2.0 * E.K * block_pairs(E.ia, entry_rows(E), E.ja, entry_cols(E));
            }
        const size_t mid = at;
        // Strips: the remainder of a source's row run right behind a full block (<= kStripMax rows x the block's 128
        // columns) or of its column run beside it (the block's 128 rows x <= kStripMax columns) rides with the block
        // -- k_chol_dense has that block's operands staged and fetches 16 rows more per chunk, where k_chol_big
        // staged the 128-wide window again for a sliver of products (Flan-class: 62 000 such entries, a third of the
        // bytes the ragged launches staged; tools/pair_stats.py).  PARSY_DENSE_STRIPS=0: never.
        int32_t nstrips = 0;
        absorbed.assign(j - i, 0);
        if (lmode && B.knobs.dense_strips && mid > i) {
            strip_of.clear();
            for (size_t d = i; d < mid; ++d) {
                const WaveEntry& E = S.big_entries[d];
                if ((E.mn & 0xffff) == (kBigTile | (kBigTile << 8))) strip_of[{E.src, ((int64_t)E.ia << 32) | (uint32_t)E.ja}] = d;
            }
            for (size_t q = i; q < j && !strip_of.empty(); ++q) {
                const WaveEntry& R = bigk[q].e;
                if (dense_here(R)) continue;
                const int mi = entry_rows(R), nj = entry_cols(R);
                const bool row_strip = mi <= kStripMax && nj == kBigTile, col_strip = nj <= kStripMax && mi == kBigTile;
                if (!row_strip && !col_strip) continue;
                const auto it = strip_of.find({R.src, ((int64_t)(R.ia - (row_strip ? kBigTile : 0)) << 32) |
                                                      (uint32_t)(R.ja - (col_strip ? kBigTile : 0))});
                if (it == strip_of.end()) continue;
                WaveEntry& E = S.big_entries[it->second];
                if (E.K != R.K || big_ident(E) != big_ident(R) || E.rel != R.rel || E.ld != R.ld) continue;
                if ((row_strip ? big_strip_rows(E) : big_strip_cols(E)) != 0) continue;
                if (big_strip_rows(E) == 0 && big_strip_cols(E) == 0) ++nstrips;
                E.mn |= row_strip ? mi << 17 : nj << 22;
                absorbed[q - i] = 1;
                S.dense_flops += 2.0 * R.K * block_pairs(R.ia, mi, R.ja, nj);
                dweight += ceil_div(R.K, 64);
            }
        }
        for (size_t q = i; q < j; ++q)
            if (!dense_here(bigk[q].e) && !absorbed[q - i]) {
                S.big_entries[at++] = bigk[q].e;
                weight += ceil_div(bigk[q].e.K, 16) + 4;
            }
        const size_t jend = at;     // (entries that ride with a dense block leave unused slots up to j)
        S.n_dense_entries += (int64_t)(mid - i);
        S.n_strip_entries += nstrips;
        while (t + 1 < nc && B.big_tile0[t + 1] <= tile) ++t;   // tiles ascend within a launch ...
        if (tile < B.big_tile0[t]) {                             // ... and start over with the next one
            t = 0;
            while (B.big_tile0[t + 1] <= tile) ++t;
        }
        const int nbr128 = ceil_div(S.csn[t].r, kBigTile);
        const int64_t local = tile - B.big_tile0[t];
        // (a re-cut domain's task: its window of the domain's index, in units of kBigTile positions)
        const int64_t window = bigk[i].window;
        const int32_t row0 = window ? (int32_t)(window & 0xffff) * kBigTile : (int32_t)(local % nbr128) * kBigTile;
        const int32_t col0 = window ? (int32_t)((window >> 16) & 0xffff) * kBigTile : (int32_t)(local / nbr128) * kBigTile;
        S.big_all.push_back(Schedule::BigTask{t, row0, col0,
                                              (int32_t)std::min<int64_t>(weight, INT32_MAX), (int64_t)i, (int64_t)jend,
                                              (int32_t)(launch >> 1), (int32_t)((launch & 1) == 0), bigk[i].sr, bigk[i].sc,
                                              (int64_t)mid, (int32_t)std::min<int64_t>(dweight, INT32_MAX),
                                              (int32_t)std::min<int64_t>(dchunks, INT32_MAX), nstrips, (int32_t)(window >> 32)});
        i = j;
    }
}

}  // namespace

void build_schedule(const PatternRef& P, const size_t* lC, const int* A2p, const int* A2i,
                    const uint8_t* active, Schedule& S, int compute_units) {
    S = Schedule();
    BuildState B;
    B.knobs = read_build_knobs();
    B.compute_units = compute_units;
    // resident workgroups of the chain kernel = 2 per CU; walkers of one batch take at most a quarter
    if (compute_units > 0) S.walker_batch = std::max(4, std::min(kWalkerBatch, compute_units / 2));
    describe_supernodes(P, lC, A2p, S);
    list_updates(P, lC, A2p, A2i, S, B);
    choose_sizes(S, B.knobs);
    cut_pieces(P, S, B);
    describe_updates(S, B);
    cut_subtrees(S, B);
    choose_super_tiles(S, B);
    build_wave_streams(S, B);
    find_conflict_domains(S, B);
    collect_big_entries(S, B);
    build_big_tasks(S, B);
    build_launches(S, active);
}


// ---- The knobs of build_launches (environment; diagnostics and tests), read by read_launch_knobs at the top of EVERY
// build_launches call: the tests change the environment between two set_active calls on one plan.
struct LaunchKnobs {
    bool force_unfused;          // PARSY_FORCE_UNFUSED=1: the solve's fallback form everywhere (per-block-column launches): the
                                 //   path taken when a chain launch would not be resident.  Used by the tests.
    int big_group;               // PARSY_BIG_GROUP (kBigGroup): edge of the super-tiles whose BIG tasks share an XCD (0: never group)
    int chain_split;             // PARSY_CHAIN_SPLIT (2 from kChainSplitAutoFlops update flops on, else 0): 0 = one chain launch per
                                 //   level, 1 = two for the pieces of split supernodes, 2 = two for every tiled supernode
    int bsolve_below;            // PARSY_BSOLVE_BELOW (1): 0 = never split the rows below off, 2 = for every wide supernode with rows below
    bool sub_tier_min_trees_set; // PARSY_SUB_TIER_MIN_TREES (kSubTierMinTrees): trees a band of levels must leave (0: no bands).
    int sub_tier_min_trees;      //   Set: bands whatever the density of the factor (tests)
    int solve_one;               // PARSY_SOLVE_ONE (1): 0 = never a ONE-launch solve, 1 = by size, 2 = whatever the size (tests)
};

static LaunchKnobs read_launch_knobs(const Schedule& S) {
    LaunchKnobs K{};
    const char* fu = std::getenv("PARSY_FORCE_UNFUSED");
    K.force_unfused = fu && fu[0] == '1';
    K.big_group = env_int("PARSY_BIG_GROUP", kBigGroup);
    K.chain_split = env_int("PARSY_CHAIN_SPLIT", S.update_flops >= kChainSplitAutoFlops ? 2 : 0);
    K.bsolve_below = env_int("PARSY_BSOLVE_BELOW", 1);
    K.sub_tier_min_trees_set = std::getenv("PARSY_SUB_TIER_MIN_TREES") != nullptr;
    K.sub_tier_min_trees = env_int("PARSY_SUB_TIER_MIN_TREES", kSubTierMinTrees);
    K.solve_one = env_int("PARSY_SOLVE_ONE", 1);
    return K;
}

static void build_solve_one(Schedule& S, const LaunchKnobs& K, bool sharded);

// The lists of the solves' subtree launches for many right-hand sides (schedule.hpp: SubMember, SubTree, SubTier).
// append_sub_tier lays out one tier from its trees (supernodes in index order: descendants first).  A row below a member
// that is a column of a member of the same tree maps to that column's slot, any other row to the tree's list of outside
// rows (for a whole subtree: the rows below its root).
// Column slots are a STACK: a member's columns start where its parent's end (the root's at 0), so the slots in use at
// any time are those of a path to the root -- the members are walked in postorder, and everything a walk has pending
// (forward: sums for members not yet solved; backward: x of the members already solved that a later one reads) belongs
// to the ancestors of the member in hand.  Siblings share slot numbers; the forward kernel hands a slot back as zero
// when it reads it.  Both walks are replayed here and the tier is not made if a slot would be shared at the same time.
static bool append_sub_tier(Schedule& S, const std::vector<std::vector<int32_t>>& trees, int top_level, int max_slots) {
    const size_t members0 = S.sub_members.size(), trees0 = S.sub_trees.size(), slots0 = S.sub_slots.size(),
                 outs0 = S.sub_out_rows.size();
    auto drop = [&] {
        S.sub_members.resize(members0);
        S.sub_trees.resize(trees0);
        S.sub_slots.resize(slots0);
        S.sub_out_rows.resize(outs0);
        return false;
    };
    if (trees.empty()) return false;
    std::vector<int32_t> col_slot((size_t)S.n, -1);   // per column: its slot in the tree being laid out
    std::vector<int32_t> out_slot((size_t)S.n, -1);   // per row: its outside slot, likewise
    std::vector<int32_t> root_slot((size_t)S.nsuper, -1);  // per supernode of the tree: slot of its first column
    std::vector<int32_t> owner;                       // replay: the column a slot belongs to (-1: free)
    SubTier tier{(int32_t)trees0, 0, 0, top_level};
    for (const std::vector<int32_t>& tree : trees) {
        SubTree T{};
        T.m0 = (int32_t)S.sub_members.size();
        T.out0 = (int32_t)S.sub_out_rows.size();
        // slots: parents before children
        for (size_t q = tree.size(); q-- > 0;) {
            const int32_t t = tree[q];
            const SnDesc& D = S.sn[t];
            const int p = S.sparent[(size_t)t];
            const int32_t off = (p >= 0 && root_slot[(size_t)p] >= 0) ? root_slot[(size_t)p] + S.sn[p].w : 0;
            root_slot[(size_t)t] = off;
            for (int c = 0; c < D.w; ++c) col_slot[(size_t)D.c0 + c] = off + c;
            T.ncols = std::max(T.ncols, off + D.w);
        }
        // outside rows in ascending order
        std::vector<int32_t> outs;
        for (int32_t t : tree) {
            const SnDesc& D = S.sn[t];
            for (int k = D.w; k < D.r; ++k) {
                const int32_t row = S.rows[(size_t)D.pi + k];
                if (col_slot[(size_t)row] < 0 && out_slot[(size_t)row] < 0) {
                    out_slot[(size_t)row] = 0;
                    outs.push_back(row);
                }
            }
        }
        std::sort(outs.begin(), outs.end());
        T.nout = (int32_t)outs.size();
        for (int32_t j = 0; j < T.nout; ++j) out_slot[(size_t)outs[(size_t)j]] = T.ncols + j;
        S.sub_out_rows.insert(S.sub_out_rows.end(), outs.begin(), outs.end());
        const int32_t trash = T.ncols + T.nout;
        bool ok = trash + 1 <= max_slots && trash + 1 <= 65535;
        // members: a supernode's 16-column blocks from left to right (row k of block j = row 16 j + k of the panel)
        auto row_id = [&](const SnDesc& D, int k) { return k < D.w ? D.c0 + k : S.rows[(size_t)D.pi + k]; };
        auto slot_of = [&](int32_t row) { return col_slot[(size_t)row] >= 0 ? col_slot[(size_t)row] : out_slot[(size_t)row]; };
        for (size_t q = 0; q < tree.size() && ok; ++q) {
            const SnDesc& D = S.sn[tree[q]];
            for (int j0 = 0; j0 < D.w; j0 += kTinyWidth) {
                const int wb = std::min(kTinyWidth, D.w - j0);
                SubMember M{D.px + (int64_t)j0 * D.r + j0, D.c0 + j0, wb, D.r - j0, root_slot[(size_t)tree[q]] + j0,
                            (int32_t)(S.sub_slots.size() / 16), D.r};
                for (int k0 = wb; k0 < M.r; k0 += 16)
                    for (int kq = 0; kq < 4; ++kq)
                        for (int v = 0; v < 4; ++v) {
                            const int k = k0 + 4 * v + kq;
                            S.sub_slots.push_back((uint16_t)(k < M.r ? slot_of(row_id(D, j0 + k)) : trash));
                        }
                S.sub_members.push_back(M);
            }
        }
        T.m1 = (int32_t)S.sub_members.size();
        // replay of the forward walk: a column slot is taken by the first sum that goes to it and freed when its member
        // is solved; of the backward walk: written when its member is solved, read by the members after it
        owner.assign((size_t)T.ncols, -1);
        for (size_t q = 0; q < tree.size() && ok; ++q) {
            const SnDesc& D = S.sn[tree[q]];
            for (int c = 0; c < D.w && ok; ++c) {
                int32_t& o = owner[(size_t)col_slot[(size_t)D.c0 + c]];
                ok = o < 0 || o == D.c0 + c;
                o = -1;
            }
            for (int k = D.w; k < D.r && ok; ++k) {
                const int32_t row = S.rows[(size_t)D.pi + k];
                if (col_slot[(size_t)row] < 0) continue;
                int32_t& o = owner[(size_t)col_slot[(size_t)row]];
                ok = o < 0 || o == row;
                o = row;
            }
        }
        for (int32_t o : owner) ok = ok && o < 0;   // (every sum was consumed: its column's member came later)
        owner.assign((size_t)T.ncols, -1);
        for (size_t q = tree.size(); q-- > 0 && ok;) {
            const SnDesc& D = S.sn[tree[q]];
            for (int k = D.w; k < D.r && ok; ++k) {
                const int32_t row = S.rows[(size_t)D.pi + k];
                if (col_slot[(size_t)row] >= 0) ok = owner[(size_t)col_slot[(size_t)row]] == row;
            }
            for (int c = 0; c < D.w; ++c) owner[(size_t)col_slot[(size_t)D.c0 + c]] = D.c0 + c;
        }
        for (int32_t t : tree) {
            const SnDesc& D = S.sn[t];
            for (int c = 0; c < D.w; ++c) col_slot[(size_t)D.c0 + c] = -1;
            root_slot[(size_t)t] = -1;
        }
        for (int32_t row : outs) out_slot[(size_t)row] = -1;
        if (!ok) return drop();
        tier.max_slots = std::max(tier.max_slots, trash + 1);
        S.sub_trees.push_back(T);
    }
    tier.ntrees = (int32_t)(S.sub_trees.size() - trees0);
    S.sub_tiers.push_back(tier);
    S.sub_max_slots = std::max(S.sub_max_slots, tier.max_slots);
    return true;
}

// Tier 0: the subtrees of the forward solve's subtree launch as solve_small_list / solve_small_ranges lay them out.
// Tiers above: bands of levels whose active supernodes are all at most kSubTierMaxWidth wide, every supernode not yet in a
// tier in the tree of its highest ancestor inside the band; a band grows while that leaves at least kSubTierMinTrees
// trees (PARSY_SUB_TIER_MIN_TREES; 0: no bands) whose slots fit.
// Reads the forward solve's subtree launch (solve_small_list / _ranges), S.active, the etree levels.  Fills sub_members,
// sub_trees, sub_slots, sub_out_rows, sub_tiers, sub_max_slots, sub_cover_level (all empty / reset when it is called).
static void build_sub_tiers(Schedule& S, const LaunchKnobs& K) {
    const int ns = S.nsuper;
    std::vector<uint8_t> covered((size_t)ns, 0);
    {
        std::vector<std::vector<int32_t>> trees(S.solve_small_ranges.size() / 2);
        for (size_t b = 0; b < trees.size(); ++b)
            trees[b].assign(S.solve_small_list.begin() + S.solve_small_ranges[2 * b],
                            S.solve_small_list.begin() + S.solve_small_ranges[2 * b + 1]);
        if (trees.empty() || !append_sub_tier(S, trees, -1, kSubMaxSlots + 1)) return;
        for (const auto& tr : trees)
            for (int32_t t : tr) covered[(size_t)t] = 1;
    }
    const int min_trees = K.sub_tier_min_trees;
    if (min_trees <= 0) return;
    // Bands pay where the level launches they replace are chains of latencies -- factors of few entries per row (2-D
    // problems: parabolic_fem-class, 67 entries per row: levels 3-6 of 64 right-hand sides 307 -> 133 us forward).  The
    // trees of a 3-D factor carry hundreds of outside rows each (Flan-class: 442 slots = 63 KB of LDS per wave, two waves
    // per compute unit: 4.4 ms for what the level kernels do in 2.1), so there only the subtrees keep this form (3.7 ->
    // 2.1 ms).  PARSY_SUB_TIER_MIN_TREES set: whatever the factor (tests).
    if (!K.sub_tier_min_trees_set && S.xsize >= (int64_t)kSubTierMaxDensity * S.n) return;
    std::vector<int> level((size_t)ns, 0);
    for (int l = 0; l < S.nlevels; ++l)
        for (int q = S.levelPtr[l]; q < S.levelPtr[l + 1]; ++q) level[(size_t)S.levelSet[q]] = l;
    // bands may reach up to the level below the first one with a wide (or, shards: with an inactive) supernode
    int lmax = S.nlevels - 1;
    for (int t = 0; t < ns; ++t)
        if (!covered[(size_t)t] && (S.sn[t].w > kSubTierMaxWidth || !S.active[t])) lmax = std::min(lmax, level[(size_t)t] - 1);
    // (a band must also cover every level below it completely: nothing uncovered may lie under a tier-0 subtree's level)
    auto trees_of_band = [&](int top, std::vector<std::vector<int32_t>>& trees) {
        std::vector<int32_t> root_of((size_t)ns, -1), tree_of((size_t)ns, -1);
        trees.clear();
        for (int t = ns - 1; t >= 0; --t) {   // parents first
            if (covered[(size_t)t] || level[(size_t)t] > top) continue;
            const int p = S.sparent[(size_t)t];
            if (p >= 0 && tree_of[(size_t)p] >= 0) tree_of[(size_t)t] = tree_of[(size_t)p];
            else {
                tree_of[(size_t)t] = (int32_t)trees.size();
                trees.emplace_back();
            }
        }
        for (int t = 0; t < ns; ++t)
            if (tree_of[(size_t)t] >= 0) trees[(size_t)tree_of[(size_t)t]].push_back(t);
    };
    int next = 0;   // lowest level with an uncovered supernode
    while (true) {
        next = S.nlevels;
        for (int t = 0; t < ns; ++t)
            if (!covered[(size_t)t]) next = std::min(next, level[(size_t)t]);
        if (next > lmax) break;
        // the highest top with enough trees
        // (where not even one level leaves min_trees trees -- the narrow levels right below the wide supernodes -- a last
        // band of at least a quarter as many: parabolic_fem-class, levels 7-8 as 128 trees)
        std::vector<std::vector<int32_t>> trees, best;
        int best_top = -1;
        // (the HIGHEST top that leaves enough trees: a handful of stragglers on the lowest uncovered level -- wider supernodes
        // among the leaves -- are few trees by themselves and many once the level above joins them)
        for (int need : {min_trees, std::max(min_trees / 4, 1)}) {
            for (int top = next; top <= lmax; ++top) {
                trees_of_band(top, trees);
                if ((int)trees.size() < need) continue;
                best.swap(trees);
                best_top = top;
            }
            if (best_top >= 0) break;
        }
        if (best_top < 0) break;
        // heaviest trees first
        std::vector<double> cost(best.size(), 0.0);
        for (size_t b = 0; b < best.size(); ++b)
            for (int32_t t : best[b]) cost[b] += 2e3 + (double)S.sn[t].w * S.sn[t].r;
        std::vector<size_t> order(best.size());
        for (size_t b = 0; b < order.size(); ++b) order[b] = b;
        std::stable_sort(order.begin(), order.end(), [&](size_t a, size_t b) { return cost[a] > cost[b]; });
        std::vector<std::vector<int32_t>> sorted(best.size());
        for (size_t b = 0; b < order.size(); ++b) sorted[b].swap(best[order[b]]);
        bool ok = append_sub_tier(S, sorted, best_top, kSubTierMaxSlots + 1);
        while (!ok && best_top > next) {   // (slots: a lower band)
            --best_top;
            trees_of_band(best_top, sorted);
            ok = append_sub_tier(S, sorted, best_top, kSubTierMaxSlots + 1);
        }
        if (!ok) break;
        for (const auto& tr : sorted)
            for (int32_t t : tr) covered[(size_t)t] = 1;
        S.sub_cover_level = best_top;
    }
}

// The makers of the launch records: each takes what its kind and form have, every other field keeps its default.
// (`count`, and what a launch takes from its members -- lds_bytes, stage, width, task_count --, is filled in by name
// while build_launches appends the launch's descriptors.)
static Launch main_launch(int32_t kind, int32_t first, int32_t level) {
    Launch L{kind};
    L.first = first;
    L.level = level;
    return L;
}
// TILES and the BIG / DENSE launches of a PUSH: on the side stream once `wait_level` is complete; the main-stream
// launches of `level` wait for it
static Launch side_launch(int32_t kind, int32_t first, int32_t level, int32_t wait_level) {
    Launch L = main_launch(kind, first, level);
    L.side = 1;
    L.wait_level = wait_level;
    return L;
}
static Launch small_launch(int32_t first, int32_t level) { return main_launch(kLaunchSmall, first, level); }
static Launch subtrees_launch(int32_t kind) {   // SMALL, SOLVE_SMALL, BACK_BLOCK: the pairs [0, count) of the kind's range array
    Launch L = main_launch(kind, 0, 0);
    L.form = kFormSubtrees;
    return L;
}
static Launch chain_launch(int32_t first, int32_t level, int32_t ticket, bool rows_only) {
    Launch L = main_launch(kLaunchChain, first, level);
    L.ticket = ticket;
    L.rows_only = rows_only;
    return L;
}
static Launch solve_small_launch(int32_t first, int32_t count, int32_t level) {
    Launch L = main_launch(kLaunchSolveSmall, first, level);
    L.count = count;
    return L;
}
// chain form of SOLVE_PANEL / BACK_BLOCK: a ticket counter and a task range (solve_mtasks / bsolve_pairs) from task_first on
static Launch level_chain_launch(int32_t kind, int32_t first, int32_t level, int32_t ticket, int32_t task_first) {
    Launch L = main_launch(kind, first, level);
    L.form = kFormChain;
    L.ticket = ticket;
    L.task_first = task_first;
    return L;
}
static Launch fixup_launch(int32_t count, int32_t level) {
    Launch L = main_launch(kLaunchSolveFixup, 0, level);
    L.count = count;
    return L;
}
static Launch back_block_launch(int32_t first, int32_t count, int32_t level, int32_t width_class) {
    Launch L = main_launch(kLaunchBackBlock, first, level);
    L.count = count;
    L.width_class = width_class;
    return L;
}

namespace {

using BigTaskList = std::vector<const Schedule::BigTask*>;

// What the passes of build_launches hand to each other and is not part of the Schedule.
struct LaunchState {
    LaunchKnobs knobs;
    std::vector<Launch> early;             // the side-stream launches, spliced into S.chol when every level is there
    std::vector<size_t> level_begin;       // index in S.chol where each level's main-stream launches start
    std::vector<BigTaskList> big_next, big_push;   // BIG tasks of every (source level, kind), active targets only
};

// Everything build_launches fills, empty again: the lists and counters of the three launch sequences.
void reset_launch_lists(Schedule& S) {
    S.n_chain_launches = 0;
    S.n_solve_chain_launches = 0;
    S.n_solve_wide = 0;
    S.n_bpart_slots = 0;
    S.small_list.clear();
    S.small_ranges.clear();
    S.tiles.clear();
    S.big_tasks.clear();
    S.chol.clear();
    S.solve_small_list.clear();
    S.solve_small_ranges.clear();
    S.solve_panels.clear();
    S.solve_mtasks.clear();
    S.solve_fix_list.clear();
    S.solve_wide_list.clear();
    S.solve.clear();
    S.sub_members.clear();
    S.sub_trees.clear();
    S.sub_slots.clear();
    S.sub_out_rows.clear();
    S.sub_tiers.clear();
    S.sub_max_slots = 0;
    S.sub_cover_level = -1;
    S.bsolve_blocks.clear();
    S.bsolve_pairs.clear();
    S.bsolve_below.clear();
    S.bsolve_ranges.clear();
    S.bsolve.clear();
}

// Reads the masks.  Fills S.active, S.active_piece, and solve_subtree / bsolve_subtree: the subtrees the mask contains whole.
void apply_masks(Schedule& S, const uint8_t* active, const uint8_t* active_pieces) {
    const int ns = S.nsuper;
    S.active.assign(ns, 1);
    if (active) S.active.assign(active, active + ns);
    // the factorization goes by PIECES of the Cholesky view (a multi-device run deals the pieces of a split
    // supernode to different devices); without a piece mask a piece is active with its supernode
    const int npieces = (int)S.csn.size();
    S.active_piece.assign((size_t)npieces, 1);
    for (int t = 0; t < npieces; ++t)
        S.active_piece[t] = active_pieces ? (active_pieces[t] != 0) : S.active[S.csn_real[t]];
    // A subtree launch of the solves walks its subtree without waiting for anything outside it.  Under a supernode mask
    // (a rank's share) that holds only for the subtrees the mask contains whole: the active members of the others go to
    // the level launches, which a solve in steps of levels (plan_solve_levels) separates by its exchange steps.
    if (S.solve_subtree_all.empty()) {
        S.solve_subtree_all = S.solve_subtree;
        S.bsolve_subtree_all = S.bsolve_subtree;
    }
    S.solve_subtree = S.solve_subtree_all;
    S.bsolve_subtree = S.bsolve_subtree_all;
    if (active)
        for (auto* sub : {&S.solve_subtree, &S.bsolve_subtree}) {
            const int count = sub == &S.solve_subtree ? S.n_solve_subtrees : S.n_bsolve_subtrees;
            std::vector<uint8_t> whole((size_t)std::max(count, 0), 1);
            for (int t = 0; t < ns; ++t)
                if ((*sub)[t] >= 0 && !S.active[t]) whole[(size_t)(*sub)[t]] = 0;
            for (int t = 0; t < ns; ++t)
                if ((*sub)[t] >= 0 && !whole[(size_t)(*sub)[t]]) (*sub)[t] = -1;
        }
}

// Order of a BIG launch's tasks: appends the tasks of `all` that have a dense part (dense: for k_chol_dense -- TileDesc::part
// = its 8-wide k chunks --), else those that have a ragged rest, to S.big_tasks; returns L with first / count filled in.
// Workgroups are dealt round-robin over the 8 XCDs (block b runs on the
// XCD of every block b + 8k; observed placement, used for speed only) and each XCD has its own L2, so
// tiles that read the same rows of a source should share an XCD at the same time: the tasks are grouped
// into g x g super-tiles of one target's tile grid (g row windows + g column windows of the source feed
// g*g tasks), the groups are dealt to 8 sequences -- heaviest group first, each to the least loaded
// sequence -- and sequence x fills the positions 8s + x (shorter sequences are padded with empty tasks,
// which return at once).  Small launches keep the plain heaviest-first order.  PARSY_BIG_GROUP=g
// (0: never group).
Launch emit_big(Schedule& S, int big_group, const BigTaskList& all, Launch L, bool dense) {
    BigTaskList v;
    for (const Schedule::BigTask* b : all)
        if (dense ? b->em > b->e0 : b->e1 > b->em) v.push_back(b);
    if (v.empty()) return L;
    L.first = (int32_t)S.big_tasks.size();
    auto wt = [dense](const Schedule::BigTask* b) { return dense ? b->dweight : b->weight; };
    auto desc = [dense](const Schedule::BigTask* b) {
        return dense ? TileDesc{b->sn, b->row0, b->col0, b->dchunks | (b->strips > 0 ? kDenseStripTask : 0), b->e0, b->em}
                     : TileDesc{b->sn, b->row0, b->col0, 0, b->em, b->e1};
    };
    auto by_weight = [&](const Schedule::BigTask* a, const Schedule::BigTask* b) { return wt(a) > wt(b); };
    // group edge: as large as leaves every XCD at least kBigGroupsPerXcd groups to balance with
    int g = big_group;
    // (a group of g x g tiles holds g * g / (sr * sc) tasks)
    const int per_task = v[0]->sr * v[0]->sc;
    while (g > 1 && (int64_t)v.size() * per_task < (int64_t)8 * kBigGroupsPerXcd * g * g) g /= 2;
    if (g < std::max(v[0]->sr, v[0]->sc)) g = 1;
    if (g <= 1) {
        std::stable_sort(v.begin(), v.end(), by_weight);
        for (const Schedule::BigTask* b : v) S.big_tasks.push_back(desc(b));
        L.count = (int32_t)v.size();
        return L;
    }
    struct Group { std::pair<int64_t, int64_t> key; int64_t weight; int32_t maxw; BigTaskList tasks; };
    BigTaskList seq[8];
    int64_t load[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    auto least = [&] {
        int x = 0;
        for (int q = 1; q < 8; ++q)
            if (load[q] < load[x]) x = q;
        return x;
    };
    // the bulk goes in g x g groups; the lightest kBigTailGroups groups are dealt again at half the edge
    // (and so on down to single tasks), so that the sequences end together
    BigTaskList rest(v);
    for (; !rest.empty(); g /= 2) {
        if (g <= 1) {
            std::stable_sort(rest.begin(), rest.end(), by_weight);
            for (const Schedule::BigTask* b : rest) {
                const int x = least();
                seq[x].push_back(b);
                load[x] += wt(b);
            }
            break;
        }
        using GroupKey = std::pair<int64_t, int64_t>;   // (piece, domain), window group
        std::vector<std::pair<GroupKey, const Schedule::BigTask*>> keyed;
        keyed.reserve(rest.size());
        for (const Schedule::BigTask* b : rest) {
            const int64_t gi = b->row0 / (kBigTile * g), gj = b->col0 / (kBigTile * g);
            keyed.push_back({GroupKey{((int64_t)b->sn << 32) | b->domain, (gj << 32) | gi}, b});
        }
        std::stable_sort(keyed.begin(), keyed.end(), [](const auto& a, const auto& b) { return a.first < b.first; });
        std::vector<Group> groups;
        for (const auto& kb : keyed) {
            if (groups.empty() || groups.back().key != kb.first) groups.push_back(Group{kb.first, 0, 0, {}});
            Group& G = groups.back();
            G.tasks.push_back(kb.second);
            G.weight += wt(kb.second);
            G.maxw = std::max(G.maxw, wt(kb.second));
        }
        std::stable_sort(groups.begin(), groups.end(), [](const Group& a, const Group& b) {
            return a.maxw != b.maxw ? a.maxw > b.maxw : a.weight > b.weight;
        });
        const size_t bulk = groups.size() > (size_t)kBigTailGroups ? groups.size() - kBigTailGroups : 0;
        rest.clear();
        for (size_t q = 0; q < groups.size(); ++q) {
            Group& G = groups[q];
            if (q >= bulk) {
                rest.insert(rest.end(), G.tasks.begin(), G.tasks.end());
                continue;
            }
            const int x = least();
            std::stable_sort(G.tasks.begin(), G.tasks.end(), by_weight);
            seq[x].insert(seq[x].end(), G.tasks.begin(), G.tasks.end());
            load[x] += G.weight;
        }
    }
    size_t len = 0;
    for (int x = 0; x < 8; ++x) len = std::max(len, seq[x].size());
    for (size_t s = 0; s < len; ++s)
        for (int x = 0; x < 8; ++x) {
            if (s < seq[x].size()) {
                S.big_tasks.push_back(desc(seq[x][s]));
            } else {
                S.big_tasks.push_back(TileDesc{0, 0, 0, 0, 0, 0});  // padding: no entries
            }
        }
    L.count = (int32_t)(8 * len);
    return L;
}

// The active supernodes of every subtree in index order (descendants first), subtrees by falling cost:
// append(supernode) appends to the kind's list, position() is the list's length; fills the (begin, end) pairs of the list
// positions into `ranges` and returns the number of subtrees that have an active member.
template <class Position, class Append>
int32_t subtree_ranges(const Schedule& S, const std::vector<int32_t>& subtree, int count, const std::vector<double>& cost,
                       Position&& position, Append&& append, std::vector<int32_t>& ranges, bool chol = false) {
    std::vector<std::vector<int32_t>> members((size_t)count);
    std::vector<double> total((size_t)count, 0.0);
    for (int t = 0; t < S.nsuper; ++t)
        if (subtree[t] >= 0 && (chol ? S.active_piece[S.piece0[t]] : S.active[t])) {
            members[(size_t)subtree[t]].push_back(t);
            total[(size_t)subtree[t]] += cost[t];
        }
    std::vector<int32_t> order;
    for (int k = 0; k < count; ++k)
        if (!members[(size_t)k].empty()) order.push_back(k);
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return total[(size_t)a] > total[(size_t)b]; });
    for (int k : order) {
        ranges.push_back(position());
        for (int32_t t : members[(size_t)k]) append(t);
        ranges.push_back(position());
    }
    return (int32_t)order.size();
}

// SMALL: piece t joins launch L -- dynamic LDS for the largest panel, and the stage size: the largest descendant block,
// capped (kernel: kSmallStage = 2048 doubles)
void add_small(Schedule& S, int t, Launch& L) {
    const SnDesc& T = S.csn[t];
    S.small_list.push_back(t);
    L.lds_bytes = std::max<int32_t>(L.lds_bytes, T.w * T.r * (int)sizeof(double));
    for (int64_t u = T.upd0; u < T.upd0 + T.nupd; ++u)
        L.stage = std::max<int32_t>(L.stage, std::min<int64_t>((int64_t)S.upd[u].m * S.upd[u].K, 2048));
}

// SMALL launches of level lev (in front of level 0: the subtrees of SMALL supernodes, one workgroup each).  Fills small_list,
// small_ranges, S.chol; returns the level's tiled pieces in `tiled`.
void small_launches(Schedule& S, int lev, std::vector<int>& tiled) {
    tiled.clear();
    if (lev == 0 && S.n_chol_subtrees > 0) {
        Launch L = subtrees_launch(kLaunchSmall);
        L.count = subtree_ranges(
            S, S.chol_subtree, S.n_chol_subtrees, S.chol_cost, [&] { return (int32_t)S.small_list.size(); },
            [&](int32_t t) { add_small(S, S.piece0[t], L); }, S.small_ranges, true);
        if (L.count > 0) S.chol.push_back(L);
    }
    Launch L = small_launch((int32_t)S.small_list.size(), lev);
    for (int q = S.clevelPtr[lev]; q < S.clevelPtr[lev + 1]; ++q) {
        const int t = S.clevelSet[q];
        if (!S.active_piece[t] || S.chol_subtree[S.csn_real[t]] >= 0) continue;
        if (is_small(S.csn[t])) add_small(S, t, L);
        else tiled.push_back(t);
    }
    L.count = (int32_t)S.small_list.size() - L.first;
    if (L.count > 0) S.chol.push_back(L);
}

// PUSH(lev): this level's wide supernodes update everything at least two levels up (side
// stream, once the level is complete); NEXT(lev - 1): the level below updates this level's tiles.
// Side-stream launches -- TILES(lev): the early wave streams of level lev's tiles, PUSH(s): the BIG
// updates from level s's supernodes into targets at levels >= s + 2 -- are enqueued right before the
// main-stream launches of the level in between (lev - 1 = s + 1), so that they run while the main
// stream works through that level's chain; Launch::level = lev = s + 2 is the level whose main-stream
// launches wait for them.
void push_next_launches(Schedule& S, LaunchState& LS, int lev) {
    const int g = LS.knobs.big_group;
    if (lev + 2 < S.cnlevels) {
        Launch Ld = emit_big(S, g, LS.big_push[lev], side_launch(kLaunchDense, 0, lev + 2, lev), true);
        if (Ld.count > 0) LS.early.push_back(Ld);
        Launch Lp = emit_big(S, g, LS.big_push[lev], side_launch(kLaunchBig, 0, lev + 2, lev), false);
        if (Lp.count > 0) LS.early.push_back(Lp);
    }
    if (lev > 0) {
        Launch Ld = emit_big(S, g, LS.big_next[lev - 1], main_launch(kLaunchDense, 0, lev), true);
        if (Ld.count > 0) S.chol.push_back(Ld);
        Launch Ln = emit_big(S, g, LS.big_next[lev - 1], main_launch(kLaunchBig, 0, lev), false);
        if (Ln.count > 0) S.chol.push_back(Ln);
    }
}

// TILES: the early part of the external updates of level lev's tiled pieces, longest streams first (side stream)
void tiles_launch(Schedule& S, LaunchState& LS, int lev, const std::vector<int>& tiled) {
    Launch Lt = side_launch(kLaunchTiles, (int32_t)S.tiles.size(), lev, lev - 2);
    std::vector<std::pair<int32_t, TileDesc>> wt;  // (weight, tile)
    for (int t : tiled) {
        const SnDesc& T = S.csn[t];
        const int nbc = ceil_div(T.w, kTile), nbr = ceil_div(T.r, kTile);
        const int32_t* tw = &S.tile_w[S.sn_tw0[t]];
        for (int J = 0; J < nbc; ++J)
            for (int I = J; I < nbr; ++I) {
                const int32_t wgt = tw[((size_t)J * nbr + I) * 2];
                if (wgt <= 0) continue;
                const int64_t si = S.tile_split[S.sn_tw0[t] / 2 + (size_t)J * nbr + I];
                if (si < 0) {
                    wt.push_back({wgt, TileDesc{t, I * kTile, J * kTile, 0,
                                                S.sn_wp0[t] + (((int64_t)J * nbr + I) * 2) * 4, -1}});
                } else {
                    const Schedule::SplitDesc& sd = S.split_desc[(size_t)si];
                    for (int part = 0; part < sd.nparts; ++part)
                        wt.push_back({ceil_div(wgt, sd.nparts),
                                      TileDesc{t, I * kTile, J * kTile, part | (sd.nparts << 8),
                                               sd.ranges + part * 8, sd.sp}});
                }
            }
    }
    std::stable_sort(wt.begin(), wt.end(),
                     [](const auto& a, const auto& b) { return a.first > b.first; });
    for (auto& x : wt) S.tiles.push_back(x.second);
    Lt.count = (int32_t)S.tiles.size() - Lt.first;
    if (Lt.count > 0) LS.early.push_back(Lt);
}

// CHAIN: every tile of the level's tiled supernodes, producers before consumers.
// Group J of a supernode: the walker (J = 0 only: it owns every diagonal tile), the two tiles
// the walker needs prepared for its step J -- (J+1,J) and (J+1,J+1) -- and then the other
// tiles of block column J, which wait for diagonal tile J.
// On large jobs the chain takes two launches per level: the tiles of the diagonal squares with the walkers
// first, the tiles of the rows below the squares afterwards.  In one launch those tiles -- hundreds to
// thousands per piece of a top separator -- were dispatched long before the walker reached their block
// column and waited for it holding a workgroup slot (72 KB of LDS: one of the two k_chol_big workgroups of
// the PUSH launch that runs beside the chain cannot be resident on that compute unit meanwhile); in a launch
// of their own every diagonal tile is there when they start, no flag is waited for, and the kernel of the
// second launch (k_chol_chain_rows: no walker, no prepared tile) gets by with 52 KB of LDS: three workgroups
// per compute unit.  Flan-class input: 371.2 -> 365.8 ms with the same kernel for both launches, 347.6 ms
// with k_chol_chain_rows; 27-point grids 56^3 ... 80^3: -3 ... -6 %; 48^3: +-0, 40^3: +9 %, nd24k-class
// 3.92 -> 4.21 ms (small jobs without BIG launches: the chain is the critical path), so the split is taken
// from kChainSplitAutoFlops update flops on.  Splitting only the pieces of split supernodes loses everywhere
// (mode 1).  PARSY_CHAIN_SPLIT=0: never; 2: always (diagnostics).
void chain_launches(Schedule& S, int chain_split_mode, int lev, const std::vector<int>& tiled) {
    auto splits = [&S, chain_split_mode](int t) {
        const int real = S.csn_real[t];
        return chain_split_mode == 2 || (chain_split_mode == 1 && S.piece0[real + 1] - S.piece0[real] > 1);
    };
    bool chain_split = false;
    for (int t : tiled) chain_split = chain_split || splits(t);
    for (int part = 0; part < (chain_split ? 2 : 1); ++part) {
        // part 1: only tiles below the squares (k_chol_chain_rows: three workgroups per compute unit)
        Launch Lc = chain_launch((int32_t)S.tiles.size(), lev, S.n_chain_launches++, part == 1);
        // Walkers stay resident for their whole chain, so the block-column-major interleaving is
        // done per batch of at most walker_batch supernodes: what a walker waits for then lies at most
        // one batch of tiles ahead of it in ticket order, and the walkers of the batches in flight
        // never take more than a fraction of the resident workgroups.
        for (size_t b0 = 0; b0 < tiled.size(); b0 += (size_t)S.walker_batch) {
            const size_t b1 = std::min(tiled.size(), b0 + (size_t)S.walker_batch);
            int maxnb = 0;
            for (size_t q = b0; q < b1; ++q) maxnb = std::max(maxnb, ceil_div(S.csn[tiled[q]].w, kTile));
            for (int J = 0; J < maxnb; ++J)
                for (size_t q = b0; q < b1; ++q) {
                    const int t = tiled[q];
                    const SnDesc& T = S.csn[t];
                    const int nbc = ceil_div(T.w, kTile), nbr = ceil_div(T.r, kTile);
                    if (J >= nbc) continue;
                    auto push = [&](int I, int Jc) {
                        if (chain_split && ((I < nbc || !splits(t)) != (part == 0))) return;   // square / rows below it
                        const int64_t si = S.tile_split[S.sn_tw0[t] / 2 + (size_t)Jc * nbr + I];
                        S.tiles.push_back(TileDesc{t, I * kTile, Jc * kTile,
                                                   si < 0 ? 0 : S.split_desc[(size_t)si].nparts,
                                                   S.sn_wp0[t] + (((int64_t)Jc * nbr + I) * 2 + 1) * 4,
                                                   si < 0 ? -1 : S.split_desc[(size_t)si].sp});
                    };
                    if (J == 0) push(0, 0);
                    const bool next_diag = J + 1 < nbc;
                    if (next_diag) {
                        push(J + 1, J);
                        push(J + 1, J + 1);
                    }
                    for (int I = next_diag ? J + 2 : J + 1; I < nbr; ++I) push(I, J);
                }
        }
        Lc.count = (int32_t)S.tiles.size() - Lc.first;
        if (Lc.count > 0) S.chol.push_back(Lc);
        else --S.n_chain_launches;
    }
}

// Splices the side launches (LS.early) into S.chol in front of the level before the one that waits for them (stable: PUSH
// before TILES of the same level).  Fills
// chol_level_begin[lev]: where level lev's launches start in S.chol (its side launches first) -- the steps
// of a factorization that is run level by level (parsy_factor_level)
void splice_side_launches(Schedule& S, LaunchState& LS) {
    S.chol_level_begin.assign(LS.level_begin.begin(), LS.level_begin.end());
    if (!LS.early.empty()) {
        std::vector<Launch> merged;
        size_t e = 0;
        std::stable_sort(LS.early.begin(), LS.early.end(), [](const Launch& a, const Launch& b) { return a.level < b.level; });
        for (int lev = 0; lev < S.cnlevels; ++lev) {
            S.chol_level_begin[(size_t)lev] = merged.size();
            while (e < LS.early.size() && LS.early[e].level - 1 <= lev) merged.push_back(LS.early[e++]);
            const size_t b0 = LS.level_begin[lev], b1 = lev + 1 < S.cnlevels ? LS.level_begin[lev + 1] : S.chol.size();
            merged.insert(merged.end(), S.chol.begin() + b0, S.chol.begin() + b1);
        }
        S.chol.swap(merged);
    }
    S.chol_level_begin.push_back(S.chol.size());
}

// The launches of the factorization, level by level of the Cholesky view.  Fills small_list / small_ranges, tiles, big_tasks,
// S.chol, chol_level_begin, n_chain_launches.
void cholesky_launches(Schedule& S, LaunchState& LS) {
    // BIG tasks of every (source level, kind), active targets only, heaviest first
    LS.big_next.assign((size_t)S.cnlevels, {});
    LS.big_push.assign((size_t)S.cnlevels, {});
    for (const Schedule::BigTask& b : S.big_all)
        if (S.active_piece[b.sn]) (b.next ? LS.big_next : LS.big_push)[b.src_level].push_back(&b);
    std::vector<int> tiled;
    for (int lev = 0; lev < S.cnlevels && !S.solve_only; ++lev) {
        LS.level_begin.push_back(S.chol.size());
        small_launches(S, lev, tiled);
        push_next_launches(S, LS, lev);
        if (tiled.empty()) continue;
        tiles_launch(S, LS, lev, tiled);
        chain_launches(S, LS.knobs.chain_split, lev, tiled);
    }
    splice_side_launches(S, LS);
}

// Forward solve, level by level.  Fills solve_small_list / _ranges, solve_panels, solve_mtasks, solve_wide_list,
// solve_fix_list, S.solve, n_solve_wide; takes ticket counters from n_solve_chain_launches.
void forward_solve_launches(Schedule& S, const LaunchKnobs& K) {
    // chain launches take their work by ticket (producers first): any number of workgroups is fine
    const int max_chain = K.force_unfused ? -1 : INT_MAX;
    std::vector<int> sbigs;
    for (int lev = 0; lev < S.nlevels; ++lev) {
        sbigs.clear();
        if (lev == 0 && S.n_solve_subtrees > 0) {
            Launch L = subtrees_launch(kLaunchSolveSmall);
            L.count = subtree_ranges(
                S, S.solve_subtree, S.n_solve_subtrees, S.solve_cost, [&] { return (int32_t)S.solve_small_list.size(); },
                [&](int32_t t) {
                    S.solve_small_list.push_back(t);
                    L.width = std::max<int32_t>(L.width, S.sn[t].w);
                },
                S.solve_small_ranges);
            if (L.count > 0) S.solve.push_back(L);
        }
        {
            // supernodes of one block column: the tiny ones (width <= kTinyWidth: one wave each) in a launch of
            // their own when there are enough of them, the others one workgroup each
            // (forward: the second width class of the one-wave kernel measured no faster than the workgroup kernel)
            std::vector<int32_t> tiny, narrow;
            for (int q = S.levelPtr[lev]; q < S.levelPtr[lev + 1]; ++q) {
                const int t = S.levelSet[q];
                if (!S.active[t] || S.solve_subtree[t] >= 0) continue;
                if (S.sn[t].w <= kTinyWidth) tiny.push_back(t);
                else if (S.sn[t].w <= kTile) narrow.push_back(t);
                else sbigs.push_back(t);
            }
            if (!narrow.empty() && tiny.size() < 64) {
                narrow.insert(narrow.end(), tiny.begin(), tiny.end());
                tiny.clear();
            }
            for (const std::vector<int32_t>* group : {&tiny, &narrow}) {
                if (group->empty()) continue;
                Launch L = solve_small_launch((int32_t)S.solve_small_list.size(), (int32_t)group->size(), lev);
                for (int32_t t : *group) {
                    S.solve_small_list.push_back(t);
                    L.width = std::max<int32_t>(L.width, S.sn[t].w);  // widest supernode of the launch
                }
                S.solve.push_back(L);
            }
        }
        if (sbigs.empty()) continue;
        S.n_solve_wide += (int)sbigs.size();
        int chain_wgs = 0;
        for (int t : sbigs) chain_wgs += ceil_div(S.sn[t].r, kSolveRows);
        if (chain_wgs <= max_chain) {
            // one launch: every 256-row chunk of every wide supernode of the level
            Launch Lc = level_chain_launch(kLaunchSolvePanel, (int32_t)S.solve_panels.size(), lev, S.n_solve_chain_launches++,
                                           (int32_t)S.solve_mtasks.size());
            for (int t : sbigs)
                for (int c = 0; c * kSolveRows < S.sn[t].r; ++c)
                    S.solve_panels.push_back(PanelDesc{t, c, c * kSolveRows, 0});
            Lc.count = (int32_t)S.solve_panels.size() - Lc.first;
            // the same launch for many right-hand sides (k_solve_blocks_mrhs): the block columns of the triangles
            // first (producers, ascending), then the row chunks below the supernodes' own columns
            for (int t : sbigs)
                for (int jb = 0; jb * kTile < S.sn[t].w; ++jb) S.solve_mtasks.push_back(PanelDesc{t, jb, -1, 0});
            for (int t : sbigs)
                for (int c = 0, row0 = S.sn[t].w; row0 < S.sn[t].r; ++c, row0 += kSolveRowsMrhs)
                    S.solve_mtasks.push_back(PanelDesc{t, c, row0, 0});
            Lc.task_count = (int32_t)S.solve_mtasks.size() - Lc.task_first;
            S.solve.push_back(Lc);
            for (int t : sbigs) {
                for (int jb = 0; jb * kTile < S.sn[t].w; ++jb) {
                    S.solve_wide_list.push_back(t);
                    S.solve_wide_list.push_back(jb);
                }
            }
        } else {
            int maxnb = 0;
            for (int t : sbigs) maxnb = std::max(maxnb, ceil_div(S.sn[t].w, kTile));
            for (int jb = 0; jb < maxnb; ++jb) {
                Launch Lp = main_launch(kLaunchSolvePanel, (int32_t)S.solve_panels.size(), lev);
                for (int t : sbigs) {
                    const SnDesc& T = S.sn[t];
                    if (ceil_div(T.w, kTile) <= jb) continue;
                    const int wb = std::min(kTile, T.w - jb * kTile);
                    S.solve_panels.push_back(PanelDesc{t, jb, -1, 0});
                    for (int row0 = jb * kTile + wb; row0 < T.r; row0 += kSolveRows)
                        S.solve_panels.push_back(PanelDesc{t, jb, row0, 0});
                }
                Lp.count = (int32_t)S.solve_panels.size() - Lp.first;
                S.solve.push_back(Lp);
            }
            S.solve_fix_list.insert(S.solve_fix_list.end(), sbigs.begin(), sbigs.end());
        }
    }
    if (!S.solve_fix_list.empty())
        S.solve.push_back(fixup_launch((int32_t)S.solve_fix_list.size(), S.nlevels));
}

// backward solve: the supernodes that the level launches solve (the others: the subtree launch)
inline bool in_level_launches(const Schedule& S, int t) { return S.active[t] && S.bsolve_subtree[t] < 0; }

// Backward solve: the supernodes of one block column of a level: the tiny ones (one wave each: Launch::width_class = 1) in a
// launch of their own when there are enough of them, the others one workgroup each
void back_narrow_launches(Schedule& S, int lev) {
    std::vector<int32_t> tiny, tiny2, narrow;
    for (int q = S.levelPtr[lev]; q < S.levelPtr[lev + 1]; ++q) {
        const int t = S.levelSet[q];
        if (!in_level_launches(S, t) || S.sn[t].w > kTile) continue;
        (S.sn[t].w <= kTinyWidth ? tiny : S.sn[t].w <= kTinyWidth2 ? tiny2 : narrow).push_back(t);
    }
    // (a group too small for a launch of its own joins the next wider one; the second width class of the
    // one-wave kernel pays from a few hundred supernodes on: Flan-class backward solve 7.60 -> 7.32 ms, but
    // +6 % on the nd24k-class input with an extra launch per level)
    if (tiny2.size() < 512 && !narrow.empty()) {
        narrow.insert(narrow.end(), tiny2.begin(), tiny2.end());
        tiny2.clear();
    }
    if (tiny.size() < 64 && !(tiny2.empty() && narrow.empty())) {
        (tiny2.empty() ? narrow : tiny2).insert((tiny2.empty() ? narrow : tiny2).end(), tiny.begin(), tiny.end());
        tiny.clear();
    }
    for (const std::vector<int32_t>* group : {&tiny, &tiny2, &narrow}) {
        if (group->empty()) continue;
        Launch Ln = back_block_launch((int32_t)S.bsolve_blocks.size(), (int32_t)group->size(), lev,
                                      group == &tiny ? 1 : group == &tiny2 ? 2 : 0);
        for (int32_t t : *group) S.bsolve_blocks.push_back(PanelDesc{t, 0, 0, 0});
        S.bsolve.push_back(Ln);
    }
}

// Backward solve of level lev's wide supernodes in one chain launch (and, where it pays, a BACK_BELOW launch in front of it).
// One right-hand side: a block column's sums over the rows BELOW the supernode's own columns (x final there)
// need no hand-off, but in the chain launch only the block column's own four waves stream them -- a level of
// few, tall supernodes (the separators below the root: 53 workgroups for 0.9 GB of panel) ran at 1.2 TB/s.
// There the rows below go to a launch of their own, 512-row chunks over the whole device, partial sums into
// slots that the chain adds up in a fixed order (bitwise reproducible).
void back_chain_launch(Schedule& S, int below_mode, int lev) {
    Launch Lc = level_chain_launch(kLaunchBackBlock, (int32_t)S.bsolve_blocks.size(), lev, S.n_solve_chain_launches++,
                                   (int32_t)S.bsolve_pairs.size());
    int64_t groups_here = 0;
    for (int q = S.levelPtr[lev]; q < S.levelPtr[lev + 1]; ++q) {
        const int t = S.levelSet[q];
        if (S.active[t] && S.sn[t].w > kTile) groups_here += ceil_div(ceil_div(S.sn[t].w, kTile), kBackGroup);
    }
    const bool below_level = below_mode >= 2 || (below_mode == 1 && groups_here <= kBelowMaxGroups);
    Launch Lw = main_launch(kLaunchBackBelow, (int32_t)S.bsolve_below.size(), lev);
    for (int q = S.levelPtr[lev]; q < S.levelPtr[lev + 1]; ++q) {
        const int t = S.levelSet[q];
        const int nbc = ceil_div(S.sn[t].w, kTile);
        if (!S.active[t] || nbc < 2) continue;
        const int below = S.sn[t].r - S.sn[t].w;
        int32_t slot1 = 0;
        if (below_level && below >= (below_mode >= 2 ? 1 : kBelowRows) &&
            S.n_bpart_slots + (int64_t)nbc * ceil_div(below, kBelowRows) < 0x7fffffffLL) {
            const int nch = ceil_div(below, kBelowRows);
            slot1 = (int32_t)S.n_bpart_slots + 1;
            for (int jb = 0; jb < nbc; ++jb)
                for (int c = 0; c < nch; ++c)
                    S.bsolve_below.push_back(PanelDesc{t, jb, S.sn[t].w + c * kBelowRows, (int32_t)(S.n_bpart_slots + (int64_t)jb * nch + c)});
            S.n_bpart_slots += (int64_t)nbc * nch;
        }
        for (int jb = nbc - 1; jb >= 0; --jb) S.bsolve_blocks.push_back(PanelDesc{t, jb, 0, 0});
        for (int jb = nbc - 1; jb >= 0; jb -= kBackGroup)
            S.bsolve_pairs.push_back(PanelDesc{t, jb, std::min(kBackGroup, jb + 1), slot1});
    }
    Lw.count = (int32_t)S.bsolve_below.size() - Lw.first;
    if (Lw.count > 0) S.bsolve.push_back(Lw);
    Lc.count = (int32_t)S.bsolve_blocks.size() - Lc.first;
    Lc.task_count = (int32_t)S.bsolve_pairs.size() - Lc.task_first;
    S.bsolve.push_back(Lc);
}

// Backward solve: root level first.  Per level one chain launch for the block columns of
// the wide supernodes (last block column first: block jb waits for the published x of blocks
// jb+1.. of its supernode; every workgroup of the launch must be resident) and one launch for the
// supernodes of a single block; when the chain would not be resident, one launch per block-column
// index from the last one down.  Fills bsolve_blocks, bsolve_pairs, bsolve_below, bsolve_ranges, n_bpart_slots, S.bsolve.
void backward_solve_launches(Schedule& S, const LaunchKnobs& K) {
    const int max_chain = K.force_unfused ? -1 : INT_MAX;
    for (int lev = S.nlevels - 1; lev >= 0; --lev) {
        int maxnb = 0, wide_blocks = 0;
        for (int q = S.levelPtr[lev]; q < S.levelPtr[lev + 1]; ++q) {
            const int t = S.levelSet[q];
            if (!in_level_launches(S, t)) continue;
            const int nbc = ceil_div(S.sn[t].w, kTile);
            maxnb = std::max(maxnb, nbc);
            if (nbc > 1) wide_blocks += nbc;
        }
        if (wide_blocks > 0 && wide_blocks <= max_chain) {
            back_chain_launch(S, K.bsolve_below, lev);
            back_narrow_launches(S, lev);
            continue;
        }
        for (int jb = maxnb - 1; jb >= 1; --jb) {
            Launch Lb = back_block_launch((int32_t)S.bsolve_blocks.size(), 0, lev, 0);
            for (int q = S.levelPtr[lev]; q < S.levelPtr[lev + 1]; ++q) {
                const int t = S.levelSet[q];
                if (in_level_launches(S, t) && ceil_div(S.sn[t].w, kTile) > jb) S.bsolve_blocks.push_back(PanelDesc{t, jb, 0, 0});
            }
            Lb.count = (int32_t)S.bsolve_blocks.size() - Lb.first;
            if (Lb.count > 0) S.bsolve.push_back(Lb);
        }
        if (maxnb > 1) {   // block column 0 of the wide supernodes (their other block columns: the launches above)
            Launch Lb = back_block_launch((int32_t)S.bsolve_blocks.size(), 0, lev, 0);
            for (int q = S.levelPtr[lev]; q < S.levelPtr[lev + 1]; ++q) {
                const int t = S.levelSet[q];
                if (in_level_launches(S, t) && ceil_div(S.sn[t].w, kTile) > 1) S.bsolve_blocks.push_back(PanelDesc{t, 0, 0, 0});
            }
            Lb.count = (int32_t)S.bsolve_blocks.size() - Lb.first;
            if (Lb.count > 0) S.bsolve.push_back(Lb);
        }
        back_narrow_launches(S, lev);
    }
    if (S.n_bsolve_subtrees > 0) {
        // the subtrees last: every ancestor outside them is final; inside, a workgroup walks from the subtree's
        // root down (the forward order reversed)
        Launch L = subtrees_launch(kLaunchBackBlock);
        L.width_class = 1;   // (tiny supernodes: one wave per subtree)
        std::vector<int32_t> members;
        L.count = subtree_ranges(
            S, S.bsolve_subtree, S.n_bsolve_subtrees, S.solve_cost,
            [&] {
                for (size_t q = members.size(); q-- > 0;) S.bsolve_blocks.push_back(PanelDesc{members[q], 0, 0, 0});
                members.clear();
                return (int32_t)S.bsolve_blocks.size();
            },
            [&](int32_t t) { members.push_back(t); }, S.bsolve_ranges);
        if (L.count > 0) S.bsolve.push_back(L);
    }
}

}  // namespace

void build_launches(Schedule& S, const uint8_t* active, const uint8_t* active_pieces) {
    LaunchState LS;
    LS.knobs = read_launch_knobs(S);
    reset_launch_lists(S);
    apply_masks(S, active, active_pieces);
    cholesky_launches(S, LS);
    forward_solve_launches(S, LS.knobs);
    build_sub_tiers(S, LS.knobs);
    backward_solve_launches(S, LS.knobs);
    build_solve_one(S, LS.knobs, active != nullptr || active_pieces != nullptr);
}


// ONE-launch solves (schedule.hpp: Schedule::OneLists).  The lists of the launch that holds the supernodes of `member`:
// the supernodes are taken block column by block column (<= 64 columns, a window of the supernode's panel like a piece of
// the Cholesky view); what block p subtracts from the x of a row below its columns -- a later column of its supernode or
// a row of an ancestor -- goes into slot slot0[p] + (row - w) of a hand-off buffer (written once, so the data can be its
// own flag); the block that owns that row gathers its slots -- listed here per owner: (slot, column of the owner).
static void build_one_lists(const Schedule& S, const std::vector<uint8_t>& member, Schedule::OneLists& O) {
    const int ns = S.nsuper;
    O.clear();
    O.member = member;
    // the blocks in ticket order: level by level, a supernode's block columns from left to right
    std::vector<int32_t> blk_of_col((size_t)S.n, -1), blk_sn;
    for (int q = 0; q < ns; ++q) {
        const int t = S.levelSet[(size_t)q];
        if (!member[(size_t)t]) continue;
        const SnDesc& T = S.sn[t];
        for (int cb = 0; cb < T.w; cb += kTile) {
            SnDesc B = T;
            B.c0 = T.c0 + cb;
            B.w = std::min(kTile, T.w - cb);
            B.r = T.r - cb;
            B.px = T.px + (int64_t)cb * T.r + cb;
            B.pi = T.pi + cb;
            B.ld = T.r;
            for (int c = B.c0; c < B.c0 + B.w; ++c) blk_of_col[(size_t)c] = (int32_t)O.sn.size();
            O.slot0.push_back(O.nslots);
            O.wleft.push_back(T.w - cb);
            O.nslots += B.r - B.w;
            O.sn.push_back(B);
            blk_sn.push_back(t);
        }
    }
    const int nb = (int)O.sn.size();
    if (O.nslots > INT32_MAX / 2) throw std::runtime_error("schedule: too many hand-off slots for a ONE-launch solve");
    // column of the row k (counted inside block p's window of the panel): a later column of the supernode, or lR
    auto col_of = [&](int p, int k) {
        const SnDesc& T = S.sn[blk_sn[(size_t)p]];
        const int kk = (O.sn[(size_t)p].c0 - T.c0) + k;   // row of the supernode's panel
        return kk < T.w ? T.c0 + kk : S.rows[(size_t)T.pi + kk];
    };
    O.pull_ptr.assign((size_t)nb + 1, 0);
    for (int p = 0; p < nb; ++p)
        for (int k = O.sn[(size_t)p].w; k < O.sn[(size_t)p].r; ++k) {
            const int owner = blk_of_col[(size_t)col_of(p, k)];
            if (owner <= p) throw std::runtime_error("schedule: a row below a block's columns is not owned by a later block of the launch");
            O.pull_ptr[(size_t)owner + 1]++;
        }
    for (int p = 0; p < nb; ++p) O.pull_ptr[(size_t)p + 1] += O.pull_ptr[(size_t)p];
    O.pull_slot.resize((size_t)O.pull_ptr[(size_t)nb]);
    O.pull_pos.resize(O.pull_slot.size());
    std::vector<int32_t> at(O.pull_ptr.begin(), O.pull_ptr.end() - 1);
    for (int p = 0; p < nb; ++p)
        for (int k = O.sn[(size_t)p].w; k < O.sn[(size_t)p].r; ++k) {
            const int col = col_of(p, k), owner = blk_of_col[(size_t)col];
            const int32_t e = at[(size_t)owner]++;
            O.pull_slot[(size_t)e] = (int32_t)(O.slot0[(size_t)p] + (k - O.sn[(size_t)p].w));
            O.pull_pos[(size_t)e] = col - O.sn[(size_t)owner].c0;
        }
}

// Which solves go into ONE launch (schedule.hpp).  PARSY_SOLVE_ONE=0: never, 1: by size, 2: whatever the size (tests).
static void build_solve_one(Schedule& S, const LaunchKnobs& K, bool sharded) {
    const int ns = S.nsuper;
    S.solve_one = S.solve_one_back = S.one_subtrees = S.one_forced = S.one_big = false;
    S.one_f.clear();
    S.one_b.clear();
    const int mode = K.solve_one;
    if (mode == 0 || sharded || ns == 0 || (int)S.levelSet.size() != ns) return;   // (a rank's share of the supernodes: level launches)
    // with subtree launches: the supernodes outside them (the launch must be the first of `solve` / the last of `bsolve`)
    const bool sub = S.n_solve_subtrees > 0 || S.n_bsolve_subtrees > 0;
    std::vector<uint8_t> mf((size_t)ns, 1), mb((size_t)ns, 1);
    int64_t nf = ns, nbk = ns;
    if (sub) {
        nf = nbk = 0;
        for (int t = 0; t < ns; ++t) {
            mf[(size_t)t] = S.solve_subtree[t] < 0;
            mb[(size_t)t] = S.bsolve_subtree[t] < 0;
            nf += mf[(size_t)t];
            nbk += mb[(size_t)t];
        }
        int nfused_f = 0, nfused_b = 0;
        for (const Launch& l : S.solve) nfused_f += l.form == kFormSubtrees && l.kind == kLaunchSolveSmall;
        for (const Launch& l : S.bsolve) nfused_b += l.form == kFormSubtrees && l.kind == kLaunchBackBlock;
        const bool first_ok = nfused_f == (S.n_solve_subtrees > 0) && (nfused_f == 0 || S.solve.front().form == kFormSubtrees);
        const bool last_ok = nfused_b == (S.n_bsolve_subtrees > 0) && (nfused_b == 0 || S.bsolve.back().form == kFormSubtrees);
        if (!first_ok || !last_ok || nf == 0 || nbk == 0) return;
    }
    auto fits = [&](int64_t members) {
        return S.xsize <= kOneMaxEntries && members <= 2 * kOneMaxSupernodes &&
               (members <= kOneMaxSupernodes || S.xsize >= kOneLargeEntries * (int64_t)ns);
    };
    // (the backward solve also above the subtree launch of a much larger plan, one right-hand side at a time: Flan-class, 15 000
    // supernodes outside it, 5.76 -> 4.55 ms.  The forward solve there: 4.27 or 4.65 ms from one process to the next against
    // 4.60 - 4.64 of the level launches, and 560 MB of hand-off slots: it stays with the level launches)
    const bool ok_f = mode == 2 || fits(nf);
    const bool ok_b = mode == 2 || fits(nbk) || (sub && nbk <= kOneMaxSupernodesBig);
    S.one_big = mode != 2 && !fits(nbk);
    if (!ok_f && !ok_b) return;
    // (a pattern whose rows are not owned by later members -- not an etree's -- or too many slots: the plan keeps its
    // level launches instead of failing as a whole)
    try {
        if (ok_f) build_one_lists(S, mf, S.one_f);
        if (ok_b && (!ok_f || mb != mf)) build_one_lists(S, mb, S.one_b);
    } catch (const std::runtime_error&) {
        S.one_f.clear();
        S.one_b.clear();
        S.one_big = false;
        return;
    }
    S.one_subtrees = sub;
    S.one_forced = mode == 2;
    S.solve_one = ok_f;
    S.solve_one_back = ok_b;
}

int64_t simulate_chain(const Schedule& S, int slots) {
    if (slots < 1) slots = 1;
    std::vector<uint8_t> fin((size_t)std::max<int64_t>(S.n_tflags, 1), 0), prep(fin.size(), 0);
    struct Task {
        int32_t sn, I, J, role;  // role 0 walker, 1 prepared tile left of a diagonal tile, 2 prepared diagonal tile, 3 other
        int32_t k;               // walker: current step; others: block columns already seen published
    };
    int64_t stuck = 0;
    for (const Launch& L : S.chol) {
        if (L.kind != kLaunchChain) continue;
        std::vector<Task> resident;
        int64_t next = 0;
        const int64_t count = L.count;
        bool progress = true;
        while (progress && (next < count || !resident.empty())) {
            progress = false;
            while ((int)resident.size() < slots && next < count) {
                const TileDesc& td = S.tiles[(size_t)L.first + (size_t)next++];
                const SnDesc& D = S.csn[td.sn];
                const int nbc = ceil_div(D.w, kTile);
                Task t{td.sn, td.row0 / kTile, td.col0 / kTile, 3, 0};
                if (t.I == 0 && t.J == 0) t.role = 0;
                else if (t.I == t.J) t.role = 2;
                else if (t.I == t.J + 1 && t.I < nbc) t.role = 1;
                if (L.rows_only && t.I < nbc) ++stuck;   // a rows launch holds no tile of a diagonal square
                resident.push_back(t);
                progress = true;
            }
            for (size_t q = 0; q < resident.size();) {
                Task& t = resident[q];
                const SnDesc& D = S.csn[t.sn];
                const int nbc = ceil_div(D.w, kTile);
                auto flag = [&](int I, int J) { return (size_t)D.tflag0 + (size_t)I * nbc + J; };
                bool done = false;
                if (t.role == 0) {
                    for (;;) {  // step k: diagonal tile k is published; then the two prepared tiles are needed
                        fin[flag(t.k, t.k)] = 1;
                        if (t.k + 1 >= nbc) {
                            done = true;
                            break;
                        }
                        if (!prep[flag(t.k + 1, t.k)] || !prep[flag(t.k + 1, t.k + 1)]) break;
                        fin[flag(t.k + 1, t.k)] = 1;
                        ++t.k;
                        progress = true;
                    }
                } else {
                    const int need = t.role == 2 ? t.J - 1 : t.J;
                    while (t.k < need && fin[flag(t.I, t.k)] && fin[flag(t.J, t.k)]) ++t.k;
                    if (t.k >= need) {
                        if (t.role == 3) {
                            if (fin[flag(t.J, t.J)]) {
                                fin[flag(t.I, t.J)] = 1;
                                done = true;
                            }
                        } else {
                            prep[flag(t.I, t.J)] = 1;
                            done = true;
                        }
                    }
                }
                if (done) {
                    resident[q] = resident.back();
                    resident.pop_back();
                    progress = true;
                } else {
                    ++q;
                }
            }
        }
        stuck += (count - next) + (int64_t)resident.size();
    }
    return stuck;
}

// The launches of both solves: every active supernode of one block column is solved exactly once in each direction
// (subtree runs in index order forward, reversed backward; a member's ancestors inside the run), every 256-row
// chunk / block column of an active wide supernode appears once, the backward chain's groups cover a supernode's
// block columns from the last one down, a level's launches come after (forward) / before (backward) the levels
// below it.
static void check_solve_launches(const Schedule& S, const std::function<void(const std::string&)>& fail) {
    const int ns = S.nsuper;
    std::vector<int> level_of(ns, 0);
    for (int l = 0; l < S.nlevels; ++l)
        for (int q = S.levelPtr[l]; q < S.levelPtr[l + 1]; ++q) level_of[S.levelSet[q]] = l;
    // ---- forward
    {
        std::vector<int> seen(ns, 0);
        std::vector<int64_t> chunks(ns, 0);
        int last_level = -1;
        for (const Launch& l : S.solve) {
            if (l.kind == kLaunchSolveSmall) {
                if (l.form == kFormSubtrees) {
                    for (int b = l.first; b < l.first + l.count; ++b) {
                        const int32_t q0 = S.solve_small_ranges[2 * (size_t)b], q1 = S.solve_small_ranges[2 * (size_t)b + 1];
                        if (q0 < 0 || q1 <= q0 || q1 > (int32_t)S.solve_small_list.size()) {
                            fail("forward subtree launch: bad range " + std::to_string(b));
                            continue;
                        }
                        for (int32_t q = q0; q < q1; ++q) {
                            const int t = S.solve_small_list[q];
                            seen[t]++;
                            if (q > q0 && t <= S.solve_small_list[q - 1]) fail("forward subtree run is not in index order");
                            if (S.sn[t].w > l.width) fail("forward subtree launch: supernode wider than the launch's width class");
                        }
                    }
                } else {
                    if (l.level < last_level) fail("forward solve launches go down a level");
                    last_level = l.level;
                    for (int q = l.first; q < l.first + l.count; ++q) {
                        const int t = S.solve_small_list[q];
                        seen[t]++;
                        if (level_of[t] != l.level) fail("forward launch holds a supernode of another level");
                        if (S.sn[t].w > l.width || S.sn[t].w > kTile) fail("forward launch: supernode wider than its width class");
                    }
                }
            } else if (l.kind == kLaunchSolvePanel) {
                if (l.level < last_level) fail("forward solve launches go down a level");
                last_level = l.level;
                for (int q = l.first; q < l.first + l.count; ++q) {
                    const PanelDesc& pd = S.solve_panels[q];
                    if (pd.sn < 0 || pd.sn >= ns || S.sn[pd.sn].w <= kTile || level_of[pd.sn] != l.level)
                        fail("forward chain launch: bad chunk descriptor " + std::to_string(q));
                    else if (l.form == kFormChain) {
                        if (pd.row0 != pd.jb * kSolveRows || pd.row0 >= S.sn[pd.sn].r) fail("forward chain launch: bad chunk rows");
                        chunks[pd.sn]++;
                    }
                }
                if (l.form == kFormChain) {
                    // the same launch for many right-hand sides: per supernode its block columns in ascending order BEFORE
                    // anything that waits for them (tickets go in list order), every row below its columns exactly once
                    if (l.task_first < 0 || l.task_count < 0 || (size_t)l.task_first + (size_t)l.task_count > S.solve_mtasks.size())
                        fail("forward chain launch solve[" + std::to_string(&l - S.solve.data()) + "]: bad task range (many right-hand sides)");
                    else {
                        std::vector<int> next_block(ns, 0);
                        std::vector<int64_t> next_row(ns, -1);
                        for (int q = l.task_first; q < l.task_first + l.task_count; ++q) {
                            const PanelDesc& pd = S.solve_mtasks[(size_t)q];
                            if (pd.sn < 0 || pd.sn >= ns || S.sn[pd.sn].w <= kTile || level_of[pd.sn] != l.level) {
                                fail("forward chain launch: bad task " + std::to_string(q));
                                continue;
                            }
                            const SnDesc& T = S.sn[pd.sn];
                            if (pd.row0 < 0) {
                                if (pd.jb != next_block[pd.sn]++ || pd.jb * kTile >= T.w) fail("forward chain launch: block columns out of order");
                                if (next_row[pd.sn] >= 0) fail("forward chain launch: a block column after the row chunks that wait for it");
                            } else {
                                if (next_block[pd.sn] != ceil_div(T.w, kTile)) fail("forward chain launch: row chunk before the supernode's block columns");
                                if (next_row[pd.sn] < 0) next_row[pd.sn] = T.w;
                                if (pd.row0 != next_row[pd.sn] || pd.row0 >= T.r) fail("forward chain launch: row chunks do not tile the rows below");
                                next_row[pd.sn] = pd.row0 + kSolveRowsMrhs;
                            }
                        }
                        for (int q = l.first; q < l.first + l.count; ++q) {
                            const int t = S.solve_panels[q].sn;
                            if (t < 0 || t >= ns) continue;
                            const SnDesc& T = S.sn[t];
                            if (next_block[t] != ceil_div(T.w, kTile) || (T.r > T.w && next_row[t] < T.r) || (T.r == T.w && next_row[t] >= 0))
                                fail("forward chain launch: supernode " + std::to_string(t) + " is not covered by the many-right-hand-side tasks");
                        }
                    }
                }
            }
        }
        for (int t = 0; t < ns; ++t) {
            const bool narrow = S.sn[t].w <= kTile;
            if (narrow && seen[t] != (S.active[t] ? 1 : 0))
                fail("supernode " + std::to_string(t) + " is in " + std::to_string(seen[t]) + " forward launches");
            if (!narrow && S.solve_fix_list.empty() && chunks[t] != (S.active[t] ? ceil_div(S.sn[t].r, kSolveRows) : 0))
                fail("wide supernode " + std::to_string(t) + ": " + std::to_string(chunks[t]) + " forward chunks");
        }
    }
    // ---- backward
    {
        std::vector<int> seen(ns, 0);
        std::vector<int64_t> blocks(ns, 0), grouped(ns, 0);
        {
            // k_bsolve_below: every slot written exactly once, by the task of its (supernode, block column, chunk); a
            // chain group that names slots finds all of its supernode's there, and the launch that fills them comes first
            std::vector<uint8_t> slot_seen((size_t)S.n_bpart_slots, 0);
            for (const PanelDesc& pd : S.bsolve_below) {
                const SnDesc& T = S.sn[(size_t)pd.sn];
                if (pd.pad < 0 || pd.pad >= S.n_bpart_slots || slot_seen[(size_t)pd.pad]++) fail("backward solve: a partial-sum slot is written twice or out of range");
                if (pd.row0 < T.w || pd.row0 >= T.r || (pd.row0 - T.w) % kBelowRows || pd.jb < 0 || pd.jb * kTile >= T.w)
                    fail("backward solve: a k_bsolve_below task has a bad chunk");
            }
            for (uint8_t v : slot_seen)
                if (v != 1) fail("backward solve: a partial-sum slot is never written");
            int64_t below_done = 0;
            for (const Launch& l : S.bsolve) {
                if (l.kind == kLaunchBackBelow) below_done += l.count;
                if (l.kind != kLaunchBackBlock || l.form != kFormChain) continue;
                for (int g = l.task_first; g < l.task_first + l.task_count; ++g) {
                    const PanelDesc& pd = S.bsolve_pairs[(size_t)g];
                    if (pd.pad <= 0) continue;
                    const SnDesc& T = S.sn[(size_t)pd.sn];
                    const int nch = ceil_div(T.r - T.w, kBelowRows), nbc = ceil_div(T.w, kTile);
                    const int64_t last = (int64_t)(pd.pad - 1) + (int64_t)nbc * nch;
                    if (T.r <= T.w || last > S.n_bpart_slots) fail("backward solve: a chain group names partial sums that do not exist");
                    // the tasks of this supernode are the slots [pad - 1, last): all before this launch
                    if (last > 0 && below_done < (int64_t)S.bsolve_below.size()) {
                        bool found = false;
                        for (int64_t q = 0; q < below_done && !found; ++q) found = S.bsolve_below[(size_t)q].pad == last - 1;
                        if (!found) fail("backward solve: a chain launch runs before the launch that forms its partial sums");
                    }
                }
            }
        }
        for (const Launch& l : S.bsolve) {
            if (l.kind != kLaunchBackBlock) continue;
            if (l.form == kFormSubtrees) {
                for (int b = l.first; b < l.first + l.count; ++b) {
                    const int32_t q0 = S.bsolve_ranges[2 * (size_t)b], q1 = S.bsolve_ranges[2 * (size_t)b + 1];
                    if (q0 < 0 || q1 <= q0 || q1 > (int32_t)S.bsolve_blocks.size()) {
                        fail("backward subtree launch: bad range " + std::to_string(b));
                        continue;
                    }
                    for (int32_t q = q0; q < q1; ++q) {
                        const int t = S.bsolve_blocks[q].sn;
                        seen[t]++;
                        if (q > q0 && t >= S.bsolve_blocks[q - 1].sn) fail("backward subtree run is not in reverse index order");
                        if (S.sn[t].w > kTinyWidth) fail("backward subtree launch: supernode wider than the one-wave kernel");
                    }
                }
                continue;
            }
            for (int q = l.first; q < l.first + l.count; ++q) {
                const PanelDesc& pd = S.bsolve_blocks[q];
                if (pd.sn < 0 || pd.sn >= ns || pd.jb < 0 || pd.jb * kTile >= S.sn[pd.sn].w || level_of[pd.sn] != l.level) {
                    fail("backward launch: bad block descriptor " + std::to_string(q));
                    continue;
                }
                if (S.sn[pd.sn].w <= kTile) {
                    seen[pd.sn]++;
                    if (l.width_class == 1 && S.sn[pd.sn].w > kTinyWidth) fail("backward launch: supernode wider than its width class");
                    if (l.width_class == 2 && S.sn[pd.sn].w > kTinyWidth2) fail("backward launch: supernode wider than its width class");
                } else {
                    blocks[pd.sn]++;
                }
            }
            if (l.form == kFormChain) {
                // the groups of the one-right-hand-side kernel: the same block columns, last one first
                int prev_sn = -1, next_jb = -1;
                for (int g = l.task_first; g < l.task_first + l.task_count; ++g) {
                    const PanelDesc& pd = S.bsolve_pairs[(size_t)g];
                    if (pd.sn != prev_sn) {
                        if (prev_sn >= 0 && next_jb != -1) fail("backward groups of supernode " + std::to_string(prev_sn) + " stop early");
                        prev_sn = pd.sn;
                        next_jb = ceil_div(S.sn[pd.sn].w, kTile) - 1;
                    }
                    if (pd.jb != next_jb || pd.row0 < 1 || pd.row0 > kBackGroup || pd.row0 > pd.jb + 1)
                        fail("backward group " + std::to_string(g) + " does not continue its supernode's block columns");
                    grouped[pd.sn] += pd.row0;
                    next_jb = pd.jb - pd.row0;
                }
                if (prev_sn >= 0 && next_jb != -1) fail("backward groups of supernode " + std::to_string(prev_sn) + " stop early");
            }
        }
        for (int t = 0; t < ns; ++t) {
            const int nbc = ceil_div(S.sn[t].w, kTile);
            if (nbc == 1 && seen[t] != (S.active[t] ? 1 : 0))
                fail("supernode " + std::to_string(t) + " is in " + std::to_string(seen[t]) + " backward launches");
            if (nbc > 1 && blocks[t] != (S.active[t] ? nbc : 0))
                fail("wide supernode " + std::to_string(t) + ": " + std::to_string(blocks[t]) + " backward blocks");
            if (nbc > 1 && S.active[t] && !S.bsolve_pairs.empty() && grouped[t] != nbc)
                fail("wide supernode " + std::to_string(t) + ": groups cover " + std::to_string(grouped[t]) + " block columns");
        }
    }
}

// The ONE-launch solves: the members are all supernodes or -- with subtree launches -- the ones outside the direction's
// subtree launch; the blocks tile the members in ticket order; every row below a block's columns has a slot of its own and
// is gathered exactly once, by the block that owns its column, at the right column, from a block with an earlier ticket
// (the backward solve takes the same blocks in reverse order).
template <class Fail>
static void check_one_lists(const Schedule& S, const Schedule::OneLists& O, const std::vector<int32_t>* subtree, const char* dir,
                            Fail&& fail) {
    const int ns = S.nsuper, nb = (int)O.sn.size();
    const std::string who = std::string("one-launch ") + dir + " solve: ";
    if ((int)O.member.size() != ns || (int)O.pull_ptr.size() != nb + 1 || (int)O.slot0.size() != nb || (int)O.wleft.size() != nb ||
        O.pull_slot.size() != O.pull_pos.size() || (int64_t)O.pull_slot.size() != O.nslots ||
        O.pull_ptr[(size_t)nb] != (int32_t)O.pull_slot.size()) {
        fail(who + "lists of the wrong length");
        return;
    }
    for (int t = 0; t < ns; ++t)
        if ((O.member[(size_t)t] != 0) != (subtree ? (*subtree)[(size_t)t] < 0 : true))
            fail(who + "supernode " + std::to_string(t) + " is on the wrong side of the subtree launch");
    std::vector<int32_t> blk_of_col((size_t)S.n, -1), slot_blk((size_t)O.nslots, -1), slot_col((size_t)O.nslots, -1);
    {
        int p = 0;
        int64_t slots = 0;
        for (int q = 0; q < ns; ++q) {
            const int t = S.levelSet[(size_t)q];
            if (!O.member[(size_t)t]) continue;
            const SnDesc& T = S.sn[t];
            for (int cb = 0; cb < T.w && p < nb; cb += kTile, ++p) {
                const SnDesc& B = O.sn[(size_t)p];
                const int wbk = std::min(kTile, T.w - cb);
                if (B.c0 != T.c0 + cb || B.w != wbk || B.r != T.r - cb || B.ld != T.r || B.px != T.px + (int64_t)cb * T.r + cb ||
                    B.pi != T.pi + cb || O.slot0[(size_t)p] != slots || O.wleft[(size_t)p] != T.w - cb)
                    fail(who + "block " + std::to_string(p) + " is not a block column of its supernode");
                for (int kk = cb + wbk; kk < T.r; ++kk) {
                    slot_blk[(size_t)(slots + (kk - cb - wbk))] = p;
                    slot_col[(size_t)(slots + (kk - cb - wbk))] = kk < T.w ? T.c0 + kk : S.rows[(size_t)T.pi + kk];
                }
                slots += B.r - B.w;
                for (int c = B.c0; c < B.c0 + B.w; ++c) blk_of_col[(size_t)c] = p;
            }
        }
        if (p != nb || slots != O.nslots) {
            fail(who + "the blocks do not tile the supernodes");
            return;
        }
    }
    std::vector<uint8_t> seen((size_t)O.nslots, 0);
    for (int p = 0; p < nb; ++p)
        for (int32_t e = O.pull_ptr[(size_t)p]; e < O.pull_ptr[(size_t)p + 1]; ++e) {
            const int32_t slot = O.pull_slot[(size_t)e], pos = O.pull_pos[(size_t)e];
            const bool in = slot >= 0 && slot < O.nslots;
            if (!in || seen[(size_t)slot] || pos < 0 || pos >= O.sn[(size_t)p].w || slot_col[(size_t)slot] != O.sn[(size_t)p].c0 + pos ||
                slot_blk[(size_t)slot] >= p) {
                fail(who + "bad entry " + std::to_string(e) + " in the gather list of block " + std::to_string(p));
                continue;
            }
            seen[(size_t)slot] = 1;
        }
    for (int64_t sl = 0; sl < O.nslots; ++sl)
        if (!seen[(size_t)sl]) fail(who + "slot " + std::to_string(sl) + " is never gathered");
}

template <class Fail>
static void check_solve_one(const Schedule& S, Fail&& fail) {
    if (!S.solve_one && !S.solve_one_back) return;
    if ((int)S.levelSet.size() != S.nsuper) {
        fail("one-launch solve: no level sets");
        return;
    }
    if (S.solve_one) check_one_lists(S, S.one_f, S.one_subtrees ? &S.solve_subtree : nullptr, "forward", fail);
    if (!S.solve_one_back) return;
    if (!S.one_b.sn.empty()) check_one_lists(S, S.one_b, S.one_subtrees ? &S.bsolve_subtree : nullptr, "backward", fail);
    else if (!S.solve_one) fail("one-launch backward solve: no lists");
    else if (S.one_subtrees)
        for (int t = 0; t < S.nsuper; ++t)
            if ((S.solve_subtree[t] < 0) != (S.bsolve_subtree[t] < 0)) {
                fail("one-launch backward solve: shares the forward lists although the subtree launches differ");
                break;
            }
    if (S.one_subtrees) {
        if (S.n_solve_subtrees > 0 && (S.solve.empty() || S.solve.front().form != kFormSubtrees))
            fail("one-launch forward solve: the subtree launch is not the first launch");
        if (S.n_bsolve_subtrees > 0 && (S.bsolve.empty() || S.bsolve.back().form != kFormSubtrees))
            fail("one-launch backward solve: the subtree launch is not the last launch");
    }
}

// The subtree / band launches of the many-right-hand-side solves (SubTier): every member a 16-column block of an active
// supernode with the panel window that goes with it; members of a tree in index order; every supernode in at most one tree,
// whole (all its blocks, left to right); the subtrees of tier 0 are those of the forward solve's subtree launch; every
// active supernode of a level <= sub_cover_level is in a tier and no launch list is needed for it; slots inside the tree's
// range, a member's own columns on the stack below its rows' targets; outside rows sorted and not columns of the tree.
template <class Fail>
static void check_sub_tiers(const Schedule& S, Fail&& fail) {
    if (S.sub_tiers.empty()) return;
    const int ns = S.nsuper;
    std::vector<int32_t> sn_of_col((size_t)S.n, -1);
    for (int t = 0; t < ns; ++t)
        for (int c = 0; c < S.sn[t].w; ++c) sn_of_col[(size_t)S.sn[t].c0 + c] = t;
    std::vector<int> level((size_t)ns, 0);
    for (int l = 0; l < S.nlevels; ++l)
        for (int q = S.levelPtr[l]; q < S.levelPtr[l + 1]; ++q) level[(size_t)S.levelSet[q]] = l;
    std::vector<int32_t> tree_of((size_t)ns, -1);
    int32_t next_tree = 0;
    for (size_t k = 0; k < S.sub_tiers.size(); ++k) {
        const SubTier& R = S.sub_tiers[k];
        if (R.tree0 != next_tree || R.ntrees <= 0 || (size_t)(R.tree0 + R.ntrees) > S.sub_trees.size())
            return fail("sub tiers: tiers do not tile the trees");
        next_tree = R.tree0 + R.ntrees;
        if (k == 0 && (size_t)R.ntrees != S.solve_small_ranges.size() / 2) return fail("sub tiers: tier 0 is not the subtree launch");
        for (int32_t b = R.tree0; b < R.tree0 + R.ntrees; ++b) {
            const SubTree& T = S.sub_trees[(size_t)b];
            if (T.m0 >= T.m1 || (size_t)T.m1 > S.sub_members.size() || T.ncols + T.nout + 1 > R.max_slots ||
                (size_t)(T.out0 + T.nout) > S.sub_out_rows.size())
                return fail("sub tiers: a tree's ranges");
            int32_t prev_sn = -1, expect_c = -1;
            for (int32_t q = T.m0; q < T.m1; ++q) {
                const SubMember& M = S.sub_members[(size_t)q];
                if (M.c0 < 0 || M.c0 >= S.n || M.w < 1 || M.w > kTinyWidth) return fail("sub tiers: a member's columns");
                const int t = sn_of_col[(size_t)M.c0];
                const SnDesc& D = S.sn[t];
                const int j0 = M.c0 - D.c0;
                if (!S.active[t] || j0 % kTinyWidth != 0 || M.w != std::min(kTinyWidth, D.w - j0) || M.r != D.r - j0 || M.ld != D.r ||
                    M.px != D.px + (int64_t)j0 * D.r + j0)
                    return fail("sub tiers: a member is not a 16-column block of an active supernode");
                if (j0 == 0) {
                    if (tree_of[(size_t)t] >= 0) return fail("sub tiers: a supernode in two trees");
                    if (t <= prev_sn) return fail("sub tiers: members out of index order");
                    if (k == 0 ? S.solve_subtree[t] < 0 : (level[(size_t)t] > R.top_level || S.sn[t].w > kSubTierMaxWidth))
                        return fail("sub tiers: a supernode that does not belong to its tier");
                    tree_of[(size_t)t] = b;
                    prev_sn = t;
                } else if (t != prev_sn || M.c0 != expect_c) {
                    return fail("sub tiers: the blocks of a supernode are not in a row");
                }
                expect_c = M.c0 + M.w;
                if (M.slot0 < 0 || M.slot0 + M.w > T.ncols) return fail("sub tiers: a member's column slots");
                const int nch = (M.r - M.w + 15) / 16;
                if ((size_t)(M.so + nch) * 16 > S.sub_slots.size()) return fail("sub tiers: a member's slot words");
                for (int ch = 0; ch < nch; ++ch)
                    for (int e = 0; e < 16; ++e) {
                        const int k2 = M.w + 16 * ch + 4 * (e & 3) + (e >> 2), slot = S.sub_slots[(size_t)(M.so + ch) * 16 + e];
                        if (k2 >= M.r) {
                            if (slot != T.ncols + T.nout) return fail("sub tiers: a padding row not in the padding slot");
                            continue;
                        }
                        const int32_t row = j0 + k2 < D.w ? D.c0 + j0 + k2 : S.rows[(size_t)D.pi + j0 + k2];
                        if (slot < T.ncols) {   // a column of a member of this tree that comes later
                            const int tt = sn_of_col[(size_t)row];
                            bool found = false;
                            for (int32_t q2 = q + 1; q2 < T.m1 && !found; ++q2) {
                                const SubMember& M2 = S.sub_members[(size_t)q2];
                                found = row >= M2.c0 && row < M2.c0 + M2.w && slot == M2.slot0 + row - M2.c0;
                            }
                            if (!found || tt < 0) return fail("sub tiers: a row's column slot does not belong to a later member");
                        } else if (slot >= T.ncols + T.nout || S.sub_out_rows[(size_t)T.out0 + slot - T.ncols] != row) {
                            return fail("sub tiers: a row's outside slot");
                        }
                    }
            }
            for (int32_t j = 0; j < T.nout; ++j) {
                const int32_t row = S.sub_out_rows[(size_t)T.out0 + j];
                if (j > 0 && row <= S.sub_out_rows[(size_t)T.out0 + j - 1]) return fail("sub tiers: outside rows not sorted");
                if (tree_of[(size_t)sn_of_col[(size_t)row]] == b) return fail("sub tiers: an outside row is a column of the tree");
            }
        }
    }
    for (int t = 0; t < ns; ++t) {
        if (S.solve_subtree[t] >= 0 && S.active[t] && tree_of[(size_t)t] < 0) return fail("sub tiers: a supernode of the subtree launch is missing");
        if (S.active[t] && level[(size_t)t] <= S.sub_cover_level && tree_of[(size_t)t] < 0) return fail("sub tiers: a covered level has a supernode outside the tiers");
    }
}

// The launch records themselves: a record's kind belongs to its list, and every field that its kind and form do not have
// holds its default -- what a positional initialiser of the record could not keep apart.
static void check_launch_records(const Schedule& S, const std::function<void(const std::string&)>& fail) {
    static const char* const kind_name[] = {"SMALL", "TILES", "CHAIN", "BIG", "BACK_BELOW", "SOLVE_SMALL", "SOLVE_PANEL",
                                            "SOLVE_FIXUP", "BACK_BLOCK", "DENSE"};
    auto check_list = [&](const std::vector<Launch>& seq, const char* list, auto&& in_list, int ntickets) {
        for (size_t i = 0; i < seq.size(); ++i) {
            const Launch& l = seq[i];
            const int k = l.kind;
            const bool known = k >= 0 && k <= kLaunchDense;
            const std::string who = std::string("launch ") + list + "[" + std::to_string(i) + "] (" + (known ? kind_name[k] : "?") + "): ";
            if (!known || !in_list(k)) {
                fail(who + "kind " + std::to_string(k) + " does not belong to this list");
                continue;
            }
            const bool may_chain = k == kLaunchSolvePanel || k == kLaunchBackBlock;
            const bool may_subtrees = k == kLaunchSmall || k == kLaunchSolveSmall || k == kLaunchBackBlock;
            if (!(l.form == kFormEach || (l.form == kFormChain && may_chain) || (l.form == kFormSubtrees && may_subtrees)))
                fail(who + "form " + std::to_string(l.form) + " is not one of its kind's");
            const bool chain_form = may_chain && l.form == kFormChain;
            if (l.first < 0 || l.count < 0) fail(who + "negative descriptor range");
            if (l.side != 0 && !(l.side == 1 && (k == kLaunchTiles || k == kLaunchBig || k == kLaunchDense)))
                fail(who + "side = " + std::to_string(l.side) + " on a kind that has no side-stream launches");
            if (l.wait_level < -1 || (l.wait_level != -1 && !l.side)) fail(who + "wait_level = " + std::to_string(l.wait_level) + " on a main-stream launch or below -1");
            if (l.rows_only != 0 && !(l.rows_only == 1 && k == kLaunchChain)) fail(who + "rows_only is set");
            if (l.ticket != 0 && !(k == kLaunchChain || chain_form)) fail(who + "has a ticket counter but takes no tickets");
            if (l.ticket < 0 || (l.ticket > 0 && l.ticket >= ntickets)) fail(who + "ticket counter " + std::to_string(l.ticket) + " does not exist");
            if ((l.lds_bytes != 0 || l.stage != 0) && k != kLaunchSmall) fail(who + "lds_bytes / stage are set");
            if (l.lds_bytes < 0 || l.stage < 0) fail(who + "negative lds_bytes / stage");
            if (l.width != 0 && k != kLaunchSolveSmall) fail(who + "width is set");
            if (l.width_class < 0 || l.width_class > 2 || (l.width_class != 0 && k != kLaunchBackBlock))
                fail(who + "width_class = " + std::to_string(l.width_class));
            if ((l.task_first != 0 || l.task_count != 0) && !chain_form) fail(who + "has a task range but is no chain-form launch");
        }
    };
    check_list(S.chol, "chol", [](int k) { return is_chol_launch(k); }, S.n_chain_launches);
    check_list(S.solve, "solve", [](int k) { return k == kLaunchSolveSmall || k == kLaunchSolvePanel || k == kLaunchSolveFixup; },
               S.n_solve_chain_launches);
    check_list(S.bsolve, "bsolve", [](int k) { return k == kLaunchBackBelow || k == kLaunchBackBlock; }, S.n_solve_chain_launches);
}

int64_t check_schedule(const Schedule& S, std::string& what) {
    int64_t bad = 0;
    auto fail = [&](const std::string& msg) {
        if (bad++ == 0) what = msg;
    };
    check_launch_records(S, fail);
    check_solve_launches(S, fail);
    check_solve_one(S, fail);
    check_sub_tiers(S, fail);
    if (S.solve_only) return bad;
    const int nc = (int)S.csn.size();
    // ---- pieces tile their supernode; levels respect the chain-extended etree
    for (int t = 0; t < S.nsuper; ++t) {
        int cols = 0;
        for (int p = S.piece0[t]; p < S.piece0[t + 1]; ++p) {
            const SnDesc& C = S.csn[p];
            if (C.c0 != S.sn[t].c0 + cols || C.rbias != cols || C.r != S.sn[t].r - cols || C.ld != S.sn[t].r)
                fail("piece " + std::to_string(p) + " is not a window of its supernode's panel");
            if (p > S.piece0[t] && S.level_of[p] != S.level_of[p - 1] + 1) fail("pieces of a supernode are not on consecutive levels");
            cols += C.w;
        }
        if (cols != S.sn[t].w) fail("pieces of supernode " + std::to_string(t) + " do not add up to its width");
    }
    // ---- every update comes from a lower level; wave + BIG entries cover it exactly (flop identity)
    std::vector<double> covered(S.upd.size(), 0.0);
    auto entry_flops = [](const WaveEntry& E, bool same_window) {
        const double K = E.K, mi = E.mn & 255, nj = (E.mn >> 8) & 255;
        return same_window ? K * nj * (nj + 1) + 2.0 * K * (mi - nj) * nj : 2.0 * K * mi * nj;
    };
    // a BIG entry is any block of the source's rows x rows: the pairs (i, j), i >= j, of it
    auto block_flops = [](const WaveEntry& E) {
        const int mi = E.mn & 255, nj = (E.mn >> 8) & 255;
        auto pairs_of = [](int ia, int m, int ja, int n) {
            double pairs = 0;
            for (int j = ja; j < ja + n; ++j) pairs += std::max(0, ia + m - std::max(ia, j));
            return pairs;
        };
        // (+ the strips that ride with a dense block: rows behind it x its columns, its rows x columns beside it)
        return 2.0 * E.K * (pairs_of(E.ia, mi, E.ja, nj) + pairs_of(E.ia + mi, big_strip_rows(E), E.ja, nj) +
                            pairs_of(E.ia, mi, E.ja + nj, big_strip_cols(E)));
    };
    for (int t = 0; t < nc; ++t) {
        const SnDesc& T = S.csn[t];
        for (int64_t u = T.upd0; u < T.upd0 + T.nupd; ++u)
            if (S.level_of[S.upd_src[u]] >= S.level_of[t]) fail("update " + std::to_string(u) + " comes from a level that is not below its target");
        if (is_small(T) || T.nupd == 0) continue;
        // map an entry back to its update: (src, K) is unique among the updates of one target
        auto find_upd = [&](const WaveEntry& E) -> int64_t {
            for (int64_t u = T.upd0; u < T.upd0 + T.nupd; ++u)
                if (S.upd[u].src == E.src && S.upd[u].K == E.K) return u;
            return -1;
        };
        if (S.sn_wp0[t] >= 0) {
            const int nbc = ceil_div(T.w, kTile), nbr = ceil_div(T.r, kTile);
            const int64_t* wp = &S.wave_ptr[S.sn_wp0[t]];
            for (size_t key = 0; key < (size_t)nbc * nbr * 8; ++key)
                for (int64_t e = wp[key]; e < wp[key + 1]; ++e) {
                    const WaveEntry& E = S.wave_entries[(size_t)e];
                    const int64_t u = find_upd(E);
                    const int mi = E.mn & 255, nj = (E.mn >> 8) & 255;
                    if (u < 0 || mi < 1 || mi > kSub || nj < 1 || nj > kSub || E.ia + mi > S.upd[u].m || E.ja + nj > S.upd[u].n1) {
                        fail("wave entry " + std::to_string(e) + " of piece " + std::to_string(t) + " has a bad window");
                        continue;
                    }
                    covered[(size_t)u] += entry_flops(E, E.ia == E.ja);
                }
        }
    }
    // What fixes the order of sums within a launch: no two tasks write the same entry of L.  Tasks of the tile cut own
    // disjoint super-tiles.  Tasks of re-cut conflict domains: per launch and piece every column belongs to at most one
    // domain (the tile cut counts as one), a domain's members all have the same rows, its tasks have pairwise
    // disjoint windows of that index, and every entry's rows lie in its task's window.  Tasks of interval domains (members'
    // rows differ): pairwise different (row interval, column interval), and over all entries of the domain every panel
    // position named under interval index i lies below every position named under a larger index -- so the rectangles
    // interval i x interval j of the piece's panel are disjoint, and an entry's positions lie in its task's.
    std::vector<int32_t> col_domain;                  // of the current (launch, piece): -1 = not named yet
    std::map<int32_t, int64_t> domain_upd;            // ... domain -> its first update seen: the rows every member must have
    std::vector<std::array<int32_t, 3>> domain_wins;  // ... (domain, row0, col0) of its tasks
    std::map<std::pair<int32_t, int32_t>, std::pair<int32_t, int32_t>> ival_span;   // ... (interval domain, index) -> (lowest, highest) position named
    const Schedule::BigTask* group = nullptr;
    auto close_group = [&]() {
        int32_t dom = 0, top = -1;
        for (const auto& kv : ival_span) {
            if (kv.first.first != dom) dom = kv.first.first, top = -1;
            if (kv.second.first <= top)
                fail("intervals " + std::to_string(kv.first.second) + " and below of a conflict domain of piece " + std::to_string(group->sn) + " overlap");
            top = std::max(top, kv.second.second);
        }
        ival_span.clear();
        std::sort(domain_wins.begin(), domain_wins.end());
        if (std::adjacent_find(domain_wins.begin(), domain_wins.end()) != domain_wins.end())
            fail("two BIG tasks of piece " + std::to_string(group->sn) + " own the same window of a conflict domain");
        domain_wins.clear();
        domain_upd.clear();
    };
    for (const Schedule::BigTask& b : S.big_all) {
        const SnDesc& T = S.csn[b.sn];
        if (b.src_level >= S.level_of[b.sn] || (b.next != 0) != (b.src_level == S.level_of[b.sn] - 1))
            fail("BIG task of piece " + std::to_string(b.sn) + " is filed under the wrong source level");
        if (!group || group->sn != b.sn || group->src_level != b.src_level || group->next != b.next) {
            if (group) close_group();
            group = &b;
            col_domain.assign((size_t)T.w, -1);
        }
        const int win_r = kBigTile * b.sr, win_c = kBigTile * b.sc;
        if (b.domain < 0 || b.sr < 1 || b.sc < 1 || b.row0 % win_r || b.col0 % win_c || b.row0 + win_r <= b.col0 ||
            (b.domain ? b.sr != 1 || b.sc != 1 : b.row0 >= T.r || b.col0 >= T.w))
            fail("BIG task of piece " + std::to_string(b.sn) + " has a bad tile origin");
        if (b.domain) domain_wins.push_back({b.domain, b.row0, b.col0});
        for (int64_t e = b.e0; e < b.e1; ++e) {
            const WaveEntry& E = S.big_entries[(size_t)e];
            int64_t u = -1;
            for (int64_t q = T.upd0; q < T.upd0 + T.nupd; ++q)
                if (S.upd[q].src == E.src && S.upd[q].K == E.K) u = q;
            const int mi = E.mn & 255, nj = (E.mn >> 8) & 255;
            const bool ident = big_ident(E);
            const int ms = big_strip_rows(E), ns = big_strip_cols(E);
            if ((ms || ns) && (e >= b.em || mi != kBigTile || nj != kBigTile || ms > kStripMax || ns > kStripMax))
                fail("BIG entry " + std::to_string(e) + " carries a strip but is not a full dense block");
            if (u < 0 || mi < 1 || mi > kBigTile || nj < 1 || nj > kBigTile || E.ia + mi + ms > S.upd[u].m || E.ja + nj + ns > S.upd[u].n1 ||
                ident != (S.upd[u].rel < 0) || S.level_of[S.upd_src[u]] != b.src_level) {
                fail("BIG entry " + std::to_string(e) + " of piece " + std::to_string(b.sn) + " has a bad window or source");
                continue;
            }
            auto rel_at = [&](int k) { return ident ? k : S.relpos[(size_t)S.upd[u].rel + k] - T.rbias; };
            for (int k = E.ja; k < E.ja + nj + ns; ++k) {
                int32_t& d = col_domain[(size_t)rel_at(k)];
                if (d >= 0 && d != b.domain)
                    fail("column " + std::to_string(rel_at(k)) + " of piece " + std::to_string(b.sn) + " belongs to two conflict domains of a launch");
                d = b.domain;
            }
            if (!b.domain) {
                // tile cut: the rows it names land in the task's tile
                if (rel_at(E.ia) / win_r != b.row0 / win_r || rel_at(E.ia + mi + ms - 1) / win_r != b.row0 / win_r ||
                    rel_at(E.ja) / win_c != b.col0 / win_c || rel_at(E.ja + nj + ns - 1) / win_c != b.col0 / win_c)
                    fail("BIG entry " + std::to_string(e) + " names rows outside its task's tile");
            } else if (b.domain >= kIntervalDomain) {
                // interval cut: the positions it names, filed under its task's row and column interval
                auto name = [&](int32_t index, int k0, int k1) {
                    auto& span = ival_span.emplace(std::make_pair(b.domain, index), std::make_pair(INT32_MAX, -1)).first->second;
                    span.first = std::min(span.first, (int32_t)rel_at(k0));
                    span.second = std::max(span.second, (int32_t)rel_at(k1 - 1));
                };
                name(b.row0 / kBigTile, E.ia, E.ia + mi + ms);
                name(b.col0 / kBigTile, E.ja, E.ja + nj + ns);
            } else {
                // re-cut: the rows it names lie in the task's window of the domain's index (a remainder of <= kStripMax
                // positions at the end of the index may sit in the window before it: recut_blocks) ...
                const UpdDesc& U = S.upd[u];
                auto inside = [](int first, int count, int win0, int len) {
                    const int end = first + count, wend = win0 + kBigTile;
                    return first >= win0 && (end <= wend || (end <= len && len - wend <= kStripMax));
                };
                if (!inside(E.ia, mi + ms, b.row0, U.m) || !inside(E.ja, nj + ns, b.col0, U.n1))
                    fail("BIG entry " + std::to_string(e) + " names rows outside its task's window");
                // ... and that index is every member's own row order
                const UpdDesc& U0 = S.upd[(size_t)domain_upd.emplace(b.domain, u).first->second];
                bool same = U.m == U0.m && U.n1 == U0.n1 && (U.rel < 0) == (U0.rel < 0);
                if (&U != &U0 && !ident) {
                    for (int k = E.ia; k < E.ia + mi + ms && same; ++k) same = S.relpos[(size_t)U.rel + k] == S.relpos[(size_t)U0.rel + k];
                    for (int k = E.ja; k < E.ja + nj + ns && same; ++k) same = S.relpos[(size_t)U.rel + k] == S.relpos[(size_t)U0.rel + k];
                }
                if (!same) fail("BIG entry " + std::to_string(e) + ": the members of its conflict domain do not have the same rows");
            }
            covered[(size_t)u] += block_flops(E);
        }
    }
    if (group) close_group();
    {
        // the BIG / DENSE launches hold every non-empty part (dense: [e0, em), ragged: [em, e1)) of every task of an
        // active target exactly once, under its (source level, kind), the dense part in a launch enqueued BEFORE the
        // one that holds the ragged part; padding tasks (XCD sequences of unequal length) have no entries
        std::vector<int64_t> starts;
        std::vector<int64_t> dense_pos(S.big_all.size(), -1), ragged_pos(S.big_all.size(), -1);
        int64_t li = 0;
        for (const Launch& l : S.chol) {
            ++li;
            if (l.kind != kLaunchBig && l.kind != kLaunchDense) continue;
            const bool dense = l.kind == kLaunchDense;
            const bool side = l.side != 0;
            auto find_task = [&](int64_t e) -> const Schedule::BigTask* {   // the task whose entry range holds big_entries[e]
                auto it = std::upper_bound(S.big_all.begin(), S.big_all.end(), e,
                                           [](int64_t v, const Schedule::BigTask& b) { return v < b.e0; });
                if (it == S.big_all.begin()) return nullptr;
                --it;
                return e < it->e1 ? &*it : nullptr;
            };
            auto right_launch = [&](const Schedule::BigTask& b) {
                return side != (b.next != 0) && (side ? l.wait_level : l.level - 1) == b.src_level;
            };
            for (int q = l.first; q < l.first + l.count; ++q) {
                const TileDesc& td = S.big_tasks[(size_t)q];
                if (td.wp >= td.sp) {
                    if (td.wp != td.sp) fail("BIG launch task " + std::to_string(q) + " has a negative entry range");
                    continue;
                }
                const Schedule::BigTask* it = find_task(td.wp);
                const bool ok = it && (dense ? (it->e0 == td.wp && it->em == td.sp && (td.part & ~kDenseStripTask) == it->dchunks &&
                                                ((td.part & kDenseStripTask) != 0) == (it->strips > 0))
                                             : (it->em == td.wp && it->e1 == td.sp));
                if (!ok || it->sn != td.sn || it->row0 != td.row0 || it->col0 != td.col0) {
                    fail("BIG launch task " + std::to_string(q) + " is not a task of the plan");
                    continue;
                }
                if (!right_launch(*it)) fail("BIG launch task " + std::to_string(q) + " runs in the launch of another source level");
                (dense ? dense_pos : ragged_pos)[(size_t)(it - S.big_all.data())] = li;
                starts.push_back(td.wp);
            }
        }
        std::sort(starts.begin(), starts.end());
        if (std::adjacent_find(starts.begin(), starts.end()) != starts.end()) fail("a BIG task is launched twice");
        int64_t want = 0;
        for (size_t k = 0; k < S.big_all.size(); ++k) {
            const Schedule::BigTask& b = S.big_all[k];
            if (b.em < b.e0 || b.em > b.e1) fail("BIG task " + std::to_string(k) + " has a bad dense / ragged split");
            int64_t dch = 0;
            int32_t nst = 0;
            for (int64_t e = b.e0; e < b.em; ++e) {
                const WaveEntry& E = S.big_entries[(size_t)e];
                nst += big_strip_rows(E) || big_strip_cols(E);
                if (E.K < kDenseChunk) fail("BIG entry " + std::to_string(e) + " is filed as dense but is narrower than a chunk");
                dch += ceil_div(E.K, kDenseChunk);
            }
            if (dch != b.dchunks) fail("BIG task " + std::to_string(k) + " has a wrong dense chunk count");
            if (nst != b.strips) fail("BIG task " + std::to_string(k) + " has a wrong count of entries with strips");
            if (!S.active_piece[b.sn]) continue;
            want += (b.em > b.e0) + (b.e1 > b.em);
            if (b.em > b.e0 && b.e1 > b.em && !(dense_pos[k] > 0 && ragged_pos[k] > dense_pos[k]))
                fail("BIG task " + std::to_string(k) + ": the ragged part is not launched after the dense part");
        }
        if ((int64_t)starts.size() != want)
            fail("BIG launches hold " + std::to_string(starts.size()) + " task parts, the active targets have " + std::to_string(want));
    }
    for (int t = 0; t < nc; ++t) {
        const SnDesc& T = S.csn[t];
        if (is_small(T)) continue;
        for (int64_t u = T.upd0; u < T.upd0 + T.nupd; ++u) {
            const UpdDesc& U = S.upd[u];
            const double want = (double)U.K * U.n1 * (U.n1 + 1) + 2.0 * U.K * (double)(U.m - U.n1) * U.n1;
            if (std::abs(covered[(size_t)u] - want) > 1e-9 * want + 0.5)
                fail("update " + std::to_string(u) + " of piece " + std::to_string(t) + " is not covered exactly once by its entries");
        }
    }
    // ---- subtree launches: what a member depends on is in the same subtree; a workgroup's run is in index
    // order; every active SMALL supernode is factored by exactly one workgroup of one launch
    for (int t = 0; t < nc; ++t) {
        const int real = S.csn_real[t], st = S.chol_subtree[real];
        if (st < 0) continue;
        if (!is_small(S.csn[t])) fail("supernode " + std::to_string(real) + " of a subtree is not a SMALL one");
        for (int64_t u = S.csn[t].upd0; u < S.csn[t].upd0 + S.csn[t].nupd; ++u)
            if (S.chol_subtree[S.csn_real[S.upd_src[u]]] != st)
                fail("supernode " + std::to_string(real) + " of a subtree is updated from outside the subtree");
    }
    {
        std::vector<int> seen(nc, 0);
        for (const Launch& l : S.chol) {
            if (l.kind != kLaunchSmall) continue;
            if (l.form == kFormSubtrees) {
                for (int b = l.first; b < l.first + l.count; ++b) {
                    const int32_t q0 = S.small_ranges[2 * (size_t)b], q1 = S.small_ranges[2 * (size_t)b + 1];
                    if (q0 < 0 || q1 <= q0 || q1 > (int32_t)S.small_list.size()) {
                        fail("subtree launch: bad range " + std::to_string(b));
                        continue;
                    }
                    for (int32_t q = q0; q < q1; ++q) {
                        seen[S.small_list[q]]++;
                        if (q > q0 && S.small_list[q] <= S.small_list[q - 1]) fail("subtree launch: a run is not in index order");
                        if (S.chol_subtree[S.csn_real[S.small_list[q]]] != S.chol_subtree[S.csn_real[S.small_list[q0]]])
                            fail("subtree launch: a run mixes subtrees");
                    }
                }
            } else {
                for (int q = l.first; q < l.first + l.count; ++q) seen[S.small_list[q]]++;
            }
        }
        for (int t = 0; t < nc; ++t)
            if (seen[t] != ((is_small(S.csn[t]) && S.active_piece[t]) ? 1 : 0))
                fail("SMALL supernode " + std::to_string(t) + " is in " + std::to_string(seen[t]) + " launches");
    }
    // ---- launch sequence: a side launch comes before the main-stream launches of the level that waits for it and
    // after every main-stream launch of the levels it waits for; the main stream never goes down a level
    int main_level = -1;
    for (size_t i = 0; i < S.chol.size(); ++i) {
        const Launch& l = S.chol[i];
        if (l.side) {
            if (l.wait_level >= 0 && main_level > l.wait_level + 0 && main_level >= l.level)
                fail("side launch " + std::to_string(i) + " is enqueued after the level that waits for it");
            for (size_t j = i + 1; j < S.chol.size(); ++j)
                if (!S.chol[j].side && S.chol[j].level <= l.wait_level)
                    fail("side launch " + std::to_string(i) + " precedes a main-stream launch of a level it waits for");
        } else {
            if (l.level < main_level) fail("main-stream launches go down a level");
            main_level = l.level;
        }
    }
    return bad;
}

}  // namespace parsy
