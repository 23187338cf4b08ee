// The dispatch of the solves (solve_route.hpp): every condition that chooses a solve kernel, a layout of X or a prologue.
// tests/solve_cases.py (predict) is the tests' independent copy of what is chosen here -- change both.
#include "solve_route.hpp"

#include <algorithm>
#include <cstdlib>

namespace parsy {

// The gates of the solves' kernel variants (SolveGates), from the environment.
SolveGates read_solve_gates() {
    SolveGates g;
    auto num = [](const char* name, int& v) {
        const char* e = std::getenv(name);
        if (e && *e) v = std::atoi(e);
        return e && *e;
    };
    int m = 0;
    num("PARSY_MRHS_MIN", m);
    if (m > 0) {
        g.mrhs_min = m;
        g.chain_mrhs_min = std::min(m, g.chain_mrhs_min);
    }
    num("PARSY_BMRHS_MIN", g.bmrhs_min);
    const char* w = std::getenv("PARSY_BMRHS_WIDE_ONLY");
    g.bmrhs_wide_only = !(w && w[0] == '0');
    num("PARSY_BMRHS_WIDE_BLOCKS", g.bmrhs_wide_blocks);
    num("PARSY_BCHAIN_MIN_BLOCKS", g.bchain_min_blocks);
    num("PARSY_SMALL_MRHS_HALVES_MIN", g.small_halves_min);
    num("PARSY_SUB_MRHS_MIN", g.sub_mrhs_min);
    g.xt_min_set = num("PARSY_XT_MIN", g.xt_min);
    num("PARSY_CHAIN_FEW_CHUNKS", g.chain_few_chunks);
    const char* st = std::getenv("PARSY_DEBUG_SOLVE_STALL");
    g.wait_bias = (st && st[0] == '1') ? (1 << 20) : 0;
    num("PARSY_SUB_ABL", g.sub_abl);
    return g;
}

namespace {

constexpr WitnessKernel kNothing = kWitnessCount;

// The subtree launches of a solve with this many right-hand sides take the form of one wave per subtree and 16 right-
// hand sides (trsv_sub_kernels.hip; PARSY_SUB_MRHS_MIN, 0: never)
// (the kernels address x by a 32-bit byte offset from a wave-uniform base: 16 rows or right-hand sides of either stride)
bool sub_tiers_usable(const Schedule& S, const SolveGates& G, const RouteRuntime& rt, int nrhs, int ldx) {
    const int m = G.sub_mrhs_min;
    return rt.sub_ntiers > 0 && !S.sub_tiers.empty() && m > 0 && nrhs >= m && ldx < (1 << 24) && nrhs < (1 << 20);
}

// SOLVE_SMALL by width, right-hand sides and count
WitnessKernel small_kernel(const SolveGates& G, const Launch& l, int nrhs) {
    if (nrhs < G.mrhs_min) return l.width <= kTinyWidth ? kWSolveTiny : kWSolveSmall;   // one wave per supernode (or per subtree of them) | a workgroup
    if (l.width <= 16) return kWSolveSmallMrhs16;
    if (l.width <= 32) return kWSolveSmallMrhs32;
    // (at most 32 right-hand sides: one sweep either way, fewer registers)
    return (l.count >= G.small_halves_min || nrhs <= 32) ? kWSolveSmallMrhs64Halves : kWSolveSmallMrhs64;
}

// BACK_BLOCK of every form but the one-right-hand-side chain and the subtree tiers
WitnessKernel back_block_kernel(const SolveGates& G, const Launch& l, int nrhs) {
    const bool chain = l.form == kFormChain;
    // many right-hand sides: 64 per pass, matrix cores, one wave per supernode
    if (l.width_class == 1 && nrhs >= G.bmrhs_min) return kWBsolveTinyMrhs;
    // width class kTinyWidth (1) or kTinyWidth2 (2), a subtree launch or a level's launch: one wave each
    if (l.width_class && nrhs < G.bmrhs_min) return l.width_class == 1 ? kWBsolveTiny16 : kWBsolveTiny32;
    // launches of few blocks (the top of the tree, small inputs: a chain of hand-offs, not a stream of L) keep the
    // light kernel -- 4 right-hand sides per workgroup, up to 8 workgroups per block side by side (nd24k-class, 16
    // right-hand sides: 1.02 ms against 2.06 with the matrix-core kernel everywhere)
    // (G.bmrhs_wide_only; PARSY_BMRHS_WIDE_ONLY=0: the matrix-core kernel everywhere)
    // (round 5) chain launches of more than 16 right-hand sides: k_bsolve_chain_mrhs from G.bchain_min_blocks (128) block
    // columns on (PARSY_BCHAIN_MIN_BLOCKS), 64 right-hand sides per pass
    if (chain && nrhs > 16 && nrhs >= G.bmrhs_min && l.count >= G.bchain_min_blocks) return kWBsolveChainMrhs;
    // 64 right-hand sides per pass over L, products on the matrix cores: launches of few blocks (the top of the tree,
    // small inputs) take 16 right-hand sides per pass in up to 8 workgroups per block side by side; the others 64 per
    // pass (L read once per 64)
    if (nrhs >= G.bmrhs_min && (!G.bmrhs_wide_only || l.count >= G.bmrhs_wide_blocks))
        return (l.count >= G.bmrhs_wide_blocks && nrhs > 16) ? kWBsolveBlockMrhs4 : kWBsolveBlockMrhs1;
    return nrhs == 1 ? kWBsolveBlock1 : kWBsolveBlock4;
}

// Whether a solve is ONE launch (its counters follow the status word in the hand-off buffers; no chain tickets)
// (how many right-hand sides: 8 where the launch has at most kOneSmallBlocks blocks -- ex15-class, 8: 0.130 -> 0.087 ms --, else
// 4 -- from 6 on the level launches use the matrix cores: nd24k-class, 8: 0.75 vs 1.24 ms this way; 4: 0.81 -> 0.60 --, and 1 for
// the backward solve beside a subtree launch -- parabolic_fem-class, 4: 0.79 vs 0.86 ms -- and for the much larger plans)
bool takes_one_launch(const Schedule& S, const RouteRuntime& rt, int nrhs, bool backward) {
    if (!(backward ? S.solve_one_back : S.solve_one)) return false;
    if (rt.one_off[backward ? 1 : 0]) return false;   // (its buffers could not be allocated)
    const size_t nblocks = backward ? S.one_back().sn.size() : S.one_f.sn.size();
    // (round 5, tools/gate_sweep.py: forward blocks of 5-8 right-hand sides through the ONE launch on factors of fewer than
    // 400 entries per row -- 2-D grids of 3 400 .. 14 000 supernodes 0.26 -> 0.18, 0.33 -> 0.24, 0.35 -> 0.31 ms; 3-D grids of
    // 580-670 entries per row lose 5 %, the backward solve loses wherever the plan is not small)
    // -- and up to 4 096 blocks: the parabolic_fem-class plan, 6 546 blocks, takes 8 right-hand sides through its subtree and
    // band launches in 0.51 ms against 0.60; likewise the backward solve beside a subtree launch: 4 right-hand sides per
    // ONE launch up to that size (grids of 2 000 .. 4 000 blocks: 0.44 -> 0.34, 1.11 -> 0.93, 0.81 -> 0.68, 0.40 -> 0.26 ms), one
    // beyond it (parabolic_fem-class, 4: 0.79 vs 0.86 ms)
    const bool mid = nblocks <= (size_t)kOneMidBlocks && !S.one_big;
    const bool f8 = !backward && mid && S.xsize < (int64_t)kOneRhs8Density * S.n;
    const int max_rhs = (S.one_forced || nblocks <= (size_t)kOneSmallBlocks || f8)   ? kOneMaxRhs
                        : (S.one_big || (backward && S.one_subtrees && !mid))        ? 1
                                                                                     : 4;
    return nrhs <= max_rhs;
}

// a launch outside the profiling record
void push_plain(SolveRoute& out, WitnessKernel k) {
    SolveStep s;
    s.kernel = k;
    out.steps.push_back(s);
}

// a launch record: always marked, enqueued where route_launch names a kernel
void push_launch(const Schedule& S, const SolveGates& G, const RouteRuntime& rt, bool backward, size_t li, int nrhs, int ldx,
                 SolveRoute& out) {
    const Launch& l = (backward ? S.bsolve : S.solve)[li];
    SolveStep s;
    s.kernel = route_launch(S, G, rt, l, nrhs, ldx);
    s.launch = (int32_t)li;
    if (s.kernel == kWSolveSubMrhs || s.kernel == kWBsolveSubMrhs) s.tier = 0;
    s.kind = l.kind, s.level = l.level, s.side = l.side, s.count = l.count;
    out.steps.push_back(s);
}

void push_marked(SolveRoute& out, WitnessKernel k, int tier, int kind, int count) {
    if (count <= 0) k = kNothing;   // (an empty launch is marked, not enqueued)
    SolveStep s;
    s.kernel = k;
    s.tier = tier;
    s.kind = kind, s.level = 0, s.side = 0, s.count = count;
    out.steps.push_back(s);
}

// what the prologue of a solve by level launches enqueues: k_solve_arm_wide, then k_diag_inverse for the wide supernodes
void push_prologue(const Schedule& S, int nrhs, SolveRoute& out) {
    const bool nwide = S.solve_wide_list.size() >= 2;
    out.dinv = nwide;
    out.bpart = out.bpart && nrhs == 1 && S.n_bpart_slots > 0;
    if (out.arm_wide) push_plain(out, kWSolveArmWide);
    if (nwide) push_plain(out, kWDiagInverse);
}

}  // namespace

WitnessKernel route_launch(const Schedule& S, const SolveGates& G, const RouteRuntime& rt, const Launch& l, int nrhs, int ldx) {
    const bool chain = l.form == kFormChain;
    // (the subtree launch with many right-hand sides: a wave per subtree and 16 right-hand sides, traffic in LDS)
    const bool tier0 = l.form == kFormSubtrees && sub_tiers_usable(S, G, rt, nrhs, ldx) && S.sub_tiers[0].ntrees == l.count;
    switch (l.kind) {
        case kLaunchSolveSmall:
            if (l.count <= 0) return kNothing;
            return tier0 ? kWSolveSubMrhs : small_kernel(G, l, nrhs);
        case kLaunchSolvePanel:
            if (chain && nrhs >= G.chain_mrhs_min)   // (narrow up to 16 right-hand sides)
                return l.task_count <= 0 ? kNothing : nrhs <= 16 ? kWSolveBlocksMrhsNarrow : kWSolveBlocksMrhs;
            if (l.count <= 0) return kNothing;
            if (chain) return l.count <= G.chain_few_chunks ? kWSolveChainW2 : kWSolveChainW4;   // (one right-hand side: chain_mrhs_min is at most 2)
            return kWSolvePanel;
        case kLaunchSolveFixup: return l.count <= 0 ? kNothing : kWSolveFixup;
        case kLaunchBackBelow: return (nrhs == 1 && l.count > 0) ? kWBsolveBelow : kNothing;
        case kLaunchBackBlock:
            // one right-hand side: the wave dataflow over block-column pairs
            if (chain && nrhs == 1) return l.task_count <= 0 ? kNothing : kWBsolveChainW;
            if (l.count <= 0) return kNothing;
            return tier0 ? kWBsolveSubMrhs : back_block_kernel(G, l, nrhs);
        default: return kNothing;
    }
}

void solve_route(const Schedule& S, const SolveGates& G, const RouteRuntime& rt, int nrhs, int ldx, bool backward,
                 SolveRoute& out) {
    out.clear();
    const std::vector<Launch>& seq = backward ? S.bsolve : S.solve;
    if (takes_one_launch(S, rt, nrhs, backward)) {
        // the whole solve -- or everything above the subtree launch, which comes first (forward) / follows (backward) -- is
        // ONE launch (k_solve_one, k_bsolve_one)
        // (a direction's buffers hold 1, 4 or 8 right-hand sides)
        out.one = true;
        out.one_cap = nrhs == 1 ? 1 : nrhs <= 4 ? 4 : kOneMaxRhs;
        const int c = out.one_cap == 1 ? 0 : out.one_cap == 4 ? 1 : 2;
        if (!backward) {
            if (S.one_subtrees && S.n_solve_subtrees > 0 && !seq.empty()) push_launch(S, G, rt, false, 0, nrhs, ldx, out);
            push_marked(out, (WitnessKernel)(kWSolveOne1 + c), -1, kLaunchSolveSmall, (int)S.one_f.sn.size());
        } else {
            push_marked(out, (WitnessKernel)(kWBsolveOne1 + c), -1, kLaunchBackBlock, (int)S.one_back().sn.size());
            if (S.one_subtrees && S.n_bsolve_subtrees > 0 && !seq.empty()) push_launch(S, G, rt, true, seq.size() - 1, nrhs, ldx, out);
        }
        out.tail = out.steps.size();
        return;
    }
    const int64_t cols = (int64_t)ldx * nrhs;
    if (!backward) {
        // From 16 right-hand sides on the solve works on X with the right-hand sides of a row contiguous (transposed in
        // and out: both kernels a solve of that many takes -- k_solve_small_mrhs, k_solve_blocks_mrhs -- read and write
        // whole rows then; a supernode's x block was 64 eight-byte pieces per column).  PARSY_XT_MIN=k (0: never).
        // (measured, 64 right-hand sides: Flan-class 23.1 -> 20.4 ms, nd24k-class 1.31 -> 1.19 ms; parabolic_fem-class 1.72 ->
        // 1.75 ms -- its factor has 67 entries per row and the two transposes, 0.3 ms, cost what the kernels gain: the layout
        // is taken from 200 entries of L per row on)
        out.use_xt = G.xt_min > 0 && nrhs >= G.xt_min && nrhs >= G.mrhs_min && S.solve_fix_list.empty() &&
                     (S.xsize >= (int64_t)150 * S.n || G.xt_min_set);
        out.ldq = out.use_xt ? (nrhs + 15) & ~15 : 0;
        const int64_t need = out.use_xt ? (int64_t)S.n * out.ldq : cols;
        // The chain launches of the wide supernodes take the whole buffer armed -- k_solve_chain_w (one right-hand side),
        // k_solve_blocks_mrhs (from G.chain_mrhs_min on) --, or where it can (no fixup list) the latter's prologue launch,
        // k_solve_arm_wide, arms their columns and zeroes the status word and the tickets.
        out.arm_wide = nrhs >= G.chain_mrhs_min && S.n_solve_wide > 0 && !S.solve_wide_list.empty() && S.solve_fix_list.empty();
        out.scratch = out.armed = S.n_solve_wide > 0 ? need : 0;
    } else {
        // (several right-hand sides and wide supernodes: one prologue launch instead of memsets + a fill of n x nrhs entries)
        const bool wide = !S.solve_wide_list.empty();
        out.arm_wide = nrhs > 1 && wide;
        out.scratch = S.max_width > kTile ? cols : 0;
        out.armed = wide ? cols : 0;
        out.bpart = true;
    }
    push_prologue(S, nrhs, out);
    if (out.use_xt && S.n > 0) push_plain(out, kWTransposeX);
    out.body = out.steps.size();
    // The level launches.  Where the subtree tiers serve the solve, the bands of levels that are one launch each take the
    // place of the level launches they cover: first in the forward solve, last in the backward one.
    if (!sub_tiers_usable(S, G, rt, nrhs, ldx) || S.sub_cover_level < 0) {
        for (size_t li = 0; li < seq.size(); ++li) push_launch(S, G, rt, backward, li, nrhs, ldx, out);
    } else {
        const int ntiers = std::min<int>(rt.sub_ntiers, (int)S.sub_tiers.size());
        if (!backward)
            for (int k = 0; k < ntiers; ++k) push_marked(out, kWSolveSubMrhs, k, kLaunchSolveSmall, S.sub_tiers[(size_t)k].ntrees);
        for (size_t li = 0; li < seq.size(); ++li)
            if (seq[li].form != kFormSubtrees && seq[li].level > S.sub_cover_level) push_launch(S, G, rt, backward, li, nrhs, ldx, out);
        if (backward)
            for (int k = ntiers; k-- > 0;) push_marked(out, kWBsolveSubMrhs, k, kLaunchBackBlock, S.sub_tiers[(size_t)k].ntrees);
    }
    out.tail = out.steps.size();
    if (out.use_xt && S.n > 0) push_plain(out, kWTransposeX);
}

int64_t route_kernels(const SolveRoute& R, int32_t* out, int64_t cap) {
    int64_t n = 0;
    for (const SolveStep& s : R.steps) {
        if (s.kernel == kNothing) continue;
        if (out && n < cap) out[n] = s.kernel;
        ++n;
    }
    return n;
}

void solve_route_levels(const Schedule& S, const SolveGates& G, const RouteRuntime& rt, int nrhs, int ldx, bool backward,
                        int lev0, int lev1, bool first, bool last, SolveRoute& out) {
    out.clear();
    if (first) {
        // (the wide supernodes' chains: one right-hand side forward hands over through the first ldx entries)
        const int64_t cols = (int64_t)ldx * nrhs;
        out.scratch = (S.n_solve_wide > 0 || S.max_width > kTile) ? cols : 0;
        out.armed = S.n_solve_wide == 0 ? 0 : (!backward && nrhs == 1) ? (int64_t)ldx : cols;
        out.bpart = backward;
        push_prologue(S, nrhs, out);
    }
    out.body = out.steps.size();
    const std::vector<Launch>& seq = backward ? S.bsolve : S.solve;
    for (size_t li = 0; li < seq.size(); ++li)
        if ((seq[li].level >= lev0 && seq[li].level < lev1) || (last && seq[li].kind == kLaunchSolveFixup))
            push_launch(S, G, rt, backward, li, nrhs, ldx, out);
    out.tail = out.steps.size();
}

}  // namespace parsy
