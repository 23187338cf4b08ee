// Which kernels a forward / backward solve launches, in which order: one pure host function of the schedule, the gates and
// what the plan learned at run time.  No HIP: the route of a plan can be built, printed (parsy_debug_solve_route) and
// tested without a device.  The executor (executor.hip) builds the route of every solve, runs one prologue from its facts and
// walks its steps; the launch functions of the trsv sources take the kernel the route chose and choose nothing.
#pragma once
#include <cstdint>
#include <utility>
#include <vector>

#include "schedule.hpp"

namespace parsy {

// The thresholds that choose between the solves' kernel variants, and the solves' diagnostics.  The defaults are the tuned
// values; the variables (diagnostics, tests: every variant can be forced) are read ONCE at the start of every forward /
// backward solve call (read_solve_gates, into the plan, on the host) -- not per process, so a test can change them between
// solves, and not per launch (a solve makes hundreds of launches).
// Every choice made with them is in ONE place in C++, solve_route.cpp.  tests/solve_cases.py (predict, GATE_DEFAULTS) is
// the tests' independent copy of these defaults and of those choices: a change here or in solve_route.cpp is made there
// too.  The host tier compares the two copies point by point (test_solve_route_host.py), the GPU tier both with the
// kernel witness.
struct SolveGates {
    int mrhs_min = 6;             // PARSY_MRHS_MIN=k (this: k, the next: min(k, 2)): narrow supernodes take k_solve_small_mrhs from here on
    int chain_mrhs_min = 2;       // ... the wide supernodes' chain k_solve_blocks_mrhs (armed hand-off buffer)
    int bmrhs_min = 16;           // PARSY_BMRHS_MIN: the backward solve's many-right-hand-side kernels
    bool bmrhs_wide_only = true;  // PARSY_BMRHS_WIDE_ONLY=0: k_bsolve_block_mrhs on launches of few blocks too
    int bmrhs_wide_blocks = 128;  // PARSY_BMRHS_WIDE_BLOCKS: launches of at least this many blocks take k_bsolve_block_mrhs<4> (64 right-hand sides per pass)
    int bchain_min_blocks = 128;  // PARSY_BCHAIN_MIN_BLOCKS: chain launches take k_bsolve_chain_mrhs from this many block columns on
    int small_halves_min = 512;   // PARSY_SMALL_MRHS_HALVES_MIN: k_solve_small_mrhs<64> sweeps in halves from this many supernodes on
    int sub_mrhs_min = 6;         // PARSY_SUB_MRHS_MIN: the subtree launches take the many-right-hand-side form (0: never)
    int xt_min = 16;              // PARSY_XT_MIN: forward solves of this many right-hand sides work on X row-major (0: never)
    bool xt_min_set = false;      // ... set: whatever the factor's density
    int chain_few_chunks = 384;   // PARSY_CHAIN_FEW_CHUNKS: one right-hand side, forward chain launches of more chunks take k_solve_chain_w<4>, the others <2>
    int wait_bias = 0;            // PARSY_DEBUG_SOLVE_STALL=1: 1 << 20, no hand-off wait of the solve is ever satisfied
    int sub_abl = 0;              // PARSY_SUB_ABL: ablation mask of the subtree kernels (diagnostic build, trsv_sub_kernels.hip)
};
SolveGates read_solve_gates();

// Kernel witness (diagnostics, tests): one host-side counter per solve kernel instantiation and per factor kernel that a
// launch function can enqueue, bumped next to its hipLaunchKernelGGL (a relaxed atomic add on the host: nothing on the
// GPU).  Exported through parsy_debug_kernel_* so that a test can prove which kernels a factorization or a solve ran.
// A solve's route names its kernels by these entries.
#define PARSY_WITNESS_KERNELS(X)                                                                                     \
    X(SolveTiny, "k_solve_tiny<16>")                                                                                 \
    X(SolveSmall, "k_solve_small")                                                                                   \
    X(SolveSmallMrhs16, "k_solve_small_mrhs<16>")                                                                    \
    X(SolveSmallMrhs32, "k_solve_small_mrhs<32>")                                                                    \
    X(SolveSmallMrhs64, "k_solve_small_mrhs<64>")                                                                    \
    X(SolveSmallMrhs64Halves, "k_solve_small_mrhs<64,true>")                                                         \
    X(SolvePanel, "k_solve_panel")                                                                                   \
    X(DiagInverse, "k_diag_inverse")                                                                                 \
    X(SolveChainW2, "k_solve_chain_w<2>")                                                                            \
    X(SolveChainW4, "k_solve_chain_w<4>")                                                                            \
    X(SolveBlocksMrhsNarrow, "k_solve_blocks_mrhs<true>")                                                            \
    X(SolveBlocksMrhs, "k_solve_blocks_mrhs<false>")                                                                 \
    X(TransposeX, "k_transpose_x")                                                                                   \
    X(SolveArmWide, "k_solve_arm_wide")                                                                              \
    X(SolveOne1, "k_solve_one<1>")                                                                                   \
    X(SolveOne4, "k_solve_one<4>")                                                                                   \
    X(SolveOne8, "k_solve_one<8>")                                                                                   \
    X(BsolveOne1, "k_bsolve_one<1>")                                                                                 \
    X(BsolveOne4, "k_bsolve_one<4>")                                                                                 \
    X(BsolveOne8, "k_bsolve_one<8>")                                                                                 \
    X(BsolveBlock1, "k_bsolve_block<1>")                                                                             \
    X(BsolveBlock4, "k_bsolve_block<4>")                                                                             \
    X(BsolveBlockMrhs1, "k_bsolve_block_mrhs<1>")                                                                    \
    X(BsolveBlockMrhs4, "k_bsolve_block_mrhs<4>")                                                                    \
    X(BsolveChainMrhs, "k_bsolve_chain_mrhs")                                                                        \
    X(BsolveTiny16, "k_bsolve_tiny<16>")                                                                             \
    X(BsolveTiny32, "k_bsolve_tiny<32>")                                                                             \
    X(BsolveTinyMrhs, "k_bsolve_tiny_mrhs")                                                                          \
    X(BsolveBelow, "k_bsolve_below")                                                                                 \
    X(BsolveChainW, "k_bsolve_chain_w")                                                                              \
    X(SolveFixup, "k_solve_fixup")                                                                                   \
    X(RhsOnes, "k_rhs_ones")                                                                                         \
    X(CopySegments, "k_copy_segments")                                                                               \
    X(SolveSubMrhs, "k_solve_sub_mrhs")                                                                              \
    X(BsolveSubMrhs, "k_bsolve_sub_mrhs")                                                                            \
    X(ScatterA, "k_scatter_a")                                                                                       \
    X(CholSmall, "k_chol_small")                                                                                     \
    X(CholTiles, "k_chol_tiles")                                                                                     \
    X(CholChain, "k_chol_chain")                                                                                     \
    X(CholChainRows, "k_chol_chain_rows")                                                                            \
    X(CholBig, "k_chol_big")                                                                                         \
    X(CholDense, "k_chol_dense")
enum WitnessKernel : int {
#define PARSY_WITNESS_ENUM(id, name) kW##id,
    PARSY_WITNESS_KERNELS(PARSY_WITNESS_ENUM)
#undef PARSY_WITNESS_ENUM
    kWitnessCount   // (in a route: a launch record that enqueues nothing)
};
void witness_launch(WitnessKernel k);

// What the choice depends on beyond the schedule and the gates.
struct RouteRuntime {
    bool one_off[2] = {false, false};   // forward, backward: the ONE-launch buffers could not be allocated -- level launches from then on
    int sub_ntiers = 0;                 // the subtree tiers that can be launched (a plan without a device: S.sub_tiers.size())
};

// One launch of a solve.  It runs on a launch record (launch: index into S.solve / S.bsolve), on a subtree tier (tier: index
// into S.sub_tiers; where a tier takes a record's place, both), or on neither: the ONE launch, k_transpose_x in and out,
// k_solve_arm_wide, k_diag_inverse.  kind < 0: the launch is not part of the profiling record; otherwise (kind, level,
// side, count) is what the record says of it.  kernel == kWitnessCount: the record is marked and nothing is enqueued
// (BACK_BELOW with more than one right-hand side).
struct SolveStep {
    WitnessKernel kernel = kWitnessCount;
    int32_t launch = -1, tier = -1;
    int32_t kind = -1, level = -1, side = 0, count = 0;
};

struct SolveRoute {
    std::vector<SolveStep> steps;   // in enqueue order: [0, body) before the profiling record, [body, tail) in it, [tail, ..) after
    size_t body = 0, tail = 0;
    // the prologue facts
    bool one = false;        // the solve is ONE launch (beside a subtree launch where the plan keeps those)
    int one_cap = 0;         // ... its capacity class: 1, 4 or 8 right-hand sides
    bool use_xt = false;     // the level launches work on X row-major ...
    int ldq = 0;             // ... with this row stride (0: the caller's layout)
    bool arm_wide = false;   // k_solve_arm_wide zeroes the status word and the tickets and arms the wide supernodes' columns
    int64_t scratch = 0;     // entries of xscratch
    int64_t armed = 0;       // ... the first so many armed by a fill (not with arm_wide)
    bool bpart = false;      // the backward partial sums are needed
    bool dinv = false;       // the inverse diagonal blocks are needed
    void clear() {   // (the steps keep their capacity)
        std::vector<SolveStep> keep = std::move(steps);
        keep.clear();
        *this = SolveRoute();
        steps = std::move(keep);
    }
};

// The kernel of one launch record of a solve with nrhs right-hand sides at a column stride of ldx (kWitnessCount: nothing).
// A subtree-form record whose trees are tier 0 goes to the tier's kernel where the tiers serve the solve.
WitnessKernel route_launch(const Schedule& S, const SolveGates& G, const RouteRuntime& rt, const Launch& l, int nrhs, int ldx);

// The route of a whole solve.  `out` is reused: its steps keep their capacity.
void solve_route(const Schedule& S, const SolveGates& G, const RouteRuntime& rt, int nrhs, int ldx, bool backward,
                 SolveRoute& out);
// ... and of one step of a solve in steps of etree levels [lev0, lev1): level launches only (no ONE launch, no bands), the
// caller's layout of X.  The
// prologue facts and launches are those of the solve's first step; the last step takes the fixup launches too.
void solve_route_levels(const Schedule& S, const SolveGates& G, const RouteRuntime& rt, int nrhs, int ldx, bool backward,
                        int lev0, int lev1, bool first, bool last, SolveRoute& out);

// The witness indices of the launches a route enqueues, in order (the steps that only mark a record left out): at most cap
// entries are written (out may be null); returns their number.
int64_t route_kernels(const SolveRoute& R, int32_t* out, int64_t cap);

}  // namespace parsy
