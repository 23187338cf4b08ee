// Launch wrappers of the HIP kernels (chol_kernels.hip, trsv_*kernels.hip).
// All pointers are device pointers; launches are asynchronous on `stream`.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "schedule.hpp"

namespace parsy {

constexpr int kPassLanes = 8;    // passes over the right-hand sides of a solve that run side by side

// The thresholds that choose between the solves' kernel variants, and the solves' diagnostics.  The defaults are the tuned
// values; the variables (diagnostics, tests: every variant can be forced) are read ONCE at the start of every forward /
// backward solve call (read_solve_gates, into the plan's DevicePattern, where the launch functions take them from) -- not
// per process, so a test can change them between solves, and not per launch (a solve makes hundreds of launches).
// tests/solve_cases.py (predict, GATE_DEFAULTS) mirrors these defaults and the choices the executor and the launch
// functions make with them, to pin the solve catalogue to its kernels without a GPU: a change here, in run_range /
// plan_solve / plan_backsolve (executor.hip) or in a launch function of the trsv sources is made there too.  The GPU
// tier compares that copy with the kernel witness, cell by cell.
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
    kWitnessCount
};
void witness_launch(WitnessKernel k);

struct DevicePattern {           // device copies of Schedule arrays
    const SnDesc* sn = nullptr;           // the supernodes (solve kernels)
    const SnDesc* csn = nullptr;          // Cholesky view (pieces of the very wide ones): Cholesky kernels
    const UpdDesc* upd = nullptr;
    const int32_t* relpos = nullptr;
    const int64_t* a_dst = nullptr;
    const int32_t* rows = nullptr;
    const WaveEntry* wave_entries = nullptr;  // update streams of the tile kernel
    const int64_t* wave_ptr = nullptr;
    const int64_t* split_ranges = nullptr;     // shares of the wave lists of tiles whose early stream is split
    double* tile_scratch = nullptr;            // partial tiles of the split streams
    const int32_t* small_list = nullptr;
    const int32_t* small_ranges = nullptr;        // subtree launches: (begin, end) pairs into the lists,
    const int32_t* solve_small_ranges = nullptr;  // one per workgroup
    const int32_t* bsolve_ranges = nullptr;
    const TileDesc* tiles = nullptr;
    const WaveEntry* big_entries = nullptr;   // BIG launches: (source, row window, column window) per task
    const TileDesc* big_tasks = nullptr;
    const int32_t* solve_small_list = nullptr;
    const PanelDesc* solve_panels = nullptr;
    const PanelDesc* solve_mtasks = nullptr;
    const int32_t* solve_fix_list = nullptr;
    const int32_t* solve_wide_list = nullptr;   // (supernode, block column) pairs: diagonal blocks to invert
    const PanelDesc* bsolve_pairs = nullptr;   // backward chain launches, one right-hand side: block-column pairs
    const PanelDesc* bsolve_below = nullptr;   // k_bsolve_below tasks
    double* bpart = nullptr;                   // their partial sums (64 doubles per slot; allocated by the first backward solve)
    const PanelDesc* bsolve_blocks = nullptr;  // backward solve: (supernode, block column) per workgroup  // supernodes solved by SOLVE_CHAIN (need inverse blocks)
    // the solves' subtree launch for many right-hand sides (Schedule::sub_*; sub_ntrees == 0: not available)
    const SubMember* sub_members = nullptr;
    const SubTree* sub_trees = nullptr;
    const uint16_t* sub_slots = nullptr;
    const int32_t* sub_out_rows = nullptr;
    int sub_ntiers = 0;
    int* info = nullptr;         // first failed pivot column + 1 (0x7f7f7f7f = none, < 0: wait timed out)
    int* tflags = nullptr;       // Cholesky chain: per tile, epoch of the factorization that published it
                                 // ([0, n_tflags): finished tiles, [n_tflags, 2 n_tflags): tiles prepared for the walker)
    int n_tflags = 0;
    int* tickets = nullptr;      // one counter per CHAIN launch (zeroed at the start of a factorization)
    int* sinfo = nullptr;        // status of the last solve: 0 ok, < 0 a hand-off wait timed out (own word: a solve
                                 // never touches the factorization's status)
    int* stickets = nullptr;     // one counter per chain launch of the forward / backward solve
    // ONE-launch solves (Schedule::OneLists; one_b = one_f where the backward solve shares the forward lists)
    struct OneDev {
        const SnDesc* sn = nullptr;          // the block columns (<= 64 columns each) in ticket order
        const int64_t* slot0 = nullptr;      // the first hand-off slot of each
        const int32_t* wleft = nullptr;      // the columns of its supernode from its first column on
        const int32_t* pull_ptr = nullptr;   // per block its gather list [ptr[p], ptr[p + 1]) of
        const int32_t* pull_slot = nullptr;  // ... (slot of the hand-off buffer,
        const int32_t* pull_pos = nullptr;   //      column of the block)
        int nblocks = 0;
        int64_t nslots = 1;
    } one_f, one_b;
    SolveGates gates;   // of the running solve (read_solve_gates at its start)
};

// lValues[a_dst[q]] = values[q]
void launch_scatter_a(const double* values, const int64_t* a_dst, double* L, int64_t nnz,
                      hipStream_t stream);
void launch_chol_small(const DevicePattern& P, int first, int count, int lds_bytes, int stage_cap, bool subtrees,
                       double* L, hipStream_t stream);
void launch_chol_big(const DevicePattern& P, int first, int count, double* L, hipStream_t stream);
void launch_chol_dense(const DevicePattern& P, int first, int count, double* L, hipStream_t stream);
void launch_chol_tiles(const DevicePattern& P, int first, int count, double* L, hipStream_t stream);
int chain_workgroups_per_cu();
void launch_chol_chain(const DevicePattern& P, int first, int count, int ticket, int epoch, bool rows, double* L,
                       hipStream_t stream);

void launch_solve_small(const DevicePattern& P, int first, int count, int wmax, bool subtrees, const double* L,
                        double* x, int nrhs, int ldx, int ldq, hipStream_t stream);
// (y: the hand-off buffer armed for this solve -- forward: nslots x cap, backward: n x cap values, cap = 1, 4 or 8 right-hand sides --,
// y_next: the one this solve arms for the next of its kind; state / state_next: {status, ticket} likewise)
void launch_solve_one(const DevicePattern& P, const double* L, double* x, int nrhs, int ldx,
                      double* y, double* y_next, int* state, int* state_next, int wait_bias, int cap, hipStream_t stream);
void launch_bsolve_one(const DevicePattern& P, int n, const double* L, double* x, int nrhs, int ldx,
                       double* y, double* y_next, int* state, int* state_next, int wait_bias, int cap, hipStream_t stream);
void launch_solve_panel(const DevicePattern& P, int first, int count, const double* L, double* x,
                        double* xscratch, int nrhs, int ldx, hipStream_t stream);
void launch_solve_chain(const DevicePattern& P, int first, int count, const double* L, const double* dinv, double* x,
                        double* xscratch, int ticket, int wait_bias, hipStream_t stream);   // (one right-hand side)
void launch_solve_blocks_mrhs(const DevicePattern& P, int first, int count, const double* L, const double* dinv,
                              double* x, double* xscratch, int nrhs, int ldx, int ldq, int ticket, int wait_bias,
                              hipStream_t stream);
void launch_transpose_x(double* x, int64_t ldx, double* xt, int64_t ldq, int n, int nrhs, bool to_rows, hipStream_t stream);
// the subtree launch of a solve with many right-hand sides: one wave per (subtree, 16 right-hand sides), the subtree's
// traffic in LDS (trsv_sub_kernels.hip); ldq > 0: X row-major with that row stride
void launch_solve_sub_mrhs(const DevicePattern& P, const SubTier& T, const double* L, double* x, int nrhs, int ldx, int ldq,
                           hipStream_t stream);
void launch_bsolve_sub_mrhs(const DevicePattern& P, const SubTier& T, const double* L, double* x, int nrhs, int ldx,
                            hipStream_t stream);
int solve_sub_prepare(int max_slots);   // once per plan: LDS beyond 64 KB per workgroup needs the kernels' attribute (-1: refused)
hipError_t solve_arm_handoff(double* xscratch, int64_t n, hipStream_t stream);
// several right-hand sides: status word + ticket counters zeroed and the hand-off buffer armed at the wide supernodes' columns
void launch_solve_arm_wide(const DevicePattern& P, int npairs, double* xscratch, int nrhs, int ldx, int ldq, int ntickets,
                           hipStream_t stream);
void launch_diag_inverse(const DevicePattern& P, int count, const double* L, double* dinv,
                         hipStream_t stream);
void launch_bsolve_chain_w(const DevicePattern& P, int first, int count, const double* L, const double* dinv,
                           double* x, double* xscratch, int ticket, int wait_bias, hipStream_t stream);
void launch_bsolve_below(const DevicePattern& P, int first, int count, const double* L, const double* x, hipStream_t stream);
void launch_bsolve_block(const DevicePattern& P, int first, int count, const double* L, const double* dinv,
                         double* x, double* xscratch, int nrhs, int ldx, LaunchForm form, int width_class, int ticket,
                         int wait_bias, hipStream_t stream);
void launch_rhs_ones(const DevicePattern& P, int nsuper, int max_rows, const double* L, double* b,
                     hipStream_t stream);
void launch_copy_segments(double* dst, const double* src, const int64_t* dst_off, const int64_t* src_off,
                          const int32_t* len, int64_t nseg, hipStream_t stream);
void launch_solve_fixup(const DevicePattern& P, int first, int count, double* x,
                        const double* xscratch, int nrhs, int ldx, hipStream_t stream);

}  // namespace parsy
