/*
 * parsy_amd.h -- C ABI of the MI355X-native supernodal Cholesky + BCSC
 * triangular-solve executor (libparsy_amd.so).
 *
 * Section 1 are DROP-IN replacements: same names, argument lists, ownership
 * and return values as the reference's executors, so the reference's drivers
 * (examples/choleskyTest01.cpp, choleskyTest03.cpp, triangularTest02.cpp) can
 * link this library instead of including the OpenMP headers.  All pointers
 * are caller-owned HOST pointers; the library uploads the pattern once per
 * distinct pointer set (cached plan) and runs every numeric step in HIP
 * kernels on the selected device.  There is no CPU fallback: when no HIP
 * device is usable the functions fail loudly (stderr + false / 0).
 *
 * Section 2 is the plan (handle) API the drop-ins are built on: pattern
 * resident in HBM, device pointers in / out, caller-supplied stream.
 *
 * Section 3/4 are host-side helpers (inspector, synthetic matrices) so the
 * path can be exercised without the reference's inspector.
 *
 * Plain C: pointers and sizes only, no C++ or torch types.
 */
#ifndef PARSY_AMD_H
#define PARSY_AMD_H

#include <stdbool.h>
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------ */
/* 1. Drop-in operators                                                      */
/* ------------------------------------------------------------------------ */

/* Replaces cholesky_left_par_05, reference cholesky/parallel_PB_Cholesky_05.h:27-39.
 *   n            matrix order
 *   c, r, values CSC of the LOWER triangle of P A P' (reference's A2)
 *   lC           value offset of every column of L (size n+1)          [L->p]
 *   lR           sorted row ids of every supernode (size ssize)        [L->s]
 *   Li_ptr       offset into lR for every column (size n+1)            [L->i_ptr]
 *   lValues      OUT: BCSC values (size lC[n]); must be zeroed by the caller
 *   blockSet     first column of every supernode (size supNo+1)        [L->super]
 *   timing       OUT: [0] seconds of the level-parallel phase, [1] seconds of
 *                the root phase (the GPU schedule has no separate root phase:
 *                [1] = 0), [2] device seconds of the numeric kernels only
 *   aTree        supernodal etree (-1 root)                            [L->sParent]
 *   cT, rT       CSC pattern of the UPPER triangle of P A P' (reference's A1)
 *   col2Sup      column -> supernode
 *   nLevels, levelPtr, levelSet, nPar, parPtr, partition: H-level schedule of the
 *                reference's inspector.  The factor is schedule independent; the
 *                GPU executor validates the partition (every supernode exactly
 *                once) and schedules by etree level itself.
 *   chunk, threads, super_max, col_max, nodCost: accepted for signature
 *                compatibility, unused (the reference ignores chunk/nodCost too).
 * Returns false iff a diagonal block is not positive definite (lValues is then
 * partial) or the device path could not run. */
bool cholesky_left_par_05(int n, int* c, int* r, double* values, size_t* lC, int* lR,
                          size_t* Li_ptr, double* lValues, int* blockSet, int supNo,
                          double* timing, int* aTree, int* cT, int* rT, int* col2Sup,
                          int nLevels, int* levelPtr, int* levelSet, int nPar, int* parPtr,
                          int* partition, int chunk, int threads, int super_max, int col_max,
                          double* nodCost);

/* The reference's PRUNE build of the same operator (parallel_PB_Cholesky_05.h:27-39 with
 * `#define PRUNE`, :30-34 and :120-123): the update lists are passed instead of the etree and the
 * upper pattern -- prunePtr (supNo+1) / pruneSet from getBlockedPruneSet
 * (cholesky/Inspection_Prune.h).  A C ABI cannot overload, hence the suffix. */
bool cholesky_left_par_05_prune(int n, int* c, int* r, double* values, size_t* lC, int* lR,
                                size_t* Li_ptr, double* lValues, int* blockSet, int supNo,
                                double* timing, int* prunePtr, int* pruneSet, int nLevels,
                                int* levelPtr, int* levelSet, int nPar, int* parPtr, int* partition,
                                int chunk, int threads, int super_max, int col_max, double* nodCost);

/* Replaces cholesky_left_par_waveFront, reference
 * cholesky/Parallel_PB_Cholesky_wavefront.h:10-20.  levelPtr/levelSet are etree
 * level sets (common/TreeUtils.h:119).  Like the reference it reports `true`
 * unless the device path could not run; a non-positive pivot is reported on
 * stderr only (the reference ignores LAPACK's info here, :137). */
bool cholesky_left_par_waveFront(int n, int* c, int* r, double* values, size_t* lC, int* lR,
                                 size_t* Li_ptr, double* lValues, int* blockSet, int supNo,
                                 double* timing, int* aTree, int* cT, int* rT, int* col2Sup,
                                 int nLevels, int* levelPtr, int* levelSet, int chunk,
                                 int threads, int super_max, int col_max);

/* Replace the BCSC forward solves L x = b (x in/out, one right-hand side),
 * reference triangularSolve/Triangular_BCSC.h:14 / :115 / :171 / :238.
 * Return 1 on success, 0 when Lp, Li or x is NULL (as the reference) or when
 * the device path could not run.  NNZ, col2sup and chunk are unused, as in the
 * reference.  All four run the same level-scheduled HIP solve; the level /
 * partition arrays are validated, not interpreted. */
int blockedLsolve(int n, size_t* Lp, int* Li, double* Lx, int NNZ, size_t* Li_ptr,
                  int* col2sup, int* sup2col, int supNo, double* x);
int leveledBlockedLsolve(int n, size_t* Lp, int* Li, double* Lx, int NNZ, size_t* Li_ptr,
                         int* col2sup, int* sup2col, int supNo, double* x, int levels,
                         int* levelPtr, int* levelSet, int chunk);
int H2LeveledBlockedLsolve(int n, size_t* Lp, int* Li, double* Lx, int NNZ, size_t* Li_ptr,
                           int* col2sup, int* sup2col, int supNo, double* x, int levels,
                           int* levelPtr, int* levelSet, int parts, int* parPtr,
                           int* partition, int chunk);
int H2LeveledBlockedLsolve_Peeled(int n, size_t* Lp, int* Li, double* Lx, int NNZ,
                                  size_t* Li_ptr, int* col2sup, int* sup2col, int supNo,
                                  double* x, int levels, int* levelPtr, int* levelSet,
                                  int parts, int* parPtr, int* partition, int chunk,
                                  int threads);

/* Replace the pruned BCSC forward solve, reference triangularSolve/Triangular_BCSC.h:55: L x = b for the supernodes of
 * BPSet alone (PBSetSize of them, in any order), numbered as the reference's loop reads them -- supernode i has the
 * columns sup2col[i - 1] .. sup2col[i] - 1, i = 1 .. supNo.  x is read and written only in the columns of the listed
 * supernodes.  The list must be closed towards the root of the supernodal etree, as the reach of a right-hand side
 * (common/Reach.h:31) is: the reference has no defined result for any other list, and such a list is refused.  Returns
 * 1, or 0 when Lp, Li or x is NULL (as the reference) or, loudly, when the list is refused or the device path could not
 * run.  NNZ is unused.  Runs PARSY_SPARSE_GINV (below) on a handle whose B and selected rows are those columns. */
int blockedPrunedLSolve(int n, size_t* Lp, int* Li, double* Lx, int NNZ, size_t* Li_ptr, int* BPSet, int PBSetSize,
                        int* sup2col, int supNo, double* x);

/* Drop the plans cached by the drop-in operators (frees device memory). */
void parsy_dropin_reset(void);

/* ------------------------------------------------------------------------ */
/* 2. Plan API (pattern resident on the device)                              */
/* ------------------------------------------------------------------------ */

typedef struct parsy_plan parsy_plan;
/* A plan owns scratch that its launches share (tile flags and ticket counters of the factorization; inverse
 * diagonal blocks, the hand-off vector and ticket counters of the solves): calls on ONE plan must be issued on
 * one stream, or be separated by the caller (events / synchronisation) -- one factorization or solve of a plan in
 * flight at a time.  Independent work in flight takes one plan each (plans of the same pattern are cheap next to
 * the factor: DESIGN.md, `throughput_in_flight`).  The drop-in operators of section 1 hold a per-plan mutex across
 * a call; the plan API itself is not thread-safe per plan (two host threads must not use one plan at once). */

/* Sizes and work counts of a plan (all exact, from the pattern). */
typedef struct parsy_plan_info {
    int32_t n, nsuper, nlevels, max_width, max_rows;
    int32_t n_small, n_big;        /* supernodes on the LDS-resident / tiled path */
    int32_t chol_launches;         /* kernel launches per factorization */
    int32_t solve_launches;        /* kernel launches per forward solve */
    int64_t nnzA, ssize, xsize, nnzL;
    int64_t n_updates;             /* (target, descendant) pairs */
    int64_t relpos_len;            /* relative-index entries */
    int64_t device_bytes;          /* pattern + schedule bytes resident in HBM */
    double flops_stored;           /* executed flops on the stored structure */
    double update_flops;           /* flops in the SYRK/GEMM update kernels */
    double reread_bytes;           /* left-looking re-read traffic 8*sum K*nSupRs */
    double inner_flops;            /* in-supernode SYRK/GEMM flops of the tiled path */
    double tile_update_flops;      /* external-update flops applied by the tile kernel's wave streams */
    double big_flops;              /* update flops applied by the BIG (LDS-staged GEMM) launches */
    int64_t big_entries;           /* (tile, source) pairs of the BIG launches */
    int32_t big_tasks;             /* workgroups of the BIG launches per factorization */
    int32_t n_pieces;              /* supernodes of the Cholesky view (very wide ones cut into pieces) */
    int32_t chol_levels;           /* levels of the Cholesky view's (chain-extended) etree */
    int32_t piece_width, big_min_k;
    /* subtree launches: etree subtrees of narrow supernodes walked by one workgroup each (the reference's
     * w-partitions, parallel_PB_Cholesky_05.h:66-84 / Triangular_BCSC.h:171-232) and the supernodes in them */
    int32_t chol_subtrees, chol_subtree_supernodes;
    int32_t solve_subtrees, solve_subtree_supernodes;
    int32_t backsolve_launches;    /* kernel launches per backward solve */
    int32_t dense_tasks;           /* workgroups of the DENSE launches (k_chol_dense) per factorization */
    double dense_flops;            /* part of big_flops in dense entries (full 128 x 128 blocks below the diagonal): k_chol_dense */
    int64_t dense_entries;
    int32_t solve_one;             /* a small plan -- blocks of at most 8 right-hand sides are solved in ONE launch instead of
                                    * one per level (k_solve_one / k_bsolve_one): bit 0 the forward, bit 1 the backward solve;
                                    * bit 2: the subtree launch of the narrow supernodes stays beside it */
    int32_t solve_one_blocks;      /* block columns (workgroups) of the forward ONE launch */
    int32_t sub_mrhs_trees;        /* subtrees of the solves' subtree launch for many right-hand sides (one wave per subtree and
                                    * 16 right-hand sides, the subtree's traffic in LDS); 0: that form is not available */
    int32_t sub_mrhs_slots;        /* ... and the LDS slots (16 right-hand sides each) of the largest */
    int32_t sub_mrhs_tiers;        /* launches of that form per solve: the subtrees at the bottom of the etree, then bands of levels */
    int32_t sub_mrhs_cover_level;  /* ... which replace every level launch up to this etree level (-1: only the subtree launch) */
    int64_t dense_strip_entries;   /* dense entries that carry the remainder of their source's row / column run (<= 16 rows behind
                                    * or beside the block), multiplied with the block's staged operands */
    int32_t split_tiles;           /* tiles whose early wave stream is split: separate workgroups apply its parts to partial tiles
                                    * (tile scratch), summed in a fixed order when the chain launch loads the tile */
    int32_t split_parts;           /* ... and the sum of their parts (>= 2 each) */
} parsy_plan_info;

/* Build a plan from the reference-shaped symbolic arrays (host pointers, copied).
 * device < 0 builds the host schedule only (no HIP call; for CPU-side tests).
 * Returns NULL on error (see parsy_last_error). */
parsy_plan* parsy_plan_create(int n, int supNo, const int* blockSet, const size_t* lC,
                              const size_t* Li_ptr, const int* lR, const int* aTree,
                              const int* col2Sup, const int* cT, const int* rT, const int* c,
                              const int* r, int device);
void parsy_plan_destroy(parsy_plan* plan);
int parsy_plan_get_info(const parsy_plan* plan, parsy_plan_info* info);

/* Restrict the work of the NEXT factor/solve calls to a set of supernodes
 * (multi-GPU: the subtrees this rank owns, or the root part).  mask has one
 * byte per supernode (non-zero = process).  NULL restores "all". Rebuilds the
 * launch schedule; not meant for the timed region. */
int parsy_plan_set_active(parsy_plan* plan, const uint8_t* mask);
/* Host-side dry run of the factorization's in-launch hand-offs (tiles of the wide supernodes are
 * passed between workgroups inside one launch per etree level) with `slots` resident workgroups:
 * returns the number of tiles that would never be finished -- 0 means the schedule cannot
 * deadlock at that residency -- or -1 for a bad argument.  The kernel runs 2 workgroups per CU. */
long long parsy_plan_chain_check(const parsy_plan* plan, int slots);
/* Host-side consistency check of the plan's schedules -- factorization: pieces, levels, windows of the update
 * entries, exact cover of every (target, descendant) update, subtree launches, launch order; solves: every active
 * supernode / chunk / block column solved exactly once in each direction, subtree runs in order, width classes,
 * the backward chain's groups --: number of violations, 0 = consistent (parsy_last_error describes the first
 * one).  For tests and for callers that build plans from their own arrays. */
long long parsy_plan_check(const parsy_plan* plan);

/* Numeric factorization, everything on the device.
 *   d_values  device, nnz(A2) doubles (same order as the host `values`)
 *   d_lValues device, xsize doubles; zeroed and overwritten
 *   stream    hipStream_t (NULL = default stream); the call is asynchronous
 * Returns 0 when the launches were enqueued, <0 on a HIP error. */
int parsy_factor_device(parsy_plan* plan, const double* d_values, double* d_lValues,
                        void* stream);
/* As parsy_factor_device with flags: PARSY_FACTOR_NO_INIT skips the zero-fill and the
 * A scatter (multi-GPU: the root-part pass on a buffer that already holds A and the
 * gathered subtree panels). */
#define PARSY_FACTOR_NO_INIT 1
int parsy_factor_device_ex(parsy_plan* plan, const double* d_values, double* d_lValues,
                           void* stream, int flags);
/* After the stream has been synchronised: 0 = factor ok, k > 0 = first
 * non-positive pivot seen at (1-based) column k, as LAPACK's dpotrf info. */
int parsy_factor_status(parsy_plan* plan);

/* ---- Level-by-level factorization and the pieces of the Cholesky view -------------------------------
 * The factorization runs on the "Cholesky view" of the pattern: the supernodes, with the very wide ones
 * cut into pieces (column ranges of one panel) that are factored one after the other; its etree levels are the
 * wavefronts of cholesky_left_par_waveFront (Parallel_PB_Cholesky_wavefront.h:28-45: one level at a time).
 * A caller that has work of its own between two levels -- the exchange step of a multi-device run -- enqueues
 * the levels one by one:  parsy_factor_begin, parsy_factor_level(0 .. chol_levels-1, ascending, no gaps),
 * parsy_factor_end; parsy_factor_device is exactly that sequence.  Everything is asynchronous on `stream`. */
int parsy_factor_begin(parsy_plan* plan, const double* d_values, double* d_lValues, void* stream, int flags);
int parsy_factor_level(parsy_plan* plan, int level, double* d_lValues, void* stream);
int parsy_factor_end(parsy_plan* plan, void* stream);
/* The pieces (n_pieces of parsy_plan_info; any output array may be NULL): supernode, level in the Cholesky
 * view, first column, width, rows (from the piece's diagonal down), and the range [value_begin, value_end) of
 * lValues that holds the piece's columns (column-major with the leading dimension of its supernode). Returns
 * the number of pieces. */
int parsy_plan_pieces(const parsy_plan* plan, int32_t* supernode, int32_t* level, int32_t* col0, int32_t* width,
                      int32_t* rows, int64_t* value_begin, int64_t* value_end);
/* As parsy_plan_set_active for the factorization, at the granularity of pieces (one byte per piece); the
 * solves keep the supernode mask.  NULL restores "all". */
int parsy_plan_set_active_pieces(parsy_plan* plan, const uint8_t* piece_mask);

/* ---- Distribution of one factorization over the devices of a node (host logic) -----------------------
 * Below a cut whole etree subtrees go to one rank each (independent: a target only reads its descendants,
 * common/Reach.h:122-135 -- the independence of the reference's w-partitions, InspectionLevel_06.h:196-217;
 * packed heaviest first, cf. common/TreeUtils.h:217-255); above it the pieces are dealt over the ranks level
 * by level.  The owner of a piece applies every update into it; after a level is complete each of its pieces
 * travels to the ranks that own a target it updates (only the rows those targets read).  The messages are
 * lists of (offset, length) segments of lValues, the same on the sending and the receiving side. */
typedef struct parsy_dist parsy_dist;
typedef struct parsy_dist_info {
    int32_t nranks, nlevels, n_pieces, n_subtrees, n_root_pieces, n_messages;
    int64_t exchange_elements;        /* doubles that travel per factorization, all messages */
    double total_cost, root_cost;     /* flops: whole job / pieces above the cut */
    double max_rank_cost;             /* the most loaded rank */
    double lockstep_cost;             /* sum over levels of the most loaded rank of that level */
} parsy_dist_info;
/* block: consecutive pieces of one split supernode that stay on one rank (<= 0: the default, 2). The plan may be
 * a host-only one (device < 0). */
parsy_dist* parsy_dist_create(const parsy_plan* plan, int nranks, int block);
void parsy_dist_destroy(parsy_dist* dist);
int parsy_dist_get_info(const parsy_dist* dist, parsy_dist_info* info);
/* owner[n_pieces]; in_subtree[n_pieces] (1: the piece lies below the cut, in a subtree that went to one rank as a
 * whole; 0: above it); rank_cost[nranks]; level_cost[nlevels * nranks] (any may be NULL) */
int parsy_dist_get(const parsy_dist* dist, int32_t* owner, uint8_t* in_subtree, double* rank_cost,
                   double* level_cost);
/* Messages that follow level `level`: their number; message `index` of them (borrowed pointers, valid until
 * the dist is destroyed): sender, receiver, number of segments, elements of the packed buffer, and per segment
 * its offset in lValues, its length and its offset in the packed buffer. */
int parsy_dist_level_messages(const parsy_dist* dist, int level);
int parsy_dist_message(const parsy_dist* dist, int level, int index, int32_t* src, int32_t* dst, int64_t* nseg,
                       int64_t* total, const int64_t** off, const int32_t** len, const int64_t** packed);
/* Host-side consistency check (every update across ranks finds its source rows delivered right after the
 * source's level; subtrees walked by one workgroup stay on one rank): number of violations. */
long long parsy_dist_check(const parsy_plan* plan, const parsy_dist* dist);

/* Forward solve L X = B in place, X is n x nrhs column-major with leading
 * dimension ldx (device pointers). Asynchronous on `stream`. */
int parsy_solve_device(parsy_plan* plan, const double* d_lValues, double* d_x, int nrhs,
                       int ldx, void* stream);

/* After the stream has been synchronised: 0 = the last forward / backward solve on this plan completed,
 * -1 = a hand-off wait inside one of its chain launches timed out (internal error; x is not the solution).
 * The host conveniences and the drop-in solves check it themselves and fail loudly. */
int parsy_solve_status(parsy_plan* plan);

/* Backward solve L' X = Y in place (same layout as parsy_solve_device).  Not part of the
 * reference (it only has the forward solve): forward + backward solve A x = b
 * for the permuted system, x = P' L'^-1 L^-1 P b. Asynchronous on `stream`. */
int parsy_backsolve_device(parsy_plan* plan, const double* d_lValues, double* d_x, int nrhs, int ldx,
                           void* stream);
/* A forward / backward solve in STEPS of etree levels (triangularSolve/Triangular_BCSC.h:115-164: one level set at a time):
 * the level launches of the plan's active supernodes (parsy_plan_set_active) whose etree level lies in
 * [level_begin, level_end).  A solve that is distributed above the cut puts its exchange steps between two calls, as
 * parsy_factor_level does for the factorization.  flags: */
/* The etree level of every supernode (nsuper entries; NULL: only the count) as the solves' launches go by it; returns the
 * number of levels.  A supernode's rows below its own columns belong to supernodes of higher levels. */
int parsy_plan_solve_levels(const parsy_plan* plan, int32_t* level);
#define PARSY_SOLVE_FIRST 1     /* the first step of a solve: status word, hand-off buffer, inverse diagonal blocks */
#define PARSY_SOLVE_LAST 2      /* the last step */
#define PARSY_SOLVE_BACKWARD 4  /* L' x = y (the steps then go from the root level down) */
/* X keeps the caller's layout (n x nrhs, leading dimension ldx); asynchronous on `stream`; parsy_solve_status as usual. */
int parsy_solve_levels_device(parsy_plan* plan, const double* d_lValues, double* d_x, int nrhs, int ldx, void* stream,
                              int level_begin, int level_end, int flags);
/* d_b = L * 1 on the stored structure (device pointers, n doubles, overwritten): the right-hand side the
 * reference's triangularTest solves (rhsInitBlocked, common/Util.h:277-288), so that L x = b has x = 1. */
int parsy_rhs_ones_device(parsy_plan* plan, const double* d_lValues, double* d_b, void* stream);
/* Device helper of the multi-GPU exchange: d_dst[dst_off[q] + i] = d_src[src_off[q] + i], i < len[q], for nseg
 * contiguous runs (all pointers device pointers).  Packs the panel rows of a subtree that the root part
 * reads into one send buffer, and unpacks them on the receiving rank. Asynchronous on `stream`. */
int parsy_copy_segments_device(double* d_dst, const double* d_src, const int64_t* d_dst_off,
                               const int64_t* d_src_off, const int32_t* d_len, int64_t nseg, void* stream);
/* Host convenience: forward (if `forward` != 0) then backward solve on host buffers. */
int parsy_solve2_host(parsy_plan* plan, const double* lValues, double* x, int nrhs, int ldx,
                      int forward, double* seconds);

/* ---- A x = b in the caller's ordering: residuals, backward errors, iterative refinement ---------------
 * The plan holds P A P' (A2 order, lower triangle); these calls take and return vectors in the caller's ordering
 * and refine with LAPACK dporfs's loop, column by column: r = Pb - A z, berr = max_i |r_i| / (|A||z| + |Pb|)_i
 * (with dporfs's safe1 / safe2 guards), then z += (L L')^-1 r while berr > 2^-53, berr halved at least, and fewer
 * than max_steps steps were taken.  The residual is FP64 and bitwise reproducible.  The values may differ from the
 * values that were factored (a stale factor of nearby values): refinement then stops on the halving test.  Refused:
 * host-only and solve-only plans, plans under parsy_plan_set_active / _set_active_pieces, an open factorization or
 * level-stepped solve, nrhs < 1, a leading dimension < n, NULL pointers.  Return 0, or < 0 with parsy_last_error. */
/* The ordering of the caller's A: perm[new] = old, n entries (host, copied; refused unless a permutation of 0..n-1);
 * NULL = identity (the default: plans from parsy_plan_create already hold the permuted system). */
int parsy_plan_set_perm(parsy_plan* plan, const int* perm);
/* R = B - A X and the componentwise backward error of every column (device pointers, d_values in A2 order as
 * parsy_factor_device takes them).  d_r may be NULL; berr (host, nrhs) may be NULL; a non-NULL berr synchronises
 * `stream`. */
int parsy_residual_device(parsy_plan* plan, const double* d_values, const double* d_x, int ldx, const double* d_b,
                          int ldb, double* d_r, int ldr, int nrhs, double* berr, void* stream);
/* X = A^-1 B with up to max_steps refinement steps.  d_x may equal d_b when ldx == ldb.  steps / berr: host, nrhs
 * entries each, may be NULL; berr is the backward error of the returned X.  With max_steps > 0 the call synchronises
 * `stream` once per step (and fails, X untouched, when a solve's hand-off wait timed out); with max_steps == 0 and
 * both NULL it is fully asynchronous (check parsy_solve_status). */
int parsy_solve_spd_device(parsy_plan* plan, const double* d_values, const double* d_lValues, const double* d_b,
                           int ldb, double* d_x, int ldx, int nrhs, int max_steps, int32_t* steps, double* berr,
                           void* stream);
/* Host-buffer convenience (H2D, the call above, D2H); seconds = device time of the call above. */
int parsy_solve_spd_host(parsy_plan* plan, const double* values, const double* lValues, const double* b, int ldb,
                         double* x, int ldx, int nrhs, int max_steps, int32_t* steps, double* berr, double* seconds);

/* ---- Forward error bounds and a condition estimate of the SPD solve ---------------------------------------------
 * The companions of the backward error above, as LAPACK has them: dporfs's FERR, a bound on
 * ||x - x_true||_inf / ||x||_inf for every right-hand side, and dpocon's reciprocal condition number.  Both rest on
 * Higham's 1-norm estimator (dlacn2), run on the device for all columns at once with the factor as the operator:
 *   FERR_q  = est || |A^-1| w_q ||_inf / ||x_q||_inf,  w = |r| + nz eps (|A||x| + |b|)  (nz = most entries of a row + 1,
 *             eps = 2^-53, dporfs's safe1 added where |A||x| + |b| <= safe2),
 *   RCOND   = 1 / (||A||_1 est ||A^-1||_1)  (0 when the estimate is 0).
 * Every column advances in lockstep through many-right-hand-side solves: a call enqueues at most 11 forward + backward
 * solve pairs whatever nrhs is (dlacn2's 1 + 1 + 4 x 2 + 1 applications), and synchronises `stream` once per pair.  A
 * column that finishes early rides along with a zero operand.  Given the same solve results the estimates are bitwise
 * reproducible (fixed reduction orders, no float atomics).  An estimate is a lower bound of the quantity it estimates,
 * in practice within a factor 3 of it and usually exact to rounding.
 * STALE FACTOR: the operator of both estimates is (L L')^-1, the inverse of the matrix that was FACTORED; anorm, the
 * residual r and the weights w come from `values`.  When `values` differ from the factored values, FERR bounds the
 * error only as far as (L L')^-1 stands for A^-1 (to first order in the difference), and RCOND is
 * 1 / (||A||_1 ||(L L')^-1||_1): the numbers describe the factored matrix.
 * A non-finite estimate is returned as NaN with return value 0.  Refused, with parsy_last_error set and the outputs
 * untouched: what the refinement calls refuse, nrhs > 65535, and a solve whose hand-off wait timed out.  The first call
 * allocates its workspace (two n x nrhs vectors, a byte per entry for the saved signs, the column states) and adds it to
 * the plan's device_bytes. */
typedef struct parsy_cond_info {
    int32_t applications;   /* solve pairs (forward + backward) the last bounds / rcond call enqueued */
    int32_t columns;        /* right-hand sides of that call (1 for rcond) */
    int64_t device_bytes;   /* workspace held by this feature (0 before the first device call) */
} parsy_cond_info;
int parsy_cond_get_info(parsy_plan* plan, parsy_cond_info* info);      /* host-only plans too */
/* BERR and FERR of a given X (caller's ordering, as parsy_residual_device takes it).  ferr / berr: host, nrhs entries,
 * either may be NULL (both NULL is refused).  Synchronises stream. */
int parsy_error_bounds_device(parsy_plan* plan, const double* d_values, const double* d_lValues, const double* d_x,
                              int ldx, const double* d_b, int ldb, int nrhs, double* ferr, double* berr, void* stream);
/* parsy_solve_spd_device with FERR of the returned X (taken from the vectors the refinement ends with: no second
 * permutation in).  ferr == NULL: exactly parsy_solve_spd_device. */
int parsy_solve_spd_bounds_device(parsy_plan* plan, const double* d_values, const double* d_lValues, const double* d_b,
                                  int ldb, double* d_x, int ldx, int nrhs, int max_steps, int32_t* steps, double* berr,
                                  double* ferr, void* stream);
int parsy_solve_spd_bounds_host(parsy_plan* plan, const double* values, const double* lValues, const double* b, int ldb,
                                double* x, int ldx, int nrhs, int max_steps, int32_t* steps, double* berr, double* ferr,
                                double* seconds);
/* dpocon: *anorm = ||A||_1 of `values`, *rcond = 1 / (anorm * est ||(L L')^-1||_1).  Either may be NULL, not both (with
 * rcond NULL no solve is enqueued).  Host pointers; synchronises stream. */
int parsy_rcond_device(parsy_plan* plan, const double* d_values, const double* d_lValues, double* anorm, double* rcond,
                       void* stream);
int parsy_rcond_host(parsy_plan* plan, const double* values, const double* lValues, double* anorm, double* rcond,
                     double* seconds);

/* ---- The smallest eigenpairs of A v = lambda M v, through the factor -----------------------------------------------
 * The k lowest eigenvalues of the pencil (A, M), A and M symmetric positive definite on the plan's pattern, and their
 * eigenvectors: a block Davidson iteration with (L L')^-1 as preconditioner and a thick restart, the basis held on the
 * device (at most max_basis <= 128 columns; V, A V and M V side by side: 3 n max_basis doubles, 2 n max_basis with
 * M = I, plus a few n x 16 blocks).
 *   d_values, d_mvalues  A's and M's values in A2 order, as parsy_factor_device takes them; M lives on the pattern of A,
 *                        absent entries are stored zeros; d_mvalues NULL: M = I.
 *   d_x0, ldx0, block    the start block, n x block column-major in the caller's ordering (parsy_plan_set_perm), as
 *                        parsy_residual_device takes vectors; 1 <= block <= 16 is also the number of columns a step
 *                        adds.  The library holds no random number generator: the same x0 gives the same bits.
 *   lambda, resid        host, k entries: the eigenvalues ascending and eta_i = ||A y_i - lambda_i M y_i||_inf /
 *                        ((||A||_inf + |lambda_i| ||M||_inf) ||y_i||_inf), the normwise backward error of the pair,
 *                        computed from the RETURNED vectors by fresh products with `values` (not from kept quantities).
 *   d_y, ldy             k columns, M-orthonormal, caller's ordering.
 *   *nconv               host: the returned pairs with resid <= tol.
 * Returns 0 when the loop ran: *nconv < k after max_iter iterations is not an error, the other pairs are the current
 * Ritz pairs with their true eta (a pair the basis does not hold yet -- fewer than k columns after max_iter steps --
 * comes back as lambda = NaN, resid = +inf and a zero column).  With *nconv == k every resid[i] <= tol.  -1: a refusal, a
 * HIP error or a solve whose hand-off wait timed out.  -2: the Gram matrix of a block is not positive definite beyond
 * the drop rule, which means M is not SPD; parsy_last_error names the iteration.
 * Each step takes two projections against the basis and two passes of Cholesky-QR in the M inner product; in the first
 * the Gram matrix is scaled to unit diagonal and a column whose pivot falls below 2^-26 is dropped (counted in
 * `dropped`); if every column of a block is dropped the call ends as unconverged.
 * STALE FACTOR: the expansion is (L L')^-1 (A y - theta M y), the residual of `values`, so lValues may be the factor of
 * nearby values or of A - sigma M with sigma below the spectrum: the eigenpairs returned are those of `values` and
 * d_mvalues, the factor only sets the number of iterations.
 * Refused up front, with parsy_last_error set and the outputs untouched: what parsy_residual_device refuses; k < 1,
 * block < 1, block > 16; max_basis > 128, > n or < k + 2 block (max_basis == 0: max(3 k, k + 4 block) clipped to
 * min(n, 128), refused when that is below k + 2 block); max_iter < 1; tol < (max_row + 1) 2^-52 (max_row: most entries
 * in a row of A), which an FP64 residual cannot show; a leading dimension < n; NULL pointers other than d_mvalues.
 * SYNCHRONISATION: the small dense work -- a Jacobi eigensolver of the projected matrix, a Cholesky factor of a block's
 * Gram matrix -- runs on the host: the stream is waited for four times per iteration (the projected matrix, the eta
 * of the k wanted pairs, the Gram matrix of each Cholesky-QR pass), once more at a restart and before the returned pairs
 * are formed (V'MV, which squares the rotation up), and the call returns with the stream idle.
 * The feature's own kernels sum in fixed orders without atomics: given the same solve results the outputs are bitwise
 * reproducible (the many-right-hand-side solves of a plan with wide supernodes add with float atomics and are not, as
 * for the estimates above).  The first call allocates the workspace and
 * adds it to the plan's device_bytes; it grows with max_basis. */
typedef struct parsy_eigs_info {
    int32_t iterations;     /* of the last call: expansions of the basis */
    int32_t restarts;
    int32_t nconv;
    int32_t basis;          /* columns of V at return */
    int32_t dropped;        /* columns the drop rule removed */
    int32_t reserved;
    int64_t solve_columns;  /* right-hand sides sent through forward + backward solve pairs */
    int64_t device_bytes;   /* workspace held by this feature (0 before the first device call) */
} parsy_eigs_info;
int parsy_eigs_get_info(parsy_plan* plan, parsy_eigs_info* info);      /* host-only plans too */
int parsy_eigs_device(parsy_plan* plan, const double* d_values, const double* d_mvalues, const double* d_lValues, int k,
                      const double* d_x0, int ldx0, int block, double tol, int max_basis, int max_iter, double* lambda,
                      double* d_y, int ldy, double* resid, int32_t* nconv, void* stream);
/* Host buffers: H2D, the call above, D2H; seconds (may be NULL) = device time.  Synchronous. */
int parsy_eigs_host(parsy_plan* plan, const double* values, const double* mvalues, const double* lValues, int k,
                    const double* x0, int ldx0, int block, double tol, int max_basis, int max_iter, double* lambda,
                    double* y, int ldy, double* resid, int32_t* nconv, double* seconds);

/* ---- Selected inversion: entries of A^-1 on the pattern of L, and log det A -------------------------------------
 * Z = (P A P')^-1 on the stored pattern of L by the Takahashi recurrences, level by level from the root of the tree of
 * the block columns (at most 64 columns of a supernode each).  Two kernel paths: a tiled one (FP64 MFMA, one workgroup
 * per 64-row tile of a block column's rows below it) and a small one (one workgroup per block column) for block columns
 * with fewer than PARSY_SELINV_TILED_MIN rows below them (read at every call).  No float atomics: Z, the diagonal and the
 * log-determinant are bitwise reproducible.  The device calls refuse host-only and solve-only plans, plans under
 * parsy_plan_set_active / _set_active_pieces, an open factorization or level-stepped solve and NULL pointers, with
 * parsy_last_error set and the outputs untouched.  A plan that never calls them allocates nothing for them; the first
 * call allocates the gather map and the scratch and adds them to the plan's device_bytes. */
typedef struct parsy_selinv_info {
    int32_t levels;               /* depth of the block-column tree = level steps per call */
    int32_t block_columns;        /* sum over supernodes of ceil(w / 64) */
    int32_t tiled_block_columns;  /* of those, on the tiled path under the current threshold */
    int32_t launches;             /* kernel launches per parsy_selinv_device call */
    double  flops;                /* sum_b 2 |R_b|^2 w_b + 4 |R_b| w_b^2 (the products Z Y, L T, Y' Z) */
    int64_t device_bytes;         /* map + scratch held once built (0 before the first device call) */
} parsy_selinv_info;
int parsy_selinv_get_info(parsy_plan* plan, parsy_selinv_info* info);   /* host-only plans too */
/* Violations of the schedule (every block column scheduled once, below its parent; every gather position holds the
 * row it stands for); parsy_last_error describes the first.  Host-only plans too. */
long long parsy_selinv_check(const parsy_plan* plan);
/* Z = (P A P')^-1 on the pattern of L, in lValues' layout (xsize doubles, overwritten; the strict upper part of every
 * diagonal block is 0).  d_z must not overlap d_lValues.  Asynchronous on stream after the first call. */
int parsy_selinv_device(parsy_plan* plan, const double* d_lValues, double* d_z, void* stream);
/* d_diag[perm[i]] = Z(i, i): diag(A^-1) in the caller's ordering (parsy_plan_set_perm; identity by default). */
int parsy_inverse_diag_device(parsy_plan* plan, const double* d_z, double* d_diag, void* stream);
/* Host buffers: H2D, the two calls above, D2H; diag may be NULL; seconds = device time. */
int parsy_selinv_host(parsy_plan* plan, const double* lValues, double* z, double* diag, double* seconds);
/* log det A = 2 sum log L_jj into *logdet (host; synchronises stream).  Returns 0; k > 0: the first (1-based, plan
 * ordering) column whose diagonal entry is not positive and finite, *logdet = NaN; < 0: error. */
int parsy_logdet_device(parsy_plan* plan, const double* d_lValues, double* logdet, void* stream);

/* ---- Gradients with respect to the values of A ---------------------------------------------------------------------
 * Conventions.  `values` is what parsy_factor_device takes: the lower triangle of P A P' in A2 order, nnzA entries; entry
 * q sits at the permuted position (i_q, j_q), i_q >= j_q.  SYMMETRIC PARAMETERISATION: a stored off-diagonal value stands
 * for both A_ij and A_ji, so every gradient with respect to values[q] counts both occurrences: w_q = 2 when i_q != j_q,
 * w_q = 1 on the diagonal.  Vectors (x, lambda) are in the caller's ordering under parsy_plan_set_perm (identity by
 * default), column-major with a leading dimension, exactly as parsy_residual_device takes X.  Outputs `g` hold nnzA
 * doubles in A2 order.  Every sum runs in a fixed order with no atomics: results are bitwise reproducible from call to
 * call.  The device calls refuse host-only and solve-only plans, NULL pointers and bad sizes with parsy_last_error set
 * and the outputs untouched; they take no part in the factorization's or the solves' state, so they may run on a plan
 * whatever else is open on it.  Like every call on a plan they belong on ONE stream per plan: the staging workspace of
 * parsy_pattern_outer_device and the partials of parsy_trace_inverse_device are per plan and not synchronised, so two
 * such calls of one plan on different streams must be ordered by the caller.  A plan that never calls them allocates nothing for them; the first device call uploads
 * the pattern's coordinates (8 nnzA bytes) and adds them, and any workspace, to the plan's device_bytes. */
/* The pattern of A as the plan sees it: row[q] = i_q, col[q] = j_q (permuted coordinates), dst[q] = the offset of the
 * entry in lValues / Z (where the factorization scatters values[q]).  Any pointer may be NULL; returns nnzA (< 0: error).
 * Host-only plans too. */
int64_t parsy_plan_pattern(const parsy_plan* plan, int32_t* row, int32_t* col, int64_t* dst);
typedef struct parsy_grad_info {
    int64_t entries;           /* nnzA */
    int64_t offdiag_entries;   /* of those, i_q != j_q */
    int64_t device_bytes;      /* coordinates + workspaces held (0 before the first device call) */
    int32_t last_lanes;        /* lanes per entry of the last parsy_pattern_outer_device call: 0 none yet, 1 the direct
                                * kernel, 8 / 16 / 32 / 64 the many-right-hand-side kernel */
} parsy_grad_info;
int parsy_grad_get_info(parsy_plan* plan, parsy_grad_info* info);   /* host-only plans too */
/* g[q] = beta g[q] + alpha S_q,  S_q = sum_k lambda[i,k] x[j,k] + lambda[j,k] x[i,k]  (i != j),
 *                                S_q = sum_k lambda[i,k] x[i,k]                       (i == j):
 * S_q = d(lambda' A x) / d values[q].  With lambda = A^-1 w and alpha = -1 this is the gradient of w' x, x = A^-1 b,
 * with respect to the values.  With beta == 0, g is not read (it may hold NaN).  Two kernels, chosen per call: fewer
 * right-hand sides than PARSY_GRAD_MRHS_MIN (default 5, read at every call) take one thread per entry; from there on
 * the vectors are staged with the right-hand sides of a row contiguous (workspace of 2 n pitch doubles, pitch = nrhs
 * rounded up to 8, grown on demand) and 8 / 16 / 32 / 64 lanes share an entry.  Asynchronous on `stream`. */
int parsy_pattern_outer_device(parsy_plan* plan, const double* d_lambda, int ldl, const double* d_x, int ldx, int nrhs,
                               double alpha, double beta, double* d_g, void* stream);
/* g[q] = beta g[q] + alpha w_q Z[dst[q]] for Z as parsy_selinv_device leaves it; PARSY_PATTERN_PLAIN in flags sets
 * w_q = 1 (the entries of (P A P')^-1 themselves).  alpha = 1, beta = 0 gives d log det A / d values, bit for bit a copy
 * or a doubling of Z's entries.  Asynchronous on `stream`. */
#define PARSY_PATTERN_PLAIN 1
int parsy_inverse_pattern_device(parsy_plan* plan, const double* d_z, double alpha, double beta, int flags, double* d_g,
                                 void* stream);
/* out[m] = tr(A^-1 B_m) = sum_q w_q Z[dst[q]] B_m[q], m < nb, for symmetric matrices B_m on A's pattern given as the
 * columns (leading dimension ldb >= nnzA) of d_bvalues in A2 order: the derivative of log det A along B_m.  out: host,
 * nb doubles; the call synchronises `stream`.  Two passes with fixed ranges and a fixed tree. */
int parsy_trace_inverse_device(parsy_plan* plan, const double* d_z, const double* d_bvalues, int64_t ldb, int nb,
                               double* out, void* stream);
/* Host buffers: H2D, the call above, D2H; seconds (may be NULL) = device time.  z as parsy_selinv_host returns it. */
int parsy_pattern_outer_host(parsy_plan* plan, const double* lambda, int ldl, const double* x, int ldx, int nrhs,
                             double alpha, double beta, double* g, double* seconds);
int parsy_inverse_pattern_host(parsy_plan* plan, const double* z, double alpha, double beta, int flags, double* g,
                               double* seconds);

/* ---- The factor as an operator: products with L and L', Gaussian samples ------------------------------------------
 * With the plan's ordering P (parsy_plan_set_perm: perm[new] = old, identity when unset) and G = P' L we have G G' = A, so
 * x = mu + G z draws from N(mu, A), x = mu + G^-T z from N(mu, A^-1), G^-1 (x - mu) whitens and ||G^-1 r||^2 is the
 * Mahalanobis form.  One entry point applies the four operators to the nrhs columns of X (column-major, leading
 * dimension ldx >= n) in the caller's ordering:
 *     PARSY_OP_G      Y = beta Y + alpha P' L X          PARSY_OP_GT      Y = beta Y + alpha L' P X
 *     PARSY_OP_GINV   Y = beta Y + alpha L^-1 P X        PARSY_OP_GINVT   Y = beta Y + alpha P' L^-T X
 * With beta == 0, Y is not read (it may hold NaN).  Only the first n rows of each column of Y are written; X is not
 * changed; X and Y must be different arrays.  d_lValues may hold any values on the pattern of L; the strict upper
 * triangle of a supernode's diagonal block is never read.
 * The two products are kernels of their own with no floating-point atomics: a call repeated gives the same bits, and
 * column q of a call with nrhs columns is bitwise what the call with that column alone gives, for any leading
 * dimensions.  They pass over lValues once per block of block_columns right-hand sides and hold a workspace of
 * workspace_bytes for one block, the transpose of the row lists (row -> its positions in lR) and their task lists on the
 * device; all of it is made by the first device call and counted in the plan's device_bytes.
 * The two inverse operators permute into an n x nrhs workspace, run parsy_solve_device / parsy_backsolve_device on it
 * unchanged and write out; their status is the solves' (parsy_solve_status after the stream is synchronised).
 * Refusals (parsy_last_error names each; nothing is written): a NULL argument, nrhs < 1, ldx < n or ldy < n, op outside
 * 0 .. 3, X and Y the same array, a host-only plan.  One stream per plan, as for every call on a plan. */
enum { PARSY_OP_G = 0, PARSY_OP_GT = 1, PARSY_OP_GINV = 2, PARSY_OP_GINVT = 3 };
int parsy_factor_apply_device(parsy_plan* plan, const double* d_lValues, int op, const double* d_x, int ldx, int nrhs,
                              double alpha, double beta, double* d_y, int ldy, void* stream);
/* Host buffers: H2D, the call above, D2H; seconds (may be NULL) = device time.  Synchronous; for the inverse operators a
 * bad solve status fails the call and leaves y untouched. */
int parsy_factor_apply_host(parsy_plan* plan, const double* lValues, int op, const double* x, int ldx, int nrhs,
                            double alpha, double beta, double* y, int ldy, double* seconds);
typedef struct parsy_apply_info {
    int32_t rows;              /* n */
    int32_t max_occurrences;   /* most panels a row appears in */
    int64_t occurrences;       /* entries of the row lists (ssize) */
    int32_t block_columns;     /* right-hand sides per pass over lValues */
    int32_t last_op;           /* op of the last device call (-1: none yet) */
    int32_t last_launches;     /* kernels it enqueued (besides the solve's own for the inverse operators) */
    int32_t reserved;
    int64_t workspace_bytes;   /* workspace of the products for one block of right-hand sides (known on the host) */
    int64_t device_bytes;      /* index, task lists and workspaces held (0 before the first device call) */
} parsy_apply_info;
int parsy_factor_apply_get_info(parsy_plan* plan, parsy_apply_info* info);          /* host-only plans too */
/* The transpose of the row lists: the positions k of lR with lR[k] == row are pos[ptr[row]] .. pos[ptr[row + 1] - 1],
 * ascending; ptr holds n + 1 entries, pos ssize.  Host-only plans too. */
int parsy_factor_apply_row_index(const parsy_plan* plan, int64_t* ptr, int64_t* pos);

/* ---- Update and downdate of the factor: A + W W' and A - W W' without a refactorization ------------------------------
 * W is a sparse n x k matrix (k >= 0) in compressed columns in the caller's ordering: wp (k + 1 entries) and wi (row
 * indices, strictly ascending within a column) on the host, the values on the device.  Its rows go through the plan's
 * ordering (parsy_plan_set_perm).  The call turns d_lValues, the factor of P A P', into the factor of P (A + sign W W') P'
 * by one rotation per (column of L, column of W) pair, columns of L ascending:
 *     r = sqrt(d^2 + sign w^2), c = r / d, s = w / d with d = L_jj, w = W_jt;  L_jj = r, W_jt = 0, and below the diagonal
 *     L_ij = (L_ij + sign s W_it) / c,  W_it = c W_it - s L_ij.
 * Only the supernodes on the etree paths above the first row j_t (factor's ordering) of each column t of W are read and
 * written, each panel once per block of 8 columns of W; everything else of d_lValues keeps its bits, the strict upper
 * triangles of the diagonal blocks are neither read nor written, and d_wx is not changed.
 * THE PATTERN OF L DOES NOT CHANGE: a column t with a non-zero outside the structure of column j_t of L (the row list of
 * j_t's supernode from j_t on) is refused, on the host, before anything is enqueued; the message names the column and the
 * row.  Further refusals (parsy_last_error names each; nothing is written): a NULL argument with k > 0, sign other than
 * +1 / -1, k < 0, a row index outside 0 .. n - 1, indices unsorted or repeated within a column, a plan restricted by
 * parsy_plan_set_active / _set_active_pieces, a host-only plan.  k == 0 and empty columns are no-ops.
 * A pivot with r^2 <= 0 or not finite (a downdate that leaves the matrix indefinite) is reported by parsy_updown_status
 * after the stream is synchronised: 0, or the first such column, 1-based, in the factor's ordering (-1: the plan has no
 * device, as parsy_factor_status).  Its rotation is
 * left out, so no NaN spreads, but d_lValues is then NO LONGER A FACTOR of anything; the plan stays usable (factor
 * again).  The caller's values of A are not touched: whoever refines afterwards supplies the values of A + sign W W'.
 * The call uploads W's pattern and waits for the stream once before it enqueues; kernels are ordered by the stream alone.
 * The first device call makes an n x 8 workspace, counted in the plan's device_bytes. */
int parsy_factor_updown_device(parsy_plan* plan, double* d_lValues, int sign, int k, const int* wp, const int* wi,
                               const double* d_wx, void* stream);
/* Host buffers: H2D, the call above, D2H; seconds (may be NULL) = device time.  Synchronous. */
int parsy_factor_updown_host(parsy_plan* plan, double* lValues, int sign, int k, const int* wp, const int* wi,
                             const double* wx, double* seconds);
int parsy_updown_status(parsy_plan* plan);
/* The supernodes the call above would touch, ascending, each with the first column (factor's ordering) the rotations
 * reach in it: the start column j_t in the supernode that holds it, the first row below the child's columns in an
 * ancestor.  supernodes / first_col (either may be NULL) hold up to nsuper entries.  Returns the count, or -1 for a W the
 * update would refuse.  Host-only plans too. */
int parsy_updown_path(const parsy_plan* plan, int k, const int* wp, const int* wi, int* supernodes, int* first_col);
typedef struct parsy_updown_info {
    int32_t path_supernodes;   /* of the last device call (0: none yet) */
    int32_t last_launches;     /* kernels it enqueued */
    int32_t last_k;
    int32_t last_sign;
    int64_t block_columns;     /* block columns of 64 columns on that path, from the entry columns on */
    int64_t entries_touched;   /* stored entries of L in the columns walked, summed over the blocks of 8 columns of W */
    int64_t device_bytes;      /* workspace, coefficient table and W's pattern held (0 before the first device call) */
} parsy_updown_info;
int parsy_updown_get_info(parsy_plan* plan, parsy_updown_info* info);          /* host-only plans too */

/* ---- Row delete and row add: take a variable out of the factor and put it back, without a refactorization -----------
 * `row` is in the caller's ordering (parsy_plan_set_perm); p is its position in the factor's ordering.  With
 *     L = [L11 0 0; l12' l22 0; L31 l32 L33]      (row and column p in the middle)
 * DELETE turns d_lValues, the factor of P A P', into the factor of the matrix whose row and column p are the identity's:
 *     w = l32;  l12 = 0, l22 = 1, l32 = 0 (exactly);  then the update L33 L33' + w w'.
 * ADD takes the new column of the symmetric matrix -- nz row indices ci (host, strictly ascending, caller's ordering, the
 * diagonal entry `row` among them) and the values d_cx on the device, never written -- and makes
 *     L11 l12 = a12;  l22 = sqrt(a22 - l12' l12);  l32 = (a32 - L31 l12) / l22;  then the downdate L33 L33' - l32 l32'.
 * What stood in row p left of the diagonal, in l22 and in column p before an add is NEVER READ; it is overwritten.  The
 * caller's obligation: everything else of d_lValues is the factor of A with row and column `row` deleted -- after a
 * delete, or after factoring values whose row `row` is the identity's.  The plan keeps no record of deleted rows:
 * entries of the column that couple `row` to another row that is still deleted must be left out by the caller.
 * THE PATTERN OF L DOES NOT CHANGE: every off-diagonal non-zero (i, p) of the column must be a stored entry of L -- for
 * i > p, i in the structure of column p; for i < p, p in the row list of i's supernode from i on.  A column that breaks
 * the rule is refused on the host, before anything is enqueued; the message names the row in both orderings.
 * Further refusals (parsy_last_error names each; nothing is written): a NULL argument, a row outside 0 .. n - 1, indices
 * unsorted or repeated, a missing diagonal entry, a plan restricted by parsy_plan_set_active / _set_active_pieces, a
 * host-only plan.
 * Only these stored entries are written: row p in the panels of the supernodes whose row list holds p (the row subtree
 * T(p), parsy_rowmod_reach), column p, and the columns of the rotation pass -- parsy_factor_updown_device's own, entered
 * at the first row below p of column p.  Everything else keeps its bits; the strict upper triangles of the diagonal
 * blocks are neither read nor written.  An add reads every entry of L in the columns of T(p) and in the rows below them
 * once.  Two calls on the same input give the same bits.
 * STATUS: parsy_rowmod_status after the stream is synchronised (it is parsy_updown_status's word): 0; `p + 1` when the
 * add's own pivot a22 - l12' l12 was <= 0 or not finite -- column p is then left as the identity's, row p as the solve
 * left it, and no downdate is enqueued; a larger column when the downdate behind it left the matrix indefinite.  After a
 * failure d_lValues is NO LONGER A FACTOR of anything, and nothing in it is NaN or Inf that was not before; the plan
 * stays usable (factor again).
 * Each call uploads its lists and waits for the stream once before it enqueues; an add whose column has rows below p
 * waits a second time, behind the kernel that forms l22, to read the status word.  Kernels are ordered by the stream
 * alone.  The first device call makes the workspaces (one double per entry of the row lists, n doubles, the transpose
 * of the row lists) and, where it does not exist yet, parsy_factor_updown_device's; all counted in the plan's
 * device_bytes.  parsy_updown_get_info's counters do not move with a row call (its device_bytes may). */
int parsy_factor_rowdel_device(parsy_plan* plan, double* d_lValues, int row, void* stream);
int parsy_factor_rowadd_device(parsy_plan* plan, double* d_lValues, int row, int nz, const int* ci, const double* d_cx,
                               void* stream);
/* Host buffers: H2D, the call above, D2H; seconds (may be NULL) = device time.  Synchronous. */
int parsy_factor_rowdel_host(parsy_plan* plan, double* lValues, int row, double* seconds);
int parsy_factor_rowadd_host(parsy_plan* plan, double* lValues, int row, int nz, const int* ci, const double* cx,
                             double* seconds);
int parsy_rowmod_status(parsy_plan* plan);
/* T(p) of `row`, ascending: per supernode the position of p in its row list and its height inside T(p) (0: no child in
 * T(p), else 1 + the largest height of its children there).  p's own supernode is a member when p is not its first
 * column.  The arrays (each may be NULL) hold up to nsuper entries.  Returns the count, or -1.  Host-only plans too. */
int parsy_rowmod_reach(parsy_plan* plan, int row, int* supernodes, int* position, int* height);
typedef struct parsy_rowmod_info {
    int32_t last_op;             /* of the last device call: 0 none yet, 1 delete, 2 add */
    int32_t last_row;            /* its row in the factor's ordering (-1: none yet) */
    int32_t reach_supernodes;    /* supernodes of T(p) */
    int32_t heights;             /* heights of T(p): launches of each of the two row kernels of an add */
    int32_t row_launches;        /* kernels enqueued over T(p): solve and panel per height and the clearing; delete: one */
    int32_t column_launches;     /* the kernel on column p (1) */
    int32_t rotation_launches;   /* kernels of the rotation pass */
    int32_t reserved;
    int64_t entries_read;        /* stored entries of L the row pass of an add reads (0 after a delete) */
    int64_t entries_walked;      /* stored entries of L in the columns the rotation pass walks (read and written once) */
    int64_t device_bytes;        /* index and workspaces held (0 before the first device call) */
} parsy_rowmod_info;
int parsy_rowmod_get_info(parsy_plan* plan, parsy_rowmod_info* info);          /* host-only plans too */

/* ---- Normal matrices: N = F diag(w) F' + beta I + A0 on the plan's pattern, and least squares through its factor -----
 * F is a sparse n x m matrix in compressed columns: Fp (m + 1 entries) and Fi (row indices, strictly ascending within a
 * column, in the caller's ordering) on the host; the values fx (nnzF doubles, in that order; positions count from
 * Fp[0]) and the weights w (m doubles, any finite values; NULL: all ones) on the device.  F's rows go through the
 * plan's ordering (parsy_plan_set_perm) like every vector of the refinement calls.  A0 is optional: nnzA doubles in A2
 * order, or NULL.
 * THE PATTERN OF A DOES NOT CHANGE: every pair of rows that share a column of F, and every row of F on the diagonal,
 * must be a stored entry of the plan's pattern of A (parsy_plan_pattern).  An F that breaks the rule is refused on the
 * host, when the handle is made; the message names the column of F and the two rows in both orderings.  Entries of the
 * pattern that F does not produce get 0 (+ beta on the diagonal) (+ A0).
 *
 * parsy_normal_pattern: the lower triangle of the pattern of F F' with a full diagonal as sorted CSC (Ap: n + 1 ints;
 * Ai == NULL: only Ap and the count) -- what to hand to parsy_order_nd and parsy_analyze, with any values, for a plan
 * that satisfies the rule.  Returns the entry count, or -1. */
int64_t parsy_normal_pattern(int n, int m, const int* Fp, const int* Fi, int* Ap, int* Ai);
/* A handle belongs to one plan and one pattern of F; several handles per plan are allowed, host-only plans (device < 0)
 * too: only the device calls refuse those.  The handle copies the plan's ordering as it stands: a later
 * parsy_plan_set_perm does not move it.  The plan is borrowed and must outlive the handle's calls.
 * The inspector runs here, once: per A2 entry q = (i, j) the list of triples (a, b, k) -- column k of F holds both rows,
 * a is the position in fx of the entry on row i, b the one on row j (i >= j in the factor's ordering, a == b on the
 * diagonal) -- ascending in k, which is the summation order; lists of more than 512 triples are cut into chunks of 512
 * (the last one shorter), the others binned by length into three classes (1, 8, 64 lanes per entry) whose borders are
 * constants; and the transposed index of F (row -> its positions in fx and their columns, ascending).
 * Refused, with parsy_last_error naming the reason and nothing allocated (NULL is returned): a NULL argument, m < 0, a
 * row outside 0 .. n - 1, indices unsorted or repeated within a column, Fp decreasing, more than 2^31 - 1 chunks (nnzF
 * is bounded by Fp's type), a plan built from L's pattern alone, the pattern rule. */
typedef struct parsy_normal parsy_normal;
parsy_normal* parsy_normal_create(parsy_plan* plan, int m, const int* Fp, const int* Fi);
void parsy_normal_destroy(parsy_normal* nrm);
typedef struct parsy_normal_info {
    int32_t n, m, nnzF;
    int32_t longest_list;        /* triples of the longest list */
    int32_t chunked_entries;     /* entries whose list is cut into chunks */
    int32_t chunks;              /* their chunks */
    int32_t border[3];           /* longest list of the 1-, 8- and 64-lane class (constants: 8, 64, 512) */
    int32_t launches;            /* kernels of one values call: one per non-empty class, two for the chunks */
    int64_t class_entries[3];    /* entries of each class */
    int64_t pairs;               /* triples in all = sum over the columns of F of c (c + 1) / 2 */
    int64_t entries_untouched;   /* entries of A's pattern that F does not produce */
    int64_t device_bytes;        /* index and workspace held by the handle (0 before its first device call); not part
                                    of the plan's figure */
} parsy_normal_info;
int parsy_normal_get_info(const parsy_normal* nrm, parsy_normal_info* info);
/* List q (0 <= q < nnzA): a, b, k (each may be NULL) hold up to longest_list entries.  Returns the length, or -1. */
int64_t parsy_normal_pairs(const parsy_normal* nrm, int64_t q, int32_t* a, int32_t* b, int32_t* k);
/* Violations of the index (0: sound): every pair of every column appears exactly once, every list ascends in k, the
 * chunks tile their lists, every entry is in the class of its length, every position of the row index holds its row. */
long long parsy_normal_check(const parsy_normal* nrm);

/* d_values[q] = ((s_q + beta on the diagonal) + d_base[q]) for EVERY entry q of A's pattern (no zero-fill needed), with
 * s_q = sum over list q of (fx[a] w[k]) fx[b] by fma in the fixed order above (w == NULL: fx[a] fx[b], the same bits as
 * w = 1).  d_base may be NULL and may be d_values itself.  One launch per non-empty class and two for the chunks,
 * ordered by the stream alone; no float atomics: two calls give the same bits, on any device.  The first device call of
 * a handle uploads its index (12 bytes per triple and the rest). */
int parsy_normal_values_device(parsy_normal* nrm, const double* d_fx, const double* d_w, double beta,
                               const double* d_base, double* d_values, void* stream);
/* Y = beta Y + alpha op(X):  PARSY_NORMAL_F   Y (n x nrhs) = beta Y + alpha F (diag(w) X),  X m x nrhs;
 *                            PARSY_NORMAL_FT  Y (m x nrhs) = beta Y + alpha F' X,           X n x nrhs (d_w is not read).
 * Column-major with leading dimensions, the n-side in the caller's ordering.  The right-hand sides go in blocks of 8;
 * column q of a call with nrhs columns is bitwise what a call with that column alone gives.  beta == 0: Y is not read.
 * Refused: a NULL argument (d_w may be NULL), another op, nrhs < 1, a leading dimension below the rows of its operand,
 * d_x == d_y, a host-only plan. */
#define PARSY_NORMAL_F 0
#define PARSY_NORMAL_FT 1
int parsy_normal_apply_device(parsy_normal* nrm, int op, const double* d_fx, const double* d_w, const double* d_x, int ldx,
                              int nrhs, double alpha, double beta, double* d_y, int ldy, void* stream);
/* Least squares: X (n x nrhs) minimises sum_k w_k (f_k' x - c_k)^2 + beta ||x||^2 for every column of C (m x nrhs), by
 * the corrected normal equations.  S is the plan's forward + backward solve with d_lValues in the handle's ordering,
 * exactly as parsy_solve_spd_device with max_steps = 0 runs it:
 *     x = S F W c;   `steps` times (steps >= 0):  r = c - F' x,  g = F W r - beta x,  x += S g;
 * and at the end r and g are formed once more from the returned x -- the residual (d_r, m x nrhs) and the gradient
 * (d_g, n x nrhs) at the answer; each may be NULL, with both NULL the last pass is skipped.  Everything is enqueued with
 * no host wait; read parsy_solve_status after synchronising (a solve of the call whose hand-off wait timed out shows
 * there).  There is no convergence test.
 * STALE FACTOR: the operator of every correction is (L L')^-1, the inverse of the matrix that was FACTORED; r and g come
 * from fx, w and beta as given.  So d_lValues may be the factor of N at nearby weights or beta: the loop is then
 * iterative refinement of the normal equations through it, and x converges to the minimiser of the problem as GIVEN as
 * far as (L L')^-1 stands for N^-1; the factor only sets the number of steps.
 * The workspace (n x nrhs + m x nrhs doubles) is the handle's, grown on demand, counted in its device_bytes.
 * Refused, with the outputs untouched: what parsy_residual_device refuses; steps < 0, nrhs < 1; ldc < m, ldx < n,
 * ldr < m, ldg < n; d_x == d_c. */
int parsy_lsq_solve_device(parsy_normal* nrm, const double* d_fx, const double* d_w, double beta, const double* d_lValues,
                           const double* d_c, int ldc, double* d_x, int ldx, int nrhs, int steps, double* d_r, int ldr,
                           double* d_g, int ldg, void* stream);
/* Host buffers: H2D, the call above, D2H; seconds (may be NULL) = device time.  Synchronous.  (lsq: x stays untouched
 * when a solve's status is bad.) */
int parsy_normal_values_host(parsy_normal* nrm, const double* fx, const double* w, double beta, const double* base,
                             double* values, double* seconds);
int parsy_normal_apply_host(parsy_normal* nrm, int op, const double* fx, const double* w, const double* x, int ldx, int nrhs,
                            double alpha, double beta, double* y, int ldy, double* seconds);
int parsy_lsq_solve_host(parsy_normal* nrm, const double* fx, const double* w, double beta, const double* lValues,
                         const double* c, int ldc, double* x, int ldx, int nrhs, int steps, double* r, int ldr, double* g,
                         int ldg, double* seconds);

/* ---- Solves with sparse right-hand sides for selected rows of the result ------------------------------------------------
 * CHOLMOD's solve2 with Bset / Xset, and the reference's blockedPrunedLSolve / reach_sn on blocks of right-hand sides.
 * B is n x nrhs in compressed columns: bp (nrhs + 1 entries from 0, non-decreasing) and bi (rows strictly ascending
 * within a column) on the host, in the caller's ordering (parsy_plan_set_perm); an empty column is allowed, its column
 * of X is exactly zero.  xi lists nx distinct rows of the result in the caller's ordering, in any order; NULL: all n rows
 * (nx is then ignored).  With P the plan's ordering:
 *   F = the supernodes of the rows of P B and all their ancestors in the supernodal etree: L^-1 P B is zero elsewhere;
 *   K = the supernodes of the rows of P xi and all their ancestors: those rows of L^-T y need nothing else.
 * A call reads only the panels of F (forward) and of K (backward): parsy_reach_info.fwd_entries / bwd_entries stored
 * entries of L, against xsize for the plan's full solves.  Every reach ends at the root: where the top separators hold
 * most of L the full solve of the plan may well be faster.  The call never falls back by itself; the counts let a caller
 * choose.
 * A handle belongs to one plan, one pattern of B and one xi, and is built once: supernodes wider than 256 columns are cut
 * into pieces of 256 (the last one shorter), a step is a set of pieces with no dependency among them (a supernode's first
 * piece one step after the last pieces of its children in the set, piece k + 1 one step after piece k; the backward pass
 * takes the steps of K in reverse), and every vector of a call lives in one compact numbering of the columns of F u K:
 * nothing a handle holds, on the host or on the device, is of size n, ssize or xsize.  The handle copies the plan's
 * ordering as it stands: a later parsy_plan_set_perm does not reach it.  The plan is borrowed and must outlive the
 * handle's calls; the handle's memory is its own and is not in the plan's device_bytes.  Host-only plans (device < 0)
 * too: only the device call refuses those.
 * Refused, with parsy_last_error naming the reason (NULL is returned, nothing is allocated): a NULL argument (bi may be
 * NULL when B has no entry), nrhs < 1, bp not non-decreasing from 0, a row outside 0 .. n - 1, rows of a column not
 * strictly ascending, a repeated row in xi, nx < 1 with xi given, a plan restricted by parsy_plan_set_active /
 * _set_active_pieces. */
typedef struct parsy_reach parsy_reach;
parsy_reach* parsy_reach_create(parsy_plan* plan, int nrhs, const int* bp, const int* bi, int nx, const int* xi);
void parsy_reach_destroy(parsy_reach* reach);
typedef struct parsy_reach_info {
    int32_t nrhs, nx;
    int32_t fwd_supernodes, fwd_pieces;   /* of F */
    int32_t bwd_supernodes, bwd_pieces;   /* of K */
    int32_t fwd_steps, bwd_steps;
    int32_t last_op;             /* of the last device call (-1: none yet) */
    int32_t last_kernels;        /* kernels it enqueued: the load, per step of each pass the triangles and -- where a piece
                                    of the step has rows below it -- the panels, the gather, the clearing */
    int64_t fwd_entries;         /* stored entries of L a forward pass over F reads */
    int64_t bwd_entries;         /* ... a backward pass over K */
    int64_t xsize;               /* ... the factor holds: what each of the plan's full solves reads */
    int64_t device_bytes;        /* index and workspaces held by the handle (0 before its first device call) */
} parsy_reach_info;
int parsy_reach_get_info(const parsy_reach* reach, parsy_reach_info* info);   /* host-only plans too */
/* F into fwd (fwd_supernodes entries) and K into bwd (bwd_supernodes entries), ascending; each may be NULL. */
int parsy_reach_get(const parsy_reach* reach, int32_t* fwd, int32_t* bwd);
/* Violations of the handle's index (0: sound): both sets closed towards the root, the steps in the order above, every
 * piece and every panel row in exactly one launch of its pass, the gather lists ascending. */
long long parsy_reach_check(const parsy_reach* reach);
#define PARSY_SPARSE_A 0      /* X = (A^-1 B)[xi, :]: forward over F, backward over K */
#define PARSY_SPARSE_GINV 1   /* X = (L^-1 P B) rows P xi: forward only, over F */
#define PARSY_SPARSE_GINVT 2  /* X = (P' L^-T P B) rows xi: backward only, over K; entries of B outside K's columns are
                                 not read */
/* d_bx: the bp[nrhs] values of B in the order of bi, never written; d_x: nx x nrhs column-major, ldx >= nx, row k the
 * row xi[k]; d_lValues: the factor in the handle's ordering.  The right-hand sides go in blocks of 8 that share nothing
 * but the read of L: column q of a call is bitwise what a handle of that column alone gives, a row of a call what a
 * handle with fewer selected rows gives for it, and entries of B that carry 0.0 change nothing.  Every sum has one order,
 * fixed by the pattern (occurrences of a row in ascending position of lR, columns of a panel ascending, segments of 1024
 * rows ascending); kernels are ordered by the stream alone, without flags, tickets or float atomics: two calls give the
 * same bits.  The plan's own solve schedule is not used and nothing of the plan is written.
 * The handle's first device call uploads its index and makes its workspaces (all zero between calls: a call ends by
 * clearing exactly what it wrote); after it a call allocates nothing and waits for nothing, it only enqueues.  One call
 * per handle at a time.
 * Refused, with nothing written: a NULL argument (d_bx may be NULL when B has no entry), ldx < nx, an unknown op, a plan
 * restricted by parsy_plan_set_active / _set_active_pieces, a handle of a host-only plan. */
int parsy_solve_sparse_device(parsy_reach* reach, const double* d_lValues, const double* d_bx, int op, double* d_x, int ldx,
                              void* stream);
/* Host buffers, through the staging layer of the other host calls: the whole factor goes up into the plan's staging
 * buffer (xsize doubles, as parsy_solve_host does it -- the upload reads all of L even where the solve does not), bx up,
 * the call above, x back; seconds (may be NULL) = device time.  Synchronous. */
int parsy_solve_sparse_host(parsy_reach* reach, const double* lValues, const double* bx, int op, double* x, int ldx,
                            double* seconds);

/* Host-buffer conveniences (H2D + kernels + D2H, synchronous). `seconds`, if
 * non-NULL, receives the device time of the numeric kernels alone. */
int parsy_factor_host(parsy_plan* plan, const double* values, double* lValues, double* seconds);
int parsy_solve_host(parsy_plan* plan, const double* lValues, double* x, int nrhs, int ldx,
                     double* seconds);

/* Device time (ms, hipEvents on the launch stream) of the last factor / solve
 * enqueued through the *_device calls, after synchronisation; <0 if none. */
double parsy_last_factor_ms(parsy_plan* plan);
double parsy_last_solve_ms(parsy_plan* plan);

/* Per-launch timing with hipEvents on the launch stream (adds two event records per
 * kernel launch, so keep it out of throughput measurements).
 *   parsy_plan_profile(plan, 1) on, (plan, 0) off, (plan, 2) on + reset accumulators.
 *   parsy_plan_profile_collect(plan): after the stream is synchronised, add the
 *     elapsed time of every launch of the last factor/solve to its kernel kind.
 *   parsy_plan_profile_get: accumulated ms and launch counts per kind (PARSY_PROFILE_KINDS = 10 entries:
 *     0 SMALL, 1 TILES, 2 CHAIN, 3 BIG, 4 unused, 5 SOLVE_SMALL, 6 SOLVE_PANEL, 7 SOLVE_FIXUP,
 *     8 BACK_BLOCK, 9 unused; the arrays passed must hold 10 entries) and the number of collected runs. */
#define PARSY_PROFILE_KINDS 10
int parsy_plan_profile(parsy_plan* plan, int enable);
int parsy_plan_profile_collect(parsy_plan* plan);
int parsy_plan_profile_get(parsy_plan* plan, double* kind_ms, int* kind_launches, int* runs);
/* The factorization launches of the collected runs per level of the Cholesky view: accumulated ms of the launches
 * that run on the caller's stream (main_ms[chol_levels]) and of those that belong to the plan's side stream
 * (side_ms[level] = the side launches whose targets start at that level).  Returns chol_levels. */
int parsy_plan_profile_levels(parsy_plan* plan, double* main_ms, double* side_ms);

/* Thread-local message of the last failing call. */
const char* parsy_last_error(void);

/* Number of visible HIP devices (0 when none / runtime unusable). */
int parsy_device_count(void);

/* ---- Diagnostics: kernel witness ------------------------------------------------------------------------
 * One host-side counter per factor and solve kernel instantiation that the library can enqueue (process-wide, every
 * plan and device), incremented when a launch of it is enqueued.  Tests use it to prove which kernels a factorization
 * or a solve ran.
 * Entries 0 .. parsy_debug_kernel_count() - 1; the name is the kernel's, template arguments included (for example
 * "k_solve_small_mrhs<64,true>"; NULL out of range). */
int parsy_debug_kernel_count(void);
const char* parsy_debug_kernel_name(int k);
unsigned long long parsy_debug_kernel_launches(int k);
void parsy_debug_kernel_reset(void);

/* ------------------------------------------------------------------------ */
/* 3. Inspector (host)                                                       */
/* ------------------------------------------------------------------------ */

typedef struct parsy_symbolic parsy_symbolic;

/* Borrowed pointers into a parsy_symbolic (valid until it is freed).
 * Names follow the reference's BCSC (common/def.h:117-204). */
typedef struct parsy_symbolic_view {
    int32_t n, nsuper, nlevels, maxSupWid, maxCol;
    int64_t ssize, xsize, nnzL, nnzA, n_updates;
    double flops_colcount, flops_stored;
    const int* Perm;       /* n, new -> old */
    const int* Parent;     /* n, column etree */
    const int* ColCount;   /* n */
    const int* super;      /* nsuper+1 */
    const int* col2Sup;    /* n */
    const int* sParent;    /* nsuper */
    const size_t* p;       /* n+1 */
    const size_t* i_ptr;   /* n+1 */
    const int* s;          /* ssize */
    const int* A1p; const int* A1i;                       /* upper PAP' pattern */
    const int* A2p; const int* A2i; const double* A2x;    /* lower PAP' */
    const int* A2src;      /* nnzA: position of each A2 entry in the input Ax */
    const int* levelPtr;   /* nlevels+1 */
    const int* levelSet;   /* nsuper */
    const int64_t* updPtr; /* nsuper+1 */
    const int* updSn; const int* updLb; const int* updUb; /* n_updates each */
} parsy_symbolic_view;

/* Ap/Ai/Ax: lower triangle, CSC, sorted (what common/Util.h:77 reads).
 * perm: n entries new->old or NULL.  nrelax/zrelax: 3 entries each or NULL for
 * the reference driver's defaults {4,16,48} / {0.8,0.1,0.05}. */
parsy_symbolic* parsy_analyze(int n, const int* Ap, const int* Ai, const double* Ax,
                              const int* perm, const int* nrelax, const double* zrelax);
void parsy_symbolic_free(parsy_symbolic* sym);
int parsy_symbolic_get(const parsy_symbolic* sym, parsy_symbolic_view* view);
/* Plan straight from an inspector result. */
parsy_plan* parsy_plan_from_symbolic(const parsy_symbolic* sym, int device);

/* ------------------------------------------------------------------------ */
/* 4. Synthetic SPD matrices / orderings (host)                              */
/* ------------------------------------------------------------------------ */

/* Lower triangle of a grid stencil matrix (5/9-point 2-D with nz = 1, 7/27-point
 * 3-D): off-diagonals -1, diagonal = degree + shift.  Call with Ai = Ax = NULL to
 * get the entry count; Ap needs nx*ny*nz+1 ints. Returns nnz or <0. */
int64_t parsy_grid_spd_lower(int nx, int ny, int nz, int stencil, double shift, int* Ap,
                             int* Ai, double* Ax);
/* Geometric nested dissection, perm[new] = old, nx*ny*nz entries. */
int parsy_grid_nested_dissection(int nx, int ny, int nz, int leaf, int* perm);
/* Fill-reducing ordering of an arbitrary symmetric pattern (lower triangle, CSC): nested dissection
 * on the graph with level-structure separators (the reference calls METIS, cholesky/LSparsity.h:
 * not in this build).  leaf <= 0 picks the default (64).  perm[new] = old, n entries.  0 on success. */
int parsy_order_nd(int n, const int* Ap, const int* Ai, int leaf, int* perm);

/* ------------------------------------------------------------------------ */
/* 5. One process, several devices: the distributed factorization            */
/* ------------------------------------------------------------------------ */

/* The distribution of section 2 run by ONE process that drives every device (the drivers' path; bench.py runs the
 * same distribution with one process per GPU and RCCL point-to-point messages).
 * `devices` lists one HIP device per rank; a device may appear more than once (several ranks share it: how the
 * path is exercised on a node with fewer GPUs).  Every rank keeps its own lValues; finished pieces travel as
 * device-to-device copies (peer access over xGMI between different devices) of exactly the segments of the
 * parsy_dist messages, ordered by events.  values: host, nnz(A2) doubles.
 * STATUS: verified bit for bit with several ranks sharing ONE device (tests/test_gpu_parity.py::test_distributed_*).
 * The distinct-device branch -- hipDeviceEnablePeerAccess, hipStreamWaitEvent on another device's event, the copy
 * kernel reading a peer's buffer -- has NOT run on hardware yet: no node with two GPUs was available to the builder
 * (tests/test_multigpu_gpu.py::test_two_distinct_devices_* run it wherever two devices are visible). */
typedef struct parsy_mg parsy_mg;
parsy_mg* parsy_mg_create(const parsy_symbolic* sym, int nranks, const int* devices, int block);
void parsy_mg_destroy(parsy_mg* mg);
int parsy_mg_set_values(parsy_mg* mg, const double* values);
/* Enqueue one distributed factorization on every rank's stream and wait for it; seconds (may be NULL) = wall
 * time from the first enqueue to the last rank's completion.  Returns 0, or the factorization status of the
 * first rank that reports one (> 0: non-positive pivot column, < 0: error). */
int parsy_mg_factor(parsy_mg* mg, double* seconds);
/* One factorization with every launch timed by itself: the ranks take turns (a rank's step of a level runs alone
 * on its device, also when ranks share one), per-launch hipEvents as parsy_plan_profile.  main_ms / side_ms:
 * nranks x chol_levels (row = rank) ms of the main-stream and side-stream launches per level; copy_ms: nranks x
 * chol_levels ms of the copies a rank receives after a level.  What a rank would spend on a device of its own,
 * for the model of DESIGN.md section 6.  Returns as parsy_mg_factor. */
int parsy_mg_profile(parsy_mg* mg, double* main_ms, double* side_ms, double* copy_ms);
/* Per rank: device milliseconds of its last factorization (hipEvents on its stream). rank_ms[nranks]. */
int parsy_mg_rank_ms(parsy_mg* mg, double* rank_ms);
/* Collect the factor on the host: every piece from its owner (lValues: xsize doubles). */
int parsy_mg_gather_host(parsy_mg* mg, double* lValues);
const parsy_dist* parsy_mg_dist(const parsy_mg* mg);
parsy_plan* parsy_mg_plan(parsy_mg* mg, int rank);

#ifdef __cplusplus
}
#endif
#endif /* PARSY_AMD_H */
