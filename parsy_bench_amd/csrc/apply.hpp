// The factor as an operator: G = P' L with G G' = A, applied as G, G', G^-1 or G^-T to column-major blocks of vectors
// in the caller's ordering (apply.cpp, apply_kernels.hip).
//
// The two products are new kernels without floating-point atomics.  Every output element has ONE summation order,
// whatever the number of right-hand sides: the work is cut on the host, once per plan, into wave-sized tasks whose
// shapes depend on the pattern alone, and the right-hand sides are processed in blocks of kApplyBlock columns that
// share nothing but the read of L.
//
//   Y = L X    pass A: a task is 64 consecutive rows of one chunk (<= kApplyChunk columns) of a supernode's panel; a
//              lane owns a row and runs one fma chain over the chunk's columns in ascending order into T, which has a
//              row per (chunk, entry of the row list lR).  Pass B: a lane per output row adds that row's occurrences in
//              T in ascending lR position (within an occurrence: ascending chunk) and writes Y.
//   Y = L' X   X is staged with the right-hand sides of a row contiguous.  Pass A: a task is <= kApplyCols columns of a
//              panel over one segment of <= kApplySeg rows; lane l takes the rows i = l (mod 64) in ascending order,
//              a butterfly adds the lanes.  Pass B: a lane per output column adds the segments' partials in order.
//
// The inverse operators permute into an n x nrhs workspace and call the existing solves on it.  The plan holds an
// ApplyState only once one of these calls (or parsy_factor_apply_get_info) has run.
#pragma once
#include <cstdint>
#include <vector>

#include "schedule.hpp"

struct parsy_plan;

namespace parsy {

constexpr int kApplyBlock = 8;     // B: right-hand sides per pass over L (accumulators of a lane; workspace columns)
constexpr int kApplyChunk = 256;   // columns of a panel that one fma chain of Y = L X runs over (a multiple of 64)
constexpr int kApplySeg = 2048;    // rows of a panel per partial of Y = L' X (a multiple of 64)
constexpr int kApplyCols = 4;      // columns of a panel that one wave of Y = L' X sums side by side

// The transpose of the row lists: row -> its positions in lR, ascending.
struct ApplyIndex {
    std::vector<int64_t> ptr;   // n + 1
    std::vector<int64_t> pos;   // ssize
    int32_t max_occurrences = 0;
};
void build_apply_index(const Schedule& S, ApplyIndex& I);

struct ApplyTaskL {    // 64 rows of one chunk of a panel (Y = L X, pass A)
    int64_t px;        // offset in lValues of (row 0, first column of the chunk)
    int64_t toff;      // row of T of (this chunk, row 0 of the panel)
    int32_t r;         // rows of the panel
    int32_t x0;        // row of X of the chunk's first column
    int32_t i0;        // first row of the task (a multiple of 64, >= cb)
    int32_t ncol;      // columns of the chunk
    int32_t cb;        // first column of the chunk inside the panel
    int32_t pad;
};
struct ApplyOcc {      // one occurrence of a row in lR (Y = L X, pass B), in the order of ApplyIndex::pos
    int64_t off;       // row of T of (chunk 0, this row of the panel)
    int32_t stride;    // rows of T between two chunks (= rows of the panel)
    int32_t n;         // chunks that reach this row
};
struct ApplyTaskLt {   // <= kApplyCols columns of a panel over one segment of its rows (Y = L' X, pass A)
    int64_t px;        // offset in lValues of (row 0, first column of the task)
    int64_t poff;      // row of the partials of (this segment, first column of the task)
    int64_t pi;        // offset of the panel's row ids in lR
    int32_t r;         // rows of the panel
    int32_t c;         // first column of the task inside the panel
    int32_t nc;        // columns of the task
    int32_t i0, i1;    // rows [i0, i1) of the panel, i0 a multiple of 64
    int32_t pad;
};
struct ApplyCol {      // one output of Y = L' X (pass B)
    int64_t off;       // row of the partials of (the first segment that reaches the column, the column)
    int32_t stride;    // rows of the partials between two segments (= width of the supernode)
    int32_t n;         // segments from there on
};

struct ApplyLayout {
    std::vector<ApplyTaskL> l_tasks;
    std::vector<ApplyOcc> occ;        // ssize, transposed order
    std::vector<ApplyTaskLt> lt_tasks;
    std::vector<ApplyCol> col;        // n
    int64_t t_rows = 0;               // rows of T
    int64_t p_rows = 0;               // rows of the partials of Y = L' X
};
void build_apply_layout(const Schedule& S, const ApplyIndex& I, ApplyLayout& A);
// doubles of the products' workspace for blocks of kApplyBlock columns: T, or the partials and the staged X
int64_t apply_workspace_len(const Schedule& S, const ApplyLayout& A);

struct ApplyState;   // the device state (feature_states.hpp)
// the host index of a plan, made on first use (host-only plans too)
int apply_ensure_host(parsy_plan* pl);
// refusals of parsy_factor_apply_device / _host that need no device; 0, or -1 with the message set
int apply_check_args(const parsy_plan* pl, const char* who, const void* lValues, int op, const void* x, int ldx,
                     int nrhs, const void* y, int ldy);
// Y = beta Y + alpha op(X) (stream: a hipStream_t)
int plan_factor_apply(parsy_plan* pl, const double* d_L, int op, const double* d_x, int ldx, int nrhs, double alpha,
                      double beta, double* d_y, int ldy, void* stream);

}  // namespace parsy
