// Solves with sparse right-hand sides for selected rows of the result (reach.cpp, sparse_solve_kernels.hip): the reference's
// blockedPrunedLSolve / reach_sn (triangularSolve/Triangular_BCSC.h:55, common/Reach.h:31) on blocks of right-hand sides,
// with the backward direction.
//
// B is n x nrhs in compressed columns, Xset a list of rows of the result, both in the caller's ordering.  Two sets of
// supernodes, each closed towards the root of the supernodal etree (Schedule::sparent):
//   F  the supernodes of the rows of P B (union over the columns) and their ancestors: L^-1 P B is zero outside their columns;
//   K  the supernodes of the rows of P Xset and their ancestors: row j of L^-T y needs x on the ancestors of j's supernode only.
// Every row below a supernode of a closed set belongs to a supernode of the set, so one compact numbering over the
// columns of F u K carries every vector of a call: nothing a handle holds is of size n, ssize or xsize.
//
// Supernodes wider than kSparsePiece columns are cut into pieces (column ranges of kSparsePiece, the last one shorter): a
// piece is a triangle and every panel row below it, the supernode's own later columns among those rows.  A step is a set
// of pieces with no dependency among them: a supernode's first piece comes one step after the last pieces of its children
// in the set, piece k + 1 one step after piece k; the backward pass takes the steps of its own set in reverse order.
#pragma once
#include <cstdint>
#include <vector>

#include "schedule.hpp"

struct parsy_reach;

namespace parsy {

constexpr int kSparsePiece = 256;   // columns of a piece = columns of y a panel workgroup stages
constexpr int kSparseBlock = 8;     // right-hand sides per block (accumulators of a lane)
constexpr int kSparseTile = 64;     // block column of the triangle solves
constexpr int kSparseRows = 256;    // forward panel: rows per workgroup, a lane each
constexpr int kSparseCols = 4;      // backward panel: columns of a task
constexpr int kSparseSeg = 1024;    // backward panel: rows of a segment (one partial per column and segment)

struct SparsePiece {      // a piece as the kernels read it
    int64_t px;           // the supernode's panel in lValues
    int64_t e0;           // the supernode's first row-list entry in the compact map (and in T)
    int64_t p0;           // backward: its first partial; (segment, column of the piece) is p0 + segment * nc + column
    int32_t r, w;         // rows and width of the supernode
    int32_t c0, nc;       // the piece: first column inside the supernode, columns
    int32_t y0;           // compact index of the piece's first column
    int32_t nseg;         // backward: segments of the rows below the piece
};

struct SparsePass {                   // one direction over one closed set
    std::vector<int32_t> sn;          // the set, ascending
    std::vector<SparsePiece> pieces;  // grouped by step (stable: ascending supernode, then piece)
    std::vector<int32_t> step_first;  // steps + 1: first piece of every step
    std::vector<int32_t> work;        // the panel launches' pairs, grouped by step -- forward: (piece, first row) per workgroup;
                                      // backward: (piece, segment * column groups + column group) per wave
    std::vector<int32_t> work_first;  // steps + 1: first pair of every step
    int64_t entries = 0;              // stored entries of L a pass reads: per supernode its triangle and the rows below
    int steps() const { return (int)step_first.size() - 1; }
};

struct ReachIndex {
    int n = 0, nrhs = 0, nx = 0;
    int64_t xsize = 0;
    int32_t ncomp = 0;                // columns of F u K = length of the compact numbering
    int64_t nent = 0;                 // row-list entries of the supernodes of F u K
    int64_t npart = 0;                // partials of the backward panel launches
    std::vector<int32_t> cmap;        // nent: the compact index of every row-list entry's row
    std::vector<uint8_t> colmask;     // ncomp: 1 = a column of F, 2 = of K
    std::vector<uint8_t> entmask;     // nent: 1 = an entry of a supernode of F
    std::vector<int64_t> gptr, gpos;  // per compact column its occurrences below the columns of the supernodes of F
                                      // (entries of cmap / T), ascending = ascending position in lR
    std::vector<int32_t> bcol, bcomp; // per entry of B: its column, the compact index of its row
    std::vector<int32_t> xcomp;       // nx: the compact index of every selected row, in the order of Xset
    SparsePass fwd, bwd;              // over F, over K
};

// The whole index of a handle.  inv: the plan's ordering (inv[old] = new; empty: identity); xi null: all rows (nx is then
// ignored).  0, or -1 with the refusal as the last error (out is then empty).
int reach_build(const Schedule& S, const std::vector<int>& inv, const char* who, int nrhs, const int* bp, const int* bi, int nx,
                const int* xi, ReachIndex& out);
// Violations of an index (0: sound): both sets closed, the steps ordered as the rule says, every piece and every panel
// row of a pass in exactly one launch, the compact map inside its range, the gather lists ascending.
long long reach_check(const Schedule& S, const ReachIndex& I);
// kernels one device call enqueues (op: PARSY_SPARSE_*): the load, per forward step the triangles and -- where a piece of
// the step has rows below -- the panels, per backward step likewise, the gather and the clearing
int reach_kernels(const ReachIndex& I, int op);

// the device call and the refusals of both solve calls that need no device (sparse_solve_kernels.hip; stream: a hipStream_t)
int reach_check_args(const parsy_reach* h, const char* who, const void* lValues, const void* bx, int op, const void* x, int ldx);
int reach_solve(parsy_reach* h, const double* d_L, const double* d_bx, int op, double* d_x, int ldx, void* stream);

}  // namespace parsy
