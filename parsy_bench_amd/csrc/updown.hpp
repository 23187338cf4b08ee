// Update and downdate of the factor in place: given a sparse n x k matrix W, L L' = A becomes the factor of A + W W'
// (sign +1) or A - W W' (sign -1) without a refactorization (updown.cpp, updown_kernels.hip).
//
// In the factor's ordering, for column j of L and column t of W, with d = L_jj, w = W_jt and sigma = sign:
//     r = sqrt(d^2 + sigma w^2), c = r / d, s = w / d, L_jj = r, W_jt = 0, and for the rows i > j of column j
//     L_ij = (L_ij + sigma s W_it) / c, then W_it = c W_it - s L_ij (the new one).
// Columns j ascend; w == 0 is the identity.  The pattern of L does not change: a column t of W whose first row (in the
// factor's ordering) is j_t may have non-zeros only in the structure of column j_t of L -- the row list of j_t's
// supernode from j_t on -- and then no rotation ever leaves the pattern.  The host refuses every other W before anything
// is enqueued.
//
// Only the supernodes on the etree paths from the supernodes of the j_t to the root are touched; they go in ascending
// order (parents have larger indices), each from the column it is entered at, in block columns of kUpdownTile columns:
// one launch for the diagonal tile of a block column (it leaves the rotations' coefficients in a table), one for all
// panel rows below that tile.  W goes through in blocks of kUpdownBlock columns that share the reads and writes of L.
// Stream order is the only dependency: no flags, no tickets, no waits between workgroups.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "schedule.hpp"

struct parsy_plan;

namespace parsy {

constexpr int kUpdownBlock = 8;    // columns of W per pass over the path (W values a lane carries; workspace columns)
constexpr int kUpdownTile = 64;    // columns of a block column; edge of the diagonal tile
constexpr int kUpdownRows = 256;   // panel rows of one workgroup of the rows launch
constexpr int kUpdownCoef = 4;     // doubles per rotation in the coefficient table: 1/c, sigma s, c, -s

// A checked W in the factor's ordering: per column the rows ascending, and where each value stands in the caller's wx.
struct UpdownW {
    int k = 0;
    std::vector<int> ptr;   // k + 1
    std::vector<int> row;   // rows in the factor's ordering
    std::vector<int> src;   // index into the caller's values
};
struct UpdownNode {         // a supernode of a path and the first column the rotations reach in it
    int32_t sn, first_col;
};

// the supernode that holds column j
int supernode_of(const Schedule& S, int j);
// The refusals that need no device and the pattern rule; 0 with `out` filled, or -1 with the message set.  perm: the
// plan's ordering (perm[new] = old; empty: identity).
int updown_prepare(const Schedule& S, const std::vector<int>& perm, const char* who, int k, const int* wp, const int* wi,
                   UpdownW& out);
// The union of the etree paths of the non-empty columns [t0, t1) of W, ascending.
void updown_path(const Schedule& S, const UpdownW& W, int t0, int t1, std::vector<UpdownNode>& path);
// block columns of a path: per supernode those from the one that holds first_col on
int64_t updown_block_columns(const Schedule& S, const std::vector<UpdownNode>& path);

struct UpdownState;   // the device state (feature_states.hpp)
// refusals of parsy_factor_updown_device / _host that need no device; 0, or -1 with the message set
int updown_check_args(const parsy_plan* pl, const char* who, const void* lValues, int sign, int k, const void* wp,
                      const void* wi, const void* wx);
// the plan's state, made on first use (host-only plans too: it holds the counters of parsy_updown_get_info)
int updown_ensure_host(parsy_plan* pl);
int plan_factor_updown(parsy_plan* pl, double* d_L, int sign, int k, const int* wp, const int* wi, const double* d_wx,
                       void* stream);
int plan_updown_status(parsy_plan* pl);

// The rotation pass alone, for ONE column that already stands in column 0 of the workspace (rowmod.hpp): the path entered
// at first_col (< 0: no path), with the same launches as a call with k = 1 makes behind its scatter.  _begin makes the
// device state and uploads the path's row lists on `stream` (nothing of it is read before the stream has run that copy);
// _reset arms the status word as a call does; _run enqueues.  The counters of parsy_updown_get_info do not move.
struct UpdownWalk {
    std::vector<UpdownNode> path;
    int64_t rows_total = 0;          // rows of the path's row lists
    int launches = 0;
    int64_t entries = 0;             // stored entries of L in the columns walked
};
int plan_updown_walk_begin(parsy_plan* pl, int first_col, UpdownWalk& Wk, void* stream);
int plan_updown_status_reset(parsy_plan* pl, void* stream);
int plan_updown_walk_run(parsy_plan* pl, double* d_L, int sign, UpdownWalk& Wk, void* stream);
double* plan_updown_workspace(parsy_plan* pl);       // (null before the device state exists)
int32_t* plan_updown_status_word(parsy_plan* pl);

}  // namespace parsy
