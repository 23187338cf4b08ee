// Row delete and row add in the factor, in place (rowmod.cpp, rowmod_kernels.hip): CHOLMOD's rowdel and rowadd on the
// pattern the analysis holds.  With p the position of the caller's row in the factor's ordering and
//     L = [L11 0 0; l12' l22 0; L31 l32 L33]   (row / column p in the middle):
//   delete  w = l32, then l12 = 0, l22 = 1, l32 = 0 and the update L33 L33' + w w';
//   add     L11 l12 = a12, l22 = sqrt(a22 - l12' l12), l32 = (a32 - L31 l12) / l22, then the downdate L33 L33' - l32 l32'.
// The rotation pass is updown's own (updown.hpp: plan_updown_walk), entered at the first row below p of column p.
//
// The row subtree T(p): the supernodes whose row list holds p -- p's own supernode with its leading p - c0 columns when p
// is not its first column.  It is a subtree of the supernodal etree; the non-zeros of l12 lie in its columns, every row
// i < p of one of its row lists belongs to one of its supernodes and every row i > p lies in the structure of column p.
// So one pass over T(p) in ascending HEIGHT (0: no child in T(p)) yields l12 and L31 l12: per height one launch that
// solves with the diagonal blocks and one that multiplies the rows below them, each supernode leaving its products in
// T, a workspace with one double per entry of the row lists, from where the next height (and at last column p) gathers
// them in ascending position.  Stream order is the only dependency.
#pragma once
#include <cstdint>
#include <vector>

#include "apply.hpp"
#include "schedule.hpp"

struct parsy_plan;

namespace parsy {

constexpr int kRowmodTile = 64;    // block columns of the triangular solve inside a supernode
constexpr int kRowmodRows = 256;   // panel rows of one workgroup of k_rowadd_panel; columns of y staged at a time

struct RowmodNode {     // a supernode of T(p)
    int32_t sn;
    int32_t pos;        // position of p in its row list
    int32_t ks;         // columns that take part: its width, or p - c0 for p's own supernode
    int32_t height;     // inside T(p): 0 without a child in T(p), else 1 + the largest of its children's
};
// T(p), ascending, from the transpose of the row lists (build_apply_index).
void rowmod_reach(const Schedule& S, const ApplyIndex& index, int p, std::vector<RowmodNode>& out);
// entries of L the row pass of an add reads: per supernode the triangle of its ks columns and the rows below them
int64_t rowmod_entries_read(const Schedule& S, const std::vector<RowmodNode>& reach);
// first row below p of column p of L: where the rotation pass is entered (-1: the column ends with its diagonal)
int rowmod_first_below(const Schedule& S, int p);

// A checked column in the factor's ordering: rows ascending, and where each value stands in the caller's cx.
struct RowmodColumn {
    int p = -1;
    std::vector<int32_t> row, src;
};
// The position of the caller's row under the inverse of the plan's ordering (inv[old] = new; empty: identity:
// plan_perm_inverse); -1 with the message set for a row outside 0 .. n - 1.
int rowmod_position(const Schedule& S, const std::vector<int>& inv, const char* who, int row);
// The refusals of an add that need no device and the pattern rule; 0 with `out` filled, or -1 with the message set.
int rowadd_prepare(const Schedule& S, const std::vector<int>& inv, const char* who, int row, int nz, const int* ci,
                   RowmodColumn& out);

struct RowmodState;   // the device state (feature_states.hpp)
// the plan's state with the transposed index, made on first use (host-only plans too)
int rowmod_ensure_host(parsy_plan* pl);
// refusals of the device / host-buffer calls that need no device, in the order of the header; 0, or -1 with the message set
int rowdel_check_args(parsy_plan* pl, const char* who, const void* lValues, int row, int* p);
int rowadd_check_args(parsy_plan* pl, const char* who, const void* lValues, int row, int nz, const void* ci,
                      const void* cx, RowmodColumn& col);
int plan_factor_rowdel(parsy_plan* pl, double* d_L, int row, void* stream);
int plan_factor_rowadd(parsy_plan* pl, double* d_L, int row, int nz, const int* ci, const double* d_cx, void* stream);

}  // namespace parsy
