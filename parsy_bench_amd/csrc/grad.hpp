// Gradients with respect to the values of A: the pattern of A as the plan sees it, the product of two sets of vectors
// sampled on that pattern, and the entries of Z = (P A P')^-1 gathered to it (grad.cpp, grad_kernels.hip).
//
// Host part (grad.cpp, plain C++: host-only plans use it too): the permuted coordinates (row[q], col[q]), row >= col,
// of every A2 entry q, recovered from where the factorization scatters it -- a_dst[q] = px + (col - c0) * r + (position
// of row in the supernode's row list), as the refinement's pattern is (refine_kernels.hip).  Device part: a GradState,
// which a plan holds only once one of the device calls has run; a plan that never calls them allocates nothing.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "schedule.hpp"

struct parsy_plan;

namespace parsy {

// Default number of right-hand sides from which parsy_pattern_outer_device stages its operands and splits an entry's
// sum over lanes (PARSY_GRAD_MRHS_MIN): the residual kernels' split (refine_kernels.hip, nrhs <= 4 direct).
constexpr int kGradMrhsMin = 5;
int grad_mrhs_min();   // PARSY_GRAD_MRHS_MIN, read at every call

struct GradPattern {
    std::vector<int32_t> row, col;   // nnzA entries each, A2 order
    int64_t offdiag = 0;             // entries with row != col
};
// false with `what` set when an entry lies outside its supernode's panel or above the diagonal
bool build_grad_pattern(const Schedule& S, GradPattern& P, std::string& what);

struct GradState;   // the device state (feature_states.hpp)

}  // namespace parsy
