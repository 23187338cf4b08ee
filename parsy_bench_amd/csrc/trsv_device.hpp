// What more than one of the solve kernel sources (trsv_kernels.hip, trsv_bwd_kernels.hip, trsv_aux_kernels.hip) uses,
// and nothing else: a constant or helper with one user lives in that user's file.
#pragma once
#include <hip/hip_runtime.h>

#include "device_util.hpp"
#include "kernels.hpp"

namespace parsy {

static constexpr int kThreads = 256;
static constexpr int kRhsM = 64;        // right-hand sides per pass
static constexpr int kLdXm = kRhsM + 16;  // row stride of the staged x_jb / t_jb (doubles): conflict-free operand reads

// The armed pattern of the hand-off buffers (k_solve_chain_w's comment, trsv_kernels.hip, has the protocol): a value is
// valid as soon as it differs from it.
static constexpr unsigned kXArmedWord = 0xFFF7A5A5u;   // both 32-bit halves of the armed pattern
static constexpr long long kXArmed = (long long)(((unsigned long long)kXArmedWord << 32) | kXArmedWord);
// A published value must differ from the armed pattern.  Arithmetic cannot produce it (operations on NaNs return quiet
// NaNs), only an input can carry it: it is published as a quiet NaN instead, so that the hand-off completes and the
// NaN propagates like any other (without this such a right-hand side ran into the 2 s timeout and status -1).
__device__ __forceinline__ double unarmed(double v) {
    return __double_as_longlong(v) == kXArmed ? __longlong_as_double(0x7FF8000000000000LL) : v;
}
static constexpr int kInvPacked = kTile * (kTile + 1) / 2;   // packed lower triangle of an inverse diagonal block
static constexpr int kChainThreads = 2 * kSolveRows;         // eight waves

}  // namespace parsy
