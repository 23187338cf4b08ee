// Device helpers shared by the HIP translation units (included by the .hip files only).
#pragma once
#include <hip/hip_runtime.h>

#include "device_wait.hpp"
#include "schedule.hpp"

namespace parsy {

typedef double double4_t __attribute__((ext_vector_type(4)));   // accumulator of v_mfma_f64_16x16x4_f64

static constexpr int kLdDiag = kTile + 1;   // padded leading dimension of a 64 x 64 diagonal block in LDS

__device__ __forceinline__ double readlane_f64(double v, int src_lane) {
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), src_lane),
                            __builtin_amdgcn_readlane(__double2loint(v), src_lane));
}

// 16x16 MFMA product acc += X Y of blocks of an LDS matrix (column-major, leading dimension LD); lane (l15, kq) holds
// column l15, rows kq + 4 v of the result (v_mfma_f64_16x16x4_f64: A lane = (row l15, k kq), B lane = (k kq, column l15)).
template <int LD = kLdDiag>
__device__ __forceinline__ double4_t mm16(double4_t acc, const double* __restrict__ X, const double* __restrict__ Y,
                                          int l15, int kq) {
#pragma unroll
    for (int st = 0; st < 4; ++st)
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(X[(4 * st + kq) * LD + l15], Y[l15 * LD + 4 * st + kq], acc, 0, 0, 0);
    return acc;
}
template <int LD = kLdDiag>
__device__ __forceinline__ void put16(double* __restrict__ Z, double4_t acc, double sign, int l15, int kq) {
#pragma unroll
    for (int v = 0; v < 4; ++v) Z[l15 * LD + kq + 4 * v] = sign * acc[v];
}

// beta == 0: y is not read (it may hold NaN)
__device__ __forceinline__ void store_y(double* __restrict__ y, double alpha, double beta, double s) {
    *y = beta == 0.0 ? alpha * s : fma(beta, *y, alpha * s);
}

}  // namespace parsy
