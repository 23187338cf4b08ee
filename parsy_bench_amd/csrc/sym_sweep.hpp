// The symmetric row sweep under the A x = b calls: every row of both triangles of P A P' (RefineState's CSR) gives
// acc = sum a z and den = sum |a||z| per right-hand side, and an epilogue `Out` turns (b, acc, den) into the value stored
// for the row (by the row's first lane) and the bits the workgroup max-reduces.  The residual (refine_kernels.hip) and
// dporfs's weights (cond_kernels.hip) are two epilogues of the one loop, so both take their sums in the same fixed
// order: a fixed lane split and a fixed butterfly, no float atomics, bitwise the same from run to run.  Maxima are
// reduced as the bit patterns of non-negative doubles (an unsigned max: a NaN outranks every number and so survives
// the reduction).
// The products Y = A X of the eigensolver (eigs_kernels.hip) are a third epilogue.  The gathered values are an argument:
// the A x = b calls pass RefineState::d_vf, the eigensolver one buffer for A and one for M.
// Device code: included by those three files only.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <type_traits>
#include <utility>

#include "executor.hpp"
#include "hip_check.hpp"
#include "kernels.hpp"
#include "plan_util.hpp"
#include "refine.hpp"

namespace parsy {

__device__ __forceinline__ u64 shfl_xor_u64(u64 v, int m) {
    const int lo = __shfl_xor((int)(unsigned)v, m), hi = __shfl_xor((int)(unsigned)(v >> 32), m);
    return ((u64)(unsigned)hi << 32) | (u64)(unsigned)lo;
}

// One wave's max, then the workgroup's across its four waves; lane 0 of wave w leaves its value in sm[w].
__device__ __forceinline__ u64 block_max(u64 v, u64* sm) {
    for (int o = 32; o; o >>= 1) v = max(v, shfl_xor_u64(v, o));
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = v;
    __syncthreads();
    return max(max(sm[0], sm[1]), max(sm[2], sm[3]));
}

__device__ __forceinline__ u64 abs_bits(double v) { return (u64)__double_as_longlong(fabs(v)); }

// ||A||_1 of the symmetric A: the largest row sum of |vf| (row sums = column sums), G lanes per row; part[blockIdx.x].
// (Not an epilogue of the sweep: it reads neither ci nor z and sums with +=, where the sweep's sums are fma chains.)
template <int G>
__global__ __launch_bounds__(kRefineThreads) void k_sym_norm1(const int64_t* __restrict__ rp, const double* __restrict__ vf,
                                                              int n, u64* __restrict__ part) {
    __shared__ u64 sm[4];
    const int tid = threadIdx.x, g = tid % G;
    constexpr int kRows = kRefineThreads / G;
    u64 mx = 0;
    for (int64_t row = (int64_t)blockIdx.x * kRows + tid / G; row < n; row += (int64_t)gridDim.x * kRows) {
        double s = 0.0;
        const int64_t e1 = rp[row + 1];
        for (int64_t e = rp[row] + g; e < e1; e += G) s += fabs(vf[e]);
#pragma unroll
        for (int o = G / 2; o; o >>= 1) s += __shfl_xor(s, o);
        mx = max(mx, abs_bits(s));
    }
    const u64 v = block_max(mx, sm);
    if (tid == 0) part[blockIdx.x] = v;
}

// dporfs's constants of a sweep, nz = 1 + the most entries in a row: nz eps, nz safmin, nz safmin / eps.  An Out is an
// aggregate with this one base and
//   u64 operator()(double* dst, bool first, double b, double acc, double den, const double* zp) const
// which stores the row's value to *dst when `first` (one lane of the row) and returns the bits to max-reduce; zp points
// at z[row, column] in the layout the kernel reads.
struct SweepScale {
    double nzeps, safe1, safe2;
};

// 1-4 right-hand sides (z, pb, dst column-major, leading dimension n): G lanes per row split its entries (lane g takes
// g, g + G, ...), a butterfly sums them.  Grid-stride over the rows; partial maxima part[c * gridDim.x + blockIdx.x].
template <int G, int NR, class Out>
__global__ __launch_bounds__(kRefineThreads) void k_sym_sweep(const int64_t* __restrict__ rp, const int* __restrict__ ci,
                                                              const double* __restrict__ vf, const double* __restrict__ z,
                                                              const double* __restrict__ pb, double* __restrict__ dst,
                                                              int n, Out out, u64* __restrict__ part) {
    __shared__ u64 sm[4];
    const int tid = threadIdx.x, g = tid % G;
    constexpr int kRows = kRefineThreads / G;
    u64 mx[NR];
#pragma unroll
    for (int c = 0; c < NR; ++c) mx[c] = 0;
    for (int64_t row = (int64_t)blockIdx.x * kRows + tid / G; row < n; row += (int64_t)gridDim.x * kRows) {
        double acc[NR], den[NR];
#pragma unroll
        for (int c = 0; c < NR; ++c) acc[c] = den[c] = 0.0;
        const int64_t e1 = rp[row + 1];
        for (int64_t e = rp[row] + g; e < e1; e += G) {
            const double a = vf[e];
            const int64_t j = ci[e];
#pragma unroll
            for (int c = 0; c < NR; ++c) {
                const double zj = z[j + (int64_t)c * n];
                acc[c] = fma(a, zj, acc[c]);
                den[c] = fma(fabs(a), fabs(zj), den[c]);
            }
        }
#pragma unroll
        for (int o = G / 2; o; o >>= 1)
#pragma unroll
            for (int c = 0; c < NR; ++c) {
                acc[c] += __shfl_xor(acc[c], o);
                den[c] += __shfl_xor(den[c], o);
            }
#pragma unroll
        for (int c = 0; c < NR; ++c) {
            const int64_t i = row + (int64_t)c * n;
            mx[c] = max(mx[c], out(dst + i, g == 0, pb[i], acc[c], den[c], z + i));
        }
    }
#pragma unroll
    for (int c = 0; c < NR; ++c) {
        const u64 v = block_max(mx[c], sm);
        if (tid == 0) part[(int64_t)c * gridDim.x + blockIdx.x] = v;
    }
}

// Many right-hand sides: L lanes per row, one right-hand side each (column q = blockIdx.y * L + lane), on z staged with
// the right-hand sides of a row contiguous (zt, row stride ldq: k_transpose_x, as the forward solves stage X), so the
// gathers z[j, q0 .. q0 + L) of an entry are one coalesced run.  pb and dst stay column-major.
template <int L, class Out>
__global__ __launch_bounds__(kRefineThreads) void k_sym_sweep_mrhs(const int64_t* __restrict__ rp,
                                                                   const int* __restrict__ ci, const double* __restrict__ vf,
                                                                   const double* __restrict__ zt, int ldq,
                                                                   const double* __restrict__ pb, double* __restrict__ dst,
                                                                   int n, int nrhs, Out out, u64* __restrict__ part) {
    __shared__ u64 sm[4][64];
    const int tid = threadIdx.x, lq = tid % L;
    const int q = (int)blockIdx.y * L + lq;
    const bool on = q < nrhs;
    constexpr int kRows = kRefineThreads / L;
    u64 mx = 0;
    for (int64_t row = (int64_t)blockIdx.x * kRows + tid / L; row < n; row += (int64_t)gridDim.x * kRows) {
        if (!on) continue;
        double acc = 0.0, den = 0.0;
        const int64_t e1 = rp[row + 1];
        for (int64_t e = rp[row]; e < e1; ++e) {
            const double a = vf[e];
            const double zj = zt[(int64_t)ci[e] * ldq + q];
            acc = fma(a, zj, acc);
            den = fma(fabs(a), fabs(zj), den);
        }
        const int64_t i = row + (int64_t)q * n;
        mx = max(mx, out(dst + i, true, pb[i], acc, den, zt + row * ldq + q));
    }
    for (int o = L; o < 64; o <<= 1) mx = max(mx, shfl_xor_u64(mx, o));   // the lanes of one column within the wave
    if ((tid & 63) < L) sm[tid >> 6][tid & 63] = mx;
    __syncthreads();
    if (tid < L && on)
        part[(int64_t)q * gridDim.x + blockIdx.x] = max(max(sm[0][tid], sm[1][tid]), max(sm[2][tid], sm[3][tid]));
}

// f(std::integral_constant<int, V>) for the V of the list that v equals; false: v is not in the list
template <int... Vs, class F>
bool dispatch_int(int v, std::integer_sequence<int, Vs...>, F&& f) {
    return ((v == Vs ? (f(std::integral_constant<int, Vs>()), true) : false) || ...);
}

using SweepGroups = std::integer_sequence<int, 4, 8, 16, 32>;   // RefineState::group

// workgroups of a sweep (grid-stride over the rows) = partials per column
inline int sym_sweep_blocks(int n, int rows_per_block) {
    return (int)std::max<int64_t>(1, std::min<int64_t>(kRefinePartials, ((int64_t)n + rows_per_block - 1) / rows_per_block));
}

// dst = Out of (pb, A z), A's values on the full pattern in vf, and the partial maxima of every column; returns the number
// of partials per column (< 0: error)
template <class Out>
int sym_sweep_enqueue(parsy_plan* pl, const double* vf, const double* z, const double* pb, double* dst, int nrhs, u64* part,
                      hipStream_t stream) {
    const RefineState& R = *pl->refine;
    const int n = pl->S.n;
    const double nz = (double)(R.max_row + 1), safe1 = nz * DBL_MIN;
    const Out out{{nz * 0x1p-53, safe1, safe1 / 0x1p-53}};
    const dim3 threads(kRefineThreads);
    if (nrhs <= 4) {
        const int nb = sym_sweep_blocks(n, kRefineThreads / R.group);
        dispatch_int(R.group, SweepGroups(), [&](auto g) {
            dispatch_int(nrhs, std::integer_sequence<int, 1, 2, 3, 4>(), [&](auto nr) {
                hipLaunchKernelGGL((k_sym_sweep<decltype(g)::value, decltype(nr)::value, Out>), dim3(nb), threads, 0, stream,
                                   R.d_rp, R.d_ci, vf, z, pb, dst, n, out, part);
            });
        });
        PARSY_HIP(hipGetLastError());
        return nb;
    }
    // stage z with the right-hand sides of a row contiguous in the plan's xt (the forward solves' staging buffer: a
    // solve fills it afresh, the sweep runs between solves)
    const int ldq = (nrhs + 15) & ~15;
    PARSY_HIP(pl->xt.grow((int64_t)n * ldq));
    launch_transpose_x(const_cast<double*>(z), n, pl->xt.data(), ldq, n, nrhs, true, stream);
    const int L = nrhs <= 8 ? 8 : nrhs <= 16 ? 16 : nrhs <= 32 ? 32 : 64;
    const int nb = sym_sweep_blocks(n, kRefineThreads / L);
    const dim3 grid(nb, (nrhs + L - 1) / L);
    dispatch_int(L, std::integer_sequence<int, 8, 16, 32, 64>(), [&](auto l) {
        hipLaunchKernelGGL((k_sym_sweep_mrhs<decltype(l)::value, Out>), grid, threads, 0, stream, R.d_rp, R.d_ci, vf,
                           pl->xt.data(), ldq, pb, dst, n, nrhs, out, part);
    });
    PARSY_HIP(hipGetLastError());
    return nb;
}

}  // namespace parsy
