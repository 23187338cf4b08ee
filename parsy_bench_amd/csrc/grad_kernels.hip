// Gradients with respect to the values of A on the device (grad.hpp): everything is a gather and a fixed-order sum over
// the pattern of A in A2 order, one writer per output entry and no atomics, so every result is bitwise reproducible.
//
//   k_pattern_outer<NR>       g[q] = beta g[q] + alpha S_q, S_q = sum_k lam[i,k] x[j,k] + lam[j,k] x[i,k] (one term on the
//                             diagonal): one thread per entry, row / col / g coalesced, the vectors gathered from the
//                             caller's arrays through the plan's ordering.  Few right-hand sides.
//   k_pattern_stage           P lam and P x with the right-hand sides of a row contiguous (an LDS tile transpose), then
//   k_pattern_outer_mrhs<L>   L lanes per entry, lane l takes the right-hand sides l, l + L, ...: each of the four operand
//                             reads of an entry is one coalesced run; a butterfly leaves every lane with the sum.
//   k_inverse_pattern         g[q] = beta g[q] + alpha w_q Z[a_dst[q]]  (w_q = 2 off the diagonal, 1 on it or when PLAIN)
//   k_trace_part / _final     tr(A^-1 B_m) = sum_q w_q Z[a_dst[q]] B_m[q]: fixed ranges and a fixed tree, as the
//                             log-determinant (selinv_kernels.hip).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../include/parsy_amd.h"
#include "errors.hpp"
#include "hip_check.hpp"
#include "executor.hpp"
#include "plan_util.hpp"
#include "feature_states.hpp"

namespace parsy {

namespace {

constexpr int kGThreads = 256;
constexpr int kGridCap = 1024;      // workgroups of the grid-stride kernels: 4 per CU
constexpr int kTraceParts = 256;    // workgroups (= partials) per matrix of the trace's first pass
constexpr int kStage = 32;          // rows x right-hand sides of a staging tile

__device__ __forceinline__ void store_g(double* __restrict__ g, int64_t q, double alpha, double beta, double s) {
    g[q] = beta == 0.0 ? alpha * s : fma(beta, g[q], alpha * s);   // beta == 0: g is not read (it may hold NaN)
}

// NR right-hand sides when NR > 0 (unrolled), nrhs of them when NR == 0
template <int NR>
__global__ __launch_bounds__(kGThreads) void k_pattern_outer(const int32_t* __restrict__ row, const int32_t* __restrict__ col,
                                                             const int* __restrict__ perm, const double* __restrict__ lam,
                                                             int64_t ldl, const double* __restrict__ x, int64_t ldx,
                                                             int nrhs, double alpha, double beta, double* __restrict__ g,
                                                             int64_t nnz) {
    const int nr = NR > 0 ? NR : nrhs;
    for (int64_t q = (int64_t)blockIdx.x * kGThreads + threadIdx.x; q < nnz; q += (int64_t)gridDim.x * kGThreads) {
        const int i = row[q], j = col[q];
        const bool off = i != j;
        const int64_t pi = perm ? perm[i] : i, pj = perm ? perm[j] : j;
        double s = 0.0;
#pragma unroll
        for (int k = 0; k < nr; ++k) {
            const double li = lam[pi + k * ldl], xj = x[pj + k * ldx];
            const double lj = lam[pj + k * ldl], xi = x[pi + k * ldx];
            s = fma(li, xj, s);
            s = off ? fma(lj, xi, s) : s;
        }
        store_g(g, q, alpha, beta, s);
    }
}

// dst[which][i * pitch + k] = src[which][perm[i] + k * ld]  (which = blockIdx.z: lambda, x); the columns nrhs .. pitch of a
// row are never read
__global__ __launch_bounds__(kGThreads) void k_pattern_stage(const int* __restrict__ perm, const double* __restrict__ lam,
                                                             int64_t ldl, const double* __restrict__ x, int64_t ldx, int n,
                                                             int nrhs, int pitch, double* __restrict__ ws) {
    __shared__ double tile[kStage][kStage + 1];
    const double* __restrict__ src = blockIdx.z ? x : lam;
    const int64_t ld = blockIdx.z ? ldx : ldl;
    double* __restrict__ dst = ws + (int64_t)blockIdx.z * n * pitch;
    const int i0 = blockIdx.x * kStage, k0 = blockIdx.y * kStage;
    const int tx = threadIdx.x % kStage, ty = threadIdx.x / kStage;   // ty < 8
    const int i = i0 + tx;
    const int64_t pi = i < n ? (perm ? perm[i] : i) : 0;
    for (int kk = ty; kk < kStage; kk += kGThreads / kStage)
        if (i < n && k0 + kk < nrhs) tile[kk][tx] = src[pi + (int64_t)(k0 + kk) * ld];
    __syncthreads();
    for (int ii = ty; ii < kStage; ii += kGThreads / kStage)
        if (i0 + ii < n && k0 + tx < nrhs) dst[(int64_t)(i0 + ii) * pitch + k0 + tx] = tile[tx][ii];
}

template <int L>
__global__ __launch_bounds__(kGThreads) void k_pattern_outer_mrhs(const int32_t* __restrict__ row,
                                                                  const int32_t* __restrict__ col,
                                                                  const double* __restrict__ lt, const double* __restrict__ xt,
                                                                  int pitch, int nrhs, double alpha, double beta,
                                                                  double* __restrict__ g, int64_t nnz) {
    constexpr int kEntries = kGThreads / L;
    const int l = threadIdx.x % L;
    // (every lane of a wave runs the same number of turns: the butterfly needs them all)
    for (int64_t q0 = (int64_t)blockIdx.x * kEntries; q0 < nnz; q0 += (int64_t)gridDim.x * kEntries) {
        const int64_t q = q0 + threadIdx.x / L;
        const int64_t qc = q < nnz ? q : nnz - 1;
        const int i = row[qc], j = col[qc];
        const bool off = i != j;
        const double* __restrict__ li = lt + (int64_t)i * pitch;
        const double* __restrict__ lj = lt + (int64_t)j * pitch;
        const double* __restrict__ xi = xt + (int64_t)i * pitch;
        const double* __restrict__ xj = xt + (int64_t)j * pitch;
        double s = 0.0;
        for (int k = l; k < nrhs; k += L) {
            s = fma(li[k], xj[k], s);
            s = off ? fma(lj[k], xi[k], s) : s;
        }
#pragma unroll
        for (int o = L / 2; o; o >>= 1) s += __shfl_xor(s, o);
        if (l == 0 && q < nnz) store_g(g, q, alpha, beta, s);
    }
}

__global__ __launch_bounds__(kGThreads) void k_inverse_pattern(const int32_t* __restrict__ row, const int32_t* __restrict__ col,
                                                               const int64_t* __restrict__ dst, const double* __restrict__ Z,
                                                               double alpha, double beta, int plain, double* __restrict__ g,
                                                               int64_t nnz) {
    for (int64_t q = (int64_t)blockIdx.x * kGThreads + threadIdx.x; q < nnz; q += (int64_t)gridDim.x * kGThreads) {
        const double w = (plain || row[q] == col[q]) ? 1.0 : 2.0;
        store_g(g, q, alpha, beta, w * Z[dst[q]]);
    }
}

// First pass: workgroup (b, m) sums w_q Z[dst[q]] B_m[q] over its contiguous range of entries (fixed lane split and tree).
__global__ __launch_bounds__(kGThreads) void k_trace_part(const int32_t* __restrict__ row, const int32_t* __restrict__ col,
                                                          const int64_t* __restrict__ dst, const double* __restrict__ Z,
                                                          const double* __restrict__ B, int64_t ldb, int64_t nnz,
                                                          double* __restrict__ part) {
    __shared__ double ss[kGThreads];
    const int64_t per = (nnz + gridDim.x - 1) / gridDim.x, lo = blockIdx.x * per, hi = lo + per < nnz ? lo + per : nnz;
    const double* __restrict__ Bm = B + (int64_t)blockIdx.y * ldb;
    double s = 0.0;
    for (int64_t q = lo + threadIdx.x; q < hi; q += kGThreads) {
        const double w = row[q] == col[q] ? 1.0 : 2.0;
        s = fma(w * Z[dst[q]], Bm[q], s);
    }
    ss[threadIdx.x] = s;
    __syncthreads();
    for (int o = kGThreads / 2; o; o >>= 1) {
        if (threadIdx.x < o) ss[threadIdx.x] += ss[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) part[(int64_t)blockIdx.y * gridDim.x + blockIdx.x] = ss[0];
}

// Second pass: matrix m's partials in order.
__global__ void k_trace_final(const double* __restrict__ part, int nparts, int nb, double* __restrict__ out) {
    const int m = blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= nb) return;
    double s = 0.0;
    for (int b = 0; b < nparts; ++b) s += part[(int64_t)m * nparts + b];
    out[m] = s;
}

int ensure_host_pattern(parsy_plan* pl, const char* who) {
    if (!pl->grad) pl->grad = std::make_unique<GradState>(&pl->meter);
    GradState& G = *pl->grad;
    if (G.built) return 0;
    std::string what;
    if (!build_grad_pattern(pl->S, G.P, what)) return set_last_error(std::string(who) + ": " + what), -1;
    G.built = true;
    return 0;
}

int ensure_device_pattern(parsy_plan* pl, const char* who) {
    if (ensure_host_pattern(pl, who) != 0) return -1;
    GradState& G = *pl->grad;
    PARSY_HIP(hipSetDevice(pl->device));
    if (G.on_device) return 0;
    DevicePool pool(&G.meter);
    int32_t *d_row = pool.upload(G.P.row), *d_col = pool.upload(G.P.col);
    if (pool.error() != hipSuccess) return pool_failed(pool);
    G.pattern = std::move(pool);
    G.d_row = d_row, G.d_col = d_col;
    G.on_device = true;
    std::vector<int32_t>().swap(G.P.row);   // (the host copy has served; the counts stay)
    std::vector<int32_t>().swap(G.P.col);
    return 0;
}

unsigned capped_grid(int64_t items, int per_block) {
    return (unsigned)std::max<int64_t>(1, std::min<int64_t>(kGridCap, (items + per_block - 1) / per_block));
}

}  // namespace

int plan_pattern_outer(parsy_plan* pl, const double* d_lam, int ldl, const double* d_x, int ldx, int nrhs, double alpha,
                       double beta, double* d_g, hipStream_t stream) {
    const char* who = "parsy_pattern_outer_device";
    if (check_plan(pl, who, kNeedsA) != 0) return -1;
    const int n = pl->S.n;
    if (nrhs < 1 || ldl < n || ldx < n)
        return set_last_error(std::string(who) + ": need nrhs >= 1 and leading dimensions >= n"), -1;
    if (nrhs > 65535 * kStage)   // (the staging kernel's grid)
        return set_last_error(std::string(who) + ": too many right-hand sides (nrhs <= 2097120)"), -1;
    const int* perm = nullptr;
    if (ensure_device_pattern(pl, who) != 0 || plan_perm_device(pl, &perm) != 0) return -1;
    GradState& G = *pl->grad;
    const int64_t nnz = pl->S.nnzA;
    if (nrhs < grad_mrhs_min()) {
        G.last_lanes = 1;
        if (nnz == 0) return 0;
        const dim3 grid(capped_grid(nnz, kGThreads));
#define G_DIRECT(NN)                                                                                                  \
    hipLaunchKernelGGL(k_pattern_outer<NN>, grid, dim3(kGThreads), 0, stream, G.d_row, G.d_col, perm, d_lam, (int64_t)ldl, \
                       d_x, (int64_t)ldx, nrhs, alpha, beta, d_g, nnz)
        switch (nrhs) {
            case 1: G_DIRECT(1); break;
            case 2: G_DIRECT(2); break;
            case 3: G_DIRECT(3); break;
            case 4: G_DIRECT(4); break;
            default: G_DIRECT(0); break;
        }
#undef G_DIRECT
        PARSY_HIP(hipGetLastError());
        return 0;
    }
    const int L = nrhs <= 8 ? 8 : nrhs <= 16 ? 16 : nrhs <= 32 ? 32 : 64;
    G.last_lanes = L;
    if (nnz == 0) return 0;
    const int pitch = (nrhs + 7) & ~7;
    const int64_t half = (int64_t)n * pitch;
    PARSY_HIP(G.ws.grow(2 * half));
    double* const ws = G.ws.data();
    const unsigned ky = (unsigned)((nrhs + kStage - 1) / kStage);
    hipLaunchKernelGGL(k_pattern_stage, dim3((unsigned)((n + kStage - 1) / kStage), ky, 2), dim3(kGThreads), 0, stream, perm,
                       d_lam, (int64_t)ldl, d_x, (int64_t)ldx, n, nrhs, pitch, ws);
    const dim3 grid(capped_grid(nnz, kGThreads / L));
#define G_MRHS(LL)                                                                                                    \
    if (L == LL)                                                                                                      \
        hipLaunchKernelGGL(k_pattern_outer_mrhs<LL>, grid, dim3(kGThreads), 0, stream, G.d_row, G.d_col, ws, ws + half, \
                           pitch, nrhs, alpha, beta, d_g, nnz);
    G_MRHS(8) G_MRHS(16) G_MRHS(32) G_MRHS(64)
#undef G_MRHS
    PARSY_HIP(hipGetLastError());
    return 0;
}

int plan_inverse_pattern(parsy_plan* pl, const double* d_z, double alpha, double beta, int flags, double* d_g,
                         hipStream_t stream) {
    const char* who = "parsy_inverse_pattern_device";
    if (check_plan(pl, who, kNeedsA) != 0 || ensure_device_pattern(pl, who) != 0) return -1;
    GradState& G = *pl->grad;
    const int64_t nnz = pl->S.nnzA;
    if (nnz == 0) return 0;
    hipLaunchKernelGGL(k_inverse_pattern, dim3(capped_grid(nnz, kGThreads)), dim3(kGThreads), 0, stream, G.d_row, G.d_col,
                       pl->dp.a_dst, d_z, alpha, beta, flags & PARSY_PATTERN_PLAIN, d_g, nnz);
    PARSY_HIP(hipGetLastError());
    return 0;
}

int plan_trace_inverse(parsy_plan* pl, const double* d_z, const double* d_b, int64_t ldb, int nb, double* out,
                       hipStream_t stream) {
    const char* who = "parsy_trace_inverse_device";
    if (check_plan(pl, who, kNeedsA) != 0) return -1;
    const int64_t nnz = pl->S.nnzA;
    if (nb < 1 || nb > 65535 || ldb < nnz)
        return set_last_error(std::string(who) + ": need 1 <= nb <= 65535 and ldb >= nnz(A)"), -1;
    if (ensure_device_pattern(pl, who) != 0) return -1;
    GradState& G = *pl->grad;
    const int nparts = (int)std::max<int64_t>(1, std::min<int64_t>(kTraceParts, (nnz + kGThreads - 1) / kGThreads));
    PARSY_HIP(G.tpart.grow((int64_t)nb * (nparts + 1)));
    double* const tpart = G.tpart.data();
    double* res = tpart + (int64_t)nb * nparts;
    hipLaunchKernelGGL(k_trace_part, dim3(nparts, nb), dim3(kGThreads), 0, stream, G.d_row, G.d_col, pl->dp.a_dst, d_z, d_b,
                       ldb, nnz, tpart);
    hipLaunchKernelGGL(k_trace_final, dim3((nb + 63) / 64), dim3(64), 0, stream, tpart, nparts, nb, res);
    PARSY_HIP(hipGetLastError());
    PARSY_HIP(hipMemcpyAsync(out, res, (size_t)nb * 8, hipMemcpyDeviceToHost, stream));
    PARSY_HIP(hipStreamSynchronize(stream));
    return 0;
}

}  // namespace parsy

using parsy::set_last_error;

extern "C" {

int parsy_grad_get_info(parsy_plan* pl, parsy_grad_info* info) {
    if (!pl || !info) {
        set_last_error("parsy_grad_get_info: null argument");
        return -1;
    }
    info->entries = info->offdiag_entries = info->device_bytes = 0;
    info->last_lanes = 0;
    if (pl->solve_only) return 0;
    if (parsy::ensure_host_pattern(pl, "parsy_grad_get_info") != 0) return -1;
    const parsy::GradState& G = *pl->grad;
    info->entries = pl->S.nnzA;
    info->offdiag_entries = G.P.offdiag;
    info->device_bytes = G.meter.bytes;
    info->last_lanes = G.last_lanes;
    return 0;
}

int parsy_pattern_outer_device(parsy_plan* pl, const double* d_lam, int ldl, const double* d_x, int ldx, int nrhs,
                               double alpha, double beta, double* d_g, void* stream) {
    if (!pl || !d_lam || !d_x || !d_g) {
        set_last_error("parsy_pattern_outer_device: null argument");
        return -1;
    }
    return parsy::plan_pattern_outer(pl, d_lam, ldl, d_x, ldx, nrhs, alpha, beta, d_g, (hipStream_t)stream);
}

int parsy_inverse_pattern_device(parsy_plan* pl, const double* d_z, double alpha, double beta, int flags, double* d_g,
                                 void* stream) {
    if (!pl || !d_z || !d_g) {
        set_last_error("parsy_inverse_pattern_device: null argument");
        return -1;
    }
    return parsy::plan_inverse_pattern(pl, d_z, alpha, beta, flags, d_g, (hipStream_t)stream);
}

int parsy_trace_inverse_device(parsy_plan* pl, const double* d_z, const double* d_bvalues, int64_t ldb, int nb,
                               double* out, void* stream) {
    if (!pl || !d_z || !d_bvalues || !out) {
        set_last_error("parsy_trace_inverse_device: null argument");
        return -1;
    }
    return parsy::plan_trace_inverse(pl, d_z, d_bvalues, ldb, nb, out, (hipStream_t)stream);
}

}  // extern "C"
