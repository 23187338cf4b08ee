// The factor as an operator on the device (apply.hpp).  The two products stream lValues once per block of kApplyBlock
// right-hand sides, lanes along the rows of a panel (every read of L is a run of 64 consecutive doubles of one column),
// and talk to their second passes through kernel boundaries alone: no flags, no waits, no tickets, no atomics.
//
//   k_apply_l_panels<NB>    T[(chunk, row of lR), q] = sum over the chunk's columns c <= min(i, w - 1), ascending, of
//                           L[i, c] X[c0 + c, q]: a wave per task, a lane per row, X through wave-uniform loads
//   k_apply_l_rows<NB>      Y[perm[row], q] = beta Y + alpha (the row's occurrences in T, ascending): a lane per row
//   k_apply_stage<NB>       xt[k, q] = X[perm[k], q] with the right-hand sides of a row contiguous
//   k_apply_lt_panels<NB>   partial[(segment, column), q] = sum over the segment's rows i >= c of L[i, c] xt[rows[i], q]:
//                           a wave per task, lane l the rows i = l (mod 64) in ascending order, then a butterfly
//   k_apply_lt_cols<NB>     Y[k, q] = beta Y + alpha (the column's partials, ascending): a lane per column
//   k_perm_gather / _scatter  (executor.hip) the orderings around the solves of the inverse operators
//
// NB (1 .. kApplyBlock) is the number of right-hand sides of the block; it changes how many sums a lane carries, never
// the order of one: column q of a call is bitwise what the call with that column alone gives.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../include/parsy_amd.h"
#include "device_util.hpp"
#include "errors.hpp"
#include "hip_check.hpp"
#include "executor.hpp"
#include "plan_util.hpp"
#include "feature_states.hpp"

namespace parsy {

namespace {

constexpr int kAThreads = 256;
constexpr int kAWaves = kAThreads / 64;   // tasks of a workgroup of the panel kernels: a wave each

template <int NB>
__global__ __launch_bounds__(kAThreads) void k_apply_l_panels(const ApplyTaskL* __restrict__ tasks, int64_t ntasks,
                                                              const double* __restrict__ L, const double* __restrict__ X,
                                                              int64_t ldx, double* __restrict__ T) {
    const int lane = threadIdx.x & 63;
    const int64_t task = (int64_t)blockIdx.x * kAWaves + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (task >= ntasks) return;
    const ApplyTaskL K = tasks[task];
    const int i = K.i0 + lane;
    const bool on = i < K.r;
    const int ii = on ? i : K.r - 1;   // (lanes past the panel read its last row and store nothing)
    const int64_t r = K.r;
    const double* __restrict__ g = L + K.px + ii;
    const double* __restrict__ x = X + K.x0;
    double s[NB];
#pragma unroll
    for (int q = 0; q < NB; ++q) s[q] = 0.0;
    // columns that every row of the task has: c <= i0
    const int nfull = min(K.ncol, K.i0 - K.cb + 1);
    int cc = 0;
    for (; cc + 4 <= nfull; cc += 4) {
        const double g0 = g[cc * r], g1 = g[(cc + 1) * r], g2 = g[(cc + 2) * r], g3 = g[(cc + 3) * r];
#pragma unroll
        for (int q = 0; q < NB; ++q) {
            const double* __restrict__ xq = x + cc + q * ldx;
            s[q] = fma(g0, xq[0], s[q]);
            s[q] = fma(g1, xq[1], s[q]);
            s[q] = fma(g2, xq[2], s[q]);
            s[q] = fma(g3, xq[3], s[q]);
        }
    }
    for (; cc < nfull; ++cc) {
        const double g0 = g[cc * r];
#pragma unroll
        for (int q = 0; q < NB; ++q) s[q] = fma(g0, x[cc + q * ldx], s[q]);
    }
    // the triangle of the diagonal block: row i stops at column i; the strict upper triangle is never read
    const int nend = min(K.ncol, K.i0 + 64 - K.cb);
    for (; cc < nend; ++cc) {
        const bool v = K.cb + cc <= ii;
        const double g0 = v ? g[cc * r] : 0.0;
#pragma unroll
        for (int q = 0; q < NB; ++q) s[q] = v ? fma(g0, x[cc + q * ldx], s[q]) : s[q];
    }
    if (on) {
        double* __restrict__ t = T + (K.toff + i) * NB;
#pragma unroll
        for (int q = 0; q < NB; ++q) t[q] = s[q];
    }
}

template <int NB>
__global__ __launch_bounds__(kAThreads) void k_apply_l_rows(const int64_t* __restrict__ ptr, const ApplyOcc* __restrict__ occ,
                                                            const double* __restrict__ T, const int* __restrict__ perm,
                                                            double alpha, double beta, double* __restrict__ Y, int64_t ldy,
                                                            int n) {
    const int row = blockIdx.x * kAThreads + threadIdx.x;
    if (row >= n) return;
    double s[NB];
#pragma unroll
    for (int q = 0; q < NB; ++q) s[q] = 0.0;
    for (int64_t k = ptr[row], e = ptr[row + 1]; k < e; ++k) {
        const ApplyOcc O = occ[k];
        for (int j = 0; j < O.n; ++j) {
            const double* __restrict__ t = T + (O.off + (int64_t)j * O.stride) * NB;
#pragma unroll
            for (int q = 0; q < NB; ++q) s[q] += t[q];
        }
    }
    double* __restrict__ y = Y + (perm ? perm[row] : row);
#pragma unroll
    for (int q = 0; q < NB; ++q) store_y(y + q * ldy, alpha, beta, s[q]);
}

template <int NB>
__global__ __launch_bounds__(kAThreads) void k_apply_stage(const int* __restrict__ perm, const double* __restrict__ X,
                                                           int64_t ldx, int n, double* __restrict__ xt) {
    const int k = blockIdx.x * kAThreads + threadIdx.x;
    if (k >= n) return;
    const double* __restrict__ x = X + (perm ? perm[k] : k);
#pragma unroll
    for (int q = 0; q < NB; ++q) xt[(int64_t)k * NB + q] = x[q * ldx];
}

template <int NB>
__global__ __launch_bounds__(kAThreads) void k_apply_lt_panels(const ApplyTaskLt* __restrict__ tasks, int64_t ntasks,
                                                               const int32_t* __restrict__ rows, const double* __restrict__ L,
                                                               const double* __restrict__ xt, double* __restrict__ P) {
    const int lane = threadIdx.x & 63;
    const int64_t task = (int64_t)blockIdx.x * kAWaves + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (task >= ntasks) return;
    const ApplyTaskLt K = tasks[task];
    const int64_t r = K.r;
    const double* __restrict__ g = L + K.px;
    double s[kApplyCols][NB];
#pragma unroll
    for (int u = 0; u < kApplyCols; ++u)
#pragma unroll
        for (int q = 0; q < NB; ++q) s[u][q] = 0.0;
    for (int b = K.i0; b < K.i1; b += 64) {
        const int i = b + lane;
        const bool on = i < K.i1;
        const int ii = on ? i : K.i1 - 1;
        const double* __restrict__ xr = xt + (int64_t)rows[K.pi + ii] * NB;
        double xv[NB];
#pragma unroll
        for (int q = 0; q < NB; ++q) xv[q] = xr[q];
#pragma unroll
        for (int u = 0; u < kApplyCols; ++u) {
            if (u < K.nc) {
                const bool v = on && K.c + u <= i;   // column c holds the rows i >= c
                const double g0 = v ? g[u * r + ii] : 0.0;
#pragma unroll
                for (int q = 0; q < NB; ++q) s[u][q] = v ? fma(g0, xv[q], s[u][q]) : s[u][q];
            }
        }
    }
#pragma unroll
    for (int u = 0; u < kApplyCols; ++u) {
        if (u < K.nc) {
#pragma unroll
            for (int q = 0; q < NB; ++q) {
                double v = s[u][q];
#pragma unroll
                for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o);
                if (lane == 0) P[(K.poff + u) * NB + q] = v;
            }
        }
    }
}

template <int NB>
__global__ __launch_bounds__(kAThreads) void k_apply_lt_cols(const ApplyCol* __restrict__ col, const double* __restrict__ P,
                                                             double alpha, double beta, double* __restrict__ Y, int64_t ldy,
                                                             int n) {
    const int k = blockIdx.x * kAThreads + threadIdx.x;
    if (k >= n) return;
    const ApplyCol C = col[k];
    double s[NB];
#pragma unroll
    for (int q = 0; q < NB; ++q) s[q] = 0.0;
    for (int j = 0; j < C.n; ++j) {
        const double* __restrict__ p = P + (C.off + (int64_t)j * C.stride) * NB;
#pragma unroll
        for (int q = 0; q < NB; ++q) s[q] += p[q];
    }
#pragma unroll
    for (int q = 0; q < NB; ++q) store_y(Y + k + q * ldy, alpha, beta, s[q]);
}

int ensure_device(parsy_plan* pl) {
    if (apply_ensure_host(pl) != 0) return -1;
    ApplyState& A = *pl->apply;
    PARSY_HIP(hipSetDevice(pl->device));
    if (A.on_device) return 0;
    DevicePool pool(&A.meter);
    int64_t* d_ptr = pool.upload(A.I.ptr);
    ApplyOcc* d_occ = pool.upload(A.A.occ);
    ApplyTaskL* d_l_tasks = pool.upload(A.A.l_tasks);
    ApplyTaskLt* d_lt_tasks = pool.upload(A.A.lt_tasks);
    ApplyCol* d_col = pool.upload(A.A.col);
    if (pool.error() != hipSuccess) return pool_failed(pool);
    A.index = std::move(pool);
    A.d_ptr = d_ptr, A.d_occ = d_occ, A.d_l_tasks = d_l_tasks, A.d_lt_tasks = d_lt_tasks, A.d_col = d_col;
    A.on_device = true;
    A.I = ApplyIndex{{}, {}, A.I.max_occurrences};   // (the host copies have served; the counts stay)
    A.A = ApplyLayout();
    return 0;
}

unsigned blocks_of(int64_t items, int per_block) { return (unsigned)std::max<int64_t>(1, (items + per_block - 1) / per_block); }

#define APPLY_NB(NBV, CALL)       \
    switch (NBV) {                \
        case 1: CALL(1); break;   \
        case 2: CALL(2); break;   \
        case 3: CALL(3); break;   \
        case 4: CALL(4); break;   \
        case 5: CALL(5); break;   \
        case 6: CALL(6); break;   \
        case 7: CALL(7); break;   \
        default: CALL(8); break;  \
    }
static_assert(kApplyBlock == 8, "APPLY_NB lists the instantiations 1 .. kApplyBlock");

}  // namespace

int apply_ensure_host(parsy_plan* pl) {
    if (!pl->apply) pl->apply = std::make_unique<ApplyState>(&pl->meter);
    ApplyState& A = *pl->apply;
    if (A.built) return 0;
    build_apply_index(pl->S, A.I);
    build_apply_layout(pl->S, A.I, A.A);
    A.ws_need = apply_workspace_len(pl->S, A.A);
    A.n_l_tasks = (int64_t)A.A.l_tasks.size();
    A.n_lt_tasks = (int64_t)A.A.lt_tasks.size();
    A.built = true;
    return 0;
}

int apply_check_args(const parsy_plan* pl, const char* who, const void* lValues, int op, const void* x, int ldx, int nrhs,
                     const void* y, int ldy) {
    const std::string w(who);
    if (!pl || !lValues || !x || !y) return set_last_error(w + ": null argument"), -1;
    if (pl->device < 0) return set_last_error(w + ": plan was built without a device (device < 0)"), -1;
    if (nrhs < 1) return set_last_error(w + ": need nrhs >= 1"), -1;
    if (ldx < pl->S.n || ldy < pl->S.n) return set_last_error(w + ": need leading dimensions ldx >= n and ldy >= n"), -1;
    if (op < PARSY_OP_G || op > PARSY_OP_GINVT) return set_last_error(w + ": op must be one of PARSY_OP_G .. PARSY_OP_GINVT (0 .. 3)"), -1;
    if (x == y) return set_last_error(w + ": x and y are the same array (in place is not supported)"), -1;
    return 0;
}

int plan_factor_apply(parsy_plan* pl, const double* d_L, int op, const double* d_x, int ldx, int nrhs, double alpha,
                      double beta, double* d_y, int ldy, void* stream_) {
    const char* who = "parsy_factor_apply_device";
    hipStream_t stream = (hipStream_t)stream_;
    if (apply_check_args(pl, who, d_L, op, d_x, ldx, nrhs, d_y, ldy) != 0) return -1;
    const int* perm = nullptr;
    if (ensure_device(pl) != 0 || plan_perm_device(pl, &perm) != 0) return -1;
    ApplyState& A = *pl->apply;
    const int n = pl->S.n;
    A.last_op = op;
    A.last_launches = 0;
    if (n == 0) return 0;
    const dim3 threads(kAThreads);
    const unsigned nblocks = blocks_of(n, kAThreads);
    if (op == PARSY_OP_GINV || op == PARSY_OP_GINVT) {
        PARSY_HIP(A.sol.grow((int64_t)n * nrhs));
        double* const sol = A.sol.data();
        const bool back = op == PARSY_OP_GINVT;
        enqueue_perm_gather(back ? nullptr : perm, d_x, ldx, sol, nullptr, n, nrhs, stream);
        PARSY_HIP(hipGetLastError());
        if ((back ? plan_backsolve(pl, d_L, sol, nrhs, n, stream) : plan_solve(pl, d_L, sol, nrhs, n, stream)) != 0)
            return -1;
        enqueue_perm_scatter(back ? perm : nullptr, sol, alpha, beta, d_y, ldy, n, nrhs, stream);
        PARSY_HIP(hipGetLastError());
        A.last_launches = 2;   // (besides the solve's own)
        return 0;
    }
    PARSY_HIP(A.ws.grow(A.ws_need));
    double* const ws = A.ws.data();
    for (int q0 = 0; q0 < nrhs; q0 += kApplyBlock) {
        const int nb = std::min(kApplyBlock, nrhs - q0);
        const double* x = d_x + (int64_t)q0 * ldx;
        double* y = d_y + (int64_t)q0 * ldy;
        if (op == PARSY_OP_G) {
            if (A.n_l_tasks > 0) {
#define APPLY_L_PANELS(NN)                                                                                              \
    hipLaunchKernelGGL(k_apply_l_panels<NN>, dim3(blocks_of(A.n_l_tasks, kAWaves)), threads, 0, stream, A.d_l_tasks, \
                       A.n_l_tasks, d_L, x, (int64_t)ldx, ws)
                APPLY_NB(nb, APPLY_L_PANELS)
#undef APPLY_L_PANELS
                ++A.last_launches;
            }
#define APPLY_L_ROWS(NN)                                                                                                  \
    hipLaunchKernelGGL(k_apply_l_rows<NN>, dim3(nblocks), threads, 0, stream, A.d_ptr, A.d_occ, ws, perm, alpha, beta, y, \
                       (int64_t)ldy, n)
            APPLY_NB(nb, APPLY_L_ROWS)
#undef APPLY_L_ROWS
            ++A.last_launches;
        } else {
            double* xt = ws + A.ws_need - (int64_t)n * kApplyBlock;   // (the last n rows of the workspace, behind the partials)
#define APPLY_STAGE(NN) hipLaunchKernelGGL(k_apply_stage<NN>, dim3(nblocks), threads, 0, stream, perm, x, (int64_t)ldx, n, xt)
            APPLY_NB(nb, APPLY_STAGE)
#undef APPLY_STAGE
            ++A.last_launches;
            if (A.n_lt_tasks > 0) {
#define APPLY_LT_PANELS(NN)                                                                                                \
    hipLaunchKernelGGL(k_apply_lt_panels<NN>, dim3(blocks_of(A.n_lt_tasks, kAWaves)), threads, 0, stream, A.d_lt_tasks, \
                       A.n_lt_tasks, pl->dp.rows, d_L, xt, ws)
                APPLY_NB(nb, APPLY_LT_PANELS)
#undef APPLY_LT_PANELS
                ++A.last_launches;
            }
#define APPLY_LT_COLS(NN) \
    hipLaunchKernelGGL(k_apply_lt_cols<NN>, dim3(nblocks), threads, 0, stream, A.d_col, ws, alpha, beta, y, (int64_t)ldy, n)
            APPLY_NB(nb, APPLY_LT_COLS)
#undef APPLY_LT_COLS
            ++A.last_launches;
        }
        PARSY_HIP(hipGetLastError());
    }
    return 0;
}

}  // namespace parsy
