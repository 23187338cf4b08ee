// Normal matrices on the plan's pattern (normal.hpp): N = F diag(w) F' + beta I + A0 in A2 order, the products by F and
// F', least squares through the factor.  gfx950, wave64.  No flags, tickets, spin-waits or float atomics: the stream is
// the only order between launches, and every sum has one order fixed by the pattern.
//
//   values   per class of list lengths one launch of k_normal_values<LANES>: the LANES lanes of an entry stride its list
//            (consecutive lanes read consecutive words of the three triple arrays), one fma chain each, folded by a
//            butterfly.  Lists above kNormalChunk: one wave per chunk writes a partial (k_normal_values_chunks), a thread
//            per entry adds its partials in chunk order (k_normal_values_fold).  Every entry of the pattern is written.
//   F' X     a thread per column of F gathers down the column (k_normal_ft<NR>).
//   F W X    a thread per row of F gathers along the transposed index in ascending position (k_normal_f<NR>).
//            Both keep NR <= kNormalBlock accumulators, one fma chain per right-hand side: a column's bits do not depend
//            on the columns beside it.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "../../include/parsy_amd.h"
#include "device_util.hpp"
#include "errors.hpp"
#include "executor.hpp"
#include "feature_states.hpp"
#include "hip_check.hpp"
#include "normal.hpp"
#include "plan_util.hpp"

namespace parsy {

namespace {

constexpr int kNThreads = 256;
constexpr int kNWaves = kNThreads / 64;

// one term chain of a lane: t = t0, t0 + step, ... below t1
__device__ __forceinline__ double normal_chain(const int32_t* __restrict__ ta, const int32_t* __restrict__ tb,
                                               const int32_t* __restrict__ tk, const double* __restrict__ fx,
                                               const double* __restrict__ w, int64_t t0, int64_t t1, int step) {
    double acc = 0.0;
    if (w) {
        for (int64_t t = t0; t < t1; t += step) acc = fma(fx[ta[t]] * w[tk[t]], fx[tb[t]], acc);
    } else {
        for (int64_t t = t0; t < t1; t += step) acc = fma(fx[ta[t]], fx[tb[t]], acc);
    }
    return acc;
}

// v = ((s + beta on the diagonal) + A0[q]); base may be the array values is
__device__ __forceinline__ void normal_store(double s, int64_t q, const uint8_t* __restrict__ diag, double beta,
                                             const double* base, double* values) {
    if (diag[q]) s += beta;
    if (base) s += base[q];
    values[q] = s;
}

template <int LANES>
__global__ __launch_bounds__(kNThreads) void k_normal_values(const int32_t* __restrict__ entries, int64_t count,
                                                             const int64_t* __restrict__ lptr,
                                                             const int32_t* __restrict__ ta, const int32_t* __restrict__ tb,
                                                             const int32_t* __restrict__ tk, const double* __restrict__ fx,
                                                             const double* __restrict__ w, double beta,
                                                             const uint8_t* __restrict__ diag, const double* base,
                                                             double* values) {
    const int64_t tid = (int64_t)blockIdx.x * kNThreads + threadIdx.x;
    const int64_t e = tid / LANES;
    const int lane = (int)(tid % LANES);
    const bool live = e < count;   // (a dead lane takes part in the butterfly with a zero)
    const int64_t q = live ? entries[e] : 0;
    double acc = 0.0;
    if (live) acc = normal_chain(ta, tb, tk, fx, w, lptr[q] + lane, lptr[q + 1], LANES);
#pragma unroll
    for (int o = LANES / 2; o; o >>= 1) acc += __shfl_xor(acc, o);
    if (live && lane == 0) normal_store(acc, q, diag, beta, base, values);
}

__global__ __launch_bounds__(kNThreads) void k_normal_values_chunks(const int64_t* __restrict__ chunk_off,
                                                                    const int32_t* __restrict__ chunk_len, int64_t chunks,
                                                                    const int32_t* __restrict__ ta,
                                                                    const int32_t* __restrict__ tb,
                                                                    const int32_t* __restrict__ tk,
                                                                    const double* __restrict__ fx,
                                                                    const double* __restrict__ w, double* __restrict__ part) {
    const int64_t c = (int64_t)blockIdx.x * kNWaves + threadIdx.x / 64;
    const int lane = threadIdx.x % 64;
    if (c >= chunks) return;   // (a whole wave)
    const int64_t t0 = chunk_off[c];
    double acc = normal_chain(ta, tb, tk, fx, w, t0 + lane, t0 + chunk_len[c], 64);
#pragma unroll
    for (int o = 32; o; o >>= 1) acc += __shfl_xor(acc, o);
    if (lane == 0) part[c] = acc;
}

__global__ __launch_bounds__(kNThreads) void k_normal_values_fold(const int32_t* __restrict__ fold_q,
                                                                  const int32_t* __restrict__ fold_ptr, int64_t count,
                                                                  const double* __restrict__ part, double beta,
                                                                  const uint8_t* __restrict__ diag, const double* base,
                                                                  double* values) {
    const int64_t f = (int64_t)blockIdx.x * kNThreads + threadIdx.x;
    if (f >= count) return;
    double s = 0.0;
    for (int32_t c = fold_ptr[f]; c < fold_ptr[f + 1]; ++c) s += part[c];
    normal_store(s, fold_q[f], diag, beta, base, values);
}

// Y[k, q] = beta_y Yin[k, q] + alpha sum_p fx[p] X[fi[p], q] over column k of F
template <int NR>
__global__ __launch_bounds__(kNThreads) void k_normal_ft(const int32_t* __restrict__ fp, const int32_t* __restrict__ fi,
                                                         const double* __restrict__ fx, int m, const double* __restrict__ x,
                                                         int64_t ldx, double alpha, double beta_y, const double* yin,
                                                         int64_t ldin, double* y, int64_t ldy) {
    const int64_t k = (int64_t)blockIdx.x * kNThreads + threadIdx.x;
    if (k >= m) return;
    double acc[NR];
#pragma unroll
    for (int q = 0; q < NR; ++q) acc[q] = 0.0;
    for (int p = fp[k]; p < fp[k + 1]; ++p) {
        const double f = fx[p];
        const double* xr = x + fi[p];
#pragma unroll
        for (int q = 0; q < NR; ++q) acc[q] = fma(f, xr[q * ldx], acc[q]);
    }
#pragma unroll
    for (int q = 0; q < NR; ++q)
        y[k + q * ldy] = beta_y == 0.0 ? alpha * acc[q] : fma(beta_y, yin[k + q * ldin], alpha * acc[q]);
}

// Y[rowmap[i], q] = beta_y Yin[i, q] + alpha sum_t (fx[p] w[k]) X[k, q] over row i of F, (p, k) = (rpos[t], rcol[t])
template <int NR>
__global__ __launch_bounds__(kNThreads) void k_normal_f(const int64_t* __restrict__ rptr, const int32_t* __restrict__ rpos,
                                                        const int32_t* __restrict__ rcol, const double* __restrict__ fx,
                                                        const double* __restrict__ w, int n, const double* __restrict__ x,
                                                        int64_t ldx, double alpha, double beta_y, const double* yin,
                                                        int64_t ldin, const int* __restrict__ rowmap, double* y,
                                                        int64_t ldy) {
    const int64_t i = (int64_t)blockIdx.x * kNThreads + threadIdx.x;
    if (i >= n) return;
    double acc[NR];
#pragma unroll
    for (int q = 0; q < NR; ++q) acc[q] = 0.0;
    for (int64_t t = rptr[i]; t < rptr[i + 1]; ++t) {
        const int k = rcol[t];
        const double f = w ? fx[rpos[t]] * w[k] : fx[rpos[t]];
        const double* xr = x + k;
#pragma unroll
        for (int q = 0; q < NR; ++q) acc[q] = fma(f, xr[q * ldx], acc[q]);
    }
    const int64_t o = rowmap ? rowmap[i] : i;
#pragma unroll
    for (int q = 0; q < NR; ++q)
        y[o + q * ldy] = beta_y == 0.0 ? alpha * acc[q] : fma(beta_y, yin[i + q * ldin], alpha * acc[q]);
}

// ctl = -1 once a solve has left a negative status word
__global__ void k_normal_note_status(const int* __restrict__ word, int* __restrict__ ctl) {
    if (threadIdx.x == 0 && *word < 0) *ctl = -1;
}
// ... and the last solve's word takes it over, for parsy_solve_status
__global__ void k_normal_put_status(const int* __restrict__ ctl, int* __restrict__ word) {
    if (threadIdx.x == 0 && *ctl < 0) *word = -1;
}

unsigned blocks_of(int64_t items, int per_block) { return (unsigned)std::max<int64_t>(1, (items + per_block - 1) / per_block); }

#define NORMAL_NB(NBV, CALL)      \
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
static_assert(kNormalBlock == 8, "NORMAL_NB lists the instantiations 1 .. kNormalBlock");

int refuse(const char* who, const std::string& what) {
    set_last_error(std::string(who) + ": " + what);
    return -1;
}

// the whole index on the device, on the handle's first device call
int ensure_device(parsy_normal* h) {
    NormalState& D = h->dev;
    if (D.on_device) return 0;
    const NormalIndex& I = h->I;
    PARSY_HIP(hipSetDevice(h->plan->device));
    DevicePool pool(&D.meter);
    int64_t* d_lptr = pool.upload(I.lptr);
    int32_t *d_ta = pool.upload(I.ta), *d_tb = pool.upload(I.tb), *d_tk = pool.upload(I.tk);
    int32_t* d_cls[kNormalClasses];
    for (int c = 0; c < kNormalClasses; ++c) d_cls[c] = pool.upload(I.cls[c]);
    int64_t* d_chunk_off = pool.upload(I.chunk_off);
    int32_t *d_chunk_len = pool.upload(I.chunk_len), *d_fold_q = pool.upload(I.fold_q), *d_fold_ptr = pool.upload(I.fold_ptr);
    uint8_t* d_diag = pool.upload(I.diag);
    double* d_part = pool.alloc<double>(std::max<int64_t>(I.chunks(), 1));
    int32_t *d_fp = pool.upload(I.fp), *d_fi = pool.upload(I.fi);
    int64_t* d_rptr = pool.upload(I.rptr);
    int32_t *d_rpos = pool.upload(I.rpos), *d_rcol = pool.upload(I.rcol);
    int *d_perm = nullptr, *d_inv = nullptr;
    if (!I.perm.empty()) d_perm = pool.upload(I.perm), d_inv = pool.upload(I.inv);
    int* d_ctl = pool.alloc<int>(1);
    if (pool.error() != hipSuccess) return pool_failed(pool);
    D.index = std::move(pool);
    D.d_lptr = d_lptr, D.d_ta = d_ta, D.d_tb = d_tb, D.d_tk = d_tk;
    for (int c = 0; c < kNormalClasses; ++c) D.d_cls[c] = d_cls[c];
    D.d_chunk_off = d_chunk_off, D.d_chunk_len = d_chunk_len, D.d_fold_q = d_fold_q, D.d_fold_ptr = d_fold_ptr;
    D.d_diag = d_diag, D.d_part = d_part, D.d_fp = d_fp, D.d_fi = d_fi, D.d_rptr = d_rptr, D.d_rpos = d_rpos, D.d_rcol = d_rcol;
    D.d_perm = d_perm, D.d_inv = d_inv, D.d_ctl = d_ctl;
    D.on_device = true;
    return 0;
}

// Y = beta_y Yin + alpha F' X in blocks of kNormalBlock columns
void enqueue_ft(const parsy_normal* h, const double* fx, const double* x, int64_t ldx, int nrhs, double alpha, double beta_y,
                const double* yin, int64_t ldin, double* y, int64_t ldy, hipStream_t stream) {
    const NormalState& D = h->dev;
    const int m = h->I.m;
    if (m == 0) return;
    for (int q0 = 0; q0 < nrhs; q0 += kNormalBlock) {
        const int nb = std::min(kNormalBlock, nrhs - q0);
#define NORMAL_FT(NN)                                                                                                   \
    hipLaunchKernelGGL(k_normal_ft<NN>, dim3(blocks_of(m, kNThreads)), dim3(kNThreads), 0, stream, D.d_fp, D.d_fi, fx, m, \
                       x + q0 * ldx, ldx, alpha, beta_y, yin ? yin + q0 * ldin : nullptr, ldin, y + q0 * ldy, ldy)
        NORMAL_NB(nb, NORMAL_FT)
#undef NORMAL_FT
    }
}

// Y[rowmap] = beta_y Yin + alpha F (diag(w) X)
void enqueue_f(const parsy_normal* h, const double* fx, const double* w, const double* x, int64_t ldx, int nrhs, double alpha,
               double beta_y, const double* yin, int64_t ldin, const int* rowmap, double* y, int64_t ldy,
               hipStream_t stream) {
    const NormalState& D = h->dev;
    const int n = h->I.n;
    if (n == 0) return;
    for (int q0 = 0; q0 < nrhs; q0 += kNormalBlock) {
        const int nb = std::min(kNormalBlock, nrhs - q0);
#define NORMAL_F(NN)                                                                                                       \
    hipLaunchKernelGGL(k_normal_f<NN>, dim3(blocks_of(n, kNThreads)), dim3(kNThreads), 0, stream, D.d_rptr, D.d_rpos,      \
                       D.d_rcol, fx, w, n, x + q0 * ldx, ldx, alpha, beta_y, yin ? yin + q0 * ldin : nullptr, ldin, rowmap, \
                       y + q0 * ldy, ldy)
        NORMAL_NB(nb, NORMAL_F)
#undef NORMAL_F
    }
}

}  // namespace

int normal_check_values_args(const parsy_normal* h, const char* who, const void* fx, const void* values) {
    if (!h || !values || (!fx && h->I.nnzF() > 0)) return refuse(who, "null argument");
    if (h->plan->device < 0) return refuse(who, "plan was built without a device (device < 0)");
    return 0;
}

int normal_check_apply_args(const parsy_normal* h, const char* who, int op, const void* fx, const void* x, int ldx, int nrhs,
                            const void* y, int ldy) {
    if (!h || !x || !y || (!fx && h->I.nnzF() > 0)) return refuse(who, "null argument");
    if (h->plan->device < 0) return refuse(who, "plan was built without a device (device < 0)");
    if (op != PARSY_NORMAL_F && op != PARSY_NORMAL_FT) return refuse(who, "op must be PARSY_NORMAL_F or PARSY_NORMAL_FT (0, 1)");
    if (nrhs < 1) return refuse(who, "need nrhs >= 1");
    const int nx = op == PARSY_NORMAL_F ? h->I.m : h->I.n, ny = op == PARSY_NORMAL_F ? h->I.n : h->I.m;
    if (ldx < nx || ldy < ny)
        return refuse(who, op == PARSY_NORMAL_F ? "need leading dimensions ldx >= m and ldy >= n"
                                                : "need leading dimensions ldx >= n and ldy >= m");
    if (x == y) return refuse(who, "x and y are the same array (in place is not supported)");
    return 0;
}

int normal_check_lsq_args(const parsy_normal* h, const char* who, const void* fx, const void* lValues, const void* c, int ldc,
                          const void* x, int ldx, int nrhs, int steps, const void* r, int ldr, const void* g, int ldg) {
    if (!h || !lValues || !c || !x || (!fx && h->I.nnzF() > 0)) return refuse(who, "null argument");
    if (check_plan(h->plan, who, kNeedsIdle) != 0) return -1;
    if (steps < 0) return refuse(who, "need steps >= 0");
    if (nrhs < 1 || nrhs > 65535) return refuse(who, "need 1 <= nrhs <= 65535");
    if (ldc < h->I.m || ldx < h->I.n || (r && ldr < h->I.m) || (g && ldg < h->I.n))
        return refuse(who, "need leading dimensions ldc >= m, ldx >= n, ldr >= m and ldg >= n");
    if (x == c) return refuse(who, "x and c are the same array");
    return 0;
}

int normal_values(parsy_normal* h, const double* d_fx, const double* d_w, double beta, const double* d_base, double* d_values,
                  void* stream_) {
    const char* who = "parsy_normal_values_device";
    hipStream_t stream = (hipStream_t)stream_;
    if (normal_check_values_args(h, who, d_fx, d_values) != 0 || ensure_device(h) != 0) return -1;
    const NormalIndex& I = h->I;
    const NormalState& D = h->dev;
#define NORMAL_VALUES(C, LANES)                                                                                             \
    if (!I.cls[C].empty())                                                                                                  \
        hipLaunchKernelGGL(k_normal_values<LANES>, dim3(blocks_of((int64_t)I.cls[C].size() * LANES, kNThreads)),            \
                           dim3(kNThreads), 0, stream, D.d_cls[C], (int64_t)I.cls[C].size(), D.d_lptr, D.d_ta, D.d_tb, D.d_tk, \
                           d_fx, d_w, beta, D.d_diag, d_base, d_values)
    NORMAL_VALUES(0, 1);
    NORMAL_VALUES(1, 8);
    NORMAL_VALUES(2, 64);
#undef NORMAL_VALUES
    static_assert(kNormalLanes[0] == 1 && kNormalLanes[1] == 8 && kNormalLanes[2] == 64, "the launches above");
    if (I.chunks() > 0) {
        hipLaunchKernelGGL(k_normal_values_chunks, dim3(blocks_of(I.chunks(), kNWaves)), dim3(kNThreads), 0, stream,
                           D.d_chunk_off, D.d_chunk_len, I.chunks(), D.d_ta, D.d_tb, D.d_tk, d_fx, d_w, D.d_part);
        hipLaunchKernelGGL(k_normal_values_fold, dim3(blocks_of((int64_t)I.fold_q.size(), kNThreads)), dim3(kNThreads), 0,
                           stream, D.d_fold_q, D.d_fold_ptr, (int64_t)I.fold_q.size(), D.d_part, beta, D.d_diag, d_base,
                           d_values);
    }
    PARSY_HIP(hipGetLastError());
    return 0;
}

int normal_apply(parsy_normal* h, int op, const double* d_fx, const double* d_w, const double* d_x, int ldx, int nrhs,
                 double alpha, double beta, double* d_y, int ldy, void* stream_) {
    const char* who = "parsy_normal_apply_device";
    hipStream_t stream = (hipStream_t)stream_;
    if (normal_check_apply_args(h, who, op, d_fx, d_x, ldx, nrhs, d_y, ldy) != 0 || ensure_device(h) != 0) return -1;
    if (op == PARSY_NORMAL_F)
        enqueue_f(h, d_fx, d_w, d_x, ldx, nrhs, alpha, beta, d_y, ldy, nullptr, d_y, ldy, stream);
    else
        enqueue_ft(h, d_fx, d_x, ldx, nrhs, alpha, beta, d_y, ldy, d_y, ldy, stream);
    PARSY_HIP(hipGetLastError());
    return 0;
}

int normal_lsq(parsy_normal* h, const double* d_fx, const double* d_w, double beta, const double* d_L, const double* d_c,
               int ldc, double* d_x, int ldx, int nrhs, int steps, double* d_r, int ldr, double* d_g, int ldg, void* stream_) {
    const char* who = "parsy_lsq_solve_device";
    hipStream_t stream = (hipStream_t)stream_;
    if (normal_check_lsq_args(h, who, d_fx, d_L, d_c, ldc, d_x, ldx, nrhs, steps, d_r, ldr, d_g, ldg) != 0 ||
        ensure_device(h) != 0)
        return -1;
    parsy_plan* pl = h->plan;
    NormalState& D = h->dev;
    const int n = h->I.n, m = h->I.m;
    if (n == 0) return 0;
    PARSY_HIP(D.ws.grow((int64_t)(n + std::max(m, 1)) * nrhs));
    double* const z = D.ws.data();               // n x nrhs in the factor's ordering: the operand of the solves
    double* const rm = z + (int64_t)n * nrhs;    // m x nrhs: the residual of a step
    PARSY_HIP(hipMemsetAsync(D.d_ctl, 0, sizeof(int), stream));
    // z = S z: forward + backward solve, the status of each folded into d_ctl
    auto solve = [&]() -> int {
        for (int back = 0; back < 2; ++back) {
            if ((back ? plan_backsolve(pl, d_L, z, nrhs, n, stream) : plan_solve(pl, d_L, z, nrhs, n, stream)) != 0) return -1;
            hipLaunchKernelGGL(k_normal_note_status, dim3(1), dim3(64), 0, stream,
                               pl->solve_status_word ? pl->solve_status_word : pl->dp.sinfo, D.d_ctl);
        }
        PARSY_HIP(hipGetLastError());
        return 0;
    };
    // x = S F W c
    enqueue_f(h, d_fx, d_w, d_c, ldc, nrhs, 1.0, 0.0, nullptr, 0, D.d_inv, z, n, stream);
    if (solve() != 0) return -1;
    enqueue_perm_scatter(D.d_perm, z, 1.0, 0.0, d_x, ldx, n, nrhs, stream);
    for (int s = 0; s < steps; ++s) {
        // r = c - F' x, g = F W r - beta x (into z, in the factor's ordering), x += S g
        enqueue_ft(h, d_fx, d_x, ldx, nrhs, -1.0, 1.0, d_c, ldc, rm, std::max(m, 1), stream);
        enqueue_f(h, d_fx, d_w, rm, std::max(m, 1), nrhs, 1.0, -beta, d_x, ldx, D.d_inv, z, n, stream);
        if (solve() != 0) return -1;
        enqueue_perm_scatter(D.d_perm, z, 1.0, 1.0, d_x, ldx, n, nrhs, stream);
    }
    if (d_r || d_g) {
        double* r = d_r ? d_r : rm;
        const int64_t ld = d_r ? ldr : std::max(m, 1);
        enqueue_ft(h, d_fx, d_x, ldx, nrhs, -1.0, 1.0, d_c, ldc, r, ld, stream);
        if (d_g) enqueue_f(h, d_fx, d_w, r, ld, nrhs, 1.0, -beta, d_x, ldx, nullptr, d_g, ldg, stream);
    }
    hipLaunchKernelGGL(k_normal_put_status, dim3(1), dim3(64), 0, stream, D.d_ctl,
                       const_cast<int*>(pl->solve_status_word ? pl->solve_status_word : pl->dp.sinfo));
    PARSY_HIP(hipGetLastError());
    return 0;
}

}  // namespace parsy
