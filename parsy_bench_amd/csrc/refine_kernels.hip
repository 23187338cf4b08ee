// A x = b in the caller's ordering (refine.hpp): the symmetric residual with its componentwise backward error, the
// permutations in and out, and LAPACK dporfs's refinement loop run column by column on the device.
//
// The residual works on both triangles of P A P' held as CSR (built once per plan from the A2 pattern).  Every row's sums
// are taken in a fixed order (a fixed lane split and a fixed butterfly), with no float atomics, so that a result is
// bitwise the same from run to run.  The backward error is max-reduced as the bit patterns of non-negative doubles
// (an unsigned max: a NaN outranks every number and so survives the reduction): one partial per workgroup and column,
// then a second pass (k_refine_state) that also applies dporfs's stopping test.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <string>
#include <vector>

#include "errors.hpp"
#include "hip_check.hpp"
#include "executor.hpp"
#include "plan_util.hpp"
#include "kernels.hpp"
#include "refine.hpp"
#include "cond.hpp"

namespace parsy {

namespace {

constexpr int kRThreads = kRefineThreads;

__device__ __forceinline__ u64 berr_bits(double b, double rr, double den, double safe1, double safe2) {
    // dporfs: den > safe2 ? |r| / den : (|r| + safe1) / (den + safe1); den = |b| + sum |a||z|
    const double d = fabs(b) + den;
    const double ratio = d > safe2 ? fabs(rr) / d : (fabs(rr) + safe1) / (d + safe1);
    return (u64)__double_as_longlong(ratio);
}

// 1-4 right-hand sides (z, pb, r column-major, leading dimension n): G lanes per row split its entries (lane g takes
// g, g + G, ...), a butterfly sums them.  Grid-stride over the rows; partial maxima part[c * gridDim.x + blockIdx.x].
template <int G, int NR>
__global__ __launch_bounds__(kRThreads) void k_sym_residual(const int64_t* __restrict__ rp, const int* __restrict__ ci,
                                                            const double* __restrict__ vf, const double* __restrict__ z,
                                                            const double* __restrict__ pb, double* __restrict__ r, int n,
                                                            double safe1, double safe2, u64* __restrict__ part) {
    __shared__ u64 sm[4];
    const int tid = threadIdx.x, g = tid % G;
    constexpr int kRows = kRThreads / G;
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
            const double b = pb[row + (int64_t)c * n], rr = b - acc[c];
            if (g == 0) r[row + (int64_t)c * n] = rr;
            mx[c] = max(mx[c], berr_bits(b, rr, den[c], safe1, safe2));
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
// gathers z[j, q0 .. q0 + L) of an entry are one coalesced run.  pb and r stay column-major.
template <int L>
__global__ __launch_bounds__(kRThreads) void k_sym_residual_mrhs(const int64_t* __restrict__ rp, const int* __restrict__ ci,
                                                                 const double* __restrict__ vf, const double* __restrict__ zt,
                                                                 int ldq, const double* __restrict__ pb,
                                                                 double* __restrict__ r, int n, int nrhs, double safe1,
                                                                 double safe2, u64* __restrict__ part) {
    __shared__ u64 sm[4][64];
    const int tid = threadIdx.x, lq = tid % L;
    const int q = (int)blockIdx.y * L + lq;
    const bool on = q < nrhs;
    constexpr int kRows = kRThreads / L;
    u64 mx = 0;
    for (int64_t row = (int64_t)blockIdx.x * kRows + tid / L; row < n; row += (int64_t)gridDim.x * kRows) {
        double acc = 0.0, den = 0.0;
        const int64_t e1 = rp[row + 1];
        if (on)
            for (int64_t e = rp[row]; e < e1; ++e) {
                const double a = vf[e];
                const double zj = zt[(int64_t)ci[e] * ldq + q];
                acc = fma(a, zj, acc);
                den = fma(fabs(a), fabs(zj), den);
            }
        if (on) {
            const double b = pb[row + (int64_t)q * n], rr = b - acc;
            r[row + (int64_t)q * n] = rr;
            mx = max(mx, berr_bits(b, rr, den, safe1, safe2));
        }
    }
    for (int o = L; o < 64; o <<= 1) mx = max(mx, shfl_xor_u64(mx, o));   // the lanes of one column within the wave
    if ((tid & 63) < L) sm[tid >> 6][tid & 63] = mx;
    __syncthreads();
    if (tid < L && on)
        part[(int64_t)q * gridDim.x + blockIdx.x] = max(max(sm[0][tid], sm[1][tid]), max(sm[2][tid], sm[3][tid]));
}

// vf[e] = values[src[e]]: the caller's A2-order values on the full pattern (once per call)
__global__ __launch_bounds__(kRThreads) void k_refine_gather_values(const double* __restrict__ values,
                                                                    const int* __restrict__ src, double* __restrict__ vf,
                                                                    int64_t nnz) {
    for (int64_t e = (int64_t)blockIdx.x * kRThreads + threadIdx.x; e < nnz; e += (int64_t)gridDim.x * kRThreads)
        vf[e] = values[src[e]];
}

// dst[k, q] = src[perm[k], q] (dst leading dimension n; a second copy into dst2 when given); perm null: identity
__global__ __launch_bounds__(kRThreads) void k_refine_permute_in(const double* __restrict__ src, int64_t ld,
                                                                 const int* __restrict__ perm, double* __restrict__ dst,
                                                                 double* __restrict__ dst2, int n) {
    const int64_t k = (int64_t)blockIdx.x * kRThreads + threadIdx.x;
    if (k >= n) return;
    const int64_t q = blockIdx.y;
    const double v = src[(perm ? perm[k] : k) + q * ld];
    dst[k + q * n] = v;
    if (dst2) dst2[k + q * n] = v;
}

// dst[perm[k], q] = src[k, q]
__global__ __launch_bounds__(kRThreads) void k_refine_permute_out(const double* __restrict__ src,
                                                                  const int* __restrict__ perm, double* __restrict__ dst,
                                                                  int64_t ld, int n) {
    const int64_t k = (int64_t)blockIdx.x * kRThreads + threadIdx.x;
    if (k >= n) return;
    const int64_t q = blockIdx.y;
    dst[(perm ? perm[k] : k) + q * ld] = src[k + q * n];
}

// z[:, q] += d[:, q] for the columns still active
__global__ __launch_bounds__(kRThreads) void k_refine_update(double* __restrict__ z, const double* __restrict__ d,
                                                             const int* __restrict__ active, int n) {
    const int64_t k = (int64_t)blockIdx.x * kRThreads + threadIdx.x;
    const int64_t q = blockIdx.y;
    if (k >= n || !active[q]) return;
    z[k + q * n] += d[k + q * n];
}

__global__ void k_refine_init(double* __restrict__ lstres, int* __restrict__ active, int* __restrict__ steps, int nrhs) {
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= nrhs) return;
    lstres[q] = 3.0;
    active[q] = 1;
    steps[q] = 0;
}

// ctl[1] = -1 when the solve that left its status word at `word` timed out in a hand-off wait (parsy_solve_status)
__global__ void k_refine_note_status(const int* __restrict__ word, int* __restrict__ ctl) {
    if (threadIdx.x == 0 && *word < 0) ctl[1] = -1;
}

// Second pass of the max-reduction, one workgroup per column.  report: berr[q] only.  Otherwise dporfs's test for an
// active column: go on (lstres = berr, one more step, counted in ctl[0]) or freeze the column (active = 0).
__global__ __launch_bounds__(kRThreads) void k_refine_state(const u64* __restrict__ part, int nb, double* __restrict__ berr,
                                                            double* __restrict__ lstres, int* __restrict__ active,
                                                            int* __restrict__ steps, int max_steps, int report,
                                                            int* __restrict__ ctl) {
    __shared__ u64 sm[4];
    const int q = blockIdx.x;
    u64 v = 0;
    for (int b = threadIdx.x; b < nb; b += kRThreads) v = max(v, part[(int64_t)q * nb + b]);
    v = block_max(v, sm);
    if (threadIdx.x != 0) return;
    const double be = __longlong_as_double((long long)v);
    if (report) {
        berr[q] = be;
        return;
    }
    if (!active[q]) return;
    berr[q] = be;
    const double eps = 0x1p-53;
    if (be > eps && 2.0 * be <= lstres[q] && steps[q] < max_steps) {
        lstres[q] = be;
        steps[q] += 1;
        atomicAdd(&ctl[0], 1);
    } else {
        active[q] = 0;
    }
}

dim3 grid_nq(int n, int nrhs) { return dim3((unsigned)((n + kRThreads - 1) / kRThreads), (unsigned)nrhs); }

RefineState& state(parsy_plan* pl) {
    if (!pl->refine) pl->refine = new RefineState;
    return *pl->refine;
}

}  // namespace

ColState col_state(RefineState& R, int cap) {
    ColState c;
    char* p = R.colstate;
    c.part = (u64*)p;
    p += (size_t)kRefinePartials * cap * sizeof(u64);
    c.berr = (double*)p;
    p += (size_t)cap * sizeof(double);
    c.lstres = (double*)p;
    p += (size_t)cap * sizeof(double);
    c.active = (int*)p;
    p += (size_t)cap * sizeof(int);
    c.steps = (int*)p;
    p += (size_t)cap * sizeof(int);
    c.ctl = (int*)p;
    return c;
}

// Both triangles of P A P' as CSR, on first use.  (row, col) of an A2 entry q is recovered from where the factorization
// scatters it: a_dst[q] = px + (col - c0) * r + (position of row in the supernode's row list).
int refine_ensure_pattern(parsy_plan* pl) {
    RefineState& R = state(pl);
    if (R.d_rp) return 0;
    const Schedule& S = pl->S;
    const int n = S.n;
    std::vector<int> arow((size_t)S.nnzA), acol((size_t)S.nnzA);
    std::vector<int64_t> rp((size_t)n + 1, 0);
    for (int t = 0; t < S.nsuper; ++t) {
        const SnDesc& d = S.sn[t];
        for (int q = d.a0; q < d.a1; ++q) {
            const int64_t v = S.a_dst[q] - d.px;
            if (v < 0 || v >= (int64_t)d.w * d.r) return set_last_error("refine: A entry outside its supernode's panel"), -1;
            const int col = d.c0 + (int)(v / d.r), row = S.rows[d.pi + v % d.r];
            if (row < col || row >= n) return set_last_error("refine: A2 entry above the diagonal"), -1;
            arow[q] = row;
            acol[q] = col;
            rp[row + 1] += 1;
            if (row != col) rp[col + 1] += 1;
        }
    }
    for (int i = 0; i < n; ++i) rp[i + 1] += rp[i];
    const int64_t nf = rp[n];
    std::vector<int> ci((size_t)std::max<int64_t>(nf, 1)), src((size_t)std::max<int64_t>(nf, 1));
    std::vector<int64_t> fill(rp.begin(), rp.end() - 1);
    int max_row = 0;
    for (int i = 0; i < n; ++i) max_row = std::max<int64_t>(max_row, rp[i + 1] - rp[i]);
    for (int64_t q = 0; q < S.nnzA; ++q) {   // ascending A2 order: every row's entries come in one fixed order
        const int row = arow[q], col = acol[q];
        ci[fill[row]] = col;
        src[fill[row]++] = (int)q;
        if (row != col) {
            ci[fill[col]] = row;
            src[fill[col]++] = (int)q;
        }
    }
    R.nnz_full = nf;
    R.max_row = max_row;
    const double mean = n > 0 ? (double)nf / n : 0;
    R.group = mean > 24 ? 32 : mean > 12 ? 16 : mean > 6 ? 8 : 4;
    PARSY_HIP(hipSetDevice(pl->device));
    int64_t bytes = 0;
    if (upload_counted(R.d_rp, rp, bytes) != 0 || upload_counted(R.d_ci, ci, bytes) != 0 ||
        upload_counted(R.d_src, src, bytes) != 0)
        return -1;
    PARSY_HIP(hipMalloc((void**)&R.d_vf, ci.size() * 8));
    R.pattern_bytes = bytes + (int64_t)ci.size() * 8;
    pl->device_bytes += R.pattern_bytes;
    return 0;
}

// pb, z, r (n x nrhs) and the per-column state, grown on demand; the perm's device copy
int refine_ensure_workspace(parsy_plan* pl, int nrhs) {
    RefineState& R = state(pl);
    const int64_t need = 3 * (int64_t)pl->S.n * nrhs;
    PARSY_HIP(hipSetDevice(pl->device));
    if (grow_counted(pl, R.ws, R.ws_len, need) != 0) return -1;
    if (R.colstate_cap < nrhs) {
        R.colstate_cap = 0;
        if (grow_counted(pl, R.colstate, R.colstate_len, (int64_t)nrhs * (kRefinePartials * 8 + 8 + 8 + 4 + 4) + 8) != 0)
            return -1;
        R.colstate_cap = nrhs;
    }
    const int* perm = nullptr;
    return plan_perm_device(pl, &perm);
}

// r = pb - A z and the partial maxima of every column's backward error; returns the number of partials (< 0: error)
int refine_residual_enqueue(parsy_plan* pl, const double* z, const double* pb, double* r, int nrhs, u64* part,
                     hipStream_t stream) {
    RefineState& R = *pl->refine;
    const int n = pl->S.n;
    const double safe1 = (double)(R.max_row + 1) * DBL_MIN, safe2 = safe1 / 0x1p-53;
    auto nblocks = [&](int rows_per_block) {
        return (int)std::max<int64_t>(1, std::min<int64_t>(kRefinePartials, ((int64_t)n + rows_per_block - 1) / rows_per_block));
    };
    if (nrhs <= 4) {
        const int G = R.group, nb = nblocks(kRThreads / G);
#define R_GROUP(GG, NN)                                                                                              \
    if (G == GG && nrhs == NN)                                                                                       \
        hipLaunchKernelGGL((k_sym_residual<GG, NN>), dim3(nb), dim3(kRThreads), 0, stream, R.d_rp, R.d_ci, R.d_vf, z, \
                           pb, r, n, safe1, safe2, part);
#define R_GROUPS(GG) R_GROUP(GG, 1) R_GROUP(GG, 2) R_GROUP(GG, 3) R_GROUP(GG, 4)
        R_GROUPS(4) R_GROUPS(8) R_GROUPS(16) R_GROUPS(32)
#undef R_GROUPS
#undef R_GROUP
        PARSY_HIP(hipGetLastError());
        return nb;
    }
    // stage z with the right-hand sides of a row contiguous in the plan's xt (the forward solves' staging buffer: a
    // solve fills it afresh, the residual runs between solves)
    const int ldq = (nrhs + 15) & ~15;
    const int64_t need = (int64_t)n * ldq;
    PARSY_HIP(grow_device(pl->xt, pl->xt_len, need));
    launch_transpose_x(const_cast<double*>(z), n, pl->xt, ldq, n, nrhs, true, stream);
    const int L = nrhs <= 8 ? 8 : nrhs <= 16 ? 16 : nrhs <= 32 ? 32 : 64;
    const int nb = nblocks(kRThreads / L);
    const dim3 grid(nb, (nrhs + L - 1) / L);
#define R_MRHS(LL)                                                                                                  \
    if (L == LL)                                                                                                    \
        hipLaunchKernelGGL(k_sym_residual_mrhs<LL>, grid, dim3(kRThreads), 0, stream, R.d_rp, R.d_ci, R.d_vf, pl->xt, \
                           ldq, pb, r, n, nrhs, safe1, safe2, part);
    R_MRHS(8) R_MRHS(16) R_MRHS(32) R_MRHS(64)
#undef R_MRHS
    PARSY_HIP(hipGetLastError());
    return nb;
}

int refine_gather_values(parsy_plan* pl, const double* d_values, hipStream_t stream) {
    RefineState& R = *pl->refine;
    const int64_t nb = std::max<int64_t>(1, std::min<int64_t>(8192, (R.nnz_full + kRThreads - 1) / kRThreads));
    hipLaunchKernelGGL(k_refine_gather_values, dim3((unsigned)nb), dim3(kRThreads), 0, stream, d_values, R.d_src, R.d_vf,
                       R.nnz_full);
    PARSY_HIP(hipGetLastError());
    return 0;
}

// forward + backward solve of the permuted system in place on x (leading dimension n); every solve's status word is
// folded into ctl[1] on the device
int refine_solve_enqueue(parsy_plan* pl, const double* d_L, double* x, int nrhs, int* ctl, hipStream_t stream) {
    const int n = pl->S.n;
    if (plan_solve(pl, d_L, x, nrhs, n, stream) != 0) return -1;
    hipLaunchKernelGGL(k_refine_note_status, dim3(1), dim3(64), 0, stream,
                       pl->solve_status_word ? pl->solve_status_word : pl->dp.sinfo, ctl);
    if (plan_backsolve(pl, d_L, x, nrhs, n, stream) != 0) return -1;
    hipLaunchKernelGGL(k_refine_note_status, dim3(1), dim3(64), 0, stream,
                       pl->solve_status_word ? pl->solve_status_word : pl->dp.sinfo, ctl);
    PARSY_HIP(hipGetLastError());
    return 0;
}

int refine_permute_in(parsy_plan* pl, const double* src, int64_t ld, double* dst, double* dst2, int nrhs,
                      hipStream_t stream) {
    const int n = pl->S.n;
    if (n > 0)
        hipLaunchKernelGGL(k_refine_permute_in, grid_nq(n, nrhs), dim3(kRThreads), 0, stream, src, ld, pl->refine->d_perm,
                           dst, dst2, n);
    PARSY_HIP(hipGetLastError());
    return 0;
}

int refine_report_berr(parsy_plan* pl, int nb, int nrhs, hipStream_t stream) {
    RefineState& R = *pl->refine;
    const ColState c = col_state(R, R.colstate_cap);
    hipLaunchKernelGGL(k_refine_state, dim3(nrhs), dim3(kRThreads), 0, stream, c.part, nb, c.berr, c.lstres, c.active,
                       c.steps, 0, 1, c.ctl);
    PARSY_HIP(hipGetLastError());
    return 0;
}

void refine_free(parsy_plan* pl) {
    RefineState* R = pl->refine;
    if (!R) return;
    if (pl->device >= 0) {
        for (void* p : {(void*)R->d_perm, (void*)R->d_rp, (void*)R->d_ci, (void*)R->d_src, (void*)R->d_vf, (void*)R->ws,
                        (void*)R->colstate})
            if (p) (void)hipFree(p);
    }
    delete R;
    pl->refine = nullptr;
}

int plan_set_perm(parsy_plan* pl, const int* perm) {
    const int n = pl->S.n;
    std::vector<int> p;
    if (perm) {
        p.assign(perm, perm + n);
        std::vector<char> seen((size_t)n, 0);
        for (int v : p) {
            if (v < 0 || v >= n || seen[v])
                return set_last_error("parsy_plan_set_perm: perm is not a permutation of 0..n-1"), -1;
            seen[v] = 1;
        }
    }
    RefineState& R = state(pl);
    if (R.d_perm) {
        (void)hipSetDevice(pl->device);
        (void)hipDeviceSynchronize();   // (a call may still read the old one)
        (void)hipFree(R.d_perm);
        pl->device_bytes -= (int64_t)R.perm.size() * 4;
        R.d_perm = nullptr;
    }
    R.perm.swap(p);
    return 0;
}

int plan_perm_device(parsy_plan* pl, const int** out) {
    *out = nullptr;
    RefineState* R = pl->refine;
    if (!R || R->perm.empty()) return 0;
    if (!R->d_perm) {
        PARSY_HIP(hipMalloc((void**)&R->d_perm, R->perm.size() * 4));
        PARSY_HIP(hipMemcpy(R->d_perm, R->perm.data(), R->perm.size() * 4, hipMemcpyHostToDevice));
        pl->device_bytes += (int64_t)R->perm.size() * 4;
    }
    *out = R->d_perm;
    return 0;
}

int plan_residual(parsy_plan* pl, const double* d_values, const double* d_x, int ldx, const double* d_b, int ldb,
                  double* d_r, int ldr, int nrhs, double* berr, hipStream_t stream) {
    const char* who = "parsy_residual_device";
    if (check_plan(pl, who, kNeedsIdle) != 0) return -1;
    const int n = pl->S.n;
    if (nrhs < 1 || nrhs > 65535 || ldx < n || ldb < n || (d_r && ldr < n))
        return set_last_error(std::string(who) + ": need 1 <= nrhs <= 65535 and leading dimensions >= n"), -1;
    if (refine_ensure_pattern(pl) != 0 || refine_ensure_workspace(pl, nrhs) != 0) return -1;
    RefineState& R = *pl->refine;
    const int64_t nn = (int64_t)n * nrhs;
    double *pb = R.ws, *z = R.ws + nn, *r = R.ws + 2 * nn;
    const ColState c = col_state(R, R.colstate_cap);
    if (refine_gather_values(pl, d_values, stream) != 0) return -1;
    if (n > 0) {
        hipLaunchKernelGGL(k_refine_permute_in, grid_nq(n, nrhs), dim3(kRThreads), 0, stream, d_x, (int64_t)ldx, R.d_perm,
                           z, (double*)nullptr, n);
        hipLaunchKernelGGL(k_refine_permute_in, grid_nq(n, nrhs), dim3(kRThreads), 0, stream, d_b, (int64_t)ldb, R.d_perm,
                           pb, (double*)nullptr, n);
    }
    const int nb = refine_residual_enqueue(pl, z, pb, r, nrhs, c.part, stream);
    if (nb < 0) return -1;
    if (d_r && n > 0)
        hipLaunchKernelGGL(k_refine_permute_out, grid_nq(n, nrhs), dim3(kRThreads), 0, stream, r, R.d_perm, d_r,
                           (int64_t)ldr, n);
    if (berr) {
        hipLaunchKernelGGL(k_refine_state, dim3(nrhs), dim3(kRThreads), 0, stream, c.part, nb, c.berr, c.lstres, c.active,
                           c.steps, 0, 1, c.ctl);
        PARSY_HIP(hipGetLastError());
        PARSY_HIP(hipMemcpyAsync(berr, c.berr, (size_t)nrhs * 8, hipMemcpyDeviceToHost, stream));
        PARSY_HIP(hipStreamSynchronize(stream));
    }
    PARSY_HIP(hipGetLastError());
    return 0;
}

int plan_solve_refined(parsy_plan* pl, const double* d_values, const double* d_L, const double* d_b, int ldb, double* d_x,
                       int ldx, int nrhs, int max_steps, int32_t* steps, double* berr, double* ferr, hipStream_t stream) {
    const char* who = ferr ? "parsy_solve_spd_bounds_device" : "parsy_solve_spd_device";
    if (check_plan(pl, who, kNeedsIdle) != 0) return -1;
    const int n = pl->S.n;
    if (nrhs < 1 || nrhs > 65535 || ldx < n || ldb < n || max_steps < 0)
        return set_last_error(std::string(who) + ": need 1 <= nrhs <= 65535, max_steps >= 0 and leading dimensions >= n"), -1;
    if (d_x == d_b && ldx != ldb) return set_last_error(std::string(who) + ": d_x == d_b needs ldx == ldb"), -1;
    const bool residuals = max_steps > 0 || steps || berr || ferr;
    if ((residuals && refine_ensure_pattern(pl) != 0) || refine_ensure_workspace(pl, nrhs) != 0) return -1;
    RefineState& R = *pl->refine;
    const int64_t nn = (int64_t)n * nrhs;
    double *pb = R.ws, *z = R.ws + nn, *r = R.ws + 2 * nn;
    const ColState c = col_state(R, R.colstate_cap);
    PARSY_HIP(hipMemsetAsync(c.ctl, 0, 2 * sizeof(int), stream));
    if (n > 0)
        hipLaunchKernelGGL(k_refine_permute_in, grid_nq(n, nrhs), dim3(kRThreads), 0, stream, d_b, (int64_t)ldb, R.d_perm,
                           pb, z, n);
    if (refine_solve_enqueue(pl, d_L, z, nrhs, c.ctl, stream) != 0) return -1;
    if (residuals) {
        if (refine_gather_values(pl, d_values, stream) != 0) return -1;
        hipLaunchKernelGGL(k_refine_init, dim3((nrhs + 255) / 256), dim3(256), 0, stream, c.lstres, c.active, c.steps, nrhs);
        for (;;) {
            PARSY_HIP(hipMemsetAsync(c.ctl, 0, sizeof(int), stream));
            const int nb = refine_residual_enqueue(pl, z, pb, r, nrhs, c.part, stream);
            if (nb < 0) return -1;
            hipLaunchKernelGGL(k_refine_state, dim3(nrhs), dim3(kRThreads), 0, stream, c.part, nb, c.berr, c.lstres,
                               c.active, c.steps, max_steps, 0, c.ctl);
            PARSY_HIP(hipGetLastError());
            int ctl[2] = {0, 0};
            PARSY_HIP(hipMemcpyAsync(ctl, c.ctl, sizeof(ctl), hipMemcpyDeviceToHost, stream));
            PARSY_HIP(hipStreamSynchronize(stream));
            if (ctl[1] < 0)
                return set_last_error(std::string(who) +
                                      ": a hand-off wait inside a chain launch timed out; x is not the solution"),
                       -1;
            if (ctl[0] == 0) break;
            // the columns that go on: z += (L L')^-1 r (every column rides along in the solves; frozen ones are not updated)
            if (refine_solve_enqueue(pl, d_L, r, nrhs, c.ctl, stream) != 0) return -1;
            hipLaunchKernelGGL(k_refine_update, grid_nq(n, nrhs), dim3(kRThreads), 0, stream, z, r, c.active, n);
        }
    }
    // (before X is written: a solve of the bounds that timed out leaves every output untouched)
    if (ferr && cond_bounds_phase(pl, who, d_L, nrhs, ferr, stream) != 0) return -1;
    if (n > 0)
        hipLaunchKernelGGL(k_refine_permute_out, grid_nq(n, nrhs), dim3(kRThreads), 0, stream, z, R.d_perm, d_x,
                           (int64_t)ldx, n);
    PARSY_HIP(hipGetLastError());
    if (steps) PARSY_HIP(hipMemcpyAsync(steps, c.steps, (size_t)nrhs * 4, hipMemcpyDeviceToHost, stream));
    if (berr) PARSY_HIP(hipMemcpyAsync(berr, c.berr, (size_t)nrhs * 8, hipMemcpyDeviceToHost, stream));
    if (steps || berr) PARSY_HIP(hipStreamSynchronize(stream));
    return 0;
}

}  // namespace parsy
