// A x = b in the caller's ordering (refine.hpp): the symmetric residual with its componentwise backward error and
// LAPACK dporfs's refinement loop run column by column on the device.
//
// The residual is the row sweep of sym_sweep.hpp over both triangles of P A P' held as CSR (built once per plan from the
// A2 pattern) with the epilogue ResidualOut: r = b - A z stored, the backward error max-reduced, one partial per
// workgroup and column, then a second pass (k_refine_state) that also applies dporfs's stopping test.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "errors.hpp"
#include "hip_check.hpp"
#include "executor.hpp"
#include "plan_util.hpp"
#include "kernels.hpp"
#include "refine.hpp"
#include "sym_sweep.hpp"
#include "cond.hpp"

namespace parsy {

namespace {

constexpr int kRThreads = kRefineThreads;

// r = b - A z of a row, and its term of the componentwise backward error
struct ResidualOut : SweepScale {
    __device__ __forceinline__ u64 operator()(double* r, bool first, double b, double acc, double den,
                                              const double*) const {
        // dporfs: den > safe2 ? |r| / den : (|r| + safe1) / (den + safe1); den = |b| + sum |a||z|
        const double rr = b - acc;
        if (first) *r = rr;
        const double d = fabs(b) + den;
        const double ratio = d > safe2 ? fabs(rr) / d : (fabs(rr) + safe1) / (d + safe1);
        return (u64)__double_as_longlong(ratio);
    }
};

// vf[e] = values[src[e]]: the caller's A2-order values on the full pattern (once per call)
__global__ __launch_bounds__(kRThreads) void k_refine_gather_values(const double* __restrict__ values,
                                                                    const int* __restrict__ src, double* __restrict__ vf,
                                                                    int64_t nnz) {
    for (int64_t e = (int64_t)blockIdx.x * kRThreads + threadIdx.x; e < nnz; e += (int64_t)gridDim.x * kRThreads)
        vf[e] = values[src[e]];
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
    if (!pl->refine) pl->refine = std::make_unique<RefineState>(&pl->meter);
    return *pl->refine;
}

}  // namespace

ColState col_state(RefineState& R, int cap) {
    ColState c;
    char* p = R.colstate.data();
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
    if (R.pattern_ready) return 0;
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
    PARSY_HIP(hipSetDevice(pl->device));
    DevicePool pool(&R.meter);
    int64_t* d_rp = pool.upload(rp);
    int *d_ci = pool.upload(ci), *d_src = pool.upload(src);
    double* d_vf = pool.alloc<double>((int64_t)ci.size());
    if (pool.error() != hipSuccess) return pool_failed(pool);
    R.pattern = std::move(pool);
    R.d_rp = d_rp, R.d_ci = d_ci, R.d_src = d_src, R.d_vf = d_vf;
    R.nnz_full = nf;
    R.max_row = max_row;
    const double mean = n > 0 ? (double)nf / n : 0;
    R.group = mean > 24 ? 32 : mean > 12 ? 16 : mean > 6 ? 8 : 4;
    R.pattern_ready = true;
    return 0;
}

// pb, z, r (n x nrhs) and the per-column state, grown on demand; *perm: the plan's ordering on the device
int refine_ensure_workspace(parsy_plan* pl, int nrhs, const int** perm) {
    RefineState& R = state(pl);
    const int64_t need = 3 * (int64_t)pl->S.n * nrhs;
    PARSY_HIP(hipSetDevice(pl->device));
    PARSY_HIP(R.ws.grow(need));
    if (R.colstate_cap < nrhs) {
        R.colstate_cap = 0;
        PARSY_HIP(R.colstate.grow((int64_t)nrhs * (kRefinePartials * 8 + 8 + 8 + 4 + 4) + 8));
        R.colstate_cap = nrhs;
    }
    return plan_perm_device(pl, perm);
}

int refine_residual_enqueue(parsy_plan* pl, const double* z, const double* pb, double* r, int nrhs, u64* part,
                            hipStream_t stream) {
    return sym_sweep_enqueue<ResidualOut>(pl, pl->refine->d_vf, z, pb, r, nrhs, part, stream);
}

int refine_gather_values(parsy_plan* pl, const double* d_values, double* vf, hipStream_t stream) {
    RefineState& R = *pl->refine;
    const int64_t nb = std::max<int64_t>(1, std::min<int64_t>(8192, (R.nnz_full + kRThreads - 1) / kRThreads));
    hipLaunchKernelGGL(k_refine_gather_values, dim3((unsigned)nb), dim3(kRThreads), 0, stream, d_values, R.d_src, vf,
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

int refine_report_berr(parsy_plan* pl, int nb, int nrhs, hipStream_t stream) {
    RefineState& R = *pl->refine;
    const ColState c = col_state(R, R.colstate_cap);
    hipLaunchKernelGGL(k_refine_state, dim3(nrhs), dim3(kRThreads), 0, stream, c.part, nb, c.berr, c.lstres, c.active,
                       c.steps, 0, 1, c.ctl);
    PARSY_HIP(hipGetLastError());
    return 0;
}

int plan_residual(parsy_plan* pl, const double* d_values, const double* d_x, int ldx, const double* d_b, int ldb,
                  double* d_r, int ldr, int nrhs, double* berr, hipStream_t stream) {
    const char* who = "parsy_residual_device";
    if (check_plan(pl, who, kNeedsIdle) != 0) return -1;
    const int n = pl->S.n;
    if (nrhs < 1 || nrhs > 65535 || ldx < n || ldb < n || (d_r && ldr < n))
        return set_last_error(std::string(who) + ": need 1 <= nrhs <= 65535 and leading dimensions >= n"), -1;
    const int* perm = nullptr;
    if (refine_ensure_pattern(pl) != 0 || refine_ensure_workspace(pl, nrhs, &perm) != 0) return -1;
    RefineState& R = *pl->refine;
    const int64_t nn = (int64_t)n * nrhs;
    double *pb = R.ws.data(), *z = pb + nn, *r = pb + 2 * nn;
    const ColState c = col_state(R, R.colstate_cap);
    if (refine_gather_values(pl, d_values, R.d_vf, stream) != 0) return -1;
    enqueue_perm_gather(perm, d_x, ldx, z, nullptr, n, nrhs, stream);
    enqueue_perm_gather(perm, d_b, ldb, pb, nullptr, n, nrhs, stream);
    const int nb = refine_residual_enqueue(pl, z, pb, r, nrhs, c.part, stream);
    if (nb < 0) return -1;
    if (d_r) enqueue_perm_scatter(perm, r, 1.0, 0.0, d_r, ldr, n, nrhs, stream);
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
    const int* perm = nullptr;
    if ((residuals && refine_ensure_pattern(pl) != 0) || refine_ensure_workspace(pl, nrhs, &perm) != 0) return -1;
    RefineState& R = *pl->refine;
    const int64_t nn = (int64_t)n * nrhs;
    double *pb = R.ws.data(), *z = pb + nn, *r = pb + 2 * nn;
    const ColState c = col_state(R, R.colstate_cap);
    PARSY_HIP(hipMemsetAsync(c.ctl, 0, 2 * sizeof(int), stream));
    enqueue_perm_gather(perm, d_b, ldb, pb, z, n, nrhs, stream);
    if (refine_solve_enqueue(pl, d_L, z, nrhs, c.ctl, stream) != 0) return -1;
    if (residuals) {
        if (refine_gather_values(pl, d_values, R.d_vf, stream) != 0) return -1;
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
    enqueue_perm_scatter(perm, z, 1.0, 0.0, d_x, ldx, n, nrhs, stream);
    PARSY_HIP(hipGetLastError());
    if (steps) PARSY_HIP(hipMemcpyAsync(steps, c.steps, (size_t)nrhs * 4, hipMemcpyDeviceToHost, stream));
    if (berr) PARSY_HIP(hipMemcpyAsync(berr, c.berr, (size_t)nrhs * 8, hipMemcpyDeviceToHost, stream));
    if (steps || berr) PARSY_HIP(hipStreamSynchronize(stream));
    return 0;
}

}  // namespace parsy
