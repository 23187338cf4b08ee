// Forward error bounds and the condition estimate of the SPD solve (cond.hpp): dporfs's weights
// w = |r| + nz eps (|A||z| + |b|), ||A||_1, and Higham's 1-norm estimator (LAPACK dlacn2) of W A^-1 (FERR) or A^-1 (RCOND)
// with (L L')^-1 as the operator.
//
// The estimator is reverse communication: between two applications of the operator it looks at the vector that came back
// and writes the next one.  Here that is ONE kernel (k_cond_step, a workgroup per column) run between two solves of all
// the columns at once; the state of a column (CondCol) lives on the device, and the host reads one word per application:
// the number of columns that still go on.  A column takes at most 11 applications (1 + 1 + 4 x 2 + 1), so a call
// enqueues at most 11 solve pairs whatever the number of right-hand sides; a column that has finished keeps a zero
// operand and a frozen state.  The weights are the row sweep of sym_sweep.hpp with the epilogue WeightOut, the
// residual's own sums; every other sum here also runs in a fixed order, nothing is accumulated with float atomics, and
// maxima are reduced as the bit patterns of non-negative doubles (a NaN survives): given the same solve results the
// estimate is bitwise the same.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <string>

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

constexpr int kCThreads = kRefineThreads;
constexpr int kCondMaxApplications = 11;

// dporfs's weight of a row, and |z| of the row for the column's max (z is read here, behind the sums)
struct WeightOut : SweepScale {
    __device__ __forceinline__ u64 operator()(double* w, bool first, double b, double acc, double den,
                                              const double* zp) const {
        // |r| + nz eps (|b| + sum |a||z|), + safe1 unless the sum is > safe2
        const double s = fabs(b) + den;
        const double v = fabs(b - acc) + nzeps * s;
        if (first) *w = s > safe2 ? v : v + safe1;
        return abs_bits(*zp);
    }
};

enum Produce { kZero, kUniform, kSigns, kUnit, kAlternating };

// Everything dlacn2 (and dporfs's multiplications by W) does between two applications of (L L')^-1 to column
// q = blockIdx.x of v (leading dimension n).  w null: the operator is A^-1 itself (RCOND).  Consume: the vector that
// came back, times w when the application was W A^-1 -- its 1-norm, its signs against the saved ones, the first index
// of its largest magnitude.  Decide: the column's next state.  Produce: the next operand, times w when the next
// application is A^-1 W.  ctl[0] counts the columns that go on.
__global__ __launch_bounds__(kCThreads) void k_cond_step(double* __restrict__ v, const double* __restrict__ w,
                                                         unsigned char* __restrict__ sgn, CondCol* __restrict__ cols,
                                                         int n, int* __restrict__ ctl) {
    __shared__ double s_sum[4];
    __shared__ u64 s_bits[4];
    __shared__ int s_idx[4];
    const int q = blockIdx.x, tid = threadIdx.x;
    double* x = v + (int64_t)q * n;
    const double* wq = w ? w + (int64_t)q * n : nullptr;
    unsigned char* sg = sgn + (int64_t)q * n;
    CondCol st = cols[q];   // (uniform; written back by thread 0 behind the barriers below)
    if (st.done) {
        for (int i = tid; i < n; i += kCThreads) x[i] = 0.0;
        return;
    }
    const bool post = wq && st.kase == 1;
    double sum = 0.0;
    u64 mb = 0;
    int mi = n, differ = 0;
    if (st.jump != 0) {
        for (int i = tid; i < n; i += kCThreads) {   // (ascending: the first index of a thread's largest magnitude)
            const double val = post ? x[i] * wq[i] : x[i];
            sum += fabs(val);
            const u64 b = abs_bits(val);
            if (mi == n || b > mb) mb = b, mi = i;
            if (st.jump == 3) differ |= (val >= 0.0 ? 1 : 0) != (int)sg[i];
        }
        for (int o = 32; o; o >>= 1) {
            sum += __shfl_xor(sum, o);
            const u64 ob = shfl_xor_u64(mb, o);
            const int oi = __shfl_xor(mi, o);
            if (ob > mb || (ob == mb && oi < mi)) mb = ob, mi = oi;
        }
        if ((tid & 63) == 0) s_sum[tid >> 6] = sum, s_bits[tid >> 6] = mb, s_idx[tid >> 6] = mi;
        differ = __syncthreads_or(differ);
        sum = (s_sum[0] + s_sum[1]) + (s_sum[2] + s_sum[3]);
        mb = s_bits[0], mi = s_idx[0];
        for (int k = 1; k < 4; ++k)
            if (s_bits[k] > mb || (s_bits[k] == mb && s_idx[k] < mi)) mb = s_bits[k], mi = s_idx[k];
    }
    int produce = kZero;
    switch (st.jump) {
    case 0:
        produce = kUniform, st.kase = 1, st.jump = 1;
        break;
    case 1:
        st.est = sum;
        if (n == 1) st.done = 1;
        else produce = kSigns, st.kase = 2, st.jump = 2;
        break;
    case 2:
        st.j = mi, st.iter = 2;
        produce = kUnit, st.kase = 1, st.jump = 3;
        break;
    case 3:
        st.estold = st.est, st.est = sum;
        if (!differ || st.est <= st.estold) produce = kAlternating, st.kase = 1, st.jump = 5;
        else produce = kSigns, st.kase = 2, st.jump = 4;
        break;
    case 4: {
        st.jlast = st.j, st.j = mi;
        const double last = post ? x[st.jlast] * wq[st.jlast] : x[st.jlast];
        if (fabs(last) != __longlong_as_double((long long)mb) && st.iter < 5)
            st.iter += 1, produce = kUnit, st.kase = 1, st.jump = 3;
        else
            produce = kAlternating, st.kase = 1, st.jump = 5;
        break;
    }
    default: {
        const double temp = 2.0 * (sum / (3.0 * (double)n));
        if (temp > st.est) st.est = temp;
        st.done = 1;
        break;
    }
    }
    __syncthreads();   // (every read of x above is done before x is overwritten)
    const bool pre = wq && !st.done && st.kase == 2;
    for (int i = tid; i < n; i += kCThreads) {
        double o = 0.0;
        if (produce == kUniform) {
            o = 1.0 / (double)n;
        } else if (produce == kSigns) {
            const double val = post ? x[i] * wq[i] : x[i];
            const int plus = val >= 0.0 ? 1 : 0;
            sg[i] = (unsigned char)plus;
            o = plus ? 1.0 : -1.0;
        } else if (produce == kUnit) {
            o = i == st.j ? 1.0 : 0.0;
        } else if (produce == kAlternating) {
            o = ((i & 1) ? -1.0 : 1.0) * (1.0 + (double)i / (double)(n - 1));
        }
        x[i] = pre ? o * wq[i] : o;
    }
    if (tid == 0) {
        cols[q] = st;
        if (!st.done) atomicAdd(&ctl[0], 1);
    }
}

// One workgroup per column: out[q] = est / max |z[:, q]| (est when that is 0) from nb partials per column.
// rcond (one column, the partials of k_sym_norm1): out[0] = anorm, out[1] = 1 / (anorm est), 0 when est is 0.
__global__ __launch_bounds__(kCThreads) void k_cond_finish(const CondCol* __restrict__ cols, const u64* __restrict__ part,
                                                           int nb, double* __restrict__ out, int rcond) {
    __shared__ u64 sm[4];
    const int q = blockIdx.x;
    u64 v = 0;
    for (int b = threadIdx.x; b < nb; b += kCThreads) v = max(v, part[(int64_t)q * nb + b]);
    v = block_max(v, sm);
    if (threadIdx.x != 0) return;
    const double top = __longlong_as_double((long long)v), est = cols[q].est;
    if (rcond) {
        out[0] = top;
        out[1] = est == 0.0 ? 0.0 : 1.0 / (top * est);
    } else {
        out[q] = top != 0.0 ? est / top : est;
    }
}

// the parts of CondState::cols
struct CondCols {
    u64* part;
    CondCol* col;
    double* out;
};

CondCols cond_cols(CondState& C) {
    CondCols c;
    char* p = C.cols.data();
    c.part = (u64*)p;
    p += (size_t)kRefinePartials * C.cols_cap * sizeof(u64);
    c.col = (CondCol*)p;
    p += (size_t)C.cols_cap * sizeof(CondCol);
    c.out = (double*)p;
    return c;
}

// w, the operand and the signs (n x nrhs each) and the per-column state, grown on demand
int ensure_cond(parsy_plan* pl, int nrhs) {
    if (!pl->cond) pl->cond = std::make_unique<CondState>(&pl->meter);
    CondState& C = *pl->cond;
    const int64_t nn = std::max<int64_t>((int64_t)pl->S.n * nrhs, 1);
    PARSY_HIP(hipSetDevice(pl->device));
    PARSY_HIP(C.ws.grow(2 * nn));
    PARSY_HIP(C.sgn.grow(nn));
    if (C.cols_cap < nrhs) {
        C.cols_cap = 0;
        static_assert(sizeof(CondCol) % 8 == 0, "the results behind the states are doubles");
        PARSY_HIP(C.cols.grow((int64_t)nrhs * (kRefinePartials * 8 + (int64_t)sizeof(CondCol) + 8) + 16));
        C.cols_cap = nrhs;
    }
    return 0;
}

// The estimator's loop over `ncols` columns of the operand v (w null: no weights): est of every column in its CondCol.
// ctl = {columns that go on, status of the solves}; the host reads it once per application.
int estimate(parsy_plan* pl, const char* who, const double* d_L, double* v, const double* w, int ncols, int* ctl,
             hipStream_t stream) {
    CondState& C = *pl->cond;
    const CondCols c = cond_cols(C);
    const int n = pl->S.n;
    C.applications = 0;
    PARSY_HIP(hipMemsetAsync(c.col, 0, (size_t)ncols * sizeof(CondCol), stream));
    if (n == 0) return 0;   // (est = 0)
    PARSY_HIP(hipMemsetAsync(ctl, 0, sizeof(int), stream));
    hipLaunchKernelGGL(k_cond_step, dim3(ncols), dim3(kCThreads), 0, stream, v, w, C.sgn.data(), c.col, n, ctl);
    PARSY_HIP(hipGetLastError());
    for (;;) {
        if (refine_solve_enqueue(pl, d_L, v, ncols, ctl, stream) != 0) return -1;
        C.applications += 1;
        PARSY_HIP(hipMemsetAsync(ctl, 0, sizeof(int), stream));
        hipLaunchKernelGGL(k_cond_step, dim3(ncols), dim3(kCThreads), 0, stream, v, w, C.sgn.data(), c.col, n, ctl);
        PARSY_HIP(hipGetLastError());
        int h[2] = {0, 0};
        PARSY_HIP(hipMemcpyAsync(h, ctl, sizeof(h), hipMemcpyDeviceToHost, stream));
        PARSY_HIP(hipStreamSynchronize(stream));
        if (h[1] < 0)
            return set_last_error(std::string(who) + ": a hand-off wait inside a chain launch timed out; nothing was returned"),
                   -1;
        if (h[0] == 0) return 0;
        if (C.applications >= kCondMaxApplications)
            return set_last_error(std::string(who) + ": the estimator went past its 11 applications (internal error)"), -1;
    }
}

}  // namespace

int cond_bounds_phase(parsy_plan* pl, const char* who, const double* d_L, int nrhs, double* ferr, hipStream_t stream) {
    if (ensure_cond(pl, nrhs) != 0) return -1;
    RefineState& R = *pl->refine;
    CondState& C = *pl->cond;
    C.columns = nrhs;
    const int64_t nn = (int64_t)pl->S.n * nrhs;
    const double *pb = R.ws.data(), *z = pb + nn;
    double *w = C.ws.data(), *v = w + std::max<int64_t>(nn, 1);
    const CondCols c = cond_cols(C);
    const int nb = sym_sweep_enqueue<WeightOut>(pl, R.d_vf, z, pb, w, nrhs, c.part, stream);
    if (nb < 0) return -1;
    if (estimate(pl, who, d_L, v, w, nrhs, col_state(R, R.colstate_cap).ctl, stream) != 0) return -1;
    hipLaunchKernelGGL(k_cond_finish, dim3(nrhs), dim3(kCThreads), 0, stream, c.col, c.part, nb, c.out, 0);
    PARSY_HIP(hipGetLastError());
    PARSY_HIP(hipMemcpyAsync(ferr, c.out, (size_t)nrhs * 8, hipMemcpyDeviceToHost, stream));
    PARSY_HIP(hipStreamSynchronize(stream));
    return 0;
}

int plan_error_bounds(parsy_plan* pl, const double* d_values, const double* d_L, const double* d_x, int ldx,
                      const double* d_b, int ldb, int nrhs, double* ferr, double* berr, hipStream_t stream) {
    const char* who = "parsy_error_bounds_device";
    if (check_plan(pl, who, kNeedsIdle) != 0) return -1;
    const int n = pl->S.n;
    if (nrhs < 1 || nrhs > 65535 || ldx < n || ldb < n)
        return set_last_error(std::string(who) + ": need 1 <= nrhs <= 65535 and leading dimensions >= n"), -1;
    const int* perm = nullptr;
    if (refine_ensure_pattern(pl) != 0 || refine_ensure_workspace(pl, nrhs, &perm) != 0) return -1;
    RefineState& R = *pl->refine;
    const int64_t nn = (int64_t)n * nrhs;
    double *pb = R.ws.data(), *z = pb + nn, *r = pb + 2 * nn;
    const ColState c = col_state(R, R.colstate_cap);
    PARSY_HIP(hipMemsetAsync(c.ctl, 0, 2 * sizeof(int), stream));
    if (refine_gather_values(pl, d_values, R.d_vf, stream) != 0) return -1;
    enqueue_perm_gather(perm, d_x, ldx, z, nullptr, n, nrhs, stream);
    enqueue_perm_gather(perm, d_b, ldb, pb, nullptr, n, nrhs, stream);
    const int nb = refine_residual_enqueue(pl, z, pb, r, nrhs, c.part, stream);
    if (nb < 0 || refine_report_berr(pl, nb, nrhs, stream) != 0) return -1;
    if (ferr && cond_bounds_phase(pl, who, d_L, nrhs, ferr, stream) != 0) return -1;
    if (berr) {
        PARSY_HIP(hipMemcpyAsync(berr, c.berr, (size_t)nrhs * 8, hipMemcpyDeviceToHost, stream));
        PARSY_HIP(hipStreamSynchronize(stream));
    }
    return 0;
}

int plan_rcond(parsy_plan* pl, const double* d_values, const double* d_L, double* anorm, double* rcond,
               hipStream_t stream) {
    const char* who = "parsy_rcond_device";
    if (check_plan(pl, who, kNeedsIdle) != 0) return -1;
    const int* perm = nullptr;   // (not read here: the workspace call uploads it as it always has)
    if (refine_ensure_pattern(pl) != 0 || refine_ensure_workspace(pl, 1, &perm) != 0 || ensure_cond(pl, 1) != 0) return -1;
    RefineState& R = *pl->refine;
    CondState& C = *pl->cond;
    C.columns = 1;
    C.applications = 0;
    const int n = pl->S.n;
    const ColState rc = col_state(R, R.colstate_cap);
    const CondCols c = cond_cols(C);
    PARSY_HIP(hipMemsetAsync(rc.ctl, 0, 2 * sizeof(int), stream));
    PARSY_HIP(hipMemsetAsync(c.col, 0, sizeof(CondCol), stream));
    if (refine_gather_values(pl, d_values, R.d_vf, stream) != 0) return -1;
    const int nb = sym_sweep_blocks(n, kCThreads / R.group);
    dispatch_int(R.group, SweepGroups(), [&](auto g) {
        hipLaunchKernelGGL(k_sym_norm1<decltype(g)::value>, dim3(nb), dim3(kCThreads), 0, stream, R.d_rp, R.d_vf, n, c.part);
    });
    PARSY_HIP(hipGetLastError());
    if (rcond && estimate(pl, who, d_L, C.ws.data() + std::max(n, 1), nullptr, 1, rc.ctl, stream) != 0) return -1;
    hipLaunchKernelGGL(k_cond_finish, dim3(1), dim3(kCThreads), 0, stream, c.col, c.part, nb, c.out, 1);
    PARSY_HIP(hipGetLastError());
    double h[2] = {0, 0};
    PARSY_HIP(hipMemcpyAsync(h, c.out, sizeof(h), hipMemcpyDeviceToHost, stream));
    PARSY_HIP(hipStreamSynchronize(stream));
    if (anorm) *anorm = h[0];
    if (rcond) *rcond = h[1];
    return 0;
}

}  // namespace parsy

extern "C" int parsy_cond_get_info(parsy_plan* pl, parsy_cond_info* info) {
    if (!pl || !info) {
        parsy::set_last_error("parsy_cond_get_info: null argument");
        return -1;
    }
    const parsy::CondState* C = pl->cond.get();
    info->applications = C ? C->applications : 0;
    info->columns = C ? C->columns : 0;
    info->device_bytes = C ? C->meter.bytes : 0;
    return 0;
}
