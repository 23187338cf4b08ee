// Row delete and row add in the factor on the device (rowmod.hpp).  Every launch is ordered against the others by the
// stream alone: no flags, no tickets, no waits between workgroups, no floating-point atomics; every output element has
// one summation order.
//
//   k_rowadd_solve    one workgroup per supernode of one height of T(p): y_j = a_j - sum of row j's occurrences in T
//                     (ascending position) for its ks columns, then the solve with the leading ks x ks triangle of its
//                     diagonal block in block columns of 64 -- the tile's lower triangle in LDS, one wave runs its 64
//                     steps, all four waves apply the block column to the rest of y (a lane per row) -- and y into row p
//                     of the panel
//   k_rowadd_panel    the panel rows below those ks columns, a lane per row, 256 rows a workgroup: y in LDS in chunks of
//                     256 columns (read as broadcasts), one fma chain per row in ascending column order, one store into
//                     T.  For a fixed column consecutive lanes read consecutive doubles of the panel.  Row p itself holds
//                     y by then, so its entry of T is y . y
//   k_rowadd_column   l22 = sqrt(a22 - sum T) and column p, l32 = (a32 - sum T) / l22, into L and into column 0 of
//                     updown's workspace; a pivot that fails is reported and leaves the identity's column
//   k_rowdel_take     column p into the workspace, zero in L, the diagonal 1
//   k_rowdel_zero     row p of every panel of T(p)
//   k_rowmod_clear    the ranges of T and y that an add has written
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
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

constexpr int kRThreads = 256;
static_assert(kRowmodRows == kRThreads, "k_rowadd_panel: a lane per row, a column of y per thread of a chunk");
static_assert(kRowmodTile == 64, "k_rowadd_solve: one wave, a lane per row of the tile");

// The new column in the factor's ordering: nz rows ascending (arow), where each value stands in cx (asrc).
struct ColumnView {
    const int32_t* arow;
    const int32_t* asrc;
    const double* cx;
    int nz;
};
__device__ __forceinline__ double a_at(const ColumnView& A, int row) {
    int lo = 0, hi = A.nz;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (A.arow[mid] < row) lo = mid + 1;
        else hi = mid;
    }
    return (lo < A.nz && A.arow[lo] == row) ? A.cx[A.asrc[lo]] : 0.0;
}
// a_row minus the occurrences of `row` in T, in ascending position
__device__ __forceinline__ double gather_row(const ColumnView& A, int row, const int64_t* __restrict__ ptr,
                                             const int64_t* __restrict__ pos, const double* __restrict__ T) {
    double acc = a_at(A, row);
    for (int64_t e = ptr[row]; e < ptr[row + 1]; ++e) acc -= T[pos[e]];
    return acc;
}

__global__ __launch_bounds__(kRThreads) void k_rowadd_solve(double* __restrict__ L, const RowmodDesc* __restrict__ nodes,
                                                            ColumnView A, const int64_t* __restrict__ ptr,
                                                            const int64_t* __restrict__ pos, const double* __restrict__ T,
                                                            double* __restrict__ y) {
    __shared__ double tile[kRowmodTile * kRowmodTile];   // column-major lower triangle of the diagonal tile
    __shared__ double yb[kRowmodTile];                   // the solved block of y
    const RowmodDesc D = nodes[blockIdx.x];
    const int tid = threadIdx.x, ks = D.ks;
    const int64_t r = D.r;
    double* __restrict__ ys = y + D.c0;
    for (int j = tid; j < ks; j += kRThreads) ys[j] = gather_row(A, D.c0 + j, ptr, pos, T);
    __syncthreads();
    for (int cb = 0; cb < ks; cb += kRowmodTile) {
        const int nc = min(kRowmodTile, ks - cb);
        const double* __restrict__ g = L + D.px + (int64_t)cb * r + cb;
        for (int e = tid; e < kRowmodTile * kRowmodTile; e += kRThreads) {
            const int j = e >> 6, i = e & 63;
            tile[e] = (i < nc && j < nc && i >= j) ? g[(int64_t)j * r + i] : 0.0;   // (never the strict upper triangle)
        }
        __syncthreads();
        if (tid < 64) {
            const int i = tid;
            double x = i < nc ? ys[cb + i] : 0.0;
            for (int j = 0; j < nc; ++j) {
                const double xj = __shfl(x, j) / tile[j * kRowmodTile + j];   // lane j's x is final at step j
                if (i == j) x = xj;
                else if (i > j) x = fma(-tile[j * kRowmodTile + i], xj, x);
            }
            if (i < nc) ys[cb + i] = x, yb[i] = x;
        }
        __syncthreads();
        // (the apply: a lane asks for its row of the block column before it waits for anything)
        for (int i = cb + nc + tid; i < ks; i += kRThreads) {
            const double* __restrict__ row = L + D.px + (int64_t)cb * r + i;
            double v[kRowmodTile];
#pragma unroll
            for (int j = 0; j < kRowmodTile; ++j) v[j] = j < nc ? row[(int64_t)j * r] : 0.0;
            double acc = ys[i];
#pragma unroll
            for (int j = 0; j < kRowmodTile; ++j)
                if (j < nc) acc = fma(-v[j], yb[j], acc);
            ys[i] = acc;
        }
        __syncthreads();
    }
    double* __restrict__ out = L + D.px + D.q;
    for (int j = tid; j < ks; j += kRThreads) out[(int64_t)j * r] = ys[j];
}

// blk: (supernode of `nodes`, first row) per workgroup
__global__ __launch_bounds__(kRThreads) void k_rowadd_panel(const double* __restrict__ L, const RowmodDesc* __restrict__ nodes,
                                                            const int32_t* __restrict__ blk, const double* __restrict__ y,
                                                            double* __restrict__ T) {
    __shared__ double ys[kRowmodRows];
    const RowmodDesc D = nodes[blk[2 * blockIdx.x]];
    const int i = blk[2 * blockIdx.x + 1] + threadIdx.x;
    const bool on = i < D.r;
    const int64_t r = D.r;
    const double* __restrict__ row = L + D.px + (on ? i : D.r - 1);   // (lanes past the panel store nothing)
    double acc = 0.0;
    for (int cb = 0; cb < D.ks; cb += kRowmodRows) {
        const int nc = min(kRowmodRows, D.ks - cb);
        __syncthreads();
        if ((int)threadIdx.x < nc) ys[threadIdx.x] = y[D.c0 + cb + threadIdx.x];
        __syncthreads();
        const double* __restrict__ col = row + (int64_t)cb * r;
#pragma unroll 16
        for (int c = 0; c < nc; ++c) acc = fma(col[(int64_t)c * r], ys[c], acc);
    }
    if (on) T[D.pi + i] = acc;
}

// Column p of the panel at px (r rows, p at position q; rows: the panel's row list); one workgroup per 256 rows from q on.
__global__ __launch_bounds__(kRThreads) void k_rowadd_column(double* __restrict__ L, int64_t px, int r, int q, int p,
                                                             const int32_t* __restrict__ rows, ColumnView A,
                                                             const int64_t* __restrict__ ptr, const int64_t* __restrict__ pos,
                                                             const double* __restrict__ T, double* __restrict__ W,
                                                             int* __restrict__ status) {
    __shared__ double pivot;
    if (threadIdx.x == 0) {
        const double d2 = gather_row(A, p, ptr, pos, T);   // a22 - l12' l12, the same in every workgroup
        const bool ok = d2 > 0.0 && d2 < HUGE_VAL;
        pivot = ok ? sqrt(d2) : 0.0;
        if (!ok && blockIdx.x == 0) atomicMin(status, p + 1);
    }
    __syncthreads();
    const double l22 = pivot;
    const bool ok = l22 > 0.0;
    const int i = q + blockIdx.x * kRThreads + threadIdx.x;
    if (i >= r) return;
    double* __restrict__ col = L + px + (int64_t)q * r;
    if (i == q) {
        col[i] = ok ? l22 : 1.0;
    } else if (!ok) {
        col[i] = 0.0;
    } else {
        const int row = rows[i];
        const double v = gather_row(A, row, ptr, pos, T) / l22;
        col[i] = v;
        W[(int64_t)row * kUpdownBlock] = v;
    }
}

__global__ __launch_bounds__(kRThreads) void k_rowdel_take(double* __restrict__ L, int64_t px, int r, int q,
                                                           const int32_t* __restrict__ rows, double* __restrict__ W) {
    const int i = q + blockIdx.x * kRThreads + threadIdx.x;
    if (i >= r) return;
    double* __restrict__ col = L + px + (int64_t)q * r;
    if (i == q) {
        col[i] = 1.0;
    } else {
        W[(int64_t)rows[i] * kUpdownBlock] = col[i];
        col[i] = 0.0;
    }
}

// seg[0 .. nn]: prefix sums of the supernodes' lengths (ks, or r); the supernode of a flat index
__device__ __forceinline__ int segment_of(const int64_t* __restrict__ seg, int nn, int64_t idx) {
    int lo = 0, hi = nn - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (seg[mid] <= idx) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

__global__ __launch_bounds__(kRThreads) void k_rowdel_zero(double* __restrict__ L, const RowmodDesc* __restrict__ nodes,
                                                           const int64_t* __restrict__ seg, int nn) {
    const int64_t idx = (int64_t)blockIdx.x * kRThreads + threadIdx.x;
    if (idx >= seg[nn]) return;
    const int s = segment_of(seg, nn, idx);
    const RowmodDesc D = nodes[s];
    L[D.px + (idx - seg[s]) * D.r + D.q] = 0.0;
}

__global__ __launch_bounds__(kRThreads) void k_rowmod_clear(const RowmodDesc* __restrict__ nodes, const int64_t* __restrict__ seg,
                                                            int nn, double* __restrict__ T, double* __restrict__ y) {
    const int64_t idx = (int64_t)blockIdx.x * kRThreads + threadIdx.x;
    if (idx >= seg[nn]) return;
    const int s = segment_of(seg, nn, idx);
    const RowmodDesc D = nodes[s];
    const int64_t i = idx - seg[s];
    if (i < D.ks) y[D.c0 + i] = 0.0;   // its columns of y; the rows below them in T
    else T[D.pi + i] = 0.0;
}

unsigned blocks_of(int64_t items, int per_block) { return (unsigned)std::max<int64_t>(1, (items + per_block - 1) / per_block); }

int ensure_device(parsy_plan* pl) {
    if (rowmod_ensure_host(pl) != 0) return -1;
    RowmodState& R = *pl->rowmod;
    PARSY_HIP(hipSetDevice(pl->device));
    if (R.on_device) return 0;
    DevicePool pool(&R.meter);
    const int64_t tlen = std::max<int64_t>((int64_t)pl->S.rows.size(), 1), ylen = std::max<int64_t>(pl->S.n, 1);
    int64_t* d_ptr = pool.upload(R.I.ptr);
    int64_t* d_pos = pool.upload(R.I.pos);
    double* d_t = pool.alloc<double>(tlen);
    double* d_y = pool.alloc<double>(ylen);
    if (pool.error() != hipSuccess) return pool_failed(pool);
    PARSY_HIP(hipMemset(d_t, 0, (size_t)tlen * sizeof(double)));
    PARSY_HIP(hipMemset(d_y, 0, (size_t)ylen * sizeof(double)));
    PARSY_HIP(hipDeviceSynchronize());   // (once per plan: the caller's stream may not wait for the null stream)
    R.fixed = std::move(pool);
    R.d_ptr = d_ptr, R.d_pos = d_pos, R.d_t = d_t, R.d_y = d_y;
    R.on_device = true;
    return 0;
}

// T(p) grouped by height (stable: ascending inside a height) as the kernels read it, and the first supernode of every
// height
void group_by_height(const Schedule& S, const std::vector<RowmodNode>& reach, std::vector<RowmodDesc>& desc,
                     std::vector<int>& first) {
    int nh = 0;
    for (const RowmodNode& N : reach) nh = std::max(nh, N.height + 1);
    first.assign((size_t)nh + 1, 0);
    for (const RowmodNode& N : reach) ++first[(size_t)N.height + 1];
    for (int h = 0; h < nh; ++h) first[(size_t)h + 1] += first[(size_t)h];
    desc.resize(reach.size());
    std::vector<int> next(first.begin(), first.end() - 1);
    for (const RowmodNode& N : reach) {
        const SnDesc& D = S.sn[(size_t)N.sn];
        desc[(size_t)next[(size_t)N.height]++] = RowmodDesc{D.px, D.pi, D.c0, D.r, N.ks, N.pos};
    }
}

// what both calls do before their first launch: the refusals that remain, the states, T(p)
int begin_call(parsy_plan* pl, const char* who, int op, int p, std::vector<RowmodNode>& reach, hipStream_t stream) {
    if (pl->sn_mask_set || pl->piece_mask_set)
        return set_last_error(std::string(who) + ": plan is restricted by parsy_plan_set_active / _set_active_pieces"), -1;
    if (check_plan(pl, who, kNeedsDevice) != 0) return -1;
    if (ensure_device(pl) != 0) return -1;
    if (plan_updown_status_reset(pl, stream) != 0) return -1;
    RowmodState& R = *pl->rowmod;
    rowmod_reach(pl->S, R.I, p, reach);
    R.last_op = op, R.last_row = p;
    R.reach = (int)reach.size(), R.heights = 0;
    for (const RowmodNode& N : reach) R.heights = std::max(R.heights, N.height + 1);
    R.row_launches = R.column_launches = R.rotation_launches = 0;
    R.entries_read = R.entries_walked = 0;
    return 0;
}

}  // namespace

int rowmod_ensure_host(parsy_plan* pl) {
    if (!pl->rowmod) pl->rowmod = std::make_unique<RowmodState>(&pl->meter);
    RowmodState& R = *pl->rowmod;
    if (!R.built) {
        build_apply_index(pl->S, R.I);
        R.built = true;
    }
    return 0;
}

int rowdel_check_args(parsy_plan* pl, const char* who, const void* lValues, int row, int* p) {
    if (!pl || !lValues) return set_last_error(std::string(who) + ": null argument"), -1;
    const int at = rowmod_position(pl->S, plan_perm_inverse(pl), who, row);
    if (p) *p = at;
    return at < 0 ? -1 : 0;
}

int rowadd_check_args(parsy_plan* pl, const char* who, const void* lValues, int row, int nz, const void* ci,
                      const void* cx, RowmodColumn& col) {
    if (!pl || !lValues || !ci || !cx) return set_last_error(std::string(who) + ": null argument"), -1;
    return rowadd_prepare(pl->S, plan_perm_inverse(pl), who, row, nz, static_cast<const int*>(ci), col);
}

int plan_factor_rowdel(parsy_plan* pl, double* d_L, int row, void* stream_) {
    const char* who = "parsy_factor_rowdel_device";
    hipStream_t stream = (hipStream_t)stream_;
    int p = -1;
    if (rowdel_check_args(pl, who, d_L, row, &p) != 0) return -1;
    const Schedule& S = pl->S;
    std::vector<RowmodNode> reach;
    if (begin_call(pl, who, 1, p, reach, stream) != 0) return -1;
    RowmodState& R = *pl->rowmod;
    UpdownWalk walk;
    if (plan_updown_walk_begin(pl, rowmod_first_below(S, p), walk, stream) != 0) return -1;
    const int nn = (int)reach.size();
    std::vector<RowmodDesc> desc;
    std::vector<int> first;
    group_by_height(S, reach, desc, first);
    std::vector<int64_t> seg((size_t)nn + 1, 0);
    for (int i = 0; i < nn; ++i) seg[(size_t)i + 1] = seg[(size_t)i] + desc[(size_t)i].ks;
    if (nn > 0) {
        PARSY_HIP(R.nodes.grow(nn));
        PARSY_HIP(R.segs.grow(nn + 1));
        PARSY_HIP(hipMemcpyAsync(R.nodes.data(), desc.data(), desc.size() * sizeof(RowmodDesc), hipMemcpyHostToDevice, stream));
        PARSY_HIP(hipMemcpyAsync(R.segs.data(), seg.data(), seg.size() * sizeof(int64_t), hipMemcpyHostToDevice, stream));
    }
    PARSY_HIP(hipStreamSynchronize(stream));   // (the host arrays end with this call)

    const dim3 threads(kRThreads);
    const SnDesc& D = S.sn[(size_t)supernode_of(S, p)];
    const int q = p - D.c0;
    hipLaunchKernelGGL(k_rowdel_take, dim3(blocks_of(D.r - q, kRThreads)), threads, 0, stream, d_L, D.px, D.r, q,
                       pl->dp.rows + D.pi, plan_updown_workspace(pl));
    ++R.column_launches;
    if (nn > 0) {
        hipLaunchKernelGGL(k_rowdel_zero, dim3(blocks_of(seg[(size_t)nn], kRThreads)), threads, 0, stream, d_L, R.nodes.data(),
                           R.segs.data(), nn);
        ++R.row_launches;
    }
    PARSY_HIP(hipGetLastError());
    if (plan_updown_walk_run(pl, d_L, +1, walk, stream) != 0) return -1;
    R.rotation_launches = walk.launches, R.entries_walked = walk.entries;
    return 0;
}

int plan_factor_rowadd(parsy_plan* pl, double* d_L, int row, int nz, const int* ci, const double* d_cx, void* stream_) {
    const char* who = "parsy_factor_rowadd_device";
    hipStream_t stream = (hipStream_t)stream_;
    RowmodColumn col;
    if (rowadd_check_args(pl, who, d_L, row, nz, ci, d_cx, col) != 0) return -1;
    const Schedule& S = pl->S;
    const int p = col.p;
    std::vector<RowmodNode> reach;
    if (begin_call(pl, who, 2, p, reach, stream) != 0) return -1;
    RowmodState& R = *pl->rowmod;
    R.entries_read = rowmod_entries_read(S, reach);
    UpdownWalk walk;
    if (plan_updown_walk_begin(pl, rowmod_first_below(S, p), walk, stream) != 0) return -1;

    // T(p) by height, the panel launches' workgroups, the clearing's prefix sums and the column's pattern go up in
    // one piece each, before the first launch
    const int nn = (int)reach.size();
    std::vector<RowmodDesc> desc;
    std::vector<int> first;
    group_by_height(S, reach, desc, first);
    const int nh = (int)first.size() - 1;
    std::vector<int64_t> seg((size_t)nn + 1, 0);
    std::vector<int32_t> ints;
    std::vector<int> blk_first((size_t)nh + 1, 0);   // per height: its first workgroup of k_rowadd_panel
    for (int h = 0; h < nh; ++h) {
        for (int i = first[(size_t)h]; i < first[(size_t)h + 1]; ++i)
            for (int row0 = desc[(size_t)i].ks; row0 < desc[(size_t)i].r; row0 += kRowmodRows) ints.push_back(i), ints.push_back(row0);
        blk_first[(size_t)h + 1] = (int)ints.size() / 2;
    }
    for (int i = 0; i < nn; ++i) seg[(size_t)i + 1] = seg[(size_t)i] + desc[(size_t)i].r;
    const int64_t a0 = (int64_t)ints.size();
    ints.insert(ints.end(), col.row.begin(), col.row.end());
    ints.insert(ints.end(), col.src.begin(), col.src.end());
    PARSY_HIP(R.nodes.grow(std::max(nn, 1)));
    PARSY_HIP(R.segs.grow(nn + 1));
    PARSY_HIP(R.ints.grow((int64_t)ints.size()));
    if (nn > 0)
        PARSY_HIP(hipMemcpyAsync(R.nodes.data(), desc.data(), desc.size() * sizeof(RowmodDesc), hipMemcpyHostToDevice, stream));
    PARSY_HIP(hipMemcpyAsync(R.segs.data(), seg.data(), seg.size() * sizeof(int64_t), hipMemcpyHostToDevice, stream));
    PARSY_HIP(hipMemcpyAsync(R.ints.data(), ints.data(), ints.size() * sizeof(int32_t), hipMemcpyHostToDevice, stream));
    PARSY_HIP(hipStreamSynchronize(stream));   // (the host arrays end with this call)

    const dim3 threads(kRThreads);
    const int cnz = (int)col.row.size();
    const ColumnView A{R.ints.data() + a0, R.ints.data() + a0 + cnz, d_cx, cnz};
    for (int h = 0; h < nh; ++h) {
        const int n_h = first[(size_t)h + 1] - first[(size_t)h];
        hipLaunchKernelGGL(k_rowadd_solve, dim3((unsigned)n_h), threads, 0, stream, d_L, R.nodes.data() + first[(size_t)h], A,
                           R.d_ptr, R.d_pos, R.d_t, R.d_y);
        ++R.row_launches;
        const int nb = blk_first[(size_t)h + 1] - blk_first[(size_t)h];
        if (nb > 0) {
            hipLaunchKernelGGL(k_rowadd_panel, dim3((unsigned)nb), threads, 0, stream, d_L, R.nodes.data(),
                               R.ints.data() + 2 * (int64_t)blk_first[(size_t)h], R.d_y, R.d_t);
            ++R.row_launches;
        }
    }
    const SnDesc& D = S.sn[(size_t)supernode_of(S, p)];
    const int q = p - D.c0;
    int32_t* const d_status = plan_updown_status_word(pl);
    hipLaunchKernelGGL(k_rowadd_column, dim3(blocks_of(D.r - q, kRThreads)), threads, 0, stream, d_L, D.px, D.r, q, p,
                       pl->dp.rows + D.pi, A, R.d_ptr, R.d_pos, R.d_t, plan_updown_workspace(pl), d_status);
    ++R.column_launches;
    if (nn > 0) {
        hipLaunchKernelGGL(k_rowmod_clear, dim3(blocks_of(seg[(size_t)nn], kRThreads)), threads, 0, stream, R.nodes.data(),
                           R.segs.data(), nn, R.d_t, R.d_y);
        ++R.row_launches;
    }
    PARSY_HIP(hipGetLastError());
    if (walk.path.empty()) return 0;
    // no downdate behind a pivot that failed: the call waits for the column and reads the status word
    int32_t st = 0;
    PARSY_HIP(hipMemcpyAsync(&st, d_status, sizeof(int32_t), hipMemcpyDeviceToHost, stream));
    PARSY_HIP(hipStreamSynchronize(stream));
    if (st == p + 1) return 0;
    if (plan_updown_walk_run(pl, d_L, -1, walk, stream) != 0) return -1;
    R.rotation_launches = walk.launches, R.entries_walked = walk.entries;
    return 0;
}

}  // namespace parsy
