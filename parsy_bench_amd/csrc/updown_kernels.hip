// Update / downdate of the factor on the device (updown.hpp).  Every launch is ordered against the others by the stream
// alone: no flags, no tickets, no waits between workgroups, no floating-point atomics.
//
//   k_updown_scatter_w   the <= kUpdownBlock columns of W under way into the zeroed workspace (a row's columns contiguous)
//   k_updown_diag        one workgroup per block column: the lower triangle of its diagonal tile in LDS and the tile's rows
//                        of the workspace in the registers of one wave (a lane per row), which runs the tile's rotations
//                        in order, leaves (1/c, sigma s, c, -s) of each in the coefficient table and reports a pivot
//                        that failed
//   k_updown_rows<NB>    every panel row below that tile, a lane per row, 256 rows a workgroup: the row's NB values of
//                        W in registers, the table in LDS (read as broadcasts), the block column's columns in ascending
//                        order -- for a fixed column consecutive lanes touch consecutive doubles of the panel
//   k_updown_clear_w     zeroes the workspace rows of the path's row lists (what a failed pivot has left behind)
//
// A rotation whose w is zero is skipped (k_updown_diag) or is exactly the identity (k_updown_rows: coefficients 1, 0, 1, 0).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
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

constexpr int kUThreads = 256;
constexpr int kUNoFailure = 0x7f7f7f7f;   // the status word between failures (a memset of 0x7f)
static_assert(kUpdownRows == kUThreads, "k_updown_rows: a lane per row");
static_assert(kUpdownTile == 64 && kUpdownBlock < 63, "k_updown_diag: one wave, a lane per row of the tile");
static_assert(kUpdownCoef == 4, "the kernels read a rotation as one double4");

__global__ __launch_bounds__(kUThreads) void k_updown_scatter_w(const int32_t* __restrict__ row, const int32_t* __restrict__ col,
                                                                const int32_t* __restrict__ src, int nnz,
                                                                const double* __restrict__ wx, double* __restrict__ W) {
    const int e = blockIdx.x * kUThreads + threadIdx.x;
    if (e < nnz) W[(int64_t)row[e] * kUpdownBlock + col[e]] = wx[src[e]];
}

// segments: seg[0 .. nseg] the prefix sums of the row lists' lengths, seg[nseg + 1 + s] the offset of list s in lR
__global__ __launch_bounds__(kUThreads) void k_updown_clear_w(const int64_t* __restrict__ seg, int nseg,
                                                              const int32_t* __restrict__ rows, double* __restrict__ W) {
    const int64_t idx = (int64_t)blockIdx.x * kUThreads + threadIdx.x;
    if (idx >= seg[nseg]) return;
    int lo = 0, hi = nseg - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (seg[mid] <= idx) lo = mid;
        else hi = mid - 1;
    }
    double* __restrict__ w = W + (int64_t)rows[seg[nseg + 1 + lo] + (idx - seg[lo])] * kUpdownBlock;
#pragma unroll
    for (int t = 0; t < kUpdownBlock; ++t) w[t] = 0.0;
}

// The tile is the nc x nc lower triangle at (cb, cb) of the panel at px (r rows); the rotations start at its column j0.
// gcol0: the factor's column of the tile's first column = its first row of the workspace.
// Four waves load and store the tile (sixteen loads in flight per lane); the first wave runs the rotations, a lane per
// row.  Per column j the squares of the pivots are one short chain, q_0 = d^2, q_(t+1) = q_t + sigma w_t^2 (a rotation with
// w_t == 0 or a failed pivot leaves q as it is), so that lane t can take the roots of q_t and q_(t+1) and form its
// rotation beside the others: the pivot before rotation t is sqrt(q_t), after it sqrt(q_(t+1)).
__global__ __launch_bounds__(kUThreads) void k_updown_diag(double* __restrict__ L, int64_t px, int r, int cb, int nc, int j0,
                                                           int gcol0, double sigma, double* __restrict__ W,
                                                           double* __restrict__ coef, int* __restrict__ status) {
    __shared__ double T[kUpdownTile * kUpdownTile];   // column-major: lane i owns row i, everyone reads the diagonal
    __shared__ __align__(16) double tab_[kUpdownTile * kUpdownBlock * kUpdownCoef];
    constexpr int kPer = kUpdownTile * kUpdownTile / kUThreads;   // entries of the tile per thread
    const int i = threadIdx.x & 63, jq = threadIdx.x >> 6;
    const bool on = i < nc;
    double* __restrict__ g = L + px + (int64_t)cb * r + cb;
    {
        double v[kPer];
#pragma unroll
        for (int m = 0; m < kPer; ++m) {
            const int j = jq + (kUThreads / 64) * m;
            v[m] = (on && j >= j0 && j < nc && i >= j) ? g[(int64_t)j * r + i] : 0.0;   // (never the strict upper triangle)
        }
#pragma unroll
        for (int m = 0; m < kPer; ++m) T[(jq + (kUThreads / 64) * m) * kUpdownTile + i] = v[m];
    }
    __syncthreads();
    if (threadIdx.x < 64) {
        double4* __restrict__ tab = reinterpret_cast<double4*>(tab_);
        double w[kUpdownBlock];
        double* __restrict__ wrow = W + (int64_t)(gcol0 + (on ? i : 0)) * kUpdownBlock;
#pragma unroll
        for (int t = 0; t < kUpdownBlock; ++t) w[t] = on ? wrow[t] : 0.0;
        for (int j = j0; j < nc; ++j) {
            const double d0 = T[j * kUpdownTile + j];
            const bool below = on && i > j;
            double x = below ? T[j * kUpdownTile + i] : 0.0;
            // the chain of squares, the same in every lane; lane t keeps w_t, lane t + 1 keeps q_(t+1)
            const bool d_ok = fabs(d0) > 0.0;
            double q = d0 * d0, my_q = q, my_w = 0.0;
            unsigned used = 0;
            bool failed = false;
#pragma unroll
            for (int t = 0; t < kUpdownBlock; ++t) {
                const double wj = __shfl(w[t], j);
                if (wj != 0.0) {
                    const double qn = fma(sigma * wj, wj, q);
                    if (!(qn > 0.0) || !(qn < HUGE_VAL) || !d_ok) failed = true;   // the rotation is left out
                    else q = qn, used |= 1u << t;
                }
                if (i == t) my_w = wj;
                if (i == t + 1) my_q = q;
            }
            // the first failure of the call is the smallest column
            if (failed && i == 0) atomicMin(status, gcol0 + j + 1);
            const double root = i == 0 ? d0 : sqrt(my_q);   // lane t: the pivot before rotation t
            const double next = __shfl_down(root, 1);       // ... and after it
            if (i < kUpdownBlock) {
                double4 co = make_double4(1.0, 0.0, 1.0, 0.0);
                if ((used >> i) & 1u) {
                    const double s = my_w / root;
                    co = make_double4(root / next, sigma * s, next / root, -s);
                }
                tab[j * kUpdownBlock + i] = co;
            }
            __builtin_amdgcn_wave_barrier();   // (one wave: its LDS accesses are served in order)
#pragma unroll
            for (int t = 0; t < kUpdownBlock; ++t) {
                if ((used >> t) & 1u) {
                    const double4 co = tab[j * kUpdownBlock + t];
                    if (below) {
                        x = fma(co.y, w[t], x) * co.x;
                        w[t] = fma(co.w, x, co.z * w[t]);
                    } else if (i == j) {
                        w[t] = 0.0;
                    }
                }
            }
            const double d_new = __shfl(root, kUpdownBlock);   // sqrt of the last q
            if (below) T[j * kUpdownTile + i] = x;
            else if (i == j && used) T[j * kUpdownTile + j] = d_new;
        }
        if (on) {
#pragma unroll
            for (int t = 0; t < kUpdownBlock; ++t) wrow[t] = w[t];
        }
    }
    __syncthreads();
#pragma unroll
    for (int m = 0; m < kPer; ++m) {
        const int j = jq + (kUThreads / 64) * m;
        if (on && j >= j0 && j < nc && i >= j) g[(int64_t)j * r + i] = T[j * kUpdownTile + i];
    }
    for (int e = j0 * kUpdownBlock * kUpdownCoef + threadIdx.x; e < nc * kUpdownBlock * kUpdownCoef; e += kUThreads)
        coef[e] = tab_[e];
}

template <int NB>
__device__ __forceinline__ void rotate_row(const double4* __restrict__ tab, int j, double& x, double (&w)[NB]) {
#pragma unroll
    for (int t = 0; t < NB; ++t) {
        const double4 q = tab[j * kUpdownBlock + t];   // 1/c, sigma s, c, -s: the same address for every lane
        x = fma(q.y, w[t], x) * q.x;
        w[t] = fma(q.w, x, q.z * w[t]);
    }
}

// The panel rows [row0, r) under the columns [cb + j0, cb + nc) of the panel at px; rows: the panel's row list.
// A lane asks for its whole row of the block column before it waits for anything (one round of memory latency), rotates
// it column by column and stores every entry once.
template <int NB>
__global__ __launch_bounds__(kUThreads) void k_updown_rows(double* __restrict__ L, int64_t px, int r, int cb, int nc, int j0,
                                                           int row0, const int32_t* __restrict__ rows,
                                                           const double* __restrict__ coef, double* __restrict__ W) {
    __shared__ __align__(16) double tab_[kUpdownTile * kUpdownBlock * kUpdownCoef];
    const int i = row0 + blockIdx.x * kUThreads + threadIdx.x;
    const bool on = i < r;
    double* __restrict__ col = L + px + (int64_t)cb * r + (on ? i : r - 1);   // (lanes past the panel store nothing)
    const int64_t ld = r;
    double x[kUpdownTile];
#pragma unroll
    for (int j = 0; j < kUpdownTile; ++j) x[j] = (j >= j0 && j < nc) ? col[j * ld] : 0.0;
    double* __restrict__ wrow = W + (int64_t)rows[on ? i : r - 1] * kUpdownBlock;
    double w[NB];
#pragma unroll
    for (int t = 0; t < NB; ++t) w[t] = wrow[t];
    for (int e = j0 * kUpdownBlock * kUpdownCoef + threadIdx.x; e < nc * kUpdownBlock * kUpdownCoef; e += kUThreads)
        tab_[e] = coef[e];
    __syncthreads();
    if (!on) return;
    const double4* __restrict__ tab = reinterpret_cast<const double4*>(tab_);
#pragma unroll
    for (int j = 0; j < kUpdownTile; ++j) {
        if (j >= j0 && j < nc) {
            rotate_row<NB>(tab, j, x[j], w);
            col[j * ld] = x[j];
        }
    }
#pragma unroll
    for (int t = 0; t < NB; ++t) wrow[t] = w[t];
}

unsigned blocks_of(int64_t items, int per_block) { return (unsigned)std::max<int64_t>(1, (items + per_block - 1) / per_block); }

#define UPDOWN_NB(NBV, CALL)      \
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
static_assert(kUpdownBlock == 8, "UPDOWN_NB lists the instantiations 1 .. kUpdownBlock");

int ensure_device(parsy_plan* pl) {
    if (updown_ensure_host(pl) != 0) return -1;
    UpdownState& U = *pl->updown;
    PARSY_HIP(hipSetDevice(pl->device));
    if (U.on_device) return 0;
    DevicePool pool(&U.meter);
    const int64_t wlen = std::max<int64_t>((int64_t)pl->S.n * kUpdownBlock, 1);
    double* d_w = pool.alloc<double>(wlen);
    double* d_coef = pool.alloc<double>((int64_t)kUpdownTile * kUpdownBlock * kUpdownCoef);
    int32_t* d_status = pool.alloc<int32_t>(1);
    if (pool.error() != hipSuccess) return pool_failed(pool);
    PARSY_HIP(hipMemset(d_w, 0, (size_t)wlen * sizeof(double)));
    PARSY_HIP(hipMemset(d_status, 0x7f, sizeof(int32_t)));
    PARSY_HIP(hipDeviceSynchronize());   // (once per plan: the caller's stream may not wait for the null stream)
    U.fixed = std::move(pool);
    U.d_w = d_w, U.d_coef = d_coef, U.d_status = d_status;
    U.on_device = true;
    return 0;
}

// The rotation pass over a path for the nb <= kUpdownBlock columns that stand in the workspace, then the clearing of
// the workspace rows of the path's row lists (d_segs: k_updown_clear_w's segments, rows_total: their last prefix sum).
void enqueue_walk(parsy_plan* pl, double* d_L, int sign, int nb, const std::vector<UpdownNode>& path, const int64_t* d_segs,
                  int64_t rows_total, hipStream_t stream, int& launches, int64_t& entries) {
    const Schedule& S = pl->S;
    UpdownState& U = *pl->updown;
    const double sigma = (double)sign;
    const dim3 threads(kUThreads);
    for (const UpdownNode& N : path) {
        const SnDesc& D = S.sn[(size_t)N.sn];
        const int first = N.first_col - D.c0;
        for (int cb = first / kUpdownTile * kUpdownTile; cb < D.w; cb += kUpdownTile) {
            const int nc = std::min(kUpdownTile, D.w - cb);
            const int j0 = std::max(first - cb, 0);
            hipLaunchKernelGGL(k_updown_diag, dim3(1), threads, 0, stream, d_L, D.px, D.r, cb, nc, j0, D.c0 + cb, sigma,
                               U.d_w, U.d_coef, U.d_status);
            ++launches;
            const int row0 = cb + nc;
            if (row0 < D.r) {
#define UPDOWN_ROWS(NN)                                                                                                 \
    hipLaunchKernelGGL(k_updown_rows<NN>, dim3(blocks_of(D.r - row0, kUThreads)), threads, 0, stream, d_L, D.px, D.r, cb, \
                       nc, j0, row0, pl->dp.rows + D.pi, U.d_coef, U.d_w)
                UPDOWN_NB(nb, UPDOWN_ROWS)
#undef UPDOWN_ROWS
                ++launches;
            }
            for (int j = cb + j0; j < cb + nc; ++j) entries += D.r - j;
        }
    }
    hipLaunchKernelGGL(k_updown_clear_w, dim3(blocks_of(rows_total, kUThreads)), threads, 0, stream, d_segs, (int)path.size(),
                       pl->dp.rows, U.d_w);
    ++launches;
}

}  // namespace

int updown_ensure_host(parsy_plan* pl) {
    if (!pl->updown) pl->updown = std::make_unique<UpdownState>(&pl->meter);
    return 0;
}

int updown_check_args(const parsy_plan* pl, const char* who, const void* lValues, int sign, int k, const void* wp,
                      const void* wi, const void* wx) {
    const std::string w(who);
    if (!pl) return set_last_error(w + ": null argument"), -1;
    if (k < 0) return set_last_error(w + ": need k >= 0"), -1;
    if (sign != 1 && sign != -1) return set_last_error(w + ": sign must be +1 (update) or -1 (downdate)"), -1;
    if (k > 0 && (!lValues || !wp)) return set_last_error(w + ": null argument"), -1;
    const int nnz = k > 0 ? static_cast<const int*>(wp)[k] - static_cast<const int*>(wp)[0] : 0;
    if (nnz > 0 && (!wi || !wx)) return set_last_error(w + ": null argument"), -1;
    return 0;
}

int plan_factor_updown(parsy_plan* pl, double* d_L, int sign, int k, const int* wp, const int* wi, const double* d_wx,
                       void* stream_) {
    const char* who = "parsy_factor_updown_device";
    hipStream_t stream = (hipStream_t)stream_;
    if (updown_check_args(pl, who, d_L, sign, k, wp, wi, d_wx) != 0) return -1;
    const Schedule& S = pl->S;
    UpdownW Wc;
    if (updown_prepare(S, pl->perm, who, k, wp, wi, Wc) != 0) return -1;
    if (pl->sn_mask_set || pl->piece_mask_set)
        return set_last_error(std::string(who) + ": plan is restricted by parsy_plan_set_active / _set_active_pieces"), -1;
    if (check_plan(pl, who, kNeedsDevice) != 0) return -1;
    if (updown_ensure_host(pl) != 0) return -1;
    UpdownState& U = *pl->updown;
    std::vector<UpdownNode> path;
    updown_path(S, Wc, 0, k, path);
    U.path_supernodes = (int)path.size();
    U.block_columns = updown_block_columns(S, path);
    U.last_launches = 0, U.last_k = k, U.last_sign = sign, U.entries_touched = 0;
    if (path.empty()) return 0;   // k == 0 or every column empty: nothing to do
    if (ensure_device(pl) != 0) return -1;

    // The blocks of columns of W: their entries (rows | workspace columns | positions in the caller's values) and the
    // row lists of their paths go up in one piece each, before the first launch.
    struct Block { int t0, nb, e0, nnz; int64_t seg0; std::vector<UpdownNode> path; };
    std::vector<Block> blocks;
    const int nnz_all = (int)Wc.row.size();
    std::vector<int32_t> pat((size_t)nnz_all * 3);
    std::vector<int64_t> segs;
    for (int t0 = 0; t0 < k; t0 += kUpdownBlock) {
        Block B;
        B.t0 = t0, B.nb = std::min(kUpdownBlock, k - t0);
        B.e0 = Wc.ptr[(size_t)t0], B.nnz = Wc.ptr[(size_t)(t0 + B.nb)] - B.e0;
        if (B.nnz == 0) continue;
        for (int t = t0; t < t0 + B.nb; ++t)
            for (int e = Wc.ptr[(size_t)t]; e < Wc.ptr[(size_t)t + 1]; ++e) {
                pat[(size_t)e] = Wc.row[(size_t)e];
                pat[(size_t)nnz_all + e] = t - t0;
                pat[(size_t)2 * nnz_all + e] = Wc.src[(size_t)e];
            }
        updown_path(S, Wc, t0, t0 + B.nb, B.path);
        B.seg0 = (int64_t)segs.size();
        int64_t run = 0;
        for (const UpdownNode& N : B.path) segs.push_back(run), run += S.sn[(size_t)N.sn].r;
        segs.push_back(run);
        for (const UpdownNode& N : B.path) segs.push_back(S.sn[(size_t)N.sn].pi);
        blocks.push_back(std::move(B));
    }
    PARSY_HIP(U.pattern.grow((int64_t)pat.size()));
    PARSY_HIP(U.segs.grow((int64_t)segs.size()));
    PARSY_HIP(hipMemcpyAsync(U.pattern.data(), pat.data(), pat.size() * sizeof(int32_t), hipMemcpyHostToDevice, stream));
    PARSY_HIP(hipMemcpyAsync(U.segs.data(), segs.data(), segs.size() * sizeof(int64_t), hipMemcpyHostToDevice, stream));
    PARSY_HIP(hipStreamSynchronize(stream));   // (the host arrays end with this call)
    PARSY_HIP(hipMemsetAsync(U.d_status, 0x7f, sizeof(int32_t), stream));
    U.used = true;

    const dim3 threads(kUThreads);
    const int32_t* const d_pat = U.pattern.data();
    for (const Block& B : blocks) {
        hipLaunchKernelGGL(k_updown_scatter_w, dim3(blocks_of(B.nnz, kUThreads)), threads, 0, stream, d_pat + B.e0,
                           d_pat + nnz_all + B.e0, d_pat + 2 * (int64_t)nnz_all + B.e0, B.nnz, d_wx, U.d_w);
        ++U.last_launches;
        const int nseg = (int)B.path.size();
        enqueue_walk(pl, d_L, sign, B.nb, B.path, U.segs.data() + B.seg0, segs[(size_t)(B.seg0 + nseg)], stream,
                     U.last_launches, U.entries_touched);
        PARSY_HIP(hipGetLastError());
    }
    return 0;
}

int plan_updown_walk_begin(parsy_plan* pl, int first_col, UpdownWalk& Wk, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    Wk = UpdownWalk();
    if (first_col < 0) return 0;
    if (ensure_device(pl) != 0) return -1;
    UpdownState& U = *pl->updown;
    const Schedule& S = pl->S;
    UpdownW one;
    one.k = 1, one.ptr = {0, 1}, one.row = {first_col}, one.src = {0};
    updown_path(S, one, 0, 1, Wk.path);
    std::vector<int64_t>& segs = U.walk_segs;
    segs.clear();
    int64_t run = 0;
    for (const UpdownNode& N : Wk.path) segs.push_back(run), run += S.sn[(size_t)N.sn].r;
    segs.push_back(run);
    for (const UpdownNode& N : Wk.path) segs.push_back(S.sn[(size_t)N.sn].pi);
    Wk.rows_total = run;
    PARSY_HIP(U.segs.grow((int64_t)segs.size()));
    PARSY_HIP(hipMemcpyAsync(U.segs.data(), segs.data(), segs.size() * sizeof(int64_t), hipMemcpyHostToDevice, stream));
    return 0;
}

int plan_updown_status_reset(parsy_plan* pl, void* stream) {
    if (ensure_device(pl) != 0) return -1;
    PARSY_HIP(hipMemsetAsync(pl->updown->d_status, 0x7f, sizeof(int32_t), (hipStream_t)stream));
    pl->updown->used = true;
    return 0;
}

int plan_updown_walk_run(parsy_plan* pl, double* d_L, int sign, UpdownWalk& Wk, void* stream) {
    if (Wk.path.empty()) return 0;
    UpdownState& U = *pl->updown;
    enqueue_walk(pl, d_L, sign, 1, Wk.path, U.segs.data(), Wk.rows_total, (hipStream_t)stream, Wk.launches, Wk.entries);
    PARSY_HIP(hipGetLastError());
    return 0;
}

double* plan_updown_workspace(parsy_plan* pl) { return pl->updown ? pl->updown->d_w : nullptr; }
int32_t* plan_updown_status_word(parsy_plan* pl) { return pl->updown ? pl->updown->d_status : nullptr; }

int plan_updown_status(parsy_plan* pl) {
    if (!pl || pl->device < 0) return -1;
    if (!pl->updown || !pl->updown->used) return 0;
    int v = 0;
    if (hipSetDevice(pl->device) != hipSuccess ||
        hipMemcpy(&v, pl->updown->d_status, sizeof(int), hipMemcpyDeviceToHost) != hipSuccess)
        return -1;
    return v >= kUNoFailure ? 0 : v;
}

}  // namespace parsy
