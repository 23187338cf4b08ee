// Solves with sparse right-hand sides for selected rows of the result, on the device (reach.hpp).  Every launch is
// ordered against the others by the stream alone: no flags, no tickets, no waits between workgroups, no floating-point
// atomics; every output element has one writer per launch and one summation order, fixed by the pattern.  A supernode's
// arithmetic does not depend on which other supernodes are in the set, a column's not on how many are computed with it.
//
// The vectors of a call live in the compact numbering of the handle, per block of kSparseBlock right-hand sides with
// the columns of a row contiguous: Y (b, then y, then x), T (one row per row-list entry of F: what the panels subtract
// from the rows below them), P (the partials of the backward panels).  The blocks of right-hand sides are the launches'
// second grid dimension; they share nothing but the read of L.  NB (1, 2, 4 or 8) is the number of columns of a block
// a lane carries; columns past the call's are zero and stay zero.
//
//   k_sparse_load          Y[row of the entry, its column] = bx[entry]
//   k_sparse_fwd_tri<NB>   one workgroup per piece of a forward step.  A supernode's first piece gathers
//                          y_j = b_j - sum of column j's occurrences in T (ascending position) for ALL its columns; a later
//                          piece takes y_j - T[its own row j].  Then the solve with the piece's triangle in block columns
//                          of 64, as k_rowadd_solve does it: the tile's lower triangle in LDS, one wave runs the 64 steps,
//                          all four waves apply the block column to the rest of the piece (a lane per row)
//   k_sparse_fwd_panel<NB> the panel rows below the piece -- the supernode's own later columns among them -- a lane per
//                          row, 256 rows a workgroup: y of the piece in LDS (read as broadcasts), one fma chain per (row,
//                          right-hand side) in ascending column order that goes on from what the pieces before left in T.
//                          For a fixed column consecutive lanes read consecutive doubles of the panel
//   k_sparse_bwd_panel<NB> L' (rows below the piece) times x at those rows, read through the compact map: a wave per task
//                          of at most 4 columns over a segment of 1024 rows, lane l the rows i = l (mod 64) in ascending
//                          order, a butterfly, one partial per (segment, column)
//   k_sparse_bwd_tri<NB>   x_j = y_j - (the column's partials, ascending), then the solve with the transposed triangle,
//                          block columns from the last to the first (the tile transposed in LDS, rows padded to 65)
//   k_sparse_gather        the selected rows into the caller's nx x nrhs block, in the order of Xset
//   k_sparse_clear         zero into exactly what the call wrote
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

constexpr int kSThreads = 256;
constexpr int kSWaves = kSThreads / 64;
constexpr int kTileLd = kSparseTile + 1;   // k_sparse_bwd_tri: the transposed tile's leading dimension
static_assert(kSparseRows == kSThreads, "k_sparse_fwd_panel: a lane per row");
static_assert(kSparsePiece <= kSThreads, "a column of the piece's y per thread");
static_assert(kSparseTile == 64, "the triangle solves: one wave, a lane per row of the tile");
static_assert(kSparseSeg % 64 == 0, "k_sparse_bwd_panel: a segment in rounds of 64 rows");

__global__ __launch_bounds__(kSThreads) void k_sparse_load(const double* __restrict__ bx, const int32_t* __restrict__ bcol,
                                                           const int32_t* __restrict__ bcomp,
                                                           const uint8_t* __restrict__ colmask, int need, int64_t nnz,
                                                           int ncomp, double* __restrict__ Y) {
    const int64_t t = (int64_t)blockIdx.x * kSThreads + threadIdx.x;
    if (t >= nnz) return;
    const int c = bcomp[t], q = bcol[t];
    if (!(colmask[c] & need)) return;   // (the backward-only solve reads B on the columns of K alone)
    Y[((int64_t)(q / kSparseBlock) * ncomp + c) * kSparseBlock + q % kSparseBlock] = bx[t];
}

template <int NB>
__global__ __launch_bounds__(kSThreads) void k_sparse_fwd_tri(const double* __restrict__ L, const SparsePiece* __restrict__ pieces,
                                                              const int64_t* __restrict__ gptr, const int64_t* __restrict__ gpos,
                                                              int ncomp, int64_t nent, double* __restrict__ Y,
                                                              const double* __restrict__ T) {
    __shared__ double tile[kSparseTile * kSparseTile];   // column-major lower triangle of the diagonal tile
    __shared__ double ys[kSparsePiece * NB];             // y of the piece
    const SparsePiece D = pieces[blockIdx.x];
    const int tid = threadIdx.x, nc = D.nc;
    const int64_t r = D.r;
    double* __restrict__ Yb = Y + ((int64_t)blockIdx.y * ncomp + D.y0) * kSparseBlock;
    const double* __restrict__ Tb = T + (int64_t)blockIdx.y * nent * kSparseBlock;
    if (D.c0 == 0) {
        // the gather, for every column of the supernode: the later pieces find theirs in Y
        for (int j = tid; j < D.w; j += kSThreads) {
            double acc[NB];
#pragma unroll
            for (int q = 0; q < NB; ++q) acc[q] = Yb[(int64_t)j * kSparseBlock + q];
            for (int64_t e = gptr[D.y0 + j], e1 = gptr[D.y0 + j + 1]; e < e1; ++e) {
                const double* __restrict__ t = Tb + gpos[e] * kSparseBlock;
#pragma unroll
                for (int q = 0; q < NB; ++q) acc[q] -= t[q];
            }
#pragma unroll
            for (int q = 0; q < NB; ++q) {
                if (j < nc) ys[j * NB + q] = acc[q];
                else Yb[(int64_t)j * kSparseBlock + q] = acc[q];
            }
        }
    } else {
        const double* __restrict__ own = Tb + (D.e0 + D.c0) * kSparseBlock;   // what the pieces before it left for its rows
        for (int j = tid; j < nc; j += kSThreads) {
#pragma unroll
            for (int q = 0; q < NB; ++q) ys[j * NB + q] = Yb[(int64_t)j * kSparseBlock + q] - own[(int64_t)j * kSparseBlock + q];
        }
    }
    __syncthreads();
    const double* __restrict__ panel = L + D.px + (int64_t)D.c0 * r + D.c0;   // the piece's first diagonal entry
    for (int cb = 0; cb < nc; cb += kSparseTile) {
        const int nct = min(kSparseTile, nc - cb);
        const double* __restrict__ g = panel + (int64_t)cb * r + cb;
        for (int e = tid; e < kSparseTile * kSparseTile; e += kSThreads) {
            const int j = e >> 6, i = e & 63;
            tile[e] = (i < nct && j < nct && i >= j) ? g[(int64_t)j * r + i] : 0.0;   // (never the strict upper triangle)
        }
        __syncthreads();
        if (tid < 64) {
            const int i = tid;
            double x[NB];
#pragma unroll
            for (int q = 0; q < NB; ++q) x[q] = i < nct ? ys[(cb + i) * NB + q] : 0.0;
            for (int j = 0; j < nct; ++j) {
                const double d = tile[j * kSparseTile + j], lij = tile[j * kSparseTile + i];
#pragma unroll
                for (int q = 0; q < NB; ++q) {
                    const double xj = __shfl(x[q], j) / d;   // lane j's x is final at step j
                    if (i == j) x[q] = xj;
                    else if (i > j) x[q] = fma(-lij, xj, x[q]);
                }
            }
            if (i < nct) {
#pragma unroll
                for (int q = 0; q < NB; ++q) ys[(cb + i) * NB + q] = x[q];
            }
        }
        __syncthreads();
        for (int i = cb + nct + tid; i < nc; i += kSThreads) {
            const double* __restrict__ row = panel + (int64_t)cb * r + i;
            double acc[NB];
#pragma unroll
            for (int q = 0; q < NB; ++q) acc[q] = ys[i * NB + q];
#pragma unroll 8
            for (int j = 0; j < nct; ++j) {
                const double l = row[(int64_t)j * r];
#pragma unroll
                for (int q = 0; q < NB; ++q) acc[q] = fma(-l, ys[(cb + j) * NB + q], acc[q]);
            }
#pragma unroll
            for (int q = 0; q < NB; ++q) ys[i * NB + q] = acc[q];
        }
        __syncthreads();
    }
    for (int j = tid; j < nc; j += kSThreads) {
#pragma unroll
        for (int q = 0; q < NB; ++q) Yb[(int64_t)j * kSparseBlock + q] = ys[j * NB + q];
    }
}

// work: (piece of `pieces`, first row) per workgroup
template <int NB>
__global__ __launch_bounds__(kSThreads) void k_sparse_fwd_panel(const double* __restrict__ L, const SparsePiece* __restrict__ pieces,
                                                                const int32_t* __restrict__ work, int ncomp, int64_t nent,
                                                                const double* __restrict__ Y, double* __restrict__ T) {
    __shared__ double ys[kSparsePiece * NB];
    const SparsePiece D = pieces[work[2 * blockIdx.x]];
    const int i = work[2 * blockIdx.x + 1] + threadIdx.x;
    const bool on = i < D.r;
    const int64_t r = D.r;
    const double* __restrict__ Yb = Y + ((int64_t)blockIdx.y * ncomp + D.y0) * kSparseBlock;
    double* __restrict__ t = T + ((int64_t)blockIdx.y * nent + D.e0 + (on ? i : D.r - 1)) * kSparseBlock;
    if ((int)threadIdx.x < D.nc) {
#pragma unroll
        for (int q = 0; q < NB; ++q) ys[threadIdx.x * NB + q] = Yb[(int64_t)threadIdx.x * kSparseBlock + q];
    }
    __syncthreads();
    const double* __restrict__ col = L + D.px + (int64_t)D.c0 * r + (on ? i : D.r - 1);   // (lanes past the panel store nothing)
    double acc[NB];
#pragma unroll
    for (int q = 0; q < NB; ++q) acc[q] = on ? t[q] : 0.0;
#pragma unroll 8
    for (int c = 0; c < D.nc; ++c) {
        const double l = col[(int64_t)c * r];
#pragma unroll
        for (int q = 0; q < NB; ++q) acc[q] = fma(l, ys[c * NB + q], acc[q]);
    }
    if (on) {
#pragma unroll
        for (int q = 0; q < NB; ++q) t[q] = acc[q];
    }
}

// work: (piece of `pieces`, segment * column groups + column group) per wave
template <int NB>
__global__ __launch_bounds__(kSThreads) void k_sparse_bwd_panel(const double* __restrict__ L, const SparsePiece* __restrict__ pieces,
                                                                const int32_t* __restrict__ work, int nwork,
                                                                const int32_t* __restrict__ cmap, int ncomp, int64_t npart,
                                                                const double* __restrict__ Y, double* __restrict__ P) {
    const int lane = threadIdx.x & 63;
    const int task = blockIdx.x * kSWaves + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (task >= nwork) return;
    const SparsePiece D = pieces[work[2 * task]];
    const int code = work[2 * task + 1];
    const int groups = (D.nc + kSparseCols - 1) / kSparseCols;
    const int seg = code / groups, cf = (code % groups) * kSparseCols;
    const int ncol = min(kSparseCols, D.nc - cf);
    const int i0 = D.c0 + D.nc + seg * kSparseSeg, i1 = min(D.r, i0 + kSparseSeg);
    const int64_t r = D.r;
    const double* __restrict__ g = L + D.px + (int64_t)(D.c0 + cf) * r;
    const double* __restrict__ Yb = Y + (int64_t)blockIdx.y * ncomp * kSparseBlock;
    const int32_t* __restrict__ rows = cmap + D.e0;
    double s[kSparseCols][NB];
#pragma unroll
    for (int u = 0; u < kSparseCols; ++u)
#pragma unroll
        for (int q = 0; q < NB; ++q) s[u][q] = 0.0;
    for (int b = i0; b < i1; b += 64) {
        const int i = b + lane;
        const bool on = i < i1;
        const int ii = on ? i : i1 - 1;
        const double* __restrict__ xr = Yb + (int64_t)rows[ii] * kSparseBlock;
        double xv[NB];
#pragma unroll
        for (int q = 0; q < NB; ++q) xv[q] = xr[q];
#pragma unroll
        for (int u = 0; u < kSparseCols; ++u) {
            if (u < ncol) {
                const double g0 = on ? g[(int64_t)u * r + ii] : 0.0;
#pragma unroll
                for (int q = 0; q < NB; ++q) s[u][q] = on ? fma(g0, xv[q], s[u][q]) : s[u][q];
            }
        }
    }
    double* __restrict__ Pb = P + ((int64_t)blockIdx.y * npart + D.p0 + (int64_t)seg * D.nc + cf) * kSparseBlock;
#pragma unroll
    for (int u = 0; u < kSparseCols; ++u) {
        if (u < ncol) {
#pragma unroll
            for (int q = 0; q < NB; ++q) {
                double v = s[u][q];
#pragma unroll
                for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o);
                if (lane == 0) Pb[u * kSparseBlock + q] = v;
            }
        }
    }
}

template <int NB>
__global__ __launch_bounds__(kSThreads) void k_sparse_bwd_tri(const double* __restrict__ L, const SparsePiece* __restrict__ pieces,
                                                              int ncomp, int64_t npart, double* __restrict__ Y,
                                                              const double* __restrict__ P) {
    __shared__ double tile[kSparseTile * kTileLd];   // tile[row * 65 + column]: lane i reads L[j, i] of row j conflict-free
    __shared__ double xs[kSparsePiece * NB];
    const SparsePiece D = pieces[blockIdx.x];
    const int tid = threadIdx.x, nc = D.nc;
    const int64_t r = D.r;
    double* __restrict__ Yb = Y + ((int64_t)blockIdx.y * ncomp + D.y0) * kSparseBlock;
    const double* __restrict__ Pb = P + ((int64_t)blockIdx.y * npart + D.p0) * kSparseBlock;
    for (int j = tid; j < nc; j += kSThreads) {
        double sum[NB];
#pragma unroll
        for (int q = 0; q < NB; ++q) sum[q] = 0.0;
        for (int sg = 0; sg < D.nseg; ++sg) {
            const double* __restrict__ p = Pb + ((int64_t)sg * nc + j) * kSparseBlock;
#pragma unroll
            for (int q = 0; q < NB; ++q) sum[q] += p[q];
        }
#pragma unroll
        for (int q = 0; q < NB; ++q) xs[j * NB + q] = Yb[(int64_t)j * kSparseBlock + q] - sum[q];
    }
    __syncthreads();
    const double* __restrict__ panel = L + D.px + (int64_t)D.c0 * r + D.c0;
    for (int cb = ((nc - 1) / kSparseTile) * kSparseTile; cb >= 0; cb -= kSparseTile) {
        const int nct = min(kSparseTile, nc - cb);
        const double* __restrict__ g = panel + (int64_t)cb * r + cb;
        for (int e = tid; e < kSparseTile * kSparseTile; e += kSThreads) {
            const int j = e >> 6, i = e & 63;   // (column, row): consecutive threads read consecutive rows of a column
            tile[i * kTileLd + j] = (i < nct && j < nct && i >= j) ? g[(int64_t)j * r + i] : 0.0;
        }
        __syncthreads();
        if (tid < 64) {
            const int i = tid;
            double x[NB];
#pragma unroll
            for (int q = 0; q < NB; ++q) x[q] = i < nct ? xs[(cb + i) * NB + q] : 0.0;
            for (int j = nct - 1; j >= 0; --j) {
                const double d = tile[j * kTileLd + j], lji = tile[j * kTileLd + i];   // L[j, i]: zero for i > j
#pragma unroll
                for (int q = 0; q < NB; ++q) {
                    const double xj = __shfl(x[q], j) / d;   // lane j's x is final at step j
                    if (i == j) x[q] = xj;
                    else if (i < j) x[q] = fma(-lji, xj, x[q]);
                }
            }
            if (i < nct) {
#pragma unroll
                for (int q = 0; q < NB; ++q) xs[(cb + i) * NB + q] = x[q];
            }
        }
        __syncthreads();
        // the block row L[cb .. cb + nct, i]' into the columns before it, a lane per column
        for (int i = tid; i < cb; i += kSThreads) {
            const double* __restrict__ col = panel + (int64_t)i * r + cb;
            double acc[NB];
#pragma unroll
            for (int q = 0; q < NB; ++q) acc[q] = xs[i * NB + q];
#pragma unroll 8
            for (int j = 0; j < nct; ++j) {
                const double l = col[j];
#pragma unroll
                for (int q = 0; q < NB; ++q) acc[q] = fma(-l, xs[(cb + j) * NB + q], acc[q]);
            }
#pragma unroll
            for (int q = 0; q < NB; ++q) xs[i * NB + q] = acc[q];
        }
        __syncthreads();
    }
    for (int j = tid; j < nc; j += kSThreads) {
#pragma unroll
        for (int q = 0; q < NB; ++q) Yb[(int64_t)j * kSparseBlock + q] = xs[j * NB + q];
    }
}

__global__ __launch_bounds__(kSThreads) void k_sparse_gather(const int32_t* __restrict__ xcomp, int nx, int nrhs, int ncomp,
                                                             const double* __restrict__ Y, double* __restrict__ X, int64_t ldx) {
    const int64_t idx = (int64_t)blockIdx.x * kSThreads + threadIdx.x;
    if (idx >= (int64_t)nx * nrhs) return;
    const int k = (int)(idx % nx), q = (int)(idx / nx);
    X[k + q * ldx] = Y[((int64_t)(q / kSparseBlock) * ncomp + xcomp[k]) * kSparseBlock + q % kSparseBlock];
}

// sets: 1 = the call ran the forward pass (the columns and the entries of F), 2 = the backward pass (the columns of K, P)
__global__ __launch_bounds__(kSThreads) void k_sparse_clear(const uint8_t* __restrict__ colmask, const uint8_t* __restrict__ entmask,
                                                            int sets, int ncomp, int64_t nent, int64_t npart, int nblocks,
                                                            double* __restrict__ Y, double* __restrict__ T,
                                                            double* __restrict__ P) {
    const int64_t idx = (int64_t)blockIdx.x * kSThreads + threadIdx.x;
    for (int b = 0; b < nblocks; ++b) {
        if (idx < ncomp && (colmask[idx] & sets)) {
            double* __restrict__ y = Y + ((int64_t)b * ncomp + idx) * kSparseBlock;
#pragma unroll
            for (int q = 0; q < kSparseBlock; ++q) y[q] = 0.0;
        }
        if (idx < nent && (entmask[idx] & sets)) {
            double* __restrict__ t = T + ((int64_t)b * nent + idx) * kSparseBlock;
#pragma unroll
            for (int q = 0; q < kSparseBlock; ++q) t[q] = 0.0;
        }
        if (idx < npart && (sets & 2)) {
            double* __restrict__ p = P + ((int64_t)b * npart + idx) * kSparseBlock;
#pragma unroll
            for (int q = 0; q < kSparseBlock; ++q) p[q] = 0.0;
        }
    }
}

unsigned blocks_of(int64_t items, int per_block) { return (unsigned)std::max<int64_t>(1, (items + per_block - 1) / per_block); }

int ensure_device(parsy_reach* h) {
    ReachState& R = h->dev;
    const ReachIndex& I = h->I;
    PARSY_HIP(hipSetDevice(h->device));
    if (R.on_device) return 0;
    const int64_t nb = (I.nrhs + kSparseBlock - 1) / kSparseBlock;
    const int64_t ylen = std::max<int64_t>(nb * I.ncomp * kSparseBlock, 1), tlen = std::max<int64_t>(nb * I.nent * kSparseBlock, 1),
                  plen = std::max<int64_t>(nb * I.npart * kSparseBlock, 1);
    DevicePool pool(&R.meter);
    ReachState N;
    N.d_fpieces = pool.upload(I.fwd.pieces), N.d_bpieces = pool.upload(I.bwd.pieces);
    N.d_fwork = pool.upload(I.fwd.work), N.d_bwork = pool.upload(I.bwd.work);
    N.d_cmap = pool.upload(I.cmap), N.d_bcol = pool.upload(I.bcol), N.d_bcomp = pool.upload(I.bcomp);
    N.d_xcomp = pool.upload(I.xcomp);
    N.d_gptr = pool.upload(I.gptr), N.d_gpos = pool.upload(I.gpos);
    N.d_colmask = pool.upload(I.colmask), N.d_entmask = pool.upload(I.entmask);
    N.d_y = pool.alloc<double>(ylen), N.d_t = pool.alloc<double>(tlen), N.d_p = pool.alloc<double>(plen);
    if (pool.error() != hipSuccess) return pool_failed(pool);
    PARSY_HIP(hipMemset(N.d_y, 0, (size_t)ylen * sizeof(double)));
    PARSY_HIP(hipMemset(N.d_t, 0, (size_t)tlen * sizeof(double)));
    PARSY_HIP(hipMemset(N.d_p, 0, (size_t)plen * sizeof(double)));
    PARSY_HIP(hipDeviceSynchronize());   // (once per handle: the caller's stream may not wait for the null stream)
    R.fixed = std::move(pool);
    R.d_fpieces = N.d_fpieces, R.d_bpieces = N.d_bpieces, R.d_fwork = N.d_fwork, R.d_bwork = N.d_bwork;
    R.d_cmap = N.d_cmap, R.d_bcol = N.d_bcol, R.d_bcomp = N.d_bcomp, R.d_xcomp = N.d_xcomp;
    R.d_gptr = N.d_gptr, R.d_gpos = N.d_gpos, R.d_colmask = N.d_colmask, R.d_entmask = N.d_entmask;
    R.d_y = N.d_y, R.d_t = N.d_t, R.d_p = N.d_p;
    R.on_device = true;
    return 0;
}

// the passes of one call for blocks of NB columns a lane; returns the kernels enqueued
template <int NB>
int enqueue_passes(const parsy_reach* h, const double* d_L, bool forward, bool backward, hipStream_t stream) {
    const ReachState& R = h->dev;
    const ReachIndex& I = h->I;
    const unsigned nb = (unsigned)((I.nrhs + kSparseBlock - 1) / kSparseBlock);
    const dim3 threads(kSThreads);
    int kernels = 0;
    if (forward) {
        const SparsePass& F = I.fwd;
        for (int t = 0; t < F.steps(); ++t) {
            const int p0 = F.step_first[(size_t)t], np = F.step_first[(size_t)t + 1] - p0;
            hipLaunchKernelGGL(k_sparse_fwd_tri<NB>, dim3((unsigned)np, nb), threads, 0, stream, d_L, R.d_fpieces + p0, R.d_gptr,
                               R.d_gpos, I.ncomp, I.nent, R.d_y, R.d_t);
            ++kernels;
            const int w0 = F.work_first[(size_t)t], nw = F.work_first[(size_t)t + 1] - w0;
            if (nw > 0) {
                hipLaunchKernelGGL(k_sparse_fwd_panel<NB>, dim3((unsigned)nw, nb), threads, 0, stream, d_L, R.d_fpieces,
                                   R.d_fwork + 2 * (int64_t)w0, I.ncomp, I.nent, R.d_y, R.d_t);
                ++kernels;
            }
        }
    }
    if (backward) {
        const SparsePass& K = I.bwd;
        for (int t = K.steps() - 1; t >= 0; --t) {
            const int w0 = K.work_first[(size_t)t], nw = K.work_first[(size_t)t + 1] - w0;
            if (nw > 0) {
                hipLaunchKernelGGL(k_sparse_bwd_panel<NB>, dim3(blocks_of(nw, kSWaves), nb), threads, 0, stream, d_L, R.d_bpieces,
                                   R.d_bwork + 2 * (int64_t)w0, nw, R.d_cmap, I.ncomp, I.npart, R.d_y, R.d_p);
                ++kernels;
            }
            const int p0 = K.step_first[(size_t)t], np = K.step_first[(size_t)t + 1] - p0;
            hipLaunchKernelGGL(k_sparse_bwd_tri<NB>, dim3((unsigned)np, nb), threads, 0, stream, d_L, R.d_bpieces + p0, I.ncomp,
                               I.npart, R.d_y, R.d_p);
            ++kernels;
        }
    }
    return kernels;
}

}  // namespace

int reach_check_args(const parsy_reach* h, const char* who, const void* lValues, const void* bx, int op, const void* x, int ldx) {
    const std::string w(who);
    if (!h || !lValues || !x || (!bx && !h->I.bcol.empty())) return set_last_error(w + ": null argument"), -1;
    if (op != PARSY_SPARSE_A && op != PARSY_SPARSE_GINV && op != PARSY_SPARSE_GINVT)
        return set_last_error(w + ": unknown op " + std::to_string(op)), -1;
    if (ldx < h->I.nx)
        return set_last_error(w + ": need ldx >= nx (ldx = " + std::to_string(ldx) + ", nx = " + std::to_string(h->I.nx) + ")"), -1;
    if (h->plan->sn_mask_set || h->plan->piece_mask_set)
        return set_last_error(w + ": plan is restricted by parsy_plan_set_active / _set_active_pieces"), -1;
    return 0;
}

int reach_solve(parsy_reach* h, const double* d_L, const double* d_bx, int op, double* d_x, int ldx, void* stream_) {
    const char* who = "parsy_solve_sparse_device";
    hipStream_t stream = (hipStream_t)stream_;
    if (reach_check_args(h, who, d_L, d_bx, op, d_x, ldx) != 0) return -1;
    if (h->device < 0) return set_last_error(std::string(who) + ": plan was built without a device (device < 0)"), -1;
    if (ensure_device(h) != 0) return -1;
    ReachState& R = h->dev;
    const ReachIndex& I = h->I;
    const bool forward = op != PARSY_SPARSE_GINVT, backward = op != PARSY_SPARSE_GINV;
    const int sets = (forward ? 1 : 0) | (backward ? 2 : 0);
    const int nblocks = (I.nrhs + kSparseBlock - 1) / kSparseBlock;
    const dim3 threads(kSThreads);
    const int64_t nnz = (int64_t)I.bcol.size();
    hipLaunchKernelGGL(k_sparse_load, dim3(blocks_of(nnz, kSThreads)), threads, 0, stream, d_bx, R.d_bcol, R.d_bcomp, R.d_colmask,
                       forward ? 1 : 2, nnz, I.ncomp, R.d_y);
    int kernels = 1;
    const int lanes = nblocks > 1 ? kSparseBlock : I.nrhs;   // columns a lane carries: the next of 1, 2, 4, 8
    if (lanes <= 1) kernels += enqueue_passes<1>(h, d_L, forward, backward, stream);
    else if (lanes <= 2) kernels += enqueue_passes<2>(h, d_L, forward, backward, stream);
    else if (lanes <= 4) kernels += enqueue_passes<4>(h, d_L, forward, backward, stream);
    else kernels += enqueue_passes<kSparseBlock>(h, d_L, forward, backward, stream);
    hipLaunchKernelGGL(k_sparse_gather, dim3(blocks_of((int64_t)I.nx * I.nrhs, kSThreads)), threads, 0, stream, R.d_xcomp, I.nx,
                       I.nrhs, I.ncomp, R.d_y, d_x, (int64_t)ldx);
    hipLaunchKernelGGL(k_sparse_clear, dim3(blocks_of(std::max<int64_t>({(int64_t)I.ncomp, I.nent, I.npart}), kSThreads)), threads, 0,
                       stream, R.d_colmask, R.d_entmask, sets, I.ncomp, I.nent, I.npart, nblocks, R.d_y, R.d_t, R.d_p);
    kernels += 2;
    PARSY_HIP(hipGetLastError());
    R.last_op = op, R.last_kernels = kernels;
    return 0;
}

}  // namespace parsy
