// HIP kernels of the level-scheduled BCSC forward solve L X = B for gfx950.
//
// Numeric contract (reference triangularSolve/Triangular_BCSC.h:139-157): per
// supernode, dense forward solve of x[cols] with the diagonal block (non-unit
// diagonal, division as triangularSolve/BLAS.h:8), tmp = L21 * x[cols], then
// x[Li[l]] -= tmp[k] with an atomic (the reference uses `omp atomic`, so its
// rounding order is schedule-dependent too).  X is n x nrhs column-major.
// HBM-bound: every stored L value is read once per pass of kRhs right-hand sides.
// The ONE-launch solves of small plans (k_solve_one, k_bsolve_one) live here too: compiled apart from them, k_solve_small
// and k_solve_panel come out with other scalar instructions around block_invert16, which all four reach (DESIGN.md,
// profiles/solve_split_evidence.md).  The backward solve: trsv_bwd_kernels.hip; what the solve sources share:
// trsv_device.hpp.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "launch.hpp"
#include "trsv_device.hpp"

namespace parsy {

static constexpr int kRhs = 8;  // right-hand sides carried per pass over a panel
// Passes over the right-hand sides are independent of each other: up to kPassLanes of them run side by
// side (workgroups of their own), the rest follow in rounds.  A block of 64 right-hand sides then costs about one pass of latency instead of eight.

// Forward solve of the staged block xs[c][q] (c < w <= 64, q < nq) with the lower-triangular
// block Dg (column-major, ld kLdDiag; entries outside w x w must be an identity).  Blocked by
// 16: the four 16x16 diagonal sub-blocks are inverted once (one column per thread, written
// transposed into the unused strict upper triangle of the sub-block), then per sub-block
//   y_b = inv(L_bb) x_b   and   x_rest -= L(rest, b) y_b
// -- 2 barriers per 16 columns instead of 2 per column.  All threads participate; ends
// synchronised.  (triangularSolve/BLAS.h:8 divides by the diagonal; so does the inversion.)
__device__ __forceinline__ void block_solve_apply16(const double* Dg, const double* invd,
                                                    double (*xs)[kRhs], int w, int nq, int tid);

__device__ __forceinline__ void block_invert16(double* Dg, double* invd, int w, int tid);
__device__ __forceinline__ void block_solve_inv16(double* Dg, double* invd, double (*xs)[kRhs], int w,
                                                  int nq, int tid) {
    block_invert16(Dg, invd, w, tid);
    block_solve_apply16(Dg, invd, xs, w, nq, tid);
}
// (the inversions alone: they do not depend on x -- k_solve_one does them before it waits for its x; ends synchronised)
// (round 5: one wave per 16 x 16 sub-block, one entry per lane, by halves -- inv [A 0; B C] = [inv A, 0; -inv(C) B inv(A),
// inv C] --, as chol_kernels.hip's invert_diag_blocks: the form before gave a column to a thread and walked its 16 rows one
// after the other (3.7 us).  Scratch: a 16 x 16 block of Dg above the block diagonal -- zeros that nothing reads.  Needs the
// whole workgroup of kThreads = 256: wave b = sub-block b.)
__device__ __forceinline__ void block_invert16(double* Dg, double* invd, int w, int tid) {
    if (tid < kTile) invd[tid] = 1.0 / Dg[tid * kLdDiag + tid];
    __syncthreads();
    const int lane = tid & 63;
    const int b = __builtin_amdgcn_readfirstlane(tid >> 6);
    if (16 * b < w) {
        double* __restrict__ B0 = Dg + (16 * b) * kLdDiag + 16 * b;      // L[i][c] = B0[c * ld + i]; W[r][c] (r > c) -> B0[r * ld + c]
        const double* __restrict__ dv = invd + 16 * b;
        double* __restrict__ Sb = Dg + (16 * (b < 3 ? b + 1 : 3)) * kLdDiag + (b < 3 ? 0 : 16);
        auto SC = [&](int e) -> double& { return Sb[(e >> 4) * kLdDiag + (e & 15)]; };
        {   // 4 x 4 diagonal blocks: lane = (d, i', k'): column k' of inv(L_dd) by substitution, entry i'
            const int d4 = 4 * (lane >> 4), ip = (lane >> 2) & 3, kp = lane & 3;
            const double* __restrict__ T = B0 + d4 * kLdDiag + d4;
            const double d0 = dv[d4], d1 = dv[d4 + 1], d2 = dv[d4 + 2], d3 = dv[d4 + 3];
            const double t10 = T[1], t20 = T[2], t30 = T[3], t21 = T[kLdDiag + 2], t31 = T[kLdDiag + 3], t32 = T[2 * kLdDiag + 3];
            const double y0 = kp == 0 ? d0 : 0.0;
            const double y1 = kp == 1 ? d1 : -d1 * (t10 * y0);
            const double y2 = kp == 2 ? d2 : -d2 * fma(t21, y1, t20 * y0);
            const double y3 = kp == 3 ? d3 : -d3 * fma(t32, y2, fma(t31, y1, t30 * y0));
            const double y = ip == 1 ? y1 : ip == 2 ? y2 : y3;
            if (ip > kp) B0[(d4 + ip) * kLdDiag + d4 + kp] = y;
        }
        __builtin_amdgcn_wave_barrier();
        {   // the 4 x 4 blocks below the diagonal of the two 8 x 8 blocks: lanes 0..31 = (e, i, j)
            const int e8 = 8 * ((lane >> 4) & 1), i = (lane >> 2) & 3, j = lane & 3;
            double lr[4], wa[4];
#pragma unroll
            for (int m = 0; m < 4; ++m) {
                lr[m] = B0[(e8 + m) * kLdDiag + e8 + 4 + i];
                wa[m] = B0[(e8 + m) * kLdDiag + e8 + j];
            }
            const double dj = dv[e8 + j], di = dv[e8 + 4 + i];
            double t = 0.0;
#pragma unroll
            for (int m = 0; m < 4; ++m) t = fma(lr[m], m > j ? wa[m] : (m == j ? dj : 0.0), t);
            if (lane < 32) SC(lane) = t;
            __builtin_amdgcn_wave_barrier();
            double wc[4], tt[4];
#pragma unroll
            for (int m = 0; m < 4; ++m) {
                wc[m] = B0[(e8 + 4 + i) * kLdDiag + e8 + 4 + m];
                tt[m] = SC((lane & 16) + 4 * m + j);
            }
            double wv = 0.0;
#pragma unroll
            for (int m = 0; m < 4; ++m) wv = fma(i > m ? wc[m] : (i == m ? di : 0.0), tt[m], wv);
            if (lane < 32) B0[(e8 + 4 + i) * kLdDiag + e8 + j] = -wv;
        }
        __builtin_amdgcn_wave_barrier();
        {   // the 8 x 8 block below the diagonal: lane = (i, j)
            const int i = lane >> 3, j = lane & 7;
            double lr[8], wa[8];
#pragma unroll
            for (int m = 0; m < 8; ++m) {
                lr[m] = B0[m * kLdDiag + 8 + i];
                wa[m] = B0[m * kLdDiag + j];
            }
            const double dj = dv[j], di = dv[8 + i];
            double t = 0.0;
#pragma unroll
            for (int m = 0; m < 8; ++m) t = fma(lr[m], m > j ? wa[m] : (m == j ? dj : 0.0), t);
            SC(lane) = t;
            __builtin_amdgcn_wave_barrier();
            double wc[8], tt[8];
#pragma unroll
            for (int m = 0; m < 8; ++m) {
                wc[m] = B0[(8 + i) * kLdDiag + 8 + m];
                tt[m] = SC(8 * m + j);
            }
            double wv = 0.0;
#pragma unroll
            for (int m = 0; m < 8; ++m) wv = fma(i > m ? wc[m] : (i == m ? di : 0.0), tt[m], wv);
            B0[(8 + i) * kLdDiag + j] = -wv;
        }
    }
    __syncthreads();
}

// The substitution itself, given the inverted sub-blocks (re-used for every pass of
// right-hand sides over the same diagonal block).
__device__ __forceinline__ void block_solve_apply16(const double* Dg, const double* invd,
                                                    double (*xs)[kRhs], int w, int nq, int tid) {
    for (int b16 = 0; b16 < w; b16 += 16) {
        // y = inv(L_bb) x_b : thread (i, q), i < 16
        double yv = 0.0;
        const int i = tid & 15, q = tid >> 4;
        const bool act = q < nq;
        if (act) {
#pragma unroll
            for (int k = 0; k < 16; ++k) {
                double lv = 0.0;
                if (k < i) lv = Dg[(b16 + i) * kLdDiag + b16 + k];  // inv(L_bb)[i][k], stored transposed
                else if (k == i) lv = invd[b16 + i];
                yv = fma(lv, xs[b16 + k][q], yv);
            }
        }
        __syncthreads();
        if (act) xs[b16 + i][q] = yv;
        __syncthreads();
        // rows below the sub-block: x[r][q] -= sum_k L[r][b16+k] y[k][q]
        const int rem = w - b16 - 16;
        for (int e = tid; e < rem * nq; e += kThreads) {
            const int qq = e / rem, rr = b16 + 16 + (e - qq * rem);
            double acc = xs[rr][qq];
#pragma unroll
            for (int k = 0; k < 16; ++k) acc = fma(-Dg[(b16 + k) * kLdDiag + rr], xs[b16 + k][qq], acc);
            xs[rr][qq] = acc;
        }
        __syncthreads();
    }
}

// An entry of x that earlier supernodes of the same launch may have updated with atomics (subtree launches: the
// same workgroup, ordered by a fence + barrier): read at the L2, where the atomics were performed.
__device__ __forceinline__ double ld_x(const double* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// SOLVE_SMALL: one workgroup per supernode of width <= 64 -- or, ranges != null (subtree launch), per subtree
// of such supernodes: list[ranges[2b] .. ranges[2b+1]) one after the other (index order: descendants first;
// what they subtract from the x of the later ones is complete when those start).
__global__ __launch_bounds__(kThreads) void k_solve_small(const SnDesc* __restrict__ sn,
                                                          const int32_t* __restrict__ list,
                                                          const int32_t* __restrict__ ranges,
                                                          const int32_t* __restrict__ rows,
                                                          const double* __restrict__ L,
                                                          double* __restrict__ x, int nrhs, int ldx) {
    __shared__ double Dg[kTile * kLdDiag];
    __shared__ double invd[kTile];
    __shared__ double xs[kTile][kRhs];
    const int tid = threadIdx.x;
    const int q_begin = ranges ? ranges[2 * blockIdx.x] : (int)blockIdx.x;
    const int q_end = ranges ? ranges[2 * blockIdx.x + 1] : q_begin + 1;
  for (int qsn = q_begin; qsn < q_end; ++qsn) {
    if (qsn > q_begin) {
        // this thread's atomics are performed (they execute at the device's coherence point: waiting for their
        // completion is all it takes -- no L2 write-back as an agent-scope fence would do) ...
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();   // ... and so are everybody's; Dg / xs are free again
    }
    const SnDesc D = sn[list[qsn]];
    const int r = D.r, w = D.w;
    const double* __restrict__ G = L + D.px;
    const int32_t* __restrict__ ri = rows + D.pi;

    const int wpad = (w + 15) & ~15;
    for (int e = tid; e < wpad * wpad; e += kThreads) {
        const int c = e / wpad, i = e - c * wpad;
        double v = (i == c) ? 1.0 : 0.0;
        if (i >= c && i < w && c < w) v = G[(int64_t)c * r + i];
        Dg[c * kLdDiag + i] = v;
    }
    bool first = true;
    for (int q0 = blockIdx.y * kRhs; q0 < nrhs; q0 += gridDim.y * kRhs) {
        const int nq = min(kRhs, nrhs - q0);
        __syncthreads();
        for (int e = tid; e < wpad * nq; e += kThreads) {
            const int q = e / wpad, c = e - q * wpad;
            xs[c][q] = (c < w) ? ld_x(&x[(int64_t)(q0 + q) * ldx + D.c0 + c]) : 0.0;
        }
        __syncthreads();
        const bool was_first = first;
        first = false;
        if (was_first) block_solve_inv16(Dg, invd, xs, w, nq, tid);
        else block_solve_apply16(Dg, invd, xs, w, nq, tid);
        for (int e = tid; e < w * nq; e += kThreads) {
            const int q = e / w, c = e - q * w;
            x[(int64_t)(q0 + q) * ldx + D.c0 + c] = xs[c][q];
        }
        for (int k = w + tid; k < r; k += kThreads) {
            double acc[kRhs];
#pragma unroll
            for (int q = 0; q < kRhs; ++q) acc[q] = 0.0;
            for (int c = 0; c < w; ++c) {
                const double lv = G[(int64_t)c * r + k];
#pragma unroll
                for (int q = 0; q < kRhs; ++q) acc[q] = fma(lv, xs[c][q], acc[q]);
            }
            const int row = ri[k];
#pragma unroll
            for (int q = 0; q < kRhs; ++q)
                if (q < nq) atomicAdd(&x[(int64_t)(q0 + q) * ldx + row], -acc[q]);
        }
    }
  }
}

// SOLVE_SMALL for supernodes of width <= 16 -- most supernodes of a nested-dissection ordering -- : one WAVE per
// supernode (or per subtree of them: ranges != null, as k_solve_small), no LDS and no barrier.  Lane i holds row i
// of the diagonal block; the substitution goes column by column with lane broadcasts (v_readlane: x_c becomes
// wave-uniform); the rows below the block are one row per lane, their first 64 loaded before the substitution
// starts, and are subtracted from x with atomics.  All loads of a supernode are in flight together: its latency
// is one memory round trip instead of the three of the workgroup kernel.
template <int kTinyW>   // width class of the launch (kTinyWidth; the backward kernel also has kTinyWidth2)
__global__ __launch_bounds__(64) void k_solve_tiny(const SnDesc* __restrict__ sn, const int32_t* __restrict__ list,
                                                   const int32_t* __restrict__ ranges,
                                                   const int32_t* __restrict__ rows, const double* __restrict__ L,
                                                   double* __restrict__ x, int nrhs, int ldx) {
    const int lane = threadIdx.x;
    const int q_begin = ranges ? ranges[2 * blockIdx.x] : (int)blockIdx.x;
    const int q_end = ranges ? ranges[2 * blockIdx.x + 1] : q_begin + 1;
    for (int qsn = q_begin; qsn < q_end; ++qsn) {
        // (subtree launch: the atomics of the supernodes before are performed before this one reads x)
        if (qsn > q_begin) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const SnDesc D = sn[list[qsn]];
        const int r = D.r, w = D.w;
        const double* __restrict__ G = L + D.px;
        const int32_t* __restrict__ ri = rows + D.pi;
        // every load is unconditional: lanes / columns past the block read its last row / column (never used)
        const int il = min(lane, w - 1);
        const int kb = min(w + lane, r - 1);   // first chunk of the rows below the block
        double l[kTinyW], lb[kTinyW];
#pragma unroll
        for (int c = 0; c < kTinyW; ++c) {
            const double* __restrict__ col = G + (int64_t)min(c, w - 1) * r;
            l[c] = col[il];
            lb[c] = col[kb];
        }
        const int row_b = ri[kb];
        double diag = 1.0;
#pragma unroll
        for (int c = 0; c < kTinyW; ++c) diag = (lane == c && c < w) ? l[c] : diag;
        const double rdiag = 1.0 / diag;   // (triangularSolve/BLAS.h:8 divides by the diagonal)
        for (int q = blockIdx.y; q < nrhs; q += gridDim.y) {
            double* __restrict__ xq = x + (int64_t)q * ldx;
            double xi = lane < w ? ld_x(&xq[D.c0 + lane]) : 0.0;
            double xc[kTinyW];   // the solved block, wave-uniform
#pragma unroll
            for (int c = 0; c < kTinyW; ++c) {
                xc[c] = 0.0;
                if (c < w) {
                    xc[c] = readlane_f64(xi * rdiag, c);
                    xi = (lane > c) ? fma(-l[c], xc[c], xi) : xi;
                }
            }
            double xfin = 0.0;
#pragma unroll
            for (int c = 0; c < kTinyW; ++c) xfin = (lane == c) ? xc[c] : xfin;
            if (lane < w) xq[D.c0 + lane] = xfin;
            // rows below the block: the prefetched chunk, then the rest
            double acc = 0.0;
#pragma unroll
            for (int c = 0; c < kTinyW; ++c) acc = fma(lb[c], xc[c], acc);
            if (w + lane < r) atomicAdd(&xq[row_b], -acc);
            for (int k = w + 64 + lane; k < r; k += 64) {
                double a2 = 0.0;
#pragma unroll
                for (int c = 0; c < kTinyW; ++c) a2 = fma(G[(int64_t)min(c, w - 1) * r + k], xc[c], a2);
                atomicAdd(&xq[ri[k]], -a2);
            }
        }
    }
}

// SOLVE_SMALL for many right-hand sides (nrhs >= 16): up to 64 of them per pass over the panel, so that L is
// read once per 64 right-hand sides instead of once per 8, and the products run on the matrix cores
// (v_mfma_f64_16x16x4_f64).  Wave q owns right-hand sides 16q..16q+15 of the pass:
//   (A) diagonal solve, blocked by 16 with the inverted 16x16 sub-blocks (as block_solve_inv16), every product
//       an MFMA with both operands in LDS; a wave only touches its own 16 columns of xs: no barrier inside;
//   (B) rows below the diagonal block, 16 at a time, distributed over the waves: x_s (64 x 64) sits in
//       registers as the A operand, the 16 x 64 piece of L comes straight from the panel (16 consecutive rows
//       per k: 128-B segments) as the B operand -- formed as x_s' L21' so that the lanes run along the ROWS --
//       and is subtracted from x with atomics (the reference's `omp atomic`, Triangular_BCSC.h:154).
// The many-right-hand-side kernels (64 per pass over L, matrix cores) take over from the 8-per-pass kernels
//   * for the narrow supernodes (k_solve_small_mrhs) from 6 right-hand sides on,
//   * for the wide supernodes' chain (k_solve_blocks_mrhs) from 2 on
// (parabolic_fem-class input, MI355X, forward solve: 4 right-hand sides 1.02 -> 0.85 ms, 8: 1.41 -> 0.89 ms; Flan-class,
// 8: 18.2 -> 11.6 ms).  PARSY_MRHS_MIN=k sets both thresholds to k (diagnostics, tests).  These and the other gates of the
// solves' variants: SolveGates (solve_route.hpp), read at the start of every solve; what is chosen with them: solve_route.cpp.
static constexpr int kLdXs = kRhsM + 4; // row stride of xs in LDS

template <int WMAX, bool HALVES = false>  // WMAX: widest supernode of the launch, rounded up to 16 / 32 / 64: sizes LDS and loops
__global__ __launch_bounds__(kThreads) void k_solve_small_mrhs(const SnDesc* __restrict__ sn,
                                                               const int32_t* __restrict__ list,
                                                               const int32_t* __restrict__ ranges,
                                                               const int32_t* __restrict__ rows,
                                                               const double* __restrict__ L,
                                                               double* __restrict__ x, int nrhs, int ldx, int ldq) {
    // X is addressed as x[row * sr + q * sq]: right-hand-side-major (the interface: sr = 1, sq = ldx) or, inside a
    // solve with many right-hand sides, row-major with the right-hand sides of a row contiguous (ldq > 0: sr = ldq,
    // sq = 1 -- a supernode's x block and its write-back are then whole 512-byte rows instead of 64 eight-byte pieces
    // per column, and the thread -> (column, right-hand side) maps of the copies follow the contiguous index)
    const bool tr = ldq > 0;
    const int64_t sr = tr ? ldq : 1, sq = tr ? 1 : ldx;
    constexpr int kLd = WMAX + 1;
    __shared__ double Dg[WMAX * kLd];
    __shared__ double invd[WMAX];
    __shared__ double xs[WMAX * kLdXs];   // xs[c * kLdXs + q]
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l15 = lane & 15, kq = lane >> 4;
    const int q_begin = ranges ? ranges[2 * blockIdx.x] : (int)blockIdx.x;   // subtree launch: as k_solve_small
    const int q_end = ranges ? ranges[2 * blockIdx.x + 1] : q_begin + 1;
  for (int qsn = q_begin; qsn < q_end; ++qsn) {
    if (qsn > q_begin) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
    }
    const SnDesc D = sn[list[qsn]];
    const int r = D.r, w = D.w;
    const double* __restrict__ G = L + D.px;
    const int32_t* __restrict__ ri = rows + D.pi;
    const int wpad = (w + 15) & ~15;

    for (int e = tid; e < WMAX * WMAX; e += kThreads) {
        const int c = e / WMAX, i = e - c * WMAX;
        double v = (i == c) ? 1.0 : 0.0;
        if (i >= c && i < w && c < w) v = G[(int64_t)c * r + i];
        Dg[c * kLd + i] = v;
    }
    __syncthreads();
    // inverses of the 16x16 diagonal sub-blocks, stored transposed in the strict upper triangle (as
    // block_solve_inv16): Dg[(b+r) * ld + b + c] = inv(L_bb)[r][c], r > c; reciprocal diagonal in invd
    if (tid < WMAX) invd[tid] = 1.0 / Dg[tid * kLd + tid];
    __syncthreads();
    if (tid < WMAX && (tid & ~15) < w) {
        const int b16 = tid & ~15, c = tid & 15;
        double y[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) y[k] = (k == c) ? invd[b16 + k] : 0.0;
#pragma unroll
        for (int rr = 1; rr < 16; ++rr) {
            double sacc = 0.0;
#pragma unroll
            for (int k = 0; k < rr; ++k) sacc = fma(Dg[(b16 + k) * kLd + b16 + rr], y[k], sacc);
            y[rr] = (rr > c) ? -sacc * invd[b16 + rr] : y[rr];
        }
        __builtin_amdgcn_s_waitcnt(0);
#pragma unroll
        for (int rr = 1; rr < 16; ++rr)
            if (rr > c) Dg[(b16 + rr) * kLd + b16 + c] = y[rr];
    }
    for (int q0 = 0; q0 < nrhs; q0 += kRhsM) {
        const int nq = min(kRhsM, nrhs - q0);
        __syncthreads();  // inverses written / xs of the previous pass consumed
        for (int e = tid; e < WMAX * kRhsM; e += kThreads) {
            const int q = tr ? e % kRhsM : e / WMAX, c = tr ? e / kRhsM : e - q * WMAX;
            xs[c * kLdXs + q] = (c < w && q < nq) ? ld_x(&x[(D.c0 + c) * sr + (q0 + q) * sq]) : 0.0;
        }
        __syncthreads();
        // ---- (A) wave `wave` solves its 16 right-hand sides
        if (16 * wave < nq) {
            const int qc = 16 * wave + l15;  // this lane's right-hand side as B operand / result column
            for (int b16 = 0; b16 < wpad; b16 += 16) {
                // y_b = inv(L_bb) x_b
                double4_t acc = {0, 0, 0, 0};
#pragma unroll
                for (int st = 0; st < 4; ++st) {
                    const int k = 4 * st + kq, i = l15;
                    double av = 0.0;                       // inv(L_bb)[i][k]
                    if (k < i) av = Dg[(b16 + i) * kLd + b16 + k];
                    else if (k == i) av = invd[b16 + i];
                    const double bv = xs[(b16 + k) * kLdXs + qc];
                    acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, acc, 0, 0, 0);
                }
#pragma unroll
                for (int v = 0; v < 4; ++v) xs[(b16 + kq + 4 * v) * kLdXs + qc] = acc[v];
                // the sub-blocks below: x_b2 -= L(b2, b) y_b
                for (int b2 = b16 + 16; b2 < wpad; b2 += 16) {
                    double4_t a2 = {0, 0, 0, 0};
#pragma unroll
                    for (int st = 0; st < 4; ++st) {
                        const int k = 4 * st + kq;
                        const double av = Dg[(b16 + k) * kLd + b2 + l15];   // L[b2 + i][b16 + k]
                        const double bv = xs[(b16 + k) * kLdXs + qc];
                        a2 = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, a2, 0, 0, 0);
                    }
#pragma unroll
                    for (int v = 0; v < 4; ++v) xs[(b2 + kq + 4 * v) * kLdXs + qc] -= a2[v];
                }
            }
        }
        __syncthreads();
        for (int e = tid; e < w * nq; e += kThreads) {
            const int q = tr ? e % nq : e / w, c = tr ? e / nq : e - q * w;
            x[(D.c0 + c) * sr + (q0 + q) * sq] = xs[c * kLdXs + q];
        }
        // ---- (B) rows below the diagonal block
        const int nfrag_n = (nq + 15) >> 4;
        // (HALVES, for launches of many supernodes up to 64 wide: the right-hand sides in two halves of 32, the rows below
        // swept once per half -- with the x operands of all 64 in registers the kernel takes 311 of them and ONE workgroup
        // fits a compute unit: Flan-class, levels 3-5, 64 right-hand sides: 12 500 supernodes in 2.75 ms; in halves 214
        // registers, two workgroups: forward solve 18.3 -> 17.6 ms.  A launch of few supernodes has the units to itself
        // either way and keeps the one sweep: nd24k- / mid3d-class +1.4 / +3 % in halves)
        constexpr int kNh = HALVES ? 2 : 4;   // 16-right-hand-side groups per sweep
        if (r > w)
          for (int n0 = 0; n0 < nfrag_n; n0 += kNh) {
            constexpr int kSt = WMAX / 4;
            double xa[kNh][kSt];  // A operands: xa[n][st] = x_s[c = 4 st + kq][rhs 16 (n0 + n) + l15]
#pragma unroll
            for (int n = 0; n < kNh; ++n)
#pragma unroll
                for (int st = 0; st < kSt; ++st) xa[n][st] = xs[(4 * st + kq) * kLdXs + 16 * (n0 + n) + l15];
            for (int k0 = w + 16 * wave; k0 < r; k0 += 16 * (kThreads / 64)) {
                const int row_l = min(k0 + l15, r - 1);
                double lv[kSt];
#pragma unroll
                for (int st = 0; st < kSt; ++st) {
                    const int c = 4 * st + kq;
                    lv[st] = (c < w) ? G[(int64_t)c * r + row_l] : 0.0;
                }
                if (tr) {
                    // X row-major: the product the other way round -- L21 x_s, lanes along the RIGHT-HAND SIDES, the
                    // register index along the rows -- so that an instruction's atomics are four rows x 128 contiguous
                    // bytes (8 requests of 64 bytes with 8 adds each) instead of 16 rows x 32 bytes (16 requests with
                    // 4 adds each): they execute at the memory side at the rate of those requests
                    int xr[4];
#pragma unroll
                    for (int v = 0; v < 4; ++v) xr[v] = ri[min(k0 + kq + 4 * v, r - 1)];
#pragma unroll
                    for (int n = 0; n < kNh; ++n) {
                        if (n0 + n < nfrag_n) {
                            double4_t acc = {0, 0, 0, 0};
#pragma unroll
                            for (int st = 0; st < kSt; ++st)
                                acc = __builtin_amdgcn_mfma_f64_16x16x4f64(lv[st], xa[n][st], acc, 0, 0, 0);
                            const int q = 16 * (n0 + n) + l15;
#pragma unroll
                            for (int v = 0; v < 4; ++v)
                                if (k0 + kq + 4 * v < r && q < nq) atomicAdd(&x[xr[v] * sr + (q0 + q) * sq], -acc[v]);
                        }
                    }
                    continue;
                }
                const int xrow = ri[row_l];
                const bool rok = k0 + l15 < r;
#pragma unroll
                for (int n = 0; n < kNh; ++n) {
                    if (n0 + n < nfrag_n) {
                        double4_t acc = {0, 0, 0, 0};
#pragma unroll
                        for (int st = 0; st < kSt; ++st)
                            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(xa[n][st], lv[st], acc, 0, 0, 0);
#pragma unroll
                        for (int v = 0; v < 4; ++v) {
                            const int q = 16 * (n0 + n) + kq + 4 * v;
                            if (rok && q < nq) atomicAdd(&x[xrow * sr + (q0 + q) * sq], -acc[v]);
                        }
                    }
                }
            }
        }
    }
  }
}

// (k: by width, right-hand sides and count -- small_kernel, solve_route.cpp)
void launch_solve_small(const DevicePattern& P, WitnessKernel k, int first, int count, bool subtrees, const double* L,
                        double* x, int nrhs, int ldx, int ldq, hipStream_t stream) {
    if (count <= 0) return;
    // subtree launch: `first` counts (begin, end) pairs of solve_small_ranges, which index the whole list
    const int32_t* list = subtrees ? P.solve_small_list : P.solve_small_list + first;
    const int32_t* ranges = subtrees ? P.solve_small_ranges + 2 * first : nullptr;
    switch (k) {
        case kWSolveTiny:   // one wave per supernode (or per subtree of them)
            launch_witnessed<k_solve_tiny<kTinyWidth>, kWSolveTiny>(dim3(count, std::min(kPassLanes, nrhs)), dim3(64), 0,
                stream, P.sn, list, ranges, P.rows, L, x, nrhs, ldx);
            break;
        case kWSolveSmallMrhs16:
            launch_witnessed<k_solve_small_mrhs<16>, kWSolveSmallMrhs16>(dim3(count), dim3(kThreads), 0, stream, P.sn,
                list, ranges, P.rows, L, x, nrhs, ldx, ldq);
            break;
        case kWSolveSmallMrhs32:
            launch_witnessed<k_solve_small_mrhs<32>, kWSolveSmallMrhs32>(dim3(count), dim3(kThreads), 0, stream, P.sn,
                list, ranges, P.rows, L, x, nrhs, ldx, ldq);
            break;
        case kWSolveSmallMrhs64Halves:
            launch_witnessed<k_solve_small_mrhs<64, true>, kWSolveSmallMrhs64Halves>(dim3(count), dim3(kThreads), 0,
                stream, P.sn, list, ranges, P.rows, L, x, nrhs, ldx, ldq);
            break;
        case kWSolveSmallMrhs64:
            launch_witnessed<k_solve_small_mrhs<64>, kWSolveSmallMrhs64>(dim3(count), dim3(kThreads), 0, stream, P.sn,
                list, ranges, P.rows, L, x, nrhs, ldx, ldq);
            break;
        case kWSolveSmall:
            launch_witnessed<k_solve_small, kWSolveSmall>(dim3(count, std::min(kPassLanes, (nrhs + kRhs - 1) / kRhs)),
                dim3(kThreads), 0, stream, P.sn, list, ranges, P.rows, L, x, nrhs, ldx);
            break;
        default: launch_refused("launch_solve_small", k);
    }
}

// SOLVE_PANEL: block column jb of a wide supernode.  Every workgroup solves the
// 64-wide diagonal block for x_jb in LDS (the designated one parks the result in
// xscratch, so the in-place block stays stable while others read it), then applies
// its 256-row chunk of the block column: x[rows] -= L[rows, jb] * x_jb.
__global__ __launch_bounds__(kThreads) void k_solve_panel(const SnDesc* __restrict__ sn,
                                                          const PanelDesc* __restrict__ pds,
                                                          const int32_t* __restrict__ rows,
                                                          const double* __restrict__ L,
                                                          double* __restrict__ x,
                                                          double* __restrict__ xscratch, int nrhs,
                                                          int ldx) {
    __shared__ double Dg[kTile * kLdDiag];
    __shared__ double invd[kTile];
    __shared__ double xs[kTile][kRhs];
    const int tid = threadIdx.x;
    const PanelDesc pd = pds[blockIdx.x];
    const SnDesc D = sn[pd.sn];
    const int r = D.r, cb = pd.jb * kTile, wbk = min(kTile, D.w - cb);
    const double* __restrict__ G = L + D.px;
    const int32_t* __restrict__ ri = rows + D.pi;

    {
        double dtmp[kTile * kTile / kThreads];
#pragma unroll
        for (int t = 0; t < kTile * kTile / kThreads; ++t) {
            const int e = t * kThreads + tid;
            const int c = e >> 6, i = e & 63;
            double v = (i == c) ? 1.0 : 0.0;
            if (c < wbk && i < wbk && i >= c) v = G[(int64_t)(cb + c) * r + cb + i];
            dtmp[t] = v;
        }
#pragma unroll
        for (int t = 0; t < kTile * kTile / kThreads; ++t) {
            const int e = t * kThreads + tid;
            Dg[(e >> 6) * kLdDiag + (e & 63)] = dtmp[t];
        }
    }
    for (int q0 = 0; q0 < nrhs; q0 += kRhs) {
        const int nq = min(kRhs, nrhs - q0);
        __syncthreads();
        for (int e = tid; e < kTile * nq; e += kThreads) {
            const int q = e >> 6, c = e & 63;
            xs[c][q] = (c < wbk) ? x[(int64_t)(q0 + q) * ldx + D.c0 + cb + c] : 0.0;
        }
        __syncthreads();
        if (q0 == 0) block_solve_inv16(Dg, invd, xs, wbk, nq, tid);
        else block_solve_apply16(Dg, invd, xs, wbk, nq, tid);
        if (pd.row0 < 0) {
            for (int e = tid; e < wbk * nq; e += kThreads) {
                const int q = e / wbk, c = e - q * wbk;
                xscratch[(int64_t)(q0 + q) * ldx + D.c0 + cb + c] = xs[c][q];
            }
            continue;
        }
        const int k = pd.row0 + tid;
        if (k < r) {
            double acc[kRhs];
#pragma unroll
            for (int q = 0; q < kRhs; ++q) acc[q] = 0.0;
            for (int c0 = 0; c0 < wbk; c0 += 16) {  // 16 loads in flight, then their FMAs
                double lv[16];
#pragma unroll
                for (int c = 0; c < 16; ++c) lv[c] = (c0 + c < wbk) ? G[(int64_t)(cb + c0 + c) * r + k] : 0.0;
#pragma unroll
                for (int c = 0; c < 16; ++c)
#pragma unroll
                    for (int q = 0; q < kRhs; ++q) acc[q] = fma(lv[c], xs[c0 + c][q], acc[q]);
            }
            const int row = ri[k];  // rows inside the supernode map to its own columns
#pragma unroll
            for (int q = 0; q < kRhs; ++q)
                if (q < nq) atomicAdd(&x[(int64_t)(q0 + q) * ldx + row], -acc[q]);
        }
    }
}

void launch_solve_panel(const DevicePattern& P, int first, int count, const double* L, double* x,
                        double* xscratch, int nrhs, int ldx, hipStream_t stream) {
    if (count <= 0) return;
    launch_witnessed<k_solve_panel, kWSolvePanel>(dim3(count), dim3(kThreads), 0, stream, P.sn, P.solve_panels + first,
        P.rows, L, x, xscratch, nrhs, ldx);
}

// SOLVE_CHAIN (the block-column chains of a level's wide supernodes in ONE launch) for ONE right-hand side: a dataflow
// of single waves, no workgroup barrier (but one when the workgroup starts) and no flag in memory.
// A workgroup = eight waves = one of the launch's 256-row chunks, taken from the launch's ticket counter (tickets
// follow the row order, so whatever a wave waits for belongs to a workgroup that has started).  Two waves share
// each 64-row block of the chunk (lane = row): wave p of the pair streams the block columns jb = p, p + 2, ... to
// the left of its rows -- takes x_jb (64 values), applies its 64 x 64 piece of L (all 64 loads of a lane's row
// issued BEFORE the wait) -- and keeps its part of the rows' running sum in registers.  A wave has 32 KiB of L in
// flight, so a row block streams at twice that: what bounds a long chain is how fast the rows right below the
// diagonal get through their block columns, not only the hand-off.  When the rows are diagonal block jb of the
// supernode, wave 1 hands its part to wave 0 (LDS), which forms t = x - sum, x_jb = inv(L_jj) t (inverse diagonal
// block staged in LDS when the wave starts: lower triangle, packed) and publishes the 64 values.
// The hand-off is the data itself.  Across workgroups: xscratch is armed with a signalling-NaN pattern (kXArmed)
// before the solve and a value is valid as soon as it differs from it -- every value is one 8-byte agent-scope
// atomic, so the producer neither waits for its stores nor raises a flag, and the consumer's poll (lane c polls
// value c) is the load of the data: one memory round trip per hand-off instead of three.  Inside a workgroup --
// three hand-offs of the critical path out of four, diagonal block to next diagonal block -- x_jb goes through
// LDS (one flag per row block, raised after its 64 values are written).
// Arithmetic never produces the armed pattern (results of operations on NaNs are quiet NaNs); should the data
// hold it, the wait times out and the solve's status word reports it, like any other abandoned hand-off.
// Rows below the supernode's own columns are scattered at the end with atomics, as in the other kernels.
// (launches of at most SolveGates::chain_few_chunks chunks, 384: the top of the tree)

// RB = 64-row blocks per workgroup (8 / RB waves share each of them): 4 where a launch has plenty of chunks, 2
// where it is the top of the tree -- few, very wide supernodes: twice the workgroups (a CU sustains about
// 45 GB/s of this access pattern, so the number of CUs that stream is what bounds a launch of few chunks) and
// twice the waves behind every row block, for half of the diagonal-to-diagonal hand-offs inside a workgroup.
template <int RB>
__global__ __launch_bounds__(kChainThreads, 1) void k_solve_chain_w(const SnDesc* __restrict__ sn,
                                                                    const PanelDesc* __restrict__ pds,
                                                                    const int32_t* __restrict__ rows,
                                                                    const double* __restrict__ L,
                                                                    const double* __restrict__ dinv,
                                                                    double* __restrict__ x, double* __restrict__ xscratch,
                                                                    int* __restrict__ info, int* __restrict__ ticket,
                                                                    int wait_bias) {
    constexpr int G = kChainThreads / 64 / RB;   // waves per row block
    constexpr int kParts = kSolveRows / kTile / RB;   // workgroups per 256-row chunk of the launch
    __shared__ double s_inv[RB][kInvPacked + 1];   // column c of the inverse from row c on, at c*64 - c(c-1)/2
                                                   // (+ one slot for the lanes above it)
    __shared__ double s_x[RB * G][kTile];          // per wave: x_jb taken from memory / t
    __shared__ double s_part[RB][G - 1][kTile];    // the other waves' parts of a diagonal block's sums, for wave 0
    __shared__ double s_pub[RB][kTile];            // x of a diagonal block, for the waves of the blocks after it
    __shared__ int s_parts_in[RB], s_ready[RB];
    __shared__ int s_task;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int rb = wave / G, p = wave % G;   // row block of the workgroup, wave of its group
    if (threadIdx.x == 0) s_task = atomicAdd(ticket, 1);
    if (threadIdx.x < RB) {
        s_ready[threadIdx.x] = 0;
        s_parts_in[threadIdx.x] = 0;
    }
    __syncthreads();   // (the only one: from here on the waves go their own way)
    const PanelDesc pd = pds[s_task / kParts];
    const SnDesc D = sn[pd.sn];
    const int r = D.r, w = D.w;
    const int row0_wg = pd.row0 + (s_task % kParts) * (RB * kTile);
    const int row0 = row0_wg + kTile * rb;
    if (row0 >= r) return;   // (the last chunk of a panel may have fewer than four blocks)
    const int nbc = (w + kTile - 1) / kTile;
    const double* __restrict__ G_ = L + D.px;
    const int k = row0 + lane;          // this lane's panel row
    const bool kv = k < r;
    const bool is_diag = row0 < w;      // the rows hold diagonal block row0 / 64
    const int nblk = is_diag ? row0 / kTile : nbc;   // block columns to the left of the rows
    const int jb_wg = row0_wg / kTile;               // block columns from here on belong to this workgroup's waves
    double* __restrict__ xs = s_x[wave];
    double* __restrict__ inv = s_inv[rb];

    double lv[kTile];
    // every load is unconditional (no branch per column): rows past the panel read its last row (their sum is
    // never used), columns past the supernode read its last column again (their x is zero).  The address walks
    // from column to column by the panel's stride: one vector add per load, nothing else.
    const char* __restrict__ lane_base = reinterpret_cast<const char*>(G_ + min(k, r - 1));
    const int64_t col_stride = (int64_t)r * (int64_t)sizeof(double);
    auto load_block = [&](int jb) {
        const int cb = jb * kTile, last = w - 1 - cb;   // columns 0..last of the block exist (last >= 0)
        const char* pcol = lane_base + (int64_t)cb * col_stride;
#pragma unroll
        for (int c = 0; c < kTile; ++c) {
            lv[c] = *reinterpret_cast<const double*>(pcol);
            pcol += (c < last) ? col_stride : 0;
        }
    };
    auto inv_at = [&](int c) { return lane >= c ? c * kTile - c * (c - 1) / 2 + (lane - c) : kInvPacked; };
    if (is_diag && p == 0) {
        // inverse diagonal block -> LDS (off the critical path: the wave starts well before its turn)
        const double* __restrict__ src = dinv + (int64_t)(D.dslot + row0 / kTile) * (kTile * kTile);
#pragma unroll
        for (int c = 0; c < kTile; ++c)
            lv[c] = *reinterpret_cast<const double*>(reinterpret_cast<const char*>(src + c * kTile) + (unsigned)lane * 8u);
#pragma unroll
        for (int c = 0; c < kTile; ++c) inv[inv_at(c)] = lv[c];
    }
    const double xv = (is_diag && p == 0 && k < w) ? x[D.c0 + k] : 0.0;
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
    for (int jb = p; jb < nblk; jb += G) {
        const int cb = jb * kTile, wbk = min(kTile, w - cb);
        load_block(jb);   // all 64 loads of the lane's row are issued BEFORE the wait for x_jb
        const double* __restrict__ xb = xs;
        if (jb >= jb_wg) {
            // ---- x_jb comes from a wave of this workgroup: LDS
            if (!wait_lds_counter(&s_ready[jb - jb_wg], 1, wait_bias, info)) {
                if (lane == 0) wait_failed(info);   // (the result is wrong and reported; nobody may hang)
                return;
            }
            xb = s_pub[jb - jb_wg];
        } else {
            // ---- x_jb comes from another workgroup: lane c polls value c of the armed buffer
            const long long* __restrict__ src = reinterpret_cast<const long long*>(xscratch + D.c0 + cb) + lane;
            long long bits = 0;
            BoundedWait wait;
            for (;;) {
                bits = lane < wbk ? __hip_atomic_load(src, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0;
                if (__all(bits != kXArmed && wait_bias == 0)) break;
                if (wait.expired(info)) {
                    if (lane == 0) wait_failed(info);
                    return;
                }
                // the rows right below the diagonal wait for the newest x: the critical path; the rows further
                // down are never critical and poll at leisure
                if (is_diag && jb >= nblk - G) __builtin_amdgcn_s_sleep(1);
                else __builtin_amdgcn_s_sleep(8);
            }
            __builtin_amdgcn_wave_barrier();
            xs[lane] = __longlong_as_double(bits);
            __builtin_amdgcn_wave_barrier();   // (one wave: LDS operations complete in order)
        }
#pragma unroll
        for (int c = 0; c < kTile; c += 4) {
            // (16 columns at a time: all 64 LDS reads hoisted above the products would not fit beside lv)
            if ((c & 15) == 0) __builtin_amdgcn_sched_barrier(0);
            a0 = fma(lv[c], xb[c], a0);
            a1 = fma(lv[c + 1], xb[c + 1], a1);
            a2 = fma(lv[c + 2], xb[c + 2], a2);
            a3 = fma(lv[c + 3], xb[c + 3], a3);
        }
        __builtin_amdgcn_sched_barrier(0);
    }
    double acc = (a0 + a1) + (a2 + a3);
    if (is_diag) {
        const int wbk = min(kTile, w - row0);
        if (p != 0) {
            // this wave's part of the sums -> wave 0 of the group
            s_part[rb][p - 1][lane] = acc;
            __builtin_amdgcn_wave_barrier();
            if (lane == 0) __hip_atomic_fetch_add(&s_parts_in[rb], 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
        } else {
            if (!wait_lds_counter(&s_parts_in[rb], G - 1, wait_bias, info)) {
                if (lane == 0) wait_failed(info);
                return;
            }
            double others = 0.0;
#pragma unroll
            for (int q = 0; q < G - 1; ++q) others += s_part[rb][q][lane];
            __builtin_amdgcn_wave_barrier();
            xs[lane] = (lane < wbk) ? xv - (acc + others) : 0.0;
            __builtin_amdgcn_wave_barrier();
            double s0 = 0.0, s1 = 0.0;
#pragma unroll
            for (int c = 0; c < kTile; c += 2) {
                if ((c & 15) == 0) __builtin_amdgcn_sched_barrier(0);
                const double d0 = inv[inv_at(c)], d1 = inv[inv_at(c + 1)];
                s0 = fma(c <= lane ? d0 : 0.0, xs[c], s0);
                s1 = fma(c + 1 <= lane ? d1 : 0.0, xs[c + 1], s1);
            }
            const double xi = (lane < wbk) ? s0 + s1 : 0.0;
            // to the waves of this workgroup through LDS (flag after the data) ...
            s_pub[rb][lane] = xi;
            __builtin_amdgcn_wave_barrier();
            if (lane == 0) __hip_atomic_store(&s_ready[rb], 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
            // ... to everybody else through the armed buffer, and into x
            if (lane < wbk) {
                __hip_atomic_store(&xscratch[D.c0 + row0 + lane], unarmed(xi), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                x[D.c0 + row0 + lane] = xi;
            }
            // a last diagonal block narrower than 64: the other rows of the block lie below the supernode's columns
            // and take this block column too
            if (kv && k >= w)
                for (int c = 0; c < wbk; ++c) acc = fma(G_[(int64_t)(row0 + c) * r + k], s_pub[rb][c], acc);
        }
    }
    // rows below the supernode's columns: each wave of the group scatters its own part of the sums
    if (kv && k >= w) atomicAdd(&x[rows[D.pi + k]], -acc);
}

static constexpr int kSolveRowsM = kSolveRowsMrhs;   // rows of a chunk task of k_solve_blocks_mrhs (schedule.hpp)

// ---------------------------------------------------------------------------
// Forward chain launch for many right-hand sides: the armed buffer of the one-vector kernels -- the data is the flag --
// and two kinds of workgroups, taken by ticket, producers first:
//   * one per BLOCK COLUMN jb of a wide supernode (task row0 < 0), the counterpart of k_bsolve_block_mrhs's chain form:
//       T = B_jb - sum_{k < jb} L(jb, k) X_k,     X_jb = inv(L_jj) T
//     with the COLUMNS of the earlier blocks as the contraction index: wave v takes columns 16 v .. 16 v + 15 of every
//     earlier block k as soon as X_k is there (lane (row, kk) holds L[cb + row][64 k + 16 v + 4 st + kk]: 128-byte
//     segments along the rows; lane (q, kk) holds X_k through the armed buffer), keeps its part of T in 16 accumulator
//     tiles, the four parts are subtracted from the staged B in a fixed order, the product with the inverse diagonal
//     block (DIAG_INVERSE) is on the matrix cores too; only the last k is on the chain's critical path (the loads of
//     L(jb, k) are issued before the wait);
//   * one per 128-ROW CHUNK of the rows below the supernode's own columns (row0 >= w): the running update of its rows
//     over ALL block columns in accumulator layout, each X_jb staged through LDS as soon as it is published, one
//     atomicAdd per (row, right-hand side) at the end (reference Triangular_BCSC.h:139-157: the `omp atomic` scatter).
// 64 right-hand sides per pass over L.  Every wait is bounded and watches the solve's status word.
// ---------------------------------------------------------------------------
#ifdef PARSY_BLKSTAMPS
// (diagnostic build, tools/blk_stamps.py) the block-column tasks of the LAST launch leave, per block column jb: 100-MHz
// clock when X_(jb-1) was seen whole, after the products with it, after the product with the inverse block, after the stores
__device__ unsigned long long g_blkstamp[512 * 8];
#define BLK_STAMP(i) do { if (tid == 0 && plane == 0 && jb < 512) g_blkstamp[jb * 8 + (i)] = wall_clock64(); } while (0)
extern "C" void parsy_debug_blkstamps(unsigned long long* out) {
    (void)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_blkstamp), sizeof(unsigned long long) * 512 * 8);
}
#else
#define BLK_STAMP(i) do { } while (0)
#endif
#define TSF(c, q) ts[(c) * kLdXm + (q)]
template <bool NARROW>   // at most 16 right-hand sides in all: the block-column tasks' waves share the rows of one group
__global__ __launch_bounds__(kThreads, 1) void k_solve_blocks_mrhs(const SnDesc* __restrict__ sn,
                                                                   const PanelDesc* __restrict__ pds,
                                                                   const int32_t* __restrict__ rows,
                                                                   const double* __restrict__ L,
                                                                   const double* __restrict__ dinv,
                                                                   double* __restrict__ x, double* __restrict__ xscratch,
                                                                   int nrhs, int ldx, int ldq, int* __restrict__ info,
                                                                   int* __restrict__ ticket, int wait_bias, int ntasks) {
    // (x and the armed buffer as x[row * sr + q * sq]: k_solve_small_mrhs)
    const bool tr = ldq > 0;
    const int64_t sr = tr ? ldq : 1, sq = tr ? 1 : ldx;
    __shared__ double Dg[kTile * kLdDiag];   // block task: inverse diagonal block, Dg[k][row] = inv(L_jj)[row][k]
    __shared__ double ts[kTile * kLdXm];     // block task: M; chunk task: the staged X_jb as [col][q]
    __shared__ double Tx[kTile * 17];        // block task, at most 16 right-hand sides: T' as [row][q]
    __shared__ int32_t s_task, s_ok;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l15 = lane & 15, kq = lane >> 4;
    if (tid == 0) {
        s_task = atomicAdd(ticket, 1);
        s_ok = 1;
    }
    __syncthreads();
    const int plane = s_task / ntasks;
    const PanelDesc pd = pds[s_task - plane * ntasks];
    const SnDesc D = sn[pd.sn];
    const int r = D.r, w = D.w;
    const int nbc = (w + kTile - 1) / kTile;
    const double* __restrict__ G = L + D.px;
    // the status word as the waits below read it.  (A local of the kernel, which the take_x lambdas capture by reference
    // as they captured the former give_up lambda: with `info` captured directly the compiler numbers the registers
    // of this kernel differently -- tools/asm_cmp.sh, profiles/wait_evidence.md.)
    const int* const status = info;

    if (pd.row0 < 0) {
        // ================= a block column of the triangle =================
        // Every wave works for itself on 16 right-hand sides and ALL 64 rows of the block -- no LDS traffic and no
        // barrier on the chain's path: lane (q, kk) keeps T[4 st + kk][q], st = 0..15, in registers (the accumulator
        // layout of v_mfma_f64_16x16x4_f64 -- lane (q, kk) holds rows kk + 4 v of a 16-row group -- IS the B-operand
        // layout of the product with the inverse block: k step st = 4 rg + v), the rows of L(jb, k) come straight from
        // the panel as A operands (each wave reads all of them: L2 hits for three of the four).
        const int jb = pd.jb, cb = jb * kTile, wbk = min(kTile, w - cb);
        {   // inverse diagonal block -> LDS (the only shared data; one barrier per task)
            const double* __restrict__ inv_blk = dinv + (int64_t)(D.dslot + jb) * (kTile * kTile);
            double dtmp[kTile * kTile / kThreads];
#pragma unroll
            for (int t = 0; t < kTile * kTile / kThreads; ++t) dtmp[t] = inv_blk[t * kThreads + tid];
#pragma unroll
            for (int t = 0; t < kTile * kTile / kThreads; ++t) {
                const int e = t * kThreads + tid;
                Dg[(e >> 6) * kLdDiag + (e & 63)] = dtmp[t];
            }
        }
        __syncthreads();
        // The chain's step, block column jb - 1 -> jb, was 64 products with X_(jb-1), 40 with the inverse block and the
        // stores, one after the other (tools/blk_stamps.py: 2.4 + 1.4 + 0.8 of a 5.7-us hop, the hand-off itself 1.0).  With
        //     M = inv(L_jj) L(jb, jb-1)   (64 x 64, needs no X: formed here, wave v its columns 16 v .. 16 v + 15, -> LDS)
        //     P = inv(L_jj) (B_jb - sum_{k < jb-1} L(jb, k) X_k)   (formed while X_(jb-1) is still on its way)
        // what is left behind the wait is X_jb = P - M X_(jb-1): the 64 products alone, in two independent sets of
        // accumulators.
        double* __restrict__ Ms = ts;   // Ms[k][row] = M[row][k], ld kLdDiag (the layout of Dg: the same operand reads)
        if (jb > 0) {
            const int cbp = cb - kTile;
            double4_t am[4];
#pragma unroll
            for (int rg = 0; rg < 4; ++rg) am[rg] = double4_t{0, 0, 0, 0};
            // B operand: lane (j = l15, kk = kq) holds L(jb, jb-1)[4 st + kk][16 v + j]
            const double* __restrict__ bcol = G + (int64_t)(cbp + 16 * wave + l15) * r + cb;
            double lb[16];
#pragma unroll
            for (int st = 0; st < 16; ++st) {
                const int i = 4 * st + kq;
                const double v = bcol[min(i, wbk - 1)];
                lb[st] = i < wbk ? v : 0.0;
            }
#pragma unroll
            for (int st = 0; st < 16; ++st)
#pragma unroll
                for (int rg = 0; rg < 4; ++rg)
                    if (st < 4 * rg + 4)
                        am[rg] = __builtin_amdgcn_mfma_f64_16x16x4f64(Dg[(4 * st + kq) * kLdDiag + 16 * rg + l15], lb[st], am[rg], 0, 0, 0);
            // accumulator (lane (j, kk): rows 16 rg + kk + 4 v of column 16 wave + j) -> Ms[column][row]
#pragma unroll
            for (int rg = 0; rg < 4; ++rg)
#pragma unroll
                for (int v = 0; v < 4; ++v) Ms[(16 * wave + l15) * kLdDiag + 16 * rg + kq + 4 * v] = am[rg][v];
            __syncthreads();
        }
        // this lane's rows of the block as A operand: row 16 rg + l15 (clamped into the block)
        const double* __restrict__ arow[4];
        bool aok[4];
#pragma unroll
        for (int rg = 0; rg < 4; ++rg) {
            aok[rg] = 16 * rg + l15 < wbk;
            arow[rg] = G + cb + min(16 * rg + l15, wbk - 1);
        }
        for (int pass = plane; pass * kRhsM < nrhs; pass += kPassLanes) {
            const int q0 = pass * kRhsM;
            const int nq = min(kRhsM, nrhs - q0);
            if constexpr (NARROW) {
                // ---- at most 16 right-hand sides: ONE group, and the four waves share its ROWS -- wave v the rows
                // 16 v .. 16 v + 15 of the block -- instead of three of them standing by: 16 products per earlier block and
                // 16 behind the last wait (64 on one wave before: parabolic_fem-class, 8 right-hand sides, the chains 305 us of
                // a 511-us solve).  P = inv(L_jj) T' needs the rows above a wave's own: T' goes through LDS once, before the wait.
                const bool qok = l15 < nq;
                const int64_t qoff = (q0 + min(l15, nq - 1)) * sq + D.c0 * sr;
                const double* __restrict__ xq = xscratch + qoff;
                const bool aokw = 16 * wave + l15 < wbk;
                const double* __restrict__ ar = G + cb + min(16 * wave + l15, wbk - 1);
                double tvo[4];   // this wave's rows of B_jb: rows 16 wave + 4 v + kq (the accumulator layout)
#pragma unroll
                for (int v = 0; v < 4; ++v) {
                    const int c = 16 * wave + 4 * v + kq;
                    const double t = x[qoff + (cb + min(c, wbk - 1)) * sr];
                    tvo[v] = (qok && c < wbk) ? t : 0.0;
                }
                bool ok = true;
                auto take_x = [&](int k, bool lazy, double (&bv)[16]) __attribute__((always_inline)) {
                    BoundedWait wait;
                    if (lazy) {
                        const long long* __restrict__ watch = reinterpret_cast<const long long*>(xq + (k * kTile + 63) * sr);
                        while (__hip_atomic_load(watch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == kXArmed || wait_bias != 0) {
                            if (wait.expired(status)) {
                                ok = false;
                                break;
                            }
                            __builtin_amdgcn_s_sleep(48);
                        }
                    }
                    while (ok) {
                        bool in = true;
#pragma unroll
                        for (int st = 0; st < 16; ++st) {
                            const long long b = __hip_atomic_load(reinterpret_cast<const long long*>(xq + (k * kTile + 4 * st + kq) * sr),
                                                                  __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                            in = in && b != kXArmed;
                            bv[st] = qok ? __longlong_as_double(b) : 0.0;
                        }
                        if (__all((in || !qok) && wait_bias == 0)) break;
                        if (wait.expired(status)) ok = false;
                        else __builtin_amdgcn_s_sleep(1);
                    }
                };
                double4_t a0 = {0, 0, 0, 0}, a1 = {0, 0, 0, 0};
                for (int k = 0; k < jb - 1 && ok; ++k) {
                    double av[16];
#pragma unroll
                    for (int st = 0; st < 16; ++st) {
                        const double a = ar[(int64_t)(k * kTile + 4 * st + kq) * r];
                        av[st] = aokw ? a : 0.0;
                    }
                    double bv[16];
                    take_x(k, true, bv);
                    if (!ok) break;
#pragma unroll
                    for (int st = 0; st < 16; st += 2) {
                        a0 = __builtin_amdgcn_mfma_f64_16x16x4f64(av[st], bv[st], a0, 0, 0, 0);
                        a1 = __builtin_amdgcn_mfma_f64_16x16x4f64(av[st + 1], bv[st + 1], a1, 0, 0, 0);
                    }
                }
                // (a hand-off that timed out is reported; the waves leave TOGETHER, behind the barrier)
                if (!ok) {
                    if (lane == 0) wait_failed(info);
                    s_ok = 0;
                }
                // T' = B - sums -> LDS as [row][q] (every wave reads the rows up to its own)
#pragma unroll
                for (int v = 0; v < 4; ++v) Tx[(16 * wave + 4 * v + kq) * 17 + l15] = tvo[v] - (a0[v] + a1[v]);
                __syncthreads();
                if (!s_ok) return;
                double4_t out = {0, 0, 0, 0};
                for (int st = 0; st < 4 * wave + 4; ++st)     // (inv(L_jj)[row][k] = 0 for k > row)
                    out = __builtin_amdgcn_mfma_f64_16x16x4f64(Dg[(4 * st + kq) * kLdDiag + 16 * wave + l15], Tx[(4 * st + kq) * 17 + l15], out, 0, 0, 0);
                if (jb > 0) {
                    double mv[16];
#pragma unroll
                    for (int st = 0; st < 16; ++st) mv[st] = Ms[(4 * st + kq) * kLdDiag + 16 * wave + l15];
                    double bv[16];
                    take_x(jb - 1, false, bv);
                    if (!ok) {
                        if (lane == 0) wait_failed(info);
                        s_ok = 0;
                    }
                    double4_t m0 = {0, 0, 0, 0}, m1 = {0, 0, 0, 0};
#pragma unroll
                    for (int st = 0; st < 16; st += 2) {
                        m0 = __builtin_amdgcn_mfma_f64_16x16x4f64(mv[st], bv[st], m0, 0, 0, 0);
                        m1 = __builtin_amdgcn_mfma_f64_16x16x4f64(mv[st + 1], bv[st + 1], m1, 0, 0, 0);
                    }
                    out -= m0 + m1;
                }
                // (this block's x stays armed after a time-out: its waiters see the status word)
#pragma unroll
                for (int v = 0; v < 4; ++v) {
                    const int c = 16 * wave + kq + 4 * v;
                    if (c < wbk && qok && ok)
                        __hip_atomic_store(&xscratch[qoff + (cb + c) * sr], unarmed(out[v]), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
#pragma unroll
                for (int v = 0; v < 4; ++v) {
                    const int c = 16 * wave + kq + 4 * v;
                    if (c < wbk && qok && ok) x[qoff + (cb + c) * sr] = out[v];
                }
                __syncthreads();   // (Tx is free for the next pass)
                if (!s_ok) return;
                continue;
            } else {
            if (16 * wave >= nq) continue;             // (this wave's 16 right-hand sides are not in the pass)
            const bool qok = 16 * wave + l15 < nq;
            const int64_t qoff = (q0 + min(16 * wave + l15, nq - 1)) * sq + D.c0 * sr;   // this lane's right-hand side, row c0
            const double* __restrict__ xq = xscratch + qoff;      // ... in the armed buffer
            // B_jb (with every contribution of the levels below): rows 4 st + kq
            double tv[16];
#pragma unroll
            for (int st = 0; st < 16; ++st) {
                const int c = 4 * st + kq;
                const double v = x[qoff + (cb + min(c, wbk - 1)) * sr];
                tv[st] = (qok && c < wbk) ? v : 0.0;
            }
            double4_t acc[4];   // [16 rows rg]: lane (q = l15, row = kq + 4 v)
#pragma unroll
            for (int rg = 0; rg < 4; ++rg) acc[rg] = double4_t{0, 0, 0, 0};
            bool ok = true;
            // X_k (this wave's 16 right-hand sides, rows 4 st + kq) as soon as it is there; lazy: a block that is not the
            // one right before this one first watches ONE value, then goes on to the full poll (normally satisfied at once)
            auto take_x = [&](int k, bool lazy, double (&bv)[16]) __attribute__((always_inline)) {
                BoundedWait wait;
                if (lazy) {
                    const long long* __restrict__ watch = reinterpret_cast<const long long*>(xq + (k * kTile + 63) * sr);
                    while (__hip_atomic_load(watch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == kXArmed || wait_bias != 0) {
                        if (wait.expired(status)) {
                            ok = false;
                            break;
                        }
                        __builtin_amdgcn_s_sleep(48);
                    }
                }
                while (ok) {
                    bool in = true;
#pragma unroll
                    for (int st = 0; st < 16; ++st) {
                        const long long b = __hip_atomic_load(reinterpret_cast<const long long*>(xq + (k * kTile + 4 * st + kq) * sr),
                                                              __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        in = in && b != kXArmed;
                        bv[st] = qok ? __longlong_as_double(b) : 0.0;
                    }
                    if (__all((in || !qok) && wait_bias == 0)) break;
                    if (wait.expired(status)) ok = false;
                    else __builtin_amdgcn_s_sleep(1);
                }
            };
            for (int k = 0; k < jb - 1 && ok; ++k) {
                // L(jb, k): columns 64 k + 4 st + kq, issued before the wait for X_k
                double av[16][4];
#pragma unroll
                for (int st = 0; st < 16; ++st) {
                    const int64_t col = (int64_t)(k * kTile + 4 * st + kq) * r;
#pragma unroll
                    for (int rg = 0; rg < 4; ++rg) {
                        const double a = arow[rg][col];
                        av[st][rg] = aok[rg] ? a : 0.0;
                    }
                }
                double bv[16];
                take_x(k, true, bv);
                if (!ok) break;
#pragma unroll
                for (int st = 0; st < 16; ++st)
#pragma unroll
                    for (int rg = 0; rg < 4; ++rg)
                        acc[rg] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[st][rg], bv[st], acc[rg], 0, 0, 0);
            }
            if (!ok) {   // a hand-off timed out: reported; this block's x stays armed, its waiters give up on the status word
                if (lane == 0) wait_failed(info);
                return;
            }
            // T' = B - sum: k step st = 4 rg + v of the product with the inverse block
#pragma unroll
            for (int rg = 0; rg < 4; ++rg)
#pragma unroll
                for (int v = 0; v < 4; ++v) tv[4 * rg + v] -= acc[rg][v];
            // P = inv(L_jj) T' (row group rg needs k <= 16 rg + 15) -- X_jb itself for the first block column
            double4_t out[4];
#pragma unroll
            for (int rg = 0; rg < 4; ++rg) out[rg] = double4_t{0, 0, 0, 0};
#pragma unroll
            for (int st = 0; st < 16; ++st)
#pragma unroll
                for (int rg = 0; rg < 4; ++rg)
                    if (st < 4 * rg + 4)
                        out[rg] = __builtin_amdgcn_mfma_f64_16x16x4f64(Dg[(4 * st + kq) * kLdDiag + 16 * rg + l15], tv[st], out[rg], 0, 0, 0);
            if (jb > 0) {
                // M as A operand (rows 16 rg + l15, columns 4 st + kq), in registers before the wait
                double mv[16][4];
#pragma unroll
                for (int st = 0; st < 16; ++st)
#pragma unroll
                    for (int rg = 0; rg < 4; ++rg) mv[st][rg] = Ms[(4 * st + kq) * kLdDiag + 16 * rg + l15];
                double bv[16];
                take_x(jb - 1, false, bv);
                if (!ok) {
                    if (lane == 0) wait_failed(info);
                    return;
                }
                BLK_STAMP(0);
                double4_t m0[4], m1[4];
#pragma unroll
                for (int rg = 0; rg < 4; ++rg) m0[rg] = m1[rg] = double4_t{0, 0, 0, 0};
#pragma unroll
                for (int st = 0; st < 16; st += 2)
#pragma unroll
                    for (int rg = 0; rg < 4; ++rg) {
                        m0[rg] = __builtin_amdgcn_mfma_f64_16x16x4f64(mv[st][rg], bv[st], m0[rg], 0, 0, 0);
                        m1[rg] = __builtin_amdgcn_mfma_f64_16x16x4f64(mv[st + 1][rg], bv[st + 1], m1[rg], 0, 0, 0);
                    }
#pragma unroll
                for (int rg = 0; rg < 4; ++rg) out[rg] -= m0[rg] + m1[rg];
            }
#ifdef PARSY_BLKSTAMPS
            asm volatile("" ::"v"(out[3][3]));
            BLK_STAMP(1);
#endif
            // straight from the accumulators to x and the armed buffer (lane (q = l15, row = kq + 4 v))
            // (the armed buffer first: it is what the next block column polls)
            BLK_STAMP(2);
#pragma unroll
            for (int rg = 0; rg < 4; ++rg)
#pragma unroll
                for (int v = 0; v < 4; ++v) {
                    const int c = 16 * rg + kq + 4 * v;
                    if (c < wbk && qok)
                        __hip_atomic_store(&xscratch[qoff + (cb + c) * sr], unarmed(out[rg][v]), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
            BLK_STAMP(3);
#pragma unroll
            for (int rg = 0; rg < 4; ++rg)
#pragma unroll
                for (int v = 0; v < 4; ++v) {
                    const int c = 16 * rg + kq + 4 * v;
                    if (c < wbk && qok) x[qoff + (cb + c) * sr] = out[rg][v];
                }
            }
        }
        return;
    }

    // ================= a 128-row chunk of the rows below the supernode's columns =================
    // wave = 32 rows; its rows of L against block column jb + 1 are loaded while block column jb is multiplied (two
    // register sets: with one set and 64 rows per wave the loads had only the hand-off to hide behind, and the one wave
    // per SIMD that fits waited for them: 16 TFLOP/s on the Flan-class input)
    const int row0 = pd.row0;
    const int wrow0 = row0 + (kSolveRowsM / 4) * wave;   // first panel row of this wave
    int prow[2];                                         // this lane's row of each 16-row fragment (-1: past the panel)
#pragma unroll
    for (int rf = 0; rf < 2; ++rf) prow[rf] = (wrow0 + 16 * rf + l15 < r && 16 * rf + (kSolveRowsM / 4) * wave < kSolveRowsM)
                                                   ? wrow0 + 16 * rf + l15 : -1;
    const bool wave_on = wrow0 < r;
    auto load_l = [&](int jb, double (&lv)[2][16]) {
        const int cb = jb * kTile, wbk = min(kTile, w - cb);
        if (!wave_on || jb >= nbc) return;
#pragma unroll
        for (int rf = 0; rf < 2; ++rf)
#pragma unroll
            for (int st = 0; st < 16; ++st) {
                const int c = 4 * st + kq;
                const bool okl = prow[rf] >= 0 && c < wbk;
                const double v = G[(int64_t)(cb + min(c, wbk - 1)) * r + max(prow[rf], 0)];
                lv[rf][st] = okl ? v : 0.0;
            }
    };
    for (int pass = plane; pass * kRhsM < nrhs; pass += kPassLanes) {
        const int q0 = pass * kRhsM;
        const int nq = min(kRhsM, nrhs - q0);
        const int nfn = (nq + 15) >> 4;                 // 16-wide fragments of right-hand sides in use
        double4_t acc[4][2];                            // [fragment of right-hand sides][fragment of rows]
#pragma unroll
        for (int nf = 0; nf < 4; ++nf)
#pragma unroll
            for (int rf = 0; rf < 2; ++rf) acc[nf][rf] = double4_t{0, 0, 0, 0};
        double lvA[2][16], lvB[2][16];
        load_l(0, lvA);
        // one block column: stage X_jb (armed buffer -> LDS), start the loads of the next one, multiply
        auto step = [&](int jb, double (&cur)[2][16], double (&nxt)[2][16]) -> bool {
            const int cb = jb * kTile, wbk = min(kTile, w - cb);
            __syncthreads();  // ts of the previous block column is free
            {   // thread (c, q) = (tid & 63, (tid >> 6) + 4 u) -- or, X row-major, ((tid >> 6) + 4 u, tid & 63): 16 values each
                BoundedWait wait;
                const int lo = tid & 63, hi = tid >> 6;
                double xv[kRhsM / 4];
                bool ok = true;
                const bool any = tr ? lo < nq : lo < wbk;
                if (any) {
                    // (a chunk far behind the chain first watches one value lazily)
                    const int cw = tr ? min(hi, wbk - 1) : lo, qw = tr ? lo : 0;
                    const long long* __restrict__ watch =
                        reinterpret_cast<const long long*>(xscratch + (D.c0 + cb + cw) * sr + (q0 + qw) * sq);
                    while (__hip_atomic_load(watch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == kXArmed || wait_bias != 0) {
                        if (wait.expired(status)) {
                            ok = false;
                            break;
                        }
                        __builtin_amdgcn_s_sleep(16);
                    }
                    while (ok) {
                        bool in = true;
#pragma unroll
                        for (int u = 0; u < kRhsM / 4; ++u) {
                            const int c = tr ? hi + 4 * u : lo, q = tr ? lo : hi + 4 * u;
                            long long b = 0;
                            if (q < nq && c < wbk)
                                b = __hip_atomic_load(reinterpret_cast<const long long*>(
                                                          xscratch + (D.c0 + cb + c) * sr + (q0 + q) * sq),
                                                      __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                            in = in && b != kXArmed;
                            xv[u] = __longlong_as_double(b);
                        }
                        if (in) break;
                        if (wait.expired(status)) ok = false;
                        else __builtin_amdgcn_s_sleep(1);
                    }
                } else {
#pragma unroll
                    for (int u = 0; u < kRhsM / 4; ++u) xv[u] = 0.0;
                }
                if (!ok) {
                    wait_failed(info);
                    s_ok = 0;
                }
#pragma unroll
                for (int u = 0; u < kRhsM / 4; ++u) {
                    const int c = tr ? hi + 4 * u : lo, q = tr ? lo : hi + 4 * u;
                    TSF(c, q) = xv[u];
                }
            }
            __syncthreads();
            if (!s_ok) return false;
            load_l(jb + 1, nxt);
            // accumulator += x_jb' L(rows, jb)'
            if (wave_on) {
#pragma unroll
                for (int nf = 0; nf < 4; ++nf) {
                    if (nf < nfn) {
#pragma unroll
                        for (int st = 0; st < 16; ++st) {
                            const double av = TSF(4 * st + kq, 16 * nf + l15);
#pragma unroll
                            for (int rf = 0; rf < 2; ++rf)
                                acc[nf][rf] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, cur[rf][st], acc[nf][rf], 0, 0, 0);
                        }
                    }
                }
            }
            return true;
        };
        for (int jb = 0; jb < nbc; jb += 2) {
            if (!step(jb, lvA, lvB)) return;
            if (jb + 1 < nbc && !step(jb + 1, lvB, lvA)) return;
        }
        // x[row] -= accumulated update
#pragma unroll
        for (int rf = 0; rf < 2; ++rf) {
            if (prow[rf] >= 0) {
                const int xrow = rows[D.pi + prow[rf]];
#pragma unroll
                for (int nf = 0; nf < 4; ++nf)
#pragma unroll
                    for (int v = 0; v < 4; ++v) {
                        const int q = 16 * nf + kq + 4 * v;
                        if (q < nq) atomicAdd(&x[xrow * sr + (q0 + q) * sq], -acc[nf][rf][v]);
                    }
            }
        }
    }
}
#undef TSF

// (k: narrow up to 16 right-hand sides -- route_launch, solve_route.cpp)
void launch_solve_blocks_mrhs(const DevicePattern& P, WitnessKernel k, int first, int count, const double* L, const double* dinv,
                              double* x, double* xscratch, int nrhs, int ldx, int ldq, int ticket, int wait_bias,
                              hipStream_t stream) {
    if (count <= 0) return;
    const int lanes_m = std::min(kPassLanes, (nrhs + kRhsM - 1) / kRhsM);
    if (k == kWSolveBlocksMrhsNarrow) {
        launch_witnessed<k_solve_blocks_mrhs<true>, kWSolveBlocksMrhsNarrow>(dim3(count * lanes_m), dim3(kThreads), 0,
            stream, P.sn, P.solve_mtasks + first, P.rows, L, dinv, x, xscratch, nrhs, ldx, ldq, P.sinfo,
            P.stickets + ticket, wait_bias, count);
    } else if (k == kWSolveBlocksMrhs) {
        launch_witnessed<k_solve_blocks_mrhs<false>, kWSolveBlocksMrhs>(dim3(count * lanes_m), dim3(kThreads), 0,
            stream, P.sn, P.solve_mtasks + first, P.rows, L, dinv, x, xscratch, nrhs, ldx, ldq, P.sinfo,
            P.stickets + ticket, wait_bias, count);
    } else {
        launch_refused("launch_solve_blocks_mrhs", k);
    }
}

// One right-hand side: the chain launches hand x over through xscratch itself (k_solve_chain_w); every entry must
// hold the armed pattern when the solve starts.
hipError_t solve_arm_handoff(double* xscratch, int64_t n, hipStream_t stream) {
    return hipMemsetD32Async((hipDeviceptr_t)xscratch, (int)kXArmedWord, (size_t)n * 2, stream);
}

// Start of a solve with several right-hand sides, ONE launch instead of three memsets and a fill of the whole hand-off
// buffer: the solve's status word and the ticket counters of its chain launches are zeroed (block 0), and the hand-off
// buffer is armed where it is polled -- the columns of the wide supernodes (one workgroup per (supernode, block column) of
// solve_wide_list: a chain launch waits only for x of block columns of its own supernode).  The fill of all n x nrhs
// entries took 39 us on the parabolic_fem-class input (269 MB at 64 right-hand sides) and the three memsets 20 us more
// with the gaps between them: 0.13 of a 1.19-ms solve.
__global__ __launch_bounds__(kThreads) void k_solve_arm_wide(const SnDesc* __restrict__ sn, const int32_t* __restrict__ wide,
                                                             int npairs, double* __restrict__ xscratch, int nrhs, int64_t sr,
                                                             int64_t sq, int* __restrict__ sinfo, int* __restrict__ stickets,
                                                             int ntickets) {
    const int tid = threadIdx.x;
    if (blockIdx.x == 0) {
        if (tid == 0) *sinfo = 0;
        for (int t = tid; t < ntickets; t += kThreads) stickets[t] = 0;
    }
    if ((int)blockIdx.x >= npairs) return;
    const SnDesc D = sn[wide[2 * blockIdx.x]];
    const int cb = kTile * wide[2 * blockIdx.x + 1], wb = min(kTile, D.w - cb);
    long long* __restrict__ xs = reinterpret_cast<long long*>(xscratch);
    // (lanes along the contiguous index of the layout: columns when right-hand-side-major, right-hand sides when row-major)
    if (sr == 1) {
        for (int e = tid; e < wb * nrhs; e += kThreads) {
            const int q = e / wb, c = e - q * wb;
            xs[(int64_t)(D.c0 + cb + c) + q * sq] = kXArmed;
        }
    } else {
        for (int e = tid; e < wb * nrhs; e += kThreads) {
            const int c = e / nrhs, q = e - c * nrhs;
            xs[(int64_t)(D.c0 + cb + c) * sr + q * sq] = kXArmed;
        }
    }
}

void launch_solve_arm_wide(const DevicePattern& P, int npairs, double* xscratch, int nrhs, int ldx, int ldq, int ntickets,
                           hipStream_t stream) {
    const bool tr = ldq > 0;
    launch_witnessed<k_solve_arm_wide, kWSolveArmWide>(dim3(std::max(npairs, 1)), dim3(kThreads), 0, stream, P.sn,
        P.solve_wide_list, npairs, xscratch, nrhs, (int64_t)(tr ? ldq : 1), (int64_t)(tr ? 1 : ldx), P.sinfo,
        P.stickets, ntickets);
}

// One right-hand side: xscratch was armed by the caller (solve_arm_handoff)
// (k: <2> up to SolveGates::chain_few_chunks chunks, else <4> -- route_launch, solve_route.cpp)
void launch_solve_chain(const DevicePattern& P, WitnessKernel k, int first, int count, const double* L, const double* dinv, double* x,
                        double* xscratch, int ticket, int wait_bias, hipStream_t stream) {
    if (count <= 0) return;
    if (k == kWSolveChainW2) {
        launch_witnessed<k_solve_chain_w<2>, kWSolveChainW2>(dim3(2 * count), dim3(kChainThreads), 0, stream, P.sn,
            P.solve_panels + first, P.rows, L, dinv, x, xscratch, P.sinfo, P.stickets + ticket, wait_bias);
    } else if (k == kWSolveChainW4) {
        launch_witnessed<k_solve_chain_w<4>, kWSolveChainW4>(dim3(count), dim3(kChainThreads), 0, stream, P.sn,
            P.solve_panels + first, P.rows, L, dinv, x, xscratch, P.sinfo, P.stickets + ticket, wait_bias);
    } else {
        launch_refused("launch_solve_chain", k);
    }
}

// ---------------------------------------------------------------------------
// ONE-launch solves of small plans (Schedule::solve_one): a job of a few thousand supernodes is ten to twenty level
// launches of a few microseconds of work each -- the ex15-class forward solve took 0.126 ms, slower than one CPU
// thread (0.0745 ms), all of it launch latency and hand-offs through memory.  Here a solve is ONE enqueue: one
// workgroup per block column, taken by ticket in level order (a workgroup only ever waits for blocks with smaller
// tickets, which are held by workgroups that run or have finished: no deadlock at any residency), and instead of
// level barriers every value is handed over as the data itself: the hand-off buffer holds the armed pattern when the
// solve starts and a value is valid once it differs (8-byte agent-scope atomics both sides, as the chain launches'
// xscratch) -- ONE memory round trip per step of the critical path.
// Forward: the tasks are BLOCK COLUMNS (<= 64 columns of a supernode: Schedule::one_sn).  What block p subtracts from
// the x of row k below its columns -- a later column of its supernode or a row of an ancestor --, c = L[k, cols] y_p,
// is not added to x but written to a slot of its own (written once); the block that owns row k gathers its slots
// (one_pull_*: all of them polled at once, one per thread), solves its diagonal block, publishes x and then its own
// c's -- from its panel, which it staged in LDS BEFORE it waited (L does not depend on anybody).
// The same sums as the level launches, in gather order (the reference's `omp atomic` order is schedule-dependent
// as well: triangularSolve/Triangular_BCSC.h:139-157).  Earlier forms, all measured on the ex15-class input:
// atomics on x + a dependency counter per supernode (three round trips per step) 0.098 ms; a pull through the
// factorization's update lists (the top separators then stream every row inside their columns themselves, after
// their last descendant) 0.175 ms; whole supernodes as tasks (the 124-column root then spends 24 us on its two block
// columns, its second diagonal block and the rows between them fetched on the critical path) 0.093 ms.
// No memset either: a solve arms the OTHER buffer of its kind (its supernode's slots / columns) and zeroes the other
// {status, ticket} pair for the solve after it; the executor alternates.  Every wait is bounded like the chain
// launches' (2 s, status -1, nobody hangs).
__device__ __forceinline__ double one_poll(const double* p, int* info, int wait_bias, bool& ok) {
    const long long* src = reinterpret_cast<const long long*>(p);
    BoundedWait wait;
    for (;;) {
        const long long b = __hip_atomic_load(src, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (b != kXArmed && wait_bias == 0) return __longlong_as_double(b);
        if (wait.expired(info)) {
            wait_failed(info);   // (the result is wrong and reported)
            ok = false;
            return 0.0;
        }
        if (wait.spins < 8) __builtin_amdgcn_s_sleep(1);
        else __builtin_amdgcn_s_sleep(8);   // (the late ones poll at leisure)
    }
}
// the values of NQ right-hand sides of one slot: the loads go out together, the polls only where a value is not there yet
// (one after the other they were NQ round trips per slot)
template <int NQ>
__device__ __forceinline__ void one_poll_n(const double* p, int64_t stride, int nrhs, double (&v)[NQ], int* info, int wait_bias,
                                           bool& ok) {
    long long b[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q)
        b[q] = q < nrhs ? __hip_atomic_load(reinterpret_cast<const long long*>(p + (int64_t)q * stride), __ATOMIC_RELAXED,
                                            __HIP_MEMORY_SCOPE_AGENT)
                        : 0;
#pragma unroll
    for (int q = 0; q < NQ; ++q)
        v[q] = q >= nrhs ? 0.0 : (b[q] == kXArmed || wait_bias != 0) ? one_poll(p + (int64_t)q * stride, info, wait_bias, ok)
                                                                     : __longlong_as_double(b[q]);
}
// what every workgroup of a ONE-launch solve does first: its part (entries [e0, e0 + len) per right-hand side, stride
// ldy) of the NEXT solve's buffer is armed, and the first ticket zeroes the next solve's {status, ticket}
__device__ __forceinline__ void one_arm_next(double* __restrict__ y_next, int* __restrict__ state_next, int64_t ldy, int64_t e0,
                                             int len, int task, int tid, int cap) {
    for (int e = tid; e < len * cap; e += kThreads) {   // (cap: right-hand sides the buffers are made for)
        const int q = e / len, c = e - q * len;
        reinterpret_cast<long long*>(y_next)[(int64_t)q * ldy + e0 + c] = kXArmed;
    }
    if (task == 0 && tid < 2) state_next[tid] = 0;
}

#ifdef PARSY_ONESTAMPS
// diagnostic build: per supernode the 100 MHz wall clock at five points of k_solve_one (tools/one_stamps.py)
__device__ unsigned long long g_onestamp[4096 * 8];
#define ONESTAMP(i) do { if (tid == 0 && t < 4096) g_onestamp[t * 8 + (i)] = wall_clock64(); } while (0)
#else
#define ONESTAMP(i) do { } while (0)
#endif
static constexpr int kOneRows = 256;     // rows below a block whose x the backward solve keeps in LDS
// doubles of a block's rows below its columns staged in LDS (a larger panel waits in registers); forward, by right-hand
// sides carried: what leaves room for TWO workgroups per compute unit beside the other arrays (80 KB each)
template <int NQ> struct OneStage { static constexpr int fwd = NQ <= 4 ? 4096 : 3584, bwd = 4096; };
// The inverse M of a diagonal block (<= 64 x 64, column-major in Dg, identity padded to wpad), in place.  First the 16 x 16
// diagonal sub-blocks (block_invert16), copied dense into s_m; then, block row by block row from the bottom up and inside
// a row from right to left,
//     M_ij = -(sum_{k = j + 1}^{i} M_ik L_kj) M_jj
// which overwrites L_ij (no later block reads it: rows above use only rows <= their own of L).  One thread per entry;
// ends synchronised.  Afterwards M[c][k], k <= c, is s_m[..] inside c's 16-block and Dg[k * kLdDiag + c] left of it.
__device__ __forceinline__ void one_invert_block(double* Dg, double* invd, double* s_t, double (*s_m)[16 * 17], int w, int wpad,
                                                 int tid) {
    block_invert16(Dg, invd, w, tid);   // (ends synchronised)
    for (int e = tid; e < (wpad / 16) * 256; e += kThreads) {
        const int b = e >> 8, rr = (e >> 4) & 15, cc = e & 15;
        s_m[b][rr * 17 + cc] = rr > cc ? Dg[(16 * b + rr) * kLdDiag + 16 * b + cc] : (rr == cc ? invd[16 * b + rr] : 0.0);
    }
    __syncthreads();
    {
        const int rr = tid >> 4, cc = tid & 15;
        for (int bi = wpad - 16; bi >= 16; bi -= 16)
            for (int bj = bi - 16; bj >= 0; bj -= 16) {
                // T = sum_k M_ik L_kj, k from j + 1 to i (M_ii from the dense copy, the others already in place)
                double tv = 0.0;
                for (int bk = bj + 16; bk < bi; bk += 16) {
#pragma unroll
                    for (int m = 0; m < 16; ++m)
                        tv = fma(Dg[(bk + m) * kLdDiag + bi + rr], Dg[(bj + cc) * kLdDiag + bk + m], tv);
                }
#pragma unroll
                for (int m = 0; m < 16; ++m) tv = fma(s_m[bi >> 4][rr * 17 + m], Dg[(bj + cc) * kLdDiag + bi + m], tv);
                s_t[rr * 17 + cc] = tv;
                __syncthreads();   // (T complete, and every read of L_ij is done: it is overwritten next)
                double mv = 0.0;
#pragma unroll
                for (int m = 0; m < 16; ++m) mv = fma(s_t[rr * 17 + m], s_m[bj >> 4][m * 17 + cc], mv);
                Dg[(bj + cc) * kLdDiag + bi + rr] = -mv;
                __syncthreads();
            }
    }
}

// NQ: right-hand sides carried (1, 4 or 8).  On the critical path -- between the last slot's arrival and the block's
// own slots going out -- there are two LDS matrix-vector products and nothing else: the INVERSE of the diagonal block
// is formed while the block waits (it had 6 - 35 us of slack on the ex15-class chain; the blocked substitution of
// k_solve_small took 1.1 - 4.8 us per step of the chain instead).
template <int NQ>
__global__ __launch_bounds__(kThreads) void k_solve_one(const SnDesc* __restrict__ blocks, const int64_t* __restrict__ slot0,
                                                        const int32_t* __restrict__ pull_ptr,
                                                        const int32_t* __restrict__ pull_slot,
                                                        const int32_t* __restrict__ pull_pos, const double* __restrict__ L,
                                                        double* __restrict__ x, int nrhs, int ldx, int64_t nslots,
                                                        double* __restrict__ y, double* __restrict__ y_next,
                                                        int* __restrict__ state, int* __restrict__ state_next,
                                                        int wait_bias, int cap) {
    __shared__ double Dg[kTile * kLdDiag];  // the diagonal block (column-major), then its inverse in place (see below);
                                            // at the end: the parts of the products below
    __shared__ double invd[kTile];
    __shared__ double s_t[16 * 17];         // a 16 x 16 block of the inverse under way
    __shared__ double s_m[kTile / 16][16 * 17];   // the inverses of the 16 x 16 diagonal sub-blocks, dense (zero above the diagonal)
    __shared__ double s_b[kTile][NQ];       // the block's right-hand side minus what the gathered slots say
    __shared__ double s_x[kTile][NQ];       // its solution
    __shared__ double s_pan[OneStage<NQ>::fwd];     // the rows below the block's columns, [c][k - w] (row stride nb | 1)
    __shared__ int s_task;
    static_assert(4 * kTile * 8 <= kTile * kLdDiag, "the products' parts reuse Dg");
    const int tid = threadIdx.x;
    if (tid == 0) s_task = atomicAdd(&state[1], 1);
    __syncthreads();
    const int t = s_task;                   // (the blocks are listed in ticket order)
    const SnDesc D = blocks[t];
    const int w = D.w, nb = D.r - w, ldp = nb | 1, ld = D.ld;
    const double* __restrict__ G = L + D.px;
    const int64_t s0 = slot0[t];
    ONESTAMP(0);
    one_arm_next(y_next, state_next, nslots, s0, nb, t, tid, cap);
    // ---- what does not depend on the other blocks: the right-hand side, the panel below the columns (small: LDS), the
    // diagonal block and its inverse
    for (int e = tid; e < kTile * NQ; e += kThreads) {
        const int q = e / kTile, c = e - q * kTile;
        s_b[c][q] = (c < w && q < nrhs) ? x[(int64_t)q * ldx + D.c0 + c] : 0.0;
    }
    const bool staged = w * ldp <= OneStage<NQ>::fwd;
    if (staged)
        for (int e = tid; e < w * nb; e += kThreads) {
            const int c = e / nb, k = e - c * nb;
            s_pan[c * ldp + k] = G[(int64_t)c * ld + w + k];
        }
    // (a larger panel: the first 256 rows below, one per thread, wait in REGISTERS -- the rows after them are streamed at the end)
    double pre[kTile];
    if (!staged && nb > 0) {
#pragma unroll
        for (int c = 0; c < kTile; ++c) pre[c] = G[(int64_t)min(c, w - 1) * ld + w + min(tid, nb - 1)];
    }
    const int wpad = (w + 15) & ~15;
    for (int e = tid; e < wpad * wpad; e += kThreads) {
        const int c = e / wpad, i = e - c * wpad;
        double v = (i == c) ? 1.0 : 0.0;
        if (i >= c && i < w && c < w) v = G[(int64_t)c * ld + i];
        Dg[c * kLdDiag + i] = v;
    }
    __syncthreads();
    one_invert_block(Dg, invd, s_t, s_m, w, wpad, tid);   // (ends synchronised)
    auto m_at = [&](int c, int k) {   // M[c][k], k <= c
        const int b = c & ~15;
        return k >= b ? s_m[b >> 4][(c - b) * 17 + (k - b)] : Dg[k * kLdDiag + c];
    };
    ONESTAMP(1);
    // ---- gather: one slot per thread and right-hand side, all polls in flight together
    {
        bool ok = true;
        for (int e = pull_ptr[t] + tid; e < pull_ptr[t + 1]; e += kThreads) {
            const int64_t slot = pull_slot[e];
            const int pos = pull_pos[e];
            double v[NQ];
            one_poll_n<NQ>(&y[slot], nslots, nrhs, v, state, wait_bias, ok);
#pragma unroll
            for (int q = 0; q < NQ; ++q)
                if (q < nrhs) unsafeAtomicAdd(&s_b[pos][q], -v[q]);
        }
    }
    __syncthreads();
    ONESTAMP(2);
    // ---- x = inv(L_bb) b: four lanes per row share the sum
    {
        const int c = tid >> 2, part = tid & 3;
        double acc[NQ];
#pragma unroll
        for (int q = 0; q < NQ; ++q) acc[q] = 0.0;
        if (c < w) {
            for (int k = part; k <= c; k += 4) {
                const double iv = m_at(c, k);
#pragma unroll
                for (int q = 0; q < NQ; ++q) acc[q] = fma(iv, s_b[k][q], acc[q]);
            }
        }
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            acc[q] += __shfl_xor(acc[q], 1);
            acc[q] += __shfl_xor(acc[q], 2);
        }
        if (part == 0 && c < kTile) {
#pragma unroll
            for (int q = 0; q < NQ; ++q) {
                s_x[c][q] = c < w ? acc[q] : 0.0;
                if (c < w && q < nrhs) x[(int64_t)q * ldx + D.c0 + c] = acc[q];
            }
        }
    }
    __syncthreads();
    ONESTAMP(3);
    auto publish = [&](int k, int q, double v) {
        __hip_atomic_store(&y[(int64_t)q * nslots + s0 + k], unarmed(v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    };
    // ---- what this block subtracts from the rows below its columns: published, one slot per row.  Up to 256 staged
    // rows: the columns are dealt over P = 4 / 2 / 1 groups of threads, the parts added up through LDS
    const int nbp = (nb + 63) & ~63;
    if (staged && nbp <= kThreads && nb > 0) {
        const int P = kThreads / nbp;                 // 4, 2 or 1 (nbp = 64, 128, 192 / 256)
        const int part = tid / nbp, k = tid - part * nbp;
        double* __restrict__ red = Dg;                // [part][q][k]: the inverse is not needed any more
        if (part < P) {
            double acc[NQ];
#pragma unroll
            for (int q = 0; q < NQ; ++q) acc[q] = 0.0;
            if (k < nb) {
                const int c_lo = part * w / P, c_hi = (part + 1) * w / P;
                for (int c = c_lo; c < c_hi; ++c) {
                    const double lv = s_pan[c * ldp + k];
#pragma unroll
                    for (int q = 0; q < NQ; ++q) acc[q] = fma(lv, s_x[c][q], acc[q]);
                }
            }
            if (P > 1) {
#pragma unroll
                for (int q = 0; q < NQ; ++q) red[(part * NQ + q) * nbp + k] = acc[q];
            } else if (k < nb) {
#pragma unroll
                for (int q = 0; q < NQ; ++q)
                    if (q < nrhs)
                        __hip_atomic_store(&y[(int64_t)q * nslots + s0 + k], unarmed(acc[q]), __ATOMIC_RELAXED,
                                           __HIP_MEMORY_SCOPE_AGENT);
            }
        }
        if (P > 1) {
            __syncthreads();
            for (int e = tid; e < nb * NQ; e += kThreads) {
                const int q = e / nb, kk = e - q * nb;
                double v = 0.0;
                for (int pp = 0; pp < P; ++pp) v += red[(pp * NQ + q) * nbp + kk];
                if (q < nrhs)
                    __hip_atomic_store(&y[(int64_t)q * nslots + s0 + kk], unarmed(v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
    } else if (staged) {
        for (int k = tid; k < nb; k += kThreads) {
            double acc[NQ];
#pragma unroll
            for (int q = 0; q < NQ; ++q) acc[q] = 0.0;
            for (int c = 0; c < w; ++c) {
                const double lv = s_pan[c * ldp + k];
#pragma unroll
                for (int q = 0; q < NQ; ++q) acc[q] = fma(lv, s_x[c][q], acc[q]);
            }
#pragma unroll
            for (int q = 0; q < NQ; ++q)
                if (q < nrhs) publish(k, q, acc[q]);
        }
    } else {
        // a larger panel: the first 256 rows from the registers they have been waiting in ...
        if (tid < nb) {
            double acc[NQ];
#pragma unroll
            for (int q = 0; q < NQ; ++q) acc[q] = 0.0;
#pragma unroll
            for (int c = 0; c < kTile; ++c)
                if (c < w) {
#pragma unroll
                    for (int q = 0; q < NQ; ++q) acc[q] = fma(pre[c], s_x[c][q], acc[q]);
                }
#pragma unroll
            for (int q = 0; q < NQ; ++q)
                if (q < nrhs) publish(tid, q, acc[q]);
        }
        // ... the rows after them in chunks of 128, two register sets (as the backward kernel's far rows): wave v takes the
        // columns v, v + 4, ..., lane l the rows l and l + 64 of a chunk and sums its 16 columns in place; the four waves'
        // parts meet in LDS (the inverse's place) and one thread per row publishes.  The loads of the chunk after next go
        // out as soon as a set is multiplied.
        if (nb > kThreads) {
            constexpr int kChunk = 128, kPc = kTile / (kThreads / 64), kPr = kChunk / 64;
            constexpr int kHalves = NQ <= 4 ? 2 : 1;   // (8 right-hand sides: one buffer of parts, two barriers per chunk)
            static_assert(kHalves * (kThreads / 64) * kChunk * NQ <= kTile * kLdDiag, "the waves' parts reuse Dg");
            const int wave = tid >> 6, lane = tid & 63;
            const int nchunks = (nb - kThreads + kChunk - 1) / kChunk;
            double fs[2][kPc][kPr];
            auto fetch = [&](double (&dst)[kPc][kPr], int ch) {
                const int k0 = kThreads + ch * kChunk;
#pragma unroll
                for (int ci = 0; ci < kPc; ++ci) {
                    const double* __restrict__ col = G + (int64_t)min(wave + (kThreads / 64) * ci, w - 1) * ld + w;
#pragma unroll
                    for (int jr = 0; jr < kPr; ++jr) dst[ci][jr] = col[min(k0 + lane + 64 * jr, nb - 1)];
                }
            };
            fetch(fs[0], 0);
            if (nchunks > 1) fetch(fs[1], 1);
            double* __restrict__ part = Dg;   // [half][wave][row of the chunk][q]
            auto step = [&](double (&cur)[kPc][kPr], int ch) {
                const int k0 = kThreads + ch * kChunk, len = min(kChunk, nb - k0);
                const int half = (kHalves == 2 ? (ch & 1) : 0) * ((kThreads / 64) * kChunk * NQ);
                double pr[kPr][NQ];
#pragma unroll
                for (int jr = 0; jr < kPr; ++jr)
#pragma unroll
                    for (int q = 0; q < NQ; ++q) pr[jr][q] = 0.0;
#pragma unroll
                for (int ci = 0; ci < kPc; ++ci) {
                    const int c = wave + (kThreads / 64) * ci;
                    if (c < w) {
#pragma unroll
                        for (int jr = 0; jr < kPr; ++jr)
#pragma unroll
                            for (int q = 0; q < NQ; ++q) pr[jr][q] = fma(cur[ci][jr], s_x[c][q], pr[jr][q]);
                    }
                }
                if (ch + 2 < nchunks) fetch(cur, ch + 2);
                if (kHalves == 1) __syncthreads();   // (the parts of the chunk before are read)
#pragma unroll
                for (int jr = 0; jr < kPr; ++jr)
#pragma unroll
                    for (int q = 0; q < NQ; ++q) part[half + ((wave * kChunk) + lane + 64 * jr) * NQ + q] = pr[jr][q];
                __syncthreads();
                if (tid < len) {
#pragma unroll
                    for (int q = 0; q < NQ; ++q) {
                        double v = 0.0;
#pragma unroll
                        for (int wv = 0; wv < kThreads / 64; ++wv) v += part[half + (wv * kChunk + tid) * NQ + q];
                        if (q < nrhs) publish(k0 + tid, q, v);
                    }
                }
            };
            for (int ch = 0; ch < nchunks; ch += 2) {
                step(fs[0], ch);
                if (ch + 1 < nchunks) step(fs[1], ch + 1);
            }
        }
    }
    ONESTAMP(4);
}

// The backward counterpart: block column p, taken by ticket from the root down (the forward order reversed), needs the x
// of every row below its columns -- the later columns of its supernode and rows of ancestors: all of them owned by
// blocks with earlier tickets --, written once each: x itself is the hand-off (y: n values per right-hand side, armed).
//     t = y_blk - L(below, blk)' x(below),   x_blk = inv(L_bb)' t
// Before it polls, the block has its panel below in LDS and the inverse of its diagonal block (as k_solve_one); after the
// last x arrives there are two LDS matrix-vector products.  The first version ran k_bsolve_block's loops (blocked
// substitution, rows below streamed from memory after the wait): ex15-class 0.086 ms.
template <int NQ>
__global__ __launch_bounds__(kThreads) void k_bsolve_one(const SnDesc* __restrict__ blocks, const int32_t* __restrict__ rows,
                                                         const int32_t* __restrict__ blk_w0, const double* __restrict__ L,
                                                         double* __restrict__ x, int nrhs, int ldx, int n, int nblocks,
                                                         double* y, double* __restrict__ y_next,
                                                         int* __restrict__ state, int* __restrict__ state_next,
                                                         int wait_bias, int cap) {
    // (y: other workgroups publish into it while this one reads: no __restrict__, every read of it is an atomic load)
    __shared__ double Dg[kTile * kLdDiag];  // the diagonal block (column-major), then its inverse in place; at the end: parts
    __shared__ double invd[kTile];
    __shared__ double s_t[16 * 17];
    __shared__ double s_m[kTile / 16][16 * 17];
    __shared__ double s_b[kTile][NQ];       // y_blk, then t
    __shared__ double s_xb[kOneRows][NQ];   // x of the rows below
    __shared__ double s_pan[OneStage<NQ>::bwd + kTile];   // the rows below the block's columns, [c][k - w] (row stride nb | 1; a larger
                                                  // panel: its first 64 rows, stride 65)
    __shared__ int s_task;
    static_assert(4 * kTile * 8 <= kTile * kLdDiag, "the products' parts reuse Dg");
    const int tid = threadIdx.x;
    if (tid == 0) s_task = atomicAdd(&state[1], 1);
    __syncthreads();
    const int t = nblocks - 1 - s_task;     // (the forward order reversed)
    const SnDesc D = blocks[t];
    const int w = D.w, nb = D.r - w, ldp = nb | 1, ld = D.ld;
    const double* __restrict__ G = L + D.px;
    // row k >= w of the block's window: a later column of its supernode (the first w0 - w rows below) or lR
    const int w_left = blk_w0[t];           // columns of the supernode from this block's first one on
    const int32_t* __restrict__ ri = rows + D.pi;
    one_arm_next(y_next, state_next, n, D.c0, w, s_task, tid, cap);
    for (int e = tid; e < kTile * NQ; e += kThreads) {
        const int q = e / kTile, c = e - q * kTile;
        s_b[c][q] = (c < w && q < nrhs) ? x[(int64_t)q * ldx + D.c0 + c] : 0.0;
    }
    const bool staged = nb <= kOneRows && w * ldp <= OneStage<NQ>::bwd;   // the panel below and the x of its rows fit in LDS
    if (staged)
        for (int e = tid; e < w * nb; e += kThreads) {
            const int c = e / nb, k = e - c * nb;
            s_pan[c * ldp + k] = G[(int64_t)c * ld + w + k];
        }
    // A larger panel: its first 64 rows -- in a wide supernode the next block column, whose x arrives last -- in LDS all the
    // same; the rows after them in chunks of kOneRows, the farthest first (their x has been there for long): wave v takes
    // the columns v, v + 4, ..., lane l the rows l, l + 64, ... of a chunk -- 64 values of L per lane, in REGISTERS; the
    // first chunk's are asked for here, before the polls
    const int near = staged ? nb : min(nb, kTile), ldn = kTile + 1;
    if (!staged)
        for (int e = tid; e < w * near; e += kThreads) {
            const int c = e / near, k = e - c * near;
            s_pan[c * ldn + k] = G[(int64_t)c * ld + w + k];
        }
    const int wave = tid >> 6, lane = tid & 63;
    // (chunks of kOneRows / 2 rows, two register sets: the loads of the chunk after are in flight while one is multiplied)
    constexpr int kChunk = kOneRows / 2, kPc = kTile / (kThreads / 64), kPr = kChunk / 64;   // columns per wave, rows per lane
    double pre[2][kPc][kPr];
    auto preload = [&](double (&dst)[kPc][kPr], int k0) {
#pragma unroll
        for (int ci = 0; ci < kPc; ++ci) {
            const double* __restrict__ col = G + (int64_t)min(wave + (kThreads / 64) * ci, w - 1) * ld + w;
#pragma unroll
            for (int j = 0; j < kPr; ++j) dst[ci][j] = col[min(k0 + lane + 64 * j, nb - 1)];
        }
    };
    const int nfar = nb - near, nchunks = (nfar + kChunk - 1) / kChunk;   // (0 when staged)
    if (nchunks > 0) preload(pre[0], near + (nchunks - 1) * kChunk);
    const int wpad = (w + 15) & ~15;
    for (int e = tid; e < wpad * wpad; e += kThreads) {
        const int c = e / wpad, i = e - c * wpad;
        double v = (i == c) ? 1.0 : 0.0;
        if (i >= c && i < w && c < w) v = G[(int64_t)c * ld + i];
        Dg[c * kLdDiag + i] = v;
    }
    __syncthreads();
    one_invert_block(Dg, invd, s_t, s_m, w, wpad, tid);   // (ends synchronised)
    auto m_at = [&](int c, int k) {   // M[c][k], k <= c
        const int b = c & ~15;
        return k >= b ? s_m[b >> 4][(c - b) * 17 + (k - b)] : Dg[k * kLdDiag + c];
    };
    bool ok = true;
    // the x of (a chunk of) the rows below: one row per thread and right-hand side, all polls in flight together
    auto gather = [&](int k0, int len) {
        for (int k = tid; k < len; k += kThreads) {
            const int row = w + k0 + k < w_left ? D.c0 + w + k0 + k : ri[w + k0 + k];
            double v[NQ];
            one_poll_n<NQ>(&y[row], n, nrhs, v, state, wait_bias, ok);
#pragma unroll
            for (int q = 0; q < NQ; ++q) s_xb[k][q] = v[q];
        }
    };
    // far chunks, the farthest first; step i uses register set i & 1 and the half i & 1 of s_xb, and asks for the chunk
    // after it -- its part of L and, with a PLAIN load, its x -- before it multiplies (one barrier per chunk: the half
    // written next was read two steps ago).  The plain load is the fast path: far rows were published long ago and the
    // line is in the L2 for every block that reads it; it can only see the armed pattern too early (a line cached before
    // the value was stored: values of earlier solves do not survive the launch boundary), and then the poll takes over.
    double xv[2][NQ];
    double facc[kPc];
#pragma unroll
    for (int ci = 0; ci < kPc; ++ci) facc[ci] = 0.0;
    auto x_ahead = [&](double (&dst)[NQ], int ch) {
        const int k0 = near + ch * kChunk, k = min(k0 + (tid & (kChunk - 1)), nb - 1);
        const int row = w + k < w_left ? D.c0 + w + k : ri[w + k];
#pragma unroll
        for (int q = 0; q < NQ; ++q)   // (a relaxed load of wavefront scope: the same cached load, defined beside the publishers' stores)
            dst[q] = q < nrhs ? __hip_atomic_load(&y[(int64_t)q * n + row], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT) : 0.0;
    };
    if (nchunks > 0) x_ahead(xv[0], nchunks - 1);
    auto far_step = [&](double (&cur)[kPc][kPr], double (&nxt)[kPc][kPr], double (&xc)[NQ], double (&xn)[NQ], int step) {
        const int ch = nchunks - 1 - step, k0 = near + ch * kChunk, len = min(kChunk, nb - k0), half = (step & 1) * kChunk;
        if (ch > 0) {
            preload(nxt, near + (ch - 1) * kChunk);
            x_ahead(xn, ch - 1);
        }
        if (tid < len) {
            const int row = w + k0 + tid < w_left ? D.c0 + w + k0 + tid : ri[w + k0 + tid];
#pragma unroll
            for (int q = 0; q < NQ; ++q) {
                double v = xc[q];
                if (q < nrhs && __double_as_longlong(v) == kXArmed) v = one_poll(&y[(int64_t)q * n + row], state, wait_bias, ok);
                s_xb[half + tid][q] = v;
            }
        }
        __syncthreads();
#pragma unroll
        for (int ci = 0; ci < kPc; ++ci) {
            const int c = wave + (kThreads / 64) * ci;
            double acc[NQ];
#pragma unroll
            for (int q = 0; q < NQ; ++q) acc[q] = 0.0;
#pragma unroll
            for (int j = 0; j < kPr; ++j) {
                const int k = lane + 64 * j;
                if (k < len) {
#pragma unroll
                    for (int q = 0; q < NQ; ++q) acc[q] = fma(cur[ci][j], s_xb[half + k][q], acc[q]);
                }
            }
            if (NQ == 1) {
                facc[ci] += acc[0];   // (one right-hand side: the lanes' parts are added up once, after the last chunk)
            } else {
#pragma unroll
                for (int q = 0; q < NQ; ++q) {
#pragma unroll
                    for (int o = 32; o >= 1; o >>= 1) acc[q] += __shfl_xor(acc[q], o);
                }
                if (lane == 0 && c < w) {
#pragma unroll
                    for (int q = 0; q < NQ; ++q) s_b[c][q] -= acc[q];   // (column c belongs to this wave alone)
                }
            }
        }
    };
    for (int step = 0; step < nchunks; step += 2) {
        far_step(pre[0], pre[1], xv[0], xv[1], step);
        if (step + 1 < nchunks) far_step(pre[1], pre[0], xv[1], xv[0], step + 1);
    }
    if (NQ == 1 && nchunks > 0) {
#pragma unroll
        for (int ci = 0; ci < kPc; ++ci) {
            double v = facc[ci];
#pragma unroll
            for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
            const int c = wave + (kThreads / 64) * ci;
            if (lane == 0 && c < w) s_b[c][0] -= v;
        }
    }
    if (near > 0) {
        // ---- the rows in LDS (all of a small panel): t = y_blk - panel' x(below), four lanes per column share the sum
        if (nchunks > 0) __syncthreads();
        gather(0, near);
        __syncthreads();
        const int c = tid >> 2, part = tid & 3, ldl = staged ? ldp : ldn;
        double acc[NQ];
#pragma unroll
        for (int q = 0; q < NQ; ++q) acc[q] = 0.0;
        if (c < w)
            for (int k = part; k < near; k += 4) {
                const double lv = s_pan[c * ldl + k];
#pragma unroll
                for (int q = 0; q < NQ; ++q) acc[q] = fma(lv, s_xb[k][q], acc[q]);
            }
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            acc[q] += __shfl_xor(acc[q], 1);
            acc[q] += __shfl_xor(acc[q], 2);
        }
        if (part == 0 && c < w) {
#pragma unroll
            for (int q = 0; q < NQ; ++q) s_b[c][q] -= acc[q];
        }
    }
    __syncthreads();
    // ---- x = inv(L_bb)' t: x[c] = sum_{k >= c} M[k][c] t[k]; four lanes per column
    {
        const int c = tid >> 2, part = tid & 3;
        double acc[NQ];
#pragma unroll
        for (int q = 0; q < NQ; ++q) acc[q] = 0.0;
        if (c < w)
            for (int k = c + part; k < w; k += 4) {
                const double iv = m_at(k, c);
#pragma unroll
                for (int q = 0; q < NQ; ++q) acc[q] = fma(iv, s_b[k][q], acc[q]);
            }
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            acc[q] += __shfl_xor(acc[q], 1);
            acc[q] += __shfl_xor(acc[q], 2);
        }
        if (part == 0 && c < w) {
#pragma unroll
            for (int q = 0; q < NQ; ++q)
                if (q < nrhs) {
                    __hip_atomic_store(&y[(int64_t)q * n + D.c0 + c], unarmed(acc[q]), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    x[(int64_t)q * ldx + D.c0 + c] = acc[q];
                }
        }
    }
}

void launch_solve_one(const DevicePattern& P, WitnessKernel k, const double* L, double* x, int nrhs, int ldx, double* y, double* y_next,
                      int* state, int* state_next, int wait_bias, int cap, hipStream_t stream) {
    const DevicePattern::OneDev& O = P.one_f;
    if (O.nblocks <= 0) return;
#define PARSY_ONE_ARGS                                                                                                  \
    dim3(O.nblocks), dim3(kThreads), 0, stream, O.sn, O.slot0, O.pull_ptr, O.pull_slot, O.pull_pos, L, x, nrhs, ldx, O.nslots, \
        y, y_next, state, state_next, wait_bias, cap
    if (k == kWSolveOne1) launch_witnessed<k_solve_one<1>, kWSolveOne1>(PARSY_ONE_ARGS);
    else if (k == kWSolveOne4) launch_witnessed<k_solve_one<4>, kWSolveOne4>(PARSY_ONE_ARGS);
    else if (k == kWSolveOne8) launch_witnessed<k_solve_one<8>, kWSolveOne8>(PARSY_ONE_ARGS);
    else launch_refused("launch_solve_one", k);
#undef PARSY_ONE_ARGS
}

#ifdef PARSY_ONESTAMPS
extern "C" void parsy_debug_onestamps(unsigned long long* out) {
    (void)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_onestamp), sizeof(unsigned long long) * 4096 * 8);
}
#endif

void launch_bsolve_one(const DevicePattern& P, WitnessKernel k, int n, const double* L, double* x, int nrhs, int ldx, double* y, double* y_next,
                       int* state, int* state_next, int wait_bias, int cap, hipStream_t stream) {
    const DevicePattern::OneDev& O = P.one_b;
    if (O.nblocks <= 0) return;
#define PARSY_ONE_ARGS                                                                                                  \
    dim3(O.nblocks), dim3(kThreads), 0, stream, O.sn, P.rows, O.wleft, L, x, nrhs, ldx, n, O.nblocks, y, y_next, state,        \
        state_next, wait_bias, cap
    if (k == kWBsolveOne1) launch_witnessed<k_bsolve_one<1>, kWBsolveOne1>(PARSY_ONE_ARGS);
    else if (k == kWBsolveOne4) launch_witnessed<k_bsolve_one<4>, kWBsolveOne4>(PARSY_ONE_ARGS);
    else if (k == kWBsolveOne8) launch_witnessed<k_bsolve_one<8>, kWBsolveOne8>(PARSY_ONE_ARGS);
    else launch_refused("launch_bsolve_one", k);
#undef PARSY_ONE_ARGS
}

// SOLVE_FIXUP: solved blocks of the wide supernodes go from scratch into x.
__global__ __launch_bounds__(kThreads) void k_solve_fixup(const SnDesc* __restrict__ sn,
                                                          const int32_t* __restrict__ list,
                                                          double* __restrict__ x,
                                                          const double* __restrict__ xscratch,
                                                          int nrhs, int ldx) {
    const SnDesc D = sn[list[blockIdx.x]];
    for (int q = blockIdx.y; q < nrhs; q += gridDim.y)
        for (int c = threadIdx.x; c < D.w; c += kThreads)
            x[(int64_t)q * ldx + D.c0 + c] = xscratch[(int64_t)q * ldx + D.c0 + c];
}

void launch_solve_fixup(const DevicePattern& P, int first, int count, double* x,
                        const double* xscratch, int nrhs, int ldx, hipStream_t stream) {
    if (count <= 0) return;
    launch_witnessed<k_solve_fixup, kWSolveFixup>(dim3(count, min(nrhs, 64)), dim3(kThreads), 0, stream, P.sn,
        P.solve_fix_list + first, x, xscratch, nrhs, ldx);
}

}  // namespace parsy
