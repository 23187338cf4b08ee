// HIP kernels of the level-scheduled backward solve L' X = Y for gfx950.
// (Numeric contract: trsv_kernels.hip; what the solve sources share: trsv_device.hpp.)
#include <hip/hip_runtime.h>

#include <algorithm>

#include "launch.hpp"
#include "trsv_device.hpp"

namespace parsy {

// ---------------------------------------------------------------------------
// Backward solve L' x = y (the reference only has the forward solve;
// with this the library solves A x = b end to end).  Pull form, no atomics: a block of <= 64
// columns [cb, cb+wbk) of a supernode is finished by one workgroup once every row below it
// is final (ancestors' columns: earlier levels; later block columns of the same supernode:
// earlier launches):   t = y_blk - L(below, blk)' x(below),   x_blk = inv(L_bb)' t.
// The product runs one wave per column with lanes along the (contiguous) rows.
// ---------------------------------------------------------------------------
static constexpr int kLdRedB = 65;   // row stride of a wave's reduction buffer (doubles): conflict-free both ways
template <int NQ>
__global__ __launch_bounds__(kThreads) void k_bsolve_block(const SnDesc* __restrict__ sn,
                                                           const PanelDesc* __restrict__ pds,
                                                           const int32_t* __restrict__ rows,
                                                           const double* __restrict__ L,
                                                           double* __restrict__ x, double* __restrict__ xscratch,
                                                           int nrhs, int ldx, int chain, int* __restrict__ info,
                                                           int* __restrict__ ticket, int wait_bias, int nblocks,
                                                           const int32_t* __restrict__ ranges,
                                                           const double* __restrict__ dinv) {
    // chain != 0: every block column of the wide supernodes of a level is in this launch; block jb takes the x
    // of blocks jb+1.. of its supernode as they are published: as the data itself, through the armed buffer
    // (xscratch: 8-byte agent-scope atomics both sides, a value is valid once it differs from kXArmed -- see
    // k_solve_chain_w), and finishes with a product with the inverse diagonal block (DIAG_INVERSE).
    // ranges != null (subtree launch, chain == 0): task b is the run pds[ranges[2b] .. ranges[2b+1]) -- a subtree
    // of single-block supernodes from its root down; the workgroup reads its own earlier x (same CU, plain
    // stores and loads ordered by the barrier between two supernodes).
    __shared__ double Dg[kTile * kLdDiag];
    __shared__ double invd[kTile];
    __shared__ double ts[kTile][NQ];
    __shared__ double s_red[kThreads / 64][(kTile / 4) * kLdRedB];   // per wave: the lanes' parts of its 16 column sums
    __shared__ int s_task;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    // chain launch: blocks are listed last block column first (producers first) and taken by ticket
    if (tid == 0) s_task = chain ? atomicAdd(ticket, 1) : (int)(blockIdx.x + blockIdx.y * nblocks);
    __syncthreads();
    // every block once per pass lane: tasks 0..nblocks-1 are lane 0, and so on
    const int plane = s_task / nblocks;
    const int task = s_task - plane * nblocks;
    const int q_begin = ranges ? ranges[2 * task] : task;
    const int q_end = ranges ? ranges[2 * task + 1] : q_begin + 1;
  for (int qsn = q_begin; qsn < q_end; ++qsn) {
    if (qsn > q_begin) __syncthreads();  // the x of the supernode before is stored; Dg / ts are free again
    const PanelDesc pd = pds[qsn];
    const SnDesc D = sn[pd.sn];
    const int r = D.r, w = D.w, cb = pd.jb * kTile, wbk = min(kTile, w - cb);
    const double* __restrict__ G = L + D.px;
    const int32_t* __restrict__ ri = rows + D.pi;
    const int kbeg = cb + wbk;  // first panel row below the block

    {   // diagonal block (identity padded) -> LDS; chain launch: its inverse instead (same layout)
        double dtmp[kTile * kTile / kThreads];
        const double* __restrict__ inv_blk = chain ? dinv + (int64_t)(D.dslot + pd.jb) * (kTile * kTile) : nullptr;
#pragma unroll
        for (int t = 0; t < kTile * kTile / kThreads; ++t) {
            const int e = t * kThreads + tid;
            const int c = e >> 6, i = e & 63;
            double v = (i == c) ? 1.0 : 0.0;
            if (chain) v = inv_blk[e];
            else if (c < wbk && i < wbk && i >= c) v = G[(int64_t)(cb + c) * r + cb + i];
            dtmp[t] = v;
        }
#pragma unroll
        for (int t = 0; t < kTile * kTile / kThreads; ++t) {
            const int e = t * kThreads + tid;
            Dg[(e >> 6) * kLdDiag + (e & 63)] = dtmp[t];
        }
    }
    __syncthreads();
    // inverses of the 16x16 diagonal sub-blocks (stored transposed in the strict upper triangle)
    if (!chain && tid < kTile) invd[tid] = 1.0 / Dg[tid * kLdDiag + tid];
    __syncthreads();
    if (!chain && tid < kTile && (tid & ~15) < wbk) {
        const int b16 = tid & ~15, c = tid & 15;
        double y[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) y[k] = (k == c) ? invd[b16 + k] : 0.0;
#pragma unroll
        for (int rr = 1; rr < 16; ++rr) {
            double sacc = 0.0;
#pragma unroll
            for (int k = 0; k < rr; ++k) sacc = fma(Dg[(b16 + k) * kLdDiag + b16 + rr], y[k], sacc);
            y[rr] = (rr > c) ? -sacc * invd[b16 + rr] : y[rr];
        }
        __builtin_amdgcn_s_waitcnt(0);
#pragma unroll
        for (int rr = 1; rr < 16; ++rr)
            if (rr > c) Dg[(b16 + rr) * kLdDiag + b16 + c] = y[rr];
    }

    const int nbc = (w + kTile - 1) / kTile;
    for (int pass = plane; pass * NQ < nrhs; pass += kPassLanes) {
        const int q0 = pass * NQ;
        const int nq = min(NQ, nrhs - q0);
        __syncthreads();
        for (int e = tid; e < kTile * NQ; e += kThreads) {
            const int c = e & 63, q = e >> 6;
            ts[c][q] = (c < wbk && q < nq) ? x[(int64_t)(q0 + q) * ldx + D.c0 + cb + c] : 0.0;
        }
        __syncthreads();
        // t[c] -= sum_k L[k, cb+c] x[row(k)]: wave `wave` takes columns wave, wave+4, ...
        {
            double acc[kTile / 4][NQ];
#pragma unroll
            for (int ci = 0; ci < kTile / 4; ++ci)
#pragma unroll
                for (int q = 0; q < NQ; ++q) acc[ci][q] = 0.0;
            // rows below the supernode's own columns (ancestors: final before this launch); without
            // the chain also the rows of the later blocks (solved by earlier launches)
            // (kBackUnroll row chunks per trip, every load of a trip issued before its products: the row ids, the
            // x they point to and the wave's 16 columns of L are three dependent-latency phases otherwise)
            constexpr int kBackUnroll = NQ == 1 ? 4 : 2;
            for (int k0 = (chain ? w : kbeg) + lane; k0 < r; k0 += 64 * kBackUnroll) {
                int xr[kBackUnroll];
                double lv[kBackUnroll][kTile / 4];
#pragma unroll
                for (int u = 0; u < kBackUnroll; ++u) {
                    const int k = min(k0 + 64 * u, r - 1);   // (clamped: the chunks past the panel multiply by zero)
                    xr[u] = (k < w) ? (D.c0 + k) : ri[k];
#pragma unroll
                    for (int ci = 0; ci < kTile / 4; ++ci) {
                        const int c = min(wave + 4 * ci, wbk - 1);
                        lv[u][ci] = G[(int64_t)(cb + c) * r + k];
                    }
                }
#pragma unroll
                for (int u = 0; u < kBackUnroll; ++u) {
                    double xk[NQ];
#pragma unroll
                    for (int q = 0; q < NQ; ++q)
                        xk[q] = (q < nq && k0 + 64 * u < r) ? x[(int64_t)(q0 + q) * ldx + xr[u]] : 0.0;
#pragma unroll
                    for (int ci = 0; ci < kTile / 4; ++ci) {
                        const double lvv = (wave + 4 * ci < wbk) ? lv[u][ci] : 0.0;
#pragma unroll
                        for (int q = 0; q < NQ; ++q) acc[ci][q] = fma(lvv, xk[q], acc[ci][q]);
                    }
                }
            }
            if (chain) {
                // the later blocks of this supernode, last one first, each as soon as it is published
                for (int I = nbc - 1; I > pd.jb; --I) {
                    // this lane's row of block I against the wave's 16 columns: loaded BEFORE the wait
                    const int k = I * kTile + lane;
                    double lv[kTile / 4];
#pragma unroll
                    for (int ci = 0; ci < kTile / 4; ++ci) {
                        const int c = wave + 4 * ci;
                        lv[ci] = (c < wbk && k < w) ? G[(int64_t)(cb + c) * r + k] : 0.0;
                    }
                    // x of block I: every lane polls its own row's values (the data is the flag); bounded, and
                    // one timeout (status word) ends every wait of the solve
                    BoundedWait wait;
                    bool ok = true;
                    double xk[NQ];
                    for (;;) {
                        bool in = true;
#pragma unroll
                        for (int q = 0; q < NQ; ++q) {
                            long long b = 0;
                            if (q < nq && k < w)
                                b = __hip_atomic_load(reinterpret_cast<const long long*>(
                                                          &xscratch[(int64_t)(q0 + q) * ldx + D.c0 + k]),
                                                      __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                            in = in && b != kXArmed;
                            xk[q] = __longlong_as_double(b);
                        }
                        if (__all(in && wait_bias == 0)) break;
                        if (wait.expired(info)) {
                            ok = false;
                            break;
                        }
                        __builtin_amdgcn_s_sleep(1);
                    }
                    if (!ok) {
                        if (lane == 0) wait_failed(info);
                        break;  // (the result is wrong and reported; nobody may hang)
                    }
                    {
#pragma unroll
                        for (int ci = 0; ci < kTile / 4; ++ci)
#pragma unroll
                            for (int q = 0; q < NQ; ++q) acc[ci][q] = fma(lv[ci], xk[q], acc[ci][q]);
                    }
                }
            }
            // column sums across the wave through LDS (as k_bsolve_chain_w: the lanes park their 16 parts, lane
            // (ci, g) adds up 16 of them, two exchanges finish the column), one right-hand side after the other
#pragma unroll
            for (int q = 0; q < NQ; ++q) {
                double* __restrict__ red = s_red[wave];
                __builtin_amdgcn_wave_barrier();   // (the parts of the right-hand side before are consumed)
#pragma unroll
                for (int ci = 0; ci < kTile / 4; ++ci) red[ci * kLdRedB + lane] = acc[ci][q];
                __builtin_amdgcn_wave_barrier();
                const int ci = lane & 15, g = lane >> 4;
                double v0 = 0.0, v1 = 0.0;
#pragma unroll
                for (int i = 0; i < 16; i += 2) {
                    v0 += red[ci * kLdRedB + 16 * g + i];
                    v1 += red[ci * kLdRedB + 16 * g + i + 1];
                }
                double v = v0 + v1;
                v += __shfl_xor(v, 16);
                v += __shfl_xor(v, 32);
                if (g == 0) ts[wave + 4 * ci][q] -= v;  // each (column, q) has one writer
            }
        }
        __syncthreads();
        if (chain) {
            // x_blk = inv(L_bb)' t as a product: x_c = sum_{k >= c} inv(L_bb)[k][c] t_k (column c of the inverse is
            // contiguous in LDS)
            double zv[(kTile * NQ + kThreads - 1) / kThreads];
#pragma unroll
            for (int u = 0; u < (kTile * NQ + kThreads - 1) / kThreads; ++u) {
                const int e = u * kThreads + tid, c = e & 63, q = e >> 6;
                double s0 = 0.0, s1 = 0.0;
                if (e < kTile * NQ && q < nq) {
                    for (int k = c; k + 1 < kTile; k += 2) {
                        s0 = fma(Dg[c * kLdDiag + k], ts[k][q], s0);
                        s1 = fma(Dg[c * kLdDiag + k + 1], ts[k + 1][q], s1);
                    }
                    if (((kTile - c) & 1) != 0) s0 = fma(Dg[c * kLdDiag + kTile - 1], ts[kTile - 1][q], s0);
                }
                zv[u] = s0 + s1;
            }
            __syncthreads();
#pragma unroll
            for (int u = 0; u < (kTile * NQ + kThreads - 1) / kThreads; ++u) {
                const int e = u * kThreads + tid;
                if (e < kTile * NQ && (e >> 6) < nq) ts[e & 63][e >> 6] = zv[u];
            }
            __syncthreads();
        }
        // x_blk = inv(L_bb)' t, 16 columns at a time from the last sub-block up
        for (int b16 = chain ? -1 : ((wbk - 1) & ~15); b16 >= 0; b16 -= 16) {
            const int i = tid & 15, q = tid >> 4;
            const bool act = q < nq;
            double zv = 0.0;
            if (act) {
#pragma unroll
                for (int k = 0; k < 16; ++k) {
                    double lv = 0.0;  // inv(L_bb)'[i][k] = inv(L_bb)[k][i]
                    if (k > i) lv = Dg[(b16 + k) * kLdDiag + b16 + i];
                    else if (k == i) lv = invd[b16 + i];
                    zv = fma(lv, ts[b16 + k][q], zv);
                }
            }
            __syncthreads();
            if (act) ts[b16 + i][q] = zv;
            __syncthreads();
            // columns above the sub-block: t[a] -= sum_k L[b16+k][a] z[k]
            for (int e = tid; e < b16 * nq; e += kThreads) {
                const int qq = e / b16, a2 = e - qq * b16;
                double accv = ts[a2][qq];
#pragma unroll
                for (int k = 0; k < 16; ++k) accv = fma(-Dg[a2 * kLdDiag + b16 + k], ts[b16 + k][qq], accv);
                ts[a2][qq] = accv;
            }
            __syncthreads();
        }
        for (int e = tid; e < wbk * nq; e += kThreads) {
            const int q = e / wbk, c = e - q * wbk;
            x[(int64_t)(q0 + q) * ldx + D.c0 + cb + c] = ts[c][q];
            if (chain)
                __hip_atomic_store(&xscratch[(int64_t)(q0 + q) * ldx + D.c0 + cb + c], unarmed(ts[c][q]), __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_AGENT);
        }
        // (chain launch: nothing else to do -- the values stored in the armed buffer are the publication)
    }
  }
}

// ---------------------------------------------------------------------------
// Backward solve, many right-hand sides (from mrhs_min() on): the counterpart of k_solve_small_mrhs /
// k_solve_blocks_mrhs -- 64 right-hand sides per pass over L instead of 4, every product on the matrix cores.
// One workgroup (4 waves) per block of <= 64 columns, as k_bsolve_block:
//     T = Y_blk - L(below, blk)' X(below)        (64 columns x 64 right-hand sides)
// with the panel ROWS as the contraction index of v_mfma_f64_16x16x4_f64: lane (c, kk) holds L[k0 + kk][cb + c]
// (A operand: 16 columns x 4 consecutive rows -- 32-byte runs of 16 panel columns per load, every 128-byte line is
// used up by four consecutive k steps) and lane (kk, q) holds X[row(k0 + kk)][q] (B operand, gathered through the
// row ids).  The 64-row chunks below the block are dealt over the four waves, each keeps all 16 tiles of T (128
// accumulator registers; one workgroup per CU); chain launches then take the later blocks of the supernode as their
// X is published (armed buffer: the data is the flag), 16 rows per wave.  The waves' parts are subtracted from the
// staged Y one after the other (fixed order: reproducible), then X_blk = inv(L_bb)' T -- chain launches: a product
// with the inverse diagonal block (DIAG_INVERSE) on the matrix cores; otherwise the blocked substitution of
// k_bsolve_block.  Reference: the backward solve is an extension; the forward kernel it mirrors
// replaces Triangular_BCSC.h:139-157.
// ---------------------------------------------------------------------------
#define TSM(c, q) ts[(c) * kLdXm + (q)]
template <int QG>   // 16-right-hand-side groups per pass: 4 (64 per pass over L) or 1 (small launches: more workgroups)
__global__ __launch_bounds__(kThreads, QG == 4 ? 1 : 2) void k_bsolve_block_mrhs(const SnDesc* __restrict__ sn,
                                                                   const PanelDesc* __restrict__ pds,
                                                                   const int32_t* __restrict__ rows,
                                                                   const double* __restrict__ L,
                                                                   double* __restrict__ x, double* __restrict__ xscratch,
                                                                   int nrhs, int ldx, int chain, int* __restrict__ info,
                                                                   int* __restrict__ ticket, int wait_bias, int nblocks,
                                                                   const int32_t* __restrict__ ranges,
                                                                   const double* __restrict__ dinv) {
    __shared__ double Dg[kTile * kLdDiag];
    __shared__ double invd[kTile];
    __shared__ double ts[kTile * kLdXm];
    __shared__ int s_task;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, l15 = lane & 15, kq = lane >> 4;
    if (tid == 0) s_task = chain ? atomicAdd(ticket, 1) : (int)(blockIdx.x + blockIdx.y * nblocks);
    __syncthreads();
    const int plane = s_task / nblocks;
    const int task = s_task - plane * nblocks;
    const int q_begin = ranges ? ranges[2 * task] : task;
    const int q_end = ranges ? ranges[2 * task + 1] : q_begin + 1;
  for (int qsn = q_begin; qsn < q_end; ++qsn) {
    if (qsn > q_begin) __syncthreads();
    const PanelDesc pd = pds[qsn];
    const SnDesc D = sn[pd.sn];
    const int r = D.r, w = D.w, cb = pd.jb * kTile, wbk = min(kTile, w - cb);
    const double* __restrict__ G = L + D.px;
    const int32_t* __restrict__ ri = rows + D.pi;
    const int kbeg = cb + wbk;
    {   // diagonal block (identity padded) -> LDS; chain launch: its inverse instead (same layout)
        double dtmp[kTile * kTile / kThreads];
        const double* __restrict__ inv_blk = chain ? dinv + (int64_t)(D.dslot + pd.jb) * (kTile * kTile) : nullptr;
#pragma unroll
        for (int t = 0; t < kTile * kTile / kThreads; ++t) {
            const int e = t * kThreads + tid;
            const int c = e >> 6, i = e & 63;
            double v = (i == c) ? 1.0 : 0.0;
            if (chain) v = inv_blk[e];
            else if (c < wbk && i < wbk && i >= c) v = G[(int64_t)(cb + c) * r + cb + i];
            dtmp[t] = v;
        }
#pragma unroll
        for (int t = 0; t < kTile * kTile / kThreads; ++t) {
            const int e = t * kThreads + tid;
            Dg[(e >> 6) * kLdDiag + (e & 63)] = dtmp[t];
        }
    }
    __syncthreads();
    if (!chain && tid < kTile) invd[tid] = 1.0 / Dg[tid * kLdDiag + tid];
    __syncthreads();
    if (!chain && tid < kTile && (tid & ~15) < wbk) {   // inverses of the 16x16 diagonal sub-blocks (as k_bsolve_block)
        const int b16 = tid & ~15, c = tid & 15;
        double y[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) y[k] = (k == c) ? invd[b16 + k] : 0.0;
#pragma unroll
        for (int rr = 1; rr < 16; ++rr) {
            double sacc = 0.0;
#pragma unroll
            for (int k = 0; k < rr; ++k) sacc = fma(Dg[(b16 + k) * kLdDiag + b16 + rr], y[k], sacc);
            y[rr] = (rr > c) ? -sacc * invd[b16 + rr] : y[rr];
        }
        __builtin_amdgcn_s_waitcnt(0);
#pragma unroll
        for (int rr = 1; rr < 16; ++rr)
            if (rr > c) Dg[(b16 + rr) * kLdDiag + b16 + c] = y[rr];
    }
    const int nbc = (w + kTile - 1) / kTile;
    constexpr int kPassRhs = 16 * QG;
    for (int pass = plane; pass * kPassRhs < nrhs; pass += kPassLanes) {
        const int q0 = pass * kPassRhs;
        const int nq = min(kPassRhs, nrhs - q0);
        __syncthreads();
        for (int e = tid; e < kTile * kPassRhs; e += kThreads) {
            const int c = e & 63, q = e >> 6;
            TSM(c, q) = (c < wbk && q < nq) ? x[(int64_t)(q0 + q) * ldx + D.c0 + cb + c] : 0.0;
        }
        double4_t acc[4][QG];   // [16 columns][16 right-hand sides]: lane (q = l15, c = kq + 4 v)
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int b = 0; b < QG; ++b) acc[a][b] = double4_t{0, 0, 0, 0};
        // operand pointers of this lane: column c = 16 cg + l15 of the block (clamped), right-hand side 16 qg + l15
        const double* __restrict__ acol[4];
        const double* __restrict__ xcol[QG];
        bool aok[4], bok[QG];
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            aok[g] = 16 * g + l15 < wbk;
            acol[g] = G + (int64_t)(cb + min(16 * g + l15, wbk - 1)) * r;
        }
#pragma unroll
        for (int g = 0; g < QG; ++g) {
            bok[g] = 16 * g + l15 < nq;
            xcol[g] = x + (int64_t)(q0 + min(16 * g + l15, nq - 1)) * ldx;
        }
        // ---- the rows below (chain: below the supernode's own columns -- ancestors, final; otherwise everything
        // below the block: the later blocks were solved by earlier launches): 64-row chunks over the waves, 16 rows
        // (4 k steps) of loads in flight ahead of their 64 products
        // Software-pipelined over the k steps (4 rows each) of all of this wave's chunks: the operands of step t + 3 are
        // loaded while the 4 x QG products of step t are issued (a ring of four operand sets); the row ids of a chunk are
        // ONE load per lane, issued a chunk and a half ahead and handed to the lanes that need them by ds_bpermute.
        // (The plain form -- ids, then operands, then 64 products, per 16 rows -- waited two dependent round trips per 64
        // products: Flan-class input, 64 right-hand sides: 45 -> 37 ms per backward solve.)
        {
            const int kstart = (chain ? w : kbeg) + 64 * wave;
            constexpr int kStride = 64 * (kThreads / 64);
            const int nsteps = kstart < r ? 16 * ((r - kstart + kStride - 1) / kStride) : 0;
            auto row_ids = [&](int j) {   // lane l: the row id of row l of this wave's chunk j (clamped into the panel)
                const int kr = min(kstart + kStride * j + lane, r - 1);
                return (kr < w) ? (D.c0 + kr) : ri[kr];
            };
            int ridA = row_ids(0), ridB = row_ids(1);
            double ra[4][4], rb[4][QG];
            auto load = [&](int t, double (&A)[4], double (&B)[QG]) {
                const int j = t >> 4, u = t & 15;
                const int k = kstart + kStride * j + 4 * u + kq;
                const bool kin = k < r && t < nsteps;
                const int kc = min(k, r - 1);
                const int rid = __builtin_amdgcn_ds_bpermute((4 * u + kq) * 4, (j & 1) ? ridB : ridA);
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const double a = acol[g][kc];
                    A[g] = (kin && aok[g]) ? a : 0.0;
                }
#pragma unroll
                for (int g = 0; g < QG; ++g) {
                    const double b2 = xcol[g][rid];
                    B[g] = (kin && bok[g]) ? b2 : 0.0;
                }
            };
            if (nsteps > 0) {
#pragma unroll
                for (int t = 0; t < 3; ++t) load(t, ra[t], rb[t]);
            }
            for (int t = 0; t < nsteps; t += 4) {
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int tt = t + i;
                    load(tt + 3, ra[(i + 3) & 3], rb[(i + 3) & 3]);
#pragma unroll
                    for (int cg = 0; cg < 4; ++cg)
#pragma unroll
                        for (int qg = 0; qg < QG; ++qg)
                            acc[cg][qg] = __builtin_amdgcn_mfma_f64_16x16x4f64(ra[i][cg], rb[i][qg], acc[cg][qg], 0, 0, 0);
                    if ((tt & 15) == 13) {   // the loads of this chunk's steps are all issued: its id register takes chunk j + 2
                        const int j = tt >> 4;
                        const int v = row_ids(j + 2);
                        if (j & 1) ridB = v;
                        else ridA = v;
                    }
                }
            }
        }
        if (chain) {
            // ---- the later blocks of this supernode, last one first, each as soon as its X is published: rows
            // 64 I + 16 wave .. + 15 for this wave
            bool ok = true;
            for (int I = nbc - 1; I > pd.jb && ok; --I) {
                double av[4][4], bv[4][QG];
                int kk[4];
#pragma unroll
                for (int st = 0; st < 4; ++st) {
                    kk[st] = I * kTile + 16 * wave + 4 * st + kq;
                    const int kc = min(kk[st], w - 1);
#pragma unroll
                    for (int g = 0; g < 4; ++g) {
                        const double a = acol[g][kc];
                        av[st][g] = (kk[st] < w && aok[g]) ? a : 0.0;
                    }
                }
                BoundedWait wait;   // (of the watch and the full poll together)
                // Only the block right above this one is on the critical path of the chain.  A workgroup further up
                // would poll for a long time, with 16 loads per lane and round, next to hundreds of others on the
                // same lines (the top separator: 313 workgroups): it first watches ONE value of the block lazily
                // (the last column this wave reads: one load per wave and round), and goes on to the full poll --
                // normally satisfied at once -- when that value is there.
                if (I - pd.jb > 1) {
                    const int kw = min(I * kTile + 16 * wave + 15, w - 1);
                    const long long* __restrict__ watch =
                        reinterpret_cast<const long long*>(xscratch + (int64_t)q0 * ldx + D.c0 + kw);
                    while (__hip_atomic_load(watch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == kXArmed ||
                           wait_bias != 0) {
                        if (wait.expired(info)) {
                            ok = false;
                            break;
                        }
                        __builtin_amdgcn_s_sleep(48);
                    }
                    if (!ok) {
                        if (lane == 0) wait_failed(info);
                        break;
                    }
                }
                for (;;) {
                    bool in = true;
#pragma unroll
                    for (int st = 0; st < 4; ++st)
#pragma unroll
                        for (int g = 0; g < QG; ++g) {
                            long long b = 0;
                            if (kk[st] < w && bok[g])
                                b = __hip_atomic_load(reinterpret_cast<const long long*>(
                                                          xscratch + (xcol[g] - x) + D.c0 + kk[st]),
                                                      __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                            in = in && b != kXArmed;
                            bv[st][g] = __longlong_as_double(b);
                        }
                    if (__all(in && wait_bias == 0)) break;
                    if (wait.expired(info)) {
                        ok = false;
                        break;
                    }
                    __builtin_amdgcn_s_sleep(1);
                }
                if (!ok) {
                    if (lane == 0) wait_failed(info);
                    break;   // (the result is wrong and reported; nobody may hang)
                }
#pragma unroll
                for (int st = 0; st < 4; ++st)
#pragma unroll
                    for (int cg = 0; cg < 4; ++cg)
#pragma unroll
                        for (int qg = 0; qg < QG; ++qg)
                            acc[cg][qg] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[st][cg], bv[st][qg], acc[cg][qg], 0, 0, 0);
            }
        }
        // ---- T = Y - (the waves' parts, one wave after the other: a fixed order of sums; waves that had no rows --
        // fewer than four 64-row chunks below the block and no chain -- are skipped)
        const int nparts = chain ? kThreads / 64 : min(kThreads / 64, (r - kbeg + 63) / 64);
        for (int wv = 0; wv < nparts; ++wv) {
            __syncthreads();
            if (wave == wv) {
#pragma unroll
                for (int cg = 0; cg < 4; ++cg)
#pragma unroll
                    for (int qg = 0; qg < QG; ++qg)
#pragma unroll
                        for (int v = 0; v < 4; ++v) TSM(16 * cg + kq + 4 * v, 16 * qg + l15) -= acc[cg][qg][v];
            }
        }
        __syncthreads();
        if (chain) {
            // X_blk = inv(L_bb)' T on the matrix cores: X[c][q] = sum_k inv(L_bb)[k][c] T[k][q]; Dg[c][k] holds
            // inv(L_bb)[k][c] (zero for k < c).  Wave = 16 columns; the result replaces T behind a barrier.
            double4_t out[QG];
#pragma unroll
            for (int qg = 0; qg < QG; ++qg) out[qg] = double4_t{0, 0, 0, 0};
            for (int st = 4 * wave; st < kTile / 4; ++st) {   // (k < 16 wave: the inverse is zero there)
                const double a = Dg[(16 * wave + l15) * kLdDiag + 4 * st + kq];
#pragma unroll
                for (int qg = 0; qg < QG; ++qg)
                    out[qg] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, TSM(4 * st + kq, 16 * qg + l15), out[qg], 0, 0, 0);
            }
            __syncthreads();
#pragma unroll
            for (int qg = 0; qg < QG; ++qg)
#pragma unroll
                for (int v = 0; v < 4; ++v) TSM(16 * wave + kq + 4 * v, 16 * qg + l15) = out[qg][v];
            __syncthreads();
        }
        // otherwise: x_blk = inv(L_bb)' t, 16 columns at a time from the last sub-block up (as k_bsolve_block)
        for (int b16 = chain ? -1 : ((wbk - 1) & ~15); b16 >= 0; b16 -= 16) {
            const int i = tid & 15;
            double zv[QG];
#pragma unroll
            for (int u = 0; u < QG; ++u) {
                const int q = (tid >> 4) + 16 * u;
                double z = 0.0;
                if (q < nq) {
#pragma unroll
                    for (int k = 0; k < 16; ++k) {
                        double lv = 0.0;  // inv(L_bb)'[i][k] = inv(L_bb)[k][i]
                        if (k > i) lv = Dg[(b16 + k) * kLdDiag + b16 + i];
                        else if (k == i) lv = invd[b16 + i];
                        z = fma(lv, TSM(b16 + k, q), z);
                    }
                }
                zv[u] = z;
            }
            __syncthreads();
#pragma unroll
            for (int u = 0; u < QG; ++u) {
                const int q = (tid >> 4) + 16 * u;
                if (q < nq) TSM(b16 + i, q) = zv[u];
            }
            __syncthreads();
            // columns above the sub-block: t[a] -= sum_k L[b16+k][a] z[k]
            for (int e = tid; e < b16 * nq; e += kThreads) {
                const int qq = e / b16, a2 = e - qq * b16;
                double accv = TSM(a2, qq);
#pragma unroll
                for (int k = 0; k < 16; ++k) accv = fma(-Dg[a2 * kLdDiag + b16 + k], TSM(b16 + k, qq), accv);
                TSM(a2, qq) = accv;
            }
            __syncthreads();
        }
        for (int e = tid; e < kTile * kPassRhs; e += kThreads) {
            const int c = e & 63, q = e >> 6;
            if (c < wbk && q < nq) {
                x[(int64_t)(q0 + q) * ldx + D.c0 + cb + c] = TSM(c, q);
                if (chain)
                    __hip_atomic_store(&xscratch[(int64_t)(q0 + q) * ldx + D.c0 + cb + c], unarmed(TSM(c, q)), __ATOMIC_RELAXED,
                                       __HIP_MEMORY_SCOPE_AGENT);
            }
        }
    }
  }
}
// ---------------------------------------------------------------------------
// The chain launches of the backward solve with many right-hand sides, 64 per pass (round 5): a kernel of its own -- inside
// k_bsolve_block_mrhs, beside that kernel's other forms, the compiler spilled 235 registers.  One workgroup per block column
// of a wide supernode, taken by ticket (last block column first).  First the rows below the supernode's own columns (x final
// there), 64-row chunks over the four waves as in k_bsolve_block_mrhs, reduced ONCE into the staged Y; then the chain, every
// wave for itself on 16 right-hand sides and all 64 columns (the comment inside).
// ---------------------------------------------------------------------------
#ifdef PARSY_BLKSTAMPS
// (diagnostic build, tools/bblk_stamps.py) the block-column tasks of the LAST launch leave 100-MHz clock stamps per block
// column jb; an array of this file's own (trsv_kernels.hip has the forward chain's: a device global cannot span two
// translation units)
__device__ unsigned long long g_bblkstamp[512 * 8];
#define BLK_STAMP(i) do { if (tid == 0 && plane == 0 && jb < 512) g_bblkstamp[jb * 8 + (i)] = wall_clock64(); } while (0)
extern "C" void parsy_debug_bblkstamps(unsigned long long* out) {
    (void)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_bblkstamp), sizeof(unsigned long long) * 512 * 8);
}
#else
#define BLK_STAMP(i) do { } while (0)
#endif
__global__ __launch_bounds__(kThreads, 1) void k_bsolve_chain_mrhs(const SnDesc* __restrict__ sn, const PanelDesc* __restrict__ pds,
                                                                  const int32_t* __restrict__ rows, const double* __restrict__ L,
                                                                  double* __restrict__ x, double* __restrict__ xscratch, int nrhs,
                                                                  int ldx, int* __restrict__ info, int* __restrict__ ticket,
                                                                  int wait_bias, int nblocks, const double* __restrict__ dinv) {
    constexpr int QG = 4;
    __shared__ double Dg[kTile * kLdDiag];
    __shared__ double ts[kTile * kLdXm];
    __shared__ double Ms[kTile * kLdDiag];   // Ms[k][c] = M[c][k]
    __shared__ int s_task;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, l15 = lane & 15, kq = lane >> 4;
    if (tid == 0) s_task = atomicAdd(ticket, 1);
    __syncthreads();
    const int plane = s_task / nblocks;
    const PanelDesc pd = pds[s_task - plane * nblocks];
    const SnDesc D = sn[pd.sn];
    const int r = D.r, w = D.w, cb = pd.jb * kTile, wbk = min(kTile, w - cb);
    const double* __restrict__ G = L + D.px;
    const int32_t* __restrict__ ri = rows + D.pi;
    {   // the inverse diagonal block (DIAG_INVERSE; identity outside the block) -> LDS: Dg[c][k] = inv(L_jj)[k][c]
        double dtmp[kTile * kTile / kThreads];
        const double* __restrict__ inv_blk = dinv + (int64_t)(D.dslot + pd.jb) * (kTile * kTile);
#pragma unroll
        for (int t = 0; t < kTile * kTile / kThreads; ++t) dtmp[t] = inv_blk[t * kThreads + tid];
#pragma unroll
        for (int t = 0; t < kTile * kTile / kThreads; ++t) {
            const int e = t * kThreads + tid;
            Dg[(e >> 6) * kLdDiag + (e & 63)] = dtmp[t];
        }
    }
    const int nbc = (w + kTile - 1) / kTile;
    const bool has_up = pd.jb + 1 < nbc;
    __syncthreads();
    if (has_up) {
        // M[c'][k] = sum_c inv(L_jj)[c][c'] L[64 (jb+1) + k][cb + c]: wave v the k's 16 v .. 16 v + 15
        const int k0 = (pd.jb + 1) * kTile + 16 * wave + l15;      // this lane's row of block jb + 1 (B operand: j = l15)
        const bool kin = k0 < w;
        const double* __restrict__ brow = G + (int64_t)cb * r + min(k0, w - 1);
        double lb[16];
#pragma unroll
        for (int st = 0; st < 16; ++st) {
            const int c = 4 * st + kq;
            const double v = brow[(int64_t)min(c, wbk - 1) * r];
            lb[st] = (kin && c < wbk) ? v : 0.0;
        }
        double4_t am[4];
#pragma unroll
        for (int cg = 0; cg < 4; ++cg) am[cg] = double4_t{0, 0, 0, 0};
#pragma unroll
        for (int st = 0; st < 16; ++st)
#pragma unroll
            for (int cg = 0; cg < 4; ++cg)
                if (st >= 4 * cg)     // (inv(L_jj)[c][c'] = 0 for c < c')
                    am[cg] = __builtin_amdgcn_mfma_f64_16x16x4f64(Dg[(16 * cg + l15) * kLdDiag + 4 * st + kq], lb[st], am[cg], 0, 0, 0);
#pragma unroll
        for (int cg = 0; cg < 4; ++cg)
#pragma unroll
            for (int v = 0; v < 4; ++v) Ms[(16 * wave + l15) * kLdDiag + 16 * cg + kq + 4 * v] = am[cg][v];
    }
    constexpr int kPassRhs = 16 * QG;
    for (int pass = plane; pass * kPassRhs < nrhs; pass += kPassLanes) {
        const int q0 = pass * kPassRhs;
        const int nq = min(kPassRhs, nrhs - q0);
        __syncthreads();
        for (int e = tid; e < kTile * kPassRhs; e += kThreads) {
            const int c = e & 63, q = e >> 6;
            TSM(c, q) = (c < wbk && q < nq) ? x[(int64_t)(q0 + q) * ldx + D.c0 + cb + c] : 0.0;
        }
        double4_t acc[4][QG];   // [16 columns][16 right-hand sides]: lane (q = l15, c = kq + 4 v)
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int b = 0; b < QG; ++b) acc[a][b] = double4_t{0, 0, 0, 0};
        // operand pointers of this lane: column c = 16 cg + l15 of the block (clamped), right-hand side 16 qg + l15
        const double* __restrict__ acol[4];
        const double* __restrict__ xcol[QG];
        bool aok[4], bok[QG];
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            aok[g] = 16 * g + l15 < wbk;
            acol[g] = G + (int64_t)(cb + min(16 * g + l15, wbk - 1)) * r;
        }
#pragma unroll
        for (int g = 0; g < QG; ++g) {
            bok[g] = 16 * g + l15 < nq;
            xcol[g] = x + (int64_t)(q0 + min(16 * g + l15, nq - 1)) * ldx;
        }
        // ---- the rows below (chain: below the supernode's own columns -- ancestors, final; otherwise everything
        // below the block: the later blocks were solved by earlier launches): 64-row chunks over the waves, 16 rows
        // (4 k steps) of loads in flight ahead of their 64 products
        // Software-pipelined over the k steps (4 rows each) of all of this wave's chunks: the operands of step t + 3 are
        // loaded while the 4 x QG products of step t are issued (a ring of four operand sets); the row ids of a chunk are
        // ONE load per lane, issued a chunk and a half ahead and handed to the lanes that need them by ds_bpermute.
        // (The plain form -- ids, then operands, then 64 products, per 16 rows -- waited two dependent round trips per 64
        // products: Flan-class input, 64 right-hand sides: 45 -> 37 ms per backward solve.)
        {
            const int kstart = w + 64 * wave;
            constexpr int kStride = 64 * (kThreads / 64);
            const int nsteps = kstart < r ? 16 * ((r - kstart + kStride - 1) / kStride) : 0;
            auto row_ids = [&](int j) {   // lane l: the row id of row l of this wave's chunk j (clamped into the panel)
                const int kr = min(kstart + kStride * j + lane, r - 1);
                return (kr < w) ? (D.c0 + kr) : ri[kr];
            };
            int ridA = row_ids(0), ridB = row_ids(1);
            double ra[4][4], rb[4][QG];
            auto load = [&](int t, double (&A)[4], double (&B)[QG]) {
                const int j = t >> 4, u = t & 15;
                const int k = kstart + kStride * j + 4 * u + kq;
                const bool kin = k < r && t < nsteps;
                const int kc = min(k, r - 1);
                const int rid = __builtin_amdgcn_ds_bpermute((4 * u + kq) * 4, (j & 1) ? ridB : ridA);
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const double a = acol[g][kc];
                    A[g] = (kin && aok[g]) ? a : 0.0;
                }
#pragma unroll
                for (int g = 0; g < QG; ++g) {
                    const double b2 = xcol[g][rid];
                    B[g] = (kin && bok[g]) ? b2 : 0.0;
                }
            };
            if (nsteps > 0) {
#pragma unroll
                for (int t = 0; t < 3; ++t) load(t, ra[t], rb[t]);
            }
            for (int t = 0; t < nsteps; t += 4) {
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int tt = t + i;
                    load(tt + 3, ra[(i + 3) & 3], rb[(i + 3) & 3]);
#pragma unroll
                    for (int cg = 0; cg < 4; ++cg)
#pragma unroll
                        for (int qg = 0; qg < QG; ++qg)
                            acc[cg][qg] = __builtin_amdgcn_mfma_f64_16x16x4f64(ra[i][cg], rb[i][qg], acc[cg][qg], 0, 0, 0);
                    if ((tt & 15) == 13) {   // the loads of this chunk's steps are all issued: its id register takes chunk j + 2
                        const int j = tt >> 4;
                        const int v = row_ids(j + 2);
                        if (j & 1) ridB = v;
                        else ridA = v;
                    }
                }
            }
        }
        {
            // ---- the later blocks of this supernode but the one right above, last one first, each as soon as its X is
            // published: rows 64 I + 16 wave .. + 15 for this wave (every 128-byte line of L read once per workgroup: with
            // all 64 rows per wave -- 16 lines per load instruction, four times over -- the Flan-class solve took 45-49 ms)
            bool ok = true;
            for (int I = nbc - 1; I > pd.jb + 1 && ok; --I) {
                double av[4][4], bv[4][QG];
                int kk[4];
#pragma unroll
                for (int st = 0; st < 4; ++st) {
                    kk[st] = I * kTile + 16 * wave + 4 * st + kq;
                    const int kc = min(kk[st], w - 1);
#pragma unroll
                    for (int g = 0; g < 4; ++g) {
                        const double a = acol[g][kc];
                        av[st][g] = (kk[st] < w && aok[g]) ? a : 0.0;
                    }
                }
                BoundedWait wait;   // (of the watch and the full poll together)
                // Only the block right above this one is on the critical path of the chain.  A workgroup further up
                // would poll for a long time, with 16 loads per lane and round, next to hundreds of others on the
                // same lines (the top separator: 313 workgroups): it first watches ONE value of the block lazily
                // (the last column this wave reads: one load per wave and round), and goes on to the full poll --
                // normally satisfied at once -- when that value is there.
                if (I - pd.jb > 1) {
                    const int kw = min(I * kTile + 16 * wave + 15, w - 1);
                    const long long* __restrict__ watch =
                        reinterpret_cast<const long long*>(xscratch + (int64_t)q0 * ldx + D.c0 + kw);
                    while (__hip_atomic_load(watch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == kXArmed ||
                           wait_bias != 0) {
                        if (wait.expired(info)) {
                            ok = false;
                            break;
                        }
                        __builtin_amdgcn_s_sleep(48);
                    }
                    if (!ok) {
                        if (lane == 0) wait_failed(info);
                        break;
                    }
                }
                for (;;) {
                    bool in = true;
#pragma unroll
                    for (int st = 0; st < 4; ++st)
#pragma unroll
                        for (int g = 0; g < QG; ++g) {
                            long long b = 0;
                            if (kk[st] < w && bok[g])
                                b = __hip_atomic_load(reinterpret_cast<const long long*>(
                                                          xscratch + (xcol[g] - x) + D.c0 + kk[st]),
                                                      __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                            in = in && b != kXArmed;
                            bv[st][g] = __longlong_as_double(b);
                        }
                    if (__all(in && wait_bias == 0)) break;
                    if (wait.expired(info)) {
                        ok = false;
                        break;
                    }
                    __builtin_amdgcn_s_sleep(1);
                }
                if (!ok) {
                    if (lane == 0) wait_failed(info);
                    break;   // (the result is wrong and reported; nobody may hang)
                }
#pragma unroll
                for (int st = 0; st < 4; ++st)
#pragma unroll
                    for (int cg = 0; cg < 4; ++cg)
#pragma unroll
                        for (int qg = 0; qg < QG; ++qg)
                            acc[cg][qg] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[st][cg], bv[st][qg], acc[cg][qg], 0, 0, 0);
            }
        }
        {
            // ---- The chain (round 5: the mirror of k_solve_blocks_mrhs's block-column task).  Its step used to be: 16 rows of
            // block I per wave (64 products), the four waves' parts subtracted from the staged Y one after the other behind
            // barriers, the product with the inverse block by 16 columns per wave behind two more, the stores through LDS -- 19 us
            // per block column on the Flan-class top separator.  Now the parts are reduced ONCE, after the block second next
            // (T in LDS), and what follows is every wave's own, on 16 right-hand sides and all 64 columns, no barrier:
            //     P = inv(L_jj)' T,     M = inv(L_jj)' L(jb + 1, jb)'   (64 x 64, formed when the pass starts)
            //     X_jb = P - M X_(jb+1)                                   (all that is left behind the last wait)
            // lane (q = l15, kk = kq) holds T[4 st + kk][q] -- the accumulator layout is the B-operand layout of k step
            // st = 4 cg + v --, results go straight from the accumulators to the armed buffer and x.
#ifdef PARSY_BLKSTAMPS
            { const int jb = pd.jb; BLK_STAMP(4); }
#endif
            // (the reduction in four rounds, all waves at once: in round rd wave v subtracts its part of the columns
            // 16 ((v + rd) & 3) .. + 15 -- disjoint quarters of T, a fixed order of sums per entry; one wave after the other
            // with all of its sixteen tiles took 4 us of the step)
#pragma unroll
            for (int rd = 0; rd < 4; ++rd) {
                __syncthreads();
#pragma unroll
                for (int cg = 0; cg < 4; ++cg)
                    if (cg == ((wave + rd) & 3)) {
#pragma unroll
                        for (int qg = 0; qg < QG; ++qg)
#pragma unroll
                            for (int v = 0; v < 4; ++v) TSM(16 * cg + kq + 4 * v, 16 * qg + l15) -= acc[cg][qg][v];
                    }
            }
            __syncthreads();
#ifdef PARSY_BLKSTAMPS
            const int jb = pd.jb;   // (BLK_STAMP's index)
            BLK_STAMP(5);
#endif
            const bool won = 16 * wave < nq;                 // this wave's 16 right-hand sides are in the pass
            const bool qok = 16 * wave + l15 < nq;
            double tv[16];
#pragma unroll
            for (int st = 0; st < 16; ++st) tv[st] = TSM(4 * st + kq, 16 * wave + l15);
            if (won) {
                const int64_t qoff = (int64_t)(q0 + min(16 * wave + l15, nq - 1)) * ldx + D.c0;   // this lane's right-hand side, row c0
                const double* __restrict__ xq = xscratch + qoff;
                bool ok = true;
                auto take_x = [&](int I, bool lazy, double (&bv)[16]) __attribute__((always_inline)) {
                    BoundedWait wait;   // (of the watch and the full poll together)
                    if (lazy) {   // (a block further up: watch ONE value first -- the top separator has 313 workgroups polling)
                        const long long* __restrict__ watch = reinterpret_cast<const long long*>(xq + min(I * kTile + 63, w - 1));
                        while (__hip_atomic_load(watch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == kXArmed || wait_bias != 0) {
                            if (wait.expired(info)) {
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
                            const int k = I * kTile + 4 * st + kq;
                            long long b = 0;
                            if (k < w && qok)
                                b = __hip_atomic_load(reinterpret_cast<const long long*>(xq + k), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                            in = in && b != kXArmed;
                            bv[st] = __longlong_as_double(b);
                        }
                        if (__all(in && wait_bias == 0)) break;
                        if (wait.expired(info)) ok = false;
                        else __builtin_amdgcn_s_sleep(1);
                    }
                };
                // P = inv(L_jj)' T: X[c'][q] = sum_{c >= c'} inv(L_jj)[c][c'] T[c][q]
                double4_t out[4];
#pragma unroll
                for (int cg = 0; cg < 4; ++cg) out[cg] = double4_t{0, 0, 0, 0};
#pragma unroll
                for (int st = 0; st < 16; ++st)
#pragma unroll
                    for (int cg = 0; cg < 4; ++cg)
                        if (st >= 4 * cg)
                            out[cg] = __builtin_amdgcn_mfma_f64_16x16x4f64(Dg[(16 * cg + l15) * kLdDiag + 4 * st + kq], tv[st], out[cg], 0, 0, 0);
                if (has_up) {
                    // (M's operands take the registers of the last block's: not before that block is multiplied)
                    asm volatile("" ::: "memory");
                    __builtin_amdgcn_sched_barrier(0);
                    double mv[16][4];
#pragma unroll
                    for (int st = 0; st < 16; ++st)
#pragma unroll
                        for (int cg = 0; cg < 4; ++cg) mv[st][cg] = Ms[(4 * st + kq) * kLdDiag + 16 * cg + l15];
                    double bv[16];
                    BLK_STAMP(6);
                    take_x(pd.jb + 1, false, bv);
                    if (!ok) {
                        if (lane == 0) wait_failed(info);
                        return;
                    }
                    BLK_STAMP(0);
                    double4_t m0[4], m1[4];
#pragma unroll
                    for (int cg = 0; cg < 4; ++cg) m0[cg] = m1[cg] = double4_t{0, 0, 0, 0};
#pragma unroll
                    for (int st = 0; st < 16; st += 2)
#pragma unroll
                        for (int cg = 0; cg < 4; ++cg) {
                            m0[cg] = __builtin_amdgcn_mfma_f64_16x16x4f64(mv[st][cg], bv[st], m0[cg], 0, 0, 0);
                            m1[cg] = __builtin_amdgcn_mfma_f64_16x16x4f64(mv[st + 1][cg], bv[st + 1], m1[cg], 0, 0, 0);
                        }
#pragma unroll
                    for (int cg = 0; cg < 4; ++cg) out[cg] -= m0[cg] + m1[cg];
                }
#ifdef PARSY_BLKSTAMPS
                asm volatile("" ::"v"(out[3][3]));
                BLK_STAMP(1);
#endif
                // straight from the accumulators (lane (q = l15, c = 16 cg + kq + 4 v)): the armed buffer first, then x
#pragma unroll
                for (int cg = 0; cg < 4; ++cg)
#pragma unroll
                    for (int v = 0; v < 4; ++v) {
                        const int c = 16 * cg + kq + 4 * v;
                        if (c < wbk && qok)
                            __hip_atomic_store(&xscratch[qoff + cb + c], unarmed(out[cg][v]), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    }
                BLK_STAMP(3);
#pragma unroll
                for (int cg = 0; cg < 4; ++cg)
#pragma unroll
                    for (int v = 0; v < 4; ++v) {
                        const int c = 16 * cg + kq + 4 * v;
                        if (c < wbk && qok) x[qoff + cb + c] = out[cg][v];
                    }
            }
        }
    }
}

#undef TSM

// Backward solve of supernodes of width <= 16: one WAVE per supernode, or per subtree of them from its root down
// (ranges != null), no LDS and no barrier -- the counterpart of k_solve_tiny.  The rows below the diagonal block
// are one row per lane (their x is final: ancestors), every lane keeps its part of t_c = sum_k L[k][c] x_k for
// the <= 16 columns and the parts are summed across the wave once, at the end (xor butterfly); lane c then holds
// column c of the diagonal block and the transposed substitution goes from the last column up with lane
// broadcasts (v_readlane).
template <int kTinyW>   // width class of the launch: kTinyWidth (16) or kTinyWidth2 (32)
__global__ __launch_bounds__(64) void k_bsolve_tiny(const SnDesc* __restrict__ sn, const PanelDesc* __restrict__ pds,
                                                    const int32_t* __restrict__ ranges,
                                                    const int32_t* __restrict__ rows, const double* __restrict__ L,
                                                    double* __restrict__ x, int nrhs, int ldx) {
    __shared__ double s_red[kTinyW * kLdRedB];   // the lanes' parts of the column sums
    const int lane = threadIdx.x;
    const int q_begin = ranges ? ranges[2 * blockIdx.x] : (int)blockIdx.x;
    const int q_end = ranges ? ranges[2 * blockIdx.x + 1] : q_begin + 1;
    for (int qsn = q_begin; qsn < q_end; ++qsn) {
        // (subtree launch: the x this wave stored for the supernode before -- an ancestor -- is read back below)
        if (qsn > q_begin) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const SnDesc D = sn[pds[qsn].sn];
        const int r = D.r, w = D.w;
        const double* __restrict__ G = L + D.px;
        const int32_t* __restrict__ ri = rows + D.pi;
        // lane c: column c of the diagonal block (rows 0..w-1); every lane: its row of the first 64 rows below
        // (unconditional loads, clamped into the panel)
        const int cl = min(lane, w - 1);
        const int kb = min(w + lane, r - 1);
        double lc[kTinyW], lb[kTinyW];
#pragma unroll
        for (int k = 0; k < kTinyW; ++k) {
            lc[k] = G[(int64_t)cl * r + min(k, w - 1)];
            lb[k] = G[(int64_t)min(k, w - 1) * r + kb];
        }
        const int row_b = ri[kb];
        double diag = 1.0;
#pragma unroll
        for (int k = 0; k < kTinyW; ++k) diag = (lane == k && k < w) ? lc[k] : diag;
        const double rdiag = 1.0 / diag;
        for (int q = blockIdx.y; q < nrhs; q += gridDim.y) {
            double* __restrict__ xq = x + (int64_t)q * ldx;
            // parts of t over this lane's rows
            double p[kTinyW];
            const double xb = (w + lane < r) ? xq[row_b] : 0.0;
#pragma unroll
            for (int c = 0; c < kTinyW; ++c) p[c] = lb[c] * xb;
            for (int k = w + 64 + lane; k < r; k += 64) {
                const double xk = xq[ri[k]];
#pragma unroll
                for (int c = 0; c < kTinyW; ++c) p[c] = fma(G[(int64_t)min(c, w - 1) * r + k], xk, p[c]);
            }
            double t = lane < w ? xq[D.c0 + lane] : 0.0;
            {
                // column sums across the wave through LDS: lane (c, g) adds up 64 / kGroups of the lanes' parts of
                // column c, the exchanges over g finish it
                constexpr int kGroups = 64 / kTinyW, kPer = 64 / kGroups;
                __builtin_amdgcn_wave_barrier();   // (the parts of the right-hand side / supernode before are consumed)
#pragma unroll
                for (int c = 0; c < kTinyW; ++c) s_red[c * kLdRedB + lane] = p[c];
                __builtin_amdgcn_wave_barrier();
                const int c = lane % kTinyW, g = lane / kTinyW;
                double v0 = 0.0, v1 = 0.0;
#pragma unroll
                for (int i = 0; i < kPer; i += 2) {
                    v0 += s_red[c * kLdRedB + kPer * g + i];
                    v1 += s_red[c * kLdRedB + kPer * g + i + 1];
                }
                double v = v0 + v1;
#pragma unroll
                for (int off = kTinyW; off < 64; off <<= 1) v += __shfl_xor(v, off);
                t = (lane < w) ? t - v : t;   // (lane c < kTinyW holds column c's sum: g == 0)
            }
            // x_k = (t_k - sum_{j > k} L[j][k] x_j) / L[k][k], from the last column up: lane c holds L[k][c] = lc[k]
            double xfin = 0.0;
#pragma unroll
            for (int k = kTinyW - 1; k >= 0; --k) {
                if (k < w) {
                    const double xk = readlane_f64(t * rdiag, k);
                    t = (lane < k) ? fma(-lc[k], xk, t) : t;
                    xfin = (lane == k) ? xk : xfin;
                }
            }
            if (lane < w) xq[D.c0 + lane] = xfin;
        }
    }
}

// Backward solve of supernodes of width <= 16, many right-hand sides: one WAVE per supernode (or per subtree of
// them from its root down), 64 right-hand sides per pass, products on the matrix cores.  T = Y - L21' X(below) as in
// k_bsolve_block_mrhs (panel rows = contraction index; 4 tiles of 16 columns x 16 right-hand sides); the result
// layout of v_mfma_f64_16x16x4_f64 (lane (q, c = kq + 4 v)) is the B-operand layout of k step v, so
// X_blk = inv(L_bb)' T is four more products per tile with T straight from the accumulators -- inv(L_bb) by
// substitution, one column per lane, through 4 KB of LDS.
__global__ __launch_bounds__(64, 4) void k_bsolve_tiny_mrhs(const SnDesc* __restrict__ sn, const PanelDesc* __restrict__ pds,
                                                         const int32_t* __restrict__ ranges,
                                                         const int32_t* __restrict__ rows, const double* __restrict__ L,
                                                         double* __restrict__ x, int nrhs, int ldx) {
    constexpr int W = kTinyWidth, kLd = W + 1;
    __shared__ double Db[W * kLd];    // diagonal block, column-major: Db[c * kLd + i] = L[i][c]
    __shared__ double Iv[W * kLd];    // its inverse:                  Iv[c * kLd + i] = inv(L_bb)[i][c]
    const int lane = threadIdx.x, l15 = lane & 15, kq = lane >> 4;
    const int q_begin = ranges ? ranges[2 * blockIdx.x] : (int)blockIdx.x;
    const int q_end = ranges ? ranges[2 * blockIdx.x + 1] : q_begin + 1;
    for (int qsn = q_begin; qsn < q_end; ++qsn) {
        // (subtree launch: the x this wave stored for the supernode before -- an ancestor -- is read back below)
        if (qsn > q_begin) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const SnDesc D = sn[pds[qsn].sn];
        const int r = D.r, w = D.w;
        const double* __restrict__ G = L + D.px;
        const int32_t* __restrict__ ri = rows + D.pi;
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int t = 0; t < W * W / 64; ++t) {
            const int e = t * 64 + lane, c = e >> 4, i = e & 15;
            double v = (i == c) ? 1.0 : 0.0;
            if (c < w && i < w && i >= c) v = G[(int64_t)c * r + i];
            Db[c * kLd + i] = v;
        }
        __builtin_amdgcn_wave_barrier();
        if (lane < W) {   // column `lane` of inv(L_bb): y_c = 1 / d_c, y_rr = -(sum_{k < rr} L[rr][k] y_k) / d_rr
            // (y lives in LDS, one row of the block per step: a register array indexed by the step would go to scratch)
            const int c = lane;
            double* __restrict__ y = &Iv[c * kLd];
#pragma unroll
            for (int k = 0; k < W; ++k) y[k] = (k == c) ? 1.0 / Db[k * kLd + k] : 0.0;
#pragma unroll 1
            for (int rr = 1; rr < W; ++rr) {
                double s0 = 0.0, s1 = 0.0;
#pragma unroll
                for (int k = 0; k < W - 1; k += 2) {
                    const double l0 = Db[k * kLd + rr], l1 = Db[(k + 1) * kLd + rr];   // (zero above the diagonal: k > rr)
                    s0 = fma(k < rr ? l0 : 0.0, y[k], s0);
                    s1 = fma(k + 1 < rr ? l1 : 0.0, y[k + 1], s1);
                }
                if (rr > c) y[rr] = -(s0 + s1) / Db[rr * kLd + rr];
            }
        }
        __builtin_amdgcn_wave_barrier();
        // A operands of the diagonal product: lane (c_out = l15, k = 4 st + kq) <- inv(L_bb)[k][c_out]
        double ainv[4];
#pragma unroll
        for (int st = 0; st < 4; ++st) ainv[st] = Iv[l15 * kLd + 4 * st + kq];
        const bool aok = l15 < w;
        const double* __restrict__ acol = G + (int64_t)min(l15, w - 1) * r;
        for (int q0 = 64 * (int)blockIdx.y; q0 < nrhs; q0 += 64 * (int)gridDim.y) {
            const int nq = min(64, nrhs - q0), nqg = (nq + 15) >> 4;
            double4_t acc[4];
#pragma unroll
            for (int g = 0; g < 4; ++g) acc[g] = double4_t{0, 0, 0, 0};
            const double* __restrict__ xcol[4];
            bool bok[4];
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                bok[g] = 16 * g + l15 < nq;
                xcol[g] = x + (int64_t)(q0 + min(16 * g + l15, nq - 1)) * ldx;
            }
            constexpr int kSt = 2;   // k steps (4 rows each) whose loads are in flight together
#pragma unroll 1
            for (int k0 = w; k0 < r; k0 += 4 * kSt) {
                double av[kSt], bv[kSt][4];
#pragma unroll
                for (int st = 0; st < kSt; ++st) {
                    const int k = k0 + 4 * st + kq;
                    const bool kin = k < r;
                    const int kc = min(k, r - 1);
                    const int rid = ri[kc];
                    const double a = acol[kc];
                    av[st] = (kin && aok) ? a : 0.0;
#pragma unroll
                    for (int g = 0; g < 4; ++g) {
                        double b = 0.0;
                        if (g < nqg) b = xcol[g][rid];
                        bv[st][g] = (kin && bok[g]) ? b : 0.0;
                    }
                }
#pragma unroll
                for (int st = 0; st < kSt; ++st)
#pragma unroll
                    for (int g = 0; g < 4; ++g)
                        if (g < nqg) acc[g] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[st], bv[st][g], acc[g], 0, 0, 0);
            }
            // T = Y - acc in the accumulator layout (lane (q = l15, c = kq + 4 v)), then X_blk = inv(L_bb)' T
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                if (g >= nqg) continue;
                double4_t t;
#pragma unroll
                for (int v = 0; v < 4; ++v) {
                    const int c = kq + 4 * v;
                    const double y = xcol[g][D.c0 + min(c, w - 1)];
                    t[v] = (c < w && bok[g]) ? y - acc[g][v] : 0.0;
                }
                double4_t out = {0, 0, 0, 0};
#pragma unroll
                for (int st = 0; st < 4; ++st) out = __builtin_amdgcn_mfma_f64_16x16x4f64(ainv[st], t[st], out, 0, 0, 0);
#pragma unroll
                for (int v = 0; v < 4; ++v) {
                    const int c = kq + 4 * v;
                    if (c < w && bok[g]) x[(int64_t)(q0 + 16 * g + l15) * ldx + D.c0 + c] = out[v];
                }
            }
        }
    }
}

// Backward solve, one right-hand side: the sums of a wide supernode's block column over the rows BELOW the supernode's
// own columns (x of the ancestors: final when the level starts), for the chain launches of few, tall supernodes.
// One workgroup (4 waves) per (supernode, block column, chunk of kBelowRows rows): wave q carries columns 16 q .. 16 q + 15
// of the block, lanes along the rows (coalesced), the lanes' parts added up through LDS as in k_bsolve_chain_w; the 64
// sums of the chunk go to its slot of `part`.  The chain adds the slots of a block column in chunk order.
__global__ __launch_bounds__(kThreads) void k_bsolve_below(const SnDesc* __restrict__ sn, const PanelDesc* __restrict__ tasks,
                                                           const int32_t* __restrict__ rows, const double* __restrict__ L,
                                                           const double* __restrict__ x, double* __restrict__ part) {
    constexpr int kCols = 16, kLdR = 65;
    __shared__ double s_red[kThreads / 64][kCols * kLdR];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const PanelDesc pd = tasks[blockIdx.x];
    const SnDesc D = sn[pd.sn];
    const int r = D.r, w = D.w;
    const int cb = pd.jb * kTile, wbk = min(kTile, w - cb);
    const double* __restrict__ G = L + D.px;
    const int32_t* __restrict__ ri = rows + D.pi;
    const double* __restrict__ colp[kCols];
#pragma unroll
    for (int ci = 0; ci < kCols; ++ci) colp[ci] = G + (int64_t)(cb + min(kCols * wave + ci, wbk - 1)) * r;
    double acc[kCols];
#pragma unroll
    for (int ci = 0; ci < kCols; ++ci) acc[ci] = 0.0;
    const int k1 = min(pd.row0 + kBelowRows, r);
    for (int k0 = pd.row0 + lane; k0 < k1; k0 += 128) {   // two 64-row pieces in flight
        const int ka = k0, kb = min(k0 + 64, r - 1);
        const int xa = ri[ka], xb = ri[kb];
        double la[kCols], lb[kCols];
#pragma unroll
        for (int ci = 0; ci < kCols; ++ci) la[ci] = colp[ci][ka];
#pragma unroll
        for (int ci = 0; ci < kCols; ++ci) lb[ci] = colp[ci][kb];
        const double va = x[xa], vb = (k0 + 64 < k1) ? x[xb] : 0.0;
#pragma unroll
        for (int ci = 0; ci < kCols; ++ci) acc[ci] = fma(la[ci], va, acc[ci]);
#pragma unroll
        for (int ci = 0; ci < kCols; ++ci) acc[ci] = fma(lb[ci], vb, acc[ci]);
    }
    double* __restrict__ red = s_red[wave];
#pragma unroll
    for (int ci = 0; ci < kCols; ++ci) red[ci * kLdR + lane] = acc[ci];
    __builtin_amdgcn_wave_barrier();
    const int c = lane % kCols, g = lane / kCols;   // 4 row groups of 16 parts per column
    double v0 = 0.0, v1 = 0.0;
#pragma unroll
    for (int i = 0; i < 16; i += 2) {
        v0 += red[c * kLdR + 16 * g + i];
        v1 += red[c * kLdR + 16 * g + i + 1];
    }
    double v = v0 + v1;
    v += __shfl_xor(v, 16);
    v += __shfl_xor(v, 32);
    if (g == 0) part[(int64_t)pd.pad * kTile + kCols * wave + c] = v;
}

void launch_bsolve_below(const DevicePattern& P, int first, int count, const double* L, const double* x, hipStream_t stream) {
    if (count <= 0) return;
    launch_witnessed<k_bsolve_below, kWBsolveBelow>(dim3(count), dim3(kThreads), 0, stream, P.sn,
        P.bsolve_below + first, P.rows, L, x, P.bpart);
}

// Backward chain for ONE right-hand side: the counterpart of k_solve_chain_w.  A workgroup = eight waves = up to
// kBackGroup (2) consecutive block columns of a wide supernode (the highest one first), taken by ticket from a list
// that runs from the last block column of a supernode to its first; four waves share a block column, 16 columns
// each, lanes along the rows (coalesced), 16 running sums per lane:
//     t_c = sum_k L[k][c] x_k   over the rows k below the block.
// First the rows below the supernode's own columns (x final: ancestors), then the supernode's later block
// columns from the last one up, each as soon as its x is there -- through the armed buffer (the data is the
// flag: lane k polls the value of row k), or through LDS when it is a higher block of this workgroup; the loads
// of four 64-row pieces are in flight before the first wait.  (More block columns per workgroup would keep more of
// the diagonal-to-diagonal hand-offs in LDS, but a block column's rows are streamed by its own waves only, and
// the number of CUs that stream is what bounds the launches of few, wide supernodes: four per workgroup measured
// 16.1 vs 7.6 ms on the Flan-class input.)  Then the sums are added up across the wave, the waves' columns meet
// in LDS, and the first wave of the
// block forms x_blk = inv(L_bb)' (y - t) as a product with the inverse diagonal block (DIAG_INVERSE; staged in LDS
// when the wave starts) and publishes it (LDS for the blocks below it in this workgroup, armed buffer + x for
// everybody else).  No workgroup barrier after the start, every wait bounded.
static constexpr int kBackBlocks = kBackGroup;            // block columns per workgroup
static constexpr int kBackWaves = 8 / kBackBlocks;        // waves per block column
static constexpr int kBackCols = kTile / kBackWaves;      // columns per wave
static constexpr int kBackAhead = 64 / kBackCols;         // 64-row pieces whose loads are issued before the first wait
static constexpr int kLdRed = 65;                         // row stride of a wave's reduction buffer (doubles)
__global__ __launch_bounds__(kChainThreads, 1) void k_bsolve_chain_w(const SnDesc* __restrict__ sn,
                                                                     const PanelDesc* __restrict__ groups,
                                                                     const int32_t* __restrict__ rows,
                                                                     const double* __restrict__ L,
                                                                     const double* __restrict__ dinv,
                                                                     double* __restrict__ x, double* __restrict__ xscratch,
                                                                     int* __restrict__ info, int* __restrict__ ticket,
                                                                     int wait_bias, const double* __restrict__ part) {
    __shared__ double s_inv[kBackBlocks][kInvPacked + 1];   // column c of the inverse from row c on (as k_solve_chain_w)
    __shared__ double s_t[kBackBlocks][kTile];              // t of a block: its waves' column sums
    __shared__ double s_pub[kBackBlocks][kTile];            // x of a block, for the blocks below it in this workgroup
    __shared__ double s_red[kChainThreads / 64][kBackCols * kLdRed];   // per wave: the lanes' parts of the column sums
    __shared__ int s_sums_in[kBackBlocks], s_ready[kBackBlocks];
    __shared__ int s_task;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int b = wave / kBackWaves, qw = wave % kBackWaves;   // block of the group (0: the highest), wave of the block
    if (threadIdx.x == 0) s_task = atomicAdd(ticket, 1);
    if (threadIdx.x < kBackBlocks) {
        s_sums_in[threadIdx.x] = 0;
        s_ready[threadIdx.x] = 0;
    }
    __syncthreads();   // (the only one)
    const PanelDesc pd = groups[s_task];    // jb: the highest block column; row0: blocks of this workgroup (1..4)
    if (b >= pd.row0) return;
    const SnDesc D = sn[pd.sn];
    const int r = D.r, w = D.w;
    const int jb = pd.jb - b, cb = jb * kTile, wbk = min(kTile, w - cb);
    const int nbc = (w + kTile - 1) / kTile;
    const double* __restrict__ G = L + D.px;
    const int32_t* __restrict__ ri = rows + D.pi;
    auto inv_at = [&](int c) { return lane >= c ? c * kTile - c * (c - 1) / 2 + (lane - c) : kInvPacked; };
    if (qw == 0) {
        // inverse diagonal block -> LDS: lane = row, column c of the inverse from row c on
        const double* __restrict__ src = dinv + (int64_t)(D.dslot + jb) * (kTile * kTile);
        double tmp[kTile];
#pragma unroll
        for (int c = 0; c < kTile; ++c) tmp[c] = src[c * kTile + lane];
#pragma unroll
        for (int c = 0; c < kTile; ++c) s_inv[b][inv_at(c)] = tmp[c];
    }
    // this wave's columns (clamped into the block: the sums of columns past it are not used); wave-uniform pointers,
    // every load unconditional
    const double* __restrict__ colp[kBackCols];
#pragma unroll
    for (int ci = 0; ci < kBackCols; ++ci) colp[ci] = G + (int64_t)(cb + min(kBackCols * qw + ci, wbk - 1)) * r;
    double acc[kBackCols];
#pragma unroll
    for (int ci = 0; ci < kBackCols; ++ci) acc[ci] = 0.0;
    double lv[kBackAhead][kBackCols];
    auto load_piece = [&](int u, int k) {
#pragma unroll
        for (int ci = 0; ci < kBackCols; ++ci) lv[u][ci] = colp[ci][k];
    };
    // ---- rows below the supernode's own columns: x is final.  Summed by k_bsolve_below before this launch (pd.pad =
    // the supernode's first slot + 1: one slot of 64 sums per block column and 512-row chunk) or streamed here.
    // Lane (c, g) of the final reduction adds the chunks g, g + 4, .. of its column, in that order: loaded now, used then.
    double below = 0.0;
    if (pd.pad > 0) {
        const int nch = (r - w + kBelowRows - 1) / kBelowRows;
        const double* __restrict__ mine = part + ((int64_t)(pd.pad - 1) + (int64_t)jb * nch) * kTile + kBackCols * qw + lane % kBackCols;
        for (int ch = lane / kBackCols; ch < nch; ch += 64 / kBackCols) below += mine[(int64_t)ch * kTile];
    }
    for (int k0 = w + lane; k0 < r && pd.pad <= 0; k0 += 64 * kBackAhead) {
        int xr[kBackAhead];
#pragma unroll
        for (int u = 0; u < kBackAhead; ++u) {
            const int k = min(k0 + 64 * u, r - 1);
            xr[u] = ri[k];
            load_piece(u, k);
        }
#pragma unroll
        for (int u = 0; u < kBackAhead; ++u) {
            const double xk = (k0 + 64 * u < r) ? x[xr[u]] : 0.0;
#pragma unroll
            for (int ci = 0; ci < kBackCols; ++ci) acc[ci] = fma(lv[u][ci], xk, acc[ci]);
        }
    }
    // ---- the later block columns of the supernode, last one first
    for (int I0 = nbc - 1; I0 > jb; I0 -= kBackAhead) {
#pragma unroll
        for (int u = 0; u < kBackAhead; ++u)   // (pieces past jb + 1: loaded again, not used)
            load_piece(u, min(max(I0 - u, jb + 1) * kTile + lane, w - 1));
#pragma unroll
        for (int u = 0; u < kBackAhead; ++u) {
            const int I = I0 - u;
            if (I <= jb) break;
            const int k = I * kTile + lane;
            double xk = 0.0;
            if (I <= pd.jb) {
                // a higher block of this workgroup: LDS
                if (!wait_lds_counter(&s_ready[pd.jb - I], 1, wait_bias, info)) {
                    if (lane == 0) wait_failed(info);   // (the result is wrong and reported; nobody may hang)
                    return;
                }
                xk = s_pub[pd.jb - I][lane];
            } else {
                const long long* __restrict__ src = reinterpret_cast<const long long*>(xscratch + D.c0) + k;
                BoundedWait wait;
                long long bits = 0;
                for (;;) {
                    bits = k < w ? __hip_atomic_load(src, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0;
                    if (__all(bits != kXArmed && wait_bias == 0)) break;
                    if (wait.expired(info)) {
                        if (lane == 0) wait_failed(info);
                        return;
                    }
                    if (I <= pd.jb + 2) __builtin_amdgcn_s_sleep(1);   // (the blocks right above: the critical path)
                    else __builtin_amdgcn_s_sleep(8);
                }
                xk = __longlong_as_double(bits);
            }
            if (k >= w) xk = 0.0;
#pragma unroll
            for (int ci = 0; ci < kBackCols; ++ci) acc[ci] = fma(lv[u][ci], xk, acc[ci]);
        }
    }
    // ---- column sums across the wave, through LDS: every lane parks its kBackCols parts, lane (c, g) adds up the
    // parts of 64 / (64 / kBackCols) rows for column c, two exchanges finish the column (16 xor butterflies of six
    // steps each took about 1 us of every step of the chain; a butterfly that halves the columns a lane carries
    // per step -- 17 exchanges -- measured slower still); then the block's waves meet in LDS
    {
        constexpr int kGroups = 64 / kBackCols;      // row groups a column's 64 parts are split into
        constexpr int kPer = 64 / kGroups;           // parts per group (= kBackCols)
        double* __restrict__ red = s_red[wave];
#pragma unroll
        for (int ci = 0; ci < kBackCols; ++ci) red[ci * kLdRed + lane] = acc[ci];
        __builtin_amdgcn_wave_barrier();
        const int c = lane % kBackCols, g = lane / kBackCols;
        double v0 = 0.0, v1 = 0.0;
#pragma unroll
        for (int i = 0; i < kPer; i += 2) {
            v0 += red[c * kLdRed + kPer * g + i];
            v1 += red[c * kLdRed + kPer * g + i + 1];
        }
        double v = v0 + v1 + below;
#pragma unroll
        for (int off = kBackCols; off < 64; off <<= 1) v += __shfl_xor(v, off);
        if (g == 0) s_t[b][kBackCols * qw + c] = v;
    }
    __builtin_amdgcn_wave_barrier();
    if (lane == 0) __hip_atomic_fetch_add(&s_sums_in[b], 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (qw != 0) return;
    if (!wait_lds_counter(&s_sums_in[b], kTile / kBackCols, wait_bias, info)) {
        if (lane == 0) wait_failed(info);
        return;
    }
    // ---- x_blk = inv(L_bb)' (y - t): x_c = sum_{k >= c} inv(L_bb)[k][c] (y_k - t_k); lane c walks its column of
    // the packed inverse
    const double tk = (lane < wbk) ? x[D.c0 + cb + lane] - s_t[b][lane] : 0.0;
    __builtin_amdgcn_wave_barrier();
    s_t[b][lane] = tk;
    __builtin_amdgcn_wave_barrier();
    double s0 = 0.0, s1 = 0.0;
    {
        // column `lane` of the inverse: rows lane..63 are contiguous from lane*64 - lane(lane-1)/2
        const double* __restrict__ col = s_inv[b] + lane * kTile - lane * (lane - 1) / 2 - lane;   // col[k], k >= lane
        for (int k = lane; k + 1 < kTile; k += 2) {
            s0 = fma(col[k], s_t[b][k], s0);
            s1 = fma(col[k + 1], s_t[b][k + 1], s1);
        }
        if (((kTile - lane) & 1) != 0) s0 = fma(col[kTile - 1], s_t[b][kTile - 1], s0);
    }
    const double xi = (lane < wbk) ? s0 + s1 : 0.0;
    if (b + 1 < pd.row0) {
        s_pub[b][lane] = xi;
        __builtin_amdgcn_wave_barrier();
        if (lane == 0) __hip_atomic_store(&s_ready[b], 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
    if (lane < wbk) {
        __hip_atomic_store(&xscratch[D.c0 + cb + lane], unarmed(xi), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        x[D.c0 + cb + lane] = xi;
    }
}

void launch_bsolve_chain_w(const DevicePattern& P, int first, int count, const double* L, const double* dinv,
                           double* x, double* xscratch, int ticket, int wait_bias, hipStream_t stream) {
    if (count <= 0) return;
    launch_witnessed<k_bsolve_chain_w, kWBsolveChainW>(dim3(count), dim3(kChainThreads), 0, stream, P.sn,
        P.bsolve_pairs + first, P.rows, L, dinv, x, xscratch, P.sinfo, P.stickets + ticket, wait_bias, P.bpart);
}

// (backward launches of at least SolveGates::bmrhs_wide_blocks blocks, 128, take 64 right-hand sides per pass)
// form: Launch::form -- kFormEach: one workgroup per block, kFormChain: chain launch (tickets), kFormSubtrees: subtree launch
// (`first` counts (begin, end) pairs of bsolve_ranges, which index the whole block list)
// (k: by width class, right-hand sides, form and count -- back_block_kernel, solve_route.cpp)
void launch_bsolve_block(const DevicePattern& P, WitnessKernel k, int first, int count, const double* L, const double* dinv,
                         double* x, double* xscratch, int nrhs, int ldx, LaunchForm form, int ticket, int wait_bias,
                         hipStream_t stream) {
    if (count <= 0) return;
    const int chain = form == kFormChain;
    const PanelDesc* pds = form == kFormSubtrees ? P.bsolve_blocks : P.bsolve_blocks + first;
    const int32_t* ranges = form == kFormSubtrees ? P.bsolve_ranges + 2 * first : nullptr;
    static_assert(kTinyWidth == 16 && kTinyWidth2 == 32, "witness entries k_bsolve_tiny<16>, <32>");
    switch (k) {
        case kWBsolveTinyMrhs: {   // many right-hand sides: 64 per pass, matrix cores, one wave per supernode
            const dim3 grid(count, std::min(kPassLanes, (nrhs + kRhsM - 1) / kRhsM));
            launch_witnessed<k_bsolve_tiny_mrhs, kWBsolveTinyMrhs>(grid, dim3(64), 0, stream, P.sn, pds, ranges, P.rows, L,
                x, nrhs, ldx);
            break;
        }
        // width class kTinyWidth or kTinyWidth2, a subtree launch or a level's launch: one wave each
        case kWBsolveTiny16:
        case kWBsolveTiny32: {
            const dim3 grid(count, std::min(kPassLanes, nrhs));
            if (k == kWBsolveTiny16) {
                launch_witnessed<k_bsolve_tiny<kTinyWidth>, kWBsolveTiny16>(grid, dim3(64), 0, stream, P.sn, pds, ranges,
                    P.rows, L, x, nrhs, ldx);
            } else {
                launch_witnessed<k_bsolve_tiny<kTinyWidth2>, kWBsolveTiny32>(grid, dim3(64), 0, stream, P.sn, pds, ranges,
                    P.rows, L, x, nrhs, ldx);
            }
            break;
        }
        case kWBsolveChainMrhs: {   // 64 right-hand sides per pass
            const int mlanes = std::min(kPassLanes, (nrhs + kRhsM - 1) / kRhsM);
            launch_witnessed<k_bsolve_chain_mrhs, kWBsolveChainMrhs>(dim3(count * mlanes), dim3(kThreads), 0, stream, P.sn,
                pds, P.rows, L, x, xscratch, nrhs, ldx, P.sinfo, P.stickets + ticket, wait_bias, count, dinv);
            break;
        }
        // products on the matrix cores: <1> 16 right-hand sides per pass in up to 8 workgroups per block side by side (launches
        // of few blocks: the top of the tree, small inputs), <4> 64 per pass (L read once per 64)
        case kWBsolveBlockMrhs4:
        case kWBsolveBlockMrhs1: {
            const bool wide = k == kWBsolveBlockMrhs4;
            const int per = wide ? kRhsM : 16;
            const int mlanes = std::min(kPassLanes, (nrhs + per - 1) / per);
            const dim3 mgrid = chain ? dim3(count * mlanes) : dim3(count, mlanes);
            if (wide) {
                launch_witnessed<k_bsolve_block_mrhs<4>, kWBsolveBlockMrhs4>(mgrid, dim3(kThreads), 0, stream, P.sn, pds,
                    P.rows, L, x, xscratch, nrhs, ldx, chain, P.sinfo, P.stickets + ticket, wait_bias, count, ranges, dinv);
            } else {
                launch_witnessed<k_bsolve_block_mrhs<1>, kWBsolveBlockMrhs1>(mgrid, dim3(kThreads), 0, stream, P.sn, pds,
                    P.rows, L, x, xscratch, nrhs, ldx, chain, P.sinfo, P.stickets + ticket, wait_bias, count, ranges, dinv);
            }
            break;
        }
        // the light kernel: 4 right-hand sides per workgroup, up to 8 workgroups per block side by side
        case kWBsolveBlock1:
        case kWBsolveBlock4: {
            const int lanes = nrhs == 1 ? 1 : std::min(kPassLanes, (nrhs + 3) / 4);
            const dim3 grid = chain ? dim3(count * lanes) : dim3(count, lanes);
            if (k == kWBsolveBlock1) {
                launch_witnessed<k_bsolve_block<1>, kWBsolveBlock1>(grid, dim3(kThreads), 0, stream, P.sn, pds, P.rows, L, x,
                    xscratch, nrhs, ldx, chain, P.sinfo, P.stickets + ticket, wait_bias, count, ranges, dinv);
            } else {
                launch_witnessed<k_bsolve_block<4>, kWBsolveBlock4>(grid, dim3(kThreads), 0, stream, P.sn, pds, P.rows, L, x,
                    xscratch, nrhs, ldx, chain, P.sinfo, P.stickets + ticket, wait_bias, count, ranges, dinv);
            }
            break;
        }
        default: launch_refused("launch_bsolve_block", k);
    }
}

}  // namespace parsy
