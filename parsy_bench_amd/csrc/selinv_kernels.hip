// Selected inversion on the device (selinv.hpp): Z = (P A P')^-1 on the pattern of L, level by level from the root,
// diag(A^-1) in the caller's ordering and log det A.
//
// Per level, two kernel paths (split by |R_b|, PARSY_SELINV_TILED_MIN):
//   TILED  k_selinv_tinv  one wave per block column: T = L_bb^-1 into a 64 x 64 scratch slot;
//          k_selinv_y     one workgroup per 64-row tile of R_b: Y_t = L(R_b tile t, b) T (MFMA) into a slot;
//          k_selinv_z     one workgroup per 64-row tile of R_b: Z(tile t, b) = -sum_k Z(tile t, chunk k) Y_k, the operand
//                         chunks gathered through the map (symmetric: the lower triangle of Z only), FP64 MFMA; then the
//                         partial Y_t' Z(tile t, b) into a slot;
//          k_selinv_zbb   one workgroup per block column: Z(b, b) = T'T - (partials summed in tile order), zeros above.
//   SMALL  k_selinv_small one workgroup per block column, in LDS, over 32-row chunks of R_b with the products
//          reassociated so that no full Y is held: W = Z(chunk, R_b) L(R_b, b), Z(chunk, b) = -W T, G += L(chunk, b)'
//          Z(chunk, b); at the end Z(b, b) = T'(T - G).
// Every output entry has one writer and every sum a fixed order, with no atomics: Z is bitwise reproducible.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <climits>
#include <cmath>
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

constexpr int kSThreads = 256;
constexpr int kLd = kLdDiag;            // LDS leading dimension of a 64-row block
constexpr int kSlot = kTile * kTile;    // doubles of a scratch slot
constexpr int kChunk = 32;              // rows of R_b per step of the small path
constexpr int kLdC = kChunk + 1;
constexpr int kLogParts = 256;          // workgroups of the log-determinant's first pass

// ---- T = L_bb^-1 in LDS, one wave: the blocked inversion of the solves' k_diag_inverse (trsv_aux_kernels.hip), spelled out
// here a second time -- one shared inline function changed the instruction schedule of both (mm16 / put16: device_util.hpp)
// M (64 x kLd doubles of LDS) := inv(L_bb), lower triangle, zeros above, an identity past wb.  Lanes 0..63 of one wave.
__device__ void tinv64(double* __restrict__ M, const double* __restrict__ G, int r, int j0, int wb) {
    const int lane = threadIdx.x & 63, l15 = lane & 15, kq = lane >> 4;
    {
        double v[kTile];
        const double* __restrict__ src = G + (int64_t)j0 * r + j0 + min(lane, wb - 1);
#pragma unroll
        for (int cc = 0; cc < kTile; ++cc) v[cc] = src[(int64_t)min(cc, wb - 1) * r];
#pragma unroll
        for (int cc = 0; cc < kTile; ++cc)
            M[cc * kLd + lane] = (cc < wb && lane < wb && lane >= cc) ? v[cc] : (lane == cc ? 1.0 : 0.0);
    }
    __builtin_amdgcn_wave_barrier();
    auto blk = [&](int bi, int bj) { return M + (16 * bj) * kLd + 16 * bi; };
    {
        double* __restrict__ B = blk(kq, kq);
        double y[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) y[k] = 0.0;
#pragma unroll
        for (int rr = 0; rr < 16; ++rr) {
            double sacc = (rr == l15) ? -1.0 : 0.0;
#pragma unroll
            for (int k = 0; k < rr; ++k) sacc = fma(B[k * kLd + rr], y[k], sacc);
            y[rr] = (rr >= l15) ? -sacc / B[rr * kLd + rr] : 0.0;
        }
        __builtin_amdgcn_s_waitcnt(0);
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int rr = 0; rr < 16; ++rr) B[l15 * kLd + rr] = y[rr];
    }
    __builtin_amdgcn_wave_barrier();
    const double4_t zero = {0, 0, 0, 0};
#pragma unroll
    for (int b = 0; b < 4; b += 2) {
        const double4_t t = mm16(zero, blk(b + 1, b), blk(b, b), l15, kq);
        __builtin_amdgcn_s_waitcnt(0);
        __builtin_amdgcn_wave_barrier();
        put16(blk(b + 1, b), t, 1.0, l15, kq);
        __builtin_amdgcn_wave_barrier();
        const double4_t u = mm16(zero, blk(b + 1, b + 1), blk(b + 1, b), l15, kq);
        __builtin_amdgcn_s_waitcnt(0);
        __builtin_amdgcn_wave_barrier();
        put16(blk(b + 1, b), u, -1.0, l15, kq);
        __builtin_amdgcn_wave_barrier();
    }
    {
        double4_t t20 = mm16(mm16(zero, blk(2, 0), blk(0, 0), l15, kq), blk(2, 1), blk(1, 0), l15, kq);
        double4_t t30 = mm16(mm16(zero, blk(3, 0), blk(0, 0), l15, kq), blk(3, 1), blk(1, 0), l15, kq);
        double4_t t21 = mm16(zero, blk(2, 1), blk(1, 1), l15, kq);
        double4_t t31 = mm16(zero, blk(3, 1), blk(1, 1), l15, kq);
        __builtin_amdgcn_s_waitcnt(0);
        __builtin_amdgcn_wave_barrier();
        put16(blk(2, 0), t20, 1.0, l15, kq);
        put16(blk(3, 0), t30, 1.0, l15, kq);
        put16(blk(2, 1), t21, 1.0, l15, kq);
        put16(blk(3, 1), t31, 1.0, l15, kq);
        __builtin_amdgcn_wave_barrier();
        double4_t x20 = mm16(zero, blk(2, 2), blk(2, 0), l15, kq);
        double4_t x21 = mm16(zero, blk(2, 2), blk(2, 1), l15, kq);
        double4_t x30 = mm16(mm16(zero, blk(3, 2), blk(2, 0), l15, kq), blk(3, 3), blk(3, 0), l15, kq);
        double4_t x31 = mm16(mm16(zero, blk(3, 2), blk(2, 1), l15, kq), blk(3, 3), blk(3, 1), l15, kq);
        __builtin_amdgcn_s_waitcnt(0);
        __builtin_amdgcn_wave_barrier();
        put16(blk(2, 0), x20, -1.0, l15, kq);
        put16(blk(2, 1), x21, -1.0, l15, kq);
        put16(blk(3, 0), x30, -1.0, l15, kq);
        put16(blk(3, 1), x31, -1.0, l15, kq);
        __builtin_amdgcn_wave_barrier();
    }
}

// acc[c] += A(16 w + ., k) B(k, 16 c + .) over k < 64, A(i, k) = A[i * ai + k * ak], B(k, j) = B[k * bk + j * bj] in LDS.
// Wave w owns rows 16 w .. 16 w + 15 of the 64 x 64 result: acc[c][v] = C(16 w + kq + 4 v, 16 c + l15).
__device__ __forceinline__ void mm64(double4_t (&acc)[4], const double* __restrict__ A, int ai, int ak,
                                     const double* __restrict__ B, int bk, int bj, int w, int l15, int kq) {
#pragma unroll 4
    for (int k4 = 0; k4 < kTile / 4; ++k4) {
        const int k = 4 * k4 + kq;
        const double a = A[(16 * w + l15) * ai + k * ak];
#pragma unroll
        for (int c = 0; c < 4; ++c)
            acc[c] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, B[k * bk + (16 * c + l15) * bj], acc[c], 0, 0, 0);
    }
}

// Z(p, q) for positions p, q of the supernode's row list: the lower triangle through the map
__device__ __forceinline__ int64_t zaddr(int64_t cbq, int64_t moq, const int32_t* __restrict__ gmap, int p) {
    return cbq + gmap[moq + p];
}

// ---- tiled path --------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_selinv_tinv(const SelinvBc* __restrict__ bcs, int d0,
                                                    const double* __restrict__ L, double* __restrict__ scr) {
    __shared__ double M[kTile * kLd];
    const SelinvBc B = bcs[d0 + blockIdx.x];
    tinv64(M, L + B.px, B.r, B.j0, B.wb);
    __builtin_amdgcn_wave_barrier();
    double* __restrict__ out = scr + (int64_t)B.tslot * kSlot;
    for (int e = threadIdx.x; e < kSlot; e += 64) {
        const int c = e >> 6, i = e & 63;
        out[e] = (i < B.wb && c < B.wb) ? M[c * kLd + i] : 0.0;
    }
}

__global__ __launch_bounds__(kSThreads) void k_selinv_y(const SelinvBc* __restrict__ bcs, const int32_t* __restrict__ tasks,
                                                        const double* __restrict__ L, double* __restrict__ scr) {
    __shared__ double As[kTile * kLd], Bs[kTile * kLd];
    const int d = tasks[2 * blockIdx.x], t = tasks[2 * blockIdx.x + 1];
    const SelinvBc B = bcs[d];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, l15 = lane & 15, kq = lane >> 4;
    const int p0 = B.j0 + B.wb, pr = p0 + kTile * t, nr = min(kTile, B.m - kTile * t);
    const double* __restrict__ G = L + B.px;
    const double* __restrict__ T = scr + (int64_t)B.tslot * kSlot;
    for (int e = tid; e < kSlot; e += kSThreads) {
        const int i = e & 63, k = e >> 6;
        As[k * kLd + i] = (i < nr && k < B.wb) ? G[(int64_t)(B.j0 + k) * B.r + pr + i] : 0.0;
        Bs[k * kLd + i] = T[e];
    }
    __syncthreads();
    double4_t acc[4] = {{0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}};
    mm64(acc, As, 1, kLd, Bs, 1, kLd, w, l15, kq);
    double* __restrict__ Y = scr + (int64_t)(B.yslot + t) * kSlot;
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int v = 0; v < 4; ++v) Y[(16 * c + l15) * kTile + 16 * w + kq + 4 * v] = acc[c][v];
}

__global__ __launch_bounds__(kSThreads) void k_selinv_z(const SelinvBc* __restrict__ bcs, const int32_t* __restrict__ tasks,
                                                        const int64_t* __restrict__ cb, const int64_t* __restrict__ mo,
                                                        const int32_t* __restrict__ gmap, double* __restrict__ Z,
                                                        double* __restrict__ scr) {
    __shared__ double As[kTile * kLd], Bs[kTile * kLd];
    __shared__ int64_t rcb[kTile], rmo[kTile], kcb[kTile], kmo[kTile];
    const int d = tasks[2 * blockIdx.x], t = tasks[2 * blockIdx.x + 1];
    const SelinvBc B = bcs[d];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, l15 = lane & 15, kq = lane >> 4;
    const int p0 = B.j0 + B.wb, pr = p0 + kTile * t, nr = min(kTile, B.m - kTile * t);
    if (tid < nr) {
        rcb[tid] = cb[B.pi + pr + tid];
        rmo[tid] = mo[B.pi + pr + tid];
    }
    double4_t acc[4] = {{0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}};
    const int nk = (B.m + kTile - 1) / kTile;
    for (int kc = 0; kc < nk; ++kc) {
        const int pk = p0 + kTile * kc, nkk = min(kTile, B.m - kTile * kc);
        __syncthreads();   // (the previous chunk's products have read As / Bs)
        if (tid < nkk) {
            kcb[tid] = cb[B.pi + pk + tid];
            kmo[tid] = mo[B.pi + pk + tid];
        }
        const double* __restrict__ Yk = scr + (int64_t)(B.yslot + kc) * kSlot;
        for (int e = tid; e < kSlot; e += kSThreads) Bs[(e >> 6) * kLd + (e & 63)] = Yk[e];
        __syncthreads();
        // A(i, k) = Z(pr + i, pk + k): the stored entry of the pair's lower triangle
        for (int e = tid; e < kSlot; e += kSThreads) {
            const int i = e & 63, k = e >> 6, p = pr + i, q = pk + k;
            double v = 0.0;
            if (i < nr && k < nkk) v = Z[p >= q ? zaddr(kcb[k], kmo[k], gmap, p) : zaddr(rcb[i], rmo[i], gmap, q)];
            As[k * kLd + i] = v;
        }
        __syncthreads();
        mm64(acc, As, 1, kLd, Bs, 1, kLd, w, l15, kq);
    }
    __syncthreads();
    // Z(tile, b) = -acc: through LDS (coalesced stores), kept there for the partial
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int v = 0; v < 4; ++v) As[(16 * c + l15) * kLd + 16 * w + kq + 4 * v] = -acc[c][v];
    const double* __restrict__ Yt = scr + (int64_t)(B.yslot + t) * kSlot;
    for (int e = tid; e < kSlot; e += kSThreads) Bs[(e >> 6) * kLd + (e & 63)] = Yt[e];
    __syncthreads();
    double* __restrict__ G = Z + B.px;
    for (int e = tid; e < kSlot; e += kSThreads) {
        const int i = e & 63, c = e >> 6;
        if (i < nr && c < B.wb) G[(int64_t)(B.j0 + c) * B.r + pr + i] = As[c * kLd + i];
    }
    // partial P(a, c) = sum_i Y_t(i, a) Z(tile i, c)
    double4_t pacc[4] = {{0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}};
    mm64(pacc, Bs, kLd, 1, As, 1, kLd, w, l15, kq);
    double* __restrict__ P = scr + (int64_t)(B.pslot + t) * kSlot;
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int v = 0; v < 4; ++v) P[(16 * c + l15) * kTile + 16 * w + kq + 4 * v] = pacc[c][v];
}

// Z(b, b) = T'T - sum_t P_t (lower triangle), zeros in the rows above it (the supernode's diagonal block's upper part)
__device__ __forceinline__ void write_diag_block(const SelinvBc& B, const double* __restrict__ Ts, int ldt,
                                                 const double* __restrict__ Gs, const double* __restrict__ parts, int nparts,
                                                 double* __restrict__ Z) {
    double* __restrict__ G = Z + B.px;
    for (int e = threadIdx.x; e < kSlot; e += kSThreads) {
        const int a = e & 63, c = e >> 6;
        if (a >= B.wb || c >= B.wb || a < c) continue;
        double s = 0.0;
        if (Gs) {   // small path: T'(T - G)
            for (int q = a; q < B.wb; ++q) s = fma(Ts[a * ldt + q], Ts[c * ldt + q] - Gs[c * kLd + q], s);
        } else {
            for (int q = a; q < B.wb; ++q) s = fma(Ts[a * ldt + q], Ts[c * ldt + q], s);
            for (int u = 0; u < nparts; ++u) s -= parts[(int64_t)u * kSlot + c * kTile + a];
        }
        G[(int64_t)(B.j0 + c) * B.r + B.j0 + a] = s;
    }
    for (int c = 0; c < B.wb; ++c)
        for (int i = threadIdx.x; i < B.j0 + c; i += kSThreads) G[(int64_t)(B.j0 + c) * B.r + i] = 0.0;
}

__global__ __launch_bounds__(kSThreads) void k_selinv_zbb(const SelinvBc* __restrict__ bcs, int d0,
                                                          const double* __restrict__ scr, double* __restrict__ Z) {
    __shared__ double Ts[kTile * kLd];
    const SelinvBc B = bcs[d0 + blockIdx.x];
    const double* __restrict__ T = scr + (int64_t)B.tslot * kSlot;
    for (int e = threadIdx.x; e < kSlot; e += kSThreads) Ts[(e >> 6) * kLd + (e & 63)] = T[e];
    __syncthreads();
    const int nparts = (B.m + kTile - 1) / kTile;
    write_diag_block(B, Ts, kLd, nullptr, scr + (int64_t)B.pslot * kSlot, nparts, Z);
}

// ---- small path: one workgroup per block column -------------------------------------------------------------------
__global__ __launch_bounds__(kSThreads) void k_selinv_small(const SelinvBc* __restrict__ bcs, int d0,
                                                            const double* __restrict__ L, const int64_t* __restrict__ cb,
                                                            const int64_t* __restrict__ mo, const int32_t* __restrict__ gmap,
                                                            double* __restrict__ Z) {
    __shared__ double M[kTile * kLd];          // T
    __shared__ double Buf[2 * kTile * kLdC];   // W | Zc (32-row chunks, ld kLdC), later L's chunk in W; at the end G
    const SelinvBc B = bcs[d0 + blockIdx.x];
    const int tid = threadIdx.x, ci = tid & (kChunk - 1), tg = tid >> 5;   // chunk row ci; columns tg + 8 u
    const double* __restrict__ Lp = L + B.px;
    double* __restrict__ Zp = Z + B.px;
    if (tid < 64) tinv64(M, Lp, B.r, B.j0, B.wb);
    __syncthreads();
    double* __restrict__ W = Buf;
    double* __restrict__ Zc = Buf + kTile * kLdC;
    const int p0 = B.j0 + B.wb;
    double g[16];
#pragma unroll
    for (int u = 0; u < 16; ++u) g[u] = 0.0;
    for (int i0 = 0; i0 < B.m; i0 += kChunk) {
        const int nr = min(kChunk, B.m - i0), p = p0 + i0 + ci;
        // W(ci, t) = sum_k Z(p, p0 + k) L(p0 + k, j0 + t)
        double acc[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) acc[u] = 0.0;
        if (ci < nr) {
            const int64_t pcb = cb[B.pi + p], pmo = mo[B.pi + p];
            for (int k = 0; k < B.m; ++k) {
                const int q = p0 + k;
                const double z = Z[p >= q ? zaddr(cb[B.pi + q], mo[B.pi + q], gmap, p) : zaddr(pcb, pmo, gmap, q)];
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const int tc = tg + 8 * u;
                    if (tc < B.wb) acc[u] = fma(z, Lp[(int64_t)(B.j0 + tc) * B.r + q], acc[u]);
                }
            }
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) W[(tg + 8 * u) * kLdC + ci] = acc[u];
        __syncthreads();
        // Zc(ci, c) = -sum_{t >= c} W(ci, t) T(t, c), stored to Z
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int c = tg + 8 * u;
            double s = 0.0;
            for (int q = c; q < B.wb; ++q) s = fma(W[q * kLdC + ci], M[c * kLd + q], s);
            const bool ok = ci < nr && c < B.wb;
            Zc[c * kLdC + ci] = ok ? -s : 0.0;
            if (ok) Zp[(int64_t)(B.j0 + c) * B.r + p] = -s;
        }
        __syncthreads();
        // L's chunk into W: W(ci, a) = L(p, j0 + a)
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int a = tg + 8 * u;
            W[a * kLdC + ci] = (ci < nr && a < B.wb) ? Lp[(int64_t)(B.j0 + a) * B.r + p] : 0.0;
        }
        __syncthreads();
        // G(a, c) += sum_i W(i, a) Zc(i, c): entries tid + 256 u
#pragma unroll
        for (int u = 0; u < 16; ++u) {
            const int e = tid + kSThreads * u, a = e & 63, c = e >> 6;
            double s = g[u];
            for (int i = 0; i < nr; ++i) s = fma(W[a * kLdC + i], Zc[c * kLdC + i], s);
            g[u] = s;
        }
        __syncthreads();
    }
    double* __restrict__ Gs = Buf;   // G(a, c) at Gs[c * kLd + a]
#pragma unroll
    for (int u = 0; u < 16; ++u) {
        const int e = tid + kSThreads * u;
        Gs[(e >> 6) * kLd + (e & 63)] = g[u];
    }
    __syncthreads();
    write_diag_block(B, M, kLd, Gs, nullptr, 0, Z);
}

// ---- diagonal and log-determinant ---------------------------------------------------------------------------------
__global__ __launch_bounds__(kSThreads) void k_selinv_diag(const double* __restrict__ Z, const int64_t* __restrict__ doff,
                                                           const int* __restrict__ perm, int n, double* __restrict__ diag) {
    const int i = blockIdx.x * kSThreads + threadIdx.x;
    if (i >= n) return;
    diag[perm ? perm[i] : i] = Z[doff[i]];
}

// First pass: workgroup b sums log L_jj over its contiguous range of columns (fixed lane split and tree), and finds the
// range's first column whose diagonal entry is not positive and finite.
__global__ __launch_bounds__(kSThreads) void k_logdet_part(const double* __restrict__ L, const int64_t* __restrict__ doff,
                                                           int n, double* __restrict__ part) {
    __shared__ double ss[kSThreads];
    __shared__ int sb[kSThreads];
    const int per = (n + gridDim.x - 1) / gridDim.x, lo = blockIdx.x * per, hi = min(n, lo + per);
    double s = 0.0;
    int bad = INT_MAX;
    for (int i = lo + threadIdx.x; i < hi; i += kSThreads) {
        const double v = L[doff[i]];
        if (v > 0.0 && v <= DBL_MAX) s += log(v);
        else bad = min(bad, i);
    }
    ss[threadIdx.x] = s;
    sb[threadIdx.x] = bad;
    __syncthreads();
    for (int o = kSThreads / 2; o; o >>= 1) {
        if (threadIdx.x < o) {
            ss[threadIdx.x] += ss[threadIdx.x + o];
            sb[threadIdx.x] = min(sb[threadIdx.x], sb[threadIdx.x + o]);
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        part[blockIdx.x] = ss[0];
        part[kLogParts + blockIdx.x] = sb[0] == INT_MAX ? -1.0 : (double)sb[0];
    }
}

// Second pass (one wave): the partials in order; out[0] = 2 sum (NaN on a bad column), out[1] = that column + 1, or 0.
__global__ void k_logdet_final(double* __restrict__ part, int nparts) {
    if (threadIdx.x != 0) return;
    double s = 0.0, bad = -1.0;
    for (int b = 0; b < nparts; ++b) {
        s += part[b];
        if (bad < 0 && part[kLogParts + b] >= 0) bad = part[kLogParts + b];
    }
    part[2 * kLogParts] = bad >= 0 ? __builtin_nan("") : 2.0 * s;
    part[2 * kLogParts + 1] = bad + 1.0;
}

// per column the offset of its diagonal entry, and the log-determinant's partials
int ensure_diag(parsy_plan* pl) {
    SelinvState& X = selinv_state(pl);
    if (X.diag_ready) return 0;
    const Schedule& S = pl->S;
    std::vector<int64_t> doff((size_t)S.n);
    for (int s = 0; s < S.nsuper; ++s)
        for (int q = 0; q < S.sn[s].w; ++q) doff[S.sn[s].c0 + q] = S.sn[s].px + (int64_t)q * S.sn[s].r + q;
    PARSY_HIP(hipSetDevice(pl->device));
    DevicePool pool(&X.diag_meter);
    int64_t* d_doff = pool.upload(doff);
    double* d_lpart = pool.alloc<double>(2 * kLogParts + 2);
    if (pool.error() != hipSuccess) return pool_failed(pool);
    X.diag = std::move(pool);
    X.d_doff = d_doff, X.d_lpart = d_lpart;
    X.diag_ready = true;
    return 0;
}

// the host schedule, the map on the device, and the split under the current threshold (descriptors, scratch)
int ensure_selinv(parsy_plan* pl) {
    SelinvState& X = selinv_state(pl);
    PARSY_HIP(hipSetDevice(pl->device));
    if (!X.map_ready) {
        std::string what;
        SelinvSchedule sched;
        if (!build_selinv(pl->S, sched, what)) return set_last_error("parsy_selinv_device: " + what), -1;
        int64_t task_cap = 0;
        for (int b = 0; b < sched.nbc; ++b) {
            const SnDesc& d = pl->S.sn[sched.bc_sn[b]];
            const int j0 = sched.bc_j[b] * kTile;
            task_cap += (d.r - j0 - std::min(kTile, d.w - j0) + kTile - 1) / kTile;
        }
        DevicePool pool(&X.meter);
        int64_t *d_cb = pool.upload(sched.cb), *d_mo = pool.upload(sched.mo);
        int32_t* d_gmap = pool.upload(sched.gmap);
        SelinvBc* d_bcs = pool.alloc<SelinvBc>(std::max(sched.nbc, 1));
        int32_t* d_tasks = pool.alloc<int32_t>(std::max<int64_t>(2 * task_cap, 1));
        if (pool.error() != hipSuccess) return pool_failed(pool);
        X.map = std::move(pool);
        X.X = std::move(sched);
        X.d_cb = d_cb, X.d_mo = d_mo, X.d_gmap = d_gmap, X.d_bcs = d_bcs, X.d_tasks = d_tasks;
        X.task_cap = task_cap;
        X.map_ready = true;
    }
    const int tmin = selinv_tiled_min();
    if (X.sp.tiled_min != tmin) {
        if (X.used) PARSY_HIP(hipDeviceSynchronize());   // (an earlier call may still read the descriptors and the scratch)
        // (the split counts as made only when its descriptors and the scratch are on the device)
        split_selinv(pl->S, X.X, tmin, X.sp);
        X.sp.tiled_min = -1;
        if (!X.sp.bcs.empty())
            PARSY_HIP(hipMemcpy(X.d_bcs, X.sp.bcs.data(), X.sp.bcs.size() * sizeof(SelinvBc), hipMemcpyHostToDevice));
        if (!X.sp.tasks.empty())
            PARSY_HIP(hipMemcpy(X.d_tasks, X.sp.tasks.data(), X.sp.tasks.size() * sizeof(int32_t), hipMemcpyHostToDevice));
        PARSY_HIP(X.d_scr.grow(X.sp.scratch_slots * kSlot));
        X.sp.tiled_min = tmin;
    }
    return 0;
}

}  // namespace

SelinvState& selinv_state(parsy_plan* pl) {
    if (!pl->selinv) pl->selinv = std::make_unique<SelinvState>(&pl->meter);
    return *pl->selinv;
}

int plan_selinv(parsy_plan* pl, const double* d_L, double* d_z, hipStream_t stream) {
    const char* who = "parsy_selinv_device";
    if (check_plan(pl, who, kNeedsIdle) != 0) return -1;
    const int64_t xs = pl->S.xsize;
    if (d_z < d_L + xs && d_L < d_z + xs) return set_last_error(std::string(who) + ": d_z overlaps d_lValues"), -1;
    if (ensure_selinv(pl) != 0) return -1;
    SelinvState& X = *pl->selinv;
    const SelinvSplit& sp = X.sp;
    X.used = true;
    double* const scr = X.d_scr.data();
    for (int l = 0; l < X.X.levels; ++l) {
        const int d0 = sp.lvl_bc[l], nt = sp.lvl_ntiled[l], nsm = sp.lvl_bc[l + 1] - d0 - nt;
        const int t0 = sp.lvl_task[l], ntask = sp.lvl_task[l + 1] - t0;
        if (nt > 0) hipLaunchKernelGGL(k_selinv_tinv, dim3(nt), dim3(64), 0, stream, X.d_bcs, d0, d_L, scr);
        if (ntask > 0) {
            hipLaunchKernelGGL(k_selinv_y, dim3(ntask), dim3(kSThreads), 0, stream, X.d_bcs, X.d_tasks + 2 * t0, d_L,
                               scr);
            hipLaunchKernelGGL(k_selinv_z, dim3(ntask), dim3(kSThreads), 0, stream, X.d_bcs, X.d_tasks + 2 * t0,
                               X.d_cb, X.d_mo, X.d_gmap, d_z, scr);
        }
        if (nt > 0) hipLaunchKernelGGL(k_selinv_zbb, dim3(nt), dim3(kSThreads), 0, stream, X.d_bcs, d0, scr, d_z);
        if (nsm > 0)
            hipLaunchKernelGGL(k_selinv_small, dim3(nsm), dim3(kSThreads), 0, stream, X.d_bcs, d0 + nt, d_L, X.d_cb,
                               X.d_mo, X.d_gmap, d_z);
    }
    PARSY_HIP(hipGetLastError());
    return 0;
}

int plan_inverse_diag(parsy_plan* pl, const double* d_z, double* d_diag, hipStream_t stream) {
    if (check_plan(pl, "parsy_inverse_diag_device", kNeedsIdle) != 0) return -1;
    PARSY_HIP(hipSetDevice(pl->device));
    const int* perm = nullptr;
    if (ensure_diag(pl) != 0 || plan_perm_device(pl, &perm) != 0) return -1;
    const int n = pl->S.n;
    if (n > 0)
        hipLaunchKernelGGL(k_selinv_diag, dim3((n + kSThreads - 1) / kSThreads), dim3(kSThreads), 0, stream, d_z,
                           pl->selinv->d_doff, perm, n, d_diag);
    PARSY_HIP(hipGetLastError());
    return 0;
}

int plan_logdet(parsy_plan* pl, const double* d_L, double* logdet, hipStream_t stream) {
    if (check_plan(pl, "parsy_logdet_device", kNeedsIdle) != 0) return -1;
    PARSY_HIP(hipSetDevice(pl->device));
    if (ensure_diag(pl) != 0) return -1;
    SelinvState& X = *pl->selinv;
    const int n = pl->S.n;
    const int nparts = std::max(1, std::min(kLogParts, (n + kSThreads - 1) / kSThreads));
    hipLaunchKernelGGL(k_logdet_part, dim3(nparts), dim3(kSThreads), 0, stream, d_L, X.d_doff, n, X.d_lpart);
    hipLaunchKernelGGL(k_logdet_final, dim3(1), dim3(64), 0, stream, X.d_lpart, nparts);
    PARSY_HIP(hipGetLastError());
    double out[2];
    PARSY_HIP(hipMemcpyAsync(out, X.d_lpart + 2 * kLogParts, sizeof(out), hipMemcpyDeviceToHost, stream));
    PARSY_HIP(hipStreamSynchronize(stream));
    *logdet = out[0];
    return (int)out[1];
}

}  // namespace parsy

using parsy::set_last_error;

extern "C" {

int parsy_selinv_get_info(parsy_plan* pl, parsy_selinv_info* info) {
    if (!pl || !info) {
        set_last_error("parsy_selinv_get_info: null argument");
        return -1;
    }
    const parsy::Schedule& S = pl->S;
    parsy::SelinvSchedule own;
    const parsy::SelinvSchedule* X = nullptr;
    if (pl->selinv && pl->selinv->map_ready) {
        X = &pl->selinv->X;
    } else {
        std::string what;
        if (!parsy::build_selinv(S, own, what)) {
            set_last_error("parsy_selinv_get_info: " + what);
            return -1;
        }
        X = &own;
    }
    parsy::SelinvSplit sp;
    parsy::split_selinv(S, *X, parsy::selinv_tiled_min(), sp);
    info->levels = X->levels;
    info->block_columns = X->nbc;
    info->tiled_block_columns = sp.ntiled;
    info->launches = sp.launches;
    info->flops = X->flops;
    info->device_bytes = pl->selinv ? pl->selinv->meter.bytes : 0;
    return 0;
}

int parsy_selinv_device(parsy_plan* pl, const double* d_lValues, double* d_z, void* stream) {
    if (!pl || !d_lValues || !d_z) {
        set_last_error("parsy_selinv_device: null argument");
        return -1;
    }
    return parsy::plan_selinv(pl, d_lValues, d_z, (hipStream_t)stream);
}

int parsy_inverse_diag_device(parsy_plan* pl, const double* d_z, double* d_diag, void* stream) {
    if (!pl || !d_z || !d_diag) {
        set_last_error("parsy_inverse_diag_device: null argument");
        return -1;
    }
    return parsy::plan_inverse_diag(pl, d_z, d_diag, (hipStream_t)stream);
}

int parsy_logdet_device(parsy_plan* pl, const double* d_lValues, double* logdet, void* stream) {
    if (!pl || !d_lValues || !logdet) {
        set_last_error("parsy_logdet_device: null argument");
        return -1;
    }
    return parsy::plan_logdet(pl, d_lValues, logdet, (hipStream_t)stream);
}

}  // extern "C"
