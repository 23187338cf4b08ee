// HIP kernels around the solves for gfx950 that are no sweep in one direction: the inverse diagonal blocks, X between
// its two layouts, the right-hand side b = L * 1 and the segment copy of the multi-GPU exchange.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "launch.hpp"
#include "trsv_device.hpp"

namespace parsy {

// DIAG_INVERSE: inverse of every 64x64 diagonal block of the wide supernodes (what the chain kernels multiply
// by: x_jb = inv(L_jj) t).  One wave per block, in place in LDS, by halves:
//     inv [A 0; B C] = [inv A, 0; -inv(C) B inv(A), inv C]
// -- the four 16x16 diagonal sub-blocks by substitution (one column per lane), then the 16x16 and the 32x32
// off-diagonal blocks as products on the matrix cores (v_mfma_f64_16x16x4_f64, operands from LDS): 16 block
// products instead of a 64-step substitution whose longest column is a chain of two thousand dependent
// multiply-adds.  dinv[(dslot + jb) * 4096 + c * 64 + i] = inv(L_jj)[i][c], zeros above the diagonal; a block
// narrower than 64 is padded with an identity.
__global__ __launch_bounds__(64) void k_diag_inverse(const SnDesc* __restrict__ sn,
                                                     const int32_t* __restrict__ list,
                                                     const double* __restrict__ L,
                                                     double* __restrict__ dinv) {
    __shared__ double M[kTile * kLdDiag];
    const SnDesc D = sn[list[2 * blockIdx.x]];   // one workgroup per (supernode, block column) pair of the list
    const int jb = list[2 * blockIdx.x + 1], lane = threadIdx.x;
    const int l15 = lane & 15, kq = lane >> 4;
    const int r = D.r, cb = jb * kTile, wbk = min(kTile, D.w - cb);
    const double* __restrict__ G = L + D.px;
    {
        // column cc, row `lane`: all 64 loads in flight together (unconditional: clamped to the block, then masked)
        double v[kTile];
        const double* __restrict__ src = G + (int64_t)cb * r + cb + min(lane, wbk - 1);
#pragma unroll
        for (int cc = 0; cc < kTile; ++cc) v[cc] = src[(int64_t)min(cc, wbk - 1) * r];
#pragma unroll
        for (int cc = 0; cc < kTile; ++cc)
            M[cc * kLdDiag + lane] = (cc < wbk && lane < wbk && lane >= cc) ? v[cc] : (lane == cc ? 1.0 : 0.0);
    }
    __builtin_amdgcn_wave_barrier();   // (one wave: its LDS operations complete in order)
    auto blk = [&](int bi, int bj) { return M + (16 * bj) * kLdDiag + 16 * bi; };   // 16x16 block (bi, bj)
    {
        // the four diagonal sub-blocks: lane (b = kq, c = l15) forms column c of inv(L_bb) and writes it in place
        double* __restrict__ B = blk(kq, kq);
        double y[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) y[k] = 0.0;
#pragma unroll
        for (int rr = 0; rr < 16; ++rr) {
            double sacc = (rr == l15) ? -1.0 : 0.0;
#pragma unroll
            for (int k = 0; k < rr; ++k) sacc = fma(B[k * kLdDiag + rr], y[k], sacc);
            y[rr] = (rr >= l15) ? -sacc / B[rr * kLdDiag + rr] : 0.0;
        }
        __builtin_amdgcn_s_waitcnt(0);   // every read of the sub-blocks precedes the in-place writes
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int rr = 0; rr < 16; ++rr) B[l15 * kLdDiag + rr] = y[rr];
    }
    __builtin_amdgcn_wave_barrier();
    const double4_t zero = {0, 0, 0, 0};
    // the two 32x32 diagonal blocks: block (b+1, b) := -inv(L_{b+1,b+1}) L_{b+1,b} inv(L_bb), b = 0, 2
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
    // the 32x32 block below: X := -inv(C) B inv(A), A = blocks (0..1, 0..1), C = blocks (2..3, 2..3), both inverted
    {
        // T = B inv(A): T_i0 = B_i0 A00 + B_i1 A10, T_i1 = B_i1 A11  (i = 2, 3)
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
        // X = -inv(C) T: X_2j = -C22 T_2j, X_3j = -(C32 T_2j + C33 T_3j)
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
    double* __restrict__ out = dinv + (int64_t)(D.dslot + jb) * (kTile * kTile);
    for (int e = lane; e < kTile * kTile; e += 64) {
        const int cc = e >> 6, i = e & 63;
        out[e] = (i >= cc) ? M[cc * kLdDiag + i] : 0.0;
    }
}

void launch_diag_inverse(const DevicePattern& P, int count, const double* L, double* dinv, hipStream_t stream) {
    if (count <= 0) return;
    launch_witnessed<k_diag_inverse, kWDiagInverse>(dim3(count), dim3(64), 0, stream, P.sn, P.solve_wide_list, L, dinv);
}

// X between its two layouts: right-hand-side-major a[q * lda + row] <-> row-major b[row * ldb + q] (64 x 64 tiles
// through LDS: both sides in 512-byte runs).  to_rows: a -> b, otherwise b -> a.
__global__ __launch_bounds__(kThreads) void k_transpose_x(double* __restrict__ a, int64_t lda, double* __restrict__ b,
                                                          int64_t ldb, int n, int nrhs, int to_rows) {
    __shared__ double T[64][65];
    const int tid = threadIdx.x, lo = tid & 63, hi = tid >> 6;
    const int row0 = 64 * (int)blockIdx.x, q0 = 64 * (int)blockIdx.y;
    if (to_rows) {
#pragma unroll
        for (int u = 0; u < 16; ++u) {
            const int q = q0 + hi + 4 * u, row = row0 + lo;
            T[hi + 4 * u][lo] = (q < nrhs && row < n) ? a[(int64_t)q * lda + row] : 0.0;
        }
        __syncthreads();
#pragma unroll
        for (int u = 0; u < 16; ++u) {
            const int row = row0 + hi + 4 * u, q = q0 + lo;
            if (row < n && q < nrhs) b[(int64_t)row * ldb + q] = T[lo][hi + 4 * u];
        }
    } else {
#pragma unroll
        for (int u = 0; u < 16; ++u) {
            const int row = row0 + hi + 4 * u, q = q0 + lo;
            T[lo][hi + 4 * u] = (row < n && q < nrhs) ? b[(int64_t)row * ldb + q] : 0.0;
        }
        __syncthreads();
#pragma unroll
        for (int u = 0; u < 16; ++u) {
            const int q = q0 + hi + 4 * u, row = row0 + lo;
            if (q < nrhs && row < n) a[(int64_t)q * lda + row] = T[hi + 4 * u][lo];
        }
    }
}
void launch_transpose_x(double* x, int64_t ldx, double* xt, int64_t ldq, int n, int nrhs, bool to_rows, hipStream_t stream) {
    if (n <= 0 || nrhs <= 0) return;
    launch_witnessed<k_transpose_x, kWTransposeX>(dim3((n + 63) / 64, (nrhs + 63) / 64), dim3(kThreads), 0, stream, x,
        ldx, xt, ldq, n, nrhs, to_rows ? 1 : 0);
}

// b = L * 1 on the stored structure (the reference's rhsInitBlocked, common/Util.h:277-288: the right-hand
// side its triangularTest solves, so that x = 1): every stored entry of a panel row is added to b[row].
// One thread per panel row (lanes along the rows: coalesced column by column), rows of a tall panel
// spread over gridDim.y workgroups.  b must be zero on entry.
__global__ __launch_bounds__(kThreads) void k_rhs_ones(const SnDesc* __restrict__ sn,
                                                       const int32_t* __restrict__ rows,
                                                       const double* __restrict__ L, double* __restrict__ b) {
    const SnDesc D = sn[blockIdx.x];
    const double* __restrict__ G = L + D.px;
    for (int i = blockIdx.y * kThreads + threadIdx.x; i < D.r; i += gridDim.y * kThreads) {
        const int cmax = min(D.w, i + 1);  // the diagonal block is lower triangular
        double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
        int c = 0;
        for (; c + 4 <= cmax; c += 4) {
            s0 += G[(int64_t)c * D.r + i];
            s1 += G[(int64_t)(c + 1) * D.r + i];
            s2 += G[(int64_t)(c + 2) * D.r + i];
            s3 += G[(int64_t)(c + 3) * D.r + i];
        }
        for (; c < cmax; ++c) s0 += G[(int64_t)c * D.r + i];
        atomicAdd(&b[rows[D.pi + i]], (s0 + s1) + (s2 + s3));
    }
}

void launch_rhs_ones(const DevicePattern& P, int nsuper, int max_rows, const double* L, double* b,
                     hipStream_t stream) {
    if (nsuper <= 0) return;
    const int ny = std::max(1, std::min(16, (max_rows + kThreads - 1) / kThreads));
    launch_witnessed<k_rhs_ones, kWRhsOnes>(dim3(nsuper, ny), dim3(kThreads), 0, stream, P.sn, P.rows, L, b);
}

// Copy contiguous runs of doubles between two device buffers: dst[dst_off[q] + i] = src[src_off[q] + i],
// i < len[q].  The multi-GPU exchange packs with it the rows of a subtree's panels that the root part
// reads (the tail of every panel column) and unpacks them on the receiving rank.
__global__ __launch_bounds__(64) void k_copy_segments(double* __restrict__ dst, const double* __restrict__ src,
                                                      const int64_t* __restrict__ dst_off,
                                                      const int64_t* __restrict__ src_off,
                                                      const int32_t* __restrict__ len, int64_t nseg) {
    for (int64_t q = blockIdx.x; q < nseg; q += gridDim.x) {
        const double* __restrict__ s = src + src_off[q];
        double* __restrict__ d = dst + dst_off[q];
        const int n = len[q];
        for (int i = threadIdx.x; i < n; i += 64) d[i] = s[i];
    }
}

void launch_copy_segments(double* dst, const double* src, const int64_t* dst_off, const int64_t* src_off,
                          const int32_t* len, int64_t nseg, hipStream_t stream) {
    if (nseg <= 0) return;
    const unsigned grid = (unsigned)std::min<int64_t>(nseg, 1 << 20);
    launch_witnessed<k_copy_segments, kWCopySegments>(dim3(grid), dim3(64), 0, stream, dst, src, dst_off, src_off, len,
        nseg);
}

}  // namespace parsy
