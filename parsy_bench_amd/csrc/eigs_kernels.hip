// The kernels of parsy_eigs_device (eigs.hpp) and their launches: the tall-skinny Gram product C = X'Y on the matrix
// cores, the rotation Z = beta Z + alpha X C, the products Y = A X and Y = M X as one more epilogue of the symmetric
// sweep (sym_sweep.hpp), and the column maxima behind eta.  No flag, no ticket, no wait and no atomic: the stream is the
// only order between launches, every sum runs in a fixed order, and the number of partial sums depends on n alone, so
// the same inputs and the same solve results give the same bits.
//
// Traffic: k_eigs_gram reads 8 n (p + q) bytes once (its partials are nchunks p q doubles, nchunks <= 256);
// k_eigs_rotate reads 8 n p and reads and writes 8 n q.  Both are bound by that.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "../../include/parsy_amd.h"
#include "device_util.hpp"
#include "eigs.hpp"
#include "errors.hpp"
#include "executor.hpp"
#include "feature_states.hpp"
#include "hip_check.hpp"
#include "kernels.hpp"
#include "plan_util.hpp"
#include "refine.hpp"
#include "sym_sweep.hpp"

namespace parsy {

namespace {

constexpr int kEThreads = kRefineThreads;
constexpr int kGramStage = 16;       // rows of X and Y a workgroup holds in LDS at a time
constexpr int kGramLd = 18;          // their leading dimension there: lane (column c, row k) reads word 18 c + k, and
                                     // 2 (18 c + k) mod 64 is different for the 32 lanes of a half-wave (c < 16, k < 2)
constexpr int kGramChunkRows = 256;  // fewest rows of a chunk
constexpr int kGramMaxChunks = 256;  // most chunks = partial sums per entry of C
constexpr int kGramCols = 2 * kEigsMaxBasis;   // most columns of X and Y together
constexpr int kGramLoads = kGramCols * kGramStage / kEThreads;   // per thread and stage

static_assert(kEigsMaxBasis == 128 && kEThreads == 256 && kGramStage == 16, "k_eigs_gram: 4 waves x 2 tile rows x 8 tile columns");

// Y = A X: the sweep's sum itself
struct ProductOut : SweepScale {
    __device__ __forceinline__ u64 operator()(double* y, bool first, double, double acc, double, const double*) const {
        if (first) *y = acc;
        return 0;
    }
};

// rows of a chunk and the number of chunks, from n alone
inline void gram_chunks(int n, int* rows, int* chunks) {
    int c = std::max(1, std::min(kGramMaxChunks, (n + kGramChunkRows - 1) / kGramChunkRows));
    int r = (n + c - 1) / c;
    r = std::max(kGramStage, (r + kGramStage - 1) / kGramStage * kGramStage);
    *rows = r;
    *chunks = std::max(1, (n + r - 1) / r);
}

// First phase of C = X'Y (X n x p, Y n x q, leading dimension n, p and q <= 128): workgroup b sums the rows of chunk b,
// 16 at a time through LDS (columns past p or q and rows past n are zeros there), with v_mfma_f64_16x16x4_f64: the A
// operand of lane l is X[row 4 s + (l >> 4), column 16 ti + (l & 15)], the B operand Y[same row, column 16 tj + (l & 15)],
// the result's column (of Y) is l & 15 and its rows (columns of X) are (l >> 4) + 4 reg.  Wave w owns the tile rows w
// and w + 4 and every tile column: 16 accumulators.  The next stage's global loads are in flight while this one is
// multiplied.  part[b][j pp + i] (pp = p rounded up to 16) holds the chunk's sums.
__global__ __launch_bounds__(kEThreads) void k_eigs_gram(const double* __restrict__ X, int p, const double* __restrict__ Y,
                                                         int q, int n, int chunk_rows, double* __restrict__ part) {
    __shared__ double sm[kGramCols * kGramLd];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, l15 = lane & 15, kq = lane >> 4;
    const int nti = (p + 15) >> 4, ntj = (q + 15) >> 4, pp = nti * 16, qp = ntj * 16, cols = pp + qp;
    const int64_t r0 = (int64_t)blockIdx.x * chunk_rows;
    const int64_t r1 = r0 + chunk_rows < n ? r0 + chunk_rows : (int64_t)n;
    const int lr = tid & 15, lc = tid >> 4;   // this thread's row of a stage and its first column (then every 16th)
    double4_t acc[2][8];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 8; ++b) acc[a][b] = double4_t{0.0, 0.0, 0.0, 0.0};
    double v[kGramLoads];
    auto fetch = [&](int64_t row0) {
        const int64_t row = row0 + lr;
#pragma unroll
        for (int u = 0; u < kGramLoads; ++u) {
            const int c = lc + 16 * u;
            double x = 0.0;
            if (c < cols && row < r1) {
                if (c < pp) {
                    if (c < p) x = X[row + (int64_t)c * n];
                } else if (c - pp < q) {
                    x = Y[row + (int64_t)(c - pp) * n];
                }
            }
            v[u] = x;
        }
    };
    fetch(r0);
    for (int64_t row0 = r0; row0 < r1; row0 += kGramStage) {
        __syncthreads();   // (the products of the stage before have read sm)
#pragma unroll
        for (int u = 0; u < kGramLoads; ++u) {
            const int c = lc + 16 * u;
            if (c < cols) sm[c * kGramLd + lr] = v[u];
        }
        __syncthreads();
        if (row0 + kGramStage < r1) fetch(row0 + kGramStage);
        if (w < nti) {
            const bool two = w + 4 < nti;
#pragma unroll
            for (int s = 0; s < kGramStage / 4; ++s) {
                const int k = 4 * s + kq;
                const double a0 = sm[(16 * w + l15) * kGramLd + k];
                const double a1 = two ? sm[(16 * (w + 4) + l15) * kGramLd + k] : 0.0;
#pragma unroll
                for (int tj = 0; tj < 8; ++tj) {
                    if (tj < ntj) {
                        const double b = sm[(pp + 16 * tj + l15) * kGramLd + k];
                        acc[0][tj] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b, acc[0][tj], 0, 0, 0);
                        if (two) acc[1][tj] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b, acc[1][tj], 0, 0, 0);
                    }
                }
            }
        }
    }
    double* out = part + (int64_t)blockIdx.x * pp * qp;
#pragma unroll
    for (int a = 0; a < 2; ++a) {
        const int ti = w + 4 * a;
        if (ti < nti) {
#pragma unroll
            for (int tj = 0; tj < 8; ++tj) {
                if (tj < ntj) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) out[(int64_t)(16 * tj + l15) * pp + 16 * ti + kq + 4 * r] = acc[a][tj][r];
                }
            }
        }
    }
}

// Second phase: C[i, j] = the chunks' sums of entry (i, j), added in chunk order
__global__ __launch_bounds__(kEThreads) void k_eigs_gram_reduce(const double* __restrict__ part, int chunks, int pp, int p,
                                                                int q, double* __restrict__ C, int ldc) {
    const int e = blockIdx.x * kEThreads + threadIdx.x;
    const int i = e % pp, j = e / pp;
    if (i >= p || j >= q) return;
    const int64_t len = (int64_t)pp * ((q + 15) & ~15);
    double s = 0.0;
    for (int b = 0; b < chunks; ++b) s += part[(int64_t)b * len + e];
    C[(int64_t)j * ldc + i] = s;
}

// Z = beta Z + alpha X C: X n x p (p <= 128), C p x q in global memory (leading dimension ldc), Q >= q columns padded
// with zeros in LDS; a thread owns a row and sums over the columns of X in ascending order.  Rows are independent.  Z
// and X must be different memory: a thread writes columns of its row that other threads' rows never touch, but the
// caller's "in place" would make X's column c the output too, so the restart rotates into a spare slab instead
// (eigs.hpp) and no call passes Z == X.
template <int Q>
__global__ __launch_bounds__(kEThreads) void k_eigs_rotate(double* __restrict__ Z, double beta, double alpha,
                                                           const double* __restrict__ X, int p, const double* __restrict__ C,
                                                           int ldc, int q, int n) {
    __shared__ double cs[kEigsMaxBasis * Q];
    for (int e = threadIdx.x; e < p * Q; e += kEThreads) {
        const int j = e / Q, c = e % Q;
        cs[e] = c < q ? C[(int64_t)c * ldc + j] : 0.0;
    }
    __syncthreads();
    const int64_t row = (int64_t)blockIdx.x * kEThreads + threadIdx.x;
    if (row >= n) return;
    double acc[Q];
#pragma unroll
    for (int c = 0; c < Q; ++c) acc[c] = 0.0;
#pragma unroll 4
    for (int j = 0; j < p; ++j) {
        const double x = X[row + (int64_t)j * n];
#pragma unroll
        for (int c = 0; c < Q; ++c) acc[c] = fma(x, cs[j * Q + c], acc[c]);
    }
#pragma unroll
    for (int c = 0; c < Q; ++c)
        if (c < q) store_y(Z + row + (int64_t)c * n, alpha, beta, acc[c]);
}

// Partial maxima of column c = blockIdx.y: of |ay - theta[c] my| (my null: of |ay|) and of |y|
__global__ __launch_bounds__(kEThreads) void k_eigs_colmax(const double* __restrict__ ay, const double* __restrict__ my,
                                                           const double* __restrict__ theta, const double* __restrict__ y,
                                                           int n, u64* __restrict__ part_r, u64* __restrict__ part_y) {
    __shared__ u64 sm[4];
    const int c = blockIdx.y;
    const double th = my ? theta[c] : 0.0;
    u64 mr = 0, myy = 0;
    for (int64_t row = (int64_t)blockIdx.x * kEThreads + threadIdx.x; row < n; row += (int64_t)gridDim.x * kEThreads) {
        const int64_t i = row + (int64_t)c * n;
        const double r = my ? fma(-th, my[i], ay[i]) : ay[i];
        mr = max(mr, abs_bits(r));
        myy = max(myy, abs_bits(y[i]));
    }
    mr = block_max(mr, sm);
    myy = block_max(myy, sm);
    if (threadIdx.x == 0) {
        part_r[(int64_t)c * gridDim.x + blockIdx.x] = mr;
        part_y[(int64_t)c * gridDim.x + blockIdx.x] = myy;
    }
}

// eta of column c = blockIdx.x from nb partials per column
__global__ __launch_bounds__(kEThreads) void k_eigs_eta(const u64* __restrict__ part_r, const u64* __restrict__ part_y, int nb,
                                                        const double* __restrict__ theta, const double* __restrict__ norms,
                                                        double* __restrict__ eta) {
    __shared__ u64 sm[4];
    const int c = blockIdx.x;
    u64 mr = 0, myy = 0;
    for (int b = threadIdx.x; b < nb; b += kEThreads) {
        mr = max(mr, part_r[(int64_t)c * nb + b]);
        myy = max(myy, part_y[(int64_t)c * nb + b]);
    }
    mr = block_max(mr, sm);
    myy = block_max(myy, sm);
    if (threadIdx.x != 0) return;
    const double r = __longlong_as_double((long long)mr), yy = __longlong_as_double((long long)myy);
    eta[c] = r / ((norms[0] + fabs(theta[c]) * norms[1]) * yy);
}

// *out = the largest of nb partials (k_sym_norm1's); nb == 0: 1, the identity's norm
__global__ __launch_bounds__(kEThreads) void k_eigs_norm(const u64* __restrict__ part, int nb, double* __restrict__ out) {
    __shared__ u64 sm[4];
    u64 v = 0;
    for (int b = threadIdx.x; b < nb; b += kEThreads) v = max(v, part[b]);
    v = block_max(v, sm);
    if (threadIdx.x == 0) *out = nb == 0 ? 1.0 : __longlong_as_double((long long)v);
}

}  // namespace

int eigs_ensure(parsy_plan* pl, int max_basis, bool with_m) {
    if (!pl->eigs) pl->eigs = std::make_unique<EigsState>(&pl->meter);
    EigsState& E = *pl->eigs;
    const RefineState& R = *pl->refine;
    const int64_t n = pl->S.n;
    int rows = 0, chunks = 0;
    gram_chunks((int)n, &rows, &chunks);
    const int64_t pad = (max_basis + 15) & ~15;
    PARSY_HIP(hipSetDevice(pl->device));
    PARSY_HIP(E.vf_a.grow(std::max<int64_t>(R.nnz_full, 1)));
    if (with_m) PARSY_HIP(E.vf_m.grow(std::max<int64_t>(R.nnz_full, 1)));
    PARSY_HIP(E.basis.grow((with_m ? 3 : 2) * n * max_basis));
    PARSY_HIP(E.blocks.grow((int64_t)kEigsBlocks * n * kEigsMaxBlock));
    PARSY_HIP(E.gram.grow((int64_t)chunks * pad * pad));
    PARSY_HIP(E.dense.grow(EigsDense::size));
    PARSY_HIP(E.part.grow((int64_t)2 * kEigsMaxBasis * kRefinePartials));
    PARSY_HIP(E.ctl.grow(2));
    return 0;
}

int eigs_gram_enqueue(parsy_plan* pl, const double* X, int p, const double* Y, int q, double* C, int ldc, hipStream_t stream) {
    EigsState& E = *pl->eigs;
    const int n = pl->S.n;
    int rows = 0, chunks = 0;
    gram_chunks(n, &rows, &chunks);
    const int pp = (p + 15) & ~15, qp = (q + 15) & ~15;
    if (p < 1 || q < 1 || p > kEigsMaxBasis || q > kEigsMaxBasis || (int64_t)chunks * pp * qp > E.gram.size())
        return set_last_error("parsy_eigs_device: a Gram product outside its workspace (internal error)"), -1;
    hipLaunchKernelGGL(k_eigs_gram, dim3(chunks), dim3(kEThreads), 0, stream, X, p, Y, q, n, rows, E.gram.data());
    hipLaunchKernelGGL(k_eigs_gram_reduce, dim3((pp * qp + kEThreads - 1) / kEThreads), dim3(kEThreads), 0, stream,
                       E.gram.data(), chunks, pp, p, q, C, ldc);
    PARSY_HIP(hipGetLastError());
    return 0;
}

int eigs_rotate_enqueue(parsy_plan* pl, double* Z, double beta, double alpha, const double* X, int p, const double* C, int ldc,
                        int q, hipStream_t stream) {
    const int n = pl->S.n;
    if (p < 0 || p > kEigsMaxBasis || q < 1 || q > kEigsMaxBlock || Z == X)
        return set_last_error("parsy_eigs_device: a rotation outside its shapes (internal error)"), -1;
    if (n == 0) return 0;
    const dim3 grid((unsigned)((n + kEThreads - 1) / kEThreads));
    const int Q = q <= 1 ? 1 : q <= 4 ? 4 : q <= 8 ? 8 : 16;
    dispatch_int(Q, std::integer_sequence<int, 1, 4, 8, 16>(), [&](auto qq) {
        hipLaunchKernelGGL(k_eigs_rotate<decltype(qq)::value>, grid, dim3(kEThreads), 0, stream, Z, beta, alpha, X, p, C, ldc,
                           q, n);
    });
    PARSY_HIP(hipGetLastError());
    return 0;
}

int eigs_product_enqueue(parsy_plan* pl, const double* vf, const double* X, double* Y, int ncols, hipStream_t stream) {
    EigsState& E = *pl->eigs;
    if (ncols < 1 || ncols > kEigsMaxBasis)
        return set_last_error("parsy_eigs_device: a product outside its shapes (internal error)"), -1;
    // (the sweep reads its b operand and writes partial maxima: X stands in for the one, the second set takes the other)
    return sym_sweep_enqueue<ProductOut>(pl, vf, X, X, Y, ncols, E.part.data() + (int64_t)kEigsMaxBasis * kRefinePartials,
                                         stream) < 0
               ? -1
               : 0;
}

int eigs_norm_enqueue(parsy_plan* pl, const double* vf, double* out, hipStream_t stream) {
    EigsState& E = *pl->eigs;
    const RefineState& R = *pl->refine;
    const int n = pl->S.n;
    int nb = 0;
    if (vf) {
        nb = sym_sweep_blocks(n, kEThreads / R.group);
        dispatch_int(R.group, SweepGroups(), [&](auto g) {
            hipLaunchKernelGGL(k_sym_norm1<decltype(g)::value>, dim3(nb), dim3(kEThreads), 0, stream, R.d_rp, vf, n,
                               E.part.data());
        });
    }
    hipLaunchKernelGGL(k_eigs_norm, dim3(1), dim3(kEThreads), 0, stream, E.part.data(), nb, out);
    PARSY_HIP(hipGetLastError());
    return 0;
}

int eigs_eta_enqueue(parsy_plan* pl, const double* ay, const double* my, const double* y, int ncols, const double* theta,
                     const double* norms, double* eta, hipStream_t stream) {
    EigsState& E = *pl->eigs;
    const int n = pl->S.n;
    if (ncols < 1 || ncols > kEigsMaxBlock)
        return set_last_error("parsy_eigs_device: column maxima outside their shapes (internal error)"), -1;
    const int nb = sym_sweep_blocks(n, kEThreads);
    u64 *part_r = E.part.data(), *part_y = part_r + (int64_t)kEigsMaxBlock * kRefinePartials;
    hipLaunchKernelGGL(k_eigs_colmax, dim3(nb, ncols), dim3(kEThreads), 0, stream, ay, my, theta, y, n, part_r, part_y);
    hipLaunchKernelGGL(k_eigs_eta, dim3(ncols), dim3(kEThreads), 0, stream, part_r, part_y, nb, theta, norms, eta);
    PARSY_HIP(hipGetLastError());
    return 0;
}

}  // namespace parsy

extern "C" int parsy_eigs_get_info(parsy_plan* pl, parsy_eigs_info* info) {
    if (!pl || !info) {
        parsy::set_last_error("parsy_eigs_get_info: null argument");
        return -1;
    }
    const parsy::EigsState* E = pl->eigs.get();
    info->iterations = E ? E->iterations : 0;
    info->restarts = E ? E->restarts : 0;
    info->nconv = E ? E->nconv : 0;
    info->basis = E ? E->basis_cols : 0;
    info->dropped = E ? E->dropped : 0;
    info->reserved = 0;
    info->solve_columns = E ? E->solve_columns : 0;
    info->device_bytes = E ? E->meter.bytes : 0;
    return 0;
}
