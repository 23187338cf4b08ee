// Normal matrices on the plan's pattern: N = F diag(w) F' + beta I + A0 assembled straight into A2 order, the products
// by F and F', and least squares through the factor of N (normal.cpp, normal_kernels.hip).
//
// F is n x m in compressed columns, its rows in the caller's ordering; a handle (parsy_normal) belongs to one plan and
// one pattern of F and keeps the plan's ordering as it stood when the handle was made.  The inspector runs once per
// pattern: per A2 entry q = (i, j) of P A P' the list of triples (a, b, k) -- column k of F holds both rows, a is the
// position in fx of the entry on row i, b the one on row j -- ascending in k, which is the summation order.  Lists of
// more than kNormalChunk triples are cut into chunks of kNormalChunk (one wave each, one partial each, folded in chunk
// order); the others are binned by length into three classes of 1, 8 and 64 lanes per entry.  The borders are
// constants: the bits of N are a function of the pattern and the values, never of the device or of the call.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "schedule.hpp"

struct parsy_plan;
struct parsy_normal;

namespace parsy {

constexpr int kNormalChunk = 512;     // triples per chunk of a long list = the longest list a class kernel takes
constexpr int kNormalClasses = 3;
constexpr int kNormalBorder[kNormalClasses] = {8, 64, kNormalChunk};   // longest list of the class
constexpr int kNormalLanes[kNormalClasses] = {1, 8, 64};                // lanes per entry of the class
constexpr int kNormalBlock = 8;       // right-hand sides per pass of the products (accumulators of a thread)

struct NormalIndex {
    int n = 0, m = 0;
    int64_t nnzA = 0, pairs = 0;
    std::vector<int> perm;            // the plan's ordering when the handle was made (perm[new] = old; empty: identity)
    std::vector<int> inv;             // its inverse (empty: identity)
    std::vector<int32_t> fp, fi;      // F's pattern as given (caller's ordering), pointers rebased to 0
    std::vector<int32_t> arow, acol;  // (row, column) of every A2 entry in the factor's ordering
    std::vector<uint8_t> diag;        // nnzA: the entry is on the diagonal
    std::vector<int64_t> lptr;        // nnzA + 1: the lists
    std::vector<int32_t> ta, tb, tk;  // pairs each: the triples, split so that consecutive lanes read consecutive words
    std::vector<int32_t> cls[kNormalClasses];   // the entries of each class, ascending
    std::vector<int32_t> chunk_len;   // per chunk: its triples
    std::vector<int64_t> chunk_off;   // per chunk: its first triple
    std::vector<int32_t> fold_q;      // the chunked entries, ascending
    std::vector<int32_t> fold_ptr;    // fold_q.size() + 1: their chunks
    std::vector<int64_t> rptr;        // n + 1: the transposed index of F by the caller's row ...
    std::vector<int32_t> rpos, rcol;  // ... positions in fx, ascending, and their columns
    int32_t longest_list = 0;
    int64_t entries_untouched = 0;
    int nnzF() const { return (int)fi.size(); }
    int64_t chunks() const { return (int64_t)chunk_len.size(); }
};

// the lower triangle of the pattern of F F' with a full diagonal, sorted CSC (Ai null: the count); -1 with the message set
int64_t normal_pattern(int n, int m, const int* Fp, const int* Fi, int* Ap, int* Ai);
// checks of F alone (who names the call); 0, or -1 with the message set
int normal_check_f(const char* who, int n, int m, const int* Fp, const int* Fi);
// the whole index of a handle; 0, or -1 with the refusal as the last error (out is then empty)
int normal_build(const Schedule& S, const std::vector<int>& perm, int m, const int* Fp, const int* Fi, NormalIndex& out);
// violations of the index against F's pattern (0: sound)
long long normal_check(const NormalIndex& I);

// the device calls (normal_kernels.hip; stream: a hipStream_t)
int normal_values(parsy_normal* h, const double* d_fx, const double* d_w, double beta, const double* d_base,
                  double* d_values, void* stream);
int normal_apply(parsy_normal* h, int op, const double* d_fx, const double* d_w, const double* d_x, int ldx, int nrhs,
                 double alpha, double beta, double* d_y, int ldy, void* stream);
int normal_lsq(parsy_normal* h, const double* d_fx, const double* d_w, double beta, const double* d_L, const double* d_c,
               int ldc, double* d_x, int ldx, int nrhs, int steps, double* d_r, int ldr, double* d_g, int ldg, void* stream);
// the refusals of the three calls that need no device; 0, or -1 with the message set
int normal_check_values_args(const parsy_normal* h, const char* who, const void* fx, const void* values);
int normal_check_apply_args(const parsy_normal* h, const char* who, int op, const void* fx, const void* x, int ldx, int nrhs,
                            const void* y, int ldy);
int normal_check_lsq_args(const parsy_normal* h, const char* who, const void* fx, const void* lValues, const void* c, int ldc,
                          const void* x, int ldx, int nrhs, int steps, const void* r, int ldr, const void* g, int ldg);

}  // namespace parsy
