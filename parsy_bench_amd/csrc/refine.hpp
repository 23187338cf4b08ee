// A x = b in the caller's ordering: residuals, backward errors and iterative refinement (refine_kernels.hip).
// The plan holds a RefineState only once one of these calls has run; a plan that never calls them allocates nothing.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

struct parsy_plan;

namespace parsy {

struct RefineState {
    // caller's ordering: perm[new] = old (empty: identity), and its device copy (null: identity)
    std::vector<int> perm;
    int* d_perm = nullptr;
    // both triangles of P A P' as CSR, built on first use from the A2 pattern the plan scatters (a_dst + L's rows):
    // row i holds its entries in ascending A2 order; src[e] is the A2 index of entry e, vf[e] = values[src[e]]
    int64_t nnz_full = 0;
    int max_row = 0;          // most entries in a row of the full symmetric A
    int group = 0;            // lanes per row of k_sym_residual with 1-4 right-hand sides (from the mean row length)
    int64_t* d_rp = nullptr;
    int* d_ci = nullptr;
    int* d_src = nullptr;
    double* d_vf = nullptr;
    int64_t pattern_bytes = 0;
    // workspace: pb, z, r (n x nrhs each, leading dimension n) and the per-column state
    double* ws = nullptr;
    int64_t ws_len = 0;       // doubles of ws
    char* colstate = nullptr; // berr bits partials (kPartials x nrhs u64), berr, lstres (nrhs doubles), active, steps (nrhs ints), ctl[2]
    int64_t colstate_len = 0; // bytes of colstate
    int colstate_cap = 0;     // right-hand sides colstate is made for
};

constexpr int kRefinePartials = 1024;   // workgroups of k_sym_residual (grid-stride over the rows) = partials per column

void refine_free(parsy_plan* pl);
int plan_set_perm(parsy_plan* pl, const int* perm);
// the device copy of that ordering, uploaded on first use (*out null: identity)
int plan_perm_device(parsy_plan* pl, const int** out);
int plan_residual(parsy_plan* pl, const double* d_values, const double* d_x, int ldx, const double* d_b, int ldb,
                  double* d_r, int ldr, int nrhs, double* berr, hipStream_t stream);
int plan_solve_refined(parsy_plan* pl, const double* d_values, const double* d_L, const double* d_b, int ldb, double* d_x,
                       int ldx, int nrhs, int max_steps, int32_t* steps, double* berr, hipStream_t stream);

}  // namespace parsy
