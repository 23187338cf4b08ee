// A x = b in the caller's ordering: residuals, backward errors and iterative refinement (refine_kernels.hip).
// The plan holds a RefineState only once one of these calls has run; a plan that never calls them allocates nothing.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "device_buffer.hpp"

struct parsy_plan;

namespace parsy {

struct RefineState {
    explicit RefineState(ByteMeter* plan) : meter(plan) {}
    ByteMeter meter;          // everything here is counted, in the plan's figure too
    // both triangles of P A P' as CSR, built on first use from the A2 pattern the plan scatters (a_dst + L's rows):
    // row i holds its entries in ascending A2 order; src[e] is the A2 index of entry e, vf[e] = values[src[e]]
    bool pattern_ready = false;   // set when the whole pattern is on the device: the fields down to d_vf are valid
    int64_t nnz_full = 0;
    int max_row = 0;          // most entries in a row of the full symmetric A
    int group = 0;            // lanes per row of k_sym_sweep with 1-4 right-hand sides (from the mean row length)
    DevicePool pattern{&meter};
    int64_t* d_rp = nullptr;
    int* d_ci = nullptr;
    int* d_src = nullptr;
    double* d_vf = nullptr;
    // workspace: pb, z, r (n x nrhs each, leading dimension n) and the per-column state
    DeviceBuf<double> ws{&meter};
    // berr bits partials (kPartials x nrhs u64), berr, lstres (nrhs doubles), active, steps (nrhs ints), ctl[2]
    DeviceBuf<char> colstate{&meter};
    int colstate_cap = 0;     // right-hand sides colstate is made for
};

constexpr int kRefinePartials = 1024;   // most workgroups of a sweep (sym_sweep.hpp) = partials per column
constexpr int kRefineThreads = 256;     // threads of a workgroup of every kernel here and in cond_kernels.hip
using u64 = unsigned long long;         // the bits of a non-negative double, max-reduced

// ---- host helpers shared with the error bounds and the condition estimate (cond_kernels.hip) ----
// the per-column state inside colstate
struct ColState {
    u64* part;
    double *berr, *lstres;
    int *active, *steps, *ctl;
};
ColState col_state(RefineState& R, int cap);
// Both triangles of P A P' as CSR, on first use; pb, z, r (n x nrhs), the per-column state and, in *perm, the plan's
// ordering on the device (plan_perm_device)
int refine_ensure_pattern(parsy_plan* pl);
int refine_ensure_workspace(parsy_plan* pl, int nrhs, const int** perm);
// vf = the caller's A2-order values on the full pattern (vf: nnz_full doubles; the A x = b calls pass d_vf)
int refine_gather_values(parsy_plan* pl, const double* d_values, double* vf, hipStream_t stream);
// r = pb - A z and the partial maxima of every column's backward error; returns the number of partials (< 0: error)
int refine_residual_enqueue(parsy_plan* pl, const double* z, const double* pb, double* r, int nrhs, u64* part,
                            hipStream_t stream);
// berr[q] of ColState from nb partials per column (the reporting form of the second pass)
int refine_report_berr(parsy_plan* pl, int nb, int nrhs, hipStream_t stream);
// forward + backward solve of the permuted system in place on x (leading dimension n); every solve's status word is
// folded into ctl[1] on the device (-1: a hand-off wait timed out)
int refine_solve_enqueue(parsy_plan* pl, const double* d_L, double* x, int nrhs, int* ctl, hipStream_t stream);

int plan_residual(parsy_plan* pl, const double* d_values, const double* d_x, int ldx, const double* d_b, int ldb,
                  double* d_r, int ldr, int nrhs, double* berr, hipStream_t stream);
// ferr (host, nrhs; may be null): the forward error bounds of the returned X (cond.hpp), taken from the z, pb and values
// the refinement ends with
int plan_solve_refined(parsy_plan* pl, const double* d_values, const double* d_L, const double* d_b, int ldb, double* d_x,
                       int ldx, int nrhs, int max_steps, int32_t* steps, double* berr, double* ferr, hipStream_t stream);

}  // namespace parsy
