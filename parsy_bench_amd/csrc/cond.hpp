// Forward error bounds (LAPACK dporfs's FERR) and the reciprocal condition number (dpocon) of the SPD solve
// (cond_kernels.hip): Higham's 1-norm estimator (dlacn2) held on the device, one state machine per column, every column
// advanced in lockstep through many-right-hand-side solves with the factor.  The plan holds a CondState only once one of
// these calls has run; a plan that never calls them allocates nothing.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "device_buffer.hpp"

struct parsy_plan;

namespace parsy {

// dlacn2's reverse-communication state of one column
struct CondCol {
    double est, estold;
    int jump;    // 0: nothing produced yet; 1 .. 5: dlacn2's ISAVE(1), the point the next vector comes back to
    int kase;    // of the application under way: 1 = W A^-1 (scaled after the solve), 2 = A^-1 W (scaled before it)
    int j, jlast, iter;
    int done;    // est is final; the column's operand stays zero
};

struct CondState {
    explicit CondState(ByteMeter* plan) : meter(plan) {}
    ByteMeter meter;                      // parsy_cond_info.device_bytes: everything here, in the plan's figure too
    DeviceBuf<double> ws{&meter};         // w, the operand (n x nrhs each, leading dimension n)
    DeviceBuf<unsigned char> sgn{&meter}; // the saved sign vector, a byte per row and column (the solve overwrites the
                                          // operand)
    DeviceBuf<char> cols{&meter};         // partial maxima of |z| or of A's row sums (kRefinePartials x cap u64),
                                          // CondCol[cap], results (cap + 2 doubles)
    int cols_cap = 0;
    int32_t applications = 0, columns = 0;   // of the last call
};

// FERR of the z the refinement workspace holds (pb, z and the gathered values as the last residual left them; ctl[1] of
// its column state carries the status of the solves so far) into ferr (host, nrhs); synchronises stream.  `who` names
// the call in a refusal.
int cond_bounds_phase(parsy_plan* pl, const char* who, const double* d_L, int nrhs, double* ferr, hipStream_t stream);
int plan_error_bounds(parsy_plan* pl, const double* d_values, const double* d_L, const double* d_x, int ldx,
                      const double* d_b, int ldb, int nrhs, double* ferr, double* berr, hipStream_t stream);
int plan_rcond(parsy_plan* pl, const double* d_values, const double* d_L, double* anorm, double* rcond,
               hipStream_t stream);

}  // namespace parsy
