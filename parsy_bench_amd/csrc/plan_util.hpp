// Host-side helpers of the files that work on a parsy_plan: the plan's refusals, the caller's ordering and the event
// pair that times a host-buffer call.  The only copy of each, defined in executor.hip.  (Device memory is owned through
// device_buffer.hpp.)
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "executor.hpp"
#include "hip_check.hpp"

namespace parsy {

// What a call needs of the plan, each level with the ones before it:
//   kNeedsDevice  a device;
//   kNeedsA       A's pattern (not a plan made from L's pattern alone): the gradient calls;
//   kNeedsIdle    no parsy_plan_set_active / _set_active_pieces restriction, no factorization and no solve in steps of
//                 levels open: refinement and selected inversion.
enum PlanNeeds { kNeedsDevice, kNeedsA, kNeedsIdle };
// 0, or -1 with the refusal as the last error; `who` names the call in the message.
int check_plan(const parsy_plan* pl, const char* who, PlanNeeds needs);

// The caller's ordering of the plan's vectors (perm[new] = old, n entries; null: back to the identity).
int plan_set_perm(parsy_plan* pl, const int* perm);
// its inverse (inv[old] = new; empty: identity), made by the first call that asks and kept until the ordering changes
const std::vector<int>& plan_perm_inverse(parsy_plan* pl);
// the device copy of that ordering, uploaded on first use and counted in device_bytes (*out null: identity)
int plan_perm_device(parsy_plan* pl, const int** out);
// The one gather and the one scatter of n x nrhs column-major operands under such a device copy (perm null: identity):
// dst[k, q] = src[perm[k], q] (src leading dimension ld, dst n; a second copy into dst2 when given), and
// dst[perm[k], q] = beta dst[perm[k], q] + alpha src[k, q] (src leading dimension n, dst ld; beta == 0: dst is not read)
void enqueue_perm_gather(const int* perm, const double* src, int64_t ld, double* dst, double* dst2, int n, int nrhs,
                         hipStream_t stream);
void enqueue_perm_scatter(const int* perm, const double* src, double alpha, double beta, double* dst, int64_t ld, int n,
                          int nrhs, hipStream_t stream);

// -1 with the failure of a DevicePool's alloc / upload (its error()) as the last error
inline int pool_failed(const DevicePool& pool) {
    set_last_error(std::string("device allocation: ") + hipGetErrorString(pool.error()));
    return -1;
}

// The pair of events on the NULL stream that times the device work of one host-buffer call.
struct EventTimer {
    hipEvent_t e0 = nullptr, e1 = nullptr;
    EventTimer() = default;
    EventTimer(const EventTimer&) = delete;
    EventTimer& operator=(const EventTimer&) = delete;
    ~EventTimer();
    bool start();                 // makes both events (false: it could not) and records the first
    bool stop(double* seconds);   // records the second and waits for it; seconds (may be null): the time between them
};

}  // namespace parsy
