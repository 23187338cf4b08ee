// Host-side helpers of the files that work on a parsy_plan: the plan's refusals, the caller's ordering, device buffers
// that grow or are uploaded with their bytes counted, and the event pair that times a host-buffer call.  The only copy of each; what is
// no template is defined in executor.hip.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <vector>

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
// the device copy of that ordering, uploaded on first use and counted in device_bytes (*out null: identity)
int plan_perm_device(parsy_plan* pl, const int** out);
// The one gather and the one scatter of n x nrhs column-major operands under such a device copy (perm null: identity):
// dst[k, q] = src[perm[k], q] (src leading dimension ld, dst n; a second copy into dst2 when given), and
// dst[perm[k], q] = beta dst[perm[k], q] + alpha src[k, q] (src leading dimension n, dst ld; beta == 0: dst is not read)
void enqueue_perm_gather(const int* perm, const double* src, int64_t ld, double* dst, double* dst2, int n, int nrhs,
                         hipStream_t stream);
void enqueue_perm_scatter(const int* perm, const double* src, double alpha, double beta, double* dst, int64_t ld, int n,
                          int nrhs, hipStream_t stream);

// buf (len elements) made at least `need` elements long; the contents are not kept
template <class T>
hipError_t grow_device(T*& buf, int64_t& len, int64_t need) {
    if (len >= need) return hipSuccess;
    if (buf) {
        const hipError_t e = hipFree(buf);
        if (e != hipSuccess) return e;
    }
    buf = nullptr;
    len = 0;
    const hipError_t e = hipMalloc((void**)&buf, (size_t)need * sizeof(T));
    if (e == hipSuccess) len = need;
    return e;
}

// ... with its bytes counted in the plan's device_bytes
template <class T>
int grow_counted(parsy_plan* pl, T*& buf, int64_t& len, int64_t need) {
    if (len >= need) return 0;
    pl->device_bytes -= len * (int64_t)sizeof(T);
    const hipError_t e = grow_device(buf, len, need);
    pl->device_bytes += len * (int64_t)sizeof(T);
    PARSY_HIP(e);
    return 0;
}

// d = a new device copy of h (room for one element when h is empty); its bytes are added to `bytes`
template <class T>
int upload_counted(T*& d, const std::vector<T>& h, int64_t& bytes) {
    const size_t b = std::max<size_t>(h.size(), 1) * sizeof(T);
    PARSY_HIP(hipMalloc((void**)&d, b));
    if (!h.empty()) PARSY_HIP(hipMemcpy(d, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice));
    bytes += (int64_t)b;
    return 0;
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
