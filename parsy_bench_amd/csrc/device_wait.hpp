// Everything a kernel needs to wait inside a launch (included by device_util.hpp).
//
// The protocol, once:
//  * `info` is the status word of the run: the factorization's (0x7f7f7f7f = no failed pivot, else the 1-based failing
//    column) or the solve's (parsy_solve_status, reset per solve).  A negative value means that a wait was abandoned
//    and the result is wrong; the host reports it.
//  * A wait gives up when 2 s have passed since it began (kWaitTicks) OR when the status word is already negative:
//    whoever times out first reports with wait_failed(), and that one report ends every other wait of the run at its
//    next check instead of after 2 s of its own.  The clock and the status word are looked at on every 16th pass
//    only (BoundedWait::expired), so a wait that succeeds soon costs one increment per pass.
//  * `wait_bias` is a kernel argument that is 0 in every real run.  PARSY_DEBUG_SOLVE_STALL=1 makes it nonzero, and
//    a wait whose condition carries `|| wait_bias != 0` / `&& wait_bias == 0` then never succeeds: the tests drive
//    the timeout path with it.
//  * A loop that sleeps must hold a budget: every loop with a __builtin_amdgcn_s_sleep in it owns (or shares with the
//    loop before it) a BoundedWait and leaves when it expires.  What a kernel does then -- return, break, or go on
//    with whatever is there so that no barrier is missed -- is the kernel's business; the report is wait_failed(),
//    under the caller's own `lane == 0` / `tid == 0` guard where it has one.
// The poll loops themselves stay open-coded at their sites: each has its own load, memory order, scope and sleep
// policy, and a shared loop template changes the kernels' code.
// Only chol_kernels.hip, trsv_kernels.hip and trsv_bwd_kernels.hip wait inside a launch; trsv_sub_kernels.hip and
// the feature kernels are ordered by the stream (tests/test_wait_host.py holds this by search).
#pragma once
#include <hip/hip_runtime.h>

namespace parsy {

static constexpr unsigned long long kWaitTicks = 200000000ull;  // 2 s of the 100 MHz wall clock

// status < 0: a wait timed out / was abandoned
__device__ __forceinline__ void wait_failed(int* info) { atomicMin(info, -1); }

// The budget of one wait (or of two consecutive loops that wait for the same thing, a lazy watch and then the poll).
struct BoundedWait {
    const unsigned long long t0 = wall_clock64();
    int spins = 0;   // passes so far

    // the rule without its cadence, for a loop that counts its passes itself
    __device__ __forceinline__ bool expired_now(const int* info) const {
        return wall_clock64() - t0 > kWaitTicks || __hip_atomic_load(info, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < 0;
    }
    // one pass more; true on every 16th when the time is up or the run has failed already
    __device__ __forceinline__ bool expired(const int* info) { return (++spins & 15) == 0 && expired_now(info); }
};

// Wait until a counter of this workgroup's LDS has reached `want`; false when the wait was abandoned.
__device__ __forceinline__ bool wait_lds_counter(int* flag, int want, int wait_bias, const int* info) {
    BoundedWait w;
    while (__hip_atomic_load(flag, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) < want || wait_bias != 0) {
        if (w.expired(info)) return false;
        __builtin_amdgcn_s_sleep(1);
    }
    return true;
}

}  // namespace parsy
