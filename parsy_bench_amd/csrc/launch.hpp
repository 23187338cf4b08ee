// The one way to enqueue a kernel that has a witness entry (solve_route.hpp, PARSY_WITNESS_KERNELS): the bump of the entry and
// the launch are one call, so that neither can be written without the other.  Kernel and entry are template arguments --
// the launch is a direct one, as a hipLaunchKernelGGL spelled out at the call site.  HIP sources only.
#pragma once
#include <hip/hip_runtime.h>

#include "kernels.hpp"

namespace parsy {

template <auto Kernel, WitnessKernel W, typename... Args>
inline void launch_witnessed(dim3 grid, dim3 block, size_t lds_bytes, hipStream_t stream, Args... args) {
    witness_launch(W);
    hipLaunchKernelGGL(Kernel, grid, block, lds_bytes, stream, args...);
}

// A launch function was handed a kernel it does not serve (the route and the function disagree): the last error names
// both, nothing is enqueued.
void launch_refused(const char* function, WitnessKernel k);

}  // namespace parsy
