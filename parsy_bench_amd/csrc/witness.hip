// Kernel witness (solve_route.hpp; include/parsy_amd.h, diagnostics): host-side launch counters of the factor and the solve
// kernels.
#include <atomic>

#include <string>

#include "errors.hpp"
#include "launch.hpp"

namespace parsy {

static std::atomic<unsigned long long> g_witness[kWitnessCount];
static const char* const kWitnessNames[kWitnessCount] = {
#define PARSY_WITNESS_NAME(id, name) name,
    PARSY_WITNESS_KERNELS(PARSY_WITNESS_NAME)
#undef PARSY_WITNESS_NAME
};
void witness_launch(WitnessKernel k) { g_witness[k].fetch_add(1, std::memory_order_relaxed); }
void launch_refused(const char* function, WitnessKernel k) {
    set_last_error(std::string(function) + ": not a kernel of this launch function: " +
                   (k >= 0 && k < kWitnessCount ? kWitnessNames[k] : "(none)"));
}

}  // namespace parsy

// Kernel witness (include/parsy_amd.h, diagnostics)
extern "C" int parsy_debug_kernel_count(void) { return parsy::kWitnessCount; }
extern "C" const char* parsy_debug_kernel_name(int k) {
    return k >= 0 && k < parsy::kWitnessCount ? parsy::kWitnessNames[k] : nullptr;
}
extern "C" unsigned long long parsy_debug_kernel_launches(int k) {
    return k >= 0 && k < parsy::kWitnessCount ? parsy::g_witness[k].load(std::memory_order_relaxed) : 0ull;
}
extern "C" void parsy_debug_kernel_reset(void) {
    for (auto& c : parsy::g_witness) c.store(0, std::memory_order_relaxed);
}
