// Stand-alone check of csrc/device_buffer.hpp (test_device_buffer_host.py compiles it with the address and undefined-
// behaviour sanitizers and runs it; it needs no device).
//   default             the allocator is a counting malloc / free that fails the k-th allocation on request
//   -DCHECK_REAL_PAIR   the header's own pair: without a device hipMalloc fails, and nothing may be left behind.  (The
//                       program defines hipFree itself, ahead of the runtime library's, to count the calls: without a
//                       device every HIP call fails alike and leaves no other trace.)
#include <hip/hip_runtime_api.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <utility>
#include <vector>

#ifndef CHECK_REAL_PAIR
#define PARSY_DEVICE_ALLOC_PROVIDED
namespace parsy {
static int g_live = 0, g_mallocs = 0, g_frees = 0, g_fail_at = 0;   // g_fail_at: the k-th allocation from now fails (0: none)
inline hipError_t device_malloc(void** p, size_t bytes) {
    if (g_fail_at > 0 && --g_fail_at == 0) return hipErrorOutOfMemory;
    *p = std::malloc(bytes ? bytes : 1);
    ++g_mallocs, ++g_live;
    return hipSuccess;
}
inline hipError_t device_free(void* p) {
    if (!p) {
        std::fprintf(stderr, "device_free(nullptr)\n");
        std::abort();
    }
    std::free(p);
    ++g_frees, --g_live;
    return hipSuccess;
}
inline hipError_t device_fill(void* d, const void* h, size_t bytes) {
    std::memcpy(d, h, bytes);
    return hipSuccess;
}
}  // namespace parsy
#endif

#include "device_buffer.hpp"

using namespace parsy;

#define CHECK(cond)                                                         \
    do {                                                                    \
        if (!(cond)) {                                                      \
            std::fprintf(stderr, "%s:%d: CHECK(%s)\n", __FILE__, __LINE__, #cond); \
            std::exit(1);                                                   \
        }                                                                   \
    } while (0)

#ifndef CHECK_REAL_PAIR

static void check_buf() {
    ByteMeter plan, m(&plan);
    {
        DeviceBuf<double> b(&m);
        CHECK(b.data() == nullptr && b.size() == 0 && m.bytes == 0);
        CHECK(b.grow(10) == hipSuccess);
        CHECK(b.data() && b.size() == 10 && m.bytes == 80 && plan.bytes == 80 && g_mallocs == 1 && g_frees == 0);
        // larger: one free, one allocation, exactly the length asked for
        CHECK(b.grow(25) == hipSuccess);
        CHECK(b.size() == 25 && m.bytes == 25 * 8 && plan.bytes == 25 * 8 && g_mallocs == 2 && g_frees == 1 && g_live == 1);
        // smaller or equal: nothing
        double* const p = b.data();
        CHECK(b.grow(25) == hipSuccess && b.grow(3) == hipSuccess && b.grow(0) == hipSuccess);
        CHECK(b.data() == p && b.size() == 25 && m.bytes == 25 * 8 && g_mallocs == 2 && g_frees == 1);
        // a failed grow: empty, and its share off the meter
        g_fail_at = 1;
        CHECK(b.grow(100) == hipErrorOutOfMemory);
        CHECK(b.data() == nullptr && b.size() == 0 && m.bytes == 0 && plan.bytes == 0 && g_live == 0);
        // ... and it can be grown again
        CHECK(b.grow(4) == hipSuccess && m.bytes == 32 && g_live == 1);
        // moves: the source is empty, nothing is freed twice
        DeviceBuf<double> c(std::move(b));
        CHECK(b.data() == nullptr && b.size() == 0 && c.size() == 4 && m.bytes == 32 && g_live == 1);
        CHECK(c.reset() == hipSuccess && c.reset() == hipSuccess && m.bytes == 0 && g_live == 0);
        // an uncounted buffer
        DeviceBuf<int> u;
        CHECK(u.grow(7) == hipSuccess && m.bytes == 0 && g_live == 1);
    }
    CHECK(g_live == 0 && m.bytes == 0 && plan.bytes == 0 && g_mallocs == g_frees);
}

static void check_pool() {
    ByteMeter plan, m(&plan);
    DeviceBuf<char> other(&m);
    CHECK(other.grow(5) == hipSuccess);
    const int live0 = g_live;
    const int64_t bytes0 = m.bytes;
    const std::vector<int64_t> a(6, 1);
    const std::vector<int> b, c(3, 2);   // (b: room for one element)
    struct State {
        DevicePool pool;
        int64_t* a = nullptr;
        int *b = nullptr, *c = nullptr;
        bool ready = false;
    } st;
    // the build an ensure_* function makes: locals first, the state in one step
    auto build = [&]() -> bool {
        DevicePool local(&m);
        const int mallocs0 = g_mallocs;
        int64_t* da = local.upload(a);
        int *db = local.upload(b), *dc = local.upload(c);
        if (local.error() != hipSuccess) {
            // (the first block exists until the scope ends; after a failure the pool makes nothing more)
            CHECK(local.error() == hipErrorOutOfMemory && da && !db && !dc && g_mallocs == mallocs0 + 1);
            return false;
        }
        CHECK(std::memcmp(da, a.data(), 48) == 0 && std::memcmp(dc, c.data(), 12) == 0);
        st.pool = std::move(local);
        CHECK(local.empty());
        st.a = da, st.b = db, st.c = dc;
        st.ready = true;
        return true;
    };
    // the second allocation fails: after the local pool's scope everything is as before
    g_fail_at = 2;
    CHECK(!build());
    CHECK(!st.ready && st.pool.empty() && g_live == live0 && m.bytes == bytes0 && plan.bytes == bytes0);
    // ... and the next call starts again and commits: exactly the three blocks
    CHECK(build());
    CHECK(st.ready && g_live == live0 + 3 && m.bytes == bytes0 + 48 + 4 + 12 && plan.bytes == m.bytes);
    // uncounted blocks of a counted pool
    CHECK(st.pool.alloc<int>(9, false) != nullptr && g_live == live0 + 4 && m.bytes == bytes0 + 64);
    // move construction; clear, then the destructor
    {
        DevicePool moved(std::move(st.pool));
        CHECK(st.pool.empty() && !moved.empty() && g_live == live0 + 4 && m.bytes == bytes0 + 64);
        moved.clear();
        CHECK(moved.empty() && g_live == live0 && m.bytes == bytes0);
        moved.clear();
    }
    CHECK(g_live == live0 && m.bytes == bytes0);
    // a pool without a meter
    {
        DevicePool plain;
        CHECK(plain.alloc<double>(4) != nullptr && g_live == live0 + 1 && m.bytes == bytes0);
    }
    CHECK(g_live == live0);
    CHECK(other.reset() == hipSuccess && g_live == 0 && m.bytes == 0 && plan.bytes == 0);
}

int main() {
    check_buf();
    check_pool();
    CHECK(g_live == 0 && g_mallocs == g_frees);
    std::puts("device_buffer: ok");
    return 0;
}

#else  // CHECK_REAL_PAIR

static int g_free_calls = 0;
extern "C" hipError_t hipFree(void*) {
    ++g_free_calls;
    return hipErrorNoDevice;
}

int main() {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) == hipSuccess && ndev > 0) {
        // (left at once: what the runtime keeps for its devices until the process ends is not this program's to report)
        std::puts("device_buffer: a device is present, nothing to check");
        std::fflush(stdout);
        std::_Exit(0);
    }
    ByteMeter m;
    {
        DeviceBuf<double> buf(&m);
        DevicePool pool(&m);
        CHECK(buf.grow(16) == hipErrorNoDevice);
        CHECK(buf.data() == nullptr && buf.size() == 0 && m.bytes == 0);
        CHECK(pool.upload(std::vector<int>(5, 1)) == nullptr && pool.error() == hipErrorNoDevice);
        CHECK(pool.alloc<double>(3) == nullptr && pool.error() == hipErrorNoDevice);
        CHECK(pool.empty() && m.bytes == 0);
        // clearing, moving and destroying empty owners makes no HIP call
        pool.clear();
        (void)buf.reset();
        DevicePool moved(std::move(pool));
        DeviceBuf<double> moved_buf(std::move(buf));
    }
    CHECK(g_free_calls == 0 && m.bytes == 0);
    std::puts("device_buffer: ok");
    return 0;
}

#endif
