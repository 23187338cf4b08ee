// Ownership of device memory on the host side: a byte meter, one growable buffer (DeviceBuf) and many fixed blocks that
// are freed together (DevicePool).  Every allocation of the library goes through one of the two; what is counted in a
// device_bytes figure is what was given a meter, and an owner takes its bytes off the meter again when it frees.
// Host-only, nothing of the plan.  Neither type synchronises and neither frees a null pointer (without a device even
// hipFree(nullptr) is an error): the waits that guard a free stay with the callers.
#pragma once
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <utility>
#include <vector>

namespace parsy {

// The one pair of functions that reaches the allocator, and the copy that fills a fresh block.  A stand-alone test
// program defines PARSY_DEVICE_ALLOC_PROVIDED and its own three (same names, same namespace) before it includes this
// header.
#ifndef PARSY_DEVICE_ALLOC_PROVIDED
inline hipError_t device_malloc(void** p, size_t bytes) { return hipMalloc(p, bytes); }
inline hipError_t device_free(void* p) { return hipFree(p); }
inline hipError_t device_fill(void* d, const void* h, size_t bytes) { return hipMemcpy(d, h, bytes, hipMemcpyHostToDevice); }
#endif

// Bytes of live device memory of one owner.  A meter with a parent passes every change on: a feature's state counts its
// own buffers and the plan's figure holds them too.
struct ByteMeter {
    int64_t bytes = 0;
    ByteMeter* const parent;
    explicit ByteMeter(ByteMeter* parent_ = nullptr) : parent(parent_) {}
    ByteMeter(const ByteMeter&) = delete;
    ByteMeter& operator=(const ByteMeter&) = delete;
    void add(int64_t b) {
        for (ByteMeter* m = this; m; m = m->parent) m->bytes += b;
    }
};

// One buffer that grows on demand to exactly the length asked for; the contents are not kept.  meter null: not counted.
template <class T>
class DeviceBuf {
public:
    explicit DeviceBuf(ByteMeter* meter = nullptr) : meter_(meter) {}
    DeviceBuf(DeviceBuf&& o) noexcept : p_(o.p_), n_(o.n_), meter_(o.meter_) { o.p_ = nullptr, o.n_ = 0; }
    ~DeviceBuf() { (void)reset(); }

    T* data() const { return p_; }
    int64_t size() const { return n_; }   // elements

    // at least `need` elements.  On an error the buffer is empty and the meter holds nothing of it.
    hipError_t grow(int64_t need) {
        if (n_ >= need) return hipSuccess;
        hipError_t e = reset();
        if (e != hipSuccess) return e;
        void* p = nullptr;
        e = device_malloc(&p, (size_t)need * sizeof(T));
        if (e != hipSuccess) return e;
        p_ = static_cast<T*>(p), n_ = need;
        if (meter_) meter_->add(n_ * (int64_t)sizeof(T));
        return hipSuccess;
    }
    hipError_t reset() {
        if (!p_) return hipSuccess;
        if (meter_) meter_->add(-n_ * (int64_t)sizeof(T));
        T* p = p_;
        p_ = nullptr, n_ = 0;
        return device_free(p);
    }

private:
    T* p_ = nullptr;
    int64_t n_ = 0;
    ByteMeter* meter_;
};

// Blocks of fixed size that live and die together.  alloc / upload hand out raw pointers, or null once a call has failed:
// error() says why, the pool keeps what it made before and makes nothing more until clear().  An ensure_* function builds
// into a local pool and local pointers, asks error() once and moves the pool into its state only when everything
// exists: a local pool that goes out of scope frees its blocks and takes their bytes off the meter.  meter null:
// nothing is counted.
class DevicePool {
public:
    explicit DevicePool(ByteMeter* meter = nullptr) : meter_(meter) {}
    DevicePool(DevicePool&& o) noexcept : blocks_(std::move(o.blocks_)), counted_(o.counted_), meter_(o.meter_), err_(o.err_) {
        o.blocks_.clear(), o.counted_ = 0;
    }
    DevicePool& operator=(DevicePool&& o) noexcept {
        if (this != &o) {
            clear();
            blocks_ = std::move(o.blocks_), counted_ = o.counted_, meter_ = o.meter_, err_ = o.err_;
            o.blocks_.clear(), o.counted_ = 0;
        }
        return *this;
    }
    ~DevicePool() { clear(); }

    // room for `count` elements (counted: whether the meter sees them)
    template <class T>
    T* alloc(int64_t count, bool counted = true) {
        void* p = nullptr;
        const int64_t bytes = count * (int64_t)sizeof(T);
        if (err_ == hipSuccess) err_ = device_malloc(&p, (size_t)bytes);
        if (err_ != hipSuccess) return nullptr;
        blocks_.push_back(p);
        if (counted && meter_) counted_ += bytes, meter_->add(bytes);
        return static_cast<T*>(p);
    }
    // a device copy of h (room for one element when h is empty)
    template <class T>
    T* upload(const std::vector<T>& h) {
        T* d = alloc<T>((int64_t)std::max<size_t>(h.size(), 1));
        if (d && !h.empty()) {
            err_ = device_fill(d, h.data(), h.size() * sizeof(T));
            if (err_ != hipSuccess) return nullptr;
        }
        return d;
    }
    hipError_t error() const { return err_; }   // of the first alloc / upload that failed
    bool empty() const { return blocks_.empty(); }
    void clear() {
        for (void* p : blocks_) (void)device_free(p);
        blocks_.clear();
        if (meter_) meter_->add(-counted_);
        counted_ = 0;
        err_ = hipSuccess;
    }

private:
    std::vector<void*> blocks_;
    int64_t counted_ = 0;
    ByteMeter* meter_;
    hipError_t err_ = hipSuccess;
};

}  // namespace parsy
