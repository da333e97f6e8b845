// device_mem.h -- owners of the HIP resources the mapper's host code holds (host only).  Each is move-only and frees what it holds in its
// destructor; each reports a failure as drprg::Error, the way HIPCHK does.  No pools, no sharing: one allocation, one owner.
#pragma once
#include "common.h"
#include <hip/hip_runtime.h>
#include <string>
#include <utility>
#include <vector>

namespace drprg {

#define HIPCHK(x)                                                                                              \
    do {                                                                                                       \
        hipError_t e_ = (x);                                                                                   \
        if (e_ != hipSuccess)                                                                                  \
            throw Error(e_ == hipErrorOutOfMemory ? DRPRG_ENOMEM : DRPRG_EIO,                                  \
                std::string("HIP error: ") + hipGetErrorString(e_) + " at " + __FILE__ + ":" + std::to_string(__LINE__)); \
    } while (0)

// What the four owners share: one handle, null when empty, handed on by a move and given back to the runtime by reset().
template <typename H, hipError_t (*Release)(H)> class Owner {
public:
    Owner() = default;
    Owner(Owner&& o) noexcept : h_(std::exchange(o.h_, H {})) {}
    Owner& operator=(Owner&& o) noexcept
    {
        if (this != &o) {
            reset();
            h_ = std::exchange(o.h_, H {});
        }
        return *this;
    }
    ~Owner() { reset(); }
    explicit operator bool() const { return h_ != H {}; }
    void reset()
    {
        if (h_) (void)Release(h_);
        h_ = H {};
    }

protected:
    H h_ {};
};

// Device memory for size() elements.  Contents do not survive a regrow; an empty request still allocates one element.
template <typename T> class DeviceBuffer : public Owner<void*, hipFree> {
public:
    T* data() const { return static_cast<T*>(h_); }
    size_t size() const { return h_ ? n_ : 0; } // capacity in elements
    size_t bytes() const { return size() * sizeof(T); }
    void alloc(size_t n)
    {
        reset(); // (first: the peak footprint of a regrow is the new block, not old + new)
        HIPCHK(hipMalloc(&h_, (n ? n : 1) * sizeof(T)));
        n_ = n;
    }
    // room for `need` elements: nothing to do (false), or the block replaced by one of `grown` elements (true)
    bool reserve(size_t need, size_t grown)
    {
        if (need <= size()) return false;
        alloc(grown);
        return true;
    }
    // a fresh block holding these elements (a blocking copy)
    void upload(const T* src, size_t n)
    {
        alloc(n);
        if (n) HIPCHK(hipMemcpy(h_, src, n * sizeof(T), hipMemcpyHostToDevice));
    }
    void upload(const std::vector<T>& v) { upload(v.data(), v.size()); }

private:
    size_t n_ = 0;
};

// Page-locked host memory the device can address (the small read-back words of the launch sequences).
template <typename T> class PinnedBuffer : public Owner<void*, hipHostFree> {
public:
    T* data() const { return static_cast<T*>(h_); }
    T* device_ptr() const { return h_ ? dev_ : nullptr; }
    T& operator[](size_t i) const { return data()[i]; }
    void alloc(size_t n)
    {
        reset();
        HIPCHK(hipHostMalloc(&h_, n * sizeof(T), hipHostMallocDefault));
        const hipError_t e = hipHostGetDevicePointer((void**)&dev_, h_, 0);
        if (e != hipSuccess) reset(); // (all or nothing)
        HIPCHK(e);
    }

private:
    T* dev_ = nullptr;
};

class Event : public Owner<hipEvent_t, hipEventDestroy> {
public:
    operator hipEvent_t() const { return h_; }
    void create(bool timing)
    {
        reset();
        HIPCHK(timing ? hipEventCreate(&h_) : hipEventCreateWithFlags(&h_, hipEventDisableTiming));
    }
};

class Stream : public Owner<hipStream_t, hipStreamDestroy> {
public:
    operator hipStream_t() const { return h_; }
    void create() // non-blocking
    {
        reset();
        HIPCHK(hipStreamCreateWithFlags(&h_, hipStreamNonBlocking));
    }
};

} // namespace drprg
