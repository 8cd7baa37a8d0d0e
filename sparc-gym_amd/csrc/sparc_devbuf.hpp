// sparc_devbuf.hpp — ownership of the context's device and pinned memory.  The only place that
// allocates or frees either: a buffer frees itself when it goes out of scope or is assigned over,
// so an error path cannot leak one and nothing is freed twice.  Every call returns HIP's status
// for the caller's HIPCHK.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

#include <utility>
#include <vector>

namespace sparc {

// n elements of T in device memory; move-only
template <class T>
class DevBuf {
  public:
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    DevBuf(DevBuf&& o) noexcept : p_(std::exchange(o.p_, nullptr)), n_(std::exchange(o.n_, 0)) {}
    DevBuf& operator=(DevBuf&& o) noexcept {
        if (this != &o) {
            reset();
            p_ = std::exchange(o.p_, nullptr);
            n_ = std::exchange(o.n_, 0);
        }
        return *this;
    }
    ~DevBuf() { reset(); }

    T* get() const { return p_; }   // for kernel arguments; null when empty
    size_t size() const { return n_; }
    explicit operator bool() const { return p_ != nullptr; }
    void reset() {
        if (p_) (void)hipFree(p_);
        p_ = nullptr;
        n_ = 0;
    }
    // n fresh elements (the old contents are gone, also when the allocation fails)
    hipError_t alloc(size_t n) {
        reset();
        const hipError_t e = hipMalloc(reinterpret_cast<void**>(&p_), sizeof(T) * n);
        if (e != hipSuccess) p_ = nullptr;
        else n_ = n;
        return e;
    }
    // scratch of at least n elements: grows only, and keeps nothing when it grows
    hipError_t reserve(size_t n) { return n <= n_ ? hipSuccess : alloc(n); }

  private:
    T* p_ = nullptr;
    size_t n_ = 0;
};

// allocate n elements and copy them from the host: blocking, or queued on a stream (src must then
// stay alive until the stream has run the copy)
template <class T>
hipError_t upload(DevBuf<T>& b, const T* src, size_t n) {
    const hipError_t e = b.alloc(n);
    return e != hipSuccess ? e : hipMemcpy(b.get(), src, sizeof(T) * n, hipMemcpyHostToDevice);
}
template <class T>
hipError_t upload(DevBuf<T>& b, const std::vector<T>& src) { return upload(b, src.data(), src.size()); }
template <class T>
hipError_t upload(DevBuf<T>& b, const std::vector<T>& src, hipStream_t stream) {
    const hipError_t e = b.alloc(src.size());
    return e != hipSuccess ? e : hipMemcpyAsync(b.get(), src.data(), sizeof(T) * src.size(), hipMemcpyHostToDevice, stream);
}

// one T in pinned host memory that kernels and copies write (the queue count, the one-env
// record); allocated on first use, dev() is its device address when mapped
template <class T>
class PinnedWord {
  public:
    PinnedWord() = default;
    PinnedWord(const PinnedWord&) = delete;
    PinnedWord& operator=(const PinnedWord&) = delete;
    ~PinnedWord() {
        if (h_) (void)hipHostFree(h_);
    }
    T* get() const { return h_; }
    T* dev() const { return d_; }
    hipError_t ensure(unsigned flags) {
        if (h_) return hipSuccess;
        hipError_t e = hipHostMalloc(reinterpret_cast<void**>(&h_), sizeof(T), flags);
        if (e != hipSuccess) {
            h_ = nullptr;
            return e;
        }
        if (flags & hipHostMallocMapped) e = hipHostGetDevicePointer(reinterpret_cast<void**>(&d_), h_, 0);
        if (e != hipSuccess) {
            (void)hipHostFree(h_);
            h_ = d_ = nullptr;
        }
        return e;
    }

  private:
    T* h_ = nullptr;
    T* d_ = nullptr;
};

}  // namespace sparc
