// t2d_devbuf.h -- the one owner of device and pinned host memory in libt2d_hip.so.  Every hipMalloc / hipHostMalloc of the
// library is a DevBuf / PinBuf member or local: the destructor frees, a move hands the block on, and a failure path is a
// plain `return`.  Views that go to kernels by value (t2d_pool.h) keep plain pointers BORROWED from the owner next to them.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <atomic>
#include <type_traits>
#include <utility>

namespace t2d {

// live {device bytes, device blocks, pinned bytes, pinned blocks} of the process (defined in t2d_api.hip; read by
// t2d_debug_memory of include/t2d_debug.h only)
extern std::atomic<int64_t> g_mem_live[4] __attribute__((visibility("hidden")));

template <class T, bool PINNED>
class Buf {
    T* p_ = nullptr;
    size_t bytes_ = 0;
    void count(int64_t sign) {
        g_mem_live[PINNED ? 2 : 0].fetch_add(sign * (int64_t)bytes_, std::memory_order_relaxed);
        g_mem_live[PINNED ? 3 : 1].fetch_add(sign, std::memory_order_relaxed);
    }

public:
    Buf() = default;
    Buf(Buf&& o) noexcept : p_(std::exchange(o.p_, nullptr)), bytes_(std::exchange(o.bytes_, 0)) {}
    Buf& operator=(Buf&& o) noexcept {   // (frees what was held, then takes o's block)
        if (this != &o) {
            (void)reset();
            p_ = std::exchange(o.p_, nullptr);
            bytes_ = std::exchange(o.bytes_, 0);
        }
        return *this;
    }
    ~Buf() { (void)reset(); }

    // n elements (bytes of a void / char blob), uninitialised; frees what was held first.  `flags`: hipHostMalloc's (pinned
    // only).  A failed allocation leaves the buffer empty and the runtime's sticky error cleared.
    hipError_t alloc(size_t n, unsigned flags = 0) {
        hipError_t e = reset();
        if (e != hipSuccess) return e;
        const size_t bytes = n * sizeof(std::conditional_t<std::is_void<T>::value, char, T>);
        void* q = nullptr;
        e = PINNED ? hipHostMalloc(&q, bytes, flags) : hipMalloc(&q, bytes);
        if (e != hipSuccess) (void)hipGetLastError();
        if (e != hipSuccess || !q) return e;   // (!q: an empty request)
        p_ = static_cast<T*>(q);
        bytes_ = bytes;
        count(1);
        return hipSuccess;
    }
    hipError_t alloc_zeroed(size_t n) {
        const hipError_t e = alloc(n);
        return e == hipSuccess && p_ ? hipMemset(p_, 0, bytes_) : e;
    }
    hipError_t reset() {
        if (!p_) return hipSuccess;
        count(-1);
        bytes_ = 0;
        return PINNED ? hipHostFree(std::exchange(p_, nullptr)) : hipFree(std::exchange(p_, nullptr));
    }
    T* get() const { return p_; }
    operator T*() const { return p_; }   // what views borrow
    size_t bytes() const { return bytes_; }
};
template <class T = void> using DevBuf = Buf<T, false>;
template <class T = void> using PinBuf = Buf<T, true>;

}  // namespace t2d
