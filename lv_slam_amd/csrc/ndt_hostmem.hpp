// ndt_hostmem.hpp -- owners of the engine's device buffers, pinned host blocks, streams and events (host side of mi355_ndt.hip only).
// Each frees what it holds when it is destroyed or re-allocated; errors of the release are ignored.  A failed allocation leaves the owner
// empty (null, cap 0), so the next call allocates again instead of trusting a freed buffer.  Move-only; no pooling, no policy.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <type_traits>
#include <utility>

template <typename T, typename Traits>
struct HipBuf {
  T* p = nullptr;
  size_t cap = 0;                                 // elements
  HipBuf() = default;
  HipBuf(const HipBuf&) = delete;
  HipBuf& operator=(const HipBuf&) = delete;
  HipBuf(HipBuf&& o) noexcept : p(std::exchange(o.p, nullptr)), cap(std::exchange(o.cap, 0)) {}
  HipBuf& operator=(HipBuf&& o) noexcept { std::swap(p, o.p); std::swap(cap, o.cap); return *this; }
  ~HipBuf() { if (p) (void)Traits::release((void*)p); }
  operator T*() const { return p; }
  // free, then allocate exactly n elements (`flags`: hipHostMalloc's, pinned blocks only)
  hipError_t realloc_exact(size_t n, unsigned flags = 0) {
    hipError_t e = p ? Traits::release((void*)p) : hipSuccess;
    p = nullptr; cap = 0;
    if (e == hipSuccess) e = Traits::alloc((void**)&p, n * sizeof(T), flags);
    if (e == hipSuccess) cap = n; else p = nullptr;
    return e;
  }
  // grow only: re-allocates (at exactly n) when n exceeds the capacity
  hipError_t reserve(size_t n, unsigned flags = 0) { return n <= cap ? hipSuccess : realloc_exact(n, flags); }
  // mapped pinned blocks: the device's address of the block (null on failure)
  std::remove_volatile_t<T>* dev() const {
    void* d = nullptr;
    return p && hipHostGetDevicePointer(&d, (void*)p, 0) == hipSuccess ? (std::remove_volatile_t<T>*)d : nullptr;
  }
};
struct DevMem {
  static hipError_t alloc(void** p, size_t bytes, unsigned) { return hipMalloc(p, bytes); }
  static hipError_t release(void* p) { return hipFree(p); }
};
struct PinMem {
  static hipError_t alloc(void** p, size_t bytes, unsigned flags) { return hipHostMalloc(p, bytes, flags); }
  static hipError_t release(void* p) { return hipHostFree(p); }
};
template <typename T> using DevBuf = HipBuf<T, DevMem>;
template <typename T> using PinBuf = HipBuf<T, PinMem>;

// a stream / an event the engine created
template <typename H, hipError_t (*Destroy)(H)>
struct HipOwned {
  H h = nullptr;
  HipOwned() = default;
  HipOwned(const HipOwned&) = delete;
  HipOwned& operator=(const HipOwned&) = delete;
  HipOwned(HipOwned&& o) noexcept : h(std::exchange(o.h, nullptr)) {}
  HipOwned& operator=(HipOwned&& o) noexcept { std::swap(h, o.h); return *this; }
  ~HipOwned() { reset(); }
  operator H() const { return h; }
  void reset() { if (h) (void)Destroy(h); h = nullptr; }
  template <typename Create, typename... A>
  hipError_t create(Create fn, A... a) { reset(); hipError_t e = fn(&h, a...); if (e != hipSuccess) h = nullptr; return e; }
};
struct HipStream : HipOwned<hipStream_t, hipStreamDestroy> {
  hipError_t create() { return HipOwned::create(hipStreamCreateWithFlags, (unsigned)hipStreamNonBlocking); }
};
struct HipEvent : HipOwned<hipEvent_t, hipEventDestroy> {
  hipError_t create(unsigned flags = hipEventDisableTiming) { return HipOwned::create(hipEventCreateWithFlags, flags); }
};
