// gg_devmem.h — who owns device memory (host only; DESIGN.md "Device memory
// ownership").  Two types and nothing more:
//   gg_arena      blocks that live as long as their owner (a context's cache
//                 state, a coherent run's arrays): alloc() hands out a raw
//                 pointer, everything goes when the arena is cleared or dies;
//   gg_dbuf<T>    one block of batch scratch that is grown on demand, or a
//                 call-local temporary freed on every way out of the call.
// Kernels and the structs passed to them by value keep plain pointers, filled
// from alloc() / get().  Frees happen where the owner is cleared, reset or
// destroyed (hipFree synchronises); nothing is pooled or deferred.
//
// The allocator is the pair alloc / release of a policy type: gg_mem_device,
// or gg_mem_pinned for a gg_dbuf of page-locked host memory.  The two below
// are the only callers of hipMalloc / hipFree in the backend; a CPU program
// defines GG_DEVMEM_ALLOCATOR and supplies both types itself before including
// this header.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <utility>
#include <vector>

#include "../../include/graphite_gpu.h"

#ifndef GG_DEVMEM_ALLOCATOR
#include <hip/hip_runtime.h>
gg_status gg_hip_check(hipError_t e, const char* what);   // gg_capi.hip
struct gg_mem_device {
  static gg_status alloc(void** p, size_t bytes)
  {
    const hipError_t e = hipMalloc(p, bytes);
    return e == hipSuccess ? GG_OK : gg_hip_check(e, "hipMalloc");
  }
  static void release(void* p) { (void)hipFree(p); }
};
struct gg_mem_pinned {    // page-locked host memory
  static gg_status alloc(void** p, size_t bytes)
  {
    const hipError_t e = hipHostMalloc(p, bytes, hipHostMallocDefault);
    return e == hipSuccess ? GG_OK : gg_hip_check(e, "hipHostMalloc");
  }
  static void release(void* p) { (void)hipHostFree(p); }
};
#endif

class gg_arena {
 public:
  gg_arena() = default;
  gg_arena(const gg_arena&) = delete;
  gg_arena& operator=(const gg_arena&) = delete;
  ~gg_arena() { clear(); }
  // n elements (at least one); *p is set on success only
  template <class T> gg_status alloc(T** p, uint64_t n)
  {
    void* v = nullptr;
    blocks_.reserve(blocks_.size() + 1);
    if (gg_status st = gg_mem_device::alloc(&v, sizeof(T) * (size_t)(n ? n : 1))) return st;
    blocks_.push_back(v);
    *p = (T*)v;             // (T may carry a device address space: gg_coh_dev.h)
    return GG_OK;
  }
  void clear()
  {
    for (void* v : blocks_) gg_mem_device::release(v);
    blocks_.clear();
  }
 private:
  std::vector<void*> blocks_;
};

template <class T, class M = gg_mem_device>
class gg_dbuf {
 public:
  gg_dbuf() = default;
  gg_dbuf(gg_dbuf&& o) noexcept : p_(std::exchange(o.p_, nullptr)), cap_(std::exchange(o.cap_, 0)) {}
  gg_dbuf& operator=(gg_dbuf&& o) noexcept
  {
    if (this != &o) { reset(); p_ = std::exchange(o.p_, nullptr); cap_ = std::exchange(o.cap_, 0); }
    return *this;
  }
  ~gg_dbuf() { reset(); }
  T* get() const { return p_; }
  operator T*() const { return p_; }       // launch arguments and pointer views read as with a raw pointer
  uint64_t capacity() const { return cap_; }   // elements
  void reset()
  {
    if (p_) M::release(p_);
    p_ = nullptr; cap_ = 0;
  }
  // Room for `need` elements: nothing when there is room already, else the
  // block is freed and one of new_capacity elements allocated in its place
  // (the contents are not kept).  A failure leaves the buffer empty.
  gg_status reserve(uint64_t need, uint64_t new_capacity)
  {
    if (need <= cap_) return GG_OK;
    reset();
    void* v = nullptr;
    if (gg_status st = M::alloc(&v, sizeof(T) * (size_t)new_capacity)) return st;
    p_ = static_cast<T*>(v); cap_ = new_capacity;
    return GG_OK;
  }
  gg_status reserve(uint64_t need) { return reserve(need, need); }
 private:
  T* p_ = nullptr;
  uint64_t cap_ = 0;
};

// Buffers that share one capacity, grown together: the members short of `need`
// are all freed first, then allocated in order.  After a failure part-way every
// member is either valid for its own capacity() or empty, and a retry grows
// exactly the ones that are short.
template <class... B>
gg_status gg_reserve_all(uint64_t need, uint64_t new_capacity, B&... b)
{
  ((need > b.capacity() ? b.reset() : void()), ...);
  gg_status st = GG_OK;
  ((st == GG_OK ? void(st = b.reserve(need, new_capacity)) : void()), ...);
  return st;
}
