// The one owner of device and pinned host memory in libvo_mi355x.so: a pointer with its capacity in elements, freed by its destructor.
// A workspace struct made of these needs no list of pointers to free; a pointer INTO such a buffer stays a plain pointer, with a comment
// that names its owner.  Nothing here zero-fills, pools or sub-allocates, and events, streams and graphs are not memory: they stay by hand.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

// The two memory policies: allocate bytes, release
struct vo_mem_device {
  static hipError_t alloc(void** p, size_t bytes) { return hipMalloc(p, bytes); }
  static void release(void* p) { (void)hipFree(p); }
};
struct vo_mem_pinned {
  static hipError_t alloc(void** p, size_t bytes) { return hipHostMalloc(p, bytes, hipHostMallocDefault); }
  static void release(void* p) { (void)hipHostFree(p); }
};

template <class T, class Mem>
class vo_buf {
 public:
  vo_buf() = default;
  vo_buf(const vo_buf&) = delete;
  vo_buf& operator=(const vo_buf&) = delete;
  vo_buf(vo_buf&& o) noexcept { swap(o); }
  vo_buf& operator=(vo_buf&& o) noexcept {
    if (this != &o) { reset(); swap(o); }
    return *this;
  }
  ~vo_buf() { reset(); }

  // Grow-only room for n elements.  n <= cap(): nothing happens.  Otherwise the old block goes first (the peak is one block, the contents
  // are not kept), then n elements are allocated; a refused allocation leaves the buffer empty -- null, capacity 0 -- and comes back
  hipError_t reserve(size_t n) {
    grew_ = false;
    if (n <= cap_) return hipSuccess;
    reset();
    void* p = nullptr;
    const hipError_t e = Mem::alloc(&p, n * sizeof(T));
    if (e != hipSuccess) return e;
    p_ = static_cast<T*>(p);
    cap_ = n;
    grew_ = true;
    return hipSuccess;
  }
  void reset() {
    if (p_) Mem::release(p_);
    p_ = nullptr;
    cap_ = 0;
    grew_ = false;
  }
  void swap(vo_buf& o) noexcept {
    T* p = p_; p_ = o.p_; o.p_ = p;
    const size_t n = cap_; cap_ = o.cap_; o.cap_ = n;
    const bool g = grew_; grew_ = o.grew_; o.grew_ = g;
  }
  T* get() const { return p_; }
  operator T*() const { return p_; }
  size_t cap() const { return cap_; }                  // elements
  size_t bytes() const { return cap_ * sizeof(T); }
  bool grew() const { return grew_; }                  // the last reserve allocated: the block is new and holds nothing yet

 private:
  T* p_ = nullptr;
  size_t cap_ = 0;
  bool grew_ = false;
};
template <class T> using vo_dev = vo_buf<T, vo_mem_device>;
template <class T> using vo_pinned = vo_buf<T, vo_mem_pinned>;

// Build, then attach: a workspace W is constructed, build(*w) fills it (0 = VO_OK), and only a complete one lands in the slot of the
// context.  A failed build deletes it with whatever it had allocated and leaves the slot null, so the next call starts afresh.  A caller
// that replaces a smaller workspace has destroyed it before
template <class W, class Build>
inline int32_t vo_ws_replace(W*& slot, Build build) {
  W* w = new W();
  const int32_t r = build(*w);
  if (r != 0) { delete w; w = nullptr; }
  slot = w;
  return r;
}
