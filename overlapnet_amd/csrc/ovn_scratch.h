// Carving a scratch block.  A consumer lists its regions ONCE, in the constructor of a small layout struct that takes them from an
// OvnCarver in order.  Run over a NULL base the same constructor measures (every pointer NULL, bytes() the size to reserve); run
// over the reserved block it places.  Size and placement therefore cannot disagree and regions cannot overlap.  Plain C++17.
#pragma once

#include <stddef.h>

class OvnCarver {
 public:
  static constexpr size_t ALIGN = 256;   // every region starts on a multiple of ALIGN bytes from the (equally aligned) base
  explicit OvnCarver(void* base) : base_(static_cast<char*>(base)) {}
  // `count` elements of T at the current position (NULL when measuring); take(0) takes nothing
  template <class T>
  T* take(size_t count) {
    T* p = base_ ? reinterpret_cast<T*>(base_ + off_) : nullptr;
    off_ += (count * sizeof(T) + ALIGN - 1) / ALIGN * ALIGN;
    return p;
  }
  size_t bytes() const { return off_; }   // the total so far: a multiple of ALIGN

 private:
  char* base_;
  size_t off_ = 0;
};

// bytes the layout L needs for the shape `a...`: its constructor on a measuring carver
template <class L, class... A>
size_t ovn_scratch_bytes(const A&... a) {
  OvnCarver m(nullptr);
  L probe(m, a...);
  (void)probe;
  return m.bytes();
}
