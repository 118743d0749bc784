// Carving one allocation into typed spans: a cursor over a base address.  A layout is a function that takes spans from a
// Carver in a fixed order; run over a null base it only measures (total()), run over two bases it yields two views whose
// offsets cannot differ (a device buffer and its pinned host mirror).  No HIP, no context.
#pragma once
#include <cstddef>
#include <cstdint>

struct Carver {
  uintptr_t base;
  size_t at = 0;
  explicit Carver(const void* b = nullptr) : base(reinterpret_cast<uintptr_t>(b)) {}
  // the cursor rounded up to a multiple of a (a power of two)
  void align(size_t a) { at = (at + a - 1) & ~(a - 1); }
  // count elements of T from an a-byte boundary on
  template <typename T>
  T* take(size_t count, size_t a = alignof(T)) {
    align(a);
    T* p = reinterpret_cast<T*>(base + at);
    at += count * sizeof(T);
    return p;
  }
  char* here() const { return reinterpret_cast<char*>(base + at); }
  size_t total() const { return at; }
};
