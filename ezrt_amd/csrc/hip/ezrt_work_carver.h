// ezrt_work_carver.h -- a caller's `work` buffer cut into typed pieces, one after the other.  A layout is written once, as a
// function that takes its pieces from a carver: over the caller's pointer it yields the kernels' arrays, over a null pointer the size
// the caller has to bring (ezrt_*_work_bytes).  Host code with no HIP include, so that a host compiler alone can check it
// (tests/test_work_carver.py runs it under the sanitizers).
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstdlib>

namespace ezi {
class WorkCarver {
 public:
  explicit WorkCarver(void* base) : base_((unsigned char*)base) {}
  // the next `count` elements of T: null over a null base.  A piece that would start off T's alignment is a mistake in the layout,
  // not in a caller's arguments: it ends the process.
  template <class T>
  T* take(uint64_t count) {
    if (off_ % alignof(T)) {
      std::fprintf(stderr, "WorkCarver: a piece of %zu-byte alignment at offset %llu\n", alignof(T), (unsigned long long)off_);
      std::abort();
    }
    const uint64_t at = off_;
    off_ += count * (uint64_t)sizeof(T);
    return base_ ? (T*)(base_ + at) : nullptr;
  }
  uint64_t offset() const { return off_; }
  // what the pieces taken so far need: the running offset rounded up to 8
  size_t bytes() const { return (size_t)((off_ + 7) / 8 * 8); }

 private:
  unsigned char* base_;
  uint64_t off_ = 0;
};
} // namespace ezi
