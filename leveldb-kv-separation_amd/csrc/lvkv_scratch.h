// Carving a caller's scratch buffer into typed arrays. A layout is listed
// once, in a function that takes its arrays from a Carver: run over a null
// base it only sizes the layout (a *_scratch_bytes function), run over the
// caller's buffer it fills in the pointers the kernels get.
#ifndef LVKV_SCRATCH_H_
#define LVKV_SCRATCH_H_

#include <stddef.h>
#include <stdint.h>

namespace lvkv {

// Every layout starts at the caller's pointer rounded up to this; the sizing
// functions count as many bytes of slack.
constexpr uint64_t kScratchAlign = 256;

inline uint8_t* scratch_base(void* scratch) {
  return reinterpret_cast<uint8_t*>((reinterpret_cast<uintptr_t>(scratch) + (kScratchAlign - 1)) &
                                    ~uintptr_t{kScratchAlign - 1});
}

class Carver {
 public:
  explicit Carver(uint8_t* base) : base_(base) {}
  // The bytes taken so far: the offset of what is taken next, once aligned.
  uint64_t bytes() const { return at_; }
  void align(uint64_t a) { at_ = (at_ + a - 1) & ~(a - 1); }
  // `count` T at the next multiple of `align`, which the bytes are rounded up
  // to as well. nullptr when only sizing.
  template <typename T>
  T* take(uint64_t count, uint64_t align = alignof(T)) {
    this->align(align);
    const uint64_t here = at_;
    at_ += count * sizeof(T);
    this->align(align);
    return base_ != nullptr ? reinterpret_cast<T*>(base_ + here) : nullptr;
  }

 private:
  uint8_t* base_;
  uint64_t at_ = 0;
};

}  // namespace lvkv

#endif  // LVKV_SCRATCH_H_
