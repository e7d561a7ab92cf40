// BytewiseComparator on the device, stated once: used by the merge of sorted
// runs (lvkv_sst_merge.hip) and the memtable's sort (lvkv_memtable.hip).
#ifndef LVKV_KEY_COMPARE_H_
#define LVKV_KEY_COMPARE_H_

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace lvkv {

// The bytes a and b have in common at their start, of m. Eight bytes a word
// where both allow aligned loads (the first byte in memory is the word's
// lowest), two words a step so that their loads are in flight together -- a
// bisection is a chain of dependent loads, and this halves its links inside a
// key -- and a byte at a time otherwise.
__device__ __forceinline__ uint32_t common_prefix(const uint8_t* a, const uint8_t* b, uint32_t m) {
  uint32_t l = 0;
  if (((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b)) & 7u) == 0) {
    const auto word = [](const uint8_t* p) { return *reinterpret_cast<const uint64_t*>(p); };
    while (m - l >= 16u) {
      const uint64_t x0 = word(a + l) ^ word(b + l), x1 = word(a + l + 8u) ^ word(b + l + 8u);
      if (x0 != 0) return l + (static_cast<uint32_t>(__builtin_ctzll(x0)) >> 3);
      if (x1 != 0) return l + 8u + (static_cast<uint32_t>(__builtin_ctzll(x1)) >> 3);
      l += 16u;
    }
    if (m - l >= 8u) {
      const uint64_t x = word(a + l) ^ word(b + l);
      if (x != 0) return l + (static_cast<uint32_t>(__builtin_ctzll(x)) >> 3);
      l += 8u;
    }
  }
  while (l < m && a[l] == b[l]) ++l;
  return l;
}

// Slice::compare (include/leveldb/slice.h): BytewiseComparator.
__device__ __forceinline__ int compare_bytes(const uint8_t* a, uint32_t alen, const uint8_t* b,
                                             uint32_t blen) {
  const uint32_t m = alen < blen ? alen : blen;
  const uint32_t l = common_prefix(a, b, m);
  if (l < m) return a[l] < b[l] ? -1 : 1;
  return alen < blen ? -1 : alen > blen ? 1 : 0;
}

}  // namespace lvkv

#endif  // LVKV_KEY_COMPARE_H_
