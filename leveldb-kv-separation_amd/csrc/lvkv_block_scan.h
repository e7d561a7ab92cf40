// The workgroup-wide exclusive scan of the table writers, one pass and many
// (lvkv_sst_blocks.hip's slot and layout kernels, lvkv_sst_finish.hip's
// filter and index layouts, lvkv_sst_build.hip's device-wide scan,
// lvkv_sst_entries.hip's report).
#ifndef LVKV_BLOCK_SCAN_H_
#define LVKV_BLOCK_SCAN_H_

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace lvkv {

__device__ __forceinline__ uint64_t shfl_up64(uint64_t v, uint32_t d) {
  const uint32_t lo = __shfl_up(static_cast<uint32_t>(v), d);
  const uint32_t hi = __shfl_up(static_cast<uint32_t>(v >> 32), d);
  return (static_cast<uint64_t>(hi) << 32) | lo;
}

// Exclusive scan of `local` over the workgroup's 1,024 threads: the sum of the
// threads before this one, and in *total the sum of all. wsum: 17 u64 of LDS;
// a barrier stands between a return and the next call (the caller's, after
// its stores).
__device__ __forceinline__ uint64_t block_scan(uint64_t local, uint64_t* wsum, uint64_t* total) {
  const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
  uint64_t incl = local;
  for (uint32_t d = 1; d < 64; d <<= 1) {
    const uint64_t y = shfl_up64(incl, d);
    if (lane >= d) incl += y;
  }
  if (lane == 63) wsum[w] = incl;
  __syncthreads();
  if (w == 0) {
    const uint64_t v = lane < 16 ? wsum[lane] : 0;
    uint64_t s = v;
    for (uint32_t d = 1; d < 16; d <<= 1) {
      const uint64_t y = shfl_up64(s, d);
      if (lane >= d) s += y;
    }
    if (lane < 16) wsum[lane] = s - v;  // exclusive
    if (lane == 15) wsum[16] = s;       // the pass's total
  }
  __syncthreads();
  *total = wsum[16];
  return wsum[w] + incl - local;
}

// The exclusive scan of n items by one workgroup, 1,024 a pass and an item a
// thread, the running total carried from pass to pass: item i, of value(i),
// gets place(i, carry + the values of the items before it). Returns the carry
// after the last item. The barrier block_scan asks for between two calls is
// here, so wsum is free again on return.
template <typename Value, typename Place>
__device__ __forceinline__ uint64_t block_scan_carry(uint32_t n, uint64_t carry, uint64_t* wsum,
                                                     Value value, Place place) {
  for (uint32_t base = 0; base < n; base += 1024) {
    const uint32_t i = base + threadIdx.x;
    uint64_t total;
    const uint64_t at = carry + block_scan(i < n ? uint64_t{value(i)} : 0u, wsum, &total);
    if (i < n) place(i, at);
    carry += total;
    __syncthreads();
  }
  return carry;
}

}  // namespace lvkv

#endif  // LVKV_BLOCK_SCAN_H_
