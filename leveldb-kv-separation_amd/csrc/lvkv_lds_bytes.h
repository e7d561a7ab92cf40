// Bytes in LDS as the one-wave codecs read them (lvkv_snappy.hip,
// lvkv_zstd.hip, lvkv_zstd_compress.hip): unaligned little-endian words from
// an LDS buffer, a block staged there from global memory, and a value made
// wave-uniform.
#ifndef LVKV_LDS_BYTES_H_
#define LVKV_LDS_BYTES_H_

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace lvkv {

// Little-endian dword at byte p of an LDS buffer (4-byte aligned base, padded
// by 8 bytes): two aligned reads.
__device__ __forceinline__ uint32_t ld32(const uint8_t* b, uint32_t p) {
  const uint32_t* d = reinterpret_cast<const uint32_t*>(b + (p & ~3u));
  return __builtin_amdgcn_alignbyte(d[1], d[0], p & 3u);
}
__device__ __forceinline__ uint64_t ld64(const uint8_t* b, uint32_t p) {
  const uint32_t* d = reinterpret_cast<const uint32_t*>(b + (p & ~3u));
  const uint32_t s = p & 3u;
  const uint32_t lo = __builtin_amdgcn_alignbyte(d[1], d[0], s);
  const uint32_t hi = __builtin_amdgcn_alignbyte(d[2], d[1], s);
  return (static_cast<uint64_t>(hi) << 32) | lo;
}

// A wave-uniform read. A value that is the same in every lane still lands in
// a VGPR when it is loaded, and everything computed from it would run as
// divergent code (exec masks, VALU), so the loads that steer control flow go
// through v_readfirstlane into SGPRs.
__device__ __forceinline__ uint32_t uni(uint32_t v) { return __builtin_amdgcn_readfirstlane(v); }

// A block's bytes [0, n) from global memory into LDS (4-aligned), `pad` (>= 3)
// zero bytes after them. Aligned dword loads at any source alignment: LDS
// dword i = alignbyte of source dwords i and i+1 (the second only where it
// holds bytes of the block, so nothing past the block's last dword is read).
__device__ __forceinline__ void stage(uint8_t* dst, const uint8_t* src, uint32_t n, uint32_t pad,
                                      uint32_t lane) {
  const uint32_t mis = static_cast<uint32_t>(reinterpret_cast<uintptr_t>(src)) & 3u;
  const uint32_t* s = reinterpret_cast<const uint32_t*>(src - mis);
  const uint32_t nd = (n + 3u) >> 2;
  for (uint32_t i = lane; i < nd; i += 64) {
    const uint32_t lo = s[i];
    const uint32_t hi = (mis != 0 && 4u * (i + 1u) < mis + n) ? s[i + 1] : 0u;
    reinterpret_cast<uint32_t*>(dst)[i] = __builtin_amdgcn_alignbyte(hi, lo, mis);
  }
  for (uint32_t i = n + lane; i < n + pad; i += 64) dst[i] = 0;
}

}  // namespace lvkv

#endif  // LVKV_LDS_BYTES_H_
