// What a KernelArgs::mode means, stated once for every batch CRC kernel:
// which bytes block b covers and from which init (mode_covered), against
// which stored value the CRC is checked (Covered::expected) and what lane 0
// stores (mode_store). The kernels differ in schedule only:
//   crc32c_kernel.hip (persistent) and crc32c_long_kernel (crc32c_compact.hip)
//     serve compute, SST verify / fill; the persistent kernel also the WAL
//     modes;
//   the ragged walk (crc32c_ragged_body.h: crc32c_ragged.hip, the engine's
//     lvkv_ek_ragged*, the fused whole-SSTable verify) serves every mode.
// A new mode, or a changed rule of an existing one, is an edit to this file
// and to the enum in lvkv_kernel_args.h.
#ifndef LVKV_CRC32C_MODES_H_
#define LVKV_CRC32C_MODES_H_

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "crc32c_device_common.h"
#include "lvkv_crc32c.h"
#include "lvkv_kernel_args.h"

namespace lvkv {
namespace {

// ---- host + device: the families of modes --------------------------------

// WAL records: the block's offset is its header's (db/log_reader.cc:217-221).
__host__ __device__ constexpr bool mode_is_log(uint32_t mode) {
  return mode == kModeLogVerify || mode == kModeLogFill;
}
// SST blocks: the type byte after the contents is covered, the stored CRC
// follows it (table/format.cc:92-94, table/table_builder.cc:199-203).
__host__ __device__ constexpr bool mode_is_sst(uint32_t mode) {
  return mode == kModeSstVerify || mode == kModeSstFill || mode == kModeSstTable;
}
// The stored CRC that the result is checked against follows the covered
// bytes (the ragged walk loads it beside the block's rows).
__host__ __device__ constexpr bool mode_has_trailer(uint32_t mode) {
  return mode == kModeSstVerify || mode == kModeSstTable;
}
// KernelArgs::long_split of a general-layout batch in this mode.
__host__ __device__ constexpr uint32_t mode_long_split(uint32_t mode) {
  return mode_is_log(mode) ? kLogLongBytes : kLongBytes;
}

// ---- fewer than 4 bytes: bitwise -----------------------------------------

// Bitwise register update over one byte.
__device__ __forceinline__ uint32_t crc_byte_bitwise(uint32_t reg, uint32_t byte) {
  reg ^= byte;
#pragma unroll
  for (int k = 0; k < 8; ++k) reg = (reg >> 1) ^ (kCastagnoliReflected & (0u - (reg & 1u)));
  return reg;
}

// The same over the n (< 4) little-endian bytes of `bytes`.
__device__ __forceinline__ uint32_t crc_bytes_bitwise(uint32_t reg, uint32_t bytes, uint32_t n) {
  for (uint32_t i = 0; i < n; ++i) reg = crc_byte_bitwise(reg, (bytes >> (8u * i)) & 0xffu);
  return reg;
}

// CRC of the len (< 4) bytes at ptr from register s0 = init ^ ~0
// (wave-uniform, scalar loads).
__device__ __forceinline__ uint32_t crc_tiny(uint64_t ptr, uint32_t len, uint32_t s0) {
  return crc_bytes_bitwise(s0, len ? sload_le(ptr, len) : 0u, len) ^ 0xffffffffu;
}

// ---- how a kernel reads the descriptor arrays ----------------------------

// kFresh: the kernel may run in a launch whose other workgroups wrote the
// arrays (a.fresh_desc, the fused SST verify); they are then read with
// agent-scope atomic loads after the caller's acquire, never through a
// scalar-cache line that could predate the write. Otherwise (an earlier
// launch wrote them) wave-uniform reads go through the scalar cache.
template <bool kFresh, typename T>
__device__ __forceinline__ T lane_ld(const KernelArgs& a, const T* p) {  // per lane
  return kFresh && a.fresh_desc ? __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
                                : *p;
}
template <bool kFresh>
__device__ __forceinline__ uint64_t desc_off(const KernelArgs& a, uint32_t b) {  // wave-uniform
  if (!kFresh || !a.fresh_desc) return sload_u64(a.offsets, b);
  const uint64_t v = lane_ld<true>(a, a.offsets + b);
  const uint32_t lo = __builtin_amdgcn_readfirstlane(static_cast<uint32_t>(v));
  const uint32_t hi = __builtin_amdgcn_readfirstlane(static_cast<uint32_t>(v >> 32));
  return (static_cast<uint64_t>(hi) << 32) | lo;
}
template <bool kFresh>
__device__ __forceinline__ uint32_t desc_len(const KernelArgs& a, uint32_t b) {  // wave-uniform
  if (!kFresh || !a.fresh_desc) return sload_u32(a.lengths, b);
  return __builtin_amdgcn_readfirstlane(lane_ld<true>(a, a.lengths + b));
}

// ---- which bytes, from which init, against which stored value ------------

struct Covered {
  uint64_t ptr;       // first covered byte
  uint32_t len;       // covered bytes
  uint32_t init;
  uint32_t expected;  // verify modes: unmasked stored CRC
};

// Block b of the batch, wave-uniform. With `defer_trailer`, the stored CRC
// after an SST block is not loaded here (the ragged walk loads it with a
// vector load beside the block's rows, so no scalar load is outstanding while
// it waits on its LDS reads: one lgkmcnt counts both).
template <bool kFresh>
__device__ __forceinline__ Covered mode_covered(const KernelArgs& a, uint32_t b,
                                                bool defer_trailer) {
  const uint64_t base = reinterpret_cast<uint64_t>(a.base);
  uint64_t off;
  Covered c;
  c.init = a.init;
  c.expected = 0;
  if (mode_is_log(a.mode)) {
    // [masked crc u32][len u16][type u8]; the CRC covers type + payload
    // (db/log_reader.cc:217-221, 243-247, db/log_writer.cc:94-96).
    const uint64_t hoff = desc_off<kFresh>(a, b);
    const uint32_t len_type = sload_le(base + hoff + 4, 3);
    if (a.mode == kModeLogVerify) c.expected = crc_unmask(sload_le(base + hoff, 4));
    off = hoff + 6;
    c.len = 1u + (len_type & 0xffffu);
    c.init = 0;
  } else {
    if (a.offsets != nullptr) {
      off = desc_off<kFresh>(a, b);
      c.len = desc_len<kFresh>(a, b);
      // inits belongs to the per-block layout (no entry point passes it with
      // a uniform one; reading it there too costs the persistent kernel,
      // which is at its SGPR limit, a dozen more spills)
      if (a.inits != nullptr) c.init = sload_u32(a.inits, b);
    } else {  // uniform layout: block b at base + b * stride
      off = static_cast<uint64_t>(b) * a.stride;
      c.len = a.length;
    }
  }
  if (mode_is_sst(a.mode)) {
    // contents n bytes + type byte; the masked CRC follows
    // (table/format.cc:92-94, table/table_builder.cc:199-203)
    c.len += 1;
    c.init = 0;
    if (mode_has_trailer(a.mode) && !defer_trailer)
      c.expected = crc_unmask(sload_le(base + off + c.len, 4));
  }
  c.ptr = base + off;
  return c;
}

// Covered length of block b alone, per lane (the scans for long blocks).
template <bool kFresh>
__device__ __forceinline__ uint32_t mode_covered_len(const KernelArgs& a, uint32_t b) {
  if (mode_is_log(a.mode)) {
    const uint8_t* h = a.base + lane_ld<kFresh>(a, a.offsets + b);
    return 1u + (static_cast<uint32_t>(h[4]) | (static_cast<uint32_t>(h[5]) << 8));
  }
  return (a.offsets == nullptr ? a.length : lane_ld<kFresh>(a, a.lengths + b)) + (mode_is_sst(a.mode) ? 1u : 0u);
}

// ---- what lane 0 stores --------------------------------------------------

// Table of entry e in kModeSstTable: the last report whose first <= e.
__device__ __forceinline__ uint32_t sst_table_of(const KernelArgs& a,
                                                 const lvkv_sst_report* reports, uint32_t ntables,
                                                 uint32_t e) {
  uint32_t lo = 0, hi = ntables;  // answer in [lo, hi)
  while (hi - lo > 1) {
    const uint32_t mid = (lo + hi) >> 1;
    if (lane_ld<true>(a, &reports[mid].first) <= e) lo = mid; else hi = mid;
  }
  return lo;
}

// Block b's result (covered [ptr, ptr + len), CRC `crc`) in the batch's mode.
// kTable: the kernel serves kModeSstTable (the ragged walk alone).
template <bool kTable>
__device__ __forceinline__ void mode_store(const KernelArgs& a, uint32_t b, uint64_t ptr,
                                           uint32_t len, uint32_t expected, uint32_t crc) {
  if (lane_id() != 0) return;
  if (kTable && a.mode == kModeSstTable) {
    // ReadBlock's order (format.cc:92-97, :104-158): the index parse status
    // first, then the checksum, then the type byte
    uint8_t st = lane_ld<true>(a, a.out_status + b);
    a.out_crc[b] = st == LVKV_BLOCK_OK ? crc : 0u;  // no CRC of an unreadable block
    if (st == LVKV_BLOCK_OK) {
      const uint8_t type = *reinterpret_cast<const uint8_t*>(ptr + len - 1);
      if (crc != expected)
        st = LVKV_BLOCK_CHECKSUM;
      else if (type == 1 || type == 2)  // snappy / zstd: absent in the as-built
        st = LVKV_BLOCK_COMPRESSED;     // reference (port_stdcxx.h:108-118)
      else if (type > 2)
        st = LVKV_BLOCK_BAD_TYPE;
      if (st != LVKV_BLOCK_OK) a.out_status[b] = st;
    }
    if (st != LVKV_BLOCK_OK) {
      lvkv_sst_report* reps = static_cast<lvkv_sst_report*>(a.sst_reports);
      lvkv_sst_report* r = reps + sst_table_of(a, reps, a.sst_ntables, b);
      atomicAdd(&r->nbad, 1u);
      atomicMin(&r->first_bad, b - lane_ld<true>(a, &r->first));
    }
  } else if (a.mode == kModeCompute) {
    a.out_crc[b] = a.mask ? crc_mask(crc) : crc;
  } else if (a.mode == kModeSstFill || a.mode == kModeLogFill) {
    // the stored form (Mask, little-endian): trailer bytes 1..4 follow the
    // covered n + 1 bytes; the header's CRC sits 6 bytes before the covered
    // type byte
    uint8_t* dst = reinterpret_cast<uint8_t*>(a.mode == kModeSstFill ? ptr + len : ptr - 6);
    const uint32_t m = crc_mask(crc);
#pragma unroll
    for (int k = 0; k < 4; ++k) dst[k] = static_cast<uint8_t>(m >> (8 * k));
    if (a.out_crc != nullptr) a.out_crc[b] = crc;
  } else {  // kModeSstVerify, kModeLogVerify
    a.out_crc[b] = crc;
    if (a.out_status != nullptr) a.out_status[b] = crc != expected ? 1 : 0;
  }
}

}  // namespace
}  // namespace lvkv

#endif  // LVKV_CRC32C_MODES_H_
