// LevelDB's table format as the device reads and writes it, stated once: the
// fixed-width and varint codings (util/coding.cc), a block's entries and
// restart array (table/block.cc, table/block_builder.cc), the Bloom hash
// (util/hash.cc, util/bloom.cc) and the constants of the footer and the filter
// block (table/format.h, table/filter_block.cc). Used by the table verifier
// (lvkv_sst_table.hip), the table finisher (lvkv_sst_finish.hip), the block
// builder (lvkv_sst_build.hip), and the block walker (lvkv_sst_entries.hip)
// and the point lookups (lvkv_sst_get.hip), which take decode_entry but not
// block_restarts / block_run: Block::Iter's walk and its Seek accept blocks
// those two refuse.
#ifndef LVKV_TABLE_FORMAT_H_
#define LVKV_TABLE_FORMAT_H_

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace lvkv {

constexpr uint64_t kTableMagic = 0xdb4775248b80fb57ull;  // table/format.h:76
constexpr uint64_t kFooterLen = 48;      // table/format.h:53 (2 * 20 + 8)
constexpr uint32_t kFilterBaseLg = 11;   // table/filter_block.cc:16

__device__ __forceinline__ uint32_t ld_le32(const uint8_t* p) {
  return static_cast<uint32_t>(p[0]) | (static_cast<uint32_t>(p[1]) << 8) |
         (static_cast<uint32_t>(p[2]) << 16) | (static_cast<uint32_t>(p[3]) << 24);
}

__device__ __forceinline__ void st_le32(uint8_t* p, uint32_t v) {
  for (int k = 0; k < 4; ++k) p[k] = static_cast<uint8_t>(v >> (8 * k));
}

__device__ __forceinline__ uint64_t ld_le64(const uint8_t* p) {
  uint64_t v = 0;
  for (int b = 7; b >= 0; --b) v = (v << 8) | p[b];
  return v;
}

// GetVarint32Ptr / GetVarint64Ptr (util/coding.cc) over [p, limit), in T's
// arithmetic: bytes consumed, 0 on failure (runs past `limit` or longer than
// the type allows).
template <typename T>
__device__ __forceinline__ uint32_t get_varint(const uint8_t* p, const uint8_t* limit, T* v) {
  static_assert(sizeof(T) == 4 || sizeof(T) == 8, "a varint32 or a varint64");
  constexpr uint32_t max_shift = sizeof(T) == 4 ? 28 : 63;
  T result = 0;
  uint32_t i = 0;
  for (uint32_t shift = 0; shift <= max_shift && p + i < limit; shift += 7, ++i) {
    const T b = p[i];
    if (b & 128) {
      result |= (b & 127) << shift;
    } else {
      *v = result | (b << shift);
      return i + 1;
    }
  }
  return 0;
}

// VarintLength and EncodeVarint32 / EncodeVarint64 (util/coding.cc), in T's
// arithmetic; put_varint returns the byte after the varint.
template <typename T>
__device__ __forceinline__ uint32_t varint_len(T v) {
  uint32_t n = 1;
  if constexpr (sizeof(T) == 4) {  // four compares, no branch
    for (uint32_t s = 7; s < 32; s += 7) n += v >= (T{1} << s);
  } else {  // (handles: a byte or three, seldom more)
    for (; v >= 128; v >>= 7) ++n;
  }
  return n;
}

template <typename T>
__device__ __forceinline__ uint8_t* put_varint(uint8_t* p, T v) {
  while (v >= 128u) {
    *p++ = static_cast<uint8_t>(v | 128u);
    v >>= 7;
  }
  *p++ = static_cast<uint8_t>(v);
  return p;
}

// DecodeEntry (table/block.cc:55-75) over [p, limit): the key delta, or
// nullptr when a varint or the entry's bytes run past limit.
__device__ __forceinline__ const uint8_t* decode_entry(const uint8_t* p, const uint8_t* limit,
                                                       uint32_t* shared, uint32_t* non_shared,
                                                       uint32_t* value_len) {
  if (limit - p < 3) return nullptr;
  uint32_t n;
  if ((n = get_varint(p, limit, shared)) == 0) return nullptr;
  p += n;
  if ((n = get_varint(p, limit, non_shared)) == 0) return nullptr;
  p += n;
  if ((n = get_varint(p, limit, value_len)) == 0) return nullptr;
  p += n;
  if (static_cast<uint64_t>(limit - p) < static_cast<uint64_t>(*non_shared) + *value_len)
    return nullptr;
  return p;
}

// The restart array of a block of L bytes (table/block.cc:28-45): false when
// the count does not fit; else the count and where the entries end.
__device__ __forceinline__ bool block_restarts(const uint8_t* p, uint32_t L, uint32_t* nr,
                                               uint32_t* limit) {
  if (L < 8) return false;  // (a count and at least one restart)
  const uint32_t c = ld_le32(p + L - 4);
  if (c == 0 || c > (L - 4) / 4) return false;
  *nr = c;
  *limit = L - 4 - 4 * c;
  return true;
}

// Run r of a block: [*s, *e) of the entries; false when the restart offsets
// do not delimit a run inside them (BlockBuilder's are increasing from 0, and
// a run ends where the next begins).
__device__ __forceinline__ bool block_run(const uint8_t* p, uint32_t nr, uint32_t limit, uint32_t r,
                                          uint32_t* s, uint32_t* e) {
  const uint8_t* ra = p + limit;
  *s = ld_le32(ra + 4 * r);
  *e = r + 1 < nr ? ld_le32(ra + 4 * (r + 1)) : limit;
  return (r != 0 || *s == 0) && *s < *e && *e <= limit;
}

// Hash (util/hash.cc) with BloomHash's seed (util/bloom.cc:15).
__device__ __forceinline__ uint32_t bloom_hash(const uint8_t* d, uint32_t n) {
  const uint32_t m = 0xc6a4a793u;
  uint32_t h = 0xbc9f1d34u ^ (n * m);
  uint32_t i = 0;
  for (; i + 4 <= n; i += 4) {
    h += ld_le32(d + i);
    h *= m;
    h ^= h >> 16;
  }
  const uint32_t rem = n - i;
  if (rem == 3) h += static_cast<uint32_t>(d[i + 2]) << 16;
  if (rem >= 2) h += static_cast<uint32_t>(d[i + 1]) << 8;
  if (rem >= 1) {
    h += d[i];
    h *= m;
    h ^= h >> 24;
  }
  return h;
}

}  // namespace lvkv

#endif  // LVKV_TABLE_FORMAT_H_
