// Table::InternalGet for a batch of keys on the device (table/table.cc:214-242),
// in two calls the caller decodes the touched data blocks between:
//
//   locate  Block::Iter::Seek in the decoded index block (table/block.cc:165-228),
//           BlockHandle::DecodeFrom on the entry it stops at, and
//           FilterBlockReader::KeyMayMatch (table/filter_block.cc:77-104) with
//           BloomFilterPolicy::KeyMayMatch (util/bloom.cc:56-80);
//   seek    the same Seek in one decoded data block a query, and SaveValue
//           (db/version_set.cc:263-276) on the entry it stops at.
//
// A lane a query in both: the work of a query is a chain of dependent loads
// (a bisection over the restart array, then a walk of at most a restart run)
// and no two queries share a step of it.
//
// The walk never restores a key. Block::Iter keeps key_ as a string because
// it hands it out; a seek needs only the order of key_ against one fixed
// target, and that is carried from entry to entry in three words: key_'s
// length, the length cp of the prefix it has in common with the target, and
// key_'s byte at cp. An entry that shares more than cp bytes with its
// predecessor differs from the target where the predecessor did; one that
// shares cp or fewer is compared from its delta on. That is exact for keys
// of any length. Under key_format 1 the comparator also needs key_'s last 8
// bytes where the user keys are equal, and the outputs need them for the tag:
// they are carried along as a word while they can be had from the delta and
// the predecessor's last 8 bytes (always, where an entry is no shorter than
// its predecessor or brings 8 bytes of its own), and otherwise taken by
// walking the run once more and noting which delta each of the 8 bytes came
// from (tail_by_walk) -- only when they are needed.
//
// The ordinal of an index entry in the index's forward order is the entries
// before its restart run plus its place in the run. get_count_kernel counts
// every run and says whether it is well formed (begins with shared == 0,
// decodes, ends exactly where the next begins), one scan numbers the entries
// and the runs that are not, and a query with such a run before its own counts
// from restart[0] by itself, as SeekToFirst + Next would.
//
// Counts of the per-query verdicts: a ballot a wave and status, the waves'
// counts added up in LDS and left in a slot of the workgroup's own, which a
// report kernel of one workgroup adds up. No atomic (an atomicAdd a wave on
// the report's one line was half of either call's time). Every
// dependency between workgroups is a kernel boundary.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lvkv_launch.h"
#include "lvkv_scratch.h"
#include "lvkv_snappy.h"
#include "lvkv_table_format.h"

namespace lvkv {
namespace {

constexpr uint32_t kNone = 0xffffffffu;
constexpr uint32_t kGroup = 256;  // lanes, and queries, a workgroup
constexpr uint32_t kWaves = kGroup / 64;
constexpr uint32_t kSlot = 8;     // counts a workgroup leaves: a u32 a status, 8 at the most
static_assert(LVKV_GET_NSTATUS <= kSlot && LVKV_GET_NSTATE <= kSlot, "a status a count");
static_assert(kGroup % kSlot == 0, "sum_slots' threads of a count");

constexpr uint64_t groups_of(uint64_t n) { return (n + kGroup - 1) / kGroup; }

// ---- comparing keys ----------------------------------------------------------

// Eight bytes from any address (block bytes are rarely aligned; the target
// allows unaligned global loads, and the compiler issues one).
__device__ __forceinline__ uint64_t ld_word(const uint8_t* p) {
  uint64_t v;
  __builtin_memcpy(&v, p, 8);
  return v;
}

// The bytes a and b have in common at their start, of m: eight a step (the
// first byte in memory is the word's lowest), then a byte at a time.
__device__ __forceinline__ uint32_t common_prefix(const uint8_t* a, const uint8_t* b, uint32_t m) {
  uint32_t l = 0;
  while (m - l >= 8u) {
    const uint64_t x = ld_word(a + l) ^ ld_word(b + l);
    if (x != 0) return l + (static_cast<uint32_t>(__builtin_ctzll(x)) >> 3);
    l += 8u;
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

// The call's comparator over two keys in memory. key_format 1:
// InternalKeyComparator (db/dbformat.cc:47-63), both keys 8 bytes or longer.
__device__ __forceinline__ int compare_keys(uint32_t key_format, const uint8_t* a, uint32_t alen,
                                            const uint8_t* b, uint32_t blen) {
  if (key_format == 0) return compare_bytes(a, alen, b, blen);
  const int c = compare_bytes(a, alen - 8u, b, blen - 8u);
  if (c != 0) return c;
  const uint64_t ta = ld_le64(a + alen - 8u), tb = ld_le64(b + blen - 8u);
  return ta > tb ? -1 : ta < tb ? 1 : 0;
}

// ---- Block::Iter::Seek --------------------------------------------------------

enum : uint32_t {
  kSeekValid,     // Valid(): the fields below describe the entry
  kSeekEnd,       // !Valid(), status OK (the walk reached the restart array; no restarts)
  kSeekCorrupt,   // CorruptionError ("bad entry in block"), or a key under 8 bytes (format 1)
  kSeekBadBlock,  // the error iterator ("bad block contents")
};

struct Hit {
  uint32_t verdict;
  uint32_t off;       // the entry's offset in the block
  uint32_t left;      // the restart run the walk went through
  uint32_t steps;     // entries of it the walk parsed, this one included
  uint32_t klen;      // the entry's restored key: its length,
  uint32_t cp;        // the bytes it has in common with the target at its start,
  uint64_t tail;      // and (key_format 1) its last 8 bytes, little-endian
  uint32_t val_off, val_len;  // the value, in the block
};

// The last 8 bytes of the key of the entry at `cur`, klen long, of the run
// walked from `start`: every entry up to it says which of them its delta
// holds, and the last to say so is right (a byte a later entry shares was
// there before it). The entries were decoded once already and are sound.
__device__ __forceinline__ uint64_t tail_by_walk(const uint8_t* b, uint32_t limit, uint32_t start,
                                                 uint32_t cur, uint32_t klen) {
  uint64_t tail = 0;
  uint32_t at = start;
  for (;;) {
    uint32_t sh = 0, ns = 0, vl = 0;
    const uint8_t* kp = decode_entry(b + at, b + limit, &sh, &ns, &vl);
    if (kp == nullptr) return tail;  // (never: the walk passed here)
#pragma unroll
    for (uint32_t k = 0; k < 8; ++k) {
      const uint32_t p = klen - 8u + k;
      if (p >= sh && p - sh < ns)
        tail = (tail & ~(uint64_t{0xff} << (8u * k))) | (uint64_t{kp[p - sh]} << (8u * k));
    }
    if (at == cur) return tail;
    at = static_cast<uint32_t>(kp - b) + ns + vl;
  }
}

// Seek(target) on a fresh iterator over the block b of L bytes
// (Block::NewIterator, table/block.cc:281-291, then :165-228 without the
// branch for an iterator that already stands somewhere).
__device__ __forceinline__ Hit seek_block(const uint8_t* b, uint32_t L, const uint8_t* t,
                                          uint32_t tlen, uint32_t key_format) {
  Hit h{};
  h.off = kNone;
  h.verdict = kSeekBadBlock;
  if (L < 4u) return h;
  const uint32_t nr = ld_le32(b + L - 4u);
  if (nr > (L - 4u) / 4u) return h;
  h.verdict = kSeekEnd;
  if (nr == 0) return h;  // NewEmptyIterator
  const uint32_t limit = L - 4u - 4u * nr;
  const uint8_t* ra = b + limit;
  h.verdict = kSeekCorrupt;

  uint32_t left = 0, right = nr - 1u;
  while (left < right) {
    const uint32_t mid = (left + right + 1u) / 2u;  // (nr <= 2^30: no wrap)
    const uint32_t ro = ld_le32(ra + 4u * mid);
    uint32_t sh = 0, ns = 0, vl = 0;
    // (an offset past the restart array: limit - p < 3 as well)
    const uint8_t* kp = ro <= limit ? decode_entry(b + ro, b + limit, &sh, &ns, &vl) : nullptr;
    if (kp == nullptr || sh != 0) return h;
    if (key_format == 1 && ns < 8u) return h;
    if (compare_keys(key_format, kp, ns, t, tlen) < 0) left = mid;
    else right = mid - 1u;
  }

  // SeekToRestartPoint(left), then ParseNextKey until key_ >= target
  const uint32_t start = ld_le32(ra + 4u * left);
  const uint64_t ttag = key_format == 1 ? ld_le64(t + tlen - 8u) : 0;
  uint32_t at = start, klen = 0, cp = 0, steps = 0;
  uint32_t dbyte = 0;    // key_[cp], where cp < klen
  uint64_t tail = 0;     // key_'s last 8 bytes,
  bool tail_ok = false;  // where they could be carried along
  for (;;) {
    if (at >= limit) {  // p >= limit: no more entries
      h.verdict = kSeekEnd;
      return h;
    }
    uint32_t sh = 0, ns = 0, vl = 0;
    const uint8_t* kp = decode_entry(b + at, b + limit, &sh, &ns, &vl);
    if (kp == nullptr || sh > klen) return h;
    const uint32_t cur = at, plen = klen;
    klen = sh + ns;  // (<= the deltas walked so far: no wrap)
    if (key_format == 1 && klen < 8u) return h;
    if (sh <= cp) {
      const uint32_t room = tlen - sh;  // (sh <= cp <= tlen)
      const uint32_t l = common_prefix(kp, t + sh, ns < room ? ns : room);
      cp = sh + l;
      if (l < ns) dbyte = kp[l];
    }
    if (key_format == 1) {
      if (ns >= 8u) {
        tail = ld_le64(kp + ns - 8u);
        tail_ok = true;
      } else if (tail_ok && klen >= plen) {
        // the 8 - ns bytes before `sh` lie in the predecessor's last 8
        uint64_t own = 0;
        for (uint32_t k = 0; k < ns; ++k) own |= uint64_t{kp[k]} << (8u * k);
        const uint64_t kept = (tail >> (8u * (klen - plen))) & (~uint64_t{0} >> (8u * ns));
        tail = ns == 0 ? kept : kept | (own << (8u * (8u - ns)));
      } else {
        tail_ok = false;
      }
    }
    at = static_cast<uint32_t>(kp - b) + ns + vl;
    ++steps;

    int c;
    bool need_tail = false;
    if (key_format == 0) {
      const uint32_t m = klen < tlen ? klen : tlen;
      c = cp < m ? (dbyte < t[cp] ? -1 : 1) : klen < tlen ? -1 : klen > tlen ? 1 : 0;
    } else {
      const uint32_t ku = klen - 8u, tu = tlen - 8u, m = ku < tu ? ku : tu;
      if (cp < m) c = dbyte < t[cp] ? -1 : 1;
      else if (ku != tu) c = ku < tu ? -1 : 1;
      else if (cp == klen) c = 0;
      else {
        need_tail = true;
        c = -1;
      }
    }
    // (the tag decides the order, or the walk ends here and hands the tag out)
    if (key_format == 1 && !tail_ok && (need_tail || c >= 0)) {
      tail = tail_by_walk(b, limit, start, cur, klen);
      tail_ok = true;
    }
    if (need_tail) c = tail > ttag ? -1 : tail < ttag ? 1 : 0;
    if (c >= 0) {
      h.verdict = kSeekValid;
      h.off = cur;
      h.left = left;
      h.steps = steps;
      h.klen = klen;
      h.cp = cp;
      h.tail = tail;
      h.val_off = static_cast<uint32_t>(kp - b) + ns;
      h.val_len = vl;
      return h;
    }
  }
}

// The workgroup's count of every status (kNone: a lane without a query), to
// its slot. Every thread of the workgroup calls it.
__device__ __forceinline__ void count_statuses(uint32_t status, uint32_t* parts) {
  __shared__ uint32_t waves[kWaves][kSlot];
#pragma unroll
  for (uint32_t s = 0; s < kSlot; ++s) {
    const uint64_t m = __ballot(status == s);
    if ((threadIdx.x & 63u) == 0) waves[threadIdx.x / 64u][s] = static_cast<uint32_t>(__popcll(m));
  }
  __syncthreads();
  if (threadIdx.x < kSlot) {
    uint32_t c = 0;
    for (uint32_t w = 0; w < kWaves; ++w) c += waves[w][threadIdx.x];
    parts[uint64_t{blockIdx.x} * kSlot + threadIdx.x] = c;
  }
}

// One workgroup: thread t adds up count t % kSlot of the slots t / kSlot, t /
// kSlot + kGroup / kSlot, ..; the threads of a count are then added up in LDS.
// Every thread calls it; threads 0 .. kSlot - 1 return their count's total.
__device__ __forceinline__ uint32_t sum_slots(const uint32_t* parts, uint32_t groups) {
  __shared__ uint32_t part[kGroup];
  uint32_t c = 0;
  for (uint32_t g = threadIdx.x / kSlot; g < groups; g += kGroup / kSlot)
    c += parts[uint64_t{g} * kSlot + threadIdx.x % kSlot];
  part[threadIdx.x] = c;
  __syncthreads();
  uint32_t total = 0;
  if (threadIdx.x < kSlot)
    for (uint32_t t = threadIdx.x; t < kGroup; t += kSlot) total += part[t];
  return total;
}

// ---- locate ---------------------------------------------------------------------

struct Loc {
  const uint8_t* index;
  uint32_t index_len;
  const uint8_t* filter;  // may be null
  uint32_t filter_len;
  const uint8_t* qkeys;
  const uint64_t* qoff;
  const uint32_t* qlen;
  uint32_t n, key_format;
  uint32_t max_runs;  // (index_len - 4) / 4: the most restarts the block can hold
  uint64_t* before;   // max_runs + 1: a run's entries, then their scan
  uint64_t* bad;      // max_runs + 1: 1 for a run that is not well formed, then their scan
  uint64_t* sums;
  uint32_t* parts;    // kSlot counts a workgroup of the locate kernel
  uint32_t* q_block;
  uint64_t* q_handle_off;
  uint32_t* q_handle_size;
  uint8_t* q_status;
};

__global__ void __launch_bounds__(kGroup)
get_locate_report_kernel(const uint32_t* parts, uint32_t groups, uint32_t n,
                         lvkv_sst_get_locate_report* r) {
  const uint32_t total = sum_slots(parts, groups);
  if (threadIdx.x < LVKV_GET_NSTATUS) r->count[threadIdx.x] = total;
  if (threadIdx.x == 0) {
    r->nqueries = n;
    r->reserved_ = 0;
  }
}

// A lane a restart run of the index block: its entries, where it is well
// formed. Slots past the block's restart count get 0.
__global__ void __launch_bounds__(kGroup) get_count_kernel(Loc d) {
  const uint32_t r = blockIdx.x * kGroup + threadIdx.x;
  if (r >= d.max_runs) return;
  const uint8_t* b = d.index;
  const uint32_t L = d.index_len;
  uint32_t nr = ld_le32(b + L - 4u);  // (max_runs != 0: L >= 8)
  if (nr > (L - 4u) / 4u) nr = 0;     // (no iterator: nothing is numbered)
  uint64_t cnt = 0, bad = 0;
  if (r < nr) {
    const uint32_t limit = L - 4u - 4u * nr;
    const uint32_t s = ld_le32(b + limit + 4u * r);
    const uint32_t e = r + 1u < nr ? ld_le32(b + limit + 4u * (r + 1u)) : limit;
    bool ok = s < e && e <= limit;
    uint32_t at = s, klen = 0;
    while (ok && at < e) {
      uint32_t sh = 0, ns = 0, vl = 0;
      const uint8_t* kp = decode_entry(b + at, b + limit, &sh, &ns, &vl);
      if (kp == nullptr || sh > klen) {  // (klen 0 at the run's start: shared == 0 there)
        ok = false;
        break;
      }
      klen = sh + ns;
      at = static_cast<uint32_t>(kp - b) + ns + vl;
      ++cnt;
    }
    if (!ok || at != e) bad = 1;
  }
  d.before[r] = cnt;
  d.bad[r] = bad;
}

// The entries SeekToFirst + Next hand out before the one at `off`, kNone when
// that walk does not come by it.
__device__ uint32_t ordinal_by_walk(const uint8_t* b, uint32_t L, uint32_t off) {
  const uint32_t nr = ld_le32(b + L - 4u);
  const uint32_t limit = L - 4u - 4u * nr;
  uint32_t at = ld_le32(b + limit), klen = 0, n = 0;
  while (at < off && at < limit) {
    uint32_t sh = 0, ns = 0, vl = 0;
    const uint8_t* kp = decode_entry(b + at, b + limit, &sh, &ns, &vl);
    if (kp == nullptr || sh > klen) return kNone;
    klen = sh + ns;
    at = static_cast<uint32_t>(kp - b) + ns + vl;
    ++n;
  }
  return at == off ? n : kNone;
}

// BloomFilterPolicy::KeyMayMatch (util/bloom.cc:56-80).
__device__ bool bloom_may_match(const uint8_t* key, uint32_t klen, const uint8_t* f, uint32_t len) {
  if (len < 2u) return false;
  const uint64_t bits = (uint64_t{len} - 1u) * 8u;
  const uint32_t k = f[len - 1u];
  if (k > 30u) return true;  // (a byte of 0x80 and more is a huge size_t there: the same answer)
  uint32_t h = bloom_hash(key, klen);
  const uint32_t delta = (h >> 17) | (h << 15);
  for (uint32_t j = 0; j < k; ++j) {
    const uint32_t bitpos = static_cast<uint32_t>(h % bits);
    if ((f[bitpos / 8u] & (1u << (bitpos % 8u))) == 0) return false;
    h += delta;
  }
  return true;
}

// FilterBlockReader's constructor and KeyMayMatch (table/filter_block.cc:77-104).
__device__ bool filter_may_match(const uint8_t* f, uint32_t n, uint64_t block_offset,
                                 const uint8_t* key, uint32_t klen) {
  if (n < 5u) return true;  // (num_ stays 0)
  const uint32_t base_lg = f[n - 1u];
  const uint32_t last_word = ld_le32(f + n - 5u);
  if (last_word > n - 5u) return true;
  const uint32_t num = (n - 5u - last_word) / 4u;
  // (a shift of 64 and more is undefined there; here it leaves 0)
  const uint64_t index = base_lg < 64u ? block_offset >> base_lg : 0;
  if (index < num) {
    const uint8_t* o = f + last_word + 4u * static_cast<uint32_t>(index);
    const uint32_t start = ld_le32(o), limit = ld_le32(o + 4u);
    if (start <= limit && limit <= last_word)
      return bloom_may_match(key, klen, f + start, limit - start);
    if (start == limit) return false;  // empty filters match no key
  }
  return true;  // errors are potential matches
}

__global__ void __launch_bounds__(kGroup) get_locate_kernel(Loc d) {
  const uint32_t q = blockIdx.x * kGroup + threadIdx.x;
  uint32_t status = kNone;
  if (q < d.n) {
    const uint8_t* t = d.qkeys + d.qoff[q];
    const uint32_t tlen = d.qlen[q];
    uint32_t block = kNone, hsize = 0;
    uint64_t hoff = 0;
    if (d.key_format == 1 && tlen < 8u) {
      status = LVKV_GET_BAD_KEY;
    } else {
      const Hit h = seek_block(d.index, d.index_len, t, tlen, d.key_format);
      if (h.verdict == kSeekEnd) {
        status = LVKV_GET_PAST_END;
      } else if (h.verdict != kSeekValid) {
        status = LVKV_GET_INDEX_CORRUPT;
      } else {
        // (every run before the walk's is well formed: the scan says how many entries)
        block = d.bad[h.left] == 0 ? static_cast<uint32_t>(d.before[h.left]) + h.steps - 1u
                                   : ordinal_by_walk(d.index, d.index_len, h.off);
        // BlockHandle::DecodeFrom (table/format.cc:23-31)
        const uint8_t* v = d.index + h.val_off;
        const uint8_t* vend = v + h.val_len;
        uint64_t off = 0, size = 0;
        const uint32_t n0 = get_varint(v, vend, &off);
        const uint32_t n1 = n0 != 0 ? get_varint(v + n0, vend, &size) : 0;
        if (n1 == 0 || size > 0xffffffffull) {
          status = LVKV_GET_BAD_HANDLE;
        } else {
          hoff = off;
          hsize = static_cast<uint32_t>(size);
          status = LVKV_GET_BLOCK;
          if (d.filter != nullptr &&
              !filter_may_match(d.filter, d.filter_len, off, t,
                                d.key_format == 1 ? tlen - 8u : tlen))
            status = LVKV_GET_FILTERED;
        }
      }
    }
    d.q_block[q] = block;
    d.q_handle_off[q] = hoff;
    d.q_handle_size[q] = hsize;
    d.q_status[q] = static_cast<uint8_t>(status);
  }
  count_statuses(status, d.parts);
}

// ---- seek -----------------------------------------------------------------------

struct Sk {
  const uint8_t* raw;
  const uint64_t* raw_off;
  const uint32_t* raw_len;
  const uint8_t* skip;  // may be null
  uint32_t nblocks;
  const uint8_t* qkeys;
  const uint64_t* qoff;
  const uint32_t* qlen;
  const uint32_t* q_slot;
  uint32_t n, key_format;
  uint32_t* hit_off;
  uint64_t* val_off;
  uint32_t* val_len;
  uint64_t* tag;
  uint8_t* state;
  uint32_t* parts;  // kSlot counts a workgroup of the seek kernel
};

__global__ void __launch_bounds__(kGroup)
get_seek_report_kernel(const uint32_t* parts, uint32_t groups, uint32_t n,
                       lvkv_sst_get_seek_report* r) {
  const uint32_t total = sum_slots(parts, groups);
  if (threadIdx.x < LVKV_GET_NSTATE) r->count[threadIdx.x] = total;
  if (threadIdx.x == 0) r->nqueries = n;
}

__global__ void __launch_bounds__(kGroup) get_seek_kernel(Sk d) {
  const uint32_t q = blockIdx.x * kGroup + threadIdx.x;
  uint32_t state = kNone;
  if (q < d.n) {
    const uint8_t* t = d.qkeys + d.qoff[q];
    const uint32_t tlen = d.qlen[q];
    const uint32_t slot = d.q_slot[q];
    uint32_t hit = kNone, vlen = 0;
    uint64_t voff = 0, tag = 0;
    if (d.key_format == 1 && tlen < 8u) {
      state = LVKV_GET_STATE_BAD_KEY;
    } else if (slot == kNone) {
      state = LVKV_GET_STATE_NOT_FOUND;
    } else if (slot >= d.nblocks || (d.skip != nullptr && d.skip[slot] != 0)) {
      state = LVKV_GET_STATE_UNREADABLE;
    } else {
      const uint64_t base = d.raw_off[slot];
      const Hit h = seek_block(d.raw + base, d.raw_len[slot], t, tlen, d.key_format);
      if (h.verdict == kSeekBadBlock) {
        state = LVKV_GET_STATE_BAD_BLOCK;
      } else if (h.verdict == kSeekCorrupt) {
        state = LVKV_GET_STATE_BAD_ENTRY;
      } else if (h.verdict == kSeekEnd) {
        state = LVKV_GET_STATE_NOT_FOUND;
      } else {
        hit = h.off;
        voff = base + h.val_off;
        vlen = h.val_len;
        state = LVKV_GET_STATE_NOT_FOUND;
        if (d.key_format == 0) {
          if (h.klen == tlen && h.cp == tlen) state = LVKV_GET_STATE_FOUND;
        } else {  // SaveValue (db/version_set.cc:263-276)
          tag = h.tail;
          const uint32_t type = static_cast<uint32_t>(tag & 0xffu);
          if (type > 1u) state = LVKV_GET_STATE_CORRUPT_KEY;  // ParseInternalKey
          else if (h.klen == tlen && h.cp >= tlen - 8u)
            state = type == 1u ? LVKV_GET_STATE_FOUND : LVKV_GET_STATE_DELETED;
        }
      }
    }
    d.hit_off[q] = hit;
    d.val_off[q] = voff;
    d.val_len[q] = vlen;
    d.tag[q] = tag;
    d.state[q] = static_cast<uint8_t>(state);
  }
  count_statuses(state, d.parts);
}

// The locate call's scratch, listed once. Returns the bytes from `base` (null:
// sizing only).
uint64_t carve(Loc& d, uint8_t* base, uint64_t max_runs, uint64_t n) {
  Carver c(base);
  d.before = c.take<uint64_t>(max_runs + 1, 16);
  d.bad = c.take<uint64_t>(max_runs + 1, 16);
  d.sums = c.take<uint64_t>(scan_sums_words(max_runs), 16);
  d.parts = c.take<uint32_t>(groups_of(n) * kSlot, 16);
  return c.bytes();
}

uint32_t max_runs_of(uint32_t index_len) { return index_len >= 8u ? (index_len - 4u) / 4u : 0u; }

}  // namespace

size_t sst_get_locate_scratch_bytes(uint32_t index_len, size_t nqueries) {
  Loc d{};
  return kScratchAlign + carve(d, nullptr, max_runs_of(index_len), nqueries);  // alignment slack
}

size_t sst_get_seek_scratch_bytes(size_t nqueries) {
  return kScratchAlign + ((groups_of(nqueries) * kSlot * sizeof(uint32_t) + 15u) & ~uint64_t{15});
}

hipError_t launch_sst_get_locate(const SstGetLocateArgs& a, hipStream_t stream) {
  if (a.n == 0) {
    hipLaunchKernelGGL(get_locate_report_kernel, dim3(1), dim3(kGroup), 0, stream,
                       static_cast<const uint32_t*>(nullptr), 0u, 0u, a.report);
    return hipGetLastError();
  }
  Loc d{};
  d.index = a.index;
  d.index_len = a.index_len;
  d.filter = a.filter;
  d.filter_len = a.filter_len;
  d.qkeys = a.qkeys;
  d.qoff = a.qkey_off;
  d.qlen = a.qkey_len;
  d.n = a.n;
  d.key_format = a.key_format;
  d.max_runs = max_runs_of(a.index_len);
  carve(d, scratch_base(a.scratch), d.max_runs, d.n);
  d.q_block = a.q_block;
  d.q_handle_off = a.q_handle_off;
  d.q_handle_size = a.q_handle_size;
  d.q_status = a.q_status;
  const uint32_t groups = static_cast<uint32_t>(groups_of(d.n));
  if (d.max_runs != 0) {
    hipLaunchKernelGGL(get_count_kernel, dim3((d.max_runs + kGroup - 1u) / kGroup), dim3(kGroup), 0,
                       stream, d);
    const hipError_t e = launch_exclusive_scan(d.before, d.bad, d.sums, d.max_runs, stream);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(get_locate_kernel, dim3(groups), dim3(kGroup), 0, stream, d);
  hipLaunchKernelGGL(get_locate_report_kernel, dim3(1), dim3(kGroup), 0, stream, d.parts, groups,
                     d.n, a.report);
  return hipGetLastError();
}

hipError_t launch_sst_get_seek(const SstGetSeekArgs& a, hipStream_t stream) {
  if (a.n == 0) {
    hipLaunchKernelGGL(get_seek_report_kernel, dim3(1), dim3(kGroup), 0, stream,
                       static_cast<const uint32_t*>(nullptr), 0u, 0u, a.report);
    return hipGetLastError();
  }
  Sk d{};
  d.raw = a.raw;
  d.raw_off = a.raw_off;
  d.raw_len = a.raw_len;
  d.skip = a.skip;
  d.nblocks = a.nblocks;
  d.qkeys = a.qkeys;
  d.qoff = a.qkey_off;
  d.qlen = a.qkey_len;
  d.q_slot = a.q_slot;
  d.n = a.n;
  d.key_format = a.key_format;
  d.hit_off = a.hit_off;
  d.val_off = a.val_off;
  d.val_len = a.val_len;
  d.tag = a.tag;
  d.state = a.state;
  d.parts = reinterpret_cast<uint32_t*>(scratch_base(a.scratch));
  const uint32_t groups = static_cast<uint32_t>(groups_of(d.n));
  hipLaunchKernelGGL(get_seek_kernel, dim3(groups), dim3(kGroup), 0, stream, d);
  hipLaunchKernelGGL(get_seek_report_kernel, dim3(1), dim3(kGroup), 0, stream, d.parts, groups, d.n,
                     a.report);
  return hipGetLastError();
}

}  // namespace lvkv
