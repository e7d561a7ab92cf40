// Block::Iter's forward walk over decoded data blocks on the device
// (table/block.cc:77-279): the inverse of lvkv_sst_build.hip. Blocks go in,
// the entries come out in the layout lvkv_sst_build_blocks_device takes:
// restored keys packed 8 bytes apart, values left where they are.
//
// A key depends on the key before it only inside a restart run, and a run
// whose first entry has shared == 0 is self-contained. So the counts are
// taken a run a lane (entries_count_kernel, a wave a block) and checked on
// the way: a block is `clean` when every run begins with shared == 0, decodes
// without error and ends exactly where the next begins (the last on the
// entries' end) -- then the runs laid end to end are what the serial walk
// from restart[0] sees. Any other block (restart arrays that lie, a bad
// entry, a restart-point entry with a legal shared != 0) is walked from
// restart[0] by one lane, the reference's loop, for its verdict and its
// count. The decision is per block, and both paths give the walk's result.
//
// Scans over the blocks place the runs' slots, the blocks' entries and their
// key bytes; entries_report_kernel decides the status with every count known
// and nothing written yet; entries_write_kernel copies, 16 lanes a run, only
// when that status is OK. Every dependency between workgroups is a kernel
// boundary.
//
// The write kernel never reads d_keys. A group keeps the first
// kEntriesKeyWindow bytes of its running key in LDS, word w always in the
// hands of lane w % 16, which is the only lane to read or write it: no
// ordering between lanes is needed. A byte of a longer key past the window
// that the entry shares with its predecessor is traced back, from the run's
// start, to the delta in d_raw it came from (quadratic in the run; the window
// holds every key the tables of db/ have).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lvkv_block_scan.h"
#include "lvkv_launch.h"
#include "lvkv_scratch.h"
#include "lvkv_snappy.h"
#include "lvkv_table_format.h"

namespace lvkv {
namespace {

constexpr uint32_t kNone = 0xffffffffu;
constexpr uint32_t kGroup = 16;                 // lanes a run in the write kernel
constexpr uint32_t kGroupsPerWave = 64 / kGroup;
constexpr uint32_t kBlocksPerGroup = 4;          // blocks a workgroup of 256
constexpr uint32_t kKeyWords = kEntriesKeyWindow / 4;
// a group's window, padded so that the four groups of a wave sit on
// different LDS banks
constexpr uint32_t kKeyStride = kKeyWords + 16;

// A clean block's run: where its entries and key bytes go, from the block's.
struct Slot {
  uint64_t key_rel;
  uint32_t ent_rel;
  uint32_t count;
};
static_assert(sizeof(Slot) == 16, "the sizing function counts 16 bytes a slot");

struct Ctl {
  uint32_t status;  // the report's, for the write kernel
};

struct Dev {
  const uint8_t* raw;
  const uint64_t* raw_off;
  const uint32_t* raw_len;
  const uint8_t* skip;
  uint32_t n;
  Ctl* ctl;
  uint64_t* slot_first;  // n + 1: a block's slots (its restart count, 0 where it gets none)
  uint64_t* key_first;   // n + 1: a block's key bytes, each key rounded up to 8
  uint64_t* val_bytes;   // n
  uint32_t* max_key;     // n
  uint32_t* last_key;    // n: the length of the block's last key
  uint8_t* clean;        // n: 1: the runs are in the slots
  uint64_t* sums;        // the scans' tile sums
  Slot* slots;
  uint64_t nslots;
  uint8_t* keys;
  uint64_t key_capacity;
  uint64_t* key_off;
  uint32_t* key_len;
  uint64_t* val_off;
  uint32_t* val_len;
  uint64_t max_entries;
  uint64_t* block_first;
  uint8_t* block_status;
  lvkv_sst_entries_report* report;
};

// Block::Block and Block::NewIterator (table/block.cc:25-40, 281-291).
struct Head {
  uint32_t status, nr, limit;
};

__device__ __forceinline__ Head block_head(const Dev& d, uint32_t b) {
  Head h{LVKV_ENTRIES_OK, 0, 0};
  if (d.skip != nullptr && d.skip[b] != 0) {
    h.status = LVKV_ENTRIES_SKIPPED;
    return h;
  }
  const uint32_t L = d.raw_len[b];
  if (L < 4) {
    h.status = LVKV_ENTRIES_BAD_BLOCK;
    return h;
  }
  const uint32_t nr = ld_le32(d.raw + d.raw_off[b] + L - 4);
  if (nr > (L - 4) / 4) {
    h.status = LVKV_ENTRIES_BAD_BLOCK;
    return h;
  }
  h.nr = nr;
  h.limit = L - 4 - 4 * nr;
  return h;
}

__device__ __forceinline__ uint64_t round8(uint32_t v) { return (uint64_t{v} + 7u) & ~uint64_t{7}; }

// What a run, or a whole walk, adds up to.
struct Sum {
  uint64_t key_bytes, val_bytes;
  uint32_t count, max_key, last_key;
};

// One more entry of the walk at `at` after a key of `prev` bytes: false where
// ParseNextKey calls CorruptionError. The sum of delta and value is
// decode_entry's, in 64 bits.
__device__ __forceinline__ bool next_entry(const uint8_t* p, uint32_t limit, uint32_t* at,
                                           uint32_t* prev, Sum* s, bool restart) {
  uint32_t sh, ns, vl;
  const uint8_t* q = decode_entry(p + *at, p + limit, &sh, &ns, &vl);
  if (q == nullptr || (restart ? sh != 0 : sh > *prev)) return false;
  const uint32_t klen = sh + ns;
  *at = static_cast<uint32_t>(q - p) + ns + vl;  // (<= limit: decode_entry saw to it)
  *prev = klen;
  ++s->count;
  s->key_bytes += round8(klen);
  s->val_bytes += vl;
  s->max_key = klen > s->max_key ? klen : s->max_key;
  s->last_key = klen;
  return true;
}

// Run r of a block of nr >= 1 restarts, as the clean path needs it: false
// unless it is exactly what the serial walk passes through.
__device__ bool parse_run(const uint8_t* p, const Head& h, uint32_t r, Sum* s) {
  const uint8_t* ra = p + h.limit;
  uint32_t at = ld_le32(ra + 4ull * r);
  const uint32_t end = r + 1 < h.nr ? ld_le32(ra + 4ull * (r + 1)) : h.limit;
  if (!(at < end && end <= h.limit)) return false;
  uint32_t prev = 0;
  bool restart = true;
  while (at < end) {
    if (!next_entry(p, h.limit, &at, &prev, s, restart)) return false;
    restart = false;
  }
  return at == end;
}

// SeekToFirst, then Next until !Valid() (table/block.cc:230-233, 251-278):
// the status the iterator ends with.
__device__ uint32_t walk(const uint8_t* p, const Head& h, Sum* s) {
  uint32_t at = ld_le32(p + h.limit);  // restart[0], wherever it points
  uint32_t prev = 0;
  while (at < h.limit)
    if (!next_entry(p, h.limit, &at, &prev, s, false)) return LVKV_ENTRIES_BAD_ENTRY;
  return LVKV_ENTRIES_OK;
}

// A report of no entries (nblocks == 0).
__global__ void entries_empty_kernel(lvkv_sst_entries_report* r) {
  if (threadIdx.x != 0) return;
  r->status = 0;
  r->nbad = 0;
  r->first_bad_block = kNone;
  r->max_key_len = 0;
  r->num_entries = 0;
  r->key_bytes = 0;
  r->value_bytes = 0;
}

// Per block: the slots its runs ask for. A run takes a restart and an entry
// of three bytes at least, so a block with more restarts than that allows
// cannot be clean and asks for none.
__global__ void __launch_bounds__(256) entries_head_kernel(Dev d) {
  const uint32_t b = blockIdx.x * 256u + threadIdx.x;
  if (b >= d.n) return;
  const Head h = block_head(d, b);
  uint32_t want = 0;
  if (h.status == LVKV_ENTRIES_OK && h.nr <= (d.raw_len[b] - 4u) / kEntriesRunBytes) want = h.nr;
  d.slot_first[b] = want;
}

__device__ __forceinline__ uint64_t shfl64(uint64_t v, uint32_t lane) {
  const uint32_t lo = __shfl(static_cast<uint32_t>(v), lane);
  const uint32_t hi = __shfl(static_cast<uint32_t>(v >> 32), lane);
  return (static_cast<uint64_t>(hi) << 32) | lo;
}

__device__ __forceinline__ uint64_t wave_inclusive(uint64_t v, uint32_t lane) {
  for (uint32_t o = 1; o < 64; o <<= 1) {
    const uint64_t y = shfl_up64(v, o);
    if (lane >= o) v += y;
  }
  return v;
}

// A wave a block, a run a lane, 64 runs a round: the block's counts, its
// verdict, and for a clean block the place of every run in it.
__global__ void __launch_bounds__(256) entries_count_kernel(Dev d) {
  const uint32_t b = blockIdx.x * kBlocksPerGroup + threadIdx.x / 64u;
  const uint32_t lane = threadIdx.x & 63u;
  if (b >= d.n) return;  // (the whole wave)
  const Head h = block_head(d, b);
  Sum total{};
  uint32_t status = h.status;
  bool clean = false;
  if (status == LVKV_ENTRIES_OK && h.nr != 0) {
    const uint8_t* p = d.raw + d.raw_off[b];
    const uint64_t s0 = d.slot_first[b], s1 = d.slot_first[b + 1u];
    if (s1 - s0 == h.nr && s1 <= d.nslots) {  // it asked for slots and they fit the scratch
      clean = true;
      uint64_t ent_carry = 0, key_carry = 0;
      for (uint32_t base = 0; base < h.nr; base += 64u) {
        const uint32_t r = base + lane;
        Sum s{};
        const bool good = r >= h.nr || parse_run(p, h, r, &s);
        if (__any(!good)) {
          clean = false;
          break;
        }
        const uint64_t ent_end = wave_inclusive(s.count, lane);
        const uint64_t key_end = wave_inclusive(s.key_bytes, lane);
        if (r < h.nr) {
          Slot slot;
          slot.key_rel = key_carry + key_end - s.key_bytes;
          slot.ent_rel = static_cast<uint32_t>(ent_carry + ent_end - s.count);
          slot.count = s.count;
          d.slots[s0 + r] = slot;
        }
        ent_carry += shfl64(ent_end, 63);
        key_carry += shfl64(key_end, 63);
        // (kept a lane; lane 0 gathers them below)
        total.val_bytes += s.val_bytes;
        total.max_key = s.max_key > total.max_key ? s.max_key : total.max_key;
        if (r == h.nr - 1u) total.last_key = s.last_key;
      }
      if (clean) {
        uint64_t vb = total.val_bytes;
        uint32_t mk = total.max_key, lk = total.last_key;
        for (uint32_t o = 32; o != 0; o >>= 1) {
          const uint32_t lo = __shfl_xor(static_cast<uint32_t>(vb), o);
          const uint32_t hi = __shfl_xor(static_cast<uint32_t>(vb >> 32), o);
          vb += (static_cast<uint64_t>(hi) << 32) | lo;
          const uint32_t ym = __shfl_xor(mk, o), yl = __shfl_xor(lk, o);
          mk = ym > mk ? ym : mk;
          lk = yl > lk ? yl : lk;  // (one lane holds it, the rest 0)
        }
        total.count = static_cast<uint32_t>(ent_carry);
        total.key_bytes = key_carry;
        total.val_bytes = vb;
        total.max_key = mk;
        total.last_key = lk;
      }
    }
    if (!clean && lane == 0) {
      total = Sum{};
      status = walk(p, h, &total);
    }
  }
  if (lane == 0) {
    d.block_first[b] = total.count;
    d.key_first[b] = total.key_bytes;
    d.val_bytes[b] = total.val_bytes;
    d.max_key[b] = total.max_key;
    d.last_key[b] = total.last_key;
    d.clean[b] = clean ? 1 : 0;
    d.block_status[b] = static_cast<uint8_t>(status);
  }
}

// The verdict, with every count known and nothing written yet. One workgroup
// folds the per-block words; thread 0 decides.
__global__ void __launch_bounds__(1024) entries_report_kernel(Dev d) {
  __shared__ uint64_t wsum[17];
  __shared__ uint32_t s_max, s_nbad, s_first, s_last;
  if (threadIdx.x == 0) {
    s_max = 0;
    s_nbad = 0;
    s_first = kNone;
    s_last = 0;
  }
  __syncthreads();
  uint64_t vb = 0;
  uint32_t mk = 0, nbad = 0, first = kNone, last = 0;
  for (uint32_t b = threadIdx.x; b < d.n; b += 1024u) {
    vb += d.val_bytes[b];
    mk = d.max_key[b] > mk ? d.max_key[b] : mk;
    const uint32_t st = d.block_status[b];
    if (st == LVKV_ENTRIES_BAD_BLOCK || st == LVKV_ENTRIES_BAD_ENTRY) {
      ++nbad;
      first = b < first ? b : first;
    }
    if (d.block_first[b + 1u] != d.block_first[b]) last = b + 1u;  // (b ascends)
  }
  if (mk != 0) atomicMax(&s_max, mk);
  if (nbad != 0) atomicAdd(&s_nbad, nbad);
  if (first != kNone) atomicMin(&s_first, first);
  if (last != 0) atomicMax(&s_last, last);
  uint64_t value_bytes;
  block_scan(vb, wsum, &value_bytes);  // (its barriers order the atomics too)
  if (threadIdx.x != 0) return;
  lvkv_sst_entries_report r;
  r.nbad = s_nbad;
  r.first_bad_block = s_first;
  r.max_key_len = s_max;
  r.num_entries = d.block_first[d.n];
  r.key_bytes = d.key_first[d.n];
  if (s_last != 0) {  // the last key is not rounded up
    const uint32_t lk = d.last_key[s_last - 1u];
    r.key_bytes -= round8(lk) - lk;
  }
  r.value_bytes = value_bytes;
  r.status = r.num_entries > d.max_entries || r.key_bytes > d.key_capacity
                 ? LVKV_ENTRIES_CAPACITY
                 : 0;
  d.ctl->status = static_cast<uint32_t>(r.status);
  *d.report = r;
}

// Byte j of the key before the entry at `upto`, j below that key's length:
// the delta that brought it, found by walking the run again from `start`.
__device__ uint8_t trace_byte(const uint8_t* p, uint32_t limit, uint32_t start, uint32_t upto,
                              uint32_t j) {
  const uint8_t* src = nullptr;
  for (uint32_t at = start; at < upto;) {
    uint32_t sh, ns, vl;
    const uint8_t* q = decode_entry(p + at, p + limit, &sh, &ns, &vl);
    if (q == nullptr) break;  // (not after the count kernel passed here)
    if (sh <= j && j - sh < ns) src = q + (j - sh);
    at = static_cast<uint32_t>(q - p) + ns + vl;
  }
  return src != nullptr ? *src : 0;
}

// `count` entries from `start` by a group of kGroup lanes: the descriptors by
// lane 0, the key bytes a word a lane. win: the group's window of the running
// key; word w is lane w % kGroup's alone.
__device__ void write_run(const Dev& d, const uint8_t* p, uint32_t limit, uint64_t block_off,
                          uint32_t start, uint32_t count, uint64_t ent, uint64_t key_at,
                          uint32_t* win, uint32_t sub) {
  const bool words = (reinterpret_cast<uintptr_t>(d.keys) & 3u) == 0;
  uint32_t at = start;
  for (uint32_t k = 0; k < count; ++k, ++ent) {
    uint32_t sh, ns, vl;
    const uint8_t* q = decode_entry(p + at, p + limit, &sh, &ns, &vl);
    if (q == nullptr) return;  // (not after the count kernel passed here)
    const uint32_t klen = sh + ns;
    if (sub == 0) {
      d.key_off[ent] = key_at;
      d.key_len[ent] = klen;
      d.val_off[ent] = block_off + static_cast<uint64_t>(q - p) + ns;
      d.val_len[ent] = vl;
    }
    uint8_t* dst = d.keys + key_at;
    const uint32_t in_window = klen < kEntriesKeyWindow ? klen : kEntriesKeyWindow;
    for (uint32_t lo = 4u * sub; lo < in_window; lo += 4u * kGroup) {
      uint32_t word = lo < sh ? win[lo / 4u] : 0u;
      if (lo + 4u > sh) {  // bytes of the delta
        const uint32_t from = lo > sh ? lo : sh;
        const uint32_t to = lo + 4u < klen ? lo + 4u : klen;
        for (uint32_t j = from; j < to; ++j) {
          const uint32_t shift = 8u * (j - lo);
          word = (word & ~(0xffu << shift)) | (uint32_t{q[j - sh]} << shift);
        }
        win[lo / 4u] = word;
      }
      if (words && lo + 4u <= klen) {
        *reinterpret_cast<uint32_t*>(dst + lo) = word;
      } else {
        for (uint32_t j = lo; j < lo + 4u && j < klen; ++j)
          dst[j] = static_cast<uint8_t>(word >> (8u * (j - lo)));
      }
    }
    // past the window: a byte a lane
    for (uint32_t j = kEntriesKeyWindow + sub; j < klen; j += kGroup)
      dst[j] = j >= sh ? q[j - sh] : trace_byte(p, limit, start, at, j);
    key_at += round8(klen);
    at = static_cast<uint32_t>(q - p) + ns + vl;
  }
}

// A wave a block, its four groups a run each in turn; a block that is not
// clean is group 0's from restart[0]. Returns at once unless the status is OK.
__global__ void __launch_bounds__(256) entries_write_kernel(Dev d) {
  __shared__ uint32_t window[(256u / kGroup) * kKeyStride];
  const uint32_t b = blockIdx.x * kBlocksPerGroup + threadIdx.x / 64u;
  if (b >= d.n || d.ctl->status != 0) return;
  const uint64_t first = d.block_first[b];
  const uint64_t count = d.block_first[b + 1u] - first;
  if (count == 0) return;  // (skipped, bad, or no entries)
  const Head h = block_head(d, b);
  if (h.status != LVKV_ENTRIES_OK || h.nr == 0) return;  // (not with a count)
  const uint32_t grp = (threadIdx.x & 63u) / kGroup, sub = threadIdx.x % kGroup;
  uint32_t* win = window + (threadIdx.x / kGroup) * kKeyStride;
  const uint64_t block_off = d.raw_off[b];
  const uint8_t* p = d.raw + block_off;
  const uint64_t key_at = d.key_first[b];
  if (d.clean[b] != 0) {
    const Slot* slots = d.slots + d.slot_first[b];
    for (uint32_t r = grp; r < h.nr; r += kGroupsPerWave) {
      const Slot s = slots[r];
      write_run(d, p, h.limit, block_off, ld_le32(p + h.limit + 4ull * r), s.count,
                first + s.ent_rel, key_at + s.key_rel, win, sub);
    }
  } else if (grp == 0) {
    write_run(d, p, h.limit, block_off, ld_le32(p + h.limit), static_cast<uint32_t>(count), first,
              key_at, win, sub);
  }
}

// The call's scratch, listed once: the control word, the per-block arrays,
// then the slots, which take what is left. Returns the bytes before the slots
// from `base` (null: sizing only).
uint64_t carve(Dev& d, uint8_t* base, uint64_t n) {
  Carver c(base);
  d.ctl = c.take<Ctl>(1, kScratchAlign);
  d.slot_first = c.take<uint64_t>(n + 1, 16);
  d.key_first = c.take<uint64_t>(n + 1, 16);
  d.val_bytes = c.take<uint64_t>(n, 16);
  d.max_key = c.take<uint32_t>(n, 16);
  d.last_key = c.take<uint32_t>(n, 16);
  d.clean = c.take<uint8_t>(n, 16);
  d.sums = c.take<uint64_t>(scan_sums_words(n), 16);
  d.slots = c.take<Slot>(0, 16);
  return c.bytes();
}

}  // namespace

size_t sst_entries_scratch_bytes(size_t nblocks, uint64_t total_raw_bytes) {
  Dev d{};
  // alignment slack, the arrays, a slot for every run the bytes can hold
  return kScratchAlign + carve(d, nullptr, nblocks) +
         sizeof(Slot) * (total_raw_bytes / kEntriesRunBytes);
}

hipError_t launch_sst_entries(const SstEntriesArgs& a, hipStream_t stream) {
  if (a.nblocks == 0) {
    hipLaunchKernelGGL(entries_empty_kernel, dim3(1), dim3(64), 0, stream, a.report);
    return hipGetLastError();
  }
  Dev d{};
  d.raw = a.raw;
  d.raw_off = a.raw_off;
  d.raw_len = a.raw_len;
  d.skip = a.skip;
  d.n = a.nblocks;
  uint8_t* base = scratch_base(a.scratch);
  const uint64_t used = static_cast<uint64_t>(base - a.scratch) + carve(d, base, a.nblocks);
  d.nslots = a.scratch_bytes > used ? (a.scratch_bytes - used) / sizeof(Slot) : 0;
  d.keys = a.keys;
  d.key_capacity = a.key_capacity;
  d.key_off = a.key_off;
  d.key_len = a.key_len;
  d.val_off = a.val_off;
  d.val_len = a.val_len;
  d.max_entries = a.max_entries;
  d.block_first = a.block_first;
  d.block_status = a.block_status;
  d.report = a.report;

  const uint32_t n = a.nblocks;
  const uint32_t per_wave = (n + kBlocksPerGroup - 1u) / kBlocksPerGroup;
  hipLaunchKernelGGL(entries_head_kernel, dim3((n + 255u) / 256u), dim3(256), 0, stream, d);
  hipError_t e = launch_exclusive_scan(d.slot_first, nullptr, d.sums, n, stream);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(entries_count_kernel, dim3(per_wave), dim3(256), 0, stream, d);
  e = launch_exclusive_scan(d.block_first, d.key_first, d.sums, n, stream);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(entries_report_kernel, dim3(1), dim3(1024), 0, stream, d);
  hipLaunchKernelGGL(entries_write_kernel, dim3(per_wave), dim3(256), 0, stream, d);
  return hipGetLastError();
}

}  // namespace lvkv
