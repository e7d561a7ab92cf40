// The memtable on the device (include/lvkv_memtable.h): RecoverLogFile's loop
// (db/db_impl.cc:453-488) over the logical records of a WAL in device memory,
// WriteBatch::Iterate (db/write_batch.cc:42-80) on each, MemTable::Add's
// internal keys (db/memtable.cc:77-101), and the memtable's iteration order.
// Sorted entry descriptors come out, in the build call's layout; no value byte
// is copied.
//
// Parse. A batch's walk is serial: each record begins where the last ended. A
// batch gets a wave (a workgroup of one), which pulls the batch through a
// window in LDS with 16-byte loads; lane 0 then follows the chain of tag,
// varint, skip at LDS latency. A step of the walk is taken only when the bytes
// it may look at (a tag and a varint, six at most) lie in the window, so a
// varint is never decoded across the window's edge: the window is loaded
// again from the step's first byte. Two walks: one counts (entries, key bytes,
// status a batch), a scan of the two sums places every batch, one workgroup
// decides whether anything is emitted (the paranoid status, KEY_TOO_LONG,
// CAPACITY), and the second walk writes each entry's descriptors to its
// log-order slot.
//
// Sort. What is sorted is (the first 8 bytes of the user key as a big-endian
// word, zero-padded; the log index), not keys: a compare leaves registers only
// when two prefixes tie, and then it is the merge call's compare (user key
// bytes, trailer descending) with the log index last, so the order is total
// even among duplicates. A workgroup sorts a tile in LDS (bitonic), then
// ceil(log2(tiles)) passes merge neighbouring runs pairwise: every entry
// bisects its partner run, and the passes go back and forth between two
// arrays. The host does not know the entry count: grids are sized by
// max_entries and every kernel looks at the count the decide kernel left.
//
// Publish. A lane a sorted position compares neighbours for DUPLICATE and a
// workgroup leaves its lowest in a slot of its own (no atomic); one workgroup
// folds the slots and gives the verdict; the key image (image_copy_kernel,
// lvkv_image_copy.h: the user key as a segment, the trailer as 8 generated
// bytes) and the publish kernel return at once unless it is OK. Every
// dependency between workgroups is a kernel boundary.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lvkv_image_copy.h"
#include "lvkv_key_compare.h"
#include "lvkv_launch.h"
#include "lvkv_memtable.h"
#include "lvkv_scratch.h"
#include "lvkv_table_format.h"

namespace lvkv {
namespace {

constexpr uint32_t kNone = 0xffffffffu;
constexpr uint32_t kWindow = kMemtableWindow;  // bytes of a batch in LDS at a time
constexpr uint32_t kDecide = 512;              // lanes of the deciding workgroup
constexpr uint64_t kKeyLimit = 0xfffffff8ull;  // a user key this long: KEY_TOO_LONG

constexpr uint64_t groups_of(uint64_t n) { return (n + kGroup - 1) / kGroup; }

// The words the kernels of one call hand to each other, at the head of the scratch.
struct MCtl {
  Ctl copy;          // go: the final verdict is OK; the key image and the publish kernel write
  uint32_t emit;     // 1: the decide kernel found nothing against emitting
  uint32_t n;        // the entries to sort (0 unless emit)
  uint64_t key_bytes;
  lvkv_memtable_report report;  // the decide kernel's; the verdict kernel finishes it
};

struct Dev {
  const uint8_t* payload;
  const uint64_t* batch_off;
  const uint64_t* batch_len;
  uint32_t nbatches, flags;
  uint64_t max_sequence_in;
  uint32_t max_entries;
  uint64_t key_capacity;
  MCtl* ctl;
  // a batch each
  uint64_t* b_ent;   // nbatches + 1: entries inserted, then their scan
  uint64_t* b_kb;    // nbatches + 1: internal key bytes, then their scan
  uint64_t* b_vb;    // value bytes
  uint64_t* b_last;  // sequence + (int)count - 1
  uint32_t* b_maxk;  // the longest internal key
  uint8_t* b_st;
  uint64_t* sums;
  // an entry each, at its log-order slot
  uint64_t* at;       // max_entries + 1: where the internal key lies in the image
  uint64_t* uk_off;   // the user key, in payload
  uint32_t* uk_len;
  uint64_t* v_off;
  uint32_t* v_len;
  uint64_t* trailer;
  // the sort's two arrays of pairs
  uint64_t* prefix[2];
  uint32_t* index[2];
  uint32_t* dup;  // a word a workgroup of the neighbour kernel
  // outputs
  uint8_t* batch_status;
  uint32_t* batch_entries;
  uint64_t* key_off;
  uint32_t* key_len;
  uint64_t* val_off;
  uint32_t* val_len;
  uint32_t* src;
  lvkv_memtable_report* report;
};

// ---- parse --------------------------------------------------------------------

// Bytes [pos, ..) of the batch at `src` into the window, as much as it holds:
// 16-byte loads at aligned addresses for the chunks that lie inside the batch,
// single bytes at its two ends. Returns the batch offset of window byte 0
// (which may lie up to 15 bytes before `pos`, and before the batch).
__device__ __forceinline__ int64_t load_window(uint8_t* win, const uint8_t* src, uint64_t len,
                                               uint64_t pos) {
  const uintptr_t bstart = reinterpret_cast<uintptr_t>(src), bend = bstart + len;
  const uintptr_t a0 = (bstart + pos) & ~uintptr_t{15};
  for (uint32_t k = threadIdx.x; k < kWindow / 16u; k += 64u) {
    const uintptr_t c = a0 + 16u * k;
    if (c >= bend) break;
    if (c >= bstart && c + 16u <= bend) {
      *reinterpret_cast<uint4*>(win + 16u * k) = *reinterpret_cast<const uint4*>(c);
    } else {
      for (uint32_t j = 0; j < 16u; ++j)
        if (c + j >= bstart && c + j < bend)
          win[16u * k + j] = *reinterpret_cast<const uint8_t*>(c + j);
    }
  }
  return static_cast<int64_t>(a0) - static_cast<int64_t>(bstart);
}

// WriteBatch::Iterate over batch b by one wave. Emit: MemTable::Add's
// descriptors to the batch's slots; otherwise the batch's counts.
template <bool Emit>
__device__ __forceinline__ void walk_batch(const Dev& d, uint32_t b) {
  __shared__ __attribute__((aligned(16))) uint8_t win[kWindow];
  __shared__ uint64_t s_pos;
  __shared__ uint32_t s_done;
  const uint64_t off = d.batch_off[b], len = d.batch_len[b];
  const uint8_t* src = d.payload + off;
  // lane 0's
  uint32_t status = LVKV_MEMTABLE_OK, found = 0, inserted = 0, phase = 0, maxk = 0;
  uint32_t klen = 0, tag = 0;
  uint64_t kb = 0, vb = 0, koff = 0, sequence = 0, last = 0;
  uint32_t count = 0;
  uint64_t slot = 0, key_at = 0;
  if (Emit) {
    slot = d.b_ent[b];
    key_at = d.b_kb[b];
  }
  if (len < 12u) {  // (the whole wave)
    status = LVKV_MEMTABLE_TOO_SMALL;
  } else {
    if (threadIdx.x == 0) {
      sequence = ld_le64(src);
      count = ld_le32(src + 8);
      last = sequence + static_cast<uint64_t>(static_cast<int64_t>(static_cast<int32_t>(count))) - 1u;
    }
    uint64_t pos = 12;
    bool done = pos >= len;
    while (!done) {  // (the whole wave: a window a turn)
      const int64_t w0 = load_window(win, src, len, pos);
      __syncthreads();
      if (threadIdx.x == 0) {
        const uint64_t wend = static_cast<uint64_t>(w0 + int64_t{kWindow}) < len
                                  ? static_cast<uint64_t>(w0 + int64_t{kWindow}) : len;
        for (;;) {
          if (phase == 0 && pos >= len) {
            done = true;
            break;
          }
          uint64_t need = phase == 0 ? 6u : 5u;
          if (need > len - pos) need = len - pos;
          if (pos + need > wend) break;  // the step's bytes: into the window first
          const uint8_t* p = win + (static_cast<int64_t>(pos) - w0);  // the batch's byte pos
          const uint8_t* lim = p + need;
          if (phase == 0) {
            ++found;
            tag = p[0];
            if (tag > 1u) {
              status = LVKV_MEMTABLE_UNKNOWN_TAG;
              done = true;
              break;
            }
            const uint32_t nb = get_varint(p + 1, lim, &klen);
            if (nb == 0 || klen > len - (pos + 1u + nb)) {
              status = tag == 1u ? LVKV_MEMTABLE_BAD_PUT : LVKV_MEMTABLE_BAD_DELETE;
              done = true;
              break;
            }
            if (klen >= kKeyLimit) {
              status = LVKV_MEMTABLE_KEY_TOO_LONG;
              done = true;
              break;
            }
            koff = pos + 1u + nb;
            pos = koff + klen;
            if (tag == 1u) {
              phase = 1;
              continue;
            }
          }
          uint32_t vlen = 0;
          uint64_t voff = pos;
          if (phase == 1) {
            const uint32_t nb = get_varint(p, lim, &vlen);
            if (nb == 0 || vlen > len - (pos + nb)) {
              status = LVKV_MEMTABLE_BAD_PUT;
              done = true;
              break;
            }
            voff = pos + nb;
            pos = voff + vlen;
            phase = 0;
          }
          // MemTable::Add
          if (Emit) {
            d.at[slot] = key_at;
            d.uk_off[slot] = off + koff;
            d.uk_len[slot] = klen;
            d.v_off[slot] = off + voff;
            d.v_len[slot] = vlen;
            d.trailer[slot] = ((sequence + inserted) << 8) | tag;
            ++slot;
            key_at += klen + 8u;
          }
          ++inserted;
          kb += klen + 8u;
          vb += vlen;
          if (klen + 8u > maxk) maxk = klen + 8u;
        }
        s_pos = pos;
        s_done = done ? 1u : 0u;
      }
      __syncthreads();
      pos = s_pos;
      done = s_done != 0;
      __syncthreads();  // (the window and the two words are written again)
    }
    if (status == LVKV_MEMTABLE_OK && found != count) status = LVKV_MEMTABLE_WRONG_COUNT;
  }
  if (Emit || threadIdx.x != 0) return;
  d.b_ent[b] = inserted;
  d.b_kb[b] = kb;
  d.b_vb[b] = vb;
  d.b_last[b] = last;
  d.b_maxk[b] = maxk;
  d.b_st[b] = static_cast<uint8_t>(status);
  if (d.batch_status != nullptr) d.batch_status[b] = static_cast<uint8_t>(status);
  if (d.batch_entries != nullptr) d.batch_entries[b] = inserted;
}

__global__ void __launch_bounds__(64) memtable_count_kernel(Dev d) { walk_batch<false>(d, blockIdx.x); }

__global__ void __launch_bounds__(64) memtable_emit_kernel(Dev d) {
  if (d.ctl->emit == 0) return;
  walk_batch<true>(d, blockIdx.x);
}

// ---- folding over a workgroup --------------------------------------------------

struct OpMin {
  __device__ __forceinline__ uint64_t operator()(uint64_t a, uint64_t b) const { return a < b ? a : b; }
};
struct OpMax {
  __device__ __forceinline__ uint64_t operator()(uint64_t a, uint64_t b) const { return a > b ? a : b; }
};
struct OpAdd {
  __device__ __forceinline__ uint64_t operator()(uint64_t a, uint64_t b) const { return a + b; }
};
constexpr OpMin op_min{};
constexpr OpMax op_max{};
constexpr OpAdd op_add{};

// Every thread of the workgroup (of Lanes) calls it and gets the fold of all their v.
template <uint32_t Lanes, typename Op>
__device__ __forceinline__ uint64_t fold64(uint64_t v, uint64_t* lds, Op op) {
  for (uint32_t o = 32; o != 0; o >>= 1) {
    const uint32_t lo = __shfl_xor(static_cast<uint32_t>(v), o);
    const uint32_t hi = __shfl_xor(static_cast<uint32_t>(v >> 32), o);
    v = op(v, (static_cast<uint64_t>(hi) << 32) | lo);
  }
  if ((threadIdx.x & 63u) == 0) lds[threadIdx.x / 64u] = v;
  __syncthreads();
  uint64_t r = lds[0];
  for (uint32_t w = 1; w < Lanes / 64u; ++w) r = op(r, lds[w]);
  __syncthreads();  // (lds may be folded into again)
  return r;
}


// One workgroup, after the scan of the batches' sums: everything the report
// holds but DUPLICATE, and whether the entries are emitted. nbatches == 0: the
// empty call's report.
__global__ void __launch_bounds__(kDecide) memtable_decide_kernel(Dev d) {
  __shared__ uint64_t lds[kDecide / 64u];
  const uint32_t nb = d.nbatches;
  uint64_t bad = kNone, too_long = kNone, n_small = 0, small_bytes = 0, n_bad = 0, vb = 0, maxk = 0;
#pragma unroll 2
  for (uint32_t b = threadIdx.x; b < nb; b += kDecide) {
    const uint32_t st = d.b_st[b];
    if (st != LVKV_MEMTABLE_OK && b < bad) bad = b;
    if (st == LVKV_MEMTABLE_KEY_TOO_LONG && b < too_long) too_long = b;
    if (st == LVKV_MEMTABLE_TOO_SMALL) {
      ++n_small;
      small_bytes += d.batch_len[b];
    } else if (st != LVKV_MEMTABLE_OK) {
      ++n_bad;
    }
    vb += d.b_vb[b];
    maxk = op_max(maxk, d.b_maxk[b]);
  }
  bad = fold64<kDecide>(bad, lds, op_min);
  too_long = fold64<kDecide>(too_long, lds, op_min);
  n_small = fold64<kDecide>(n_small, lds, op_add);
  small_bytes = fold64<kDecide>(small_bytes, lds, op_add);
  n_bad = fold64<kDecide>(n_bad, lds, op_add);
  vb = fold64<kDecide>(vb, lds, op_add);
  maxk = fold64<kDecide>(maxk, lds, op_max);
  const bool paranoid = (d.flags & LVKV_MEMTABLE_PARANOID) != 0;
  // the batches the loop got through: all of them, or those before the first bad one
  const uint32_t upto = paranoid && bad < nb ? static_cast<uint32_t>(bad) : nb;
  uint64_t seq = d.max_sequence_in;
#pragma unroll 2
  for (uint32_t b = threadIdx.x; b < upto; b += kDecide)
    if (d.batch_len[b] >= 12u) seq = op_max(seq, d.b_last[b]);
  seq = fold64<kDecide>(seq, lds, op_max);
  if (threadIdx.x != 0) return;
  // (field by field into memory: a report built in registers first is an object on the stack)
  lvkv_memtable_report* r = d.ctl != nullptr ? &d.ctl->report : d.report;
  int32_t status = LVKV_MEMTABLE_OK;
  uint32_t first_bad_batch = kNone;
  uint64_t n = 0, kb = 0;
  if (nb != 0) {
    n = d.b_ent[nb];
    kb = d.b_kb[nb];
    if (paranoid && bad < nb) {
      status = d.b_st[bad];
      first_bad_batch = static_cast<uint32_t>(bad);
    } else if (too_long < nb) {
      status = LVKV_MEMTABLE_KEY_TOO_LONG;
      first_bad_batch = static_cast<uint32_t>(too_long);
    } else if (n > d.max_entries || kb > d.key_capacity) {
      status = LVKV_MEMTABLE_CAPACITY;
    }
  }
  r->status = status;
  r->first_bad_batch = first_bad_batch;
  r->first_bad_entry = kNone;
  r->nentries = static_cast<uint32_t>(n < kNone ? n : kNone);
  r->key_bytes = kb;
  r->val_bytes = vb;
  r->max_key_len = static_cast<uint32_t>(maxk);
  r->n_too_small = static_cast<uint32_t>(n_small);
  r->too_small_bytes = small_bytes;
  r->max_sequence_out = seq;
  r->n_bad_batches = static_cast<uint32_t>(n_bad);
  r->reserved_ = 0;
  if (d.ctl == nullptr) return;  // (the empty call)
  const uint32_t emit = status == LVKV_MEMTABLE_OK ? 1u : 0u;
  d.ctl->copy.go = 0;
  d.ctl->emit = emit;
  d.ctl->n = emit != 0 ? static_cast<uint32_t>(n) : 0u;
  d.ctl->key_bytes = kb;
}

// ---- sort ---------------------------------------------------------------------

struct Pair {
  uint64_t prefix;
  uint32_t index;
};

// a before b, for two pairs whose prefixes tie: the user keys' bytes, the
// trailer descending, the log index.
__device__ __forceinline__ bool tie_less(const Dev& d, uint32_t a, uint32_t b) {
  const uint32_t la = d.uk_len[a], lb = d.uk_len[b];
  if (la > 8u || lb > 8u || la != lb) {  // (8 bytes and under: the prefix and the length say it)
    const int c = compare_bytes(d.payload + d.uk_off[a], la, d.payload + d.uk_off[b], lb);
    if (c != 0) return c < 0;
  }
  const uint64_t ta = d.trailer[a], tb = d.trailer[b];
  if (ta != tb) return ta > tb;
  return a < b;
}

// (kNone: the padding of a tile, after everything)
__device__ __forceinline__ bool pair_less(const Dev& d, const Pair& a, const Pair& b) {
  if (a.prefix != b.prefix) return a.prefix < b.prefix;
  if (a.index == kNone || b.index == kNone) return a.index != kNone && b.index == kNone;
  return tie_less(d, a.index, b.index);
}

// The first 8 bytes of entry e's user key as a big-endian word, zero-padded.
__device__ __forceinline__ uint64_t prefix_of(const Dev& d, uint32_t e) {
  const uint8_t* p = d.payload + d.uk_off[e];
  const uint32_t l = d.uk_len[e];
  uint64_t v = 0;
  for (uint32_t k = 0; k < 8u; ++k) v = (v << 8) | (k < l ? p[k] : 0u);
  return v;
}

// A workgroup a tile of T entries: their pairs, sorted in LDS (bitonic), to
// array 0.
template <uint32_t T>
__global__ void __launch_bounds__(kGroup) memtable_tile_sort_kernel(Dev d) {
  __shared__ uint64_t s_prefix[T];
  __shared__ uint32_t s_index[T];
  const uint32_t n = d.ctl->n;
  const uint32_t base = blockIdx.x * T;
  if (base >= n) return;  // (the whole workgroup)
  for (uint32_t t = threadIdx.x; t < T; t += kGroup) {
    const uint32_t e = base + t;
    s_prefix[t] = e < n ? prefix_of(d, e) : ~uint64_t{0};
    s_index[t] = e < n ? e : kNone;
  }
  __syncthreads();
  for (uint32_t k = 2; k <= T; k <<= 1) {
    for (uint32_t j = k >> 1; j != 0; j >>= 1) {
      for (uint32_t p = threadIdx.x; p < T / 2u; p += kGroup) {
        const uint32_t i = ((p & ~(j - 1u)) << 1) | (p & (j - 1u)), l = i | j;
        const Pair a{s_prefix[i], s_index[i]}, b{s_prefix[l], s_index[l]};
        const bool up = (i & k) == 0;
        if (up ? pair_less(d, b, a) : pair_less(d, a, b)) {
          s_prefix[i] = b.prefix;
          s_index[i] = b.index;
          s_prefix[l] = a.prefix;
          s_index[l] = a.index;
        }
      }
      __syncthreads();
    }
  }
  for (uint32_t t = threadIdx.x; t < T && base + t < n; t += kGroup) {
    d.prefix[0][base + t] = s_prefix[t];
    d.index[0][base + t] = s_index[t];
  }
}

// A lane an entry: runs of `run` entries merge pairwise from array `from` to
// the other. The entry's place is its index in its own run and the partner's
// entries before it, found by bisection (no two pairs compare equal).
__global__ void __launch_bounds__(kGroup) memtable_merge_pass_kernel(Dev d, uint32_t run, uint32_t from) {
  const uint32_t n = d.ctl->n;
  const uint32_t i = blockIdx.x * kGroup + threadIdx.x;
  if (i >= n) return;
  const uint64_t* prefix = d.prefix[from];
  const uint32_t* index = d.index[from];
  const Pair me{prefix[i], index[i]};
  const uint32_t own = i / run * run;
  const bool right = (i / run & 1u) != 0;
  // (own + run < 2^32: n < 2^31 and run <= the first power of two not below n)
  uint32_t lo = right ? own - run : own + run;
  const uint32_t first = right ? lo : own;
  uint32_t before = 0;
  if (lo < n) {
    uint32_t hi = lo + run < n ? lo + run : n;
    const uint32_t p0 = lo;
    while (lo < hi) {  // pairs below lo come before me, pairs from hi on do not
      const uint32_t mid = lo + (hi - lo) / 2u;
      const Pair o{prefix[mid], index[mid]};
      if (pair_less(d, o, me)) lo = mid + 1u;
      else hi = mid;
    }
    before = lo - p0;
  }
  const uint32_t to = first + (i - own) + before;
  d.prefix[from ^ 1u][to] = me.prefix;
  d.index[from ^ 1u][to] = me.index;
}

// ---- publish ------------------------------------------------------------------

// A lane a sorted position: is its internal key the one before it? A
// workgroup leaves the lowest log index of such an entry (equal keys lie in
// log order: it has an earlier equal), kNone for none.
__global__ void __launch_bounds__(kGroup) memtable_neighbour_kernel(Dev d, uint32_t from) {
  __shared__ uint64_t lds[kGroup / 64u];
  const uint32_t n = d.ctl->n;
  if (blockIdx.x * kGroup >= n) return;  // (the whole workgroup)
  const uint32_t i = blockIdx.x * kGroup + threadIdx.x;
  uint64_t dup = kNone;
  if (i != 0 && i < n && d.prefix[from][i] == d.prefix[from][i - 1u]) {
    const uint32_t a = d.index[from][i - 1u], b = d.index[from][i];
    const uint32_t l = d.uk_len[a];
    if (l == d.uk_len[b] && d.trailer[a] == d.trailer[b] &&
        common_prefix(d.payload + d.uk_off[a], d.payload + d.uk_off[b], l) == l)
      dup = b;
  }
  dup = fold64<kGroup>(dup, lds, op_min);
  if (threadIdx.x == 0) d.dup[blockIdx.x] = static_cast<uint32_t>(dup);
}

// One workgroup: the verdict and the report.
__global__ void __launch_bounds__(kGroup) memtable_verdict_kernel(Dev d) {
  __shared__ uint64_t lds[kGroup / 64u];
  const uint32_t groups = static_cast<uint32_t>(groups_of(d.ctl->n));
  uint64_t dup = kNone;
  for (uint32_t g = threadIdx.x; g < groups; g += kGroup) dup = op_min(dup, d.dup[g]);
  dup = fold64<kGroup>(dup, lds, op_min);
  if (threadIdx.x != 0) return;
  lvkv_memtable_report r = d.ctl->report;
  if (r.status == LVKV_MEMTABLE_OK && dup != kNone) {
    r.status = LVKV_MEMTABLE_DUPLICATE;
    r.first_bad_entry = static_cast<uint32_t>(dup);
  }
  *d.report = r;
  d.ctl->copy.go = r.status == LVKV_MEMTABLE_OK ? 1u : 0u;
}

// The image's offsets past the last entry: records without bytes, which the
// copy passes over (the host sizes the image by max_entries).
__global__ void __launch_bounds__(kGroup) memtable_pad_kernel(Dev d) {
  const uint64_t j = uint64_t{blockIdx.x} * kGroup + threadIdx.x;
  if (d.ctl->emit == 0 || j < d.ctl->n || j > d.max_entries) return;
  d.at[j] = d.ctl->key_bytes;
}

// The internal keys in log order: the user key, then the trailer's 8 bytes.
struct KeyImage {
  const uint64_t* at;  // n + 1
  uint32_t n;
  const uint8_t* payload;
  const uint64_t* uk_off;
  const uint32_t* uk_len;
  const uint64_t* trailer;

  __device__ __forceinline__ Rec rec(uint32_t r) const {
    Rec x{};
    if (at[r + 1] == at[r]) return x;
    x.sa = payload + uk_off[r];
    x.la = uk_len[r];
    x.hb = 8u;
    return x;
  }
  __device__ __forceinline__ uint8_t gen(uint32_t r, const Rec&, uint32_t k) const {
    return static_cast<uint8_t>(trailer[r] >> (8u * k));
  }
};

__global__ void __launch_bounds__(kGroup) memtable_publish_kernel(Dev d, uint32_t from) {
  const uint32_t i = blockIdx.x * kGroup + threadIdx.x;
  if (d.ctl->copy.go == 0 || i >= d.ctl->n) return;
  const uint32_t e = d.index[from][i];
  d.key_off[i] = d.at[e];
  d.key_len[i] = d.uk_len[e] + 8u;
  d.val_off[i] = d.v_off[e];
  d.val_len[i] = d.v_len[e];
  d.src[i] = e;
}

// The call's scratch, listed once. Returns the bytes from `base` (null: sizing only).
uint64_t carve(Dev& d, uint8_t* base, uint64_t nb, uint64_t me) {
  Carver c(base);
  d.ctl = c.take<MCtl>(1, kScratchAlign);
  d.b_ent = c.take<uint64_t>(nb + 1, 16);
  d.b_kb = c.take<uint64_t>(nb + 1, 16);
  d.b_vb = c.take<uint64_t>(nb, 16);
  d.b_last = c.take<uint64_t>(nb, 16);
  d.b_maxk = c.take<uint32_t>(nb, 16);
  d.b_st = c.take<uint8_t>(nb, 16);
  d.sums = c.take<uint64_t>(scan_sums_words(nb), 16);
  d.at = c.take<uint64_t>(me + 1, 16);
  d.uk_off = c.take<uint64_t>(me, 16);
  d.uk_len = c.take<uint32_t>(me, 16);
  d.v_off = c.take<uint64_t>(me, 16);
  d.v_len = c.take<uint32_t>(me, 16);
  d.trailer = c.take<uint64_t>(me, 16);
  for (int k = 0; k < 2; ++k) {
    d.prefix[k] = c.take<uint64_t>(me, 16);
    d.index[k] = c.take<uint32_t>(me, 16);
  }
  d.dup = c.take<uint32_t>(groups_of(me), 16);
  return c.bytes();
}

// lvkv_debug_set_memtable_tile: the sort tile of the next calls, 0 for kMemtableTile.
uint32_t g_tile = 0;

}  // namespace

bool memtable_set_tile(int pairs) {
  if (pairs != 0 && pairs != 512 && pairs != 1024 && pairs != 2048) return false;
  g_tile = static_cast<uint32_t>(pairs);
  return true;
}

size_t memtable_scratch_bytes(size_t nbatches, size_t max_entries) {
  Dev d{};
  return kScratchAlign + carve(d, nullptr, nbatches, max_entries);  // alignment slack
}

hipError_t launch_memtable(const MemtableArgs& a, hipStream_t stream) {
  Dev d{};
  d.report = a.report;
  d.max_sequence_in = a.max_sequence_in;
  if (a.nbatches == 0) {
    hipLaunchKernelGGL(memtable_decide_kernel, dim3(1), dim3(kDecide), 0, stream, d);
    return hipGetLastError();
  }
  d.payload = a.payload;
  d.batch_off = a.batch_off;
  d.batch_len = a.batch_len;
  d.nbatches = a.nbatches;
  d.flags = a.flags;
  d.max_entries = a.max_entries;
  d.key_capacity = a.key_capacity;
  carve(d, scratch_base(a.scratch), a.nbatches, a.max_entries);
  d.batch_status = a.batch_status;
  d.batch_entries = a.batch_entries;
  d.key_off = a.key_off;
  d.key_len = a.key_len;
  d.val_off = a.val_off;
  d.val_len = a.val_len;
  d.src = a.src;

  const uint32_t tile = g_tile != 0 ? g_tile : kMemtableTile;
  const uint32_t slots = a.max_entries != 0 ? a.max_entries : 1u;  // (a grid has a workgroup)
  const uint32_t per_entry = static_cast<uint32_t>(groups_of(slots));
  const uint32_t tiles = (slots + tile - 1u) / tile;
  hipLaunchKernelGGL(memtable_count_kernel, dim3(d.nbatches), dim3(64), 0, stream, d);
  const hipError_t e = launch_exclusive_scan(d.b_ent, d.b_kb, d.sums, d.nbatches, stream);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(memtable_decide_kernel, dim3(1), dim3(kDecide), 0, stream, d);
  hipLaunchKernelGGL(memtable_emit_kernel, dim3(d.nbatches), dim3(64), 0, stream, d);
  hipLaunchKernelGGL(memtable_pad_kernel, dim3(static_cast<uint32_t>(groups_of(uint64_t{slots} + 1))),
                     dim3(kGroup), 0, stream, d);
  switch (tile) {
    case 512:
      hipLaunchKernelGGL(memtable_tile_sort_kernel<512>, dim3(tiles), dim3(kGroup), 0, stream, d);
      break;
    case 2048:
      hipLaunchKernelGGL(memtable_tile_sort_kernel<2048>, dim3(tiles), dim3(kGroup), 0, stream, d);
      break;
    default:
      hipLaunchKernelGGL(memtable_tile_sort_kernel<1024>, dim3(tiles), dim3(kGroup), 0, stream, d);
      break;
  }
  uint32_t from = 0;
  for (uint64_t run = tile; run < slots; run *= 2u, from ^= 1u)
    hipLaunchKernelGGL(memtable_merge_pass_kernel, dim3(per_entry), dim3(kGroup), 0, stream, d,
                       static_cast<uint32_t>(run), from);
  hipLaunchKernelGGL(memtable_neighbour_kernel, dim3(per_entry), dim3(kGroup), 0, stream, d, from);
  hipLaunchKernelGGL(memtable_verdict_kernel, dim3(1), dim3(kGroup), 0, stream, d);
  KeyImage ki{d.at, a.max_entries, d.payload, d.uk_off, d.uk_len, d.trailer};
  launch_image_copy_rows<KeyImage, kCopyRows>(ki, a.keys, a.key_capacity, &d.ctl->copy, stream);
  hipLaunchKernelGGL(memtable_publish_kernel, dim3(per_entry), dim3(kGroup), 0, stream, d, from);
  return hipGetLastError();
}

}  // namespace lvkv
