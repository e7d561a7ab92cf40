// MergingIterator's forward walk over sorted runs of entries on the device
// (table/merger.cc:150-163), and the drops DoCompactionWork applies to what it
// hands out (db/db_impl.cc:1022-1055): what stands between
// lvkv_sst_read_entries_device and lvkv_sst_build_blocks_device in a
// compaction. Runs laid end to end go in; descriptors of the surviving
// entries, in merged order, come out. No key or value byte is copied.
//
// There is no serial walk. An entry's place in the merged order is its index
// in its own run plus, for every other run, the number of that run's entries
// that come before it: the entries not greater in a run of lower index, the
// entries smaller in a run of higher index -- FindSmallest keeps the earlier
// child among equals. That is a bisection per other run, and the other runs
// are shared out among up to kRankLanes lanes an entry (the smallest power of
// two that gives every lane one bisection, where kRankLanes allows). Whether
// an entry is dropped depends on it and on the entry directly before it in
// merged order alone (the loop's state is the previous key's user key and
// sequence, reset by a key that does not parse), so the flags are a lane a
// merged position.
//
// merge_runs_kernel checks the run boundaries, merge_check_kernel the keys
// and the order inside each run; merge_rank_kernel and merge_drop_kernel
// return at once when either found fault (a bisection over unsorted keys
// leaves places unfilled). A scan of the keep flags numbers the survivors,
// merge_report_kernel decides the status with every count known and nothing
// written yet, and merge_write_kernel gathers only when that status is OK.
// Every dependency between workgroups is a kernel boundary. What every
// workgroup has to say -- its longest key, the drop kernel's counts -- it
// folds in LDS and leaves in a slot of its own, which the report kernel adds
// up: no atomic. Only a workgroup that found a fault issues one, an
// atomicMin on the lowest offending entry.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lvkv_key_compare.h"
#include "lvkv_launch.h"
#include "lvkv_scratch.h"
#include "lvkv_snappy.h"
#include "lvkv_table_format.h"

namespace lvkv {
namespace {

constexpr uint32_t kNone = 0xffffffffu;
constexpr uint32_t kGroup = 256;     // lanes a workgroup, every kernel but the two of one
constexpr uint32_t kWaves = kGroup / 64;
constexpr uint32_t kRankLanes = 8;   // lanes an entry in the rank kernel, at most
constexpr uint64_t kMaxSequence = (uint64_t{1} << 56) - 1;  // kMaxSequenceNumber
static_assert(64 % kRankLanes == 0 && (kRankLanes & (kRankLanes - 1)) == 0,
              "an entry's lanes lie in one wave and fold by shuffles");

// The words the kernels of one call hand to each other, at the head of the scratch.
struct Ctl {
  uint32_t bad_runs;   // 1: d_run_first is not 0 .. nentries, non-decreasing
  uint32_t bad_key;    // lowest entry with a key under 8 bytes (key_format 1), kNone
  uint32_t unsorted;   // lowest entry not greater than its predecessor in its run, kNone
  uint32_t status;     // LVKV_MERGE_*, by merge_report_kernel
};
static_assert(sizeof(Ctl) <= kScratchAlign, "the control words' room");

// What a workgroup of the drop kernel counted; the report kernel adds them up.
struct Part {
  uint32_t hidden, obsolete;
  uint64_t key_bytes, value_bytes;  // the survivors'
};
static_assert(sizeof(Part) == 24, "the sizing function counts 24 bytes a workgroup");

struct Dev {
  const uint8_t* keys;
  const uint64_t* key_off;
  const uint32_t* key_len;
  const uint64_t* val_off;
  const uint32_t* val_len;
  const uint64_t* run_first;  // nruns + 1
  uint32_t n, nruns, key_format, compact;
  uint32_t rank_lanes;  // lanes an entry in the rank kernel: a power of two up to kRankLanes
  uint64_t snapshot;
  const uint8_t* deeper_keys;
  const uint64_t* deeper_off;  // range g: smallest at 2g, largest at 2g + 1
  const uint32_t* deeper_len;
  uint32_t n_deeper;
  Ctl* ctl;
  uint32_t* order;  // n: the input index of the entry at each merged position
  uint64_t* keep;   // n + 1: 1 for a survivor, then its scan: the survivor's slot
  Part* parts;      // a workgroup of the drop kernel each
  uint32_t* max_key;  // a workgroup of the check kernel each: its longest key
  uint64_t* sums;
  uint64_t* out_key_off;
  uint32_t* out_key_len;
  uint64_t* out_val_off;
  uint32_t* out_val_len;
  uint32_t* out_src;
  uint64_t max_out;
  uint32_t* dropped_src;  // may be null
  lvkv_sst_merge_report* report;
};

// ---- comparing keys ----------------------------------------------------------

struct Key {
  const uint8_t* p;
  uint32_t len;
};

__device__ __forceinline__ Key key_of(const Dev& d, uint32_t e) {
  return Key{d.keys + d.key_off[e], d.key_len[e]};
}

// The call's comparator. key_format 1: InternalKeyComparator
// (db/dbformat.cc:47-63) -- user keys ascending, then the trailing 8 bytes as
// a little-endian u64 descending; both keys 8 bytes or longer.
__device__ __forceinline__ int compare_keys(uint32_t key_format, const Key& a, const Key& b) {
  if (key_format == 0) return compare_bytes(a.p, a.len, b.p, b.len);
  const int c = compare_bytes(a.p, a.len - 8u, b.p, b.len - 8u);
  if (c != 0) return c;
  const uint64_t ta = ld_le64(a.p + a.len - 8u), tb = ld_le64(b.p + b.len - 8u);
  return ta > tb ? -1 : ta < tb ? 1 : 0;
}

// ---- folding over a workgroup: shuffles in the wave, LDS between the waves ----

__device__ __forceinline__ uint32_t umin(uint32_t a, uint32_t b) { return a < b ? a : b; }
__device__ __forceinline__ uint32_t umax(uint32_t a, uint32_t b) { return a > b ? a : b; }
__device__ __forceinline__ uint32_t uadd(uint32_t a, uint32_t b) { return a + b; }

// Every thread of the workgroup calls it; the result is thread 0's alone.
template <typename Op>
__device__ __forceinline__ uint32_t group_fold(uint32_t v, uint32_t* lds, Op op) {
  for (uint32_t o = 32; o != 0; o >>= 1) v = op(v, __shfl_xor(v, o));
  if ((threadIdx.x & 63u) == 0) lds[threadIdx.x / 64u] = v;
  __syncthreads();
  uint32_t r = lds[0];
  for (uint32_t w = 1; w < kWaves; ++w) r = op(r, lds[w]);
  __syncthreads();  // (lds may be folded into again)
  return r;
}

__device__ __forceinline__ uint64_t group_sum64(uint64_t v, uint64_t* lds) {
  for (uint32_t o = 32; o != 0; o >>= 1) {
    const uint32_t lo = __shfl_xor(static_cast<uint32_t>(v), o);
    const uint32_t hi = __shfl_xor(static_cast<uint32_t>(v >> 32), o);
    v += (static_cast<uint64_t>(hi) << 32) | lo;
  }
  if ((threadIdx.x & 63u) == 0) lds[threadIdx.x / 64u] = v;
  __syncthreads();
  uint64_t r = lds[0];
  for (uint32_t w = 1; w < kWaves; ++w) r += lds[w];
  __syncthreads();
  return r;
}

// ---- the kernels --------------------------------------------------------------

// A report of no entries (nentries == 0).
__global__ void merge_empty_kernel(lvkv_sst_merge_report* r) {
  if (threadIdx.x != 0) return;
  lvkv_sst_merge_report e{};
  e.status = LVKV_MERGE_OK;
  e.first_bad_entry = kNone;
  *r = e;
}

// The control words, and the run boundaries: 0 first, nentries last, never
// descending. One wave; nruns + 1 <= 65 words.
__global__ void merge_runs_kernel(Dev d) {
  bool bad = false;
  for (uint32_t r = threadIdx.x; r <= d.nruns; r += 64u) {
    const uint64_t at = d.run_first[r];
    if (r == 0 && at != 0) bad = true;
    if (r == d.nruns ? at != d.n : at > d.run_first[r + 1u]) bad = true;
  }
  bad = __any(bad);
  if (threadIdx.x != 0) return;
  Ctl c{};
  c.bad_runs = bad ? 1u : 0u;
  c.bad_key = kNone;
  c.unsorted = kNone;
  c.status = LVKV_MERGE_OK;
  *d.ctl = c;
}

// The run entry e lies in: the last one that begins at or before it (empty
// runs before it begin there too and are passed over).
__device__ __forceinline__ uint32_t run_of(const uint64_t* run_first, uint32_t nruns, uint32_t e) {
  uint32_t lo = 0, hi = nruns;  // run_first[lo] <= e < run_first[hi]
  while (hi - lo > 1u) {
    const uint32_t mid = lo + (hi - lo) / 2u;
    if (run_first[mid] <= e) lo = mid;
    else hi = mid;
  }
  return lo;
}

// Per entry: the key's length, and the order against the entry before it in
// the same run.
__global__ void __launch_bounds__(kGroup) merge_check_kernel(Dev d) {
  __shared__ uint32_t fold[kWaves];
  __shared__ uint64_t first[LVKV_MERGE_MAX_RUNS + 1];
  if (d.ctl->bad_runs != 0) return;  // (the whole grid)
  for (uint32_t r = threadIdx.x; r <= d.nruns; r += kGroup) first[r] = d.run_first[r];
  __syncthreads();
  const uint32_t i = blockIdx.x * kGroup + threadIdx.x;
  uint32_t klen = 0, bad_key = kNone, unsorted = kNone;
  if (i < d.n) {
    klen = d.key_len[i];
    if (d.key_format == 1 && klen < 8u) bad_key = i;
    if (first[run_of(first, d.nruns, i)] != i) {
      const Key k = key_of(d, i), p = key_of(d, i - 1u);
      // (a key under 8 bytes is BAD_KEY, which comes first: no verdict here)
      if ((d.key_format == 0 || (k.len >= 8u && p.len >= 8u)) &&
          compare_keys(d.key_format, p, k) >= 0)
        unsorted = i;
    }
  }
  bad_key = group_fold(bad_key, fold, umin);
  unsorted = group_fold(unsorted, fold, umin);
  klen = group_fold(klen, fold, umax);
  if (threadIdx.x != 0) return;
  if (bad_key != kNone) atomicMin(&d.ctl->bad_key, bad_key);
  if (unsorted != kNone) atomicMin(&d.ctl->unsorted, unsorted);
  d.max_key[blockIdx.x] = klen;
}

__device__ __forceinline__ bool sound(const Ctl* c) {
  return c->bad_runs == 0 && c->bad_key == kNone && c->unsorted == kNone;
}

// rank_lanes lanes an entry: lane `sub` bisects the other runs number sub, sub
// + rank_lanes, .. (the entry's own run left out of the count); their counts
// and the entry's index in its run add up to its merged position.
__global__ void __launch_bounds__(kGroup) merge_rank_kernel(Dev d) {
  __shared__ uint64_t first[LVKV_MERGE_MAX_RUNS + 1];
  if (!sound(d.ctl)) return;  // (the whole grid)
  for (uint32_t r = threadIdx.x; r <= d.nruns; r += kGroup) first[r] = d.run_first[r];
  __syncthreads();
  const uint64_t gid = uint64_t{blockIdx.x} * kGroup + threadIdx.x;
  const uint32_t lanes = d.rank_lanes;
  const uint32_t sub = static_cast<uint32_t>(gid & (lanes - 1u));
  const bool live = gid / lanes < d.n;
  const uint32_t e = live ? static_cast<uint32_t>(gid / lanes) : 0u;
  uint32_t before = 0;
  if (live) {
    const uint32_t own = run_of(first, d.nruns, e);
    const Key k = key_of(d, e);
    if (sub == 0) before = e - static_cast<uint32_t>(first[own]);
    for (uint32_t j = sub; j + 1u < d.nruns; j += lanes) {
      const uint32_t q = j < own ? j : j + 1u;
      uint32_t lo = static_cast<uint32_t>(first[q]), hi = static_cast<uint32_t>(first[q + 1u]);
      const uint32_t base = lo;
      while (lo < hi) {  // entries below lo come before e, entries from hi on do not
        const uint32_t mid = lo + (hi - lo) / 2u;
        const int c = compare_keys(d.key_format, key_of(d, mid), k);
        if (c < 0 || (c == 0 && q < own)) lo = mid + 1u;
        else hi = mid;
      }
      before += lo - base;
    }
  }
  for (uint32_t o = 1; o < lanes; o <<= 1) before += __shfl_xor(before, o);
  // (a permutation when every run ascends strictly, which the check saw to)
  if (live && sub == 0 && before < d.n) d.order[before] = e;
}

// IsBaseLevelForKey (db/version_set.cc:1518-1537): in none of the ranges,
// bounds included.
__device__ bool base_level(const Dev& d, const uint8_t* user, uint32_t ulen) {
  for (uint32_t g = 0; g < d.n_deeper; ++g) {
    const uint8_t* lo = d.deeper_keys + d.deeper_off[2u * g];
    const uint8_t* hi = d.deeper_keys + d.deeper_off[2u * g + 1u];
    if (compare_bytes(user, ulen, hi, d.deeper_len[2u * g + 1u]) <= 0 &&
        compare_bytes(user, ulen, lo, d.deeper_len[2u * g]) >= 0)
      return false;
  }
  return true;
}

// A lane a merged position: the loop of db/db_impl.cc:1022-1055 from the
// entry and the one before it. keep = 1, or 0 for a hidden entry or an
// obsolete deletion.
__global__ void __launch_bounds__(kGroup) merge_drop_kernel(Dev d) {
  __shared__ uint32_t fold[kWaves];
  __shared__ uint64_t fold64[kWaves];
  if (!sound(d.ctl)) return;  // (the whole grid)
  const uint32_t i = blockIdx.x * kGroup + threadIdx.x;
  uint32_t hidden = 0, obsolete = 0;
  uint64_t kb = 0, vb = 0;
  if (i < d.n) {
    const uint32_t e = d.order[i];
    const Key k = key_of(d, e);
    if (d.compact != 0) {
      const uint64_t tag = ld_le64(k.p + k.len - 8u);
      if ((tag & 0xffu) <= 1u) {  // ParseInternalKey (db/dbformat.h:173-183)
        // last_sequence_for_key: the predecessor's where it parses and has
        // this user key, else kMaxSequenceNumber
        uint64_t last = kMaxSequence;
        if (i != 0) {
          const Key p = key_of(d, d.order[i - 1u]);
          const uint64_t ptag = ld_le64(p.p + p.len - 8u);
          if ((ptag & 0xffu) <= 1u && p.len == k.len &&
              common_prefix(p.p, k.p, k.len - 8u) == k.len - 8u)
            last = ptag >> 8;
        }
        if (last <= d.snapshot) hidden = 1;
        else if ((tag & 0xffu) == 0 && (tag >> 8) <= d.snapshot && base_level(d, k.p, k.len - 8u))
          obsolete = 1;
      }
    }
    const uint32_t keep = 1u - hidden - obsolete;
    d.keep[i] = keep;
    if (keep != 0) {
      kb = k.len;
      vb = d.val_len[e];
    }
  }
  hidden = group_fold(hidden, fold, uadd);
  obsolete = group_fold(obsolete, fold, uadd);
  kb = group_sum64(kb, fold64);
  vb = group_sum64(vb, fold64);
  if (threadIdx.x == 0) d.parts[blockIdx.x] = Part{hidden, obsolete, kb, vb};
}

// The verdict, with the order and the counts known and nothing written yet.
// One workgroup adds up the drop kernel's slots; thread 0 decides.
__global__ void __launch_bounds__(kGroup) merge_report_kernel(Dev d) {
  __shared__ uint32_t fold[kWaves];
  __shared__ uint64_t fold64[kWaves];
  Ctl* c = d.ctl;
  uint32_t hidden = 0, obsolete = 0, max_key_len = 0;
  uint64_t kb = 0, vb = 0;
  const uint32_t groups = (d.n + kGroup - 1u) / kGroup;
  if (c->bad_runs == 0) {  // (the whole workgroup; the check kernel ran)
    for (uint32_t g = threadIdx.x; g < groups; g += kGroup)
      max_key_len = umax(max_key_len, d.max_key[g]);
    max_key_len = group_fold(max_key_len, fold, umax);
  }
  if (sound(c)) {  // (the whole workgroup; the drop kernel ran)
    for (uint32_t g = threadIdx.x; g < groups; g += kGroup) {
      const Part part = d.parts[g];
      hidden += part.hidden;
      obsolete += part.obsolete;
      kb += part.key_bytes;
      vb += part.value_bytes;
    }
    hidden = group_fold(hidden, fold, uadd);
    obsolete = group_fold(obsolete, fold, uadd);
    kb = group_sum64(kb, fold64);
    vb = group_sum64(vb, fold64);
  }
  if (threadIdx.x != 0) return;
  lvkv_sst_merge_report r{};
  r.status = LVKV_MERGE_OK;
  r.first_bad_entry = kNone;
  r.num_in = d.n;
  if (c->bad_runs != 0) {
    r.status = LVKV_MERGE_BAD_RUNS;  // (no entry was looked at)
  } else if (c->bad_key != kNone || c->unsorted != kNone) {
    r.status = c->bad_key != kNone ? LVKV_MERGE_BAD_KEY : LVKV_MERGE_UNSORTED;
    r.first_bad_entry = c->bad_key != kNone ? c->bad_key : c->unsorted;
    r.max_key_len = max_key_len;
  } else {
    r.max_key_len = max_key_len;
    r.num_out = static_cast<uint32_t>(d.keep[d.n]);
    r.num_hidden = hidden;
    r.num_obsolete = obsolete;
    r.key_bytes = kb;
    r.value_bytes = vb;
    if (r.num_out > d.max_out) r.status = LVKV_MERGE_CAPACITY;
  }
  c->status = static_cast<uint32_t>(r.status);
  *d.report = r;
}

// A lane a merged position: a survivor's descriptors to its slot, a dropped
// entry's index to its own. Returns at once unless the status is OK.
__global__ void __launch_bounds__(kGroup) merge_write_kernel(Dev d) {
  const uint32_t i = blockIdx.x * kGroup + threadIdx.x;
  if (i >= d.n || d.ctl->status != LVKV_MERGE_OK) return;
  const uint32_t e = d.order[i];
  const uint64_t at = d.keep[i];
  if (d.keep[i + 1u] != at) {  // (at < num_out <= max_out)
    d.out_key_off[at] = d.key_off[e];
    d.out_key_len[at] = d.key_len[e];
    d.out_val_off[at] = d.val_off[e];
    d.out_val_len[at] = d.val_len[e];
    d.out_src[at] = e;
  } else if (d.dropped_src != nullptr) {
    d.dropped_src[i - at] = e;
  }
}

// The call's scratch, listed once: the control words, then the arrays, each
// rounded up to 16 bytes. Returns the bytes from `base` (null: sizing only).
uint64_t carve(Dev& d, uint8_t* base, uint64_t n) {
  Carver c(base);
  d.ctl = c.take<Ctl>(1, kScratchAlign);
  d.keep = c.take<uint64_t>(n + 1, 16);
  d.order = c.take<uint32_t>(n, 16);
  d.parts = c.take<Part>((n + kGroup - 1) / kGroup, 16);
  d.max_key = c.take<uint32_t>((n + kGroup - 1) / kGroup, 16);
  d.sums = c.take<uint64_t>(scan_sums_words(n), 16);
  return c.bytes();
}

}  // namespace

size_t sst_merge_scratch_bytes(size_t nentries) {
  Dev d{};
  return kScratchAlign + carve(d, nullptr, nentries);  // alignment slack
}

hipError_t launch_sst_merge(const SstMergeArgs& a, hipStream_t stream) {
  if (a.n == 0) {
    hipLaunchKernelGGL(merge_empty_kernel, dim3(1), dim3(64), 0, stream, a.report);
    return hipGetLastError();
  }
  Dev d{};
  d.keys = a.keys;
  d.key_off = a.key_off;
  d.key_len = a.key_len;
  d.val_off = a.val_off;
  d.val_len = a.val_len;
  d.run_first = a.run_first;
  d.n = a.n;
  d.nruns = a.nruns;
  d.key_format = a.key_format;
  d.compact = a.compact;
  d.rank_lanes = 1;  // a bisection a lane where kRankLanes reaches: nruns - 1 of them
  while (d.rank_lanes < kRankLanes && d.rank_lanes + 1u < a.nruns) d.rank_lanes <<= 1;
  d.snapshot = a.smallest_snapshot;
  d.deeper_keys = a.deeper_keys;
  d.deeper_off = a.deeper_off;
  d.deeper_len = a.deeper_len;
  d.n_deeper = a.n_deeper;
  carve(d, scratch_base(a.scratch), a.n);
  d.out_key_off = a.out_key_off;
  d.out_key_len = a.out_key_len;
  d.out_val_off = a.out_val_off;
  d.out_val_len = a.out_val_len;
  d.out_src = a.out_src;
  d.max_out = a.max_out;
  d.dropped_src = a.dropped_src;
  d.report = a.report;

  const uint32_t n = a.n;
  const uint32_t per_entry = (n + kGroup - 1u) / kGroup;
  const uint64_t rank_groups = (uint64_t{n} * d.rank_lanes + kGroup - 1u) / kGroup;
  hipLaunchKernelGGL(merge_runs_kernel, dim3(1), dim3(64), 0, stream, d);
  hipLaunchKernelGGL(merge_check_kernel, dim3(per_entry), dim3(kGroup), 0, stream, d);
  hipLaunchKernelGGL(merge_rank_kernel, dim3(static_cast<uint32_t>(rank_groups)), dim3(kGroup), 0,
                     stream, d);
  hipLaunchKernelGGL(merge_drop_kernel, dim3(per_entry), dim3(kGroup), 0, stream, d);
  const hipError_t e = launch_exclusive_scan(d.keep, nullptr, d.sums, n, stream);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(merge_report_kernel, dim3(1), dim3(kGroup), 0, stream, d);
  hipLaunchKernelGGL(merge_write_kernel, dim3(per_entry), dim3(kGroup), 0, stream, d);
  return hipGetLastError();
}

}  // namespace lvkv
