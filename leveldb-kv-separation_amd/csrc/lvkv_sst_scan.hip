// DBIter over entries in MergingIterator's order on the device
// (db/db_iter.cc:134-219, 290-302): which entries a reader at a snapshot sees,
// and for a batch of ranges where Seek lands and how far the caller's loop
// walks. Descriptors of the visible entries come out; no key or value byte is
// copied.
//
// There is no serial walk. FindNextUserEntry's `skip` is, at every step, the
// user key of the last entry the walk passed that parses and is not above the
// snapshot (an "eligible" entry): a deletion sets it, a value that is yielded
// becomes it in Next, a hidden value has it already. So an entry is visible
// when it is an eligible value and the eligible entry directly before it has
// another user key, or there is none -- and that holds from wherever a Seek
// starts, since what precedes the seek position under the seek key has a
// trailer above (snapshot << 8 | 1) and is not eligible. A scan numbers the
// eligible entries, so "the eligible entry before me" is the entry directly
// before or, where that one is not eligible, a bisection over the scan,
// however many others lie between; a second scan numbers the visible ones.
//
// A query is two bisections over the input (the seek target; the limit as a
// user key) and three lookups in the scans: the visible entries before the
// seek position, before the limit, and the unparsable keys between the seek
// position and where the walk ends.
//
// Five kernels and the two scans' six: flags, scan, visible, scan, write,
// and with queries the query kernel and its report. Every dependency between
// workgroups is a kernel boundary. What a workgroup has to say -- the lowest
// fault it found, its counts -- it folds in LDS and leaves in a slot of its
// own; workgroup 0 of a later kernel adds the slots up (the visible kernel
// the faults, the write kernel the counts, with which it decides the status
// and writes the report). No atomic anywhere.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lvkv_key_compare.h"
#include "lvkv_launch.h"
#include "lvkv_scan.h"
#include "lvkv_scratch.h"
#include "lvkv_table_format.h"

namespace lvkv {
namespace {

constexpr uint32_t kNone = 0xffffffffu;
constexpr uint32_t kGroup = 256;  // lanes a workgroup, every kernel
constexpr uint32_t kWaves = kGroup / 64;

// The words the kernels of one call hand to each other, at the head of the scratch.
struct Ctl {
  uint32_t bad_key;   // lowest entry with a key under 8 bytes, kNone; by scan_visible_kernel
  uint32_t unsorted;  // lowest entry below its predecessor, kNone; by scan_visible_kernel
  uint32_t status;    // LVKV_SCAN_*, by scan_write_kernel
  uint32_t nvis;      // the visible entries, by scan_write_kernel
};
static_assert(sizeof(Ctl) <= kScratchAlign, "the control words' room");

// The lowest faults a workgroup of the flag kernel found.
struct Fault {
  uint32_t bad_key, unsorted;
};
static_assert(sizeof(Fault) == 8, "the sizing function counts 8 bytes a workgroup");

// What a workgroup of the visible kernel counted.
struct Part {
  uint64_t key_bytes, value_bytes;  // the visible entries'
  uint32_t deletions, reserved;
};
static_assert(sizeof(Part) == 24, "the sizing function counts 24 bytes a workgroup");

// What a workgroup of the query kernel counted.
struct QPart {
  uint64_t sum;
  uint32_t max, reserved;
};
static_assert(sizeof(QPart) == 16, "the sizing function counts 16 bytes a workgroup");

struct Dev {
  const uint8_t* keys;
  const uint64_t* key_off;
  const uint32_t* key_len;
  const uint64_t* val_off;
  const uint32_t* val_len;
  uint32_t n, nq;
  uint64_t snapshot;
  const uint8_t* qkeys;
  const uint64_t* start_off;
  const uint32_t* start_len;
  const uint64_t* limit_off;
  const uint32_t* limit_len;
  const uint32_t* q_max;  // may be null
  Ctl* ctl;
  uint64_t* elig;  // n + 1: 1 for an eligible entry, then its scan: the eligible before it
  uint64_t* bad;   // n + 1: 1 for a key that does not parse, then its scan
  uint64_t* vis;   // n + 1: 1 for a visible entry, then its scan: its slot
  Fault* faults;   // a workgroup of the flag kernel each
  Part* parts;     // a workgroup of the visible kernel each
  QPart* qparts;   // a workgroup of the query kernel each
  uint64_t* sums;
  uint64_t* out_key_off;
  uint32_t* out_key_len;
  uint64_t* out_val_off;
  uint32_t* out_val_len;
  uint32_t* out_src;
  uint64_t max_out;
  uint32_t* q_first;
  uint32_t* q_count;
  uint8_t* q_status;
  lvkv_sst_scan_report* report;
};

struct Key {
  const uint8_t* p;
  uint32_t len;
};

__device__ __forceinline__ Key key_of(const Dev& d, uint32_t e) {
  return Key{d.keys + d.key_off[e], d.key_len[e]};
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
__global__ void scan_empty_kernel(lvkv_sst_scan_report* r) {
  if (threadIdx.x != 0) return;
  lvkv_sst_scan_report e{};
  e.status = LVKV_SCAN_OK;
  e.first_bad_entry = kNone;
  *r = e;
}

// Per entry: the key's length, the order against the entry before it, and the
// two flags the scans number -- eligible (ParseInternalKey,
// db/dbformat.h:173-183, and sequence <= snapshot) and unparsable.
__global__ void __launch_bounds__(kGroup) scan_flag_kernel(Dev d) {
  __shared__ uint32_t fold[kWaves];
  const uint32_t i = blockIdx.x * kGroup + threadIdx.x;
  uint32_t bad_key = kNone, unsorted = kNone;
  if (i < d.n) {
    const Key k = key_of(d, i);
    uint64_t elig = 0, bad = 0;
    if (k.len < 8u) {
      bad_key = i;
    } else {
      const uint64_t tag = ld_le64(k.p + k.len - 8u);
      if ((tag & 0xffu) > 1u) bad = 1;
      else if ((tag >> 8) <= d.snapshot) elig = 1;
      if (i != 0) {
        const Key p = key_of(d, i - 1u);
        // (a key under 8 bytes is BAD_KEY, which comes first: no verdict here)
        if (p.len >= 8u) {
          const int c = compare_bytes(p.p, p.len - 8u, k.p, k.len - 8u);
          // InternalKeyComparator (db/dbformat.cc:47-63): the trailers descend
          if (c > 0 || (c == 0 && ld_le64(p.p + p.len - 8u) < tag)) unsorted = i;
        }
      }
    }
    d.elig[i] = elig;
    d.bad[i] = bad;
  }
  bad_key = group_fold(bad_key, fold, umin);
  unsorted = group_fold(unsorted, fold, umin);
  if (threadIdx.x == 0) d.faults[blockIdx.x] = Fault{bad_key, unsorted};
}

// Eligible entry number r - 1, for an entry i with r >= 1 eligible entries
// before it: entry i - 1 where that one is eligible, else the lowest j with
// elig[j + 1] >= r (the scan never descends).
__device__ __forceinline__ uint32_t eligible_before(const uint64_t* elig, uint32_t i, uint64_t r) {
  if (elig[i - 1u] != r) return i - 1u;
  uint32_t lo = 0, hi = i - 1u;  // elig[hi + 1] >= r
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo) / 2u;
    if (elig[mid + 1u] >= r) hi = mid;
    else lo = mid + 1u;
  }
  return lo;
}

// Per entry: visible = an eligible value whose eligible predecessor has
// another user key. Workgroup 0 also adds up the flag kernel's faults.
__global__ void __launch_bounds__(kGroup) scan_visible_kernel(Dev d) {
  __shared__ uint32_t fold[kWaves];
  __shared__ uint64_t fold64[kWaves];
  const uint32_t i = blockIdx.x * kGroup + threadIdx.x;
  uint32_t deletions = 0;
  uint64_t kb = 0, vb = 0;
  if (i < d.n) {
    uint64_t vis = 0;
    const uint64_t r = d.elig[i];
    if (d.elig[i + 1u] != r) {  // (eligible: the key has 8 bytes or more)
      const Key k = key_of(d, i);
      if (k.p[k.len - 8u] == 0) {
        deletions = 1;
      } else {
        vis = 1;
        if (r != 0) {  // (so i != 0)
          const Key p = key_of(d, eligible_before(d.elig, i, r));
          if (p.len == k.len && common_prefix(p.p, k.p, k.len - 8u) == k.len - 8u) vis = 0;
        }
      }
      if (vis != 0) {
        kb = k.len - 8u;
        vb = d.val_len[i];
      }
    }
    d.vis[i] = vis;
  }
  deletions = group_fold(deletions, fold, uadd);
  kb = group_sum64(kb, fold64);
  vb = group_sum64(vb, fold64);
  if (threadIdx.x == 0) d.parts[blockIdx.x] = Part{kb, vb, deletions, 0u};
  if (blockIdx.x != 0) return;
  uint32_t bad_key = kNone, unsorted = kNone;
  const uint32_t groups = (d.n + kGroup - 1u) / kGroup;
  for (uint32_t g = threadIdx.x; g < groups; g += kGroup) {
    const Fault f = d.faults[g];
    bad_key = umin(bad_key, f.bad_key);
    unsorted = umin(unsorted, f.unsorted);
  }
  bad_key = group_fold(bad_key, fold, umin);
  unsorted = group_fold(unsorted, fold, umin);
  if (threadIdx.x != 0) return;
  d.ctl->bad_key = bad_key;
  d.ctl->unsorted = unsorted;
}

// The verdict, with every count known: workgroup 0 of the write kernel adds up
// the visible kernel's slots; thread 0 decides, as every lane of the kernel
// has for itself.
__device__ void scan_verdict(const Dev& d) {
  __shared__ uint32_t fold[kWaves];
  __shared__ uint64_t fold64[kWaves];
  Ctl* c = d.ctl;
  uint32_t deletions = 0;
  uint64_t kb = 0, vb = 0;
  const uint32_t groups = (d.n + kGroup - 1u) / kGroup;
  for (uint32_t g = threadIdx.x; g < groups; g += kGroup) {
    const Part part = d.parts[g];
    deletions += part.deletions;
    kb += part.key_bytes;
    vb += part.value_bytes;
  }
  deletions = group_fold(deletions, fold, uadd);
  kb = group_sum64(kb, fold64);
  vb = group_sum64(vb, fold64);
  if (threadIdx.x != 0) return;
  lvkv_sst_scan_report r{};
  r.status = LVKV_SCAN_OK;
  r.first_bad_entry = kNone;
  r.num_in = d.n;
  r.nqueries = d.nq;
  if (c->bad_key != kNone || c->unsorted != kNone) {
    r.status = c->bad_key != kNone ? LVKV_SCAN_BAD_KEY : LVKV_SCAN_UNSORTED;
    r.first_bad_entry = c->bad_key != kNone ? c->bad_key : c->unsorted;
  } else {
    const uint32_t elig = static_cast<uint32_t>(d.elig[d.n]);
    r.num_visible = static_cast<uint32_t>(d.vis[d.n]);
    r.num_unparsable = static_cast<uint32_t>(d.bad[d.n]);
    r.num_above_snapshot = d.n - elig - r.num_unparsable;
    r.num_deletions = deletions;
    r.num_hidden = elig - deletions - r.num_visible;
    r.key_bytes = kb;
    r.value_bytes = vb;
    if (r.num_visible > d.max_out) r.status = LVKV_SCAN_CAPACITY;
  }
  c->status = static_cast<uint32_t>(r.status);
  c->nvis = r.num_visible;
  *d.report = r;
}

// A lane an entry: a visible entry's descriptors to its slot, where the
// status is OK -- no fault, and the visible entries fit. Workgroup 0 writes
// the report as well.
__global__ void __launch_bounds__(kGroup) scan_write_kernel(Dev d) {
  const uint32_t i = blockIdx.x * kGroup + threadIdx.x;
  const bool ok = d.ctl->bad_key == kNone && d.ctl->unsorted == kNone && d.vis[d.n] <= d.max_out;
  if (ok && i < d.n) {
    const uint64_t at = d.vis[i];
    if (d.vis[i + 1u] != at) {  // (at < num_visible <= max_out)
      d.out_key_off[at] = d.key_off[i];
      d.out_key_len[at] = d.key_len[i] - 8u;
      d.out_val_off[at] = d.val_off[i];
      d.out_val_len[at] = d.val_len[i];
      d.out_src[at] = i;
    }
  }
  if (blockIdx.x == 0) scan_verdict(d);
}

// The first entry whose user key is not below `user`, and among those of that
// user key the first whose trailer is not above `tag` (InternalKeyComparator:
// the trailers descend). tag = 2^64 - 1: the first entry of the user key.
__device__ __forceinline__ uint32_t lower_bound(const Dev& d, const uint8_t* user, uint32_t ulen,
                                                uint64_t tag) {
  uint32_t lo = 0, hi = d.n;  // entries below lo are below the target, entries from hi on are not
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo) / 2u;
    const Key k = key_of(d, mid);
    const int c = compare_bytes(k.p, k.len - 8u, user, ulen);
    if (c < 0 || (c == 0 && ld_le64(k.p + k.len - 8u) > tag)) lo = mid + 1u;
    else hi = mid;
  }
  return lo;
}

// A lane a query: DBIter::Seek and the caller's loop. Returns at once unless
// the status is OK (a bisection needs sorted keys of 8 bytes or more).
__global__ void __launch_bounds__(kGroup) scan_query_kernel(Dev d) {
  __shared__ uint32_t fold[kWaves];
  __shared__ uint64_t fold64[kWaves];
  if (d.ctl->status != LVKV_SCAN_OK) return;  // (the whole grid)
  const uint32_t q = blockIdx.x * kGroup + threadIdx.x;
  const uint32_t nvis = d.ctl->nvis;
  uint32_t count = 0;
  if (q < d.nq) {
    // (start, snapshot, kValueTypeForSeek), db/db_iter.cc:294-296
    const uint32_t seek = lower_bound(d, d.qkeys + d.start_off[q], d.start_len[q],
                                      (d.snapshot << 8) | 1u);
    const uint32_t first = static_cast<uint32_t>(d.vis[seek]);
    uint32_t end = nvis;
    const uint32_t llen = d.limit_len[q];
    if (llen != LVKV_SCAN_NO_LIMIT)
      end = static_cast<uint32_t>(d.vis[lower_bound(d, d.qkeys + d.limit_off[q], llen, ~uint64_t{0})]);
    count = end > first ? end - first : 0u;
    if (d.q_max != nullptr) count = umin(count, d.q_max[q]);
    // the loop's iterator ends on the visible entry after the last one counted
    const uint32_t after = first + count;
    const uint32_t stop = after < nvis ? d.out_src[after] : d.n;
    d.q_first[q] = first;
    d.q_count[q] = count;
    d.q_status[q] = d.bad[stop] != d.bad[seek] ? LVKV_SCAN_Q_CORRUPT : LVKV_SCAN_Q_OK;
  }
  const uint32_t most = group_fold(count, fold, umax);
  const uint64_t sum = group_sum64(count, fold64);
  if (threadIdx.x == 0) d.qparts[blockIdx.x] = QPart{sum, most, 0u};
}

// One workgroup adds up the query kernel's slots into the report.
__global__ void __launch_bounds__(kGroup) scan_query_report_kernel(Dev d) {
  __shared__ uint32_t fold[kWaves];
  __shared__ uint64_t fold64[kWaves];
  if (d.ctl->status != LVKV_SCAN_OK) return;  // (the whole workgroup)
  uint32_t most = 0;
  uint64_t sum = 0;
  const uint32_t groups = (d.nq + kGroup - 1u) / kGroup;
  for (uint32_t g = threadIdx.x; g < groups; g += kGroup) {
    const QPart part = d.qparts[g];
    most = umax(most, part.max);
    sum += part.sum;
  }
  most = group_fold(most, fold, umax);
  sum = group_sum64(sum, fold64);
  if (threadIdx.x != 0) return;
  d.report->max_count = most;
  d.report->sum_count = sum;
}

// The call's scratch, listed once: the control words, then the arrays, each
// rounded up to 16 bytes. Returns the bytes from `base` (null: sizing only).
uint64_t carve(Dev& d, uint8_t* base, uint64_t n, uint64_t nq) {
  Carver c(base);
  d.ctl = c.take<Ctl>(1, kScratchAlign);
  d.elig = c.take<uint64_t>(n + 1, 16);
  d.bad = c.take<uint64_t>(n + 1, 16);
  d.vis = c.take<uint64_t>(n + 1, 16);
  d.faults = c.take<Fault>((n + kGroup - 1) / kGroup, 16);
  d.parts = c.take<Part>((n + kGroup - 1) / kGroup, 16);
  d.qparts = c.take<QPart>((nq + kGroup - 1) / kGroup, 16);
  d.sums = c.take<uint64_t>(scan_sums_words(n), 16);
  return c.bytes();
}

}  // namespace

size_t sst_scan_scratch_bytes(size_t nentries, size_t nqueries) {
  Dev d{};
  return kScratchAlign + carve(d, nullptr, nentries, nqueries);  // alignment slack
}

hipError_t launch_sst_scan(const SstScanArgs& a, hipStream_t stream) {
  if (a.n == 0) {
    hipLaunchKernelGGL(scan_empty_kernel, dim3(1), dim3(64), 0, stream, a.report);
    return hipGetLastError();
  }
  Dev d{};
  d.keys = a.keys;
  d.key_off = a.key_off;
  d.key_len = a.key_len;
  d.val_off = a.val_off;
  d.val_len = a.val_len;
  d.n = a.n;
  d.nq = a.nq;
  d.snapshot = a.snapshot;
  d.qkeys = a.qkeys;
  d.start_off = a.start_off;
  d.start_len = a.start_len;
  d.limit_off = a.limit_off;
  d.limit_len = a.limit_len;
  d.q_max = a.q_max;
  carve(d, scratch_base(a.scratch), a.n, a.nq);
  d.out_key_off = a.out_key_off;
  d.out_key_len = a.out_key_len;
  d.out_val_off = a.out_val_off;
  d.out_val_len = a.out_val_len;
  d.out_src = a.out_src;
  d.max_out = a.max_out;
  d.q_first = a.q_first;
  d.q_count = a.q_count;
  d.q_status = a.q_status;
  d.report = a.report;

  const uint32_t n = a.n;
  const uint32_t per_entry = (n + kGroup - 1u) / kGroup;
  hipLaunchKernelGGL(scan_flag_kernel, dim3(per_entry), dim3(kGroup), 0, stream, d);
  hipError_t e = launch_exclusive_scan(d.elig, d.bad, d.sums, n, stream);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(scan_visible_kernel, dim3(per_entry), dim3(kGroup), 0, stream, d);
  e = launch_exclusive_scan(d.vis, nullptr, d.sums, n, stream);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(scan_write_kernel, dim3(per_entry), dim3(kGroup), 0, stream, d);
  if (a.nq != 0) {
    const uint32_t per_query = (a.nq + kGroup - 1u) / kGroup;
    hipLaunchKernelGGL(scan_query_kernel, dim3(per_query), dim3(kGroup), 0, stream, d);
    hipLaunchKernelGGL(scan_query_report_kernel, dim3(1), dim3(kGroup), 0, stream, d);
  }
  return hipGetLastError();
}

}  // namespace lvkv
