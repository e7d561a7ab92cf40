// TableBuilder::Add over sorted entries on the device (table/table_builder.cc:
// 94-123, table/block_builder.cc:55-105): prefix-compress the keys, place the
// restart points, cut a block whenever CurrentSizeEstimate() >= block_size,
// and write the blocks' contents where lvkv_sst_write_table_device reads them.
//
// Everything but the cut is per entry. With
//   A[i]  entry i's bytes with shared = lcp(key[i-1], key[i])
//   D[i]  what it costs more as a restart point (shared = 0)
//   EA    the exclusive scan of A
//   ED    the exclusive scan of D in residue-class order: entry i sits at
//         perm(i) = (entries of the classes below i % R) + i / R, so the
//         restarts s, s + R, s + 2R .. of a block that starts at s are
//         neighbours and their surcharge is a difference of two ED words
// the bytes of entries s..i-1 of a block that starts at s are ent_off(s, i)
// below, in closed form, and so is CurrentSizeEstimate() after any entry. It
// grows with the entry, so next(s), the first entry of the block after the
// one that starts at s, is a search per s, all s at once.
//
// The cut is the chain 0 -> next(0) -> next(next(0)) .. Tiles of kBuildTile
// entries resolve it in LDS by pointer doubling: build_exit_kernel leaves,
// for every entry of a tile, where a chain that passes through it leaves the
// tile; build_hop_kernel follows those exits from entry 0, one dependent load
// a tile, and leaves each tile's entry point; build_mark_kernel doubles again
// from the entry point and marks the block starts. No kernel waits for a
// workgroup of its own launch.
//
// A scan of the marks numbers the blocks, a scan of their lengths (rounded up
// to 16) places them, build_report_kernel decides the status with the whole
// layout known and nothing written yet, and build_write_kernel copies, 16
// lanes an entry, only when that status is OK.
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
constexpr uint32_t kDoublings = 12;    // 2^12 hops cover a tile
static_assert((1u << kDoublings) >= kBuildTile, "a chain has up to kBuildTile links in a tile");
static_assert(kBuildTile % 1024 == 0, "four entries a thread");
constexpr uint32_t kPerThread = kBuildTile / 1024;
constexpr uint32_t kWriteLanes = 16;   // lanes an entry in the write kernel
constexpr uint64_t kMaxBlockLen = 0x7fffffffull;

// The words the kernels of one call hand to each other, at the head of the scratch.
struct Ctl {
  uint32_t bad_key;    // lowest entry with a key under 8 bytes (key_format 1), kNone
  uint32_t unsorted;   // lowest entry not greater than its predecessor, kNone
  uint32_t max_key_len;
  uint32_t status;     // LVKV_BUILD_*, by build_report_kernel
  unsigned long long max_block_len;
  uint64_t last_len;   // the last block's contents
};
static_assert(sizeof(Ctl) <= kScratchAlign, "the control words' room");

struct Dev {
  const uint8_t* keys;
  const uint64_t* key_off;
  const uint32_t* key_len;
  const uint8_t* vals;
  const uint64_t* val_off;
  const uint32_t* val_len;
  uint32_t n, restart, key_format;
  uint32_t nq, nr;     // n / restart, n % restart
  uint64_t block_size;
  Ctl* ctl;
  uint64_t *ea, *ed, *ef, *eb;  // n + 1 each
  uint32_t *lcp, *next, *exit, *bstart, *entry;
  uint64_t* sums;
  uint8_t* raw;
  uint64_t raw_cap, max_blocks;
  uint64_t* raw_off;
  uint32_t* raw_len;
  lvkv_sst_build_report* report;
};

// Entry i's place in residue-class order.
__device__ __forceinline__ uint64_t perm(const Dev& d, uint32_t i) {
  const uint32_t c = i % d.restart, q = i / d.restart;
  return uint64_t{c} * d.nq + (c < d.nr ? c : d.nr) + q;
}

// The bytes of entries s..i-1 of a block that starts at s (s <= i <= n).
__device__ __forceinline__ uint64_t ent_off(const Dev& d, uint32_t s, uint32_t i) {
  if (i == s) return 0;
  const uint64_t p = perm(d, s), k = (i - 1u - s) / d.restart;  // restarts s .. s + kR < i
  return d.ea[i] - d.ea[s] + d.ed[p + k + 1] - d.ed[p];
}

// BlockBuilder::CurrentSizeEstimate after entry j of a block that starts at s.
__device__ __forceinline__ uint64_t estimate(const Dev& d, uint32_t s, uint32_t j) {
  return ent_off(d, s, j + 1u) + 4ull * ((j - s) / d.restart + 1u) + 4u;
}

// The first entry of the block after the one that starts at s: past the first
// j whose estimate reaches block_size (n: none does). Gallop, then bisect.
__device__ uint32_t find_next(const Dev& d, uint32_t s) {
  if (estimate(d, s, s) >= d.block_size) return s + 1u;
  const uint32_t last = d.n - 1u;
  uint32_t lo = s, hi;  // estimate(lo) < block_size <= estimate(hi)
  for (uint32_t step = 1;; step <<= 1) {
    if (step >= last - lo) {
      if (lo == last || estimate(d, s, last) < d.block_size) return d.n;
      hi = last;
      break;
    }
    const uint32_t j = lo + step;
    if (estimate(d, s, j) >= d.block_size) {
      hi = j;
      break;
    }
    lo = j;
  }
  while (hi - lo > 1u) {
    const uint32_t mid = lo + (hi - lo) / 2u;
    if (estimate(d, s, mid) >= d.block_size) hi = mid;
    else lo = mid;
  }
  return hi + 1u;
}

__global__ void build_init_kernel(Ctl* ctl) {
  if (threadIdx.x != 0) return;
  ctl->bad_key = kNone;
  ctl->unsorted = kNone;
  ctl->max_key_len = 0;
  ctl->status = LVKV_BUILD_OK;
  ctl->max_block_len = 0;
  ctl->last_len = 0;
}

// A report of no entries (nentries == 0).
__global__ void build_empty_kernel(lvkv_sst_build_report* r) {
  if (threadIdx.x != 0) return;
  r->status = LVKV_BUILD_OK;
  r->first_bad_entry = kNone;
  r->nblocks = 0;
  r->max_block_len = 0;
  r->max_key_len = 0;
  r->num_entries = 0;
  r->raw_bytes = 0;
}

// Per entry: the common prefix with the entry before, the order check that
// falls out of it, the two sizes.
__global__ void __launch_bounds__(256) build_entry_kernel(Dev d) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  uint32_t klen = 0;
  if (i < d.n) {
    klen = d.key_len[i];
    const uint32_t vlen = d.val_len[i];
    const uint8_t* k = d.keys + d.key_off[i];
    uint32_t lcp = 0;
    if (d.key_format == 1 && klen < 8u) atomicMin(&d.ctl->bad_key, i);
    if (i != 0) {
      const uint32_t plen = d.key_len[i - 1u];
      const uint8_t* p = d.keys + d.key_off[i - 1u];
      const uint32_t m = klen < plen ? klen : plen;
      // eight bytes a step where both keys allow aligned loads, then bytes
      if (((reinterpret_cast<uintptr_t>(k) | reinterpret_cast<uintptr_t>(p)) & 7u) == 0)
        while (m - lcp >= 8u && *reinterpret_cast<const uint64_t*>(k + lcp) ==
                                    *reinterpret_cast<const uint64_t*>(p + lcp))
          lcp += 8u;
      while (lcp < m && k[lcp] == p[lcp]) ++lcp;
      bool ok = true;
      if (d.key_format == 0) {
        ok = lcp < m ? k[lcp] > p[lcp] : klen > plen;
      } else if (klen >= 8u && plen >= 8u) {
        // InternalKeyComparator (db/dbformat.cc:47-63)
        const uint32_t ul = klen - 8u, pl = plen - 8u, um = ul < pl ? ul : pl;
        const uint32_t u = lcp < um ? lcp : um;
        if (u < um) ok = k[u] > p[u];
        else if (ul != pl) ok = ul > pl;
        else ok = ld_le64(k + ul) < ld_le64(p + pl);
      }
      if (!ok) atomicMin(&d.ctl->unsorted, i);
    }
    const uint64_t tail = uint64_t{varint_len(vlen)} + vlen;
    const uint64_t a = uint64_t{varint_len(lcp)} + varint_len(klen - lcp) + (klen - lcp) + tail;
    const uint64_t b = 1u + uint64_t{varint_len(klen)} + klen + tail;
    d.ea[i] = a;
    d.ed[perm(d, i)] = b - a;
    d.lcp[i] = lcp;
  }
  uint32_t mx = klen;
  for (uint32_t o = 32; o != 0; o >>= 1) {
    const uint32_t y = __shfl_xor(mx, o);
    mx = y > mx ? y : mx;
  }
  if ((threadIdx.x & 63u) == 0 && mx != 0) atomicMax(&d.ctl->max_key_len, mx);
}

// ---- the device-wide exclusive scan: n items in place, the total at [n] ------
// blockIdx.y picks the array; three launches, a kernel boundary where a
// workgroup needs another's sum. launch_exclusive_scan (below, declared in
// lvkv_launch.h) is lvkv_sst_entries.hip's scan as well.

struct ScanArgs {
  uint64_t* a[2];
  uint64_t* sums;  // tiles words an array
  uint32_t n, tiles;
};

__global__ void __launch_bounds__(1024) scan_reduce_kernel(ScanArgs s) {
  __shared__ uint64_t wsum[17];
  const uint64_t* a = s.a[blockIdx.y];
  const uint64_t first = uint64_t{blockIdx.x} * kScanTile + threadIdx.x * 4u;
  uint64_t local = 0;
  for (uint32_t k = 0; k < 4; ++k)
    if (first + k < s.n) local += a[first + k];
  uint64_t total;
  block_scan(local, wsum, &total);
  if (threadIdx.x == 0) s.sums[uint64_t{blockIdx.y} * s.tiles + blockIdx.x] = total;
}

__global__ void __launch_bounds__(1024) scan_sums_kernel(ScanArgs s) {
  __shared__ uint64_t wsum[17];
  uint64_t* sums = s.sums + uint64_t{blockIdx.x} * s.tiles;
  block_scan_carry(s.tiles, 0, wsum, [&](uint32_t t) { return sums[t]; },
                   [&](uint32_t t, uint64_t at) { sums[t] = at; });
}

__global__ void __launch_bounds__(1024) scan_apply_kernel(ScanArgs s) {
  __shared__ uint64_t wsum[17];
  uint64_t* a = s.a[blockIdx.y];
  const uint64_t first = uint64_t{blockIdx.x} * kScanTile + threadIdx.x * 4u;
  uint64_t v[4], local = 0;
  for (uint32_t k = 0; k < 4; ++k) {
    v[k] = first + k < s.n ? a[first + k] : 0;
    local += v[k];
  }
  uint64_t total;
  uint64_t run = block_scan(local, wsum, &total) +
                 s.sums[uint64_t{blockIdx.y} * s.tiles + blockIdx.x];
  for (uint32_t k = 0; k < 4; ++k) {
    if (first + k < s.n) {
      a[first + k] = run;
      run += v[k];
      if (first + k == s.n - 1u) a[s.n] = run;
    }
  }
}

// ---- the chain ----------------------------------------------------------------

// next^(2^r), stopped at the first entry at or past the tile's end.
__device__ __forceinline__ void double_jumps(const uint32_t* from, uint32_t* to, uint32_t start,
                                             uint32_t end) {
  for (uint32_t k = 0; k < kPerThread; ++k) {
    const uint32_t idx = threadIdx.x + k * 1024u;
    if (start + idx < end) {
      uint32_t v = from[idx];
      if (v < end) v = from[v - start];
      to[idx] = v;
    }
  }
}

// next(s) for every s of the tile, and where a chain through s leaves the tile.
__global__ void __launch_bounds__(1024) build_exit_kernel(Dev d) {
  __shared__ uint32_t jump[2][kBuildTile];
  const uint32_t start = blockIdx.x * kBuildTile;
  const uint32_t end = d.n - start < kBuildTile ? d.n : start + kBuildTile;
  for (uint32_t k = 0; k < kPerThread; ++k) {
    const uint32_t idx = threadIdx.x + k * 1024u;
    if (start + idx < end) {
      const uint32_t nx = find_next(d, start + idx);
      d.next[start + idx] = nx;
      jump[0][idx] = nx;
    }
  }
  __syncthreads();
  uint32_t cur = 0;
  for (uint32_t r = 0; r < kDoublings; ++r) {
    double_jumps(jump[cur], jump[cur ^ 1u], start, end);
    __syncthreads();
    cur ^= 1u;
  }
  for (uint32_t k = 0; k < kPerThread; ++k) {
    const uint32_t idx = threadIdx.x + k * 1024u;
    if (start + idx < end) d.exit[start + idx] = jump[cur][idx];
  }
  if (threadIdx.x == 0) d.entry[blockIdx.x] = kNone;
}

// From entry 0 tile to tile: one dependent load a tile the chain enters.
__global__ void build_hop_kernel(Dev d) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  for (uint32_t p = 0; p < d.n; p = d.exit[p]) d.entry[p / kBuildTile] = p;
}

// The block starts of a tile, from its entry point (kNone: a block spans it).
__global__ void __launch_bounds__(1024) build_mark_kernel(Dev d) {
  __shared__ uint32_t jump[2][kBuildTile];
  __shared__ uint8_t mark[kBuildTile];
  const uint32_t start = blockIdx.x * kBuildTile;
  const uint32_t end = d.n - start < kBuildTile ? d.n : start + kBuildTile;
  for (uint32_t k = 0; k < kPerThread; ++k) {
    const uint32_t idx = threadIdx.x + k * 1024u;
    if (start + idx < end) jump[0][idx] = d.next[start + idx];
    mark[idx] = 0;
  }
  __syncthreads();
  const uint32_t entry = d.entry[blockIdx.x];
  if (threadIdx.x == 0 && entry != kNone) mark[entry - start] = 1;
  __syncthreads();
  uint32_t cur = 0;
  if (entry != kNone) {  // (uniform over the workgroup)
    for (uint32_t r = 0; r < kDoublings; ++r) {
      // the first 2^r starts are marked and jump is next^(2^r): the next 2^r
      for (uint32_t k = 0; k < kPerThread; ++k) {
        const uint32_t idx = threadIdx.x + k * 1024u;
        if (start + idx < end && mark[idx] != 0) {
          const uint32_t v = jump[cur][idx];
          if (v < end) mark[v - start] = 1;
        }
      }
      double_jumps(jump[cur], jump[cur ^ 1u], start, end);
      __syncthreads();
      cur ^= 1u;
    }
  }
  for (uint32_t k = 0; k < kPerThread; ++k) {
    const uint32_t idx = threadIdx.x + k * 1024u;
    if (start + idx < end) {
      d.ef[start + idx] = mark[idx];
      d.eb[start + idx] = 0;  // (a length for every block index below)
    }
  }
}

// Per block start (ef scanned: the block's index): its length, rounded up to
// 16 for the scan that places it.
__global__ void __launch_bounds__(256) build_block_kernel(Dev d) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  uint64_t len = 0;
  if (i < d.n && d.ef[i + 1u] != d.ef[i]) {
    const uint32_t b = static_cast<uint32_t>(d.ef[i]), e = d.next[i];
    len = ent_off(d, i, e) + 4ull * ((e - 1u - i) / d.restart + 1u) + 4u;
    d.bstart[b] = i;
    d.eb[b] = (len + 15u) & ~uint64_t{15};
    if (e == d.n) d.ctl->last_len = len;
  }
  // the longest of the wave's blocks, one atomic a wave
  uint64_t mx = len;
  for (uint32_t o = 32; o != 0; o >>= 1) {
    const uint32_t lo = __shfl_xor(static_cast<uint32_t>(mx), o);
    const uint32_t hi = __shfl_xor(static_cast<uint32_t>(mx >> 32), o);
    const uint64_t y = (static_cast<uint64_t>(hi) << 32) | lo;
    mx = y > mx ? y : mx;
  }
  if ((threadIdx.x & 63u) == 0 && mx != 0)
    atomicMax(&d.ctl->max_block_len, static_cast<unsigned long long>(mx));
}

// The verdict, with the layout known and nothing written yet.
__global__ void build_report_kernel(Dev d) {
  if (threadIdx.x != 0) return;
  Ctl* c = d.ctl;
  lvkv_sst_build_report r;
  const uint64_t nblocks = d.ef[d.n];
  const uint64_t raw_bytes = d.eb[nblocks - 1u] + c->last_len;
  r.status = LVKV_BUILD_OK;
  r.first_bad_entry = kNone;
  r.nblocks = static_cast<uint32_t>(nblocks);
  r.max_block_len = c->max_block_len > 0xffffffffull ? 0xffffffffu
                                                    : static_cast<uint32_t>(c->max_block_len);
  r.max_key_len = c->max_key_len;
  r.num_entries = d.n;
  r.raw_bytes = raw_bytes;
  if (c->bad_key != kNone || c->unsorted != kNone) {
    // (the layout of entries out of order means nothing)
    r.status = c->bad_key != kNone ? LVKV_BUILD_BAD_KEY : LVKV_BUILD_UNSORTED;
    r.first_bad_entry = c->bad_key != kNone ? c->bad_key : c->unsorted;
    r.nblocks = 0;
    r.max_block_len = 0;
    r.raw_bytes = 0;
  } else if (c->max_block_len > kMaxBlockLen) {
    r.status = LVKV_BUILD_TOO_LARGE;
  } else if (nblocks > d.max_blocks || raw_bytes > d.raw_cap) {
    r.status = LVKV_BUILD_CAPACITY;
  }
  c->status = static_cast<uint32_t>(r.status);
  *d.report = r;
}

// kWriteLanes lanes an entry: the three varints (one lane), the key's suffix
// and the value a byte a lane; a restart point's slot; a block's first entry
// the restart count and the block's place in the caller's arrays.
__global__ void __launch_bounds__(256) build_write_kernel(Dev d) {
  const uint64_t gid = uint64_t{blockIdx.x} * 256u + threadIdx.x;
  const uint32_t sub = static_cast<uint32_t>(gid % kWriteLanes);
  if (gid / kWriteLanes >= d.n || d.ctl->status != LVKV_BUILD_OK) return;
  const uint32_t i = static_cast<uint32_t>(gid / kWriteLanes);
  const uint32_t b = static_cast<uint32_t>(d.ef[i + 1u]) - 1u;
  const uint32_t s = d.bstart[b];
  const uint32_t at = i - s;
  const bool restart = at % d.restart == 0;
  const uint64_t off = ent_off(d, s, i);
  uint8_t* const block = d.raw + d.eb[b];
  const uint32_t klen = d.key_len[i], vlen = d.val_len[i];
  const uint32_t shared = restart ? 0u : d.lcp[i];
  const uint32_t non_shared = klen - shared;
  uint8_t* dst = block + off;
  const uint32_t head = varint_len(shared) + varint_len(non_shared) + varint_len(vlen);
  if (sub == 0) put_varint(put_varint(put_varint(dst, shared), non_shared), vlen);
  dst += head;
  const uint8_t* k = d.keys + d.key_off[i] + shared;
  for (uint32_t j = sub; j < non_shared; j += kWriteLanes) dst[j] = k[j];
  dst += non_shared;
  const uint8_t* v = d.vals + d.val_off[i];
  for (uint32_t j = sub; j < vlen; j += kWriteLanes) dst[j] = v[j];
  if (restart && sub == 1) {
    const uint32_t e = d.next[s];
    uint8_t* const restarts = block + ent_off(d, s, e);
    st_le32(restarts + 4ull * (at / d.restart), static_cast<uint32_t>(off));
    if (at == 0) {
      const uint32_t count = (e - 1u - s) / d.restart + 1u;
      st_le32(restarts + 4ull * count, count);
      d.raw_off[b] = d.eb[b];
      d.raw_len[b] = static_cast<uint32_t>(ent_off(d, s, e)) + 4u * count + 4u;
    }
  }
}

}  // namespace

hipError_t launch_exclusive_scan(uint64_t* a0, uint64_t* a1, uint64_t* sums, uint32_t n,
                                 hipStream_t stream) {
  ScanArgs s{};
  s.a[0] = a0;
  s.a[1] = a1;
  s.sums = sums;
  s.n = n;
  s.tiles = (n + kScanTile - 1u) / kScanTile;
  const uint32_t arrays = a1 != nullptr ? 2u : 1u;
  hipLaunchKernelGGL(scan_reduce_kernel, dim3(s.tiles, arrays), dim3(1024), 0, stream, s);
  hipLaunchKernelGGL(scan_sums_kernel, dim3(arrays), dim3(1024), 0, stream, s);
  hipLaunchKernelGGL(scan_apply_kernel, dim3(s.tiles, arrays), dim3(1024), 0, stream, s);
  return hipGetLastError();
}

namespace {

// The call's scratch, listed once: the control words, then the arrays, each
// rounded up to 16 bytes. Returns the bytes from `base` (null: sizing only).
uint64_t carve(Dev& d, uint8_t* base, uint64_t n) {
  Carver c(base);
  d.ctl = c.take<Ctl>(1, kScratchAlign);
  d.ea = c.take<uint64_t>(n + 1, 16);
  d.ed = c.take<uint64_t>(n + 1, 16);
  d.ef = c.take<uint64_t>(n + 1, 16);
  d.eb = c.take<uint64_t>(n + 1, 16);
  d.lcp = c.take<uint32_t>(n, 16);
  d.next = c.take<uint32_t>(n, 16);
  d.exit = c.take<uint32_t>(n, 16);
  d.bstart = c.take<uint32_t>(n, 16);
  d.entry = c.take<uint32_t>((n + kBuildTile - 1) / kBuildTile, 16);
  d.sums = c.take<uint64_t>(scan_sums_words(n), 16);
  return c.bytes();
}

}  // namespace

size_t sst_build_scratch_bytes(size_t nentries) {
  Dev d{};
  return kScratchAlign + carve(d, nullptr, nentries);  // alignment slack
}

hipError_t launch_sst_build(const SstBuildArgs& a, hipStream_t stream) {
  if (a.n == 0) {
    hipLaunchKernelGGL(build_empty_kernel, dim3(1), dim3(64), 0, stream, a.report);
    return hipGetLastError();
  }
  Dev d{};
  d.keys = a.keys;
  d.key_off = a.key_off;
  d.key_len = a.key_len;
  d.vals = a.vals;
  d.val_off = a.val_off;
  d.val_len = a.val_len;
  d.n = a.n;
  d.restart = a.restart_interval;
  d.key_format = a.key_format;
  d.nq = a.n / a.restart_interval;
  d.nr = a.n % a.restart_interval;
  d.block_size = a.block_size;
  carve(d, scratch_base(a.scratch), a.n);
  d.raw = a.raw;
  d.raw_cap = a.raw_capacity;
  d.max_blocks = a.max_blocks;
  d.raw_off = a.raw_off;
  d.raw_len = a.raw_len;
  d.report = a.report;

  const uint32_t n = a.n;
  const uint32_t per_entry = (n + 255u) / 256u, tiles = (n + kBuildTile - 1u) / kBuildTile;
  hipLaunchKernelGGL(build_init_kernel, dim3(1), dim3(64), 0, stream, d.ctl);
  hipLaunchKernelGGL(build_entry_kernel, dim3(per_entry), dim3(256), 0, stream, d);
  hipError_t e = launch_exclusive_scan(d.ea, d.ed, d.sums, n, stream);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(build_exit_kernel, dim3(tiles), dim3(1024), 0, stream, d);
  hipLaunchKernelGGL(build_hop_kernel, dim3(1), dim3(64), 0, stream, d);
  hipLaunchKernelGGL(build_mark_kernel, dim3(tiles), dim3(1024), 0, stream, d);
  e = launch_exclusive_scan(d.ef, nullptr, d.sums, n, stream);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(build_block_kernel, dim3(per_entry), dim3(256), 0, stream, d);
  e = launch_exclusive_scan(d.eb, nullptr, d.sums, n, stream);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(build_report_kernel, dim3(1), dim3(64), 0, stream, d);
  const uint64_t write_groups = (uint64_t{n} * kWriteLanes + 255u) / 256u;
  hipLaunchKernelGGL(build_write_kernel, dim3(static_cast<uint32_t>(write_groups)), dim3(256), 0,
                     stream, d);
  return hipGetLastError();
}

}  // namespace lvkv
