// TableBuilder::Finish on the device (table/table_builder.cc:213-268): what a
// table holds besides its data blocks -- the filter block
// (table/filter_block.cc, util/bloom.cc), the metaindex block, the index
// block with its shortened separators (util/comparator.cc,
// db/dbformat.cc:65-97) and the footer (table/format.cc) -- from the data
// blocks' contents and the handles the block writer gave them, which exist
// only on the device. lvkv_sst_write_table_device (lvkv_capi.cpp) runs the
// block writer for the data blocks, stage 1 here, the block writer again for
// [metaindex, index], stage 2 here.
//
// The unit of the two kernels that decode entries is the restart run: its
// first entry has shared == 0, so a lane rebuilds the run's keys without what
// came before. A block has kLanes lanes (blocks of the default block_size
// hold two to four runs of 16 entries), 64 / kLanes blocks share a wave.
//
// The key scan checks every block (nothing below trusts a block it has not
// passed: a rejected block ends the call with BAD_BLOCK before any later
// kernel decodes anything) and leaves, per block, the entry count, where its
// first key lies in the block, and its last key in the scratch.
//
// The filters are built where they go, in the file at data_end, so that no
// second copy of them needs a place in the scratch the caller sized without
// knowing the key count: block i's keys belong to filter hoff[i] >> 11
// (FilterBlockBuilder::StartBlock is called with the offset after a block,
// which is the next block's handle offset), a filter's size follows from the
// keys of the blocks that share it, and the Bloom hashes are computed again
// by the bit-setting pass instead of being kept. Bits are set with atomic OR
// on the aligned dword that holds the byte (a filter starts at any byte).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lvkv_block_scan.h"
#include "lvkv_launch.h"
#include "lvkv_scratch.h"
#include "lvkv_snappy.h"
#include "lvkv_table_format.h"

namespace lvkv {
namespace {

constexpr uint32_t kLanes = 8;           // lanes a block in the entry-decoding kernels
constexpr uint32_t kBlocksPerWave = 64 / kLanes;
constexpr uint32_t kLdsKeyMax = 512;     // max_key_len up to which a wave's 64 keys live in LDS
constexpr uint32_t kBitsGroups = 256;    // workgroups of the bit-setting grid with keys in HBM
constexpr uint64_t kNowhere = uint64_t{1} << 62;  // a base offset no capacity reaches
constexpr uint32_t kNone = 0xffffffffu;
constexpr uint32_t kFlagBad = 1, kFlagLong = 2;

// The arguments as the kernels see them: typed pointers into the scratch.
struct Dev {
  const uint8_t* raw;
  const uint64_t* raw_off;
  const uint32_t* raw_len;
  uint32_t n, key_format, bits_per_key, k, max_key_len;
  SstFinishCtl* ctl;
  uint64_t *kx, *fo, *fsz, *io;
  uint32_t *cnt, *first_off, *first_len, *last_len, *head, *next_head, *sep_d, *klen, *esz;
  uint8_t* verdict;
  uint8_t *last_key, *key_buf, *meta, *index;
  uint8_t* file;
  uint64_t cap;
  const uint64_t* hoff;
  const uint32_t* hsize;
  lvkv_sst_table_report* report;
};

__global__ void finish_init_kernel(SstFinishCtl* c) {
  if (threadIdx.x != 0) return;
  SstFinishCtl z{};
  z.tail_base = kNowhere;
  z.first_bad = kNone;
  z.t_raw_off[1] = kSstMetaRoom;
  *c = z;
}

// The key scan. kLanes lanes a block, a run a lane a turn.
__global__ void __launch_bounds__(64) finish_scan_kernel(Dev d) {
  const uint32_t lane = threadIdx.x, sub = lane % kLanes;
  const uint32_t b = blockIdx.x * kBlocksPerWave + lane / kLanes;
  const bool live = b < d.n;
  uint32_t flags = 0, cnt = 0;
  if (live) {
    const uint32_t L = d.raw_len[b];
    const uint8_t* p = d.raw + d.raw_off[b];
    uint8_t* last = d.last_key + uint64_t{b} * d.max_key_len;
    uint32_t nr = 0, limit = 0;
    if (!block_restarts(p, L, &nr, &limit)) flags = kFlagBad;
    for (uint32_t r = sub; r < nr && flags == 0; r += kLanes) {
      uint32_t pos, e;
      if (!block_run(p, nr, limit, r, &pos, &e)) {
        flags = kFlagBad;
        break;
      }
      const bool keep = r + 1 == nr;  // the block's last key ends this run
      uint32_t klen = 0;
      bool first = true;
      while (pos < e) {
        uint32_t sh, ns, vl;
        const uint8_t* q = decode_entry(p + pos, p + e, &sh, &ns, &vl);
        if (q == nullptr || sh > klen || (first && sh != 0)) {
          flags = kFlagBad;
          break;
        }
        if (uint64_t{sh} + ns > d.max_key_len) {
          flags = kFlagLong;
          break;
        }
        klen = sh + ns;
        if (d.key_format == 1 && klen < 8) {
          flags = kFlagBad;
          break;
        }
        if (first && r == 0) {
          d.first_off[b] = static_cast<uint32_t>(q - p);
          d.first_len[b] = ns;
        }
        if (keep)
          for (uint32_t i = 0; i < ns; ++i) last[sh + i] = q[i];
        first = false;
        ++cnt;
        pos = static_cast<uint32_t>(q - p) + ns + vl;
      }
      if (keep) d.last_len[b] = klen;
    }
  }
  for (uint32_t m = 1; m < kLanes; m <<= 1) {
    flags |= __shfl_xor(flags, m);
    cnt += __shfl_xor(cnt, m);
  }
  if (live && sub == 0) {
    const uint8_t v = (flags & kFlagBad)    ? LVKV_TABLE_BAD_BLOCK
                      : (flags & kFlagLong) ? LVKV_TABLE_KEY_TOO_LONG
                                            : LVKV_TABLE_OK;
    d.verdict[b] = v;
    d.cnt[b] = v ? 0u : cnt;
    if (v) atomicMin(&d.ctl->first_bad, b);
  }
}

// The filter block's layout (table/filter_block.cc): the keys before each
// block, then per filter -- the blocks whose handle offset has the same
// >> 11, led by the first of them -- its keys, its bytes (util/bloom.cc:
// 29-40) and where they start. One workgroup, a block a thread a pass.
__global__ void __launch_bounds__(1024) finish_layout_kernel(Dev d) {
  __shared__ uint64_t wsum[17];
  const uint32_t t = threadIdx.x, n = d.n;
  SstFinishCtl* c = d.ctl;
  const uint64_t nkeys = block_scan_carry(n, 0, wsum, [&](uint32_t i) { return d.cnt[i]; },
                                          [&](uint32_t i, uint64_t at) { d.kx[i] = at; });
  if (t == 0) d.kx[n] = nkeys;
  __threadfence();
  __syncthreads();
  const uint64_t data_end = c->data_end;
  bool ok = c->first_bad == kNone && c->nfit_data == n && data_end <= d.cap;
  uint64_t fbytes = 0, fsize = 0, nf = 0;
  if (ok && d.bits_per_key != 0) {
    // a head's value: its filter's bytes and the probe count; 0 for the rest
    bool head = false;
    auto filter_size = [&](uint32_t i) -> uint64_t {
      const uint64_t f = d.hoff[i] >> kFilterBaseLg;
      head = i == 0 || (d.hoff[i - 1] >> kFilterBaseLg) != f;
      if (!head) return 0;
      // (a sound block and its trailer take 16 bytes or more: at most 128
      // blocks share a filter)
      uint32_t j = i;
      do d.head[j++] = i;
      while (j < n && (d.hoff[j] >> kFilterBaseLg) == f);
      const uint64_t keys = d.kx[j] - d.kx[i];
      uint64_t bits = keys * d.bits_per_key;
      if (bits < 64) bits = 64;
      const uint64_t size = (bits + 7) / 8;
      d.next_head[i] = j;
      d.fsz[i] = size;
      return size + 1;
    };
    fbytes = block_scan_carry(n, 0, wsum, filter_size, [&](uint32_t i, uint64_t at) {
      if (head) d.fo[i] = at;
    });
    // filters emitted: up to the last block's own, and the empty ones a long
    // last block leaves behind it
    if (n != 0) {
      nf = (d.hoff[n - 1] >> kFilterBaseLg) + 1;
      if ((data_end >> kFilterBaseLg) > nf) nf = data_end >> kFilterBaseLg;
    }
    fsize = fbytes + 4 * nf + 5;
    // (offsets are fixed32, the handle size the CRC kernel's u32)
    if (fsize > 0xfffffff0ull || d.cap - data_end < fsize + 5) ok = false;
  }
  if (t == 0) {
    c->nkeys = nkeys;
    c->ok = ok ? 1u : 0u;
    c->filter_bytes = ok ? fbytes : 0;
    c->filter_size = ok ? fsize : 0;
    c->nfilters = ok ? static_cast<uint32_t>(nf) : 0;
    c->t_hoff[0] = data_end;
    c->t_hsize[0] = ok ? static_cast<uint32_t>(fsize) : 0;
    c->tail_base = !ok ? kNowhere : data_end + (d.bits_per_key != 0 ? fsize + 5 : 0);
  }
}

// The filters' bytes to 0 before the bits are set.
__global__ void __launch_bounds__(256) finish_zero_kernel(Dev d) {
  const SstFinishCtl* c = d.ctl;
  if (!c->ok) return;
  uint8_t* f = d.file + c->data_end;
  const uint64_t nbytes = c->filter_bytes;
  for (uint64_t i = uint64_t{blockIdx.x} * 256u + threadIdx.x; i < nbytes;
       i += uint64_t{gridDim.x} * 256u)
    f[i] = 0;
}

// BloomFilterPolicy::CreateFilter's bits (util/bloom.cc:42-54), the keys
// rebuilt run by run in the lane's buffer: max_key_len bytes of LDS, or of the
// scratch (a grid of kBitsGroups then) where 64 keys are more than 32 KiB.
// The blocks passed the scan; every read and copy is bounded all the same.
__global__ void __launch_bounds__(64) finish_bits_kernel(Dev d) {
  extern __shared__ uint8_t lds_keys[];
  const SstFinishCtl* c = d.ctl;
  if (!c->ok) return;
  const uint32_t lane = threadIdx.x, sub = lane % kLanes;
  uint8_t* key = d.max_key_len <= kLdsKeyMax
                     ? lds_keys + lane * d.max_key_len
                     : d.key_buf + (uint64_t{blockIdx.x} * 64u + lane) * d.max_key_len;
  uint8_t* filters = d.file + c->data_end;
  for (uint64_t b64 = uint64_t{blockIdx.x} * kBlocksPerWave + lane / kLanes; b64 < d.n;
       b64 += uint64_t{gridDim.x} * kBlocksPerWave) {
    const uint32_t b = static_cast<uint32_t>(b64);
    const uint32_t L = d.raw_len[b];
    const uint8_t* p = d.raw + d.raw_off[b];
    uint32_t nr = 0, limit = 0;
    if (!block_restarts(p, L, &nr, &limit)) continue;
    const uint32_t h = d.head[b];
    const uint64_t nbits = d.fsz[h] * 8;
    uint8_t* fil = filters + d.fo[h];
    for (uint32_t r = sub; r < nr; r += kLanes) {
      uint32_t pos, e;
      if (!block_run(p, nr, limit, r, &pos, &e)) break;
      uint32_t klen = 0;
      while (pos < e) {
        uint32_t sh, ns, vl;
        const uint8_t* q = decode_entry(p + pos, p + e, &sh, &ns, &vl);
        if (q == nullptr || sh > klen || uint64_t{sh} + ns > d.max_key_len) break;
        for (uint32_t i = 0; i < ns; ++i) key[sh + i] = q[i];
        klen = sh + ns;
        if (d.key_format == 1 && klen < 8) break;
        uint32_t hv = bloom_hash(key, d.key_format == 1 ? klen - 8 : klen);
        const uint32_t delta = (hv >> 17) | (hv << 15);
        for (uint32_t j = 0; j < d.k; ++j) {
          const uint64_t bit = hv % nbits;
          const uintptr_t at = reinterpret_cast<uintptr_t>(fil + (bit >> 3));
          const uint32_t mask = (1u << (bit & 7)) << (8 * (at & 3));
          atomicOr(reinterpret_cast<uint32_t*>(at & ~uintptr_t{3}), mask);
          hv += delta;
        }
        pos = static_cast<uint32_t>(q - p) + ns + vl;
      }
    }
  }
}

// What follows the bits (filter_block.cc:46-60, 78-100): each filter's probe
// count, the offset array (an empty filter has the offset of the bytes after
// the one before it), the array's own offset, kFilterBaseLg, and the type
// byte of the block's trailer.
__global__ void __launch_bounds__(256) finish_filter_tail_kernel(Dev d) {
  const SstFinishCtl* c = d.ctl;
  if (!c->ok) return;
  uint8_t* filters = d.file + c->data_end;
  const uint64_t fbytes = c->filter_bytes, nf = c->nfilters;
  uint8_t* arr = filters + fbytes;
  const uint64_t i = uint64_t{blockIdx.x} * 256u + threadIdx.x;
  if (i == 0) {
    st_le32(arr + 4 * nf, static_cast<uint32_t>(fbytes));
    arr[4 * nf + 4] = kFilterBaseLg;
    arr[4 * nf + 5] = 0;  // kNoCompression
  }
  if (i >= d.n || d.head[i] != i) return;
  const uint64_t at = d.fo[i], size = d.fsz[i];
  filters[at + size] = static_cast<uint8_t>(d.k);
  const uint64_t f = d.hoff[i] >> kFilterBaseLg;
  const uint32_t j = d.next_head[i];
  const uint64_t fend = j < d.n ? d.hoff[j] >> kFilterBaseLg : nf;
  st_le32(arr + 4 * f, static_cast<uint32_t>(at));
  for (uint64_t g = f + 1; g < fend; ++g) st_le32(arr + 4 * g, static_cast<uint32_t>(at + size + 1));
}

// The index entry of block b: its key is FindShortestSeparator(last key of
// b, first key of b + 1), or FindShortSuccessor(last key) for the last block
// (util/comparator.cc:30-66 on the user keys; db/dbformat.cc:65-97: the
// internal key is replaced only by a shorter user key, which then carries
// kMaxSequenceNumber | kValueTypeForSeek). sep_d: the byte that is
// incremented and ends the key, kNone for the key as it is.
__global__ void __launch_bounds__(256) finish_separator_kernel(Dev d) {
  if (!d.ctl->ok) return;
  const uint64_t i64 = uint64_t{blockIdx.x} * 256u + threadIdx.x;
  if (i64 >= d.n) return;
  const uint32_t b = static_cast<uint32_t>(i64);
  const uint8_t* a = d.last_key + uint64_t{b} * d.max_key_len;
  const uint32_t tag = d.key_format == 1 ? 8u : 0u;
  const uint32_t la = d.last_len[b], ua = la - tag;
  uint32_t at = kNone;
  if (b + 1 < d.n) {
    const uint8_t* l = d.raw + d.raw_off[b + 1] + d.first_off[b + 1];
    const uint32_t ul = d.first_len[b + 1] - tag;
    const uint32_t m = ua < ul ? ua : ul;
    uint32_t x = 0;
    while (x < m && a[x] == l[x]) ++x;
    if (x < m && a[x] < 0xff && a[x] + 1u < l[x]) at = x;
  } else {
    uint32_t x = 0;
    while (x < ua && a[x] == 0xff) ++x;
    if (x < ua) at = x;
  }
  if (tag != 0 && at != kNone && at + 1 >= ua) at = kNone;  // not shorter
  const uint32_t klen = at == kNone ? la : at + 1 + tag;
  d.sep_d[b] = at;
  d.klen[b] = klen;
  const uint32_t vlen = varint_len(d.hoff[b]) + varint_len(d.hsize[b]);
  d.esz[b] = 1 + varint_len(klen) + 1 + klen + vlen;
}

// Where each index entry goes, the two contents' lengths, and the metaindex
// block itself (table_builder.cc:231-246: one entry, "filter." + the
// policy's name -> the filter block's handle; none without a policy). One
// workgroup.
__global__ void __launch_bounds__(1024) finish_index_layout_kernel(Dev d) {
  __shared__ uint64_t wsum[17];
  const uint32_t t = threadIdx.x, n = d.n;
  SstFinishCtl* c = d.ctl;
  if (!c->ok) return;  // (the lengths stay 0, the base nowhere)
  const uint64_t carry = block_scan_carry(n, 0, wsum, [&](uint32_t i) { return d.esz[i]; },
                                          [&](uint32_t i, uint64_t at) { d.io[i] = at; });
  if (t != 0) return;
  c->index_entries = carry;
  const uint32_t restarts = n != 0 ? n : 1u;  // BlockBuilder starts with one
  c->t_raw_len[1] = static_cast<uint32_t>(carry + 4 * uint64_t{restarts} + 4);
  if (n == 0) st_le32(d.index, 0);
  st_le32(d.index + carry + 4 * uint64_t{restarts}, restarts);
  uint8_t* m = d.meta;
  uint32_t len = 0;
  if (d.bits_per_key != 0) {
    const char name[] = "filter.leveldb.BuiltinBloomFilter2";
    const uint32_t klen = sizeof(name) - 1;
    const uint32_t vlen = varint_len(c->data_end) + varint_len(c->filter_size);
    m[len++] = 0;
    m[len++] = static_cast<uint8_t>(klen);
    m[len++] = static_cast<uint8_t>(vlen);
    for (uint32_t i = 0; i < klen; ++i) m[len++] = static_cast<uint8_t>(name[i]);
    len = static_cast<uint32_t>(put_varint(put_varint(m + len, c->data_end), c->filter_size) - m);
  }
  st_le32(m + len, 0);
  st_le32(m + len + 4, 1);
  c->t_raw_len[0] = len + 8;
}

// The index block's entries (restart interval 1: shared 0, every entry a
// restart) into the tail image.
__global__ void __launch_bounds__(256) finish_index_write_kernel(Dev d) {
  const SstFinishCtl* c = d.ctl;
  if (!c->ok) return;
  const uint64_t i64 = uint64_t{blockIdx.x} * 256u + threadIdx.x;
  if (i64 >= d.n) return;
  const uint32_t b = static_cast<uint32_t>(i64);
  const uint8_t* a = d.last_key + uint64_t{b} * d.max_key_len;
  const uint32_t at = d.sep_d[b], klen = d.klen[b];
  const uint64_t off = d.io[b];
  uint8_t* p = d.index + off;
  const uint32_t vlen = varint_len(d.hoff[b]) + varint_len(d.hsize[b]);
  *p++ = 0;
  p = put_varint(p, klen);
  *p++ = static_cast<uint8_t>(vlen);
  if (at == kNone) {
    for (uint32_t i = 0; i < klen; ++i) p[i] = a[i];
  } else {
    for (uint32_t i = 0; i < at; ++i) p[i] = a[i];
    p[at] = static_cast<uint8_t>(a[at] + 1);
    if (d.key_format == 1) {  // PackSequenceAndType(kMaxSequenceNumber, kValueTypeForSeek)
      p[at + 1] = 1;
      for (uint32_t i = 0; i < 7; ++i) p[at + 2 + i] = 0xff;
    }
  }
  p += klen;
  p = put_varint(p, d.hoff[b]);
  p = put_varint(p, d.hsize[b]);
  st_le32(d.index + c->index_entries + 4 * uint64_t{b}, static_cast<uint32_t>(off));
}

// Footer::EncodeTo (table/format.cc:33-46) where it fits, the count of tail
// handles the CRC kernel covers, and the report.
__global__ void finish_report_kernel(Dev d) {
  if (threadIdx.x != 0) return;
  SstFinishCtl* c = d.ctl;
  const bool filter = d.bits_per_key != 0;
  lvkv_sst_table_report r{};
  r.first_bad_block = kNone;
  r.num_entries = c->nkeys;
  r.data_end = c->data_end;
  if (c->first_bad != kNone) {
    r.status = d.verdict[c->first_bad];
    r.first_bad_block = c->first_bad;
  } else if (!c->ok || c->nfit_tail != 2 || c->tail_end > d.cap || d.cap - c->tail_end < kFooterLen) {
    r.status = LVKV_TABLE_CAPACITY;
  }
  if (c->ok) {
    r.nfilters = c->nfilters;
    r.meta_type = c->t_type[0];
    r.index_type = c->t_type[1];
    r.meta_status = c->t_status[0];
    r.index_status = c->t_status[1];
    if (filter) {
      r.filter_offset = c->t_hoff[0];
      r.filter_size = c->filter_size;
    }
    r.meta_offset = c->t_hoff[1];
    r.meta_size = c->t_hsize[1];
    r.index_offset = c->t_hoff[2];
    r.index_size = c->t_hsize[2];
  }
  if (r.status == LVKV_TABLE_OK) {
    uint8_t* f = d.file + c->tail_end;
    uint8_t* const magic = f + kFooterLen - 8;
    uint8_t* p = put_varint(put_varint(f, r.meta_offset), r.meta_size);
    p = put_varint(put_varint(p, r.index_offset), r.index_size);
    while (p < magic) *p++ = 0;
    for (uint32_t i = 0; i < 8; ++i) magic[i] = static_cast<uint8_t>(kTableMagic >> (8 * i));
    r.file_size = c->tail_end + kFooterLen;
  }
  c->tail_count = c->ok ? (filter ? 1u : 0u) + c->nfit_tail : 0u;
  *d.report = r;
}

}  // namespace

// sst_write_v2_bytes made monotone in max_len. The zstd compressor's pool is
// a slot a workgroup, and its grid halves where two workgroups' LDS no longer
// share a CU, so the pool steps down once on the way to 128 KiB (and is
// constant between multiples of 16): past that block length the value is
// the larger of the two sides.
uint64_t sst_write_v2_envelope(size_t nblocks, uint64_t total_raw, uint32_t max_len) {
  static const uint32_t peak_at = [] {
    uint32_t at = 0;
    size_t peak = 0;
    for (uint32_t m = LVKV_ZSTD_COMPRESS_MAX_BLOCK; m <= LVKV_ZSTD_COMPRESS_BIG_MAX_BLOCK; m += 16) {
      const size_t v = zstd_compress_big_scratch(m);
      if (v > peak) {
        peak = v;
        at = m;
      }
    }
    return at;
  }();
  const uint64_t v = sst_write_v2_bytes(nblocks, total_raw, max_len);
  if (max_len <= peak_at) return v;
  const uint64_t p = sst_write_v2_bytes(nblocks, total_raw, peak_at);
  return v > p ? v : p;
}

namespace {

// The call's scratch, listed once: the control words, the per-block arrays
// and the key buffers, each rounded up to 16 bytes, the tail's contents, and
// between two multiples of 256 the tail's ragged writer scratch. What the
// caller needs of the layout besides the kernels' pointers is returned
// (base null: sizing only).
SstFinishPlan carve(Dev& d, uint8_t* base, uint64_t n, uint32_t max_key_len,
                    int filter_bits_per_key) {
  static_assert(sizeof(SstFinishCtl) <= kScratchAlign, "the control words' room");
  Carver c(base);
  SstFinishPlan p{};
  d.ctl = c.take<SstFinishCtl>(1, kScratchAlign);
  d.kx = c.take<uint64_t>(n + 1, 16);
  d.fo = c.take<uint64_t>(n, 16);
  d.fsz = c.take<uint64_t>(n, 16);
  d.io = c.take<uint64_t>(n, 16);
  d.cnt = c.take<uint32_t>(n, 16);
  d.first_off = c.take<uint32_t>(n, 16);
  d.first_len = c.take<uint32_t>(n, 16);
  d.last_len = c.take<uint32_t>(n, 16);
  d.head = c.take<uint32_t>(n, 16);
  d.next_head = c.take<uint32_t>(n, 16);
  d.sep_d = c.take<uint32_t>(n, 16);
  d.klen = c.take<uint32_t>(n, 16);
  d.esz = c.take<uint32_t>(n, 16);
  d.verdict = c.take<uint8_t>(n, 16);
  d.last_key = c.take<uint8_t>(n * max_key_len, 16);
  // the bit-setting grid: a wave for every 64 / kLanes blocks and its keys in
  // LDS, or kBitsGroups waves that loop, each lane's key in the scratch
  const uint64_t waves = n != 0 ? (n + kBlocksPerWave - 1) / kBlocksPerWave : 1;
  const bool hbm_keys = filter_bits_per_key > 0 && max_key_len > kLdsKeyMax;
  p.bits_groups = static_cast<uint32_t>(hbm_keys && waves > kBitsGroups ? kBitsGroups : waves);
  d.key_buf = c.take<uint8_t>(hbm_keys ? uint64_t{p.bits_groups} * 64u * max_key_len : 0, 16);
  // an index entry: shared, the key's length (a varint32), the value's, the
  // key, two varint64 of a handle whose size is a u32, its restart; then the
  // count (and the one restart of a block without entries)
  p.index_cap = n * (uint64_t{max_key_len} + 1 + 5 + 1 + 10 + 5 + 4) + 8;
  p.tail_raw = c.bytes();
  static_assert(kSstMetaRoom % 16 == 0, "the index contents follow the metaindex's room");
  d.meta = c.take<uint8_t>(kSstMetaRoom, 16);
  d.index = c.take<uint8_t>(p.index_cap, 16);
  const uint64_t big = 128u << 10;
  p.tail_max_len = static_cast<uint32_t>(p.index_cap < big ? p.index_cap : big);
  if (p.tail_max_len < kSstMetaRoom) p.tail_max_len = kSstMetaRoom;
  p.tail_scratch_bytes = sst_write_v2_envelope(2, kSstMetaRoom + p.index_cap, p.tail_max_len);
  c.align(kScratchAlign);
  p.tail_scratch = c.bytes();
  c.take<uint8_t>(p.tail_scratch_bytes, kScratchAlign);
  p.fixed = c.bytes();
  return p;
}

}  // namespace

SstFinishPlan sst_finish_plan(size_t nblocks, uint32_t max_key_len, int filter_bits_per_key) {
  Dev d{};
  return carve(d, nullptr, nblocks, max_key_len, filter_bits_per_key);
}

hipError_t launch_sst_finish(const SstFinishArgs& a, int stage, hipStream_t stream) {
  const uint32_t n = a.nblocks;
  Dev d{};
  d.raw = a.raw;
  d.raw_off = a.raw_off;
  d.raw_len = a.raw_len;
  d.n = n;
  d.key_format = a.key_format;
  d.bits_per_key = a.bits_per_key;
  d.k = a.k;
  d.max_key_len = a.max_key_len;
  d.file = a.file;
  d.cap = a.cap;
  d.hoff = a.hoff;
  d.hsize = a.hsize;
  d.report = a.report;
  const SstFinishPlan plan = carve(d, a.base, n, a.max_key_len, static_cast<int>(a.bits_per_key));
  const uint32_t per_block = n != 0 ? (n + 255u) / 256u : 1u;
  if (stage == 0) {
    hipLaunchKernelGGL(finish_init_kernel, dim3(1), dim3(64), 0, stream, d.ctl);
  } else if (stage == 1) {
    if (n != 0)
      hipLaunchKernelGGL(finish_scan_kernel, dim3((n + kBlocksPerWave - 1) / kBlocksPerWave),
                         dim3(64), 0, stream, d);
    hipLaunchKernelGGL(finish_layout_kernel, dim3(1), dim3(1024), 0, stream, d);
    if (a.bits_per_key != 0) {
      if (n != 0) {
        hipLaunchKernelGGL(finish_zero_kernel, dim3(512), dim3(256), 0, stream, d);
        hipLaunchKernelGGL(finish_bits_kernel, dim3(plan.bits_groups), dim3(64),
                           a.max_key_len <= kLdsKeyMax ? 64u * a.max_key_len : 0u, stream, d);
      }
      hipLaunchKernelGGL(finish_filter_tail_kernel, dim3(per_block), dim3(256), 0, stream, d);
    }
    if (n != 0)
      hipLaunchKernelGGL(finish_separator_kernel, dim3(per_block), dim3(256), 0, stream, d);
    hipLaunchKernelGGL(finish_index_layout_kernel, dim3(1), dim3(1024), 0, stream, d);
    if (n != 0)
      hipLaunchKernelGGL(finish_index_write_kernel, dim3(per_block), dim3(256), 0, stream, d);
  } else {
    hipLaunchKernelGGL(finish_report_kernel, dim3(1), dim3(64), 0, stream, d);
  }
  return hipGetLastError();
}

}  // namespace lvkv
