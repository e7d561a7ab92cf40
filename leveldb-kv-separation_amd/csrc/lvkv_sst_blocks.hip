// The SSTable block writer and reader: TableBuilder::WriteBlock /
// WriteRawBlock (table/table_builder.cc:141-209) and ReadBlock
// (table/format.cc:69-159) over a batch of blocks. The writer is a pipeline
// of small kernels around a codec's launcher (lvkv_snappy.hip,
// lvkv_zstd_compress.hip): where each compressed form goes, the codec, the
// verdicts, which form each block keeps and where it lands in the file, the
// bytes. The reader is the two decompressors in block mode, one after the
// other. Both of the writer's scratch contracts are listed here, once each.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lvkv_block_scan.h"
#include "lvkv_launch.h"
#include "lvkv_scratch.h"
#include "lvkv_snappy.h"

namespace lvkv {
namespace {

// A block's slot for its compressed form: room for either codec's bound,
// rounded to 16.
__host__ __device__ constexpr uint64_t sst_slot_bytes(uint32_t n) {
  const uint64_t sb = snappy_bound(uint64_t{n}), zb = zstd_bound(uint64_t{n});
  return ((sb > zb ? sb : zb) + 15u) & ~uint64_t{15};
}

// Where each block's compressed form goes: an exclusive scan of the slots
// from `first` (the bytes before it take what a block without room writes).
// A block whose slot would end past `cap` has no room: it is compressed as
// an empty block into the spare bytes at 0 and reported by sst_status_kernel.
// One workgroup, a block a thread a pass.
__global__ void __launch_bounds__(1024) sst_slots_kernel(const uint32_t* raw_len, uint32_t n,
                                                         uint64_t first, uint64_t cap,
                                                         uint64_t* off, uint32_t* elen,
                                                         uint8_t* noroom) {
  __shared__ uint64_t wsum[17];
  uint32_t L = 0;  // the thread's block of the pass
  block_scan_carry(
      n, first, wsum,
      [&](uint32_t i) {
        L = raw_len[i];
        return sst_slot_bytes(L);
      },
      [&](uint32_t i, uint64_t at) {
        const bool room = at + sst_slot_bytes(L) <= cap;
        off[i] = room ? at : 0u;
        elen[i] = room ? L : 0u;
        noroom[i] = room ? 0 : 1;
      });
}

// The verdict the caller sees, and the one the layout acts on.
__global__ void __launch_bounds__(256) sst_status_kernel(uint8_t* cst, const uint8_t* noroom,
                                                         uint32_t n, uint8_t* status) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  uint8_t st = LVKV_SNAPPY_OK;
  if (cst != nullptr) {
    st = noroom != nullptr && noroom[i] ? static_cast<uint8_t>(LVKV_SNAPPY_TOO_LARGE) : cst[i];
    cst[i] = st;
  }
  status[i] = st;
}

// Which form each block keeps and where it lands: the compressed form when
// it is smaller than raw - raw/8 (table_builder.cc:160-168), else raw with
// type kNoCompression; handles are an exclusive scan of size + 5 (the
// trailer, :206) from file_offset, or from *base where an earlier kernel of
// the stream left the offset on the device. nfit (where asked for) = the
// blocks, a prefix, that end at or before `cap`. One workgroup, 4 blocks a
// thread a pass.
__global__ void __launch_bounds__(1024) sst_layout_kernel(const uint32_t* raw_len,
                                                          const uint32_t* clen, const uint8_t* cst,
                                                          uint32_t n, uint64_t file_offset,
                                                          uint64_t* hoff, uint32_t* hsize,
                                                          uint8_t* type, uint64_t* end,
                                                          uint32_t ctype, const uint64_t* base,
                                                          uint64_t cap, uint32_t* nfit) {
  __shared__ uint64_t wsum[17];
  __shared__ uint32_t fit;
  const uint32_t t = threadIdx.x;
  if (t == 0) fit = 0;
  uint64_t carry = base != nullptr ? *base : file_offset;
  uint32_t mine = 0;
  for (uint32_t base_i = 0; base_i < n; base_i += 4096) {
    uint32_t sz[4];
    uint8_t ty[4];
    uint64_t local = 0;
    for (uint32_t j = 0; j < 4; ++j) {
      const uint32_t i = base_i + 4 * t + j;
      sz[j] = 0;
      ty[j] = 0;
      if (i < n) {
        const uint32_t L = raw_len[i];
        const bool c = clen != nullptr && cst[i] == LVKV_SNAPPY_OK && clen[i] < L - L / 8u;
        sz[j] = c ? clen[i] : L;
        ty[j] = c ? static_cast<uint8_t>(ctype) : 0;
        local += sz[j] + 5u;
      }
    }
    uint64_t total;
    uint64_t at = carry + block_scan(local, wsum, &total);
    for (uint32_t j = 0; j < 4; ++j) {
      const uint32_t i = base_i + 4 * t + j;
      if (i < n) {
        hoff[i] = at;
        hsize[i] = sz[j];
        type[i] = ty[j];
        at += sz[j] + 5u;
        if (at <= cap) ++mine;
      }
    }
    carry += total;
    __syncthreads();
  }
  if (nfit != nullptr) {
    if (mine) atomicAdd(&fit, mine);
    __syncthreads();
    if (t == 0) *nfit = fit;
  }
  if (t == 0) *end = carry;
}

// WriteRawBlock's bytes but the CRC (table_builder.cc:195-204): the kept
// contents at the handle, the type byte after them; a block whose trailer
// would end past `cap` is left out. The masked CRC is the batch CRC kernel's
// (lvkv_sst_fill_trailers_device) over the same handles.
__global__ void __launch_bounds__(256) sst_place_kernel(const uint8_t* raw, const uint64_t* raw_off,
                                                        const uint8_t* comp, const uint64_t* comp_off,
                                                        uint64_t comp_stride, const uint64_t* hoff,
                                                        const uint32_t* hsize, const uint8_t* type,
                                                        uint8_t* file, uint64_t cap) {
  const uint32_t b = blockIdx.x, t = threadIdx.x;
  const uint32_t ty = type[b];
  const uint32_t n = hsize[b];
  if (hoff[b] > cap || cap - hoff[b] < uint64_t{n} + 5u) return;
  const uint8_t* src =
      ty ? comp + (comp_off ? comp_off[b] : b * comp_stride) : raw + raw_off[b];
  uint8_t* dst = file + hoff[b];
  for (uint32_t k = t; k < n; k += 256) dst[k] = src[k];
  if (t == 0) dst[n] = static_cast<uint8_t>(ty);
}

constexpr uint64_t kSstSpare = 16;  // the slot of the blocks without room

// The ragged scratch from its aligned start, listed once: the per-block
// arrays packed, the zstd compressor's pool (0 bytes up to 20,480 a block)
// between two multiples of 256. Returns where the slots start (base null:
// sizing only).
uint64_t carve_ragged(SstWriteScratch& s, uint8_t* base, uint64_t nblocks, uint32_t pool_max_len) {
  Carver c(base);
  s.slot_off = c.take<uint64_t>(nblocks);
  s.scan_len = c.take<uint32_t>(nblocks);
  s.clen = c.take<uint32_t>(nblocks);
  s.cst = c.take<uint8_t>(nblocks);
  s.noroom = c.take<uint8_t>(nblocks);
  s.zstd_pool = c.take<uint8_t>(zstd_compress_big_scratch(pool_max_len), kScratchAlign);
  s.slots = c.take<uint8_t>(0);
  return c.bytes();
}

}  // namespace

uint64_t snappy_write_stride(uint32_t max_len) { return sst_slot_bytes(max_len); }

SstWriteScratch sst_scratch_strided(uint8_t* scratch, const uint32_t* raw_len, uint32_t nblocks,
                                    uint32_t max_len) {
  SstWriteScratch s{};
  s.stride = snappy_write_stride(max_len);
  s.src_len = raw_len;
  Carver c(scratch);
  s.slots = c.take<uint8_t>(s.stride * nblocks);
  s.clen = c.take<uint32_t>(nblocks);
  s.cst = c.take<uint8_t>(nblocks);
  return s;
}

// The part of the v2 scratch that does not hold compressed blocks: alignment
// slack, the per-block arrays, the zstd compressor's pool.
uint64_t sst_write_v2_fixed(size_t nblocks, uint32_t max_len) {
  SstWriteScratch s{};
  return kScratchAlign + carve_ragged(s, nullptr, nblocks, max_len);
}

uint64_t sst_write_v2_bytes(size_t nblocks, uint64_t total_raw, uint32_t max_len) {
  // sum of slots <= total + total / 6 (MaxCompressedLength less its constant)
  // + 79 a block (either bound's constant + rounding)
  return sst_write_v2_fixed(nblocks, max_len) + kSstSpare + (snappy_bound(total_raw) - 32u) +
         uint64_t{nblocks} * 80u;
}

SstWriteScratch sst_scratch_ragged(uint8_t* scratch, uint64_t scratch_bytes, uint32_t nblocks,
                                   uint32_t pool_max_len) {
  SstWriteScratch s{};
  carve_ragged(s, scratch_base(scratch), nblocks, pool_max_len);
  s.src_len = s.scan_len;
  // (the caller checked: the slots start at least kSstSpare before the end)
  s.slot_cap = scratch_bytes - static_cast<uint64_t>(s.slots - scratch);
  return s;
}

// The pipeline: the slots scan (where the scratch has per-block offsets), the
// codec, the status merge (where a status is asked for), the layout, the
// place. An empty batch runs the layout alone, which stores end = file_offset.
// dest (may be null): the base offset on the device and a bound on the file.
hipError_t launch_sst_write_blocks(const uint8_t* raw, const uint64_t* raw_off,
                                   const uint32_t* raw_len, uint32_t nblocks, int compression,
                                   uint32_t max_len, const SstWriteScratch& s, uint8_t* file,
                                   uint64_t file_offset, uint64_t* hoff, uint32_t* hsize,
                                   uint8_t* type, uint64_t* end, int zstd_level, uint8_t* status,
                                   hipStream_t stream, const SstWriteDest* dest) {
  const bool any = nblocks != 0;
  const uint64_t* base = dest != nullptr ? dest->base : nullptr;
  const uint64_t cap = dest != nullptr ? dest->cap : ~uint64_t{0};
  uint32_t* nfit = dest != nullptr ? dest->nfit : nullptr;
  if (any && compression != 0) {
    if (s.slot_off != nullptr)
      hipLaunchKernelGGL(sst_slots_kernel, dim3(1), dim3(1024), 0, stream, raw_len, nblocks,
                         kSstSpare, s.slot_cap, s.slot_off, s.scan_len, s.noroom);
    hipError_t e;
    if (compression == 1) {
      // a stride was sized from max_len; a slot of its own holds any block's
      // bound, so the LDS takes a whole fragment whatever max_len is
      e = launch_snappy_compress(raw, raw_off, s.src_len, s.slots, s.slot_off, s.clen, s.cst,
                                 nblocks, s.slot_off != nullptr ? kSnappyFragment : max_len,
                                 s.stride, stream);
    } else {  // kZstdCompression (one kernel when max_len <= 20,480)
      e = launch_zstd_compress_big(raw, raw_off, s.src_len, s.slots, s.slot_off, s.clen, s.cst,
                                   nblocks, max_len, zstd_level, s.stride, s.zstd_pool, stream);
    }
    if (e != hipSuccess) return e;
  }
  if (any && status != nullptr)
    hipLaunchKernelGGL(sst_status_kernel, dim3((nblocks + 255u) / 256u), dim3(256), 0, stream,
                       s.cst, s.noroom, nblocks, status);
  hipLaunchKernelGGL(sst_layout_kernel, dim3(1), dim3(1024), 0, stream, raw_len, s.clen, s.cst,
                     nblocks, file_offset, hoff, hsize, type, end,
                     static_cast<uint32_t>(compression == 2 ? 2 : 1), base, cap, nfit);
  if (any)
    hipLaunchKernelGGL(sst_place_kernel, dim3(nblocks), dim3(256), 0, stream, raw, raw_off,
                       s.slots, s.slot_off, s.stride, hoff, hsize, type, file, cap);
  return hipGetLastError();
}

// ReadBlock over a batch: raw and Snappy blocks, then the kZstdCompression
// blocks whose checksum held (table/format.cc:138-155), which the first
// launch leaves alone.
hipError_t launch_sst_read_blocks(const uint8_t* file, const uint64_t* hoff, const uint32_t* hsize,
                                  uint32_t nblocks, uint8_t* out, const uint64_t* out_off,
                                  const uint32_t* out_cap, uint32_t* out_len, uint8_t* status,
                                  const uint8_t* vstatus, uint32_t max_ulen, hipStream_t stream) {
  const hipError_t e = launch_snappy_uncompress(file, hoff, hsize, out, out_off, out_cap, out_len,
                                                status, nblocks, max_ulen, 1, vstatus, stream);
  if (e != hipSuccess) return e;
  return launch_zstd_uncompress(file, hoff, hsize, out, out_off, out_cap, out_len, status, nullptr,
                                nblocks, max_ulen, 1, vstatus, stream);
}

}  // namespace lvkv
