// Everything that crosses a translation unit inside the library, declared
// once: the kernel launchers (each defined beside its kernels), the
// scratch-size functions their callers size buffers with (each defined beside
// the one listing of its layout; lvkv_scratch.h has the carver), the
// production kernel choices, and the two codec bounds. Every file that defines one of
// these includes this header, so a signature that drifts fails to compile
// instead of failing when the library is loaded.
#ifndef LVKV_LAUNCH_H_
#define LVKV_LAUNCH_H_

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "lvkv_crc32c.h"
#include "lvkv_kernel_args.h"
#include "lvkv_memtable.h"
#include "lvkv_scan.h"
#include "lvkv_snappy.h"
#include "lvkv_vtable.h"

namespace lvkv {

// ---- codec bounds -----------------------------------------------------------

// ZSTD_compressBound (zstd.h, ZSTD_COMPRESSBOUND): the longest frame the
// compressor writes for n bytes. In the caller's integer type.
template <typename T>
__host__ __device__ constexpr T zstd_bound(T n) {
  return n + (n >> 8) + (n < (128u << 10) ? ((128u << 10) - n) >> 11 : 0u);
}
// snappy::MaxCompressedLength (snappy.cc): the longest stream for n bytes.
template <typename T>
__host__ __device__ constexpr T snappy_bound(T n) {
  return 32u + n + n / 6u;
}
// snappy's kBlockSize: a block is compressed in fragments of this, so the
// compressor's LDS holds any block once max_len reaches it.
constexpr uint32_t kSnappyFragment = 1u << 16;
static_assert(zstd_bound(0u) == 64 && zstd_bound(4096u) == 4174, "ZSTD_compressBound");
static_assert(zstd_bound(131071u) == 131582 && zstd_bound(131072u) == 131584, "ZSTD_compressBound");
static_assert(snappy_bound(0u) == 32 && snappy_bound(4096u) == 4810, "snappy::MaxCompressedLength");

// ---- batch CRC32C (crc32c_kernel.hip, crc32c_uniform.hip, crc32c_compact.hip,
// crc32c_ragged.hip) ----------------------------------------------------------

hipError_t launch_crc32c_batch(const KernelArgs& args, bool uniform_aligned, int num_groups,
                               hipStream_t stream);
hipError_t launch_crc32c_general(const KernelArgs& a, int cus, hipStream_t stream);
int ragged_blocks_per_round(int cfg);
hipError_t launch_crc32c_ragged(const KernelArgs& a, const uint32_t* zpow,
                                const uint32_t* lane_cols, int cfg, int num_groups,
                                hipStream_t stream);
hipError_t launch_crc32c_long(const KernelArgs& args, const uint32_t* zpow,
                              const uint32_t* lane_cols, int num_groups, hipStream_t stream);
hipError_t launch_crc32c_uniform(const UniformArgs& args, int variant, int num_groups,
                                 hipStream_t stream);
// Lane tables loaded first and written with the row tables (no end barrier),
// chain A's loads issued before the row-table fill: the fastest schedule
// measured (tools/probe.py v780; profiles/).
constexpr int kSmallProductionVariant = 4 | 8;
hipError_t launch_crc32c_uniform_small(const UniformArgs& args, int variant, int num_groups,
                                       hipStream_t stream);
hipError_t launch_crc32c_compact(const UniformArgs& args, int cfg, int num_groups,
                                 hipStream_t stream);
int compact_capacity(int cfg);
int compact_occupancy(int cfg);
// 8 waves x 3 chains, two workgroups per CU, generated lane tables
constexpr int kCompactProductionCfg = 9;

// ---- whole-SSTable verify (lvkv_sst_table.hip) ------------------------------

hipError_t launch_sst_tables(const uint8_t* file, const uint64_t* toff, const uint64_t* tsize,
                             uint64_t single_size, uint32_t ntables, uint64_t* d_off,
                             uint32_t* d_size, uint32_t* d_actual, uint8_t* d_status,
                             uint32_t capacity, lvkv_sst_report* reports, const FilterKey& fk,
                             uint32_t gen, const KernelArgs& verify, const uint32_t* zpow,
                             const uint32_t* lane_cols, int groups, int form,
                             hipStream_t stream);

// ---- the WAL (lvkv_log_blocks.hip, lvkv_log_assemble.hip) -------------------

size_t log_scratch_bytes(uint64_t size, uint32_t capacity, int cus);
hipError_t launch_log_blocks(const uint8_t* file, uint64_t size, uint64_t* hdr_off,
                             uint32_t* actual, uint8_t* rec_status, uint32_t capacity,
                             uint8_t* block_status, uint32_t* block_drop, lvkv_log_report* r,
                             const uint32_t* zpow, const uint32_t* lane_cols, int cus,
                             void* scratch, uint32_t* events, uint64_t* item_off,
                             hipStream_t stream);
size_t log_asm_scratch_bytes(size_t max_items);
hipError_t launch_log_assemble(const uint32_t* events, const uint64_t* item_off,
                               const uint64_t* hdr_off, const lvkv_log_report* phys,
                               uint64_t size, uint32_t capacity, uint64_t initial_offset,
                               lvkv_log_record* recs, uint32_t rec_cap,
                               lvkv_log_corruption* reps, uint32_t rep_cap,
                               lvkv_log_read_report* out, void* scratch, hipStream_t stream);
size_t log_gather_scratch_bytes(size_t capacity);
hipError_t launch_log_gather(const uint8_t* file, const uint64_t* hdr_off, size_t capacity,
                             const lvkv_log_report* phys, const lvkv_log_record* recs,
                             uint32_t rec_cap, const lvkv_log_read_report* read, uint8_t* out,
                             uint64_t out_cap, uint64_t* rec_pos, void* look, uint32_t tag,
                             int cus, hipStream_t stream);

// ---- block codecs (lvkv_snappy.hip, lvkv_zstd.hip, lvkv_zstd_compress.hip) --
// Compressors: dst_off == nullptr puts block b's output at b * dst_stride, and
// a block longer than max_len is then TOO_LARGE. Decompressors: block_mode 1
// is ReadBlock (src_off/src_len are block handles, the type byte after the
// contents picks the codec, statuses are LVKV_READ_*), vstatus the checksum
// verdicts (nullptr: not verified).

hipError_t launch_snappy_compress(const uint8_t* src, const uint64_t* src_off,
                                  const uint32_t* src_len, uint8_t* dst, const uint64_t* dst_off,
                                  uint32_t* dst_len, uint8_t* status, uint32_t nblocks,
                                  uint32_t max_len, uint64_t dst_stride, hipStream_t stream);
hipError_t launch_snappy_uncompress(const uint8_t* src, const uint64_t* src_off,
                                    const uint32_t* src_len, uint8_t* dst, const uint64_t* dst_off,
                                    const uint32_t* dst_cap, uint32_t* out_len, uint8_t* status,
                                    uint32_t nblocks, uint32_t max_ulen, uint32_t block_mode,
                                    const uint8_t* vstatus, hipStream_t stream);
hipError_t launch_zstd_compress(const uint8_t* src, const uint64_t* src_off, const uint32_t* src_len,
                                uint8_t* dst, const uint64_t* dst_off, uint32_t* dst_len,
                                uint8_t* status, uint32_t nblocks, uint32_t max_len, int level,
                                uint64_t dst_stride, hipStream_t stream);
size_t zstd_compress_big_scratch(uint32_t max_len);
hipError_t launch_zstd_compress_big(const uint8_t* src, const uint64_t* src_off,
                                    const uint32_t* src_len, uint8_t* dst, const uint64_t* dst_off,
                                    uint32_t* dst_len, uint8_t* status, uint32_t nblocks,
                                    uint32_t max_len, int level, uint64_t dst_stride,
                                    uint8_t* scratch, hipStream_t stream);
hipError_t launch_zstd_uncompress(const uint8_t* src, const uint64_t* src_off,
                                  const uint32_t* src_len, uint8_t* dst, const uint64_t* dst_off,
                                  const uint32_t* dst_cap, uint32_t* out_len, uint8_t* status,
                                  uint32_t* detail, uint32_t nblocks, uint32_t max_ulen,
                                  uint32_t block_mode, const uint8_t* vstatus, hipStream_t stream);

// ---- the block writer and reader (lvkv_sst_blocks.hip) ----------------------

// What a call of the writer works on besides the caller's arrays: where each
// block's compressed form goes and the per-block arrays of the pipeline,
// carved out of the caller's scratch by one of the two functions below (all
// null for compression 0 and for an empty batch). Each of the two layouts is
// listed once, in lvkv_sst_blocks.hip.
struct SstWriteScratch {
  uint8_t* slots;           // the compressed forms
  uint64_t* slot_off;       // block b's at slots + slot_off[b]; nullptr: at b * stride
  uint64_t stride;
  uint64_t slot_cap;        // slot_off: the bytes the slots may take (their scan's bound)
  const uint32_t* src_len;  // the lengths the compressor reads: raw_len, or the scan's
  uint32_t* scan_len;       //   own (0 for a block without room), written by it
  uint32_t* clen;           // compressed lengths
  uint8_t* cst;             // the codec's verdicts
  uint8_t* noroom;          // slot_off: 1 for a block whose slot did not fit
  uint8_t* zstd_pool;       // slot_off: the zstd compressor's pool
};
// The fixed-stride contract, nblocks * (stride + 5) bytes
// (lvkv_sst_write_scratch_bytes): the slots, then clen, then cst.
uint64_t snappy_write_stride(uint32_t max_len);
SstWriteScratch sst_scratch_strided(uint8_t* scratch, const uint32_t* raw_len, uint32_t nblocks,
                                    uint32_t max_len);
// The ragged contract (lvkv_sst_write_scratch_bytes_v2): up to 255 bytes of
// alignment, the per-block arrays slot_off, scan_len, clen, cst, noroom, the
// zstd pool (sized by pool_max_len: 0 without zstd) between two multiples of
// 256, 16 spare bytes, then the slots.
uint64_t sst_write_v2_fixed(size_t nblocks, uint32_t max_len);
uint64_t sst_write_v2_bytes(size_t nblocks, uint64_t total_raw, uint32_t max_len);
SstWriteScratch sst_scratch_ragged(uint8_t* scratch, uint64_t scratch_bytes, uint32_t nblocks,
                                   uint32_t pool_max_len);
// For a call whose place in the file an earlier kernel of the stream decides
// (the table writer's metaindex and index blocks): the first block's file
// offset is read from *base on the device instead of file_offset (nullptr:
// file_offset), nothing is written at or past file + cap, and *nfit (when not
// null) = how many blocks, a prefix, ended at or before cap.
struct SstWriteDest {
  const uint64_t* base;
  uint64_t cap;
  uint32_t* nfit;
};
// status: the codec's verdict per block, or nullptr. dest: nullptr for the
// host's file_offset and a file that holds everything.
hipError_t launch_sst_write_blocks(const uint8_t* raw, const uint64_t* raw_off,
                                   const uint32_t* raw_len, uint32_t nblocks, int compression,
                                   uint32_t max_len, const SstWriteScratch& s, uint8_t* file,
                                   uint64_t file_offset, uint64_t* hoff, uint32_t* hsize,
                                   uint8_t* type, uint64_t* end, int zstd_level, uint8_t* status,
                                   hipStream_t stream, const SstWriteDest* dest = nullptr);
hipError_t launch_sst_read_blocks(const uint8_t* file, const uint64_t* hoff, const uint32_t* hsize,
                                  uint32_t nblocks, uint8_t* out, const uint64_t* out_off,
                                  const uint32_t* out_cap, uint32_t* out_len, uint8_t* status,
                                  const uint8_t* vstatus, uint32_t max_ulen, hipStream_t stream);

// ---- TableBuilder::Finish on the device (lvkv_sst_finish.hip) ---------------

// The words the kernels of one lvkv_sst_write_table_device call hand to each
// other and to the two writer calls around them, at the head of the scratch.
struct SstFinishCtl {
  uint64_t data_end;       // the data blocks' writer: the offset after them
  uint64_t tail_base;      // where the metaindex block goes (kNowhere: nothing is built)
  uint64_t tail_end;       // the tail's writer: the offset after the index block
  uint64_t nkeys;
  uint64_t filter_bytes;   // the filters alone, without the offset array
  uint64_t filter_size;    // the filter block's contents
  uint64_t index_entries;  // the index block's entries, without its restarts
  uint64_t t_hoff[3];      // handles of the filter, metaindex and index blocks
  uint64_t t_raw_off[2];   // metaindex and index contents in the tail image
  uint32_t t_hsize[3];
  uint32_t t_raw_len[2];
  uint32_t nfit_data, nfit_tail;  // SstWriteDest::nfit of the two writer calls
  uint32_t tail_count;     // the tail handles whose trailers get a CRC
  uint32_t first_bad;      // lowest block the key scan rejected, 0xFFFFFFFF: none
  uint32_t ok;             // 1: every data block is sound and in the file
  uint32_t nfilters;
  uint8_t t_type[2], t_status[2];
};
// What the caller of the finisher needs of its scratch layout
// (lvkv_sst_finish.hip lists it), as byte offsets from the aligned start.
// Everything before `fixed` depends on the host's arguments alone; the data
// blocks' ragged writer scratch takes what follows.
struct SstFinishPlan {
  uint64_t tail_raw;         // the metaindex contents (kMetaRoom), then the index's
  uint64_t tail_scratch, tail_scratch_bytes;  // the tail's ragged writer scratch
  uint64_t index_cap;        // the longest index block of nblocks entries
  uint64_t fixed;
  uint32_t tail_max_len;     // the tail writer's max_len: min(index_cap, 128 KiB)
  uint32_t bits_groups;      // workgroups of the bit-setting grid
};
constexpr uint32_t kSstMetaRoom = 128;
// sst_write_v2_bytes, never smaller for a larger max_len.
uint64_t sst_write_v2_envelope(size_t nblocks, uint64_t total_raw, uint32_t max_len);
SstFinishPlan sst_finish_plan(size_t nblocks, uint32_t max_key_len, int filter_bits_per_key);
struct SstFinishArgs {
  const uint8_t* raw;
  const uint64_t* raw_off;
  const uint32_t* raw_len;
  uint32_t nblocks;
  uint32_t key_format, bits_per_key, k, max_key_len;
  uint8_t* base;  // the aligned scratch (scratch_base): SstFinishCtl first
  uint8_t* file;
  uint64_t cap;
  const uint64_t* hoff;  // the data blocks' handles
  const uint32_t* hsize;
  lvkv_sst_table_report* report;
};
// stage 0: the control words, before the data blocks' writer; 1: everything
// between that writer and the tail's (key scan, filter block in place at
// data_end, metaindex and index contents); 2: footer and report, after it.
hipError_t launch_sst_finish(const SstFinishArgs& a, int stage, hipStream_t stream);

// ---- TableBuilder::Add on the device (lvkv_sst_build.hip) -------------------

// Entries a workgroup resolves the chain of block starts for in LDS; the call
// changes path with the entry count only here (one tile, several).
constexpr uint32_t kBuildTile = 4096;
// lvkv_sst_build_blocks_scratch_bytes: the call's arrays and alignment slack.
size_t sst_build_scratch_bytes(size_t nentries);
struct SstBuildArgs {
  const uint8_t* keys;
  const uint64_t* key_off;
  const uint32_t* key_len;
  const uint8_t* vals;
  const uint64_t* val_off;
  const uint32_t* val_len;
  uint32_t n, block_size, restart_interval, key_format;
  uint8_t* scratch;  // the caller's, sst_build_scratch_bytes long
  uint8_t* raw;
  uint64_t raw_capacity;
  uint64_t* raw_off;
  uint32_t* raw_len;
  uint64_t max_blocks;
  lvkv_sst_build_report* report;
};
hipError_t launch_sst_build(const SstBuildArgs& a, hipStream_t stream);
// The device-wide exclusive scan of n u64 in place, the total at [n], of a0
// and (when not null) a1 at once: three launches. sums: scan_sums_words(n)
// words the launches hand their tile sums over in.
constexpr uint32_t kScanTile = 4096;  // items a workgroup
constexpr uint64_t scan_sums_words(uint64_t n) { return 2 * ((n + kScanTile - 1) / kScanTile); }
hipError_t launch_exclusive_scan(uint64_t* a0, uint64_t* a1, uint64_t* sums, uint32_t n,
                                 hipStream_t stream);

// ---- Block::Iter's forward walk on the device (lvkv_sst_entries.hip) --------

// The fewest bytes a restart run takes in a block: a restart and an entry.
constexpr uint64_t kEntriesRunBytes = 7;
// Bytes of the running key a group of the write kernel keeps in LDS; the bytes
// of a longer key past them are traced back to the delta they came from.
constexpr uint32_t kEntriesKeyWindow = 512;
// lvkv_sst_read_entries_scratch_bytes: the per-block arrays and a slot for
// every run total_raw_bytes can hold. The call gives the runs whatever its
// scratch_bytes leave beyond the arrays.
size_t sst_entries_scratch_bytes(size_t nblocks, uint64_t total_raw_bytes);
struct SstEntriesArgs {
  const uint8_t* raw;
  const uint64_t* raw_off;
  const uint32_t* raw_len;
  const uint8_t* skip;  // may be null
  uint32_t nblocks;
  uint8_t* scratch;
  uint64_t scratch_bytes;
  uint8_t* keys;
  uint64_t key_capacity;
  uint64_t* key_off;
  uint32_t* key_len;
  uint64_t* val_off;
  uint32_t* val_len;
  uint64_t max_entries;
  uint64_t* block_first;  // nblocks + 1
  uint8_t* block_status;
  lvkv_sst_entries_report* report;
};
hipError_t launch_sst_entries(const SstEntriesArgs& a, hipStream_t stream);

// ---- MergingIterator and compaction's drops on the device (lvkv_sst_merge.hip) --

// lvkv_sst_merge_entries_scratch_bytes: the call's arrays and alignment slack
// (the same for every run count).
size_t sst_merge_scratch_bytes(size_t nentries);
struct SstMergeArgs {
  const uint8_t* keys;
  const uint64_t* key_off;
  const uint32_t* key_len;
  const uint64_t* val_off;
  const uint32_t* val_len;
  const uint64_t* run_first;  // nruns + 1
  uint32_t n, nruns, key_format;
  uint32_t compact;  // 1: LVKV_MERGE_COMPACT
  uint64_t smallest_snapshot;
  const uint8_t* deeper_keys;
  const uint64_t* deeper_off;  // 2 * n_deeper
  const uint32_t* deeper_len;
  uint32_t n_deeper;
  uint8_t* scratch;  // the caller's, sst_merge_scratch_bytes long
  uint64_t* out_key_off;
  uint32_t* out_key_len;
  uint64_t* out_val_off;
  uint32_t* out_val_len;
  uint32_t* out_src;
  uint64_t max_out;
  uint32_t* dropped_src;  // may be null
  lvkv_sst_merge_report* report;
};
hipError_t launch_sst_merge(const SstMergeArgs& a, hipStream_t stream);

// ---- Table::InternalGet for a batch of keys on the device (lvkv_sst_get.hip) ----

// lvkv_sst_get_locate_scratch_bytes: two words for every restart the index
// block can hold, their scan's sums, the counts a workgroup of queries leaves
// and alignment slack. lvkv_sst_get_seek_scratch_bytes: those counts.
size_t sst_get_locate_scratch_bytes(uint32_t index_len, size_t nqueries);
size_t sst_get_seek_scratch_bytes(size_t nqueries);
struct SstGetLocateArgs {
  const uint8_t* index;
  uint32_t index_len;
  const uint8_t* filter;  // may be null
  uint32_t filter_len;
  const uint8_t* qkeys;
  const uint64_t* qkey_off;
  const uint32_t* qkey_len;
  uint32_t n, key_format;
  uint8_t* scratch;  // the caller's, sst_get_locate_scratch_bytes long
  uint32_t* q_block;
  uint64_t* q_handle_off;
  uint32_t* q_handle_size;
  uint8_t* q_status;
  lvkv_sst_get_locate_report* report;
};
hipError_t launch_sst_get_locate(const SstGetLocateArgs& a, hipStream_t stream);
struct SstGetSeekArgs {
  const uint8_t* raw;
  const uint64_t* raw_off;
  const uint32_t* raw_len;
  const uint8_t* skip;  // may be null
  uint32_t nblocks;
  const uint8_t* qkeys;
  const uint64_t* qkey_off;
  const uint32_t* qkey_len;
  const uint32_t* q_slot;
  uint32_t n, key_format;
  uint8_t* scratch;  // the caller's, sst_get_seek_scratch_bytes long
  uint32_t* hit_off;
  uint64_t* val_off;
  uint32_t* val_len;
  uint64_t* tag;
  uint8_t* state;
  lvkv_sst_get_seek_report* report;
};
hipError_t launch_sst_get_seek(const SstGetSeekArgs& a, hipStream_t stream);

// ---- KV separation on the device (lvkv_vtable.hip) -------------------------------

// lvkv_vtable_*_scratch_bytes: the call's arrays and alignment slack.
size_t vtable_separate_scratch_bytes(size_t nentries);
size_t vtable_resolve_scratch_bytes(size_t nqueries);
size_t vtable_gather_scratch_bytes(size_t nqueries);
struct VtableSeparateArgs {
  const uint8_t* keys;
  const uint64_t* key_off;
  const uint32_t* key_len;
  const uint8_t* vals;
  const uint64_t* val_off;
  const uint32_t* val_len;
  uint32_t n;
  uint64_t kv_sep_size, file_number;
  uint8_t* scratch;  // the caller's, vtable_separate_scratch_bytes long
  uint8_t* vtb;
  uint64_t vtb_capacity;
  uint8_t* out_vals;
  uint64_t out_val_capacity;
  uint64_t* out_val_off;
  uint32_t* out_val_len;
  uint64_t* rec_off;   // may be null
  uint64_t* rec_size;  // may be null
  lvkv_vtable_separate_report* report;
};
hipError_t launch_vtable_separate(const VtableSeparateArgs& a, hipStream_t stream);
struct VtableResolveArgs {
  const uint8_t* vals;
  const uint64_t* val_off;
  const uint32_t* val_len;
  const uint8_t* state;  // may be null
  uint32_t n;
  const uint8_t* vtb;
  const uint64_t* file_off;
  const uint64_t* file_size;
  const uint64_t* file_number;
  uint32_t nfiles;
  uint8_t* scratch;  // the caller's, vtable_resolve_scratch_bytes long
  uint8_t* status;
  uint8_t* out_src;
  uint64_t* out_off;
  uint32_t* out_len;
  lvkv_vtable_resolve_report* report;
};
hipError_t launch_vtable_resolve(const VtableResolveArgs& a, hipStream_t stream);
struct VtableGatherArgs {
  const uint8_t* vals;
  const uint8_t* vtb;
  const uint8_t* status;
  const uint8_t* out_src;
  const uint64_t* out_off;
  const uint32_t* out_len;
  uint32_t n;
  uint8_t* scratch;  // the caller's, vtable_gather_scratch_bytes long
  uint8_t* dst;
  uint64_t dst_capacity;
  uint64_t* dst_off;  // n + 1
  lvkv_vtable_gather_report* report;
};
hipError_t launch_vtable_gather(const VtableGatherArgs& a, hipStream_t stream);
// The copy kernel's tile for the calls that follow, in 16-byte stores a lane
// (1, 2, 4, 8; 0: the production choice). Measurement only (tools/vtable_bench.py).
bool vtable_set_copy_rows(int rows);

// ---- the memtable on the device (lvkv_memtable.hip) -----------------------------

// Bytes of a batch its wave holds in LDS at a time, and the pairs a workgroup
// sorts in LDS; the call changes path with the sizes only there.
constexpr uint32_t kMemtableWindow = 8192;
constexpr uint32_t kMemtableTile = 1024;
// lvkv_memtable_scratch_bytes: the call's arrays and alignment slack.
size_t memtable_scratch_bytes(size_t nbatches, size_t max_entries);
struct MemtableArgs {
  const uint8_t* payload;
  const uint64_t* batch_off;
  const uint64_t* batch_len;
  uint32_t nbatches, flags;
  uint64_t max_sequence_in;
  uint8_t* scratch;  // the caller's, memtable_scratch_bytes long
  uint8_t* keys;
  uint64_t key_capacity;
  uint64_t* key_off;
  uint32_t* key_len;
  uint64_t* val_off;
  uint32_t* val_len;
  uint32_t* src;
  uint32_t max_entries;
  uint8_t* batch_status;    // may be null
  uint32_t* batch_entries;  // may be null
  lvkv_memtable_report* report;
};
hipError_t launch_memtable(const MemtableArgs& a, hipStream_t stream);
// The sort tile for the calls that follow (512, 1024, 2048; 0: the production
// choice). Measurement only (tools/memtable_bench.py).
bool memtable_set_tile(int pairs);

// ---- DBIter over merged entries at a snapshot (lvkv_sst_scan.hip) ----------------

// lvkv_sst_scan_entries_scratch_bytes: the call's arrays and alignment slack.
size_t sst_scan_scratch_bytes(size_t nentries, size_t nqueries);
struct SstScanArgs {
  const uint8_t* keys;
  const uint64_t* key_off;
  const uint32_t* key_len;
  const uint64_t* val_off;
  const uint32_t* val_len;
  uint32_t n;
  uint64_t snapshot;
  const uint8_t* qkeys;
  const uint64_t* start_off;
  const uint32_t* start_len;
  const uint64_t* limit_off;
  const uint32_t* limit_len;
  const uint32_t* q_max;  // may be null
  uint32_t nq;
  uint8_t* scratch;  // the caller's, sst_scan_scratch_bytes long
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
hipError_t launch_sst_scan(const SstScanArgs& a, hipStream_t stream);

#ifdef LVKV_PROBE_BUILD
// Probe builds (tools/probe/liblvkv_probe.so): timestamp buffers and knobs
// set through lvkv_debug_*, the schedule-variant and read-bandwidth launchers.
extern uint64_t* g_log_stamps;
extern uint64_t* g_asm_stamps;
extern uint64_t* g_sst_stamps;
extern uint32_t g_log_knobs;
extern uint64_t* g_zstd_stamps;
extern uint64_t* g_zstdc_stamps;
hipError_t launch_crc32c_probe(const KernelArgs& args, int variant, int num_groups,
                               hipStream_t stream);
hipError_t launch_read_bw(const void* p, uint64_t bytes, uint32_t* out, int num_groups,
                          hipStream_t stream);
#endif

}  // namespace lvkv

#endif  // LVKV_LAUNCH_H_
