/*
 * lvkv_snappy.h — C-ABI of the device Snappy block codec (SURVEY.md §8(f)
 * row 4): the codec on either side of the block CRC when tables are written
 * or read with kSnappyCompression.
 *
 * Library: leveldb-kv-separation_amd/liblvkv_crc32c.so (the same library as
 * lvkv_crc32c.h; return codes LVKV_OK / LVKV_ERR_* from there). Blocks are
 * described by plain device arrays; one call handles a batch of independent
 * blocks on `stream` (a hipStream_t, NULL = the default stream) and returns
 * once the work is enqueued.
 *
 * Format and bytes: Google Snappy's raw format as libsnappy 1.1.8 writes and
 * reads it (the snappy the image carries; the as-built reference has
 * HAVE_SNAPPY=0, port/port_stdcxx.h:90-133). The compressor emits exactly
 * the bytes of snappy::RawCompress 1.1.8; the decompressor accepts exactly
 * the streams snappy::RawUncompress accepts and produces the same bytes.
 * The decoders keep a block in LDS up to the call's max_ulen (at most
 * LVKV_SNAPPY_MAX_BLOCK; LevelDB's blocks are ~block_size, 4 KiB by
 * default); a block past that, of any size (block_size is a user option,
 * include/leveldb/options.h:101), is decoded by a second kernel of the same
 * call straight into its destination, so a valid block never comes back
 * TOO_LARGE from a decoder. The compressor holds the block in LDS and
 * reports a block past its max_len as LVKV_SNAPPY_TOO_LARGE.
 */
#ifndef LVKV_SNAPPY_H_
#define LVKV_SNAPPY_H_

#include <stddef.h>
#include <stdint.h>

#include "lvkv_zstd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* per-block status */
#define LVKV_SNAPPY_OK 0
#define LVKV_SNAPPY_BAD_LENGTH 1   /* Snappy_GetUncompressedLength failed: "corrupted snappy
                                      compressed block length" (table/format.cc:122-124) */
#define LVKV_SNAPPY_BAD_CONTENTS 2 /* Snappy_Uncompress failed: "corrupted snappy compressed
                                      block contents" (table/format.cc:127-131) */
#define LVKV_SNAPPY_CAPACITY 3     /* the block's uncompressed length exceeds d_dst_cap[i]
                                      (out_len says how much it needs) */
#define LVKV_SNAPPY_TOO_LARGE 4    /* compressor: a block longer than max_len; decoders:
                                      only the length-only calls (an unknown or > 32-bit
                                      zstd content size) */

#define LVKV_SNAPPY_MAX_BLOCK 49152u /* largest max_ulen of the decompressor */

/* snappy::MaxCompressedLength: 32 + n + n / 6. */
size_t lvkv_snappy_max_compressed_length(size_t n);

/*
 * Compress block i = d_src[d_src_off[i], + d_src_len[i]) into
 * d_dst[d_dst_off[i], ...) (room for lvkv_snappy_max_compressed_length of
 * its length), d_dst_len[i] = bytes written, d_status[i] = LVKV_SNAPPY_OK or
 * LVKV_SNAPPY_TOO_LARGE (a block longer than max_len; fragments of 64 KiB
 * are compressed alone, so any max_len >= 65536 takes every block).
 * Replaces port::Snappy_Compress (port/port_stdcxx.h:90-106) in
 * TableBuilder::WriteBlock (table/table_builder.cc:158-168); the 12.5% rule
 * that keeps a block raw stays with the caller (it needs both lengths).
 */
int lvkv_snappy_compress_device(const void* d_src, const uint64_t* d_src_off,
                                const uint32_t* d_src_len, void* d_dst,
                                const uint64_t* d_dst_off, uint32_t* d_dst_len,
                                uint8_t* d_status, size_t nblocks, uint32_t max_len,
                                void* stream);

/*
 * Uncompressed lengths: d_ulen[i] = the varint32 preamble of stream i,
 * d_status[i] = LVKV_SNAPPY_OK or LVKV_SNAPPY_BAD_LENGTH. Replaces
 * port::Snappy_GetUncompressedLength (port/port_stdcxx.h:108-119), the
 * first half of ReadBlock's snappy case (table/format.cc:120-125).
 */
int lvkv_snappy_uncompressed_length_device(const void* d_src, const uint64_t* d_src_off,
                                           const uint32_t* d_src_len, uint32_t* d_ulen,
                                           uint8_t* d_status, size_t nblocks, void* stream);

/*
 * Uncompress stream i = d_src[d_src_off[i], + d_src_len[i]) into
 * d_dst[d_dst_off[i], + d_dst_cap[i]): d_out_len[i] = its uncompressed
 * length (when the preamble decodes), d_status[i] = one of the statuses
 * above; on LVKV_SNAPPY_BAD_CONTENTS the destination holds garbage, as
 * after a failed RawUncompress. max_ulen (<= LVKV_SNAPPY_MAX_BLOCK) sizes
 * the LDS staging; a stream past it (a longer block, or one longer than
 * MaxCompressedLength(max_ulen)) is decoded from HBM into HBM by a second
 * kernel on the same stream, with the same verdicts. Replaces
 * port::Snappy_Uncompress (port/port_stdcxx.h:121-133) in ReadBlock
 * (table/format.cc:126-135).
 */
int lvkv_snappy_uncompress_device(const void* d_src, const uint64_t* d_src_off,
                                  const uint32_t* d_src_len, void* d_dst,
                                  const uint64_t* d_dst_off, const uint32_t* d_dst_cap,
                                  uint32_t* d_out_len, uint8_t* d_status, size_t nblocks,
                                  uint32_t max_ulen, void* stream);

/* ---- Zstd: include/lvkv_zstd.h (its entry points moved there in round 6; the
 * LVKV_SNAPPY_* status names stay valid for zstd calls: LVKV_ZSTD_* has the
 * same values) ---------------------------------------------------------- */

/* ---- the block writer and reader around the codec ----------------------- */

/* Scratch for lvkv_sst_write_blocks_device with compression 1 or 2. */
size_t lvkv_sst_write_scratch_bytes(size_t nblocks, uint32_t max_len);

/*
 * TableBuilder::WriteBlock + WriteRawBlock over a batch of finished blocks
 * (table/table_builder.cc:141-209): block i = d_raw[d_raw_off[i], +
 * d_raw_len[i]) (each at most max_len bytes), written in order from file
 * offset `file_offset` of d_file (the image of the file; d_file[0] is file
 * offset 0): with compression 1 (kSnappyCompression) or 2
 * (kZstdCompression, at zstd_compression_level 1) the compressed form when
 * it is smaller than raw - raw/8, else raw with type 0; the type byte; the
 * masked CRC32C of contents + type (the batch CRC kernel). d_handle_off /
 * d_handle_size = the BlockHandles, d_type = the kept type, d_end[0] = the
 * file offset after the last trailer (Rep::offset). compression 0 writes
 * every block raw (no scratch needed). d_file must hold the whole output:
 * at most sum(raw + 5) bytes from file_offset. A block longer than max_len
 * is kept raw (the caller's bound sized the scratch).
 */
int lvkv_sst_write_blocks_device(const void* d_raw, const uint64_t* d_raw_off,
                                 const uint32_t* d_raw_len, size_t nblocks, int compression,
                                 uint32_t max_len, void* d_scratch, void* d_file,
                                 uint64_t file_offset, uint64_t* d_handle_off,
                                 uint32_t* d_handle_size, uint8_t* d_type, uint64_t* d_end,
                                 void* stream);

/*
 * The same with Options::zstd_compression_level (include/leveldb/options.h:
 * 141) for compression 2: levels <= 2 except 0 (ZSTD_fast at every block
 * size the device takes) and max_len <= LVKV_ZSTD_COMPRESS_MAX_BLOCK; other
 * values are LVKV_ERR_INVALID (the host's libzstd path).
 */
int lvkv_sst_write_blocks_level_device(const void* d_raw, const uint64_t* d_raw_off,
                                       const uint32_t* d_raw_len, size_t nblocks, int compression,
                                       int zstd_level, uint32_t max_len, void* d_scratch,
                                       void* d_file, uint64_t file_offset, uint64_t* d_handle_off,
                                       uint32_t* d_handle_size, uint8_t* d_type, uint64_t* d_end,
                                       void* stream);

/*
 * The writer for blocks of any size, with the codec's verdict per block.
 * Semantics of lvkv_sst_write_blocks_level_device, except:
 *  - d_status[i] = the codec's status for block i: LVKV_ZSTD_OK, or
 *    LVKV_ZSTD_TOO_LARGE for a block the device did not compress (written
 *    raw, type 0 -- where TableBuilder::WriteBlock would have compressed it,
 *    so the host has to redo that block if the image is to be the
 *    reference's). With compression 0 every status is OK. A block the
 *    12.5% rule kept raw has status OK.
 *  - compression 1 (snappy): every block compresses whatever its length
 *    (fragments are 64 KiB); max_len is not used.
 *  - compression 2 (zstd): blocks up to min(max_len,
 *    LVKV_ZSTD_COMPRESS_BIG_MAX_BLOCK) compress at levels <= 2 except 0;
 *    longer blocks (frames of several Zstd blocks) are TOO_LARGE. Levels 0
 *    and >= 3 are LVKV_ERR_INVALID.
 *  - nblocks == 0 is handled before every other check: LVKV_OK with d_end[0]
 *    = file_offset, whatever the compression and level.
 *  - the scratch is ragged: block i's compressed form lives at an exclusive
 *    scan (on the device) of max(snappy MaxCompressedLength,
 *    ZSTD_compressBound)(d_raw_len[i]) rounded up to 16, so it grows with the
 *    bytes written and not with nblocks x max_len.
 *    lvkv_sst_write_scratch_bytes_v2(nblocks, total_raw_bytes, max_len) is
 *    enough for any batch of nblocks blocks of total_raw_bytes in all (it
 *    includes the zstd compressor's fixed pool for max_len, which does not
 *    depend on the batch). scratch_bytes = the bytes at d_scratch; a block
 *    whose slot would not fit (the caller's total was too small) is reported
 *    TOO_LARGE and written raw, never past the scratch. A NULL d_scratch or
 *    d_status, or a scratch too small for the fixed part, is
 *    LVKV_ERR_INVALID.
 */
size_t lvkv_sst_write_scratch_bytes_v2(size_t nblocks, uint64_t total_raw_bytes, uint32_t max_len);
int lvkv_sst_write_blocks_status_device(const void* d_raw, const uint64_t* d_raw_off,
                                        const uint32_t* d_raw_len, size_t nblocks, int compression,
                                        int zstd_level, uint32_t max_len, void* d_scratch,
                                        void* d_file, uint64_t file_offset,
                                        uint64_t* d_handle_off, uint32_t* d_handle_size,
                                        uint8_t* d_type, uint64_t* d_end, size_t scratch_bytes,
                                        uint8_t* d_status, void* stream);

/* ---- the whole table: TableBuilder::Finish on the device ------------------- */

#define LVKV_TABLE_OK 0
#define LVKV_TABLE_BAD_BLOCK 1    /* a data block is not a block BlockBuilder::Finish returns:
                                     restart count or offset outside the block, a restart that
                                     is not where an entry starts, a varint or entry past its
                                     run's end, shared longer than the previous key or not 0 at
                                     a restart, no entries, an internal key under 8 bytes */
#define LVKV_TABLE_KEY_TOO_LONG 2 /* a key longer than max_key_len */
#define LVKV_TABLE_CAPACITY 3     /* the image does not fit in file_capacity */

typedef struct lvkv_sst_table_report {
  int32_t status;           /* LVKV_TABLE_* */
  uint32_t first_bad_block; /* for BAD_BLOCK / KEY_TOO_LONG (whose verdict status is), else
                               0xFFFFFFFF */
  uint64_t num_entries;     /* TableBuilder::NumEntries */
  uint32_t nfilters;        /* entries of the filter block's offset array */
  uint8_t meta_type, index_type;     /* block types as written (0/1/2) */
  uint8_t meta_status, index_status; /* codec verdicts, as d_status[] */
  uint64_t data_end;                 /* the first byte after the data blocks */
  uint64_t filter_offset, filter_size; /* 0, 0 without a filter policy */
  uint64_t meta_offset, meta_size, index_offset, index_size;
  uint64_t file_size;                /* TableBuilder::FileSize; 0 unless status is OK */
} lvkv_sst_table_report;

/*
 * Scratch for lvkv_sst_write_table_device: enough for any nblocks blocks of
 * total_raw_bytes in all, whatever the compression (it holds the ragged
 * scratch of lvkv_sst_write_blocks_status_device for the data blocks and for
 * the metaindex and index blocks, one key of max_key_len a block and a lane,
 * and the per-block arrays). The call itself knows no total: it needs at
 * least the value for total_raw_bytes 0, and a data block whose compressed
 * form finds no room is written raw and reported LVKV_ZSTD_TOO_LARGE.
 */
size_t lvkv_sst_write_table_scratch_bytes(size_t nblocks, uint64_t total_raw_bytes,
                                          uint32_t max_len, uint32_t max_key_len,
                                          int filter_bits_per_key);
/* An upper bound of the file: every block raw, every entry 3 bytes. */
uint64_t lvkv_sst_table_file_bound(size_t nblocks, uint64_t total_raw_bytes, uint32_t max_key_len,
                                   int filter_bits_per_key);

/*
 * TableBuilder::Flush per block and TableBuilder::Finish (table/
 * table_builder.cc:104-268) in one stream-ordered call: the data blocks
 * d_raw[d_raw_off[i], + d_raw_len[i]) in key order, each the bytes
 * BlockBuilder::Finish returns, become the whole table image in d_file from
 * offset 0 -- the data blocks as lvkv_sst_write_blocks_status_device writes
 * them (compression, zstd_level, max_len, d_handle_*, d_type, d_status as
 * there), the filter block (table/filter_block.cc; filter_bits_per_key > 0:
 * NewBloomFilterPolicy(bits), 0: no policy, no filter block), the metaindex
 * block, the index block (restart interval 1, separators by
 * FindShortestSeparator / FindShortSuccessor) and the footer. key_format 0:
 * keys are byte strings under BytewiseComparator and the filter hashes whole
 * keys; 1: internal keys under InternalKeyComparator, the filter hashes user
 * keys (InternalFilterPolicy), as db/builder.cc builds tables. The metaindex
 * and index blocks go through the same writer: d_report->meta_status /
 * index_status are its verdicts (an index block past 128 KiB stays raw under
 * zstd and is LVKV_ZSTD_TOO_LARGE; the table is valid and its status OK).
 *
 * No synchronisation, no copy to the host: d_report (device memory) says how
 * it went. On a status other than OK nothing is written at or past d_file +
 * file_capacity, file_size is 0 and the bytes from data_end on are
 * unspecified; the data blocks that fit and the four arrays are as the block
 * writer leaves them. LVKV_ERR_INVALID, before any launch: a null pointer
 * (d_raw, d_raw_off, d_raw_len and the four arrays may be null when nblocks
 * is 0), compression outside 0..2, key_format outside 0..1, zstd level 0 or
 * >= 3 with compression 2, filter_bits_per_key < 0, max_key_len > 2^20,
 * nblocks x (max_key_len + 26) >= 2^32, scratch_bytes under the sizing
 * function's value for total_raw_bytes 0.
 */
int lvkv_sst_write_table_device(const void* d_raw, const uint64_t* d_raw_off,
                                const uint32_t* d_raw_len, size_t nblocks, int compression,
                                int zstd_level, uint32_t max_len, int key_format,
                                int filter_bits_per_key, uint32_t max_key_len, void* d_scratch,
                                size_t scratch_bytes, void* d_file, uint64_t file_capacity,
                                uint64_t* d_handle_off, uint32_t* d_handle_size, uint8_t* d_type,
                                uint8_t* d_status, lvkv_sst_table_report* d_report, void* stream);

/* ---- the data blocks: TableBuilder::Add on the device ----------------------- */

#define LVKV_BUILD_OK 0
#define LVKV_BUILD_UNSORTED 1     /* entry first_bad_entry is not greater than the one before it */
#define LVKV_BUILD_BAD_KEY 2      /* key_format 1 and a key under 8 bytes */
#define LVKV_BUILD_CAPACITY 3     /* more blocks than max_blocks, or more bytes than raw_capacity */
#define LVKV_BUILD_TOO_LARGE 4    /* a block's contents would pass 2^31 - 1 bytes */

typedef struct lvkv_sst_build_report {
  int32_t  status;
  uint32_t first_bad_entry;   /* lowest offending entry for UNSORTED / BAD_KEY, else 0xFFFFFFFF */
  uint32_t nblocks;           /* blocks cut; with CAPACITY: the number that would be needed */
  uint32_t max_block_len;     /* longest block's contents (max_len for the writer) */
  uint32_t max_key_len;       /* longest key (max_key_len for the table writer) */
  uint64_t num_entries;
  uint64_t raw_bytes;         /* end of the last block in d_raw; with CAPACITY: the bytes needed */
} lvkv_sst_build_report;

/* The scratch of lvkv_sst_build_blocks_device, and an upper bound of what it
 * writes to d_raw whatever the entries are (5-byte varints, a restart per
 * entry, a block per entry with 15 bytes of padding). Both never decrease
 * when an argument grows. */
size_t   lvkv_sst_build_blocks_scratch_bytes(size_t nentries, uint32_t restart_interval);
uint64_t lvkv_sst_build_blocks_raw_bound(size_t nentries, uint64_t total_key_bytes,
                                         uint64_t total_value_bytes, uint32_t restart_interval);

/*
 * TableBuilder::Add over sorted entries, then the Flush() that Finish() begins
 * with (table/table_builder.cc:94-123, 213-215), in one stream-ordered call:
 * entry i has key d_keys[d_key_off[i], + d_key_len[i]) and value
 * d_vals[d_val_off[i], + d_val_len[i]) (the two buffers may be one). Out come
 * the data blocks BlockBuilder::Add + Finish build (table/block_builder.cc:
 * shared is the byte-wise common prefix with the previous key of the same
 * block, 0 at entries whose index in the block is a multiple of
 * restart_interval), cut after the entry with which the block's
 * CurrentSizeEstimate() reaches block_size (>=; block_size 0: an entry a
 * block). Block b's contents are d_raw[d_raw_off[b], + d_raw_len[b]);
 * d_raw_off[0] = 0 and d_raw_off[b] = the end of block b - 1 rounded up to 16
 * (the bytes between blocks are not written): the first three arguments of
 * lvkv_sst_write_table_device.
 *
 * Order: key_format 0, each key byte-wise greater than the one before it; 1,
 * greater under InternalKeyComparator (db/dbformat.cc:47-63: user key
 * ascending, then the trailing 8 bytes as a little-endian u64 descending),
 * and every key 8 bytes or longer.
 *
 * No synchronisation, no copy to the host: d_report (device memory) says how
 * it went. On a status other than OK nothing at all is written to d_raw,
 * d_raw_off or d_raw_len (the layout is known before the first byte is
 * copied), and never anything at or past d_raw + raw_capacity, d_raw_off +
 * max_blocks or d_raw_len + max_blocks. BAD_KEY is reported before UNSORTED,
 * those before TOO_LARGE, that before CAPACITY; first_bad_entry is the lowest
 * entry of the reported kind. With BAD_KEY and UNSORTED nblocks,
 * max_block_len and raw_bytes are 0; with CAPACITY they are what the call
 * needs, so that it can be repeated; max_key_len and num_entries always hold.
 *
 * nentries == 0, before every other check: LVKV_OK, and a report of no blocks
 * where d_report is not null (every pointer may be null). LVKV_ERR_INVALID,
 * before any launch: a null pointer, restart_interval 0, key_format outside
 * 0..1, nentries >= 2^31, scratch_bytes under the sizing function's value.
 */
int lvkv_sst_build_blocks_device(
    const void* d_keys, const uint64_t* d_key_off, const uint32_t* d_key_len,
    const void* d_vals, const uint64_t* d_val_off, const uint32_t* d_val_len,
    size_t nentries, uint32_t block_size, uint32_t restart_interval, int key_format,
    void* d_scratch, size_t scratch_bytes,
    void* d_raw, uint64_t raw_capacity,
    uint64_t* d_raw_off, uint32_t* d_raw_len, size_t max_blocks,
    lvkv_sst_build_report* d_report, void* stream);

/* ---- the entries of decoded data blocks: Block::Iter's walk on the device ---- */

/* per block (d_block_status) */
#define LVKV_ENTRIES_OK 0
#define LVKV_ENTRIES_BAD_BLOCK 1   /* "bad block contents" (table/block.cc:25-40, 281-284) */
#define LVKV_ENTRIES_BAD_ENTRY 2   /* "bad entry in block" (table/block.cc:243-249) */
#define LVKV_ENTRIES_SKIPPED 3     /* d_skip[b] != 0: not walked */
/* report.status */
#define LVKV_ENTRIES_CAPACITY 1    /* more entries than max_entries or more key bytes than
                                      key_capacity */

typedef struct lvkv_sst_entries_report {
  int32_t  status;          /* 0, or LVKV_ENTRIES_CAPACITY */
  uint32_t nbad;            /* blocks with BAD_BLOCK or BAD_ENTRY */
  uint32_t first_bad_block; /* lowest such block, else 0xFFFFFFFF */
  uint32_t max_key_len;
  uint64_t num_entries;     /* with CAPACITY: the number needed */
  uint64_t key_bytes;       /* end of the last key in d_keys; with CAPACITY: the bytes needed */
  uint64_t value_bytes;     /* sum of the value lengths */
} lvkv_sst_entries_report;

/* The scratch of lvkv_sst_read_entries_device for nblocks blocks of
 * total_raw_bytes in all; it never decreases when an argument grows. The call
 * itself knows no total: it needs at least the value for total_raw_bytes 0,
 * and a block whose restart runs find no room in a smaller scratch than the
 * batch's total asks for is walked by one lane (slower, the same result). */
size_t lvkv_sst_read_entries_scratch_bytes(size_t nblocks, uint64_t total_raw_bytes);

/*
 * The inverse of lvkv_sst_build_blocks_device, in one stream-ordered call:
 * the decoded data blocks d_raw[d_raw_off[b], + d_raw_len[b]) -- the d_out,
 * d_out_off and d_out_len of lvkv_sst_read_blocks_device; d_skip (may be
 * null) is that call's d_status, and a block with d_skip[b] != 0 is SKIPPED
 * and not read -- become the entries Block::NewIterator + SeekToFirst + Next
 * until !Valid() hand out (table/block.cc:77-279), block after block, in the
 * layout the build call takes. Entries d_block_first[b] .. d_block_first[b +
 * 1] are block b's. Key i is the restored key (shared prefix + delta) at
 * d_keys[d_key_off[i], + d_key_len[i]); d_key_off[0] = 0 and d_key_off[i] =
 * the end of key i - 1 rounded up to 8 (the bytes between keys are not
 * written). Values are not copied: d_val_off[i] is the value's offset in
 * d_raw, which the caller passes as the build's d_vals.
 *
 * The verdicts are the walk's and nothing stricter. A block under 4 bytes or
 * with a restart count above (len - 4) / 4 is BAD_BLOCK and has no entries; a
 * restart count of 0 is OK with no entries (NewEmptyIterator). The walk
 * starts at restart[0], which need not be 0 and may lie at or past the
 * entries' end (OK, no entries), and never looks at restart[1..]: restart
 * arrays that lie change nothing. An entry DecodeEntry refuses (fewer than 3
 * bytes before the restart array, a varint that runs out or is too long, a
 * delta and value that pass the restart array) or whose shared exceeds the
 * previous key's length ends the walk with BAD_ENTRY; the entries before it
 * are emitted.
 *
 * One deliberate difference: DecodeEntry adds non_shared + value_length in 32
 * bits (table/block.cc:71), and a sum that wraps lets the reference read far
 * outside the block. Here the sum is taken in 64 bits and the entry is
 * BAD_ENTRY.
 *
 * No synchronisation, no copy to the host: d_report (device memory) says how
 * it went. d_block_first, d_block_status and the report are always written.
 * With LVKV_ENTRIES_CAPACITY nothing is written to d_keys or the four entry
 * arrays (the counts are known before the first byte is copied) and
 * num_entries and key_bytes are what a repeat needs; never anything at or
 * past d_keys + key_capacity or slot max_entries of the arrays.
 *
 * nblocks == 0, before every other check: LVKV_OK, and a report of no entries
 * where d_report is not null (every pointer may be null). LVKV_ERR_INVALID,
 * before any launch: a null pointer other than d_skip, nblocks >= 2^31,
 * scratch_bytes under the sizing function's value for total_raw_bytes 0.
 */
int lvkv_sst_read_entries_device(
    const void* d_raw, const uint64_t* d_raw_off, const uint32_t* d_raw_len,
    const uint8_t* d_skip /* may be null */, size_t nblocks,
    void* d_scratch, size_t scratch_bytes,
    void* d_keys, uint64_t key_capacity, uint64_t* d_key_off, uint32_t* d_key_len,
    uint64_t* d_val_off, uint32_t* d_val_len, size_t max_entries,
    uint64_t* d_block_first /* nblocks + 1 */, uint8_t* d_block_status,
    lvkv_sst_entries_report* d_report, void* stream);

/* ---- merging sorted runs of entries: MergingIterator and compaction's drops ---- */

#define LVKV_MERGE_OK 0
#define LVKV_MERGE_UNSORTED 1     /* entry first_bad_entry is not greater than the one before it
                                     in its run */
#define LVKV_MERGE_BAD_KEY 2      /* key_format 1 and a key under 8 bytes */
#define LVKV_MERGE_CAPACITY 3     /* more survivors than max_out */
#define LVKV_MERGE_BAD_RUNS 4     /* d_run_first does not go from 0 to nentries without descending */

#define LVKV_MERGE_MAX_RUNS 64
#define LVKV_MERGE_COMPACT 1u     /* flags: apply DoCompactionWork's drops (key_format 1 only) */

typedef struct lvkv_sst_merge_report {
  int32_t  status;
  uint32_t first_bad_entry;   /* lowest offending input entry for UNSORTED / BAD_KEY, else
                                 0xFFFFFFFF */
  uint32_t num_in;            /* nentries */
  uint32_t num_out;           /* survivors; with CAPACITY: the max_out a repeat needs */
  uint32_t num_hidden;        /* dropped: hidden by a newer entry of the same user key */
  uint32_t num_obsolete;      /* dropped: deletions nothing needs any more */
  uint32_t max_key_len;       /* longest input key */
  uint32_t reserved_;         /* 0 */
  uint64_t key_bytes;         /* sum of the survivors' key lengths */
  uint64_t value_bytes;       /* sum of the survivors' value lengths */
} lvkv_sst_merge_report;

/* The scratch of lvkv_sst_merge_entries_device; it never decreases when an
 * argument grows. */
size_t lvkv_sst_merge_entries_scratch_bytes(size_t nentries, uint32_t nruns);

/*
 * What a compaction does between lvkv_sst_read_entries_device and
 * lvkv_sst_build_blocks_device, in one stream-ordered call. The six entry
 * arrays are the build call's, and hold nruns sorted runs laid end to end:
 * run r is entries [d_run_first[r], d_run_first[r + 1]) (d_run_first: u64
 * [nruns + 1] in device memory, d_run_first[0] = 0, never descending, the
 * last word nentries -- anything else is LVKV_MERGE_BAD_RUNS; empty runs are
 * legal anywhere). Inside a run every key is greater than the one before it,
 * under the build call's comparators: key_format 0 byte-wise, 1
 * InternalKeyComparator (db/dbformat.cc:47-63) with every key 8 bytes or
 * longer. A level's files laid end to end are one run.
 *
 * The order is MergingIterator's forward walk (table/merger.cc:150-163): the
 * smallest key of the runs' heads comes next, among equal keys the run of
 * the lowest index. Equal keys in different runs are legal and all come out.
 *
 * The drops, only with LVKV_MERGE_COMPACT in flags (key_format 1): the loop of
 * DBImpl::DoCompactionWork (db/db_impl.cc:1022-1055) over that order. With
 * last = the sequence of the entry directly before in merged order where that
 * entry parses (type byte <= 1) and has the same user key -- dropped itself or
 * not -- and kMaxSequenceNumber otherwise: a key that does not parse is never
 * dropped; an entry is hidden when last <= smallest_snapshot; a deletion that
 * is not hidden is obsolete when its sequence is <= smallest_snapshot and its
 * user key lies in none of the n_deeper ranges [smallest, largest] of user
 * keys, bounds included, byte-wise (Compaction::IsBaseLevelForKey,
 * db/version_set.cc:1518-1537: the files of levels level + 2 and deeper, in
 * any order, overlapping or not). Range g is d_deeper_keys[d_deeper_off[2g],
 * + d_deeper_len[2g]) .. d_deeper_keys[d_deeper_off[2g + 1], + d_deeper_len[2g
 * + 1]). As in the reference, a smallest_snapshot of kMaxSequenceNumber (2^56
 * - 1) or more hides every entry that parses, a user key's first included.
 *
 * No key or value byte is copied. Survivor j, in merged order, is input entry
 * d_out_src[j], and d_out_key_off / d_out_key_len / d_out_val_off /
 * d_out_val_len [j] are that entry's own descriptors into d_keys and d_vals:
 * with those two buffers they are the build call's arguments. d_dropped_src
 * (u32 [nentries], may be null) lists the dropped entries' input indices in
 * merged order, num_hidden + num_obsolete of them (what a caller that keeps
 * values elsewhere marks invalid, db/db_impl.cc:1126-1135).
 *
 * No synchronisation, no copy to the host: d_report (device memory) says how
 * it went. BAD_RUNS is reported before BAD_KEY, that before UNSORTED, that
 * before CAPACITY; first_bad_entry is the lowest entry of the reported kind (a
 * pair that descends across a run boundary is no error). On a status other
 * than OK nothing at all is written to the five output arrays or to
 * d_dropped_src (the order and the counts are known before the first word is
 * stored), and never anything at or past slot max_out. num_in always holds;
 * max_key_len with every status but BAD_RUNS; the counts and sums with OK and
 * CAPACITY, and are 0 otherwise.
 *
 * nentries == 0, before every other check: LVKV_OK, and a report of no
 * entries where d_report is not null (every pointer may be null).
 * LVKV_ERR_INVALID, before any launch: a null pointer other than
 * d_dropped_src (and the three d_deeper arrays when n_deeper is 0), nruns
 * outside 1..LVKV_MERGE_MAX_RUNS, key_format outside 0..1, a flag other than
 * LVKV_MERGE_COMPACT, LVKV_MERGE_COMPACT with key_format 0, nentries or
 * n_deeper >= 2^31, scratch_bytes under the sizing function's value.
 */
int lvkv_sst_merge_entries_device(
    const void* d_keys, const uint64_t* d_key_off, const uint32_t* d_key_len,
    const void* d_vals, const uint64_t* d_val_off, const uint32_t* d_val_len, size_t nentries,
    const uint64_t* d_run_first /* nruns + 1 */, uint32_t nruns, int key_format, uint32_t flags,
    uint64_t smallest_snapshot,
    const void* d_deeper_keys, const uint64_t* d_deeper_off, const uint32_t* d_deeper_len,
    size_t n_deeper,
    void* d_scratch, size_t scratch_bytes,
    uint64_t* d_out_key_off, uint32_t* d_out_key_len, uint64_t* d_out_val_off,
    uint32_t* d_out_val_len, uint32_t* d_out_src, size_t max_out,
    uint32_t* d_dropped_src /* nentries, may be null */,
    lvkv_sst_merge_report* d_report, void* stream);

/* ---- point lookups: Table::InternalGet for a batch of keys ---- */

/* per query, lvkv_sst_get_locate_device (d_q_status) */
#define LVKV_GET_BLOCK 0          /* read this block and seek in it */
#define LVKV_GET_PAST_END 1       /* !iiter->Valid(), status OK: no block can hold the key */
#define LVKV_GET_FILTERED 2       /* the filter said no */
#define LVKV_GET_INDEX_CORRUPT 3  /* "bad entry in block" from the index iterator, or an index
                                     block no iterator can be made for */
#define LVKV_GET_BAD_HANDLE 4     /* the index entry's value is no BlockHandle (or its size does
                                     not fit 32 bits); the filter is not asked */
#define LVKV_GET_BAD_KEY 5        /* key_format 1 and a query under 8 bytes */
#define LVKV_GET_NSTATUS 6
/* per query, lvkv_sst_get_seek_device (d_state) */
#define LVKV_GET_STATE_NOT_FOUND 0
#define LVKV_GET_STATE_FOUND 1
#define LVKV_GET_STATE_DELETED 2
#define LVKV_GET_STATE_CORRUPT_KEY 3  /* ParseInternalKey fails on the entry (kCorrupt) */
#define LVKV_GET_STATE_BAD_BLOCK 4    /* "bad block contents": under 4 bytes, or the restart
                                         count too large */
#define LVKV_GET_STATE_BAD_ENTRY 5    /* "bad entry in block" during the seek */
#define LVKV_GET_STATE_UNREADABLE 6   /* d_skip says so, or d_q_slot is at or past nblocks */
#define LVKV_GET_STATE_BAD_KEY 7      /* key_format 1 and a query under 8 bytes (before the slot is
                                         looked at) */
#define LVKV_GET_NSTATE 8

typedef struct lvkv_sst_get_locate_report {
  uint32_t nqueries;
  uint32_t count[LVKV_GET_NSTATUS];  /* queries with each LVKV_GET_* status */
  uint32_t reserved_;                /* 0 */
} lvkv_sst_get_locate_report;

typedef struct lvkv_sst_get_seek_report {
  uint32_t nqueries;
  uint32_t count[LVKV_GET_NSTATE];   /* queries with each LVKV_GET_STATE_* */
} lvkv_sst_get_seek_report;

/* The scratch of lvkv_sst_get_locate_device for nqueries queries on an index
 * block of index_len bytes, and of lvkv_sst_get_seek_device for nqueries
 * queries (the counts a workgroup of queries leaves for the report); neither
 * decreases when an argument grows. */
size_t lvkv_sst_get_locate_scratch_bytes(uint32_t index_len, size_t nqueries);
size_t lvkv_sst_get_seek_scratch_bytes(size_t nqueries);

/*
 * The first half of Table::InternalGet (table/table.cc:214-227) for nqueries
 * keys, in one stream-ordered call: iiter->Seek(k) on the decoded index block
 * d_index[0, index_len), BlockHandle::DecodeFrom on the entry it stops at, and
 * filter->KeyMayMatch(handle.offset(), k) on the decoded filter block
 * d_filter[0, filter_len) (d_filter NULL: no filter policy, nothing is
 * filtered). Query q is d_qkeys[d_qkey_off[q], + d_qkey_len[q]), the build
 * call's key layout: key_format 1, internal keys as LookupKey::internal_key()
 * makes them (user key, then (sequence << 8) | kValueTypeForSeek as 8
 * little-endian bytes) under InternalKeyComparator; 0, plain keys under
 * BytewiseComparator.
 *
 * Seek is Block::Iter::Seek on a fresh iterator (table/block.cc:165-228), step
 * for step: the bisection over the restart array as it stands with mid =
 * (left + right + 1) / 2, a restart entry that does not decode (an offset
 * within 3 bytes of the restart array or past it included) or has shared != 0
 * being corrupt; then SeekToRestartPoint(left) and ParseNextKey until the key
 * is not below the query, where an offset at or past the restart array is a
 * clean end and shared above the previous key's length is corrupt. A block
 * under 4 bytes or with too large a restart count is INDEX_CORRUPT, one with
 * no restarts PAST_END (NewEmptyIterator).
 *
 * The filter is FilterBlockReader as written (table/filter_block.cc:77-104):
 * under 5 bytes or last_word > n - 5, everything may match; else index =
 * offset >> base_lg, an empty filter (start == limit) says no, any other
 * inconsistency yes; BloomFilterPolicy::KeyMayMatch (util/bloom.cc:56-80) on
 * the user key under key_format 1 (InternalFilterPolicy), on the whole key
 * under 0: a filter under 2 bytes says no, k > 30 yes. A base_lg of 64 or
 * more (an undefined shift there) gives index 0.
 *
 * Per query: d_q_status[q] = LVKV_GET_*; d_q_block[q] = the number of entries
 * SeekToFirst + Next hand out before the entry the seek stopped at
 * (0xFFFFFFFF where that walk does not come by it, as with a lying restart
 * array, and whenever the seek stopped at none); d_q_handle_off[q] and
 * d_q_handle_size[q] = the BlockHandle with BLOCK and FILTERED, else 0.
 *
 * Differences from the reference, both on purpose. Under key_format 1
 * InternalKeyComparator reads 8 bytes before the end of any key it is given:
 * here a query under 8 bytes is BAD_KEY, and a restart key or a walked key
 * under 8 bytes is INDEX_CORRUPT. DecodeEntry's non_shared + value_length is
 * taken in 64 bits, as lvkv_sst_read_entries_device does.
 *
 * No synchronisation, no copy to the host: d_report (device memory) holds
 * the count of each status. Nothing is written at or past slot nqueries.
 *
 * nqueries == 0, before every other check: LVKV_OK, and an empty report where
 * d_report is not null (every pointer may be null). LVKV_ERR_INVALID, before
 * any launch: a null pointer other than d_filter, nqueries >= 2^31,
 * key_format outside 0..1, scratch_bytes under the sizing function's value.
 */
int lvkv_sst_get_locate_device(
    const void* d_index, uint32_t index_len,
    const void* d_filter /* may be null */, uint32_t filter_len,
    const void* d_qkeys, const uint64_t* d_qkey_off, const uint32_t* d_qkey_len, size_t nqueries,
    int key_format, void* d_scratch, size_t scratch_bytes,
    uint32_t* d_q_block, uint64_t* d_q_handle_off, uint32_t* d_q_handle_size, uint8_t* d_q_status,
    lvkv_sst_get_locate_report* d_report, void* stream);

/*
 * The second half (table/table.cc:228-235): block_iter->Seek(k) in one decoded
 * data block a query, and SaveValue (db/version_set.cc:263-276) on the entry
 * it stops at. The blocks are d_raw[d_raw_off[b], + d_raw_len[b]) for b <
 * nblocks -- lvkv_sst_read_blocks_device's d_out, d_out_off and d_out_len;
 * d_skip (may be null) is that call's d_status, a non-zero byte meaning the
 * block could not be read. d_q_slot[q] picks query q's block: the caller's
 * mapping from the locate call's d_q_block to where it decoded that block, so
 * that only the blocks a batch touches need decoding. 0xFFFFFFFF: no block,
 * NOT_FOUND; any other slot at or past nblocks: UNREADABLE, and no block is
 * read for it. The queries and key_format are the locate call's.
 *
 * The seek is the locate call's, and never moves on to the next block: a
 * walk that reaches the restart array is NOT_FOUND, as in InternalGet; so is
 * a restart count of 0. Per query: d_hit_off[q] = the offset in its block of
 * the entry the seek stopped at, 0xFFFFFFFF when it stopped at none;
 * d_val_off[q] (into d_raw) and d_val_len[q] = that entry's value, 0 when
 * none -- values are not copied, and a value that is a kVTableIndex record
 * stays bytes for the caller to resolve; d_tag[q] = the last 8 bytes of the
 * entry's key as a little-endian u64 under key_format 1, else 0; d_state[q] =
 * LVKV_GET_STATE_*. Under key_format 1, FOUND and DELETED are SaveValue's:
 * the entry's key parses (type byte <= 1, else CORRUPT_KEY), its user key
 * equals the query's byte-wise, and the type decides; an entry with another
 * user key leaves NOT_FOUND with d_hit_off, the value and the tag describing
 * it. Under key_format 0, FOUND: the entry's key equals the query.
 *
 * Keys of any length are compared exactly. The same two differences from the
 * reference: a query under 8 bytes (key_format 1) is BAD_KEY, before its slot
 * is looked at; a restart key or walked key under 8 bytes is BAD_ENTRY.
 *
 * No synchronisation, no copy to the host: d_report (device memory) holds
 * the count of each state. Nothing is written at or past slot nqueries.
 *
 * nqueries == 0, before every other check: LVKV_OK, and an empty report where
 * d_report is not null (every pointer may be null). LVKV_ERR_INVALID, before
 * any launch: a null pointer other than d_skip, nqueries or nblocks >= 2^31,
 * key_format outside 0..1, scratch_bytes under the sizing function's value.
 */
int lvkv_sst_get_seek_device(
    const void* d_raw, const uint64_t* d_raw_off, const uint32_t* d_raw_len,
    const uint8_t* d_skip /* may be null */, size_t nblocks,
    const void* d_qkeys, const uint64_t* d_qkey_off, const uint32_t* d_qkey_len,
    const uint32_t* d_q_slot, size_t nqueries, int key_format,
    void* d_scratch, size_t scratch_bytes,
    uint32_t* d_hit_off, uint64_t* d_val_off, uint32_t* d_val_len, uint64_t* d_tag,
    uint8_t* d_state, lvkv_sst_get_seek_report* d_report, void* stream);

/* ReadBlock verdicts */
#define LVKV_READ_OK 0
#define LVKV_READ_CHECKSUM 1        /* "block checksum mismatch" (table/format.cc:95-98) */
#define LVKV_READ_BAD_TYPE 2        /* "bad block type" (:156-158) */
#define LVKV_READ_SNAPPY_LENGTH 3   /* "corrupted snappy compressed block length" (:122-124) */
#define LVKV_READ_SNAPPY_CONTENTS 4 /* "corrupted snappy compressed block contents" (:127-131) */
#define LVKV_READ_ZSTD_LENGTH 5     /* "corrupted zstd compressed block length" (:140-143) */
#define LVKV_READ_CAPACITY 6        /* contents longer than d_out_cap[i] (d_out_len says) */
#define LVKV_READ_TOO_LARGE 7       /* (no longer returned: blocks past max_ulen are
                                       decoded from HBM; kept for the numbering) */
#define LVKV_READ_ZSTD_CONTENTS 8   /* "corrupted zstd compressed block contents" (:145-149) */

/*
 * ReadBlock over a batch of block handles of one file image
 * (table/format.cc:69-162): the CRC of contents + type checked against the
 * trailer (verify != 0, ReadOptions::verify_checksums), then by type:
 * kNoCompression copies the contents, kSnappyCompression and
 * kZstdCompression decode them, into d_out[d_out_off[i], + d_out_cap[i]);
 * d_out_len[i] = the block's length, d_status[i] = LVKV_READ_*. Handles
 * must lie inside the file (as for lvkv_sst_verify_device; Table::Open's
 * index decode checks that).
 */
int lvkv_sst_read_blocks_device(const void* d_file, const uint64_t* d_handle_off,
                                const uint32_t* d_handle_size, size_t nblocks, int verify,
                                void* d_out, const uint64_t* d_out_off, const uint32_t* d_out_cap,
                                uint32_t* d_out_len, uint8_t* d_status, uint32_t max_ulen,
                                void* stream);

#ifdef __cplusplus
}
#endif

#endif /* LVKV_SNAPPY_H_ */
