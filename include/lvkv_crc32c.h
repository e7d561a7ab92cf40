/*
 * lvkv_crc32c.h — C-ABI of the MI355X batched CRC32C engine for
 * ArcueidType/LevelDB-KV-Separation (reference snapshot at /root/reference).
 *
 * Library: leveldb-kv-separation_amd/liblvkv_crc32c.so (built by
 * __graft_entry__.build()). Plain pointers and sizes only; no C++ or torch
 * types cross this boundary. Every function is reentrant; device state is
 * initialised once per device on first use. Nothing here throws or aborts:
 * failures are negative return codes (see lvkv_strerror).
 *
 * Which reference interface each entry replaces is cited per declaration.
 * The C++ symbol leveldb::crc32c::Extend (util/crc32c.h:17) is exported by the
 * same library; see INTEGRATION.md for the link recipe and FFI stubs.
 */
#ifndef LVKV_CRC32C_H_
#define LVKV_CRC32C_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- return codes ---------------------------------------------------- */
#define LVKV_OK 0
#define LVKV_ERR_INVALID (-1)   /* null pointer / bad argument            */
#define LVKV_ERR_NO_DEVICE (-2) /* no HIP device (the batch API never falls
                                   back to the CPU)                        */
#define LVKV_ERR_HIP (-3)       /* HIP runtime error; see lvkv_last_hip_error */
#define LVKV_ERR_RANGE (-4)     /* a block longer than 4 GiB - 1           */

/* ---- flags ------------------------------------------------------------ */
/* Store crc32c::Mask(crc) instead of crc (util/crc32c.h:29-32): the value
 * TableBuilder::WriteRawBlock / log::Writer put on disk. */
#define LVKV_FLAG_MASK 1u
/* Engine submits only: the batch runs alone — it starts after every earlier
 * dispatch of the engine has completed (host drain of the other queues + AQL
 * barrier bit), a batch of several dispatches puts all of them on one queue
 * with the barrier bit (they run one after another, never side by side), and
 * it uses the kernel shaped for the whole chip. Later submits are not held
 * back by it. Without the flag, consecutive batches (and the dispatches of
 * one large batch) overlap, each on half of every CU. */
#define LVKV_FLAG_ORDERED 2u
/* Engine submits only: the batch's first dispatch acquires at system scope
 * (invalidates the L2) instead of agent scope. Needed when the input was
 * written by a copy engine or the host since the device last read that
 * memory (hipMemcpy into a reused buffer); inputs written by kernels on this
 * device do not need it. Costs about 2.5 us per submission. */
#define LVKV_FLAG_SYSTEM_ACQUIRE 4u

/* Engine submits only: a wait will follow soon. The batch's last dispatch
 * starts after every earlier one of its queue and, when it completes,
 * releases its results at system scope into a completion signal, so the next
 * lvkv_engine_wait needs no barrier packet on that queue (the packet
 * processor's barrier costs several microseconds after the last kernel). Give
 * it to the last submit on each queue before a wait: with the default three
 * queues, the last three submits. Any mix is correct; other queues are fenced
 * as before. Ignored while profiling. */
#define LVKV_FLAG_FINAL 8u

/* Engine ragged submits only (lvkv_engine_crc32c_batch): the blocks are
 * mostly small (under ~2 KiB, e.g. log::Writer's records, db/log_writer.cc:
 * 82-108). The engine cannot see the lengths (device memory) and otherwise
 * picks the walk shaped for SST-sized blocks; with the hint it takes the
 * small-block walk (62,000 records of 0-2000 B: 0.29 of 8 TB/s overlapped
 * against 0.21). Results are the same either way. */
#define LVKV_FLAG_SMALL_BLOCKS 16u

/* ---- per-call, host CPU: the drop-in for the reference's own symbols ---- */

/* Replaces leveldb::crc32c::Extend (util/crc32c.h:17, util/crc32c.cc:276).
 * CRC32C of A||data[0,n) given init_crc = CRC32C(A). Runs on the host CPU
 * (SSE4.2 crc32 or portable slicing-by-8): one synchronous buffer per call is
 * latency-bound, so a GPU round trip would lose. */
uint32_t lvkv_crc32c_extend(uint32_t init_crc, const char* data, size_t n);
/* Replaces leveldb::crc32c::Value (util/crc32c.h:20). */
uint32_t lvkv_crc32c_value(const char* data, size_t n);
/* Replace leveldb::crc32c::Mask / Unmask (util/crc32c.h:29-38). */
uint32_t lvkv_crc32c_mask(uint32_t crc);
uint32_t lvkv_crc32c_unmask(uint32_t masked_crc);

/* ---- batched, device-resident (the GPU hot path) ---------------------- */
/* All d_* pointers are device memory of the CURRENT HIP device; `stream` is a
 * hipStream_t (NULL = the null stream). Calls are asynchronous on `stream`;
 * results are valid after the stream is synchronised. No allocation or
 * synchronisation happens inside, so the calls are graph-capturable after
 * the first call on a device (which uploads the tables). */

/* Batched leveldb::crc32c::Extend (util/crc32c.cc:276) over block i =
 * d_base[d_offsets[i], d_offsets[i] + d_lengths[i]) with init
 * d_init ? d_init[i] : init. Any offset alignment and length (0..4 GiB-1).
 * d_out[i] = CRC (or Mask(CRC) with LVKV_FLAG_MASK). This is the loop of
 * TableBuilder::WriteRawBlock (table/table_builder.cc:199-203) and
 * log::Writer::EmitPhysicalRecord (db/log_writer.cc:94-95) run for many
 * blocks in one launch. */
int lvkv_crc32c_batch_device(const void* d_base, const uint64_t* d_offsets,
                             const uint32_t* d_lengths, const uint32_t* d_init,
                             uint32_t init, uint32_t* d_out, size_t nblocks,
                             uint32_t flags, void* stream);

/* Same, for nblocks blocks of `length` bytes at d_base + i*stride (no
 * descriptor arrays; the benchmark's 10k x 4 KiB layout). */
int lvkv_crc32c_uniform_device(const void* d_base, uint64_t stride,
                               uint32_t length, uint32_t init, uint32_t* d_out,
                               size_t nblocks, uint32_t flags, void* stream);

/* ---- the AQL engine: batches dispatched into a per-device hardware queue --
 * Same kernels and results as the calls above, without the HIP launch path:
 * a submit writes AQL dispatch packets into the engine's own queue (well
 * under a microsecond of host time, against 2.7-7 us for a hipLaunchKernel)
 * and consecutive dispatches may overlap on the device (no barrier bit
 * unless LVKV_FLAG_ORDERED). This is the checksum-service form of the batch
 * loop that compaction (table_builder.cc:199-203) and recovery
 * (log_reader.cc:243-257) would run.
 * Engine dispatches are NOT ordered with HIP streams: synchronise the stream
 * that produced the input before submitting; results (and outputs reused by
 * a later submit) are safe after lvkv_engine_wait. One engine per device;
 * calls on one engine are serialised internally (thread-safe). */
typedef struct lvkv_engine lvkv_engine;
/* device = HIP device ordinal. */
int lvkv_engine_create(int device, lvkv_engine** out);
/* Waits for outstanding work, then frees the queue. NULL is a no-op. */
void lvkv_engine_destroy(lvkv_engine* engine);
/* lvkv_crc32c_uniform_device's contract, asynchronous on the engine, for any
 * length, stride and alignment and any nblocks (batches beyond one
 * dispatch's capacity become several dispatches). Blocks of 4..4096 bytes
 * (at most 16 rows of 256 B on the word grid aligned to the block's end)
 * whose ends are 4-byte aligned ((d_base + length) % 4 == 0, stride % 4 ==
 * 0) — the headline's 4 KiB blocks — run the burst kernel; other shapes
 * (over 4096 bytes, 32 KiB WAL blocks at +6, unaligned ends) the general walk
 * of lvkv_engine_crc32c_batch in its uniform layout. */
int lvkv_engine_crc32c_uniform(lvkv_engine* engine, const void* d_base, uint64_t stride,
                               uint32_t length, uint32_t init, uint32_t* d_out,
                               size_t nblocks, uint32_t flags);
/* The engine form of lvkv_crc32c_batch_device (util/crc32c.cc:276 over block i
 * = d_base[d_offsets[i], + d_lengths[i]), init d_init ? d_init[i] : init;
 * TableBuilder::WriteRawBlock's table_builder.cc:199-203 and
 * log::Writer::EmitPhysicalRecord's log_writer.cc:94-95 as a batch): any
 * offsets, lengths and alignment; blocks over 64 KiB are walked by a whole
 * workgroup inside the same dispatch. Asynchronous; results after
 * lvkv_engine_wait. */
int lvkv_engine_crc32c_batch(lvkv_engine* engine, const void* d_base, const uint64_t* d_offsets,
                             const uint32_t* d_lengths, const uint32_t* d_init, uint32_t init,
                             uint32_t* d_out, size_t nblocks, uint32_t flags);
/* The engine forms of lvkv_sst_verify_device (ReadBlock's checksum test,
 * table/format.cc:92-99), lvkv_log_verify_device (ReadPhysicalRecord's,
 * db/log_reader.cc:243-247), lvkv_sst_fill_trailers_device
 * (table/table_builder.cc:192-209) and lvkv_log_fill_headers_device
 * (db/log_writer.cc:82-108): same arguments and outputs, dispatched into the
 * engine's queues (flags: LVKV_FLAG_ORDERED / LVKV_FLAG_SYSTEM_ACQUIRE as for
 * the other submits). The compaction and recovery loops as a checksum
 * service. */
int lvkv_engine_sst_verify(lvkv_engine* engine, const void* d_file, const uint64_t* d_offsets,
                           const uint32_t* d_sizes, uint32_t* d_actual, uint8_t* d_status,
                           size_t nblocks, uint32_t flags);
int lvkv_engine_log_verify(lvkv_engine* engine, const void* d_file,
                           const uint64_t* d_hdr_offsets, uint32_t* d_actual,
                           uint8_t* d_status, size_t nrecords, uint32_t flags);
int lvkv_engine_sst_fill_trailers(lvkv_engine* engine, void* d_file, const uint64_t* d_offsets,
                                  const uint32_t* d_sizes, uint32_t* d_crc, size_t nblocks,
                                  uint32_t flags);
int lvkv_engine_log_fill_headers(lvkv_engine* engine, void* d_file,
                                 const uint64_t* d_hdr_offsets, uint32_t* d_crc,
                                 size_t nrecords, uint32_t flags);
/* Blocks until every dispatch submitted so far has completed and its results
 * are visible to the host and other devices (a barrier packet on every queue,
 * system-scope release, host spin-wait). */
int lvkv_engine_wait(lvkv_engine* engine);
/* Hardware queues the dispatches rotate over (1..4; default 3); 0 queries. */
int lvkv_engine_queues(lvkv_engine* engine, int nqueues);
/* Kernel shape: waves and chains per workgroup, workgroups per dispatch. */
int lvkv_engine_shape(lvkv_engine* engine, uint32_t* waves, uint32_t* chains,
                      uint32_t* groups);
/* Per-dispatch timing (the engine's HIP-event counterpart): with profiling on,
 * every dispatch carries a completion signal and the packet processor's start
 * and end times of it are logged (HSA system clock, us); _read copies those
 * of the most recent dispatches (up to n, in submission order), returns how
 * many and clears the log. */
int lvkv_engine_profile(lvkv_engine* engine, int enable);
long lvkv_engine_profile_read(lvkv_engine* engine, double* start_us, double* end_us,
                              size_t n);

/* Batched leveldb::ReadBlock checksum test (table/format.cc:92-99): block i
 * is the BlockHandle {d_offsets[i], d_sizes[i]} of an SST image at d_file;
 * the CRC covers contents + type byte (size+1 bytes) and is compared with
 * Unmask(DecodeFixed32(trailer+1)). d_actual[i] = computed CRC (unmasked),
 * d_status[i] = 0 on match, 1 on "block checksum mismatch". */
int lvkv_sst_verify_device(const void* d_file, const uint64_t* d_offsets,
                           const uint32_t* d_sizes, uint32_t* d_actual,
                           uint8_t* d_status, size_t nblocks, void* stream);

/* Batched log::Reader::ReadPhysicalRecord checksum test
 * (db/log_reader.cc:217-247): record i has its 7-byte header at
 * d_file + d_hdr_offsets[i]; the length is parsed on the device from header
 * bytes 4..5, the CRC covers type byte + payload and is compared with
 * Unmask(DecodeFixed32(header)). The caller guarantees header and payload
 * are inside the image (the reader's "bad record length" check, :225-236). */
int lvkv_log_verify_device(const void* d_file, const uint64_t* d_hdr_offsets,
                           uint32_t* d_actual, uint8_t* d_status,
                           size_t nrecords, void* stream);

/* ---- write side: batched trailer / header emission */
/* TableBuilder::WriteRawBlock's checksum (table/table_builder.cc:192-209) for
 * many finished blocks at once: block i occupies d_file[d_offsets[i],
 * + d_sizes[i]) followed by its 5-byte trailer whose type byte (byte 0) the
 * caller has written; writes Mask(CRC32C(contents + type)) little-endian into
 * trailer bytes 1..4. d_crc (nullable) receives the unmasked CRCs. Blocks
 * must not overlap each other's trailers. */
int lvkv_sst_fill_trailers_device(void* d_file, const uint64_t* d_offsets,
                                  const uint32_t* d_sizes, uint32_t* d_crc, size_t nblocks,
                                  void* stream);

/* log::Writer::EmitPhysicalRecord's checksum (db/log_writer.cc:82-108) for many
 * records: record i has its 7-byte header at d_file + d_hdr_offsets[i] with
 * the length (bytes 4..5) and type (byte 6) written and its payload after it;
 * writes Mask(CRC32C(type + payload)) into header bytes 0..3. */
int lvkv_log_fill_headers_device(void* d_file, const uint64_t* d_hdr_offsets, uint32_t* d_crc,
                                 size_t nrecords, void* stream);

/* ---- whole-SSTable verify, device-resident ------- */
/* report.status: what Table::Open / ReadBlock would return for the table. */
#define LVKV_SST_OK 0
#define LVKV_SST_TOO_SHORT 1       /* "file is too short to be an sstable" (table/table.cc:41) */
#define LVKV_SST_BAD_MAGIC 2       /* "not an sstable (bad magic number)" (table/format.cc:54) */
#define LVKV_SST_BAD_HANDLE 3      /* "bad block handle" in the footer (table/format.cc:28) */
#define LVKV_SST_INDEX_TRUNCATED 4 /* "truncated block read" of the index (table/format.cc:86) */
#define LVKV_SST_INDEX_CHECKSUM 5  /* "block checksum mismatch" on the index (table/format.cc:96) */
#define LVKV_SST_INDEX_TYPE 6      /* index block compressed (no codec on this path) or
                                      "bad block type" (table/format.cc:157) */
#define LVKV_SST_INDEX_CORRUPT 7   /* restart array or an entry unusable (table/block.cc:25-75) */
#define LVKV_SST_CAPACITY 8        /* more blocks than the caller's arrays hold (ndata says
                                      how many data blocks the index lists) */
/* Longest FilterPolicy::Name() the verify calls accept. */
#define LVKV_SST_MAX_POLICY_NAME 64
/* Per-block status (d_status). */
#define LVKV_BLOCK_OK 0
#define LVKV_BLOCK_CHECKSUM 1      /* "block checksum mismatch" (table/format.cc:96) */
#define LVKV_BLOCK_TRUNCATED 2     /* "truncated block read": handle past the file (:86) */
#define LVKV_BLOCK_BAD_TYPE 3      /* "bad block type": type byte not 0/1/2 (:157) */
#define LVKV_BLOCK_BAD_HANDLE 4    /* index entry value is not a BlockHandle (:28) */
#define LVKV_BLOCK_BAD_ENTRY 5     /* "bad entry in block" for the index entry (block.cc:236) */
#define LVKV_BLOCK_COMPRESSED 6    /* CRC good, type 1/2 (snappy/zstd): the as-built reference has
                                      no codec (HAVE_SNAPPY=0, HAVE_ZSTD=0) and returns "corrupted
                                      snappy|zstd compressed block length" (format.cc:120-141,
                                      port/port_stdcxx.h:108-118) */
#define LVKV_BLOCK_NOT_READ 7      /* index/metaindex: the footer did not decode, never read */

/* Written by lvkv_sst_verify_table(s)_device into device memory. */
typedef struct lvkv_sst_report {
  int32_t status;          /* LVKV_SST_* */
  uint32_t nblocks;        /* entries written to the per-block arrays: ndata + has_filter
                              (0 with LVKV_SST_CAPACITY) */
  uint32_t ndata;          /* data blocks the index lists (0 when its restart array is
                              unusable, LVKV_SST_INDEX_CORRUPT) */
  uint32_t has_filter;     /* 1: the last entry is the filter block, found under the exact
                              key "filter." + filter_policy (Table::ReadMeta) */
  uint32_t nbad;           /* entries with status != LVKV_BLOCK_OK */
  uint32_t first_bad;      /* lowest such entry (relative to `first`), or 0xffffffff */
  uint32_t index_crc;      /* computed CRC (contents + type byte) of the index block */
  uint32_t meta_crc;       /* same, metaindex block */
  uint8_t index_status;    /* LVKV_BLOCK_* of the index block */
  uint8_t meta_status;     /* LVKV_BLOCK_* of the metaindex (Table::ReadMeta ignores its
                              errors, table/table.cc:92-94; reported, not fatal) */
  uint8_t reserved0_[2];
  uint32_t first;          /* this table's first entry in the shared per-block arrays */
  uint64_t index_offset, index_size, meta_offset, meta_size;  /* footer handles */
  /* library-internal */
  uint64_t link_;          /* multi-table placement: (call generation << 32) | entries */
  uint32_t total_;         /* tables[0] only: entries verified over all tables */
  uint32_t done_;           /* fused form: the call's tag once this table's entries are out */
} lvkv_sst_report;

/* Verifies a whole SSTable image already in device memory, as Table::Open
 * (table/table.cc:38-79) with paranoid_checks + Table::ReadMeta (:81-124) +
 * ReadBlock on every block (table/format.cc:69-160) would with
 * verify_checksums: footer and magic, index and metaindex checksums and type
 * bytes, then every data block the index lists and the filter block, all on
 * the device: for a table up to 32 MiB one launch (a workgroup for the
 * footer, index and metaindex CRCs, the filter lookup and the placement,
 * while the other workgroups each decode a share of the index entries, one
 * entry per restart point as table_builder.cc:35 writes it, and checksum
 * their blocks), else two launches (three when the index is wide, its CRC
 * and entries then spread over 64 workgroups). filter_policy = FilterPolicy::Name() of the reader's
 * Options (e.g. "leveldb.BuiltinBloomFilter2" for NewBloomFilterPolicy,
 * util/bloom.cc): the filter block is the metaindex entry whose key is
 * exactly "filter." + filter_policy (table.cc:100-102); NULL = no policy
 * (Options::filter_policy == nullptr: no filter block, table.cc:82-84). Per-block outputs
 * (arrays of `capacity` entries, device memory), in index order, then the
 * filter block: d_offsets/d_sizes = the BlockHandle (0/0 for an entry that is
 * not a readable handle), d_actual = computed CRC of contents + type byte (0
 * when not computed), d_status = LVKV_BLOCK_*. index_status / meta_status are
 * ReadBlock's verdicts on those two blocks whenever the footer decoded
 * (LVKV_BLOCK_NOT_READ otherwise). Asynchronous on `stream` and
 * graph-capturable (no host synchronisation; counts live in *d_report).
 * Returns LVKV_OK when the work was enqueued (LVKV_ERR_INVALID for a policy
 * name longer than LVKV_SST_MAX_POLICY_NAME); the table's verdict is
 * d_report->status. */
int lvkv_sst_verify_table_device(const void* d_file, uint64_t file_size,
                                 uint64_t* d_offsets, uint32_t* d_sizes,
                                 uint32_t* d_actual, uint8_t* d_status, size_t capacity,
                                 const char* filter_policy, lvkv_sst_report* d_report,
                                 void* stream);

/* Many SSTables at once: compaction inputs (paranoid checks), a repair scan.
 * Table t is d_file[d_table_off[t], + d_table_size[t]) (device arrays). One
 * launch serves up to half as many tables as the device has CUs (a head
 * workgroup per table, the CRC workgroups shared out by table size), two
 * launches more; table t's entries go to the shared per-block arrays from
 * d_reports[t].first on, in table order. d_offsets are offsets into d_file
 * (table offset + BlockHandle offset). A table whose entries do not fit in
 * `capacity` gets LVKV_SST_CAPACITY (with ndata set); so do the tables after
 * it. Asynchronous; graph-capturable. */
int lvkv_sst_verify_tables_device(const void* d_file, const uint64_t* d_table_off,
                                  const uint64_t* d_table_size, size_t ntables,
                                  uint64_t* d_offsets, uint32_t* d_sizes, uint32_t* d_actual,
                                  uint8_t* d_status, size_t capacity, const char* filter_policy,
                                  lvkv_sst_report* d_reports, void* stream);

/* ---- WAL / MANIFEST verify, device-resident ----- */
#define LVKV_LOG_CAPACITY 1        /* report.status: more records than `capacity` */
/* Per physical record (d_rec_status). */
#define LVKV_REC_OK 0              /* returned by ReadPhysicalRecord */
#define LVKV_REC_CHECKSUM 1        /* "checksum mismatch" (db/log_reader.cc:243-255) */
#define LVKV_REC_DROPPED 2         /* after a mismatch in the same block: never read */
/* Per 32 KiB block (d_block_status). */
#define LVKV_LOGBLK_OK 0
#define LVKV_LOGBLK_CHECKSUM 1     /* reported, drop = bytes from that header to block end */
#define LVKV_LOGBLK_BAD_LENGTH 2   /* "bad record length", reported (:221-232) */
#define LVKV_LOGBLK_ZERO 3         /* zero-type zero-length record: rest skipped, silent (:234-240) */
#define LVKV_LOGBLK_EOF 4          /* truncated record or header at the end of the file: kEof */

typedef struct lvkv_log_report {
  int32_t status;            /* LVKV_OK or LVKV_LOG_CAPACITY */
  uint32_t nblocks;          /* ceil(file_size / 32768) */
  uint32_t nrecords;         /* candidate physical records (d_hdr_offsets entries) */
  uint32_t ngood;            /* records the reader returns */
  uint32_t ncorrupt;         /* Reporter::Corruption calls */
  uint32_t first_bad_block;  /* lowest block with a reported corruption, or 0xffffffff */
  uint64_t dropped_bytes;    /* sum of the reported drop sizes */
  uint32_t count_;           /* library-internal */
  uint32_t reserved_;
} lvkv_log_report;

/* Verifies every physical record of a log image in device memory, as
 * log::Reader(checksum = true) reading from offset 0 would (ReadPhysicalRecord,
 * db/log_reader.cc:189-271): the image is cut into 32 KiB blocks
 * (db/log_format.h), each block's headers are walked on the device, all
 * candidate records are checksummed in one batched launch, and a mismatch
 * drops the rest of its block. Outputs: d_hdr_offsets / d_actual (CRC of type
 * + payload) / d_rec_status for up to `capacity` candidates in file order;
 * d_block_status / d_block_drop for ceil(file_size / 32768) blocks; totals in
 * *d_report. Asynchronous on `stream`, no host synchronisation. */
int lvkv_log_verify_blocks_device(const void* d_file, uint64_t file_size,
                                  uint64_t* d_hdr_offsets, uint32_t* d_actual,
                                  uint8_t* d_rec_status, size_t capacity,
                                  uint8_t* d_block_status, uint32_t* d_block_drop,
                                  lvkv_log_report* d_report, void* stream);

/* ---- WAL / MANIFEST logical records (log::Reader::ReadRecord) --------- */
/* Reporter::Corruption reasons, physical and logical (lvkv_log_corruption). */
#define LVKV_LOGR_CHECKSUM 1       /* "checksum mismatch" (db/log_reader.cc:243-255) */
#define LVKV_LOGR_BAD_LENGTH 2     /* "bad record length" (:221-232) */
#define LVKV_LOGR_PARTIAL_1 3      /* "partial record without end(1)" (:86-98) */
#define LVKV_LOGR_PARTIAL_2 4      /* "partial record without end(2)" (:100-112) */
#define LVKV_LOGR_MISSING_1 5      /* "missing start of fragmented record(1)" (:114-121) */
#define LVKV_LOGR_MISSING_2 6      /* "missing start of fragmented record(2)" (:123-134) */
#define LVKV_LOGR_MIDDLE 7         /* "error in middle of record" (:145-151) */
#define LVKV_LOGR_UNKNOWN_TYPE 8   /* "unknown record type %u" (:153-162), type in .type */

typedef struct lvkv_log_record {
  uint64_t offset;   /* LastRecordOffset(): header offset of its first fragment */
  uint64_t length;   /* bytes of the record: its fragments' payloads, in order */
  uint32_t first;    /* its first fragment, an index into d_hdr_offsets */
  uint32_t nfrags;   /* its fragments are d_hdr_offsets[first .. first + nfrags) */
} lvkv_log_record;

typedef struct lvkv_log_corruption {
  uint64_t bytes;    /* Reporter::Corruption's bytes argument */
  uint32_t reason;   /* LVKV_LOGR_* */
  uint32_t type;     /* LVKV_LOGR_UNKNOWN_TYPE: the header's type byte; else 0 */
} lvkv_log_corruption;

typedef struct lvkv_log_read_report {
  int32_t status;    /* LVKV_OK, or LVKV_LOG_CAPACITY: the physical records did not fit
                        `capacity` (nothing assembled), or the records / reports exceed
                        their capacities (the counts stay exact, the arrays hold the first) */
  uint32_t nrecords; /* logical records ReadRecord returns, in order */
  uint32_t nreports; /* Reporter::Corruption calls, in order */
  uint32_t stopped;  /* 1: a header whose type byte is kEof (5) ended ReadRecord early */
  uint64_t bytes;    /* total bytes of the returned records */
} lvkv_log_read_report;

/* log::Reader(reporter, checksum = true, initial_offset) over a whole log
 * image in device memory: ReadRecord until it returns false
 * (db/log_reader.cc:55-176 over ReadPhysicalRecord :189-271). Runs
 * lvkv_log_verify_blocks_device (same physical outputs, same meaning) and then
 * the logical layer on the device: FULL records, FIRST MIDDLE* LAST
 * assembly, and every Reporter::Corruption call in the reader's order (the
 * physical "checksum mismatch" / "bad record length" drops, "partial record
 * without end", "missing start of fragmented record", "error in middle of
 * record", "unknown record type"). d_records[i] locates logical record i
 * (its fragments are consecutive physical records); d_reports[i] is the
 * i-th Reporter call. initial_offset as log::Reader's (db/log_reader.cc:29-54,
 * :80-89, :182-187, :261-266): reading starts at the block that can hold it,
 * records that start before it are skipped, MIDDLE fragments and one LAST at
 * the start are skipped (resync), and reports of bytes before it are not
 * made; the physical outputs still cover the whole image. Asynchronous on
 * `stream`, no host synchronisation; totals in *d_read. */
int lvkv_log_read_device(const void* d_file, uint64_t file_size, uint64_t* d_hdr_offsets,
                         uint32_t* d_actual, uint8_t* d_rec_status, size_t capacity,
                         uint8_t* d_block_status, uint32_t* d_block_drop,
                         lvkv_log_report* d_report, lvkv_log_record* d_records,
                         size_t record_capacity, lvkv_log_corruption* d_reports,
                         size_t report_capacity, uint64_t initial_offset,
                         lvkv_log_read_report* d_read, void* stream);

/* The records' bytes after lvkv_log_read_device, as ReadRecord hands each
 * one back (scratch->assign / append of its fragments' payloads, then
 * *record = Slice(*scratch): db/log_reader.cc:92-137), laid end to end in
 * record order: record i's contents are d_payload[d_record_pos[i],
 * + d_records[i].length). This is the buffer DBImpl::RecoverLogFile
 * (db/db_impl.cc:453) and VersionSet::Recover (db/version_set.cc:910) would
 * feed to WriteBatchInternal::SetContents / VersionEdit::DecodeFrom, one
 * record at a time. Same d_file / d_hdr_offsets / capacity / d_report /
 * d_records / record_capacity / d_read as that call (enqueue on the same
 * stream after it). payload_capacity >= d_read->bytes is needed for every
 * record to be written (file_size always suffices); a fragment that does
 * not fit is skipped. d_record_pos (record_capacity u64, nullable) gets
 * every returned record's offset in d_payload. Four launches, asynchronous. */
int lvkv_log_gather_device(const void* d_file, const uint64_t* d_hdr_offsets, size_t capacity,
                           const lvkv_log_report* d_report, const lvkv_log_record* d_records,
                           size_t record_capacity, const lvkv_log_read_report* d_read,
                           void* d_payload, uint64_t payload_capacity, uint64_t* d_record_pos,
                           void* stream);

/* ---- batched, host-resident (end-to-end incl. PCIe) ------------------- */
/* Blocks live in host memory (pageable or pinned). The library packs them
 * into pinned staging buffers, copies them to the current device with
 * hipMemcpyAsync in double-buffered chunks, runs the batch kernel and copies
 * the CRCs back. Synchronous: returns when h_out is filled. This is the
 * shape of a caller that reads blocks with pread (table/format.cc:78-80). */
int lvkv_crc32c_batch_host(const void* h_base, const uint64_t* offsets,
                           const uint32_t* lengths, const uint32_t* init_arr,
                           uint32_t init, uint32_t* h_out, size_t nblocks,
                           uint32_t flags);

/* ---- diagnostics ------------------------------------------------------ */
const char* lvkv_strerror(int code);
int lvkv_last_hip_error(void);      /* hipError_t of the last LVKV_ERR_HIP */
const char* lvkv_cpu_impl(void);    /* "sse4.2" or "portable-slice8"      */
/* Number of workgroups (one per CU) the batch kernel launches on the current
 * device, or a negative error code. */
int lvkv_device_groups(void);

#ifdef __cplusplus
}
#endif

#endif /* LVKV_CRC32C_H_ */
