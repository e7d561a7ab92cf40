/* The memtable on the device: the logical records of a WAL, as
 * lvkv_log_gather_device leaves them end to end in device memory, become the
 * sorted entries a flush builds its table from.
 *
 *   lvkv_memtable_from_batches_device  the loop of DBImpl::RecoverLogFile
 *       (db/db_impl.cc:453-488) around WriteBatch::Iterate (db/write_batch.cc:42-80),
 *       MemTableInserter / MemTable::Add (db/write_batch.cc:116-137,
 *       db/memtable.cc:77-101) and the memtable's iteration order under
 *       InternalKeyComparator (db/dbformat.cc:47-63).
 *
 * Its outputs are the six arrays lvkv_vtable_separate_device,
 * lvkv_sst_build_blocks_device and lvkv_sst_write_table_device take.
 *
 * Stream-ordered: no synchronisation, no copy to the host, every result in
 * device memory (return codes LVKV_OK / LVKV_ERR_* from lvkv_crc32c.h).
 * Nothing is ever written at or past a capacity. The sizing function never
 * decreases when an argument grows.
 *
 * NOT BUILT:
 *   - where the reference ends one memtable and begins the next:
 *     mem->ApproximateMemoryUsage() > write_buffer_size (db/db_impl.cc:476) is
 *     the arena's block count, which depends on the skiplist's random node
 *     heights. The caller says which batches make one memtable;
 *   - MemTable::Get;
 *   - the live write path (DBImpl::Write's group commit).
 */
#ifndef LVKV_MEMTABLE_H_
#define LVKV_MEMTABLE_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* d_batch_status[b], and lvkv_memtable_report.status */
#define LVKV_MEMTABLE_OK 0
#define LVKV_MEMTABLE_TOO_SMALL 1    /* under 12 bytes: "log record too small"
                                        (db/db_impl.cc:454-457); the batch is skipped */
#define LVKV_MEMTABLE_UNKNOWN_TAG 2  /* "unknown WriteBatch tag" */
#define LVKV_MEMTABLE_BAD_PUT 3      /* "bad WriteBatch Put" */
#define LVKV_MEMTABLE_BAD_DELETE 4   /* "bad WriteBatch Delete" */
#define LVKV_MEMTABLE_WRONG_COUNT 5  /* "WriteBatch has wrong count" */
/* the whole call's alone, in this precedence after a paranoid batch status */
#define LVKV_MEMTABLE_KEY_TOO_LONG 6 /* a user key of 2^32 - 8 bytes or more, whose internal
                                        key d_key_len cannot hold. DELIBERATE DIFFERENCE: the
                                        reference truncates the length in EncodeVarint32
                                        (db/memtable.cc:88). Decided at the entry, before its
                                        bytes are skipped; the batch's walk ends there and
                                        d_batch_status[b] says so too. */
#define LVKV_MEMTABLE_CAPACITY 7     /* more entries than max_entries or more key bytes than
                                        key_capacity; nentries and key_bytes say what a repeat
                                        needs */
#define LVKV_MEMTABLE_DUPLICATE 8    /* two inserted entries with equal internal keys.
                                        DELIBERATE DIFFERENCE: SkipList::Insert asserts there
                                        (db/skiplist.h:338), and TableBuilder::Add would. */
#define LVKV_MEMTABLE_NONE 0xFFFFFFFFu /* first_bad_batch / first_bad_entry: none */

/* flags */
#define LVKV_MEMTABLE_PARANOID 1u /* options.paranoid_checks: the first batch in log order
                                     that is not OK ends the recovery */

typedef struct lvkv_memtable_report {
  int32_t status;            /* LVKV_MEMTABLE_* */
  uint32_t first_bad_batch;  /* PARANOID: the lowest batch that is not OK; KEY_TOO_LONG: the
                                lowest batch with such a key; else LVKV_MEMTABLE_NONE */
  uint32_t first_bad_entry;  /* DUPLICATE: the lowest log-order index whose key equals an
                                earlier entry's (the insertion the assert fires on) */
  uint32_t nentries;         /* entries inserted, over every batch walked */
  uint64_t key_bytes;        /* their internal keys' bytes: what d_keys has to hold */
  uint64_t val_bytes;        /* their values' bytes */
  uint32_t max_key_len;      /* the longest internal key */
  uint32_t n_too_small;      /* batches under 12 bytes */
  uint64_t too_small_bytes;  /* and their bytes: what Reporter::Corruption was told */
  uint64_t max_sequence_out;
  uint32_t n_bad_batches;    /* batches with UNKNOWN_TAG, BAD_PUT, BAD_DELETE, WRONG_COUNT
                                or KEY_TOO_LONG */
  uint32_t reserved_;
} lvkv_memtable_report;

/* The scratch of lvkv_memtable_from_batches_device. */
size_t lvkv_memtable_scratch_bytes(size_t nbatches, size_t max_entries);

/* Batch b is d_payload[d_batch_off[b] .. + d_batch_len[b]), in log order:
 * lvkv_log_gather_device's buffer, its d_record_pos, and the `length` column
 * of its lvkv_log_record. No byte outside a batch's range is read for it.
 *
 * Per batch, WriteBatch::Iterate: under 12 bytes TOO_SMALL (skipped);
 * otherwise sequence = fixed64 at 0, count = fixed32 at 8, then records until
 * the input is empty: tag 1 = a length-prefixed key and value, tag 0 = a key,
 * any other tag UNKNOWN_TAG, a slice that fails BAD_PUT / BAD_DELETE; after
 * the last record found != (int)count is WRONG_COUNT. Varints decode as
 * GetVarint32 does (up to five bytes, non-canonical forms accepted, bits past
 * 32 dropped as there); a length must not exceed the bytes left in the batch.
 *
 * Entry j of a batch is inserted as it is met: its internal key is the user
 * key followed by fixed64 ((sequence + j) << 8) | tag in wrapping arithmetic;
 * its value is the bytes as they lie in d_payload, first byte included (a
 * deletion: length 0, placed at the byte after its key). Entries met before a
 * failing record stay inserted, and so do all of a WRONG_COUNT batch's.
 *
 * Without LVKV_MEMTABLE_PARANOID every batch is walked, the per-batch statuses
 * are recorded and the call's status stays OK (MaybeIgnoreError). With it the
 * lowest batch that is not OK gives the report's status and first_bad_batch,
 * and no entry comes out. The log reader's own corruption reports stop a
 * paranoid recovery as well: those are lvkv_log_read_report.nreports and stay
 * the caller's to look at. max_sequence_out starts from max_sequence_in and
 * is raised by sequence + (int)count - 1 (the int sign-extended, wrapping) of
 * every batch of 12 bytes or more; with PARANOID, of the batches before the
 * first bad one.
 *
 * Outputs, for status OK: the inserted entries in the memtable's iteration
 * order (user key ascending as unsigned bytes, a shorter key before its
 * extensions; then the 8-byte trailer descending). d_keys[0, key_bytes): the
 * internal keys packed end to end in LOG order (batch order, then entry
 * order). For sorted position i: d_key_off[i] / d_key_len[i] into d_keys,
 * d_val_off[i] / d_val_len[i] into d_payload (no value byte is copied),
 * d_src[i] the entry's log-order index. nentries == 0 with status OK is legal
 * (BuildTable then writes no file). On any other status d_keys and the five
 * per-entry arrays are untouched. d_batch_status[b] (u8) and
 * d_batch_entries[b] (entries inserted), either may be null, are written for
 * every batch whatever the status.
 *
 * nbatches == 0, before every other check: LVKV_OK, and an empty report
 * (max_sequence_out = max_sequence_in) where d_report is not null.
 * LVKV_ERR_INVALID, before any launch: a null pointer other than
 * d_batch_status / d_batch_entries, nbatches or max_entries >= 2^31,
 * scratch_bytes under lvkv_memtable_scratch_bytes. */
int lvkv_memtable_from_batches_device(
    const void* d_payload, const uint64_t* d_batch_off, const uint64_t* d_batch_len,
    size_t nbatches, uint64_t max_sequence_in, uint32_t flags, void* d_scratch,
    size_t scratch_bytes, void* d_keys, uint64_t key_capacity, uint64_t* d_key_off,
    uint32_t* d_key_len, uint64_t* d_val_off, uint32_t* d_val_len, uint32_t* d_src,
    size_t max_entries, uint8_t* d_batch_status, uint32_t* d_batch_entries,
    lvkv_memtable_report* d_report, void* stream);

/* Measurement only (tools/memtable_bench.py): the sort tile of the calls that
 * follow, 512 / 1024 / 2048 pairs, 0 for the production choice. */
int lvkv_debug_set_memtable_tile(int pairs);

#ifdef __cplusplus
}
#endif

#endif /* LVKV_MEMTABLE_H_ */
