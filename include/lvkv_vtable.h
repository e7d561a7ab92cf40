/* KV separation on the device: the value log ("vTable") of LevelDB-KV-Separation,
 * written where a flush builds its table and followed where a Get ends.
 *
 *   lvkv_vtable_separate_device  BuildTable's loop (db/builder.cc:47-74): values of
 *                                kv_sep_size bytes and more become VTableRecords of a
 *                                vTable image (table/vtable_builder.cc:11-25,
 *                                table/vtable_format.cc:22-44) and a VTableIndex
 *                                (:72-76) takes their place in the table;
 *   lvkv_vtable_resolve_device   DBImpl::DecodeValue (db/db_impl.cc:1245-1289) and
 *                                VTableReader::Get (table/vtable_reader.cc:17-45) for a
 *                                batch of values: where each value's bytes are;
 *   lvkv_vtable_gather_device    the resolved values end to end, as a multi-get
 *                                hands them back.
 *
 * All three are stream-ordered: no synchronisation, no copy to the host, every
 * result in device memory (return codes LVKV_OK / LVKV_ERR_* from
 * lvkv_crc32c.h). Nothing is ever written at or past a capacity. A sizing
 * function never decreases when an argument grows.
 */
#ifndef LVKV_VTABLE_H_
#define LVKV_VTABLE_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* lvkv_vtable_separate_report.status, lvkv_vtable_gather_report.status */
#define LVKV_VTABLE_OK 0
#define LVKV_VTABLE_BAD_KEY 1    /* a moved entry whose key ParseInternalKey refuses: under 8
                                    bytes, or a type byte above 1 (db/builder.cc:55-61,
                                    db/dbformat.h ParseInternalKey). Entries that stay are not
                                    parsed, as there. */
#define LVKV_VTABLE_BAD_VALUE 2  /* a moved entry with an empty value (kv_sep_size 0 only).
                                    DELIBERATE DIFFERENCE: value.remove_prefix(1)
                                    (db/builder.cc:62) is undefined on it there. */
#define LVKV_VTABLE_TOO_LARGE 3  /* user key + stripped value reach 2^32 - 1 bytes:
                                    RecordEncoder::Encode's assert (table/vtable_format.cc:41) */
#define LVKV_VTABLE_CAPACITY 4   /* an image does not fit its capacity; the report holds the
                                    sizes a repeat of the call needs */
#define LVKV_VTABLE_NO_ENTRY 0xFFFFFFFFu /* first_bad_entry where no entry is at fault */

#define LVKV_VTABLE_RECORD_FRAMING 14u /* fixed32 + two 5-byte varint32 */
#define LVKV_VTABLE_INDEX_MAX 31u      /* the type byte + three 10-byte varint64 */

typedef struct lvkv_vtable_separate_report {
  int32_t status;            /* LVKV_VTABLE_*: the lowest offending entry decides, and at it
                                the first check of the reference's order (BAD_KEY, BAD_VALUE,
                                TOO_LARGE); CAPACITY where no entry is at fault */
  uint32_t first_bad_entry;  /* LVKV_VTABLE_NO_ENTRY for OK and CAPACITY */
  uint64_t records_num;      /* VTableMeta::records_num (db/builder.cc:103) */
  uint64_t table_size;       /* VTableMeta::table_size (:102): the vTable image's bytes */
  uint64_t out_val_bytes;    /* the output values' bytes */
  uint32_t max_out_val_len;
  uint32_t reserved_;
  /* BAD_KEY, BAD_VALUE, TOO_LARGE: the four sizes are 0. */
} lvkv_vtable_separate_report;

/* The scratch of lvkv_vtable_separate_device for nentries entries. */
size_t lvkv_vtable_separate_scratch_bytes(size_t nentries);
/* Capacities that hold either image whatever kv_sep_size is: the keys' and
 * values' bytes and LVKV_VTABLE_RECORD_FRAMING a record for the vTable;
 * max(val_len, LVKV_VTABLE_INDEX_MAX) an output value (at most the values'
 * bytes and LVKV_VTABLE_INDEX_MAX an entry). */
uint64_t lvkv_vtable_separate_vtb_bound(size_t nentries, uint64_t total_key_bytes,
                                        uint64_t total_value_bytes);
uint64_t lvkv_vtable_separate_vals_bound(size_t nentries, uint64_t total_value_bytes);

/* BuildTable's loop (db/builder.cc:47-74) over the entries of
 * lvkv_sst_build_blocks_device: entry i is d_keys[d_key_off[i] .. + d_key_len[i])
 * (an internal key) -> d_vals[d_val_off[i] .. + d_val_len[i]).
 *
 * For every entry with d_val_len[i] >= kv_sep_size, in entry order,
 * d_vtb[0, table_size) gets what VTableBuilder::Add appends
 * (table/vtable_builder.cc:11-25): a fixed32 record length, then
 * VTableRecord::Encode (table/vtable_format.cc:22-25): varint32 user-key
 * length, the user key (the key without its last 8 bytes), varint32 value
 * length, the value without its first byte (db/builder.cc:62, whatever that
 * byte is). No padding between records.
 *
 * d_out_vals[d_out_val_off[i] .. + d_out_val_len[i]) is entry i's value as the
 * table gets it, packed end to end in entry order: the input value, copied,
 * for an entry that stays; VTableIndex::Encode (table/vtable_format.cc:72-76,
 * 60-63) for one that moved: byte 1, varint64 file_number, varint64 offset,
 * varint64 size, size = 4 + the record's bytes (RecordEncoder::GetEncodedSize).
 * With the key arrays these are lvkv_sst_build_blocks_device's arguments.
 * d_rec_off[i], d_rec_size[i] (either may be null): the VTableHandle of entry
 * i's record, 0 / 0 for an entry that stays.
 *
 * When the report's status is not LVKV_VTABLE_OK nothing is written to either
 * image or to the four per-entry arrays.
 *
 * nentries == 0, before every other check: LVKV_OK, and an empty report where
 * d_report is not null (every pointer may be null). LVKV_ERR_INVALID, before
 * any launch: a null pointer other than d_rec_off / d_rec_size,
 * nentries >= 2^31, scratch_bytes under lvkv_vtable_separate_scratch_bytes. */
int lvkv_vtable_separate_device(
    const void* d_keys, const uint64_t* d_key_off, const uint32_t* d_key_len, const void* d_vals,
    const uint64_t* d_val_off, const uint32_t* d_val_len, size_t nentries, uint64_t kv_sep_size,
    uint64_t file_number, void* d_scratch, size_t scratch_bytes, void* d_vtb,
    uint64_t vtb_capacity, void* d_out_vals, uint64_t out_val_capacity, uint64_t* d_out_val_off,
    uint32_t* d_out_val_len, uint64_t* d_rec_off, uint64_t* d_rec_size,
    lvkv_vtable_separate_report* d_report, void* stream);

/* per query, lvkv_vtable_resolve_device (d_status) */
#define LVKV_VRES_OK 0             /* type 2: the input without its first byte; type 1: the
                                      record's value */
#define LVKV_VRES_SKIPPED 1        /* d_state[q] is not LVKV_GET_STATE_FOUND: not looked at */
#define LVKV_VRES_EMPTY 2          /* "Fatal Value Error" (db/db_impl.cc:1253-1255) */
#define LVKV_VRES_BAD_TYPE 3       /* "Unsupported value type" (:1287) */
#define LVKV_VRES_BAD_INDEX 4      /* "Error decode VTableIndex" (table/vtable_format.cc:80-83) */
#define LVKV_VRES_BAD_HANDLE 5     /* "Error decode VTableHandle" (:65-70, 85-88) */
#define LVKV_VRES_NO_FILE 6        /* no image with that number: VTableReader::Open fails */
#define LVKV_VRES_PAST_END 7       /* offset + size, taken without wrap, passes the file. ONE
                                      STATUS for the reference's two: an IO error through mmap, a
                                      short read's Corruption through pread
                                      (table/vtable_reader.cc:23-35). */
#define LVKV_VRES_BAD_HEADER 8     /* size < 4: "Error decode record header" */
#define LVKV_VRES_BAD_RECORD 9     /* "Error decode VTableRecord" within record_size_ bytes */
#define LVKV_VRES_TRAILING 10      /* DecodeSrcIntoObj leaves bytes (table/vtable_format.h:101-108) */
#define LVKV_VRES_RECORD_OVERRUN 11 /* record_size_ > size - 4. DELIBERATE DIFFERENCE: the
                                      reference builds a Slice past its buffer there
                                      (table/vtable_format.cc:54); here it is refused. */
#define LVKV_VRES_NSTATUS 12

typedef struct lvkv_vtable_resolve_report {
  uint32_t nqueries;
  uint32_t count[LVKV_VRES_NSTATUS]; /* queries with each LVKV_VRES_* status */
  uint32_t max_len;                  /* the longest d_out_len of an OK query */
  uint64_t total_len;                /* the sum of d_out_len over the OK queries */
} lvkv_vtable_resolve_report;

size_t lvkv_vtable_resolve_scratch_bytes(size_t nqueries);

/* DecodeValue for a batch: value q is d_vals[d_val_off[q] .. + d_val_len[q])
 * (lvkv_sst_get_seek_device's outputs over its decoded blocks). d_state (may be
 * null): that call's d_state; only LVKV_GET_STATE_FOUND queries are looked at.
 * The vTable images lie in d_vtb: file f is d_vtb[d_file_off[f] .. +
 * d_file_size[f]) and has number d_file_number[f], ascending; a file is found
 * by bisection (a list that does not ascend may miss a file, and is never
 * read outside nfiles). nfiles may be 0 (the three arrays and d_vtb null).
 *
 * Per query: d_status[q] = LVKV_VRES_*; for OK, the value is
 * (d_out_src[q] == 0 ? d_vals : d_vtb)[d_out_off[q] .. + d_out_len[q]); no value
 * byte is copied. Other statuses leave 0 / 0 / 0. Varints decode as
 * util/coding.cc does (non-canonical forms accepted); bytes after the index
 * in the value, and after the record inside the handle, are ignored as the
 * reference ignores them.
 *
 * nqueries == 0, before every other check: LVKV_OK, and an empty report where
 * d_report is not null. LVKV_ERR_INVALID, before any launch: a null pointer
 * other than d_state (and the file arguments when nfiles == 0),
 * nqueries >= 2^31, nfiles >= 2^31, scratch_bytes under
 * lvkv_vtable_resolve_scratch_bytes. */
int lvkv_vtable_resolve_device(
    const void* d_vals, const uint64_t* d_val_off, const uint32_t* d_val_len,
    const uint8_t* d_state, size_t nqueries, const void* d_vtb, const uint64_t* d_file_off,
    const uint64_t* d_file_size, const uint64_t* d_file_number, size_t nfiles, void* d_scratch,
    size_t scratch_bytes, uint8_t* d_status, uint8_t* d_out_src, uint64_t* d_out_off,
    uint32_t* d_out_len, lvkv_vtable_resolve_report* d_report, void* stream);

typedef struct lvkv_vtable_gather_report {
  int32_t status;     /* LVKV_VTABLE_OK or LVKV_VTABLE_CAPACITY */
  uint32_t nvalues;   /* queries whose status is LVKV_VRES_OK */
  uint64_t dst_bytes; /* their bytes: what d_dst has to hold */
} lvkv_vtable_gather_report;

size_t lvkv_vtable_gather_scratch_bytes(size_t nqueries);

/* The values lvkv_vtable_resolve_device found, end to end: query q's lies at
 * d_dst[d_dst_off[q] .. d_dst_off[q + 1]) (nqueries + 1 offsets), empty for a
 * query whose status is not LVKV_VRES_OK. On LVKV_VTABLE_CAPACITY nothing is
 * written to d_dst or d_dst_off, and the report says what is needed.
 *
 * nqueries == 0, before every other check: LVKV_OK, and an empty report where
 * d_report is not null. LVKV_ERR_INVALID, before any launch: a null pointer,
 * nqueries >= 2^31, scratch_bytes under lvkv_vtable_gather_scratch_bytes. */
int lvkv_vtable_gather_device(
    const void* d_vals, const void* d_vtb, const uint8_t* d_status, const uint8_t* d_out_src,
    const uint64_t* d_out_off, const uint32_t* d_out_len, size_t nqueries, void* d_scratch,
    size_t scratch_bytes, void* d_dst, uint64_t dst_capacity, uint64_t* d_dst_off,
    lvkv_vtable_gather_report* d_report, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* LVKV_VTABLE_H_ */
