/* Range scans on the device: what a reader at a snapshot sees of entries in
 * MergingIterator's order, and where its Seeks land.
 *
 *   lvkv_sst_scan_entries_device  DBIter's forward walk (db/db_iter.cc:134-219:
 *       ParseKey, Next, FindNextUserEntry) and DBIter::Seek (db/db_iter.cc:290-302)
 *       for a batch of ranges, over the entries lvkv_sst_merge_entries_device
 *       without LVKV_MERGE_COMPACT leaves (or any single sorted run:
 *       lvkv_sst_read_entries_device's, lvkv_memtable_from_batches_device's).
 *
 * Stream-ordered: no synchronisation, no copy to the host, every result in
 * device memory (return codes LVKV_OK / LVKV_ERR_* from lvkv_crc32c.h).
 * Nothing is ever written at or past a capacity. The sizing function never
 * decreases when an argument grows.
 *
 * NOT BUILT:
 *   - Prev / SeekToLast as a walk of their own (FindPrevUserEntry). Over
 *     sorted entries the reverse walk yields the forward list backwards, so a
 *     caller reads its slice from the other end;
 *   - read sampling (DBImpl::RecordReadSample, db/db_iter.cc:137-143), which
 *     changes no result.
 */
#ifndef LVKV_SCAN_H_
#define LVKV_SCAN_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* lvkv_sst_scan_report.status */
#define LVKV_SCAN_OK 0
#define LVKV_SCAN_UNSORTED 1   /* entry first_bad_entry is below the one before it under
                                  InternalKeyComparator (equal keys are legal) */
#define LVKV_SCAN_BAD_KEY 2    /* a key under 8 bytes. DELIBERATE DIFFERENCE, as in the merge
                                  and get calls: ExtractUserKey asserts there */
#define LVKV_SCAN_CAPACITY 3   /* more visible entries than max_out */
#define LVKV_SCAN_NONE 0xFFFFFFFFu /* first_bad_entry: none */

/* d_q_status[q] */
#define LVKV_SCAN_Q_OK 0
#define LVKV_SCAN_Q_CORRUPT 1  /* "corrupted internal key in DBIter": the walk passed a key
                                  that does not parse; sticky in DBIter::status() */

#define LVKV_SCAN_NO_LIMIT 0xFFFFFFFFu /* d_limit_len[q]: the range has no upper end */

typedef struct lvkv_sst_scan_report {
  int32_t  status;              /* LVKV_SCAN_* */
  uint32_t first_bad_entry;     /* lowest offending entry for UNSORTED / BAD_KEY, else
                                   LVKV_SCAN_NONE */
  uint32_t num_in;              /* nentries */
  uint32_t num_visible;         /* with CAPACITY: the max_out a repeat needs */
  uint32_t num_above_snapshot;  /* keys that parse, sequence above the snapshot */
  uint32_t num_unparsable;      /* type byte above 1 */
  uint32_t num_deletions;       /* at or below the snapshot, kTypeDeletion */
  uint32_t num_hidden;          /* at or below the snapshot, kTypeValue, behind a newer entry
                                   of their user key */
  uint64_t key_bytes;           /* the visible entries' user keys */
  uint64_t value_bytes;         /* the visible entries' values, as stored */
  uint32_t nqueries;
  uint32_t max_count;           /* the largest d_q_count */
  uint64_t sum_count;           /* the sum of d_q_count */
} lvkv_sst_scan_report;

/* The scratch of lvkv_sst_scan_entries_device. */
size_t lvkv_sst_scan_entries_scratch_bytes(size_t nentries, size_t nqueries);

/* Entry i is the internal key d_keys[d_key_off[i], + d_key_len[i]) with the
 * value d_val_off[i] / d_val_len[i] (no value byte is read, so there is no
 * d_vals): the merge call's d_out_key_off / d_out_key_len / d_out_val_off /
 * d_out_val_len, or the arrays of one sorted run. The order is the caller's:
 * every entry not below the one before it under InternalKeyComparator
 * (db/dbformat.cc:47-63), equal keys legal (the merge hands out the same key
 * from several runs).
 *
 * Which entries a reader at `snapshot` sees. Entry i is ELIGIBLE when its key
 * parses (ParseInternalKey: type byte <= 1) and its sequence is <= snapshot.
 * It is VISIBLE when it is eligible, of kTypeValue, and the eligible entry
 * directly before it in the given order has another user key, or there is
 * none. That is FindNextUserEntry's loop: `skip` is always the user key of the
 * last eligible entry the walk passed, a deletion sets it and a yielded value
 * becomes it in Next; an entry above the snapshot or one that does not parse
 * changes nothing. The set does not depend on where a Seek starts: the entries
 * of the seek key that lie before the seek position have trailers above
 * (snapshot << 8 | 1), so none of them is eligible.
 *
 * Outputs for the call: the visible entries in order. Visible entry j is
 * input entry d_out_src[j]; d_out_key_off / d_out_key_len [j] describe its
 * USER key (the length without the 8-byte trailer) in d_keys, d_out_val_off /
 * d_out_val_len [j] its value as stored, the fork's type byte included:
 * DBIter::key() and DBIter::value(). No key or value byte is copied.
 *
 * Query q is the loop
 *     for (it->Seek(start); it->Valid() && n < max && it->key() < limit; it->Next()) ++n;
 * with start = d_qkeys[d_start_off[q], + d_start_len[q]), limit = d_qkeys[
 * d_limit_off[q], + d_limit_len[q]) (user keys; a d_limit_len of
 * LVKV_SCAN_NO_LIMIT: no limit, d_limit_off[q] is not read) and max =
 * d_q_max[q] (d_q_max null: unbounded). Seek lands at the first entry not
 * below (start, snapshot, kValueTypeForSeek) under InternalKeyComparator. The
 * entries the loop counts are visible entries d_q_first[q] .. + d_q_count[q]
 * of the output list; a start above the limit gives count 0. d_q_status[q] is
 * LVKV_SCAN_Q_CORRUPT when a key that does not parse lies between the seek
 * position and the last position the loop's iterator reaches -- the visible
 * entry after the last one counted, or the end of the input where there is
 * none -- and LVKV_SCAN_Q_OK otherwise. d_q_first[q] is written for every
 * query, also with count 0 (the number of visible entries before the seek
 * position).
 *
 * d_report (device memory) says how it went. BAD_KEY is reported before
 * UNSORTED (a pair with a key under 8 bytes gets no verdict on its order),
 * that before CAPACITY; first_bad_entry is the lowest entry of the reported
 * kind. On a status other than OK nothing at all is written to the five
 * output arrays or the three per-query arrays, and never anything at or past
 * slot max_out. num_in and nqueries always hold; the counts and sums with OK
 * and CAPACITY, max_count and sum_count with OK, and are 0 otherwise.
 *
 * nentries == 0, before every other check: LVKV_OK, and a report of no
 * entries and no queries where d_report is not null (every pointer may be
 * null; the per-query arrays are not written). LVKV_ERR_INVALID, before any
 * launch: a null pointer other than d_q_max (and the seven other query
 * arrays when nqueries is 0), snapshot above kMaxSequenceNumber (2^56 - 1),
 * nentries or nqueries >= 2^31, scratch_bytes under the sizing function's
 * value. */
int lvkv_sst_scan_entries_device(
    const void* d_keys, const uint64_t* d_key_off, const uint32_t* d_key_len,
    const uint64_t* d_val_off, const uint32_t* d_val_len, size_t nentries, uint64_t snapshot,
    const void* d_qkeys, const uint64_t* d_start_off, const uint32_t* d_start_len,
    const uint64_t* d_limit_off, const uint32_t* d_limit_len,
    const uint32_t* d_q_max /* may be null */, size_t nqueries,
    void* d_scratch, size_t scratch_bytes,
    uint64_t* d_out_key_off, uint32_t* d_out_key_len, uint64_t* d_out_val_off,
    uint32_t* d_out_val_len, uint32_t* d_out_src, size_t max_out,
    uint32_t* d_q_first, uint32_t* d_q_count, uint8_t* d_q_status,
    lvkv_sst_scan_report* d_report, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* LVKV_SCAN_H_ */
