"""Sequential restatement of DBIter (db/db_iter.cc) over a list of internal
keys in MergingIterator's order: TEST INFRASTRUCTURE, the expectation of
tests/test_sst_scan.py for lvkv_sst_scan_entries_device.

It is pinned, not trusted: test_scan_model.py holds it, entry for entry,
forward and reverse, to what the reference's own DBIter did over the
reference's tables (tests/golden/gen_scan.cc).

The walk is the reference's, one entry at a time with its own state (`skip`
and `skipping`, saved_key_ and value_type): it does NOT use the flag
formulation the device call is built on ("visible = an eligible value whose
eligible predecessor has another user key"), so the two meet only in their
results. The internal iterator is an index into the list; Prev is index - 1.
"""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

OK, UNSORTED, BAD_KEY, CAPACITY = range(4)
Q_OK, Q_CORRUPT = range(2)
NONE = 0xFFFFFFFF
NO_LIMIT = 0xFFFFFFFF
MAX_SEQUENCE = (1 << 56) - 1  # kMaxSequenceNumber
TYPE_DELETION, TYPE_VALUE = 0, 1
VALUE_TYPE_FOR_SEEK = TYPE_VALUE

REPORT_KEYS = ["status", "first_bad_entry", "num_in", "num_visible", "num_above_snapshot",
               "num_unparsable", "num_deletions", "num_hidden", "key_bytes", "value_bytes",
               "nqueries", "max_count", "sum_count"]


def parse(key: bytes) -> Optional[Tuple[bytes, int, int]]:
    """ParseInternalKey (db/dbformat.h:173-183): (user key, sequence, type),
    None for a key under 8 bytes or a type byte above kTypeValue."""
    if len(key) < 8:
        return None
    tag = int.from_bytes(key[-8:], "little")
    return (key[:-8], tag >> 8, tag & 0xFF) if (tag & 0xFF) <= TYPE_VALUE else None


def internal_compare(a: bytes, b: bytes) -> int:
    """InternalKeyComparator::Compare (db/dbformat.cc:47-63)."""
    ua, ub = a[:-8], b[:-8]
    if ua != ub:
        return -1 if ua < ub else 1
    ta, tb = int.from_bytes(a[-8:], "little"), int.from_bytes(b[-8:], "little")
    return -1 if ta > tb else 1 if ta < tb else 0


class DBIter:
    """db/db_iter.cc over keys[i]; `pos` is iter_'s position (len(keys): not
    Valid() at the end, -1: not Valid() before the start)."""

    def __init__(self, keys: Sequence[bytes], snapshot: int):
        self.keys, self.sequence = keys, snapshot
        self.pos = len(keys)
        self.valid = False
        self.forward = True
        self.corrupt = False  # status_: "corrupted internal key in DBIter", sticky
        self.saved_key = b""
        self.saved_at = -1  # where saved_value_ was taken from (kReverse)

    def _iter_valid(self) -> bool:
        return 0 <= self.pos < len(self.keys)

    def _parse_key(self):
        p = parse(self.keys[self.pos])
        if p is None:
            self.corrupt = True
        return p

    def at(self) -> int:
        """The entry key() and value() are of."""
        assert self.valid
        return self.pos if self.forward else self.saved_at

    def user_key(self) -> bytes:
        assert self.valid
        return self.keys[self.pos][:-8] if self.forward else self.saved_key

    def _find_next_user_entry(self, skipping: bool, skip: bytes) -> None:
        # db/db_iter.cc:189-219
        while True:
            p = self._parse_key()
            if p is not None and p[1] <= self.sequence:
                if p[2] == TYPE_DELETION:
                    skip, skipping = p[0], True
                elif not (skipping and p[0] <= skip):
                    self.valid = True
                    self.saved_key = b""
                    return
            self.pos += 1
            if not self._iter_valid():
                break
        self.saved_key = b""
        self.valid = False

    def _find_prev_user_entry(self) -> None:
        # db/db_iter.cc:248-288
        value_type = TYPE_DELETION
        if self._iter_valid():
            while True:
                p = self._parse_key()
                if p is not None and p[1] <= self.sequence:
                    if value_type != TYPE_DELETION and p[0] < self.saved_key:
                        break
                    value_type = p[2]
                    if value_type == TYPE_DELETION:
                        self.saved_key, self.saved_at = b"", -1
                    else:
                        self.saved_key, self.saved_at = p[0], self.pos
                self.pos -= 1
                if not self._iter_valid():
                    break
        if value_type == TYPE_DELETION:
            self.valid = False
            self.saved_key, self.saved_at = b"", -1
            self.forward = True
        else:
            self.valid = True

    def seek(self, target: bytes) -> None:
        # db/db_iter.cc:290-302
        self.forward = True
        seek_key = target + ((self.sequence << 8) | VALUE_TYPE_FOR_SEEK).to_bytes(8, "little")
        lo, hi = 0, len(self.keys)  # iter_->Seek: the first entry not below seek_key
        while lo < hi:
            mid = (lo + hi) // 2
            if internal_compare(self.keys[mid], seek_key) < 0:
                lo = mid + 1
            else:
                hi = mid
        self.pos = lo
        self.seek_pos = lo
        if self._iter_valid():
            self._find_next_user_entry(False, b"")
        else:
            self.valid = False

    def seek_to_first(self) -> None:
        self.forward = True
        self.pos = 0
        if self._iter_valid():
            self._find_next_user_entry(False, b"")
        else:
            self.valid = False

    def seek_to_last(self) -> None:
        self.forward = False
        self.pos = len(self.keys) - 1
        self._find_prev_user_entry()

    def next(self) -> None:
        # db/db_iter.cc:153-187
        assert self.valid
        if not self.forward:
            self.forward = True
            self.pos = 0 if not self._iter_valid() else self.pos + 1
            if not self._iter_valid():
                self.valid = False
                self.saved_key = b""
                return
        else:
            self.saved_key = self.keys[self.pos][:-8]
            self.pos += 1
            if not self._iter_valid():
                self.valid = False
                self.saved_key = b""
                return
        self._find_next_user_entry(True, self.saved_key)

    def prev(self) -> None:
        # db/db_iter.cc:221-246
        assert self.valid
        if self.forward:
            self.saved_key = self.keys[self.pos][:-8]
            while True:
                self.pos -= 1
                if not self._iter_valid():
                    self.valid = False
                    self.saved_key, self.saved_at = b"", -1
                    return
                if self.keys[self.pos][:-8] < self.saved_key:
                    break
            self.forward = False
        self._find_prev_user_entry()


def forward_walk(keys: Sequence[bytes], snapshot: int) -> Tuple[List[int], bool]:
    """SeekToFirst, then Next to the end: (the entries yielded, status().ok())."""
    it = DBIter(keys, snapshot)
    out = []
    it.seek_to_first()
    while it.valid:
        out.append(it.at())
        it.next()
    return out, not it.corrupt


def reverse_walk(keys: Sequence[bytes], snapshot: int) -> Tuple[List[int], bool]:
    """SeekToLast, then Prev to the start."""
    it = DBIter(keys, snapshot)
    out = []
    it.seek_to_last()
    while it.valid:
        out.append(it.at())
        it.prev()
    return out, not it.corrupt


def query(keys: Sequence[bytes], snapshot: int, start: bytes, limit: Optional[bytes],
          max_count: Optional[int]) -> Tuple[List[int], Optional[int], bool]:
    """for (it->Seek(start); it->Valid() && n < max && it->key() < limit;
    it->Next()) ++n: (the entries counted, the entry the iterator ends on or
    None, status().ok())."""
    it = DBIter(keys, snapshot)
    out = []
    it.seek(start)
    while it.valid and (max_count is None or len(out) < max_count) and \
            (limit is None or it.user_key() < limit):
        out.append(it.at())
        it.next()
    return out, (it.at() if it.valid else None), not it.corrupt


def whole_call_status(keys: Sequence[bytes]) -> Tuple[int, int]:
    """(status, first_bad_entry) before CAPACITY: BAD_KEY, then UNSORTED."""
    short = [i for i, k in enumerate(keys) if len(k) < 8]
    if short:
        return BAD_KEY, short[0]
    for i in range(1, len(keys)):
        if internal_compare(keys[i - 1], keys[i]) > 0:
            return UNSORTED, i
    return OK, NONE


def scan(keys: Sequence[bytes], val_len: Sequence[int], snapshot: int,
         queries: Sequence[Tuple[bytes, Optional[bytes], Optional[int]]] = (),
         max_out: Optional[int] = None):
    """One call: (src of the visible entries, [(first, count, status)] a query,
    report). Off OK both lists are empty (nothing is written)."""
    n = len(keys)
    rep = dict.fromkeys(REPORT_KEYS, 0)
    rep.update(status=OK, first_bad_entry=NONE, num_in=n, nqueries=len(queries) if n else 0)
    if n == 0:
        return [], [], rep
    rep["status"], rep["first_bad_entry"] = whole_call_status(keys)
    if rep["status"] != OK:
        return [], [], rep
    src, _ = forward_walk(keys, snapshot)
    parsed = [parse(k) for k in keys]
    rep["num_visible"] = len(src)
    rep["num_unparsable"] = sum(p is None for p in parsed)
    rep["num_above_snapshot"] = sum(p is not None and p[1] > snapshot for p in parsed)
    rep["num_deletions"] = sum(p is not None and p[1] <= snapshot and p[2] == TYPE_DELETION
                               for p in parsed)
    rep["num_hidden"] = n - len(src) - rep["num_unparsable"] - rep["num_above_snapshot"] - \
        rep["num_deletions"]
    rep["key_bytes"] = sum(len(keys[e]) - 8 for e in src)
    rep["value_bytes"] = sum(val_len[e] for e in src)
    if len(src) > (n if max_out is None else max_out):
        rep["status"] = CAPACITY
        return [], [], rep
    slot = {e: j for j, e in enumerate(src)}
    per_query = []
    for start, limit, max_count in queries:
        counted, end, ok = query(keys, snapshot, start, limit, max_count)
        assert counted == src[slot[counted[0]]:slot[counted[0]] + len(counted)] if counted else True
        first = slot[counted[0]] if counted else slot[end] if end is not None else len(src)
        per_query.append((first, len(counted), Q_OK if ok else Q_CORRUPT))
    rep["max_count"] = max((c for _, c, _ in per_query), default=0)
    rep["sum_count"] = sum(c for _, c, _ in per_query)
    return src, per_query, rep
