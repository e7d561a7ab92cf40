"""CPU model of MergingIterator's forward walk over sorted runs
(table/merger.cc:150-163) and of the drops DoCompactionWork applies to what
it hands out (db/db_impl.cc:1022-1055): TEST INFRASTRUCTURE, the expectation
of tests/test_sst_merge_entries.py for lvkv_sst_merge_entries_device.

It is pinned, not trusted: test_sst_merge_model.py holds it, entry for entry
and flag for flag, to what the reference's own NewMergingIterator, the loop
restated with its ParseInternalKey and comparators, and its TableBuilder
produced (tests/golden/gen_merge.cc, merge_cases.json, merge_*.sst).

The walk is restated as the reference does it -- the smallest of the runs'
heads, the lowest run among equals -- not as the device computes it (a rank
per entry), so the two check each other.
"""
from __future__ import annotations

import functools
from typing import List, Optional, Sequence, Tuple

import sst_build_model as bm

OK, UNSORTED, BAD_KEY, CAPACITY, BAD_RUNS = range(5)
NONE = 0xFFFFFFFF
MAX_SEQUENCE = (1 << 56) - 1  # kMaxSequenceNumber
KEEP, HIDDEN, OBSOLETE = range(3)
Range = Tuple[bytes, bytes]  # smallest, largest user key


def _cmp(a, b) -> int:
    return -1 if a < b else 1 if a > b else 0


def compare(a: bytes, b: bytes, key_format: int) -> int:
    """The call's comparator: byte-wise, or InternalKeyComparator::Compare
    (db/dbformat.cc:47-63)."""
    if key_format == 0:
        return _cmp(a, b)
    c = _cmp(a[:-8], b[:-8])
    return c if c else -_cmp(int.from_bytes(a[-8:], "little"), int.from_bytes(b[-8:], "little"))


def order(runs: Sequence[Sequence[bytes]], key_format: int) -> List[Tuple[int, int]]:
    """(run, index in the run) of every entry as MergingIterator hands them
    out: FindSmallest takes the first child no other is smaller than."""
    at = [0] * len(runs)
    out = []
    while True:
        best = None
        for r, keys in enumerate(runs):
            if at[r] < len(keys) and \
                    (best is None or compare(keys[at[r]], runs[best][at[best]], key_format) < 0):
                best = r
        if best is None:
            return out
        out.append((best, at[best]))
        at[best] += 1


def parse(key: bytes) -> Optional[Tuple[bytes, int, int]]:
    """ParseInternalKey (db/dbformat.h:173-183) of a key of 8 bytes or more:
    (user key, sequence, type), None for a type byte above kTypeValue."""
    tag = int.from_bytes(key[-8:], "little")
    return (key[:-8], tag >> 8, tag & 0xFF) if tag & 0xFF <= 1 else None


def base_level(user: bytes, deeper: Sequence[Range]) -> bool:
    """IsBaseLevelForKey (db/version_set.cc:1518-1537): in no file's range."""
    return not any(lo <= user <= hi for lo, hi in deeper)


def drops(keys: Sequence[bytes], smallest_snapshot: int, deeper: Sequence[Range]) -> List[int]:
    """KEEP / HIDDEN / OBSOLETE of every key of the merged order: the loop of
    db/db_impl.cc:1022-1055 with its three variables."""
    flags = []
    current, has_current, last = b"", False, MAX_SEQUENCE
    for key in keys:
        flag = KEEP
        p = parse(key)
        if p is None:
            current, has_current, last = b"", False, MAX_SEQUENCE
        else:
            user, seq, typ = p
            if not has_current or user != current:
                current, has_current, last = user, True, MAX_SEQUENCE
            if last <= smallest_snapshot:
                flag = HIDDEN
            elif typ == 0 and seq <= smallest_snapshot and base_level(user, deeper):
                flag = OBSOLETE
            last = seq
        flags.append(flag)
    return flags


def check_runs(run_first: Sequence[int], n: int) -> bool:
    return run_first[0] == 0 and run_first[-1] == n and \
        all(a <= b for a, b in zip(run_first, run_first[1:]))


def merge(keys: Sequence[bytes], val_len: Sequence[int], run_first: Sequence[int],
          key_format: int = 1, compact: bool = False, smallest_snapshot: int = 0,
          deeper: Sequence[Range] = (), max_out: Optional[int] = None):
    """One call over entries laid run after run: (src of the survivors in
    merged order, src of the dropped in merged order, report dict); both
    lists empty unless the status is OK."""
    n = len(keys)
    rep = {"status": OK, "first_bad_entry": NONE, "num_in": n, "num_out": 0, "num_hidden": 0,
           "num_obsolete": 0, "max_key_len": 0, "key_bytes": 0, "value_bytes": 0}
    if n == 0:
        return [], [], rep
    if not check_runs(run_first, n):
        rep["status"] = BAD_RUNS
        return [], [], rep
    rep["max_key_len"] = max(map(len, keys))
    firsts = set(run_first)
    if key_format == 1:
        short = [i for i, k in enumerate(keys) if len(k) < 8]
        if short:
            rep.update(status=BAD_KEY, first_bad_entry=short[0])
            return [], [], rep
    for i in range(1, n):
        if i not in firsts and compare(keys[i - 1], keys[i], key_format) >= 0:
            rep.update(status=UNSORTED, first_bad_entry=i)
            return [], [], rep
    merged = fast_order(keys, run_first, key_format)
    flags = drops([keys[e] for e in merged], smallest_snapshot, deeper) if compact \
        else [KEEP] * n
    src = [e for e, f in zip(merged, flags) if f == KEEP]
    dropped = [e for e, f in zip(merged, flags) if f != KEEP]
    rep.update(num_out=len(src), num_hidden=flags.count(HIDDEN),
               num_obsolete=flags.count(OBSOLETE), key_bytes=sum(len(keys[e]) for e in src),
               value_bytes=sum(val_len[e] for e in src))
    if max_out is not None and len(src) > max_out:
        rep["status"] = CAPACITY
        return [], [], rep
    return src, dropped, rep


def fast_order(keys: Sequence[bytes], run_first: Sequence[int], key_format: int) -> List[int]:
    """The merged order of valid inputs as input indices, by a stable sort
    (Python's): the runs laid end to end are in run order, so equal keys keep
    it. What merge() uses; the model test holds it to order()."""
    key = functools.cmp_to_key(lambda a, b: compare(keys[a], keys[b], key_format))
    return sorted(range(len(keys)), key=key)


def survivors(entries: Sequence[bm.Entry], src: Sequence[int]) -> List[bm.Entry]:
    return [entries[e] for e in src]
