"""CPU model of Block::NewIterator + SeekToFirst + Next until !Valid()
(table/block.cc:25-40, 55-75, 230-291): TEST INFRASTRUCTURE, the expectation
of tests/test_sst_read_entries.py for lvkv_sst_read_entries_device.

walk() restates the reference's forward walk with its verdicts and nothing
stricter; layout() and read() restate where the call puts what the walk
yields. It is pinned, not trusted: tests/test_sst_entries_model.py holds it
against what the reference's own Block::Iter yielded for the blocks of
tests/golden/block_walk.json (gen_block_walk.cc), damaged ones included, and
against sst_build_model.block_entries on every golden table.

One stated difference from the reference: DecodeEntry adds non_shared +
value_length in 32 bits (block.cc:71); here, as on the device, the sum is
taken exactly and an entry whose sum would have wrapped is BAD_ENTRY.
"""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

OK, BAD_BLOCK, BAD_ENTRY, SKIPPED = range(4)
CAPACITY = 1
NONE = 0xFFFFFFFF
# Status::ToString() of the iterator, per status
STATUS_TEXT = {OK: "OK", BAD_BLOCK: "Corruption: bad block contents",
               BAD_ENTRY: "Corruption: bad entry in block"}
# (key, the value's offset in the block, the value's length)
Entry = Tuple[bytes, int, int]


def _varint32(b: bytes, p: int, limit: int) -> Optional[Tuple[int, int]]:
    """GetVarint32Ptr (util/coding.cc): (value, next) or None."""
    v = 0
    for i in range(5):
        if p + i >= limit:
            return None
        c = b[p + i]
        if c & 128:
            v |= (c & 127) << (7 * i)
        else:
            return (v | (c << (7 * i))) & 0xFFFFFFFF, p + i + 1
    return None


def decode_entry(b: bytes, p: int, limit: int) -> Optional[Tuple[int, int, int, int]]:
    """DecodeEntry: (shared, non_shared, value_length, where the delta is)."""
    if limit - p < 3:
        return None
    out = []
    for _ in range(3):
        r = _varint32(b, p, limit)
        if r is None:
            return None
        out.append(r[0])
        p = r[1]
    if limit - p < out[1] + out[2]:  # (exact, not modulo 2^32: the stated difference)
        return None
    return out[0], out[1], out[2], p


def walk(block: bytes) -> Tuple[int, List[Entry]]:
    """(status, entries) of one block's forward walk."""
    block = bytes(block)
    size = len(block)
    if size < 4:
        return BAD_BLOCK, []
    nr = int.from_bytes(block[size - 4:], "little")
    if nr > (size - 4) // 4:
        return BAD_BLOCK, []
    if nr == 0:
        return OK, []  # NewEmptyIterator
    limit = size - 4 - 4 * nr
    at = int.from_bytes(block[limit:limit + 4], "little")  # restart[0]; the others are not read
    key, out = b"", []
    while at < limit:
        d = decode_entry(block, at, limit)
        if d is None or d[0] > len(key):
            return BAD_ENTRY, out
        sh, ns, vl, p = d
        key = key[:sh] + block[p:p + ns]
        out.append((key, p + ns, vl))
        at = p + ns + vl
    return OK, out


def entries_of(block: bytes) -> List[Tuple[bytes, bytes]]:
    """The (key, value) pairs the walk yields."""
    block = bytes(block)
    return [(k, block[o:o + n]) for k, o, n in walk(block)[1]]


def read(blocks: Sequence[bytes], raw_off: Sequence[int], skip: Optional[Sequence[int]] = None,
         max_entries: Optional[int] = None, key_capacity: Optional[int] = None) -> dict:
    """One call over blocks that sit at raw_off in d_raw: the packed keys
    (key i at key_off[i], the end of key i - 1 rounded up to 8), the five
    arrays, block_first, the statuses and the report."""
    keys, key_off, key_len, val_off, val_len = [], [], [], [], []
    first, status, end = [0], [], 0
    for b, (block, off) in enumerate(zip(blocks, raw_off)):
        if skip is not None and skip[b]:
            st, ents = SKIPPED, []
        else:
            st, ents = walk(block)
        status.append(st)
        for k, o, n in ents:
            at = (end + 7) & ~7
            keys.append(k)
            key_off.append(at)
            key_len.append(len(k))
            val_off.append(off + o)
            val_len.append(n)
            end = at + len(k)
        first.append(len(keys))
    bad = [b for b, st in enumerate(status) if st in (BAD_BLOCK, BAD_ENTRY)]
    rep = {"status": OK, "nbad": len(bad), "first_bad_block": bad[0] if bad else NONE,
           "max_key_len": max(key_len, default=0), "num_entries": len(keys), "key_bytes": end,
           "value_bytes": sum(val_len)}
    if (max_entries is not None and len(keys) > max_entries) or \
            (key_capacity is not None and end > key_capacity):
        rep["status"] = CAPACITY
    return {"keys": keys, "key_off": key_off, "key_len": key_len, "val_off": val_off,
            "val_len": val_len, "block_first": first, "block_status": status, "report": rep}
