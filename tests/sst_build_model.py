"""CPU model of TableBuilder::Add + the final Flush (table/table_builder.cc:
94-123, 213-215) over sorted entries: TEST INFRASTRUCTURE, the expectation of
tests/test_sst_build_blocks.py for lvkv_sst_build_blocks_device.

cut() restates where the reference ends a block; the bytes of a block are
sst_finish_model.block_of. It is pinned, not trusted: test_model_recuts_*
rebuild, byte for byte, the data blocks of tables the reference's
TableBuilder wrote with no Flush() of the generator's own
(tests/golden/table.sst, finish_nofilter.sst, cuts_*.sst).
"""
from __future__ import annotations

from typing import List, Optional, Tuple

import sst_finish_model as fm

OK, UNSORTED, BAD_KEY, CAPACITY, TOO_LARGE = range(5)
NONE = 0xFFFFFFFF
Entry = Tuple[bytes, bytes]


def block_entries(block: bytes) -> List[Entry]:
    """Every (key, value) of a block, in order (Block::Iter)."""
    block = bytes(block)
    nr = int.from_bytes(block[-4:], "little")
    limit = len(block) - 4 - 4 * nr
    out, key, p = [], b"", 0
    while p < limit:
        sh, p = fm._get_varint32(block, p, limit)
        ns, p = fm._get_varint32(block, p, limit)
        vl, p = fm._get_varint32(block, p, limit)
        key = key[:sh] + block[p:p + ns]
        out.append((key, block[p + ns:p + ns + vl]))
        p += ns + vl
    assert p == limit
    return out


def cut(entries: List[Entry], block_size: int, restart_interval: int) -> List[List[Entry]]:
    """The entry lists of the blocks TableBuilder cuts: after Add, the block
    is flushed when buffer + 4 * restarts + 4 >= block_size
    (block_builder.cc:55-59, table_builder.cc:119-122)."""
    blocks, cur, size, restarts, counter, last = [], [], 0, 1, 0, b""
    for key, value in entries:
        shared = 0
        if counter < restart_interval:
            m = min(len(last), len(key))
            while shared < m and last[shared] == key[shared]:
                shared += 1
        else:
            restarts += 1
            counter = 0
        size += (len(fm.varint(shared)) + len(fm.varint(len(key) - shared)) +
                 len(fm.varint(len(value))) + len(key) - shared + len(value))
        cur.append((key, value))
        last = key
        counter += 1
        if size + 4 * restarts + 4 >= block_size:
            blocks.append(cur)
            cur, size, restarts, counter, last = [], 0, 1, 0, b""
    if cur:
        blocks.append(cur)
    return blocks


def _internal_less(a: bytes, b: bytes) -> bool:
    """InternalKeyComparator::Compare(a, b) < 0 (db/dbformat.cc:47-63)."""
    ua, ub = a[:-8], b[:-8]
    if ua != ub:
        return ua < ub
    return int.from_bytes(a[-8:], "little") > int.from_bytes(b[-8:], "little")


def check_order(keys: List[bytes], key_format: int) -> Tuple[int, int]:
    """(status, first_bad_entry) of the order check: BAD_KEY for the lowest
    internal key under 8 bytes, else UNSORTED for the lowest entry not
    greater than the one before it."""
    if key_format == 1:
        for i, k in enumerate(keys):
            if len(k) < 8:
                return BAD_KEY, i
    for i in range(1, len(keys)):
        less = _internal_less(keys[i - 1], keys[i]) if key_format == 1 else keys[i - 1] < keys[i]
        if not less:
            return UNSORTED, i
    return OK, NONE


def build(entries: List[Entry], block_size: int, restart_interval: int, key_format: int,
          max_blocks: Optional[int] = None, raw_capacity: Optional[int] = None):
    """(blocks' bytes, raw offsets, report dict) of one call."""
    rep = {"status": OK, "first_bad_entry": NONE, "nblocks": 0, "max_block_len": 0,
           "max_key_len": max((len(k) for k, _ in entries), default=0),
           "num_entries": len(entries), "raw_bytes": 0}
    rep["status"], rep["first_bad_entry"] = check_order([k for k, _ in entries], key_format)
    if rep["status"] != OK:
        return [], [], rep
    blocks = [fm.block_of(b, restart_interval) for b in cut(entries, block_size, restart_interval)]
    offs, end = [], 0
    for b in blocks:
        offs.append((end + 15) & ~15)
        end = offs[-1] + len(b)
    rep.update(nblocks=len(blocks), max_block_len=max(map(len, blocks), default=0), raw_bytes=end)
    if (max_blocks is not None and len(blocks) > max_blocks) or \
            (raw_capacity is not None and end > raw_capacity):
        rep["status"] = CAPACITY
    return blocks, offs, rep
