"""The memtable call in plain Python: TEST INFRASTRUCTURE, the expectation of
lvkv_memtable_from_batches_device (include/lvkv_memtable.h), itself held to
the reference's own recovery by tests/test_memtable_model.py.

It restates the loop of DBImpl::RecoverLogFile (db/db_impl.cc:453-488),
WriteBatch::Iterate (db/write_batch.cc:42-80), MemTable::Add's internal key
(db/memtable.cc:77-101) and InternalKeyComparator's order
(db/dbformat.cc:47-63). Batches are (offset, length) pairs into one payload,
as the device call takes them.
"""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

(OK, TOO_SMALL, UNKNOWN_TAG, BAD_PUT, BAD_DELETE, WRONG_COUNT, KEY_TOO_LONG, CAPACITY,
 DUPLICATE) = range(9)
NONE = 0xFFFFFFFF
M64 = (1 << 64) - 1
KEY_LIMIT = (1 << 32) - 8

STATUS_TEXT = {
    "OK": OK,
    "Corruption: log record too small": TOO_SMALL,
    "Corruption: unknown WriteBatch tag": UNKNOWN_TAG,
    "Corruption: bad WriteBatch Put": BAD_PUT,
    "Corruption: bad WriteBatch Delete": BAD_DELETE,
    "Corruption: WriteBatch has wrong count": WRONG_COUNT,
}


def varint(v: int) -> bytes:
    out = bytearray()
    while v >= 128:
        out.append((v & 127) | 128)
        v >>= 7
    out.append(v)
    return bytes(out)


def get_varint32(b, p: int, limit: int) -> Optional[Tuple[int, int]]:
    """GetVarint32Ptr (util/coding.cc) over b[p:limit]: (value, bytes) or None."""
    result = 0
    for i in range(5):
        if p + i >= limit:
            return None
        byte = b[p + i]
        result |= ((byte & 127) << (7 * i)) & 0xFFFFFFFF
        if not byte & 128:
            return result, i + 1
    return None


def put(key: bytes, value: bytes) -> bytes:
    return b"\x01" + varint(len(key)) + key + varint(len(value)) + value


def delete(key: bytes) -> bytes:
    return b"\x00" + varint(len(key)) + key


def batch(sequence: int, count: int, body: bytes) -> bytes:
    return sequence.to_bytes(8, "little") + count.to_bytes(4, "little") + body


def log_records(log: bytes) -> List[bytes]:
    """The logical records of a sound log file (db/log_format.h): no checksum
    is looked at -- the fixture logs are the reference writer's."""
    out, cur = [], None
    for base in range(0, len(log), 32768):
        block = log[base:base + 32768]
        p = 0
        while p + 7 <= len(block):
            n, t = int.from_bytes(block[p + 4:p + 6], "little"), block[p + 6]
            if t == 0 and n == 0:
                break
            frag = block[p + 7:p + 7 + n]
            p += 7 + n
            if t == 1:
                out.append(frag)
            elif t == 2:
                cur = bytearray(frag)
            elif t == 3:
                cur += frag
            else:
                assert t == 4
                out.append(bytes(cur + frag))
    return out


def walk(payload, off: int, length: int, virtual_len: Optional[int] = None):
    """WriteBatch::Iterate on payload[off : off + length]: (status, entries,
    last_seq) with entries (user key offset, user key length, value offset,
    value length, trailer) in the order met. last_seq is None for a batch
    under 12 bytes. virtual_len: the length the descriptor claims, where the
    bytes behind it are not there (KEY_TOO_LONG alone can be decided then)."""
    claimed = length if virtual_len is None else virtual_len
    if claimed < 12:
        return TOO_SMALL, [], None
    end = off + claimed
    sequence = int.from_bytes(payload[off:off + 8], "little")
    count = int.from_bytes(payload[off + 8:off + 12], "little")
    signed = count - (1 << 32) if count & 0x80000000 else count
    last_seq = (sequence + signed - 1) & M64
    entries = []
    found = 0
    p = off + 12
    while p < end:
        found += 1
        tag = payload[p]
        p += 1
        if tag > 1:
            return UNKNOWN_TAG, entries, last_seq
        bad = BAD_PUT if tag == 1 else BAD_DELETE
        k = get_varint32(payload, p, end)
        if k is None or k[0] > end - (p + k[1]):
            return bad, entries, last_seq
        if k[0] >= KEY_LIMIT:
            return KEY_TOO_LONG, entries, last_seq
        koff = p + k[1]
        p = koff + k[0]
        voff, vlen = p, 0
        if tag == 1:
            v = get_varint32(payload, p, end)
            if v is None or v[0] > end - (p + v[1]):
                return bad, entries, last_seq
            voff, vlen = p + v[1], v[0]
            p = voff + vlen
        trailer = ((((sequence + len(entries)) & M64) << 8) & M64) | tag
        entries.append((koff, k[0], voff, vlen, trailer))
    if found & 0xFFFFFFFF != count:
        return WRONG_COUNT, entries, last_seq
    return OK, entries, last_seq


def sort_key(payload, e):
    """InternalKeyComparator: the user key ascending as unsigned bytes (a
    shorter key before its extensions), then the trailer descending."""
    return bytes(payload[e[0]:e[0] + e[1]]), -e[4]


def from_batches(payload, batch_off: Sequence[int], batch_len: Sequence[int], *,
                 max_sequence: int = 0, paranoid: bool = False, max_entries: Optional[int] = None,
                 key_capacity: Optional[int] = None, virtual_len=None):
    """The device call's outputs: a dict with report, batch_status,
    batch_entries, and -- for status OK -- keys (the internal keys in log
    order), key_off, key_len, val_off, val_len, src in sorted order."""
    nb = len(batch_off)
    statuses, counts, entries, lasts = [], [], [], []
    for b in range(nb):
        st, es, last = walk(payload, batch_off[b], batch_len[b],
                            virtual_len[b] if virtual_len is not None else None)
        statuses.append(st)
        counts.append(len(es))
        entries += es
        lasts.append(last)
    claimed = [virtual_len[b] if virtual_len is not None and virtual_len[b] is not None
               else batch_len[b] for b in range(nb)]
    bad = [b for b in range(nb) if statuses[b] != OK]
    too_long = [b for b in range(nb) if statuses[b] == KEY_TOO_LONG]
    upto = bad[0] if paranoid and bad else nb
    seq = max_sequence
    for b in range(upto):
        if lasts[b] is not None and lasts[b] > seq:
            seq = lasts[b]
    rep = dict(status=OK, first_bad_batch=NONE, first_bad_entry=NONE, nentries=len(entries),
               key_bytes=sum(e[1] + 8 for e in entries), val_bytes=sum(e[3] for e in entries),
               max_key_len=max([e[1] + 8 for e in entries], default=0),
               n_too_small=statuses.count(TOO_SMALL),
               too_small_bytes=sum(claimed[b] for b in range(nb) if statuses[b] == TOO_SMALL),
               max_sequence_out=seq,
               n_bad_batches=sum(1 for s in statuses if s not in (OK, TOO_SMALL)))
    res = dict(report=rep, batch_status=statuses, batch_entries=counts)
    if paranoid and bad:
        rep.update(status=statuses[bad[0]], first_bad_batch=bad[0])
        return res
    if too_long:
        rep.update(status=KEY_TOO_LONG, first_bad_batch=too_long[0])
        return res
    if (max_entries is not None and len(entries) > max_entries) or \
            (key_capacity is not None and rep["key_bytes"] > key_capacity):
        rep["status"] = CAPACITY
        return res
    ikeys = [bytes(payload[e[0]:e[0] + e[1]]) + e[4].to_bytes(8, "little") for e in entries]
    seen = {}
    for j, k in enumerate(ikeys):
        if k in seen:
            rep.update(status=DUPLICATE, first_bad_entry=j)
            return res
        seen[k] = j
    at = [0]
    for k in ikeys:
        at.append(at[-1] + len(k))
    order = sorted(range(len(entries)), key=lambda j: sort_key(payload, entries[j]))
    res.update(keys=b"".join(ikeys), src=order, key_off=[at[j] for j in order],
               key_len=[len(ikeys[j]) for j in order], val_off=[entries[j][2] for j in order],
               val_len=[entries[j][3] for j in order], ikeys=[ikeys[j] for j in order])
    return res
