"""CPU model of KV separation (include/lvkv_vtable.h): TEST INFRASTRUCTURE, the
expectation of tests/test_vtable.py for lvkv_vtable_separate_device,
lvkv_vtable_resolve_device and lvkv_vtable_gather_device.

A plain restatement of BuildTable's loop (db/builder.cc:47-74), DecodeValue
(db/db_impl.cc:1245-1289), VTableReader::Get (table/vtable_reader.cc:17-45)
and the formats of table/vtable_format.cc. It is pinned, not trusted:
tests/test_vtable_model.py holds it to what the reference's own BuildTable,
VTableReader::Get and VTableIndex::Decode did (tests/golden/gen_vtable.cc).
"""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

OK, BAD_KEY, BAD_VALUE, TOO_LARGE, CAPACITY = range(5)
NO_ENTRY = 0xFFFFFFFF
(R_OK, R_SKIPPED, R_EMPTY, R_BAD_TYPE, R_BAD_INDEX, R_BAD_HANDLE, R_NO_FILE, R_PAST_END,
 R_BAD_HEADER, R_BAD_RECORD, R_TRAILING, R_RECORD_OVERRUN) = range(12)
NSTATUS = 12
STATE_FOUND = 1  # LVKV_GET_STATE_FOUND
Entry = Tuple[bytes, bytes]


def pattern(seed: int, n: int) -> bytes:
    """gen_vtable.cc's Pattern."""
    return bytes(((seed * 131 + j * 7 + (j >> 8)) & 0xFF) for j in range(n))


def varint(v: int) -> bytes:
    out = bytearray()
    while v >= 128:
        out.append((v & 127) | 128)
        v >>= 7
    out.append(v)
    return bytes(out)


def get_varint(b: bytes, p: int, limit: int, bits: int) -> Optional[Tuple[int, int]]:
    """GetVarint32Ptr / GetVarint64Ptr (util/coding.cc): (value, the offset
    after it), None when it runs past limit or is longer than the type
    allows. Bits past the type are dropped, as the shifts there drop them."""
    v = 0
    for i in range(5 if bits == 32 else 10):
        if p + i >= limit:
            return None
        c = b[p + i]
        v |= (c & 127) << (7 * i)
        if not c & 128:
            return v & ((1 << bits) - 1), p + i + 1
    return None


def index_value(file_number: int, off: int, size: int) -> bytes:
    """VTableIndex::Encode (table/vtable_format.cc:72-76)."""
    return b"\x01" + varint(file_number) + varint(off) + varint(size)


def record(user_key: bytes, value: bytes) -> bytes:
    """VTableBuilder::Add's bytes: header and VTableRecord::Encode."""
    body = varint(len(user_key)) + user_key + varint(len(value)) + value
    return len(body).to_bytes(4, "little") + body


def check_entry(key: bytes, value_len: int, kv_sep_size: int) -> int:
    """BuildTable's checks on one entry, in its order."""
    if value_len < kv_sep_size:
        return OK
    if len(key) < 8 or key[-8] > 1:
        return BAD_KEY
    if value_len == 0:
        return BAD_VALUE
    if len(key) - 8 + value_len - 1 >= 0xFFFFFFFF:
        return TOO_LARGE
    return OK


def separate(entries: Sequence[Entry], kv_sep_size: int, file_number: int,
             vtb_capacity: Optional[int] = None, out_val_capacity: Optional[int] = None) -> dict:
    """One lvkv_vtable_separate_device call: vtb, out_vals (a list), rec_off,
    rec_size, report. Nothing but the report unless its status is OK."""
    rep = {"status": OK, "first_bad_entry": NO_ENTRY, "records_num": 0, "table_size": 0,
           "out_val_bytes": 0, "max_out_val_len": 0}
    res = {"vtb": b"", "out_vals": [], "rec_off": [], "rec_size": [], "report": rep}
    for i, (k, v) in enumerate(entries):
        st = check_entry(k, len(v), kv_sep_size)
        if st != OK:
            rep["status"], rep["first_bad_entry"] = st, i
            return res
    vtb, out, roff, rsize = bytearray(), [], [], []
    for k, v in entries:
        if len(v) < kv_sep_size:
            out.append(bytes(v))
            roff.append(0)
            rsize.append(0)
            continue
        r = record(k[:-8], v[1:])
        out.append(index_value(file_number, len(vtb), len(r)))
        roff.append(len(vtb))
        rsize.append(len(r))
        vtb += r
        rep["records_num"] += 1
    rep.update(table_size=len(vtb), out_val_bytes=sum(map(len, out)),
               max_out_val_len=max(map(len, out), default=0))
    if (vtb_capacity is not None and len(vtb) > vtb_capacity) or \
            (out_val_capacity is not None and rep["out_val_bytes"] > out_val_capacity):
        rep["status"] = CAPACITY
        return res
    res.update(vtb=bytes(vtb), out_vals=out, rec_off=roff, rec_size=rsize)
    return res


def decode_index(value: bytes):
    """VTableIndex::Decode on a whole value: (R_OK, number, off, size, bytes
    left) or (status,)."""
    if not value or value[0] != 1:
        return (R_BAD_INDEX,)
    n = get_varint(value, 1, len(value), 64)
    if n is None:
        return (R_BAD_INDEX,)
    o = get_varint(value, n[1], len(value), 64)
    s = get_varint(value, o[1], len(value), 64) if o is not None else None
    if s is None:
        return (R_BAD_HANDLE,)
    return R_OK, n[0], o[0], s[0], len(value) - s[1]


def read_record(f: bytes, off: int, size: int):
    """VTableReader::Get on the file's bytes: (R_OK, offset of the value in f,
    its length, key) or (status,)."""
    if off + size > len(f):
        return (R_PAST_END,)
    if size < 4:
        return (R_BAD_HEADER,)
    rs = int.from_bytes(f[off:off + 4], "little")
    if rs > size - 4:
        return (R_RECORD_OVERRUN,)
    p, end = off + 4, off + 4 + rs
    kl = get_varint(f, p, end, 32)
    if kl is None or end - kl[1] < kl[0]:
        return (R_BAD_RECORD,)
    kp = kl[1]
    vl = get_varint(f, kp + kl[0], end, 32)
    if vl is None or end - vl[1] < vl[0]:
        return (R_BAD_RECORD,)
    if vl[1] + vl[0] != end:
        return (R_TRAILING,)
    return R_OK, vl[1], vl[0], bytes(f[kp:kp + kl[0]])


def resolve(vals: bytes, val_off: Sequence[int], val_len: Sequence[int], vtb: bytes,
            file_off: Sequence[int], file_size: Sequence[int], file_number: Sequence[int],
            state: Optional[Sequence[int]] = None):
    """One lvkv_vtable_resolve_device call: (status, src, off, len) lists and
    the report."""
    status, src, off, ln = [], [], [], []
    for q, (vo, vl) in enumerate(zip(val_off, val_len)):
        st, s, o, l = R_OK, 0, 0, 0
        v = vals[vo:vo + vl]
        if state is not None and state[q] != STATE_FOUND:
            st = R_SKIPPED
        elif vl == 0:
            st = R_EMPTY
        elif v[0] == 2:
            o, l = vo + 1, vl - 1
        elif v[0] != 1:
            st = R_BAD_TYPE
        else:
            ix = decode_index(v)
            st = ix[0]
            if st == R_OK:
                lo, hi = 0, len(file_number)  # the first file whose number is not below
                while lo < hi:
                    mid = lo + (hi - lo) // 2
                    if file_number[mid] < ix[1]:
                        lo = mid + 1
                    else:
                        hi = mid
                if lo >= len(file_number) or file_number[lo] != ix[1]:
                    st = R_NO_FILE
                else:
                    base = file_off[lo]
                    r = read_record(vtb[base:base + file_size[lo]], ix[2], ix[3])
                    st = r[0]
                    if st == R_OK:
                        s, o, l = 1, base + r[1], r[2]
        status.append(st)
        src.append(s)
        off.append(o)
        ln.append(l)
    count = [status.count(s) for s in range(NSTATUS)]
    oklen = [l for st, l in zip(status, ln) if st == R_OK]
    rep = {"nqueries": len(status), "count": count, "max_len": max(oklen, default=0),
           "total_len": sum(oklen)}
    return status, src, off, ln, rep


def gather(vals: bytes, vtb: bytes, status, src, off, ln, capacity: Optional[int] = None):
    """One lvkv_vtable_gather_device call: (dst, dst_off of n + 1, report);
    dst and dst_off None on CAPACITY."""
    parts = [(vtb if s else vals)[o:o + l] if st == R_OK else b""
             for st, s, o, l in zip(status, src, off, ln)]
    dst_off = [0]
    for p in parts:
        dst_off.append(dst_off[-1] + len(p))
    rep = {"status": OK, "nvalues": sum(st == R_OK for st in status), "dst_bytes": dst_off[-1]}
    if capacity is not None and dst_off[-1] > capacity:
        rep["status"] = CAPACITY
        return None, None, rep
    return b"".join(parts), dst_off, rep
