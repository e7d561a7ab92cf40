"""Table::InternalGet in plain Python (table/table.cc:214-242): Block::Iter::Seek
on a fresh iterator (table/block.cc:165-228), FilterBlockReader
(table/filter_block.cc:77-104), BloomFilterPolicy::KeyMayMatch
(util/bloom.cc:56-80) and SaveValue (db/version_set.cc:263-276), with the
verdicts of lvkv_sst_get_locate_device / lvkv_sst_get_seek_device. The model
of tests/test_sst_get.py, held to the reference by tests/test_sst_get_model.py.
Test code only.
"""
from __future__ import annotations

import struct

NONE = 0xFFFFFFFF
# d_q_status
BLOCK, PAST_END, FILTERED, INDEX_CORRUPT, BAD_HANDLE, BAD_KEY = range(6)
# d_state
NOT_FOUND, FOUND, DELETED, CORRUPT_KEY, BAD_BLOCK, BAD_ENTRY, UNREADABLE, STATE_BAD_KEY = range(8)
# a seek's verdict
VALID, END, CORRUPT, BAD = "valid", "end", "corrupt", "bad block"


def varint(b: bytes, p: int, limit: int, max_shift: int):
    """GetVarint32Ptr / GetVarint64Ptr over b[p:limit]: (value, next) or None."""
    result, shift = 0, 0
    while shift <= max_shift and p < limit:
        byte = b[p]
        p += 1
        if byte & 128:
            result |= (byte & 127) << shift
        else:
            return result | (byte << shift), p
        shift += 7
    return None


def decode_entry(b: bytes, p: int, limit: int):
    """DecodeEntry (table/block.cc:55-75) over b[p:limit], the sum taken in 64
    bits: (shared, non_shared, value_length, key delta's offset) or None."""
    if limit - p < 3:
        return None
    out = []
    for _ in range(3):
        r = varint(b, p, limit, 28)
        if r is None:
            return None
        v, p = r
        out.append(v & 0xFFFFFFFF)
    if limit - p < out[1] + out[2]:
        return None
    return out[0], out[1], out[2], p


def tag_of(key: bytes) -> int:
    return struct.unpack("<Q", key[-8:])[0]


def compare(key_format: int, a: bytes, b: bytes) -> int:
    """BytewiseComparator, or InternalKeyComparator (db/dbformat.cc:47-63)."""
    if key_format == 1:
        ua, ub = a[:-8], b[:-8]
        if ua != ub:
            return -1 if ua < ub else 1
        ta, tb = tag_of(a), tag_of(b)
        return -1 if ta > tb else 1 if ta < tb else 0
    return -1 if a < b else 1 if a > b else 0


def restarts(block: bytes):
    """Block::Block + NewIterator: BAD, (0, 0) for the empty iterator, or
    (restart count, restart array's offset)."""
    n = len(block)
    if n < 4:
        return BAD
    nr = struct.unpack_from("<I", block, n - 4)[0]
    if nr > (n - 4) // 4:
        return BAD
    return nr, n - 4 - 4 * nr


def seek(block: bytes, target: bytes, key_format: int) -> dict:
    """Seek(target) on a fresh iterator: verdict, and for VALID the entry's
    offset, key, and value position in the block."""
    r = restarts(block)
    if r == BAD:
        return {"verdict": BAD}
    nr, limit = r
    if nr == 0:
        return {"verdict": END}

    def restart(i):
        return struct.unpack_from("<I", block, limit + 4 * i)[0]

    left, right = 0, nr - 1
    while left < right:
        mid = (left + right + 1) // 2
        ro = restart(mid)
        e = decode_entry(block, ro, limit) if ro <= limit else None
        if e is None or e[0] != 0:
            return {"verdict": CORRUPT}
        key = block[e[3]: e[3] + e[1]]
        if key_format == 1 and len(key) < 8:
            return {"verdict": CORRUPT}
        if compare(key_format, key, target) < 0:
            left = mid
        else:
            right = mid - 1
    at, key, steps = restart(left), b"", 0
    while True:
        if at >= limit:
            return {"verdict": END}
        e = decode_entry(block, at, limit)
        if e is None or e[0] > len(key):
            return {"verdict": CORRUPT}
        shared, ns, vl, kp = e
        key = key[:shared] + block[kp: kp + ns]
        if key_format == 1 and len(key) < 8:
            return {"verdict": CORRUPT}
        steps += 1
        if compare(key_format, key, target) >= 0:
            return {"verdict": VALID, "off": at, "key": key, "val_off": kp + ns, "val_len": vl,
                    "left": left, "steps": steps}
        at = kp + ns + vl


def forward_ordinal(block: bytes, off: int) -> int:
    """The entries SeekToFirst + Next hand out before the one at `off`, NONE
    when that walk does not come by it."""
    nr, limit = restarts(block)
    at, klen, n = struct.unpack_from("<I", block, limit)[0], 0, 0
    while at < off and at < limit:
        e = decode_entry(block, at, limit)
        if e is None or e[0] > klen:
            return NONE
        klen = e[0] + e[1]
        at = e[3] + e[1] + e[2]
        n += 1
    return n if at == off else NONE


def bloom_hash(data: bytes) -> int:
    """Hash (util/hash.cc) with BloomHash's seed."""
    m, n = 0xC6A4A793, len(data)
    h = (0xBC9F1D34 ^ (n * m)) & 0xFFFFFFFF
    i = 0
    while i + 4 <= n:
        h = (h + struct.unpack_from("<I", data, i)[0]) & 0xFFFFFFFF
        h = (h * m) & 0xFFFFFFFF
        h ^= h >> 16
        i += 4
    rem = n - i
    if rem == 3:
        h = (h + (data[i + 2] << 16)) & 0xFFFFFFFF
    if rem >= 2:
        h = (h + (data[i + 1] << 8)) & 0xFFFFFFFF
    if rem >= 1:
        h = (h + data[i]) & 0xFFFFFFFF
        h = (h * m) & 0xFFFFFFFF
        h ^= h >> 24
    return h


def bloom_may_match(key: bytes, f: bytes) -> bool:
    if len(f) < 2:
        return False
    bits = (len(f) - 1) * 8
    k = f[-1]
    if k > 30:
        return True
    h = bloom_hash(key)
    delta = ((h >> 17) | (h << 15)) & 0xFFFFFFFF
    for _ in range(k):
        bitpos = h % bits
        if not f[bitpos // 8] & (1 << (bitpos % 8)):
            return False
        h = (h + delta) & 0xFFFFFFFF
    return True


def filter_may_match(f: bytes, block_offset: int, key: bytes) -> bool:
    n = len(f)
    if n < 5:
        return True
    base_lg = f[n - 1]
    last_word = struct.unpack_from("<I", f, n - 5)[0]
    if last_word > n - 5:
        return True
    num = (n - 5 - last_word) // 4
    index = block_offset >> base_lg if base_lg < 64 else 0
    if index < num:
        start, limit = struct.unpack_from("<II", f, last_word + 4 * index)
        if start <= limit <= last_word:
            return bloom_may_match(key, f[start:limit])
        if start == limit:
            return False
    return True


def decode_handle(v: bytes):
    """BlockHandle::DecodeFrom: (offset, size) or None."""
    r = varint(v, 0, len(v), 63)
    if r is None:
        return None
    off, p = r
    r = varint(v, p, len(v), 63)
    if r is None:
        return None
    return off & (2**64 - 1), r[0] & (2**64 - 1)


def locate(index: bytes, filt, q: bytes, key_format: int):
    """(status, block, handle offset, handle size) of lvkv_sst_get_locate_device;
    filt None: no policy."""
    if key_format == 1 and len(q) < 8:
        return BAD_KEY, NONE, 0, 0
    s = seek(index, q, key_format)
    if s["verdict"] == END:
        return PAST_END, NONE, 0, 0
    if s["verdict"] != VALID:
        return INDEX_CORRUPT, NONE, 0, 0
    block = forward_ordinal(index, s["off"])
    h = decode_handle(index[s["val_off"]: s["val_off"] + s["val_len"]])
    if h is None or h[1] > 0xFFFFFFFF:
        return BAD_HANDLE, block, 0, 0
    user = q[:-8] if key_format == 1 else q
    if filt is not None and not filter_may_match(filt, h[0], user):
        return FILTERED, block, h[0], h[1]
    return BLOCK, block, h[0], h[1]


def seek_query(block, q: bytes, key_format: int, *, readable: bool = True):
    """(state, hit_off, value offset in the block, value length, tag) of
    lvkv_sst_get_seek_device for one query; block None: no slot."""
    if key_format == 1 and len(q) < 8:
        return STATE_BAD_KEY, NONE, 0, 0, 0
    if block is None:
        return NOT_FOUND, NONE, 0, 0, 0
    if not readable:
        return UNREADABLE, NONE, 0, 0, 0
    s = seek(block, q, key_format)
    if s["verdict"] == BAD:
        return BAD_BLOCK, NONE, 0, 0, 0
    if s["verdict"] == CORRUPT:
        return BAD_ENTRY, NONE, 0, 0, 0
    if s["verdict"] == END:
        return NOT_FOUND, NONE, 0, 0, 0
    key, state, tag = s["key"], NOT_FOUND, 0
    if key_format == 0:
        if key == q:
            state = FOUND
    else:
        tag = tag_of(key)
        if tag & 0xFF > 1:
            state = CORRUPT_KEY
        elif key[:-8] == q[:-8]:
            state = FOUND if tag & 0xFF == 1 else DELETED
    return state, s["off"], s["val_off"], s["val_len"], tag
