"""CPU model of TableBuilder::Flush + Finish (table/table_builder.cc:104-268)
from finished data blocks: TEST INFRASTRUCTURE, the expectation of
tests/test_sst_write_table.py for lvkv_sst_write_table_device.

Input: the data blocks in key order, each the bytes BlockBuilder::Finish
returns. Output: the whole table image. WriteBlock of every block (data,
metaindex, index) is snappy_oracle.write_blocks; the rest restates

  filter block   table/filter_block.cc (kFilterBaseLg 11), util/bloom.cc,
                 util/hash.cc
  metaindex      table_builder.cc:231-246
  index block    restart interval 1; separators by util/comparator.cc:30-66
                 (key_format 0) or db/dbformat.cc:65-97 over them (1)
  footer         table/format.cc:33-46

It is pinned, not trusted: test_model_reproduces_* rebuild tables the
reference's TableBuilder wrote (tests/golden/table.sst, finish_*.sst) from
their data blocks alone, byte for byte.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import List, Optional, Tuple

import snappy_oracle as so

FILTER_BASE_LG = 11
MAGIC = 0xDB4775248B80FB57
POLICY = b"leveldb.BuiltinBloomFilter2"
SEEK_TAG = bytes([1]) + b"\xff" * 7  # PackSequenceAndType(kMaxSequenceNumber, kValueTypeForSeek)
ZSTD_OK, ZSTD_TOO_LARGE = 0, 4
ZSTD_BIG_MAX = 128 << 10  # the device compressor's longest block


def varint(v: int) -> bytes:
    out = bytearray()
    while v >= 128:
        out.append((v & 127) | 128)
        v >>= 7
    out.append(v)
    return bytes(out)


def _get_varint32(b: bytes, p: int, limit: int) -> Tuple[int, int]:
    v = 0
    for i in range(5):
        if p + i >= limit:
            break
        c = b[p + i]
        v |= (c & 127) << (7 * i)
        if c < 128:
            return v & 0xFFFFFFFF, p + i + 1
    raise ValueError("bad varint")


def block_keys(block: bytes) -> List[bytes]:
    """Every key of a block, in order (Block::Iter over the entries)."""
    block = bytes(block)
    nr = int.from_bytes(block[-4:], "little")
    limit = len(block) - 4 - 4 * nr
    keys, key, p = [], b"", 0
    while p < limit:
        sh, p = _get_varint32(block, p, limit)
        ns, p = _get_varint32(block, p, limit)
        vl, p = _get_varint32(block, p, limit)
        key = key[:sh] + block[p:p + ns]
        keys.append(key)
        p += ns + vl
    assert p == limit
    return keys


def bloom_hash(key: bytes) -> int:
    """Hash(key, 0xbc9f1d34) (util/hash.cc)."""
    m, n = 0xC6A4A793, len(key)
    h = (0xBC9F1D34 ^ (n * m)) & 0xFFFFFFFF
    i = 0
    while i + 4 <= n:
        h = (h + int.from_bytes(key[i:i + 4], "little")) & 0xFFFFFFFF
        h = (h * m) & 0xFFFFFFFF
        h ^= h >> 16
        i += 4
    rem = n - i
    if rem == 3:
        h = (h + (key[i + 2] << 16)) & 0xFFFFFFFF
    if rem >= 2:
        h = (h + (key[i + 1] << 8)) & 0xFFFFFFFF
    if rem >= 1:
        h = (h + key[i]) & 0xFFFFFFFF
        h = (h * m) & 0xFFFFFFFF
        h ^= h >> 24
    return h


def bloom_k(bits_per_key: int) -> int:
    return max(1, min(30, int(bits_per_key * 0.69)))


def bloom_filter(keys: List[bytes], bits_per_key: int) -> bytes:
    """BloomFilterPolicy::CreateFilter (util/bloom.cc:29-55) for n > 0 keys."""
    k = bloom_k(bits_per_key)
    nbytes = (max(64, len(keys) * bits_per_key) + 7) // 8
    bits = nbytes * 8
    arr = bytearray(nbytes)
    for key in keys:
        h = bloom_hash(key)
        delta = ((h >> 17) | (h << 15)) & 0xFFFFFFFF
        for _ in range(k):
            pos = h % bits
            arr[pos // 8] |= 1 << (pos % 8)
            h = (h + delta) & 0xFFFFFFFF
    return bytes(arr) + bytes([k])


def filter_block(block_keys_: List[List[bytes]], ends: List[int], bits_per_key: int) -> Tuple[bytes, int]:
    """FilterBlockBuilder over the blocks' keys; ends[i] = the file offset
    after block i's trailer (StartBlock's argument). (contents, filters)."""
    result, offsets, pending = bytearray(), [], []

    def generate():
        offsets.append(len(result))
        if pending:
            result.extend(bloom_filter(pending, bits_per_key))
            pending.clear()

    for keys, e in zip(block_keys_, ends):
        pending.extend(keys)
        while (e >> FILTER_BASE_LG) > len(offsets):
            generate()
    if pending:
        generate()
    array_at = len(result)
    for o in offsets:
        result += o.to_bytes(4, "little")
    result += array_at.to_bytes(4, "little")
    result.append(FILTER_BASE_LG)
    return bytes(result), len(offsets)


def _separator(start: bytes, limit: bytes) -> bytes:
    m = min(len(start), len(limit))
    d = 0
    while d < m and start[d] == limit[d]:
        d += 1
    if d < m and start[d] < 0xFF and start[d] + 1 < limit[d]:
        return start[:d] + bytes([start[d] + 1])
    return start


def _successor(key: bytes) -> bytes:
    for i, c in enumerate(key):
        if c != 0xFF:
            return key[:i] + bytes([c + 1])
    return key


def index_key(last: bytes, nxt: Optional[bytes], key_format: int) -> bytes:
    """FindShortestSeparator(last, nxt), or FindShortSuccessor(last) at the
    end of the table (nxt None)."""
    if key_format == 0:
        return _separator(last, nxt) if nxt is not None else _successor(last)
    user = last[:-8]
    tmp = _separator(user, nxt[:-8]) if nxt is not None else _successor(user)
    return tmp + SEEK_TAG if len(tmp) < len(user) else last


def block_of(entries: List[Tuple[bytes, bytes]], restart_interval: int) -> bytes:
    """BlockBuilder (table/block_builder.cc)."""
    out, restarts, last, counter = bytearray(), [0], b"", 0
    for key, value in entries:
        shared = 0
        if counter < restart_interval:
            m = min(len(last), len(key))
            while shared < m and last[shared] == key[shared]:
                shared += 1
        else:
            restarts.append(len(out))
            counter = 0
        out += varint(shared) + varint(len(key) - shared) + varint(len(value))
        out += key[shared:] + value
        last = key
        counter += 1
    for r in restarts:
        out += r.to_bytes(4, "little")
    out += len(restarts).to_bytes(4, "little")
    return bytes(out)


@dataclass
class Table:
    image: bytes
    handles: List[Tuple[int, int]]  # the data blocks'
    types: List[int]
    report: dict = field(default_factory=dict)
    index_contents: bytes = b""
    meta_contents: bytes = b""


def _write(raws, compression, file_offset, zstd_level, device_limits):
    """write_blocks; with device_limits, a zstd block past the device
    compressor's bound stays raw and is reported TOO_LARGE."""
    out, handles, types, status = bytearray(), [], [], []
    for raw in raws:
        big = device_limits and compression == 2 and len(raw) > ZSTD_BIG_MAX
        b, h, t = so.write_blocks([raw], 0 if big else compression, file_offset + len(out),
                                  zstd_level)
        out += b
        handles += h
        types += t
        status.append(ZSTD_TOO_LARGE if big else ZSTD_OK)
    return bytes(out), handles, types, status


def finish(data_blocks, key_format: int = 1, bits_per_key: int = 10, compression: int = 0,
           zstd_level: int = 1, device_limits: bool = False) -> Table:
    data_blocks = [bytes(b) for b in data_blocks]
    img, handles, types, _ = _write(data_blocks, compression, 0, zstd_level, device_limits)
    img = bytearray(img)
    data_end = len(img)
    keys = [block_keys(b) for b in data_blocks]
    rep = {"status": 0, "first_bad_block": 0xFFFFFFFF, "num_entries": sum(map(len, keys)),
           "nfilters": 0, "data_end": data_end, "filter_offset": 0, "filter_size": 0}
    meta_entries = []
    if bits_per_key:
        fkeys = [[k[:-8] for k in ks] for ks in keys] if key_format == 1 else keys
        ends = [o + s + 5 for o, s in handles]
        fb, rep["nfilters"] = filter_block(fkeys, ends, bits_per_key)
        b, h, _ = so.write_blocks([fb], 0, data_end)
        img += b
        rep["filter_offset"], rep["filter_size"] = h[0]
        meta_entries.append((b"filter." + POLICY, varint(h[0][0]) + varint(h[0][1])))
    index_entries = []
    for i, (o, s) in enumerate(handles):
        nxt = keys[i + 1][0] if i + 1 < len(handles) else None
        index_entries.append((index_key(keys[i][-1], nxt, key_format), varint(o) + varint(s)))
    meta, index = block_of(meta_entries, 16), block_of(index_entries, 1)
    b, h, t, st = _write([meta, index], compression, len(img), zstd_level, device_limits)
    img += b
    rep.update(meta_offset=h[0][0], meta_size=h[0][1], index_offset=h[1][0], index_size=h[1][1],
               meta_type=t[0], index_type=t[1], meta_status=st[0], index_status=st[1])
    footer = varint(h[0][0]) + varint(h[0][1]) + varint(h[1][0]) + varint(h[1][1])
    img += footer.ljust(40, b"\0") + MAGIC.to_bytes(8, "little")
    rep["file_size"] = len(img)
    return Table(bytes(img), handles, types, rep, index, meta)
