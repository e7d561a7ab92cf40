"""Damaged index, data and filter blocks for the point-lookup tests, made from
sound ones by edits in place (and, where an edit cannot do it, by
sst_finish_model.block_of). What a lookup must say of each comes from
tests/sst_get_model.py, which the clean fixtures pin to the reference. Test
code only."""
from __future__ import annotations

import struct

import sst_finish_model as fm
import sst_get_model as gm


def layout(block: bytes):
    """(restart offsets, restart array's offset, [(offset, shared, non_shared,
    value_length, delta offset)] of a sound block's entries)."""
    nr, limit = gm.restarts(block)
    rs = list(struct.unpack_from(f"<{nr}I", block, limit))
    ents, at = [], 0
    while at < limit:
        sh, ns, vl, kp = gm.decode_entry(block, at, limit)
        ents.append((at, sh, ns, vl, kp))
        at = kp + ns + vl
    return rs, limit, ents


def _patch(block: bytes, off: int, data: bytes) -> bytes:
    out = bytearray(block)
    out[off: off + len(data)] = data
    return bytes(out)


def _restart(block: bytes, i: int, value: int) -> bytes:
    _, limit, _ = layout(block)
    return _patch(block, limit + 4 * i, struct.pack("<I", value & 0xFFFFFFFF))


def block_damage(block: bytes) -> dict:
    """name -> damaged block, of a sound block with three restarts or more and
    a restart run of two entries or more somewhere (else the cases that need
    one are left out)."""
    rs, limit, ents = layout(block)
    nr = len(rs)
    out = {}
    mid = nr // 2
    out["restart shared != 0"] = _patch(block, rs[mid], b"\x01")
    out["first restart shared != 0"] = _patch(block, rs[0], b"\x01")
    for name, at in (("restart at the array", limit), ("restart 1 before the array", limit - 1),
                     ("restart 2 before the array", limit - 2),
                     ("restart 3 before the array", limit - 3),
                     ("restart past the array", limit + 4), ("restart far past", 0xFFFFFFF0)):
        out[name + ", middle"] = _restart(block, mid, at)
        out[name + ", last"] = _restart(block, nr - 1, at)
        out[name + ", first"] = _restart(block, 0, at)
    # in order, but into the middle of entries
    lying = block
    for i in range(1, nr):
        lying = _restart(lying, i, rs[i] + 1)
    out["lying restarts, mid-entry"] = lying
    out["lying restarts, one run late"] = b"".join(
        [block[:limit]] + [struct.pack("<I", rs[min(i + 1, nr - 1)]) for i in range(nr)] +
        [struct.pack("<I", nr)])
    out["lying restarts, all zero"] = block[:limit] + b"\0" * (4 * nr) + struct.pack("<I", nr)
    second = [e for e in ents if e[0] not in rs]
    if second:
        for k, e in enumerate((second[0], second[len(second) // 2], second[-1])):
            out[f"shared above the previous key {k}"] = _patch(block, e[0], b"\x7f")
    out["restart count 0"] = block[:-4] + struct.pack("<I", 0)
    out["restart count too large"] = block[:-4] + struct.pack("<I", (len(block) - 4) // 4 + 1)
    out["restart count huge"] = block[:-4] + struct.pack("<I", 0xFFFFFFFF)
    out["3 bytes"] = block[:3]
    out["4 bytes, count 0"] = struct.pack("<I", 0)
    out["empty"] = b""
    # an entry whose varint never ends, one whose value passes the array
    out["entry varint runs out"] = _patch(block, ents[len(ents) // 2][0], b"\x80" * 6)
    last = ents[-1]
    if last[3] < 127 and last[4] - last[0] == 3:
        out["last value passes the array"] = _patch(block, last[0] + 2, bytes([last[3] + 1]))
    return out


def index_bad_handles(index: bytes) -> dict:
    """Index blocks with a value that is no BlockHandle."""
    _, _, ents = layout(index)
    out = {}
    for name, e in (("first", ents[0]), ("last", ents[-1])):
        _, _, ns, vl, kp = e
        out[f"{name} value no handle"] = _patch(index, kp + ns, b"\x80" * vl)
    return out


def short_key_block(key_format_entries, restart_interval: int, short_at: int) -> bytes:
    """A block of the entries with entry short_at's key cut to 5 bytes (an
    internal key under 8 bytes)."""
    ents = [(k[:5] if i == short_at else k, v) for i, (k, v) in enumerate(key_format_entries)]
    return fm.block_of(ents, restart_interval)


def type_byte(block: bytes, entry: int, value: int) -> bytes:
    """The block with the type byte (the first of the last 8 key bytes) of an
    entry whose delta holds its whole tag set to `value`."""
    _, _, ents = layout(block)
    _, _, ns, _, kp = ents[entry]
    assert ns >= 8
    return _patch(block, kp + ns - 8, bytes([value]))


def filter_damage(filt: bytes) -> dict:
    """name -> damaged filter block; the edits are to the first filter."""
    n = len(filt)
    last_word = struct.unpack_from("<I", filt, n - 5)[0]
    num = (n - 5 - last_word) // 4
    offs = list(struct.unpack_from(f"<{num + 1}I", filt, last_word))
    out = {"4 bytes": filt[:4], "5 bytes": filt[-5:], "empty": b""}
    out["last_word too large"] = _patch(filt, n - 5, struct.pack("<I", n - 4))
    out["last_word huge"] = _patch(filt, n - 5, struct.pack("<I", 0xFFFFFFFF))
    out["start > limit"] = _patch(filt, last_word, struct.pack("<I", offs[1] + 1))
    out["limit past the offsets"] = _patch(filt, last_word + 4, struct.pack("<I", last_word + 1))
    if num >= 2:  # (the last filter's limit is last_word itself)
        out["start == limit past the offsets"] = _patch(
            filt, last_word, struct.pack("<II", last_word + 9, last_word + 9))
    out["empty filter"] = _patch(filt, last_word, struct.pack("<I", offs[1]))
    out["one byte filter"] = _patch(filt, last_word, struct.pack("<I", offs[1] - 1))
    out["k of 31"] = _patch(filt, offs[1] - 1, b"\x1f")
    out["k of 30"] = _patch(filt, offs[1] - 1, b"\x1e")
    out["k of 0"] = _patch(filt, offs[1] - 1, b"\x00")
    out["k of 255"] = _patch(filt, offs[1] - 1, b"\xff")
    out["base_lg 0"] = filt[:-1] + b"\x00"
    out["base_lg 3"] = filt[:-1] + b"\x03"
    out["base_lg 63"] = filt[:-1] + b"\x3f"
    out["base_lg 64"] = filt[:-1] + b"\x40"
    out["base_lg 255"] = filt[:-1] + b"\xff"
    return out
