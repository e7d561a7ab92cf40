"""Zstd frames from an explicit description (TEST INFRASTRUCTURE ONLY, CPU).

The library's encoders reach a small part of RFC 8878; the decoders promise
all of it. This module turns a description of a frame -- header fields, a
list of blocks, each compressed block's literals section and its sequences
with the coding of every table forced -- into bytes, on top of the coding
primitives of oracle/zstd_encoder.py. It makes no compression decision and
checks nothing about the frame's validity: an invalid description gives an
invalid frame, which is what the refusal cases need.

    f = frame([Raw(b"abcd"), Compressed(Literals.raw(b"xy"), [Seq(2, off(4), 5)])],
              fcs_bytes=2, window=0x08, checksum=True, content=b"...")

A sequence is (literal length, offset value, match length); the offset
value is the format's: 1-3 are the repeat codes, an offset n is n + 3
(`off(n)`). Tables are ("predefined",), ("rle",) or ("rle", symbol), ("fse",
normalised counts, accuracy log) and ("repeat",).
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import List, Optional, Sequence, Tuple

import zstd_encoder as ze
import zstd_oracle as zo

MAGIC = 0xFD2FB528
SKIPPABLE = 0x184D2A50
PREDEFINED, RLE, REPEAT = ("predefined",), ("rle",), ("repeat",)


def off(n: int) -> int:
    """The offset value of a real offset n."""
    return n + 3


def fse(norm: Sequence[int], log: int):
    return ("fse", list(norm), log)


# ---- frame header, skippable frames, assembly ------------------------------------

def frame_header(*, fcs_bytes: int = 1, content_size: int = 0, window: Optional[int] = None,
                 dict_bytes: int = 0, dict_id: int = 0, checksum: bool = False,
                 reserved: bool = False, unused: bool = False) -> bytes:
    """Magic, descriptor and the fields it announces. `window` is the window
    descriptor byte (None: single segment). fcs_bytes 1 needs a single
    segment, 0 a window; a 2-byte content size is written less its 256."""
    single = window is None
    assert fcs_bytes in (0, 1, 2, 4, 8) and (fcs_bytes != 1 or single) and (fcs_bytes or not single)
    fcs_flag = {0: 0, 1: 0, 2: 1, 4: 2, 8: 3}[fcs_bytes]
    did_flag = {0: 0, 1: 1, 2: 2, 4: 3}[dict_bytes]
    fhd = (fcs_flag << 6) | (single << 5) | (unused << 4) | (reserved << 3) | (checksum << 2) | \
        did_flag
    out = bytearray(MAGIC.to_bytes(4, "little"))
    out.append(fhd)
    if not single:
        out.append(window)
    out += dict_id.to_bytes(dict_bytes, "little")
    v = content_size - 256 if fcs_bytes == 2 else content_size
    out += v.to_bytes(fcs_bytes, "little")
    return bytes(out)


def checksum_of(content: bytes) -> bytes:
    import xxhash
    return (xxhash.xxh64(bytes(content), seed=0).intdigest() & 0xFFFFFFFF).to_bytes(4, "little")


def skippable(nibble: int, data: bytes = b"") -> bytes:
    return (SKIPPABLE + nibble).to_bytes(4, "little") + len(data).to_bytes(4, "little") + data


# ---- blocks --------------------------------------------------------------------

def block_header(last: bool, btype: int, size: int) -> bytes:
    return (int(last) | (btype << 1) | (size << 3)).to_bytes(3, "little")


@dataclass
class Raw:
    data: bytes


@dataclass
class Rle:
    byte: int
    n: int


@dataclass
class Bytes:
    """A block given as its header fields and payload, whatever they are."""
    btype: int
    size: int
    payload: bytes


@dataclass
class Literals:
    mode: str  # "raw", "rle", "huf" (tree + streams) or "treeless" (streams only)
    data: bytes  # the regenerated literals
    size_format: int  # the header's 2-bit Size_Format
    byte: int = 0  # rle: the byte (data = n of it)
    weights: str = "direct"  # huf: "direct" (4-bit) or "fse"
    max_bits: int = 11  # huf: the tree's depth limit
    tree_from: Optional[bytes] = None  # huf / treeless: the bytes the tree is built for

    @classmethod
    def raw(cls, data: bytes, size_format: Optional[int] = None):
        n = len(data)
        return cls("raw", bytes(data), size_format if size_format is not None
                   else ((n & 1) << 1 if n < 32 else 1 if n < 4096 else 3))

    @classmethod
    def rle(cls, byte: int, n: int, size_format: Optional[int] = None):
        return cls("rle", bytes([byte]) * n, size_format if size_format is not None
                   else ((n & 1) << 1 if n < 32 else 1 if n < 4096 else 3), byte=byte)

    @classmethod
    def huf(cls, data: bytes, size_format: int, **kw):
        return cls("huf", bytes(data), size_format, **kw)

    @classmethod
    def treeless(cls, data: bytes, size_format: int, **kw):
        return cls("treeless", bytes(data), size_format, **kw)


@dataclass
class Seq:
    ll: int
    ofv: int  # offset value: 1-3 repeat codes, offset + 3
    ml: int


@dataclass
class Compressed:
    literals: Literals
    seqs: List[Seq] = field(default_factory=list)
    ll: Tuple = PREDEFINED
    of: Tuple = PREDEFINED
    ml: Tuple = PREDEFINED
    count_bytes: Optional[int] = None  # width of the sequence count (None: the shortest)
    pad_bits: int = 0  # > 0: unread zero bits at the bitstream's start; < 0: that many cut off
    reserved_modes: int = 0  # the modes byte's two low bits
    tail: bytes = b""  # bytes after the section


class State:
    """What a later block of the frame may repeat (the encoder's side)."""

    def __init__(self):
        self.huf = None  # (nbBits, codes)
        self.ct = {"ll": None, "of": None, "ml": None}


def huf_tables(data: bytes, max_bits: int):
    """(nbBits[256], codes[256], max symbol, depth) of HUF_buildCTable for data's counts."""
    count = [0] * 256
    for b in data:
        count[b] += 1
    max_sym = max(data)
    nb, code, depth = ze.huf_build_ctable(count, max_sym, max_bits)
    return nb + [0] * (256 - len(nb)), code + [0] * (256 - len(code)), max_sym, depth


def huf_description(nb, max_sym: int, depth: int, how: str) -> bytes:
    """Huffman_Tree_Description: weights of symbols 0..max_sym-1, 4-bit or FSE."""
    weights = [depth + 1 - nb[s] if nb[s] else 0 for s in range(max_sym)]
    if how == "fse":
        body = ze._huf_compress_weights(weights)
        assert body is not None and 1 < len(body) < 128, "weights have no FSE form"
        return bytes([len(body)]) + body
    assert how == "direct" and 1 <= max_sym <= 128
    w = weights + [0]
    return bytes([127 + max_sym]) + bytes((w[i] << 4) | w[i + 1] for i in range(0, max_sym, 2))


def huf_streams(data: bytes, streams: int, nb, code) -> bytes:
    if streams == 1:
        return ze._huf_1x(data, nb, code)
    seg = (len(data) + 3) // 4
    enc = [ze._huf_1x(data[k * seg:(k + 1) * seg] if k < 3 else data[3 * seg:], nb, code)
           for k in range(4)]
    return b"".join(len(e).to_bytes(2, "little") for e in enc[:3]) + b"".join(enc)


def literals_section(lit: Literals, st: State) -> bytes:
    n, sf = len(lit.data), lit.size_format
    if lit.mode in ("raw", "rle"):
        t = 0 if lit.mode == "raw" else 1
        if sf in (0, 2):  # (one format bit: the field's high bit is the size's lowest)
            assert n < 32 and (n & 1) << 1 == sf
            h = bytes([t | (n << 3)])
        elif sf == 1:
            assert n < 4096
            h = (t | (1 << 2) | (n << 4)).to_bytes(2, "little")
        else:
            assert n < 1 << 20
            h = (t | (3 << 2) | (n << 4)).to_bytes(3, "little")
        return h + (lit.data if t == 0 else bytes([lit.byte]))
    head = b""
    if lit.mode == "huf" or st.huf is None:
        nb, code, max_sym, depth = huf_tables(lit.tree_from or lit.data, lit.max_bits)
        if lit.mode == "huf":
            head = huf_description(nb, max_sym, depth, lit.weights)
            st.huf = (nb, code)
    else:
        nb, code = st.huf
    assert all(nb[b] for b in set(lit.data)), "a literal outside the tree"
    body = head + huf_streams(lit.data, 1 if sf == 0 else 4, nb, code)
    bits = (10, 10, 14, 18)[sf]
    assert n < 1 << bits and len(body) < 1 << bits
    t = 2 if lit.mode == "huf" else 3
    return (t | (sf << 2) | (n << 4) | (len(body) << (4 + bits))).to_bytes((3, 3, 4, 5)[sf],
                                                                           "little") + body


_DEFAULTS = {"ll": (ze.LL_DEFAULT_NORM, ze.MAX_LL, ze.LL_DEFAULT_LOG),
             "of": (ze.OF_DEFAULT_NORM, ze.DEFAULT_MAX_OFF, ze.OF_DEFAULT_LOG),
             "ml": (ze.ML_DEFAULT_NORM, ze.MAX_ML, ze.ML_DEFAULT_LOG)}


def _table(key: str, mode, codes, st: State):
    """(mode number, description bytes, FseCTable) of one of LL / OF / ML."""
    kind = mode[0]
    if kind == "predefined":
        norm, mx, log = _DEFAULTS[key]
        return 0, b"", ze.FseCTable(norm, mx, log)
    if kind == "rle":
        sym = mode[1] if len(mode) > 1 else codes[0]
        return 1, bytes([sym]), ze.FseCTable.rle(max(codes))
    if kind == "fse":
        norm, log = mode[1], mode[2]
        assert all(norm[c] for c in codes), "a code the table gives no state"
        return 2, ze.fse_write_ncount(norm, len(norm) - 1, log), \
            ze.FseCTable(norm, len(norm) - 1, log)
    assert kind == "repeat"
    ct = st.ct[key]
    if ct is None:  # (nothing to repeat: coded under the predefined table)
        norm, mx, log = _DEFAULTS[key]
        ct = ze.FseCTable(norm, mx, log)
    return 3, b"", ct


def seq_count(n: int, width: Optional[int] = None) -> bytes:
    if width is None:
        width = 1 if n < 128 else 2 if n < ze.LONGNBSEQ else 3
    if width == 1:
        assert n < 128
        return bytes([n])
    if width == 2:
        assert n < ze.LONGNBSEQ
        return bytes([(n >> 8) + 0x80, n & 255])
    return b"\xff" + (n - ze.LONGNBSEQ).to_bytes(2, "little")


def sequences_section(b: Compressed, st: State) -> bytes:
    out = bytearray(seq_count(len(b.seqs), b.count_bytes))
    if not b.seqs:
        return bytes(out) + b.tail
    llc = [ze.ll_code(s.ll) for s in b.seqs]
    mlc = [ze.ml_code(s.ml - 3) for s in b.seqs]
    ofc = [ze.highbit(s.ofv) for s in b.seqs]
    tabs = [_table(k, m, c, st) for k, m, c in (("ll", b.ll, llc), ("of", b.of, ofc),
                                                ("ml", b.ml, mlc))]
    out.append((tabs[0][0] << 6) | (tabs[1][0] << 4) | (tabs[2][0] << 2) | b.reserved_modes)
    for key, (_, desc, ct) in zip(("ll", "of", "ml"), tabs):
        out += desc
        st.ct[key] = ct
    sq = [(s.ll - zo.LL_BASE[lc], s.ofv, s.ml - zo.ML_BASE[mc])
          for s, lc, mc in zip(b.seqs, llc, mlc)]
    stream = ze.encode_sequences(sq, llc, ofc, mlc, tabs[0][2], tabs[1][2], tabs[2][2])
    if b.pad_bits:
        v = int.from_bytes(stream, "little")
        nbits = v.bit_length() - 1  # (below the end mark)
        v &= (1 << nbits) - 1
        if b.pad_bits > 0:
            v, nbits = v << b.pad_bits, nbits + b.pad_bits
        else:
            assert v & ((1 << -b.pad_bits) - 1) == 0, "the cut bits are not zeros"
            v, nbits = v >> -b.pad_bits, nbits + b.pad_bits
        v |= 1 << nbits
        stream = v.to_bytes(nbits // 8 + 1, "little")
    return bytes(out) + stream + b.tail


def blocks_bytes(blocks, last_flags: Optional[Sequence[bool]] = None) -> bytes:
    """The blocks one after another; the last one carries the last-block flag
    unless last_flags gives every block's."""
    st = State()
    out = bytearray()
    for i, b in enumerate(blocks):
        last = last_flags[i] if last_flags is not None else i == len(blocks) - 1
        if isinstance(b, Raw):
            out += block_header(last, 0, len(b.data)) + b.data
        elif isinstance(b, Rle):
            out += block_header(last, 1, b.n) + bytes([b.byte])
        elif isinstance(b, Bytes):
            out += block_header(last, b.btype, b.size) + b.payload
        else:
            body = literals_section(b.literals, st) + sequences_section(b, st)
            out += block_header(last, 2, len(body)) + body
    return bytes(out)


def frame(blocks, *, content: Optional[bytes] = None, content_size: Optional[int] = None,
          checksum=False, last_flags=None, **header) -> bytes:
    """One frame. The content size written is content_size, else len(content);
    checksum is False, True (of `content`) or the four bytes to write."""
    if content_size is None and header.get("fcs_bytes", 1):
        content_size = len(content)
    out = frame_header(content_size=content_size or 0, checksum=checksum is not False, **header)
    out += blocks_bytes(blocks, last_flags)
    if checksum is not False:
        out += checksum_of(content) if checksum is True else bytes(checksum)
    return out
