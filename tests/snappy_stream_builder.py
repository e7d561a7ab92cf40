"""Snappy streams from explicit elements (TEST INFRASTRUCTURE ONLY, CPU).

libsnappy's compressor writes the shortest form of every element and, for
blocks of 64 KiB or less, never a copy with a 4-byte offset; its decoder
takes every form. These helpers write each element exactly as asked and
check nothing: `stream(preamble(n, width), lit(b"abc", 4), copy4(3, 7))`.
"""
from __future__ import annotations


def preamble(n: int, width: int = 0) -> bytes:
    """The uncompressed length as a varint of `width` bytes (0: the shortest);
    a wider one carries continuation bits over zero groups."""
    out = bytearray()
    while n >= 128 or len(out) + 1 < width:
        out.append((n & 127) | 128)
        n >>= 7
    out.append(n)
    assert not width or len(out) == width
    return bytes(out)


def lit(data: bytes, length_bytes: int = 0) -> bytes:
    """A literal whose length is in the tag (0; at most 60 bytes) or in
    length_bytes (1-4) bytes after it."""
    n = len(data) - 1
    if length_bytes == 0:
        assert 0 <= n < 60
        return bytes([n << 2]) + data
    return lit_header(len(data), length_bytes) + data


def lit_header(length: int, length_bytes: int) -> bytes:
    """The tag and length bytes of a literal of `length` bytes, without them."""
    return bytes([(59 + length_bytes) << 2]) + (length - 1).to_bytes(length_bytes, "little")


def copy1(offset: int, length: int) -> bytes:
    assert 4 <= length <= 11 and 0 <= offset < 2048
    return bytes([1 | ((length - 4) << 2) | ((offset >> 8) << 5), offset & 255])


def copy2(offset: int, length: int) -> bytes:
    assert 1 <= length <= 64 and 0 <= offset < 1 << 16
    return bytes([2 | ((length - 1) << 2)]) + offset.to_bytes(2, "little")


def copy4(offset: int, length: int) -> bytes:
    assert 1 <= length <= 64 and 0 <= offset < 1 << 32
    return bytes([3 | ((length - 1) << 2)]) + offset.to_bytes(4, "little")


def stream(*parts: bytes) -> bytes:
    return b"".join(parts)
