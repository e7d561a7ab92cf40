"""The inputs of the any-size write path's tests (tests/test_write_any_size.py,
tests/test_codec_reuse_and_bounds.py) and the oracle's frames of them, cached
for all of those; rebuilt from seeds: the generator of the library pins
(tests/golden/gen_zstd_write_big.py), the tests and the CPU emulator's check
(tools/simt_emu/zstdc_check.py) all take them from here, so that a pinned
hash, a device frame and an emulated frame speak of the same bytes.
"""
from __future__ import annotations

import functools

import numpy as np

LEVELS = (1, 2, -1, -5)
BENCH_SIZES = (20481, 32768, 32769, 65535, 65536, 65537, 65791, 65792, 131071, 131072)


@functools.lru_cache(maxsize=1)
def bench() -> bytes:
    from tools.db_bench_data import block_batch
    return block_batch(40).tobytes()


@functools.lru_cache(maxsize=1)
def edge_blocks():
    """[(name, bytes)]: every place where a 16-bit field of the <= 20 KiB
    kernel would overflow, and the small blocks that ride along."""
    b = bench()
    rng = np.random.default_rng(7)

    def rand(n):
        return rng.integers(0, 256, n, dtype=np.uint8).tobytes()

    out = [(f"bench{n}", b[:n]) for n in BENCH_SIZES]
    out.append(("long_match", bytes(131072)))                        # a match > 65,538
    out.append(("long_literals", b[:30000] + rand(66000) + b[:30000]))  # a literal run >= 65,536
    out.append(("literals_then_match", rand(70000) + bytes(58000)))
    out.append(("periodic", (b"abcdefg" * 20000)[:131072]))
    out.append(("skewed", np.minimum(rng.geometric(0.6, 131072) - 1, 255).astype(np.uint8).tobytes()))
    out.append(("random", rand(131072)))                             # raw block, 4-byte content size
    out += [("empty", b""), ("abc", b"abc"), ("bench4096", b[:4096]), ("bench20480", b[:20480])]
    return out


def edge(name: str) -> bytes:
    return dict(edge_blocks())[name]


@functools.lru_cache(maxsize=None)
def frame(x: bytes, level: int) -> bytes:
    """The oracle's frame, computed once per (block, level) for all tests."""
    import zstd_encoder as ze
    return ze.compress(x, level)


@functools.lru_cache(maxsize=1)
def reuse_pool():
    """[(name, bytes)]: the distinct big blocks of the reuse tests
    (tests/test_codec_reuse_and_bounds.py): the 16 big edge blocks, whose
    frames test_edge_blocks computes anyway, and 24 blocks of 20,481-40,000
    bytes, cheap for the oracle."""
    out = [(n, x) for n, x in edge_blocks() if len(x) > 20480]
    out += [(f"fuzz{k}_{len(x)}", x)
            for k, x in enumerate(fuzz_inputs(np.random.default_rng(11), 24, 20481, 40000))]
    return out


@functools.lru_cache(maxsize=1)
def reuse_sequence():
    """[(name, bytes)]: what one emulated workgroup pulls in a row
    (tools/simt_emu/zstdc_check.py reuse): long then short, compressible, the
    raw exit (random) and all-zero in turn, blocks of the first kernel in
    between. Under 200 KiB in all: the emulator takes 0.15 s a KiB."""
    b = bench()
    rng = np.random.default_rng(13)

    def rand(n):
        return rng.integers(0, 256, n, dtype=np.uint8).tobytes()

    skewed = np.minimum(rng.geometric(0.6, 34000) - 1, 255).astype(np.uint8).tobytes()
    out = [("bench40000", b[:40000]), ("abc", b"abc"), ("random20481", rand(20481)),
           ("zeros32769", bytes(32769)), ("empty", b""), ("skewed34000", skewed),
           ("bench4096", b[:4096]), ("random21000", rand(21000)),
           ("periodic30000", (b"abcdefg" * 5000)[:30000]), ("bench20481", b[:20481])]
    assert sum(len(x) for _, x in out) <= 200 * 1024
    return out


def fuzz_inputs(rng, count, lo, hi):
    """The six content kinds of tests/test_zstd_write.py's _fuzz_inputs, with
    lengths drawn uniformly from [lo, hi]."""
    from tools.db_bench_data import block_batch
    bb = block_batch(64).tobytes()
    out = []
    for k in range(count):
        n = int(rng.integers(lo, hi + 1))
        kind = k % 6
        if kind == 0:
            s = int(rng.integers(0, len(bb) - n))
            out.append(bb[s:s + n])
        elif kind == 1:
            out.append(rng.integers(0, 256, n, dtype=np.uint8).tobytes())
        elif kind == 2:
            out.append(rng.integers(0, int(rng.integers(1, 20)), n, dtype=np.uint8).tobytes())
        elif kind == 3:
            p = float(rng.uniform(0.3, 0.7))
            out.append(np.minimum(rng.geometric(p, n) - 1, 255).astype(np.uint8).tobytes())
        elif kind == 4:
            base = rng.integers(0, 256, int(rng.integers(1, 64)), dtype=np.uint8).tobytes()
            x = bytearray((base * (n // len(base) + 1))[:n])
            for _ in range(int(rng.integers(0, 20))):
                x[int(rng.integers(0, n))] = int(rng.integers(0, 256))
            out.append(bytes(x))
        else:
            ent = bytearray()
            i = 0
            while len(ent) < n:
                ent += bytes([0, 16, int(rng.integers(1, 100))]) + f"key{i:013d}".encode() + \
                    rng.integers(0, 256, int(rng.integers(0, 100)), dtype=np.uint8).tobytes()
                i += 1
            out.append(bytes(ent[:n]))
    return out
