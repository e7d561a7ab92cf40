"""Generates tests/golden/snappy_foreign.{json,bin}: Snappy streams libsnappy's
compressor never writes for blocks of 64 KiB or less but its decoder takes
(copies with 4-byte offsets, literals with longer length fields than they
need, short copy-2 elements, wide preambles) and their refused neighbours,
built with tests/snappy_stream_builder.py, each with libsnappy 1.1.8's own
verdict through so.lib_uncompress (0 decoded, 1 bad length, 2 bad contents),
the output's length and its sha256.

    python tests/golden/gen_snappy_foreign.py

Each entry carries feature tags and a guess, as in gen_zstd_foreign.py; the
library's answer is the expectation and the summary lists every guess it
contradicts.
"""
from __future__ import annotations

import hashlib
import json
import sys
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
REPO = HERE.parent.parent
for p in (REPO / "tests", REPO / "oracle"):
    sys.path.insert(0, str(p))
import snappy_oracle as so  # noqa: E402
from snappy_stream_builder import (copy1, copy2, copy4, lit, lit_header, preamble,  # noqa: E402
                                   stream)

A, R, U = "accept", "reject", "unknown"


def cases():
    """[(name, tags, guess, stream)] in a fixed order."""
    rng = np.random.default_rng(20261021)
    out = []

    def rnd(n):
        return rng.integers(0, 256, n, dtype=np.uint8).tobytes()

    def add(name, tags, guess, s):
        assert all(name != c[0] for c in out), name
        out.append((name, sorted(set(tags)), guess, bytes(s)))

    def grown(n):
        """Elements that produce n bytes of period 59 (a 59-byte literal, then
        copy-2 elements of its own offset)."""
        parts, have = [lit(rnd(59))], 59
        while have < n:
            k = min(59, n - have)
            parts.append(copy2(59, k))
            have += k
        return b"".join(parts)

    # copies with a 4-byte offset
    for total, offs in ((300, (1, 255, 256, 300)), (70000, (1, 255, 256, 65535, 65536, 70000))):
        base = grown(total)
        for o in offs:
            add(f"copy4_off{o}_at{total}", ["copy4"] + (["copy4_far"] if o >= 65536 else []) +
                (["copy4_all"] if o == total else []), A,
                stream(preamble(total + 33 + 2), base, copy4(o, 33), lit(b"zz")))
        add(f"copy4_past_at{total}", ["copy4_past"], R,
            stream(preamble(total + 33), base, copy4(total + 1, 33)))
        add(f"copy4_zero_at{total}", ["copy4_zero"], R,
            stream(preamble(total + 33), base, copy4(0, 33)))
    add("copy4_high_bytes", ["copy4_past"], R,
        stream(preamble(300 + 20), grown(300), copy4(0x10000 + 5, 20)))
    add("copy4_top_byte", ["copy4_past"], R,
        stream(preamble(300 + 20), grown(300), copy4(0x01000000 + 5, 20)))
    add("copy4_every_length", ["copy4"], A,
        stream(preamble(40 + sum(range(1, 65))), lit(rnd(40)),
               *[copy4(1 + k % 40, k) for k in range(1, 65)]))
    add("copy4_cut", ["copy4_cut"], R, stream(preamble(45), lit(rnd(40)), copy4(3, 5)[:4]))

    # literals with longer length fields than they need
    for w in (1, 2, 3, 4):
        add(f"lit_len{w}_1_to_60", [f"lit_len{w}"], A,
            stream(preamble(sum(range(1, 61))), *[lit(rnd(n), w) for n in range(1, 61)]))
        for n in (1, 60, 61, 300):
            if n <= 256 ** w:
                add(f"lit_len{w}_n{n}", [f"lit_len{w}"], A, stream(preamble(n), lit(rnd(n), w)))
    # (lengths whose third byte is not zero: longer than any literal libsnappy writes)
    add("lit_len3_n65800", ["lit_len3", "lit_len_big"], A,
        stream(preamble(65800 + 4), lit(b"head"), lit(rnd(65800), 3)))
    add("lit_len4_n66000", ["lit_len4", "lit_len_big"], A,
        stream(preamble(66000), lit(rnd(66000), 4)))
    add("lit_len4_past_input", ["lit_len_past"], R,
        stream(preamble(1000), lit_header(1000, 4), rnd(999)))
    add("lit_len3_past_input", ["lit_len_past"], R,
        stream(preamble(70000), lit_header(70000, 3), rnd(500)))
    add("lit_len4_wraps", ["lit_len_wrap"], U,
        stream(preamble(5), lit(b"abcde"), lit_header(1 << 32, 4)))
    add("lit_len4_huge", ["lit_len_past"], R,
        stream(preamble(5), lit(b"ab"), lit_header(0x80000000, 4), b"cde"))
    add("lit_len_cut", ["lit_len_cut"], R, stream(preamble(300), lit_header(300, 4)[:3]))

    # copy-2 in its overlapping, run-length forms, every length
    for o in range(1, 9):
        add(f"copy2_off{o}_len_1_to_64", ["copy2_short", "copy2_overlap"], A,
            stream(preamble(8 + sum(range(1, 65))), lit(rnd(8)),
                   *[copy2(o, n) for n in range(1, 65)]))
    add("copy2_zero", ["copy2_zero"], R, stream(preamble(9), lit(rnd(8)), copy2(0, 1)))
    add("copy2_past", ["copy2_past"], R, stream(preamble(9), lit(rnd(8)), copy2(9, 1)))

    # copy-1 at short offsets and at its largest
    base = grown(2047)
    add("copy1_short_offsets", ["copy1_overlap"], A,
        stream(preamble(2047 + 8 * sum(range(4, 12))), base,
               *[copy1(o, n) for o in range(1, 9) for n in range(4, 12)]))
    add("copy1_off2047", ["copy1_far"], A,
        stream(preamble(2047 + sum(range(4, 12))), base, *[copy1(2047, n) for n in range(4, 12)]))
    add("copy1_off2047_past", ["copy1_past"], R,
        stream(preamble(2046 + 4), grown(2046), copy1(2047, 4)))

    # the preamble
    body = stream(lit(rnd(30)), copy1(7, 9), lit(rnd(3), 2))
    for w in (2, 3, 4, 5):
        add(f"preamble_{w}_bytes", ["preamble_wide", f"preamble_{w}"], A,
            stream(preamble(42, w), body))
    add("preamble_5_bytes_300", ["preamble_wide", "preamble_5"], A,
        stream(preamble(300, 5), lit(rnd(300), 2)))
    add("preamble_past_32_bits", ["preamble_over"], R, stream(b"\xaa\x80\x80\x80\x10", body))
    add("preamble_6_bytes", ["preamble_over"], R, stream(b"\xaa\x80\x80\x80\x80\x00", body))
    add("preamble_cut", ["preamble_cut"], R, b"\xaa\x80")
    add("output_one_short", ["output_short"], R, stream(preamble(43), body))
    add("output_one_past", ["output_past"], R, stream(preamble(41), body))
    add("output_copy_past", ["output_past"], R,
        stream(preamble(40), lit(rnd(30)), copy2(7, 11)))
    add("empty_input", ["empty_input"], R, b"")
    add("preamble_0", ["preamble_0"], A, preamble(0))
    add("preamble_0_wide", ["preamble_0", "preamble_wide"], A, preamble(0, 3))
    add("preamble_0_then_literal", ["preamble_0_tail"], R, stream(preamble(0), lit(b"a")))
    add("preamble_0_then_copy", ["preamble_0_tail"], R, stream(preamble(0), copy1(1, 4)))
    return out


def main():
    lib = so.system_snappy()
    if lib is None:
        raise SystemExit("libsnappy 1.1.8 not found")
    cs = cases()
    entries, wrong = [], []
    for name, tags, guess, s in cs:
        st, data = so.lib_uncompress(lib, s)
        entries.append({"name": name, "tags": tags, "guess": guess, "ok": st, "n": len(data),
                        "sha256": hashlib.sha256(data).hexdigest() if st == so.OK else None})
        if guess != "unknown" and (guess == "accept") != (st == so.OK):
            wrong.append((name, guess, st))
    blob = {"streams": [len(c[3]) for c in cs], "entries": entries,
            "source": "libsnappy 1.1.8 (/opt/conda/lib/libsnappy.so.1.1.8), "
                      "snappy_uncompressed_length / snappy_uncompress over streams of "
                      "tests/snappy_stream_builder.py"}
    (HERE / "snappy_foreign.bin").write_bytes(b"".join(c[3] for c in cs))
    (HERE / "snappy_foreign.json").write_text(json.dumps(blob, indent=0))
    c = [e["ok"] for e in entries]
    print(len(cs), "streams,", sum(blob["streams"]), "bytes:", {k: c.count(k) for k in (0, 1, 2)})
    for e in entries:
        if e["guess"] == "unknown":
            print("  no guess:", e["name"], "->", e["ok"])
    for name, guess, st in wrong:
        print(f"  the library says otherwise: {name}: guessed {guess}, verdict {st}")


if __name__ == "__main__":
    main()
