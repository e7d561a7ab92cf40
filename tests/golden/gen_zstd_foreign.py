"""Generates tests/golden/zstd_foreign.{json,bin}: valid (and nearly valid)
Zstd streams no library encoder writes, built field by field with
tests/zstd_frame_builder.py, each with libzstd 1.4.9's own verdict through
port::Zstd_Uncompress (zo.lib_uncompress: 1 decoded, 0 failed, 2 content
size unknown or huge), the output's length and its sha256.

    python tests/golden/gen_zstd_foreign.py

Every entry carries the feature tags tests/test_decoder_foreign_streams.py
counts, and a guess ("accept" / "reject" / "unknown": what the case was
written to get). The library's answer is the expectation; the summary
printed at the end lists every case whose guess it contradicts.
"""
from __future__ import annotations

import ctypes
import hashlib
import json
import sys
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
REPO = HERE.parent.parent
for p in (REPO / "tests", REPO / "oracle"):
    sys.path.insert(0, str(p))
import zstd_frame_builder as fb  # noqa: E402
import zstd_oracle as zo  # noqa: E402
from zstd_frame_builder import (Bytes, Compressed, Literals, PREDEFINED, REPEAT,  # noqa: E402
                                RLE, Raw, Rle, Seq, frame, fse, off, skippable)

A, R, U = "accept", "reject", "unknown"


def content_of(lib, blocks, last_flags=None):
    """What the library decodes the blocks to (in a frame of unknown content
    size, the largest window), or None where it refuses them."""
    f = frame(blocks, fcs_bytes=0, window=0xA8, last_flags=last_flags)
    cap = 1 << 21
    out = ctypes.create_string_buffer(cap)
    r = lib.ZSTD_decompress(out, cap, f, len(f))
    return None if lib.ZSTD_isError(r) else out.raw[:r]


def cases(lib):
    """[(name, tags, guess, stream)] in a fixed order."""
    rng = np.random.default_rng(20261020)
    out = []

    def rnd(n, k=256):
        return rng.integers(0, k, n, dtype=np.uint8).tobytes()

    def skew(n, syms):
        """n bytes over syms, each half as likely as the one before."""
        p = np.array([2.0 ** -min(i + 1, 30) for i in range(len(syms))])
        return bytes(np.asarray(syms, dtype=np.uint8)[rng.choice(len(syms), n, p=p / p.sum())])

    def add(name, tags, guess, stream):
        assert all(name != c[0] for c in out), name
        out.append((name, sorted(set(tags)), guess, bytes(stream)))

    def data(name, tags, guess, blocks, *, claim=None, last_flags=None, **hdr):
        """A data frame around blocks; the content the library's (claim: the
        content size to write where it refuses the blocks)."""
        c = content_of(lib, blocks, last_flags)
        if c is None:
            assert claim is not None, f"{name}: the library refuses the blocks; give a claim"
            c = bytes(claim)
        hdr.setdefault("fcs_bytes", 4)
        add(name, tags, guess, frame(blocks, content=c, last_flags=last_flags, **hdr))
        return c

    def sized(n):
        return [Raw(rnd(min(n, 90))), Rle(0xA7, n - 90)] if n > 90 else [Raw(rnd(n))]

    # ---- frame headers ---------------------------------------------------------
    for n in (256, 257, 65791):
        data(f"hdr_win_fcs2_{n}", ["win", "fcs2", f"fcs2_{n}"], A, sized(n), window=0x08,
             fcs_bytes=2)
    data("hdr_win_fcs4", ["win", "win_fcs4"], A, sized(300), window=0x10, fcs_bytes=4)
    data("hdr_win_fcs8", ["win", "fcs8", "win_fcs8"], A, sized(300), window=0x10, fcs_bytes=8)
    data("hdr_single_fcs2", ["fcs2"], A, sized(1000), fcs_bytes=2)
    data("hdr_single_fcs8", ["fcs8"], A, sized(77), fcs_bytes=8)
    for n, tag in ((300, "win_gt_content"), (1024, "win_eq_content"), (5000, "win_lt_content")):
        data(f"hdr_{tag}", ["win", tag], A, sized(n), window=0x00, fcs_bytes=4)
    far = [Raw(rnd(3000)), Compressed(Literals.raw(rnd(10)), [Seq(4, off(2900), 700),
                                                             Seq(2, off(3600), 1290)])]
    data("hdr_win_lt_content_far_match", ["win", "win_lt_content", "win_lt_match"], A, far,
         window=0x00, fcs_bytes=4)
    for wb in (0x00, 0x07, 0x0F, 0x53, 0x9C, 0xAF):
        data(f"hdr_win_byte_{wb:02x}", ["win", "win_byte"] + (["win_max"] if wb == 0xAF else []),
             A, sized(200), window=wb, fcs_bytes=4)
    for wb in (0xB0, 0xFF):
        data(f"hdr_win_byte_{wb:02x}", ["win_refused"], R, sized(200), window=wb, fcs_bytes=4)
    data("hdr_win_no_fcs", ["win", "win_no_fcs"], U, sized(200), window=0x10, fcs_bytes=0)
    for nb, bad in ((1, 0x01), (2, 0x0100), (4, 0x01000000)):
        data(f"hdr_dict{nb}_zero", [f"dict{nb}_zero"], A, sized(120), dict_bytes=nb, dict_id=0)
        data(f"hdr_dict{nb}_zero_win", ["win", f"dict{nb}_zero"], A, sized(120), dict_bytes=nb,
             dict_id=0, window=0x08, fcs_bytes=(0, 8, 4, 0, 8)[nb])
        data(f"hdr_dict{nb}_nonzero", [f"dict{nb}_nonzero"], R, sized(120), dict_bytes=nb,
             dict_id=bad)
    data("hdr_dict1_zero_fcs1", ["dict1_zero"], A, sized(60), dict_bytes=1, fcs_bytes=1)
    data("hdr_reserved_bit", ["hdr_reserved"], R, sized(100), reserved=True)
    data("hdr_unused_bit", ["hdr_unused_bit"], A, sized(100), unused=True)

    mixed = [Raw(rnd(50)), Rle(0x33, 70),
             Compressed(Literals.raw(rnd(12)), [Seq(5, off(100), 40), Seq(3, off(7), 9)])]
    data("cksum_right", ["cksum_right"], A, mixed, checksum=True, fcs_bytes=1)
    data("cksum_right_win", ["cksum_right", "win"], A, mixed, checksum=True, window=0x00,
         fcs_bytes=8)
    for n in (1, 4, 8, 31, 32, 33, 45, 64, 100, 2000):
        data(f"cksum_right_len{n}", ["cksum_right", "cksum_lengths"], A, [Raw(rnd(n))],
             checksum=True, fcs_bytes=2 if n >= 256 else 1)
    good = fb.checksum_of(content_of(lib, mixed))
    for k in (0, 3):
        wrong = bytearray(good)
        wrong[k] ^= 0x80
        data(f"cksum_wrong_byte{k}", ["cksum_wrong"], R, mixed, checksum=bytes(wrong), fcs_bytes=1)
    for k in (1, 3, 4):
        data(f"cksum_cut{k}", ["cksum_cut"], R, mixed, checksum=good[:4 - k], fcs_bytes=1)

    # ---- skippable frames and concatenation ------------------------------------------
    c1 = content_of(lib, mixed)
    d1 = frame(mixed, content=c1, fcs_bytes=1)
    d1c = frame(mixed, content=c1, fcs_bytes=4, window=0x08, checksum=True)
    empty = frame([Raw(b"")], content=b"", fcs_bytes=1)
    empty_win = frame([Raw(b"")], content=b"", fcs_bytes=4, window=0x00, checksum=True)
    d2 = frame([Raw(rnd(9))], content=bytes(9), fcs_bytes=1)
    add("skip_before", ["skip_before"], R, skippable(0, b"12345") + d1)
    add("skip_after", ["skip", "skip_after"], A, d1 + skippable(7, b"abc"))
    add("skip_after_len0", ["skip", "skip_len0", "skip_after"], A, d1c + skippable(15))
    add("skip_between", ["skip", "skip_between", "multi_frame"], A,
        d1 + skippable(3, rnd(40)) + skippable(9) + empty)
    add("skip_only", ["skip_only"], R, skippable(1, b"xyz") + skippable(2))
    add("skip_only_one", ["skip_only"], R, skippable(0))
    for k in (4, 7):
        add(f"skip_cut_header{k}", ["skip_cut"], R, d1 + skippable(5, b"abcdef")[:k])
    add("skip_cut_body", ["skip_cut"], R, d1 + skippable(5, b"abcdef")[:-1])
    add("skip_magic_above", ["skip_not"], R, d1 + (0x184D2A60).to_bytes(4, "little") + bytes(4))
    add("concat_empty", ["multi_frame", "concat_empty"], A, d1 + empty)
    add("concat_empty_win_cksum", ["multi_frame", "concat_empty", "win", "cksum_right"], A,
        d1c + empty_win + empty)
    add("concat_second_data", ["concat_second_data"], R, d1 + d2)
    add("concat_empty_first", ["concat_empty_first"], R, empty + d1)
    for k in (1, 2, 3, 4, 9):
        add(f"concat_garbage{k}", ["concat_garbage"], R,
            d1 + b"\x28\xb5\x2f\xfc\x20\x00\x01\x00\x00"[:k])

    # ---- blocks -----------------------------------------------------------------------
    reach = [Raw(rnd(40)), Rle(0x11, 30),
             Compressed(Literals.raw(rnd(6)), [Seq(2, off(72), 45), Seq(1, off(35), 20),
                                               Seq(0, off(1), 10)]),
             Rle(0x22, 5), Raw(rnd(3)),
             Compressed(Literals.raw(rnd(9)), [Seq(4, off(12), 11), Seq(0, off(150), 140),
                                               Seq(2, 1, 5)])]
    data("blk_mixed_reach_back", ["blk_mixed"], A, reach, fcs_bytes=2)
    data("blk_200_one_byte", ["blk_one_byte"], A,
         [Raw(rnd(1)) if k % 3 else Rle(k, 1) for k in range(200)], fcs_bytes=1)
    data("blk_rle_1", ["blk_rle_1"], A, [Rle(0x77, 1)], fcs_bytes=1)
    data("blk_rle_full", ["blk_rle_full"], A, [Raw(rnd(5)), Rle(0x78, 131072)], fcs_bytes=4)
    # (guessed refused; 1.4.9 bounds only compressed blocks by 128 KiB and takes these)
    data("blk_rle_past_full", ["blk_raw_rle_past_128k"], R, [Rle(0x79, 131073)],
         claim=bytes(131073))
    data("blk_raw_past_full", ["blk_raw_rle_past_128k"], R, [Bytes(0, 131073, rnd(131073, 2))],
         claim=bytes(131073))
    body = fb.literals_section(Literals.raw(bytes(131068)), fb.State()) + b"\x00"
    assert len(body) == 131072
    data("blk_comp_full", ["blk_size_past"], R, [Bytes(2, len(body), body)], claim=bytes(131068))
    data("blk_raw_empty_last", ["blk_raw_empty_last"], A, [Raw(rnd(33)), Raw(b"")], fcs_bytes=1)
    for k in (0, 1, 2):
        data(f"blk_comp_{k}_bytes", ["blk_comp_short"], R,
             [Raw(rnd(10)), Bytes(2, k, b"\x00\x00"[:k])], claim=bytes(10))
    data("blk_reserved_type", ["blk_reserved"], R, [Raw(rnd(10)), Bytes(3, 4, b"abcd")],
         claim=bytes(14))
    data("blk_no_last", ["blk_no_last"], R, [Raw(rnd(10)), Raw(rnd(12))],
         last_flags=[False, False], claim=bytes(22))

    # ---- literals ---------------------------------------------------------------------
    head = Raw(rnd(16))
    for mode in ("raw", "rle"):
        for sf in range(4):
            sizes = {0: (0, 2, 30), 2: (1, 31), 1: (0, 1, 31, 32, 4095),
                     3: (0, 1, 31, 32, 4095, 4096, 20000)}[sf]
            for n in sizes:
                lit = Literals.raw(rnd(n), sf) if mode == "raw" else Literals.rle(0x40 + sf, n, sf)
                blk = Compressed(lit, [Seq(min(n, 3), off(5), 4)])
                data(f"lit_{mode}_sf{sf}_n{n}", [f"lit_{mode}_sf{sf}", f"lit_{mode}_n{n}"], A,
                     [head, blk], fcs_bytes=4)
    alpha = list(b"etaoinshrdlu")
    for sf, n, n2 in ((0, 500, 300), (1, 900, 701), (2, 5000, 3002), (3, 3000, 20003)):
        blocks = [Compressed(Literals.huf(skew(n, alpha), sf), []),
                  Compressed(Literals.treeless(skew(n2, alpha[:5]), sf), [])]
        data(f"huf_sf{sf}_then_treeless", [f"huf_sf{sf}", f"treeless_sf{sf}"], A, blocks)
    for n in (1000, 1001, 1002, 1003):
        data(f"huf4_n{n}", [f"huf4_mod{n % 4}"], A,
             [Compressed(Literals.huf(skew(n, alpha), 1), [])])
    tree = b"aaaaaaaabbbbccd"
    for n in range(1, 13):
        # (1.4.9 takes a count when three streams of ceil(n / 4) fit in it: 3, 4, 6 and up)
        data(f"huf4_tiny_n{n}", ["huf4_tiny"] + {2: ["huf4_below_min"], 3: ["huf4_min"],
                                                 5: ["huf4_short_last"]}.get(n, []),
             R if n in (1, 2, 5) else A,
             [head, Compressed(Literals.huf((b"abacabad" * 2)[:n], 1, tree_from=tree), [])],
             claim=bytes(16 + n))
    data("huf_direct_odd", ["huf_direct_odd"], A,
         [Compressed(Literals.huf(skew(300, [0, 1, 2, 3, 4, 5]), 0), [])])
    data("huf_direct_even", ["huf_direct_even"], A,
         [Compressed(Literals.huf(skew(300, [0, 1, 2, 3, 4, 5, 6]), 0), [])])
    full = bytes(rng.permutation(np.repeat(np.arange(129, dtype=np.uint8), 4)))
    data("huf_direct_max", ["huf_direct_max"], A, [Compressed(Literals.huf(full, 1), [])])
    data("huf_fse_weights", ["huf_fse_weights"], A,
         [Compressed(Literals.huf(skew(2000, list(range(60, 100))), 2, weights="fse"), [])])
    deep = bytes(rng.permutation(np.repeat(np.arange(12, dtype=np.uint8),
                                           [1024, 512, 256, 128, 64, 32, 16, 8, 4, 2, 1, 1])))
    data("huf_depth_11", ["huf_depth_11"], A,
         [Compressed(Literals.huf(deep, 2), []),
          Compressed(Literals.treeless(deep[::-1][:700], 0), [])])
    data("huf_single_weight", ["huf_single_weight"], A,
         [Compressed(Literals.huf(rnd(400, 2), 0), [])])
    data("huf_symbol_255", ["huf_symbol_255"], A,
         [Compressed(Literals.huf(skew(800, [255, 0, 254, 17, 128]), 1, weights="fse"), [])])
    data("huf_with_sequences", ["huf_with_sequences"], A,
         [head, Compressed(Literals.huf(skew(600, alpha), 1),
                           [Seq(100, off(20), 30), Seq(0, off(3), 3), Seq(450, 1, 8)])])
    data("treeless_first_block", ["treeless_first"], R,
         [head, Compressed(Literals.treeless(skew(200, alpha), 0), [])], claim=bytes(216))

    # ---- sequences: counts -------------------------------------------------------------
    def small_seqs(n):
        return [Seq(i % 3, off(1 + i % 7), 3 + i % 5) for i in range(n)]

    def with_lits(seqs, extra=2):
        return Literals.raw(rnd(sum(s.ll for s in seqs) + extra))

    for n, width in ((1, None), (5, 2), (127, None), (127, 2), (128, None)):
        s = small_seqs(n)
        data(f"seq_count_{n}" + (f"_as{width}" if width else ""),
             [f"seq_count_{n}"] + (["seq_count_wide"] if width else []), A,
             [head, Compressed(with_lits(s), s, count_bytes=width)])
    for n in (0x7EFF, 0x7F00, 0x7F00 + 300):
        s = [Seq(0, off(1 + int(v)), 3) for v in rng.integers(0, 4, n)]
        data(f"seq_count_{n:#x}", ["seq_count_7eff" if n < 0x7F00 else "seq_count_long"] +
             (["seq_count_7f00"] if n == 0x7F00 else []) + ["ll0_ml3"], A,
             [Raw(rnd(8)), Compressed(Literals.raw(b""), s, ll=RLE, of=RLE, ml=RLE)])

    # ---- sequences: table modes ---------------------------------------------------------
    same = [Seq(2, off(1 + i % 4), 6) for i in range(9)]  # one code each: LL 2, OF 2, ML 3
    ll_n = [4, 4, 7, 4, 4, 2, 2, 1, 1, 1, 1] + [0] * 24 + [-1]       # 36 symbols, log 5
    of_n = [2, 6, 12, 6, 3, 1, 1, -1]                                # log 5
    ml_n = [16] + [0] * 10 + [8] + [0] * 30 + [4, 2, 1, -1]          # zero runs of 10 and 30
    var = [Seq(i % 11, off(1 + 3 * (i % 9)) if i % 4 else 1 + i % 3,
               (3, 14, 100, 140, 300, 600)[i % 6]) for i in range(60)]
    assert sum(ll_n[:-1]) + 1 == 32 and sum(of_n[:-1]) + 1 == 32 and sum(ml_n[:-1]) + 1 == 32
    for key in ("ll", "of", "ml"):
        data(f"mode_{key}_predefined", [f"{key}_predefined"], A,
             [head, Compressed(with_lits(var), var, **{"ll": fse(ll_n, 5), "of": fse(of_n, 5),
                                                       "ml": fse(ml_n, 5), key: PREDEFINED})])
        data(f"mode_{key}_rle", [f"{key}_rle"], A,
             [head, Compressed(with_lits(same), same, **{key: RLE})])
        data(f"mode_{key}_fse", [f"{key}_fse", "fse_log_min"] +
             (["fse_zero_runs"] if key == "ml" else []) + ["fse_low_prob"], A,
             [head, Compressed(with_lits(var), var, **{key: fse({"ll": ll_n, "of": of_n,
                                                                 "ml": ml_n}[key], 5)})])
        for prev, tag in ((fse({"ll": ll_n, "of": of_n, "ml": ml_n}[key], 5), "fse"),
                          (RLE, "rle"), (PREDEFINED, "predefined")):
            s1 = same if prev == RLE else var
            data(f"mode_{key}_repeat_after_{tag}", [f"{key}_repeat", f"repeat_after_{tag}"], A,
                 [head, Compressed(with_lits(s1), s1, **{key: prev}),
                  Compressed(with_lits(s1[::-1]), s1[::-1], **{key: REPEAT})])
        data(f"mode_{key}_repeat_first_block", ["repeat_first"], R,
             [head, Compressed(with_lits(same), same, **{key: REPEAT})],
             claim=bytes(16 + sum(s.ll + s.ml for s in same) + 2))
        past = {"ll": 36, "of": 32, "ml": 53}[key]
        data(f"mode_{key}_rle_symbol_{past}", ["rle_symbol_past"], R,
             [head, Compressed(with_lits(same), same, **{key: ("rle", past)})],
             claim=bytes(16 + sum(s.ll + s.ml for s in same) + 2))
    data("mode_all_repeat_across_raw", ["repeat_after_fse", "repeat_across_raw"], A,
         [head, Compressed(with_lits(var), var, ll=fse(ll_n, 5), of=fse(of_n, 5), ml=fse(ml_n, 5)),
          Raw(rnd(7)), Rle(3, 9),
          Compressed(with_lits(var[5:40]), var[5:40], ll=REPEAT, of=REPEAT, ml=REPEAT)])
    data("mode_of_rle_31", ["of_rle_31"], R,
         [head, Compressed(with_lits(same), [Seq(2, 1 << 31, 6)], of=RLE)], claim=bytes(28))
    data("mode_reserved_bits", ["seq_modes_reserved"], U,
         [head, Compressed(with_lits(same), same, reserved_modes=3)],
         claim=bytes(16 + sum(s.ll + s.ml for s in same) + 2))
    data("seq_none_then_bytes", ["seq_none_tail"], R,
         [head, Compressed(Literals.raw(rnd(20)), [], tail=b"\x00")], claim=bytes(36))

    # the largest accuracy logs (9 / 8 / 9); the codes in use hold one state each
    # (so each costs the whole log in state bits); 300 sequences a block
    ll_9 = [1] * 20 + [512 - 20 - 15] + [-1] * 15
    of_8 = [1] * 18 + [256 - 18 - 13] + [-1] * 13
    ml_9 = [1] * 45 + [512 - 45 - 7] + [-1] * 7
    costly = [Seq(int(a), off(int(o)), int(m)) for a, o, m in
              zip(rng.choice([0, 3, 15, 16, 17, 19, 21, 23], 300), rng.integers(4093, 8000, 300),
                  rng.choice([3, 34, 35, 38, 42, 50, 66, 67, 82], 300))]
    data("seq_300_costly", ["fse_log_max", "seq_costly"], A,
         [Raw(rnd(8200)), Compressed(Literals.huf(skew(sum(s.ll for s in costly) + 5, alpha), 2),
                                     costly, ll=fse(ll_9, 9), of=fse(of_8, 8), ml=fse(ml_9, 9))])
    costly2 = [Seq(int(a), off(int(o)), int(m)) for a, o, m in
               zip(rng.choice([0, 16, 19, 23, 27, 31], 300), rng.integers(65533, 131000, 300),
                   rng.integers(131, 515, 300))]
    data("seq_300_costlier", ["fse_log_max", "seq_costly"], A,
         [Rle(9, 131072), Raw(rnd(100)),
          Compressed(Literals.huf(skew(sum(s.ll for s in costly2) + 5, alpha), 2), costly2,
                     ll=fse(ll_9, 9), of=fse(of_8, 8), ml=fse(ml_9, 9))])

    # ---- sequences: every long code -------------------------------------------------------
    def at_code(base, bits, k):
        return base + (((1 << bits) - 1) if k == 0 else int(rng.integers(0, 1 << bits)))

    s = [Seq(at_code(zo.LL_BASE[c], zo.LL_BITS[c], k), off(1 + c), 3 + c % 4)
         for c in range(16, 32) for k in (0, 1)]
    data("ll_codes_16_31", [f"ll_code_{c}" for c in range(16, 32)], A,
         [head, Compressed(Literals.huf(skew(sum(x.ll for x in s) + 1, alpha), 3), s)])
    s = [Seq(at_code(zo.LL_BASE[c], zo.LL_BITS[c], 1), off(9), 5) for c in (32, 33, 34)]
    data("ll_codes_32_34", [f"ll_code_{c}" for c in (32, 33, 34)], A,
         [head, Compressed(Literals.huf(skew(sum(x.ll for x in s) + 1, alpha[:3]), 3), s)])
    for name, ll, mode in (("ll_code_35_all_bits", 131071, PREDEFINED), ("ll_code_35", 70001, RLE)):
        data(name, ["ll_code_35", "ll_rle_max"] if mode == RLE else ["ll_code_35", "ll35_all_bits"],
             A, [Raw(rnd(30)), Compressed(Literals.rle(0xEE, ll), [Seq(ll, off(ll + 25), 12)],
                                          ll=mode)])
    s = [Seq(k, off(3 + c), at_code(zo.ML_BASE[c], zo.ML_BITS[c], k))
         for c in range(32, 48) for k in (0, 1)]
    data("ml_codes_32_47", [f"ml_code_{c}" for c in range(32, 48)], A,
         [Raw(rnd(64)), Compressed(with_lits(s), s)])
    s = [Seq(1, off(50 + c), at_code(zo.ML_BASE[c], zo.ML_BITS[c], 1)) for c in range(48, 52)]
    data("ml_codes_48_51", [f"ml_code_{c}" for c in range(48, 52)], A,
         [Raw(rnd(120)), Compressed(with_lits(s), s)])
    for name, ml, mode in (("ml_code_52_all_bits", 131074, PREDEFINED), ("ml_code_52", 70003, RLE)):
        data(name, ["ml_code_52", "ml_rle_max"] if mode == RLE else ["ml_code_52", "ml52_all_bits"],
             A, [Raw(rnd(90)), Compressed(Literals.raw(rnd(3)), [Seq(2, off(61), ml)], ml=mode)])
    s = [Seq(1, 1, 4), Seq(1, 2, 4), Seq(0, 3, 5)] + \
        [Seq(1, (1 << c) + int(rng.integers(0, 1 << c)) if c < 17 else off(131072 + 60), 3 + c)
         for c in range(2, 18)]
    data("of_codes_0_17", [f"of_code_{c}" for c in range(18)], A,
         [Rle(0x55, 131072), Raw(rnd(100)), Compressed(with_lits(s), s)])
    data("of_code_17_rle", ["of_rle_fits"], A,
         [Rle(0x55, 131072), Raw(rnd(100)),
          Compressed(Literals.raw(rnd(8)), [Seq(2, off(131072 + 50 + k), 5) for k in range(3)],
                     of=RLE)])
    data("of_code_18_outside", ["of_code_outside"], R,
         [Rle(0x55, 131072), Raw(rnd(100)),
          Compressed(Literals.raw(rnd(8)), [Seq(2, off(5), 5), Seq(2, 1 << 18, 5)])],
         claim=bytes(131072 + 100 + 8 + 10))

    # the longest codes whose output still fits the decoder's LDS staging (48 KiB)
    s = [Seq(1, (1 << c) + int(rng.integers(0, 1 << c)) if c < 15 else off(40000 + c), 3 + c)
         for c in range(2, 16)]
    data("of_codes_2_15_staged", [f"of_code_{c}" for c in range(2, 16)] + ["staged_reach"], A,
         [Rle(0x56, 40000), Raw(rnd(100)), Compressed(with_lits(s), s)])
    s = [Seq(8192 + 5, off(20), 5), Seq(16384 + 16383, off(9000), 4)]
    data("ll_codes_32_33_staged", ["ll_code_32", "ll_code_33", "staged_reach"], A,
         [Raw(rnd(30)), Compressed(Literals.rle(0xED, sum(x.ll for x in s) + 2), s)])
    s = [Seq(1, off(50 + c), zo.ML_BASE[c] + int(rng.integers(0, 1 << (zo.ML_BITS[c] - 2))))
         for c in (48, 49, 50)]
    data("ml_codes_48_50_staged", [f"ml_code_{c}" for c in (48, 49, 50)] + ["staged_reach"], A,
         [Raw(rnd(120)), Compressed(with_lits(s), s)])

    # ---- sequences: repeat offsets ------------------------------------------------------------
    hist = Raw(rnd(64))
    pre = [Seq(2, off(10), 4), Seq(1, off(20), 5), Seq(3, off(30), 3)]  # rep = 30, 20, 10
    post = [Seq(1, 1, 3), Seq(1, 2, 4), Seq(1, 3, 5), Seq(0, 1, 3), Seq(0, 2, 4)]
    for code in (1, 2, 3):
        for ll in (2, 0):
            s = pre + [Seq(ll, code, 6)] + post
            data(f"rep_code{code}_ll{ll}", [f"rep{code}_ll{'pos' if ll else '0'}"], A,
                 [hist, Compressed(with_lits(s), s)])
    s = [Seq(2, off(1), 4), Seq(0, 3, 6)] + post
    data("rep3_ll0_rep1_is_1", ["rep_zero_becomes_1"], A, [hist, Compressed(with_lits(s), s)])
    s = [Seq(1, 1, 3), Seq(1, 2, 3), Seq(1, 3, 3), Seq(0, 1, 4), Seq(0, 2, 5)]
    data("rep_initial", ["rep_initial"], A, [hist, Compressed(with_lits(s), s)])
    data("rep_initial_before_start", ["rep_before_start"], R,
         [Compressed(Literals.raw(rnd(6)), [Seq(2, 3, 4)])], claim=bytes(10))
    s = [Seq(int(rng.integers(0, 3)), int(rng.integers(1, 4)), int(rng.integers(3, 9)))
         for _ in range(120)]
    data("rep_random_walk", ["rep_walk"], A, [hist, Compressed(with_lits(pre + s), pre + s)])
    nxt = [Seq(0, 1, 4), Seq(1, 3, 5), Seq(0, 3, 3), Seq(2, 2, 6)]
    data("rep_across_blocks", ["rep_across_blocks"], A,
         [hist, Compressed(with_lits(pre), pre), Compressed(with_lits(nxt), nxt)])
    data("rep_across_raw", ["rep_across_raw"], A,
         [hist, Compressed(with_lits(pre), pre), Raw(rnd(5)), Rle(1, 2),
          Compressed(with_lits(nxt), nxt)])

    # ---- sequences: overlap, edges, the bitstream's ends --------------------------------------
    mls = (3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 40, 63, 64, 65, 100, 127, 128, 129, 255, 256,
           257, 1000, 4000)
    for o in (1, 2, 3, 7, 63, 64, 65):
        s = [Seq(1, off(o), m) for m in mls]
        data(f"overlap_off{o}", [f"overlap_off{o}"], A, [Raw(rnd(80)), Compressed(with_lits(s), s)])
    s = [Seq(3, off(o), 40000) for o in (1, 2, 3, 7, 63, 64, 65)]
    data("overlap_ml40000", ["overlap_ml40000"], A, [Raw(rnd(80)), Compressed(with_lits(s), s)])
    data("match_from_frame_start", ["match_frame_start"], A,
         [Raw(rnd(20)), Compressed(Literals.raw(rnd(5)), [Seq(3, off(23), 30)])])
    data("match_before_frame_start", ["match_before_start"], R,
         [Raw(rnd(20)), Compressed(Literals.raw(rnd(5)), [Seq(3, off(24), 30)])], claim=bytes(55))
    data("match_from_block_start", ["match_block_start"], A,
         [Raw(rnd(20)), Compressed(Literals.raw(rnd(9)), [Seq(7, off(7), 30), Seq(0, off(37), 4)])])
    data("match_first_block_start", ["match_frame_start"], A,
         [Compressed(Literals.raw(rnd(9)), [Seq(7, off(7), 30)])])
    data("match_first_block_before", ["match_before_start"], R,
         [Compressed(Literals.raw(rnd(9)), [Seq(7, off(8), 30)])], claim=bytes(39))
    s = [Seq(0, off(4), 3), Seq(0, off(2), 3), Seq(0, 1, 3), Seq(0, off(60), 3)]
    data("seq_ll0_ml3", ["ll0_ml3"], A, [hist, Compressed(Literals.raw(b""), s)])
    s = small_seqs(20)
    data("lits_left_none", ["lits_left_none"], A, [hist, Compressed(with_lits(s, 0), s)])
    data("lits_left_some", ["lits_left_some"], A, [hist, Compressed(with_lits(s, 300), s)])
    data("lits_overrun", ["lits_overrun"], R,
         [hist, Compressed(Literals.raw(rnd(sum(x.ll for x in s) - 1)), s)], claim=bytes(200))
    s = small_seqs(20)[:-1] + [Seq(1, off(1), 4)]  # (the first bits written are the offset's 00)
    # (under the predefined tables 1.4.9's state update after the last sequence
    # reads on, so a few bits of padding are not "left")
    for pad, tag, guess in ((1, "bits_pad_1", U), (-1, "bits_one_short", U), (8, "bits_pad_8", U),
                            (40, "bits_left", R)):
        data(f"bits_predef_pad{pad}", [tag], guess,
             [hist, Compressed(with_lits(s), s, pad_bits=pad)],
             claim=bytes(64 + sum(x.ll + x.ml for x in s) + 2))
    # (all three tables RLE: no state bits, the sequences' own bits are all there is)
    s = [Seq(2, off(1 + i % 4), 6) for i in range(9)] + [Seq(2, off(1), 6)]
    for pad, tag, guess in ((1, "bits_one_left", R), (-1, "bits_one_short", U),
                            (0, "bits_exact", A)):
        data(f"bits_rle_pad{pad}", [tag], guess,
             [hist, Compressed(with_lits(s), s, ll=RLE, of=RLE, ml=RLE, pad_bits=pad)],
             claim=bytes(64 + sum(x.ll + x.ml for x in s) + 2))

    # ---- the same choices at random: 80 frames of 1-3 compressed blocks -----------------------
    ze = fb.ze
    nsym = {"ll": 36, "of": 32, "ml": 53}
    max_log = {"ll": 9, "of": 8, "ml": 9}

    def rand_norm(key, codes):
        """Normalised counts that give every code in use a state, over a few
        symbols more, some of them "less than 1"."""
        syms = sorted(set(codes) | {int(x) for x in rng.integers(0, nsym[key], 3)})
        log = max(int(rng.integers(5, max_log[key] + 1)), len(syms).bit_length())
        norm = [0] * nsym[key]
        heavy = [s for s in syms if rng.random() < 0.7] or syms[:1]
        for s in syms:
            norm[s] = 1 if s in heavy else -1
        rest = (1 << log) - len(syms)
        cuts = sorted(int(x) for x in rng.integers(0, rest + 1, len(heavy) - 1))
        for s, a, b in zip(heavy, [0] + cuts, cuts + [rest]):
            norm[s] += b - a
        return fse(norm, log), set(syms)

    def fse_weights_fit(d):
        nb, _, max_sym, depth = fb.huf_tables(d, 11)
        body = ze._huf_compress_weights([depth + 1 - nb[s] if nb[s] else 0 for s in range(max_sym)])
        return body is not None and 1 < len(body) < 128

    for k in range(80):
        blocks = [Raw(rnd(int(rng.integers(8, 200))))]
        produced = len(blocks[0].data)
        cover = {"ll": None, "of": None, "ml": None}  # the codes a repeat would find, if any
        huf_syms = None
        for _ in range(int(rng.integers(1, 4))):
            if rng.random() < 0.2:
                blocks.append(Rle(int(rng.integers(0, 256)), int(rng.integers(1, 50)))
                              if rng.random() < 0.5 else Raw(rnd(int(rng.integers(0, 50)))))
                produced += blocks[-1].n if isinstance(blocks[-1], Rle) else len(blocks[-1].data)
            seqs = []
            for _ in range(int(rng.integers(1, 70))):
                ll = int(rng.choice([0, 0, 1, 2, 5, 15, 16, 17, 40, 130]))
                ml = int(rng.choice([3, 3, 4, 7, 18, 35, 36, 70, 300]))
                produced += ll
                ofv = int(rng.integers(1, 4)) if rng.random() < 0.3 else \
                    off(int(rng.integers(1, min(produced, 9000) + 1)))
                seqs.append(Seq(ll, ofv, ml))
                produced += ml
            n = sum(s.ll for s in seqs) + int(rng.integers(0, 40))
            kind = int(rng.integers(0, 4))
            syms = alpha[:int(rng.integers(2, 9))]
            if kind == 0 or n < 8:
                lit = Literals.raw(rnd(n))
            elif kind == 1:
                lit = Literals.rle(int(rng.integers(0, 256)), n)
            else:
                d = skew(n, syms)
                sf = 0 if n < 1024 and rng.random() < 0.5 else \
                    int(rng.integers(1 if n < 1024 else 2, 4))
                if kind == 3 and huf_syms is not None and set(d) <= huf_syms:
                    lit = Literals.treeless(d, sf)
                elif len(set(d)) >= 2:
                    lit = Literals.huf(d, sf, weights="fse" if rng.random() < 0.5 and
                                       fse_weights_fit(d) else "direct")
                    huf_syms = set(d)
                else:
                    lit = Literals.raw(d)
            modes = {}
            codes = {"ll": [ze.ll_code(s.ll) for s in seqs],
                     "of": [ze.highbit(s.ofv) for s in seqs],
                     "ml": [ze.ml_code(s.ml - 3) for s in seqs]}
            for key in ("ll", "of", "ml"):
                used = set(codes[key])
                pick = int(rng.integers(0, 4))
                if pick == 3 and cover[key] is not None and used <= cover[key]:
                    modes[key] = REPEAT
                elif pick == 1 and len(used) == 1:
                    modes[key], cover[key] = RLE, used
                elif pick == 2:
                    modes[key], cover[key] = rand_norm(key, codes[key])
                else:
                    modes[key] = PREDEFINED
                    cover[key] = set(range(nsym[key] if key != "of" else 29))
            blocks.append(Compressed(lit, seqs, **modes))
        data(f"random_{k}", ["random"], A, blocks, checksum=bool(k % 2),
             **({"window": int(rng.integers(0, 0xA8)), "fcs_bytes": 8 if k % 4 == 0 else 4}
                if k % 3 == 0 else {}))
    return out


def main():
    lib = zo.system_zstd()
    if lib is None:
        raise SystemExit("libzstd 1.4.9 not found")
    cs = cases(lib)
    entries, wrong = [], []
    for name, tags, guess, s in cs:
        ok, out = zo.lib_uncompress(lib, s)
        v = 2 if ok is None else int(ok)
        entries.append({"name": name, "tags": tags, "guess": guess, "ok": v, "n": len(out),
                        "sha256": hashlib.sha256(out).hexdigest() if ok else None})
        if guess != "unknown" and (guess == "accept") != (v == 1):
            wrong.append((name, guess, v))
    blob = {"streams": [len(c[3]) for c in cs], "entries": entries,
            "source": "libzstd 1.4.9 (/opt/conda/lib/libzstd.so.1.4.9), ZSTD_getFrameContentSize / "
                      "ZSTD_decompress over streams of tests/zstd_frame_builder.py"}
    (HERE / "zstd_foreign.bin").write_bytes(b"".join(c[3] for c in cs))
    (HERE / "zstd_foreign.json").write_text(json.dumps(blob, indent=0))
    c = [e["ok"] for e in entries]
    print(len(cs), "streams,", sum(blob["streams"]), "bytes:", {k: c.count(k) for k in (0, 1, 2)})
    for name, v in [(e["name"], e["ok"]) for e in entries if e["guess"] == "unknown"]:
        print("  no guess:", name, "->", v)
    for name, guess, v in wrong:
        print(f"  the library says otherwise: {name}: guessed {guess}, verdict {v}")


if __name__ == "__main__":
    main()
