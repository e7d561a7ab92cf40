"""The decoders on valid streams no library encoder writes.

lvkv_zstd_uncompress_device promises ZSTD_decompressDCtx's behaviour (libzstd
1.4.9) and lvkv_snappy_uncompress_device snappy::RawUncompress's (1.1.8),
not the decoding of one encoder's output; a table read back by
sst_read_blocks may come from another port, tool or library version. Every
intact stream of the older fixtures was written by ZSTD_compress,
ZSTD_compressStream, the project's own compressor or snappy::RawCompress,
which leave most of each format unused (test_old_fixtures_lack_these_features
counts what). The fixtures here (tests/golden/gen_zstd_foreign.py,
gen_snappy_foreign.py) are built field by field with
tests/zstd_frame_builder.py and tests/snappy_stream_builder.py and carry the
libraries' own verdicts, output lengths and sha256; nothing here needs a
library at run time.

CPU: the oracles give every fixture the library's verdict and bytes; a
census of the feature tags (each with a stream the library accepts, each
refusal with one it refuses); and oracles with one plausible slip each, which
the new corpus catches and the old one does not. GPU: both kernels of both
decoders over the whole corpus at every source alignment, destinations
between borders; through ReadBlock; and the corpus twice in one call.
"""
from __future__ import annotations

import functools
import hashlib
import inspect
import json
import sys
import types

import numpy as np
import pytest

import snappy_oracle as so
import zstd_oracle as zo
from conftest import GOLDEN


def _split(blob: bytes, lengths):
    out, p = [], 0
    for n in lengths:
        out.append(blob[p:p + n])
        p += n
    assert p == len(blob)
    return out


@functools.lru_cache(maxsize=None)
def _corpus(codec):
    """[(stream, entry)] of tests/golden/{codec}_foreign.{json,bin}."""
    spec = json.loads((GOLDEN / f"{codec}_foreign.json").read_text())
    streams = _split((GOLDEN / f"{codec}_foreign.bin").read_bytes(), spec["streams"])
    assert len(streams) == len(spec["entries"])
    return list(zip(streams, spec["entries"]))


def _generator(name):
    sys.path.insert(0, str(GOLDEN))
    try:
        return __import__(name)
    finally:
        sys.path.remove(str(GOLDEN))


def _zstd_verdict(mod, f):
    ok, out = mod.uncompress(f)
    return (2 if ok is None else int(ok)), out


# ---- the oracles agree with the libraries' recorded answers ---------------------------

def test_zstd_oracle_gives_every_foreign_stream_the_librarys_verdict():
    bad = []
    for f, e in _corpus("zstd"):
        v, out = _zstd_verdict(zo, f)
        if v != e["ok"] or (v == 1 and (len(out) != e["n"] or
                                        hashlib.sha256(out).hexdigest() != e["sha256"])):
            bad.append((e["name"], v, e["ok"]))
    assert not bad, f"(stream, oracle, library): {bad}"


def test_snappy_oracle_gives_every_foreign_stream_the_librarys_verdict():
    bad = []
    for f, e in _corpus("snappy"):
        st, out = so.uncompress(f)
        if st != e["ok"] or (st == so.OK and (len(out) != e["n"] or
                                              hashlib.sha256(out).hexdigest() != e["sha256"])):
            bad.append((e["name"], st, e["ok"]))
    assert not bad, f"(stream, oracle, library): {bad}"


def test_builders_and_libraries_reproduce_the_fixtures():
    """Where the libraries are present: the builders still write the committed
    bytes and the libraries still give the recorded verdicts (and the zstd
    oracle reads the content size ZSTD_getFrameContentSize reads)."""
    zlib, slib = zo.system_zstd(), so.system_snappy()
    if zlib is None or slib is None:
        pytest.skip("libzstd 1.4.9 / libsnappy 1.1.8 not present")
    built = _generator("gen_zstd_foreign").cases(zlib)
    assert [(c[0], c[1], c[3]) for c in built] == \
        [(e["name"], e["tags"], f) for f, e in _corpus("zstd")]
    for f, e in _corpus("zstd"):
        ok, out = zo.lib_uncompress(zlib, f)
        assert (2 if ok is None else int(ok), len(out)) == (e["ok"], e["n"]), e["name"]
        assert not ok or hashlib.sha256(out).hexdigest() == e["sha256"], e["name"]
        assert zlib.ZSTD_getFrameContentSize(f, len(f)) == zo.frame_content_size(f), e["name"]
    built = _generator("gen_snappy_foreign").cases()
    assert [(c[0], c[1], c[3]) for c in built] == \
        [(e["name"], e["tags"], f) for f, e in _corpus("snappy")]
    for f, e in _corpus("snappy"):
        st, out = so.lib_uncompress(slib, f)
        assert (st, len(out)) == (e["ok"], e["n"]), e["name"]
        assert st or hashlib.sha256(out).hexdigest() == e["sha256"], e["name"]


# ---- census ----------------------------------------------------------------------------

# every tag has at least one stream the library decodes
ZSTD_ACCEPTED = (
    ["win", "fcs2", "fcs2_256", "fcs2_257", "fcs2_65791", "win_fcs4", "win_fcs8", "fcs8",
     "win_gt_content", "win_eq_content", "win_lt_content", "win_lt_match", "win_byte", "win_max",
     "dict1_zero", "dict2_zero", "dict4_zero", "hdr_unused_bit",
     "cksum_right", "cksum_lengths", "skip", "skip_len0", "skip_after", "skip_between",
     "multi_frame", "concat_empty",
     "blk_mixed", "blk_one_byte", "blk_rle_1", "blk_rle_full", "blk_raw_empty_last",
     "blk_raw_rle_past_128k"] +  # (1.4.9 bounds only compressed blocks by 128 KiB)
    [f"lit_{m}_sf{sf}" for m in ("raw", "rle") for sf in range(4)] +
    [f"lit_{m}_n{n}" for m in ("raw", "rle") for n in (0, 1, 2, 30, 31, 32, 4095, 4096, 20000)] +
    [f"huf_sf{sf}" for sf in range(4)] + [f"treeless_sf{sf}" for sf in range(4)] +
    [f"huf4_mod{k}" for k in range(4)] +
    ["huf4_min", "huf_direct_odd", "huf_direct_even", "huf_direct_max", "huf_fse_weights",
     "huf_depth_11", "huf_single_weight", "huf_symbol_255", "huf_with_sequences",
     "seq_count_1", "seq_count_5", "seq_count_127", "seq_count_128", "seq_count_wide",
     "seq_count_7eff", "seq_count_7f00", "seq_count_long", "seq_modes_reserved"] +
    [f"{k}_{m}" for k in ("ll", "of", "ml") for m in ("predefined", "rle", "fse", "repeat")] +
    ["repeat_after_fse", "repeat_after_rle", "repeat_after_predefined", "repeat_across_raw",
     "ll_rle_max", "ml_rle_max", "of_rle_fits", "fse_log_min", "fse_log_max", "fse_low_prob",
     "fse_zero_runs", "seq_costly", "ll35_all_bits", "ml52_all_bits"] +
    [f"ll_code_{c}" for c in range(16, 36)] + [f"ml_code_{c}" for c in range(32, 53)] +
    [f"of_code_{c}" for c in range(18)] +
    [f"rep{c}_ll{w}" for c in (1, 2, 3) for w in ("pos", "0")] +
    ["rep_zero_becomes_1", "rep_initial", "rep_walk", "rep_across_blocks", "rep_across_raw"] +
    [f"overlap_off{o}" for o in (1, 2, 3, 7, 63, 64, 65)] +
    ["overlap_ml40000", "match_frame_start", "match_block_start", "ll0_ml3", "lits_left_none",
     "lits_left_some", "bits_exact", "bits_one_short", "random", "staged_reach"])
# every tag has at least one stream the library refuses
ZSTD_REFUSED = ["win_refused", "dict1_nonzero", "dict2_nonzero", "dict4_nonzero", "hdr_reserved",
                "cksum_wrong", "cksum_cut", "skip_before", "skip_only", "skip_cut", "skip_not",
                "concat_second_data", "concat_empty_first", "concat_garbage",
                "blk_size_past", "blk_comp_short", "blk_reserved", "blk_no_last",
                "huf4_below_min", "huf4_short_last", "treeless_first", "repeat_first",
                "rle_symbol_past", "of_rle_31", "seq_none_tail", "of_code_outside",
                "rep_before_start", "match_before_start", "lits_overrun", "bits_one_left",
                "bits_left"]
SNAPPY_ACCEPTED = ["copy4", "copy4_far", "copy4_all", "lit_len1", "lit_len2", "lit_len3",
                   "lit_len4", "lit_len_big", "lit_len_wrap", "copy2_short", "copy2_overlap",
                   "copy1_overlap",
                   "copy1_far", "preamble_wide", "preamble_2", "preamble_3", "preamble_4",
                   "preamble_5", "preamble_0"]
SNAPPY_REFUSED = ["copy4_past", "copy4_zero", "copy4_cut", "lit_len_past", "lit_len_cut",
                  "copy2_zero", "copy2_past", "copy1_past", "preamble_over", "preamble_cut",
                  "output_short", "output_past", "empty_input", "preamble_0_tail"]


@pytest.mark.parametrize("codec,accepted,refused", [("zstd", ZSTD_ACCEPTED, ZSTD_REFUSED),
                                                    ("snappy", SNAPPY_ACCEPTED, SNAPPY_REFUSED)])
def test_census_every_feature_has_an_accepted_and_every_refusal_a_refused_stream(codec, accepted,
                                                                                 refused):
    good = 1 if codec == "zstd" else so.OK
    acc, ref, seen = set(), set(), set()
    for _, e in _corpus(codec):
        seen |= set(e["tags"])
        (acc if e["ok"] == good else ref).update(e["tags"])
    assert not [t for t in accepted if t not in acc], "no accepted stream"
    assert not [t for t in refused if t not in ref], "no refused stream"
    assert seen <= set(accepted) | set(refused) | {"win_no_fcs", "bits_pad_1", "bits_pad_8",
                                                   "huf4_tiny"}, "a tag the census does not list"
    if codec == "zstd":  # (a window and no content size: the port cannot size a buffer)
        assert [e["ok"] for _, e in _corpus("zstd") if "win_no_fcs" in e["tags"]] == [2]
        # (the long codes also in frames the LDS-staged kernel decodes: ZSTD_MAX_BLOCK)
        assert all(e["n"] <= 49152 for _, e in _corpus("zstd") if "staged_reach" in e["tags"])


def _zstd_features(f: bytes) -> set:
    """The features of a well-formed stream that the older fixtures are
    counted for: walked over frame headers, block headers and each compressed
    block's literals header and sequence count."""
    feats, p, frames = set(), 0, 0
    while p < len(f):
        if (int.from_bytes(f[p:p + 4], "little") & 0xFFFFFFF0) == 0x184D2A50:
            feats.add("skip")
            p += 8 + int.from_bytes(f[p + 4:p + 8], "little")
            continue
        frames += 1
        fhd = f[p + 4]
        h = zo.frame_header(f[p:])
        if not (fhd >> 5) & 1:
            feats.add("win")
        if fhd >> 6 == 3:
            feats.add("fcs8")
        if fhd & 3:
            feats.add("dict")
        q = p + h.size
        while True:
            bh = int.from_bytes(f[q:q + 3], "little")
            q += 3
            last, btype, bsize = bh & 1, (bh >> 1) & 3, bh >> 3
            if btype == 2:
                b0 = f[q]
                ltype, sf = b0 & 3, (b0 >> 2) & 3
                if ltype < 2:
                    lh = 1 if sf in (0, 2) else 2 if sf == 1 else 3
                    n = (b0 >> 3) if lh == 1 else int.from_bytes(f[q:q + lh], "little") >> 4
                    used = lh + (n if ltype == 0 else 1)
                else:
                    lh, bits = (3, 3, 4, 5)[sf], (10, 10, 14, 18)[sf]
                    used = lh + ((int.from_bytes(f[q:q + lh], "little") >> (4 + bits)) &
                                 ((1 << bits) - 1))
                    if ltype == 3 and sf == 3:
                        feats.add("treeless_sf3")
                if f[q + used] == 255:
                    feats.add("seq_count_long")
            q += 1 if btype == 1 else bsize
            if last:
                break
        p = q + (4 if h.checksum else 0)
    if frames > 1 or (frames == 1 and "skip" in feats):
        feats.add("multi_frame")
    return feats


def _snappy_features(s: bytes) -> set:
    feats = set()
    n = so.uncompressed_length(s)
    i = so._preamble_len(s)
    if so._varint32(n) != s[:i]:
        feats.add("preamble_wide")
    while i < len(s):
        tag = s[i]
        kind, hi = tag & 3, tag >> 2
        if kind == 0:
            k = hi - 59 if hi >= 60 else 0
            if k >= 3:
                feats.add(f"lit_len{k}")
            n = (int.from_bytes(s[i + 1:i + 1 + k], "little") + 1) & 0xFFFFFFFF if k else hi + 1
            i += 1 + k + n
        else:
            if kind == 3:
                feats.add("copy4")
            if kind == 2 and hi + 1 < 4:
                feats.add("copy2_short")
            i += (0, 2, 3, 5)[kind]
    assert i == len(s)
    return feats


@functools.lru_cache(maxsize=None)
def _old(codec):
    """The intact streams of the fixtures from before this module."""
    if codec == "snappy":
        spec = json.loads((GOLDEN / "snappy.json").read_text())
        return _split((GOLDEN / "snappy_streams.bin").read_bytes(), spec["streams"])
    out = []
    for name in ("zstd", "zstd_stream", "zstd_write"):
        spec = json.loads((GOLDEN / f"{name}.json").read_text())
        out += _split((GOLDEN / f"{name}_frames.bin").read_bytes(), spec["frames"])
    return out


def test_old_fixtures_lack_these_features():
    """The gap was real: none of the features counted as 0 in the older
    fixtures is in them, and the walkers that say so find each in the new
    ones."""
    zstd_zero = {"win", "fcs8", "dict", "skip", "multi_frame", "treeless_sf3", "seq_count_long"}
    snappy_zero = {"copy4", "lit_len3", "lit_len4", "copy2_short", "preamble_wide"}
    old = _old("zstd")
    assert len(old) == 445
    for f in old:
        assert not _zstd_features(f) & zstd_zero
    new = set()
    for f, e in _corpus("zstd"):
        if e["ok"] == 1:
            new |= _zstd_features(f)
    assert zstd_zero <= new
    old = _old("snappy")
    assert len(old) == 97
    for s in old:
        assert not _snappy_features(s) & snappy_zero
    new = set()
    for s, e in _corpus("snappy"):
        if e["ok"] == so.OK:
            new |= _snappy_features(s)
    assert snappy_zero <= new


# ---- sensitivity -----------------------------------------------------------------------

def _mutant(mod, old: str, new: str):
    """A copy of an oracle module with one piece of its text replaced."""
    src = inspect.getsource(mod)
    assert src.count(old) == 1, old
    m = types.ModuleType(mod.__name__ + "_mutant")
    exec(compile(src.replace(old, new), mod.__file__, "exec"), m.__dict__)
    return m


# name: (the oracle's text, its replacement, whether the older fixtures see it too)
ZSTD_SLIPS = {
    # (libzstd writes 2-byte content sizes in single-segment frames, so the
    # older fixtures pin the 256 there; behind a window descriptor nothing did)
    "the 2-byte content size without its 256": ("fcs += 256", "fcs += 0", True),
    "the 2-byte content size without its 256 behind a window descriptor": (
        "if fcs_size == 2:", "if fcs_size == 2 and single:", False),
    # (libzstd's matchers do write repeat codes after no literals, the fast one
    # code 1 and level 19 all three in its longer frames: the older fixtures
    # pin the shift, the rep1 - 1 case included, in one frame; the zero offset not)
    "repeat codes not shifted at ll == 0": ("idx = ofv - 1 + (1 if ll == 0 else 0)",
                                            "idx = ofv - 1", True),
    "repeat code 3 at ll == 0 is rep3": ("off = rep[0] - 1", "off = rep[2]", True),
    "a zero repeat offset is corrupt": ("off = rep[0] = 1", 'raise Corrupt("zero offset")', False),
    "checksums not verified": ('if int.from_bytes(src[q:q + 4], "little") != want:', "if False:",
                               False),
    # (what follows the first frame is taken for more frames unseen: bytes that
    # do not start a frame are still refused, as the older damaged fixtures ask)
    "stops after the first frame": (
        "        p = q\n    return bytes(out)",
        "        p = q\n        if (int.from_bytes(src[p:p + 4], 'little') == MAGIC or\n"
        "                int.from_bytes(src[p:p + 4], 'little') >> 4 == 0x184D2A5):\n"
        "            break\n    return bytes(out)", False),
}
SNAPPY_SLIPS = {
    "copy-4 offsets read as 2 bytes": ("off = _u32(src, i)", "off = _u32(src, i) & 0xFFFF", False),
    "3-byte literal lengths read as 2": (
        'ln = (int.from_bytes(src[i: i + k], "little") + 1) & 0xFFFFFFFF',
        'ln = (int.from_bytes(src[i: i + min(k, 2) + (k == 4) * 2], "little") + 1) & 0xFFFFFFFF',
        False),
}


@functools.lru_cache(maxsize=None)
def _old_with_verdicts(codec):
    """[(stream, verdict, sha256 or None)] of the older fixtures: every intact
    stream with the oracle's answer (pinned to the streams' inputs by
    tests/test_zstd.py, test_zstd_write.py and test_snappy.py) and every
    damaged one with the library's recorded verdict."""
    out = []
    if codec == "zstd":
        for f in _old("zstd"):
            v, x = _zstd_verdict(zo, f)
            out.append((f, v, hashlib.sha256(x).hexdigest() if v == 1 else None))
        spec = json.loads((GOLDEN / "zstd.json").read_text())
        for d, v in zip(_split((GOLDEN / "zstd_damaged.bin").read_bytes(), spec["damaged"]),
                        spec["verdicts"]):
            out.append((d, v["ok"], v["sha256"]))
    else:
        for s in _old("snappy"):
            st, x = so.uncompress(s)
            out.append((s, st, hashlib.sha256(x).hexdigest()))
        spec = json.loads((GOLDEN / "snappy.json").read_text())
        for d, v in zip(_split((GOLDEN / "snappy_damaged.bin").read_bytes(), spec["damaged"]),
                        spec["verdicts"]):
            out.append((d, v["status"], v["sha256"] if v["status"] == so.OK else None))
    return out


def _disagreements(codec, mod, streams):
    """The streams (stream, verdict, sha256) whose verdict or bytes mod misses."""
    good = 1 if codec == "zstd" else so.OK
    bad = 0
    for f, want, sha in streams:
        try:
            v, x = _zstd_verdict(mod, f) if codec == "zstd" else mod.uncompress(f)
        except Exception:  # (a slip may break the parser outright: a disagreement)
            bad += 1
            continue
        bad += v != want or (v == good and hashlib.sha256(x).hexdigest() != sha)
    return bad


@pytest.mark.parametrize("codec,slip", [("zstd", k) for k in ZSTD_SLIPS] +
                         [("snappy", k) for k in SNAPPY_SLIPS])
def test_a_slip_is_caught_by_the_new_corpus_and_not_by_the_old(codec, slip):
    """An oracle with one plausible kernel slip disagrees with at least one of
    the new fixtures and with none of the older ones: the new corpus bites
    where the old one could not. (The slips the older fixtures turn out to
    see as well are kept, marked so, the first beside the narrower form they
    do not see.)"""
    base, slips = (zo, ZSTD_SLIPS) if codec == "zstd" else (so, SNAPPY_SLIPS)
    old, new, old_sees = slips[slip]
    mod = _mutant(base, old, new)
    assert (_disagreements(codec, mod, _old_with_verdicts(codec)) > 0) == old_sees
    fresh = [(f, e["ok"], e["sha256"]) for f, e in _corpus(codec)]
    assert _disagreements(codec, mod, fresh) >= 1, "the new corpus does not see it"


def test_the_oracles_agree_with_the_older_fixtures():
    for codec, base in (("zstd", zo), ("snappy", so)):
        assert _disagreements(codec, base, _old_with_verdicts(codec)) == 0


# ---- the device decoders (GPU) -------------------------------------------------------------

def _i64(torch, dev, v):
    return torch.tensor(list(v), dtype=torch.int64, device=dev)


def _i32(torch, dev, v):
    return torch.tensor(list(v), dtype=torch.int32, device=dev)


def _pack(torch, dev, blobs, skew):
    """Inputs one after another from byte `skew`: every alignment."""
    offs, p = [], skew
    for b in blobs:
        offs.append(p)
        p += len(b)
    buf = np.zeros(p + 64, dtype=np.uint8)
    for o, b in zip(offs, blobs):
        buf[o:o + len(b)] = np.frombuffer(b, dtype=np.uint8)
    return torch.from_numpy(buf).to(dev), _i64(torch, dev, offs), \
        _i32(torch, dev, (len(b) for b in blobs))


ROOM_MAX = 300000  # (the largest content of the corpus is below this)


def _claim(codec, f):
    """The length the stream's header claims, or None (none, or past ROOM_MAX)."""
    n = zo.get_uncompressed_length(f) if codec == "zstd" else so.uncompressed_length(f)
    return n if n is not None and n <= ROOM_MAX else None


def _want(lvkv, codec, f, e, cap):
    """The device's status for fixture (f, e) in a room of cap bytes."""
    if codec == "zstd":
        from test_zstd import _want as zstd_want
        return zstd_want(lvkv, f, cap, ok=None if e["ok"] == 2 else bool(e["ok"]))
    n = so.uncompressed_length(f)
    if e["ok"] != so.BAD_LENGTH and n > cap:
        return lvkv.SNAPPY_CAPACITY
    return e["ok"]


def _run_and_check(lvkv, gpu, codec, items, caps, max_ulen, skew, what):
    """One uncompress call over items [(stream, entry)] into rooms of caps
    bytes between borders: the fixture's status, length and sha256, the
    borders whole. Returns the statuses."""
    import torch
    from test_codec_reuse_and_bounds import _gapped
    streams = [f for f, _ in items]
    src, soff, slen = _pack(torch, gpu, streams, skew)
    dst, doff, check = _gapped(torch, gpu, caps)
    args = dict(max_ulen=max_ulen, dst=dst, dst_offsets=_i64(torch, gpu, doff),
                dst_caps=_i32(torch, gpu, caps))
    if codec == "zstd":
        _, _, olen, st, why = lvkv.zstd_uncompress(src, soff, slen, detail=True, **args)
        why = why.cpu().tolist()
    else:
        _, _, olen, st = lvkv.snappy_uncompress(src, soff, slen, **args)
        why = [0] * len(items)
    torch.cuda.synchronize()
    st, olen, h = st.cpu().tolist(), olen.cpu().tolist(), dst.cpu().numpy()
    want = [_want(lvkv, codec, f, e, cap) for (f, e), cap in zip(items, caps)]
    bad = [(e["name"], st[k], want[k], why[k]) for k, (_, e) in enumerate(items)
           if st[k] != want[k]]
    assert not bad, f"{what}: statuses differ (stream, got, want, site): {bad[:8]}"
    bad = [e["name"] for k, (_, e) in enumerate(items) if want[k] == lvkv.SNAPPY_OK and
           (olen[k] != e["n"] or
            hashlib.sha256(h[doff[k]:doff[k] + e["n"]].tobytes()).hexdigest() != e["sha256"])]
    assert not bad, f"{what}: bytes differ from the library's: {bad[:8]}"
    check(h, what)
    return st


@pytest.mark.gpu
@pytest.mark.parametrize("skew", [0, 1, 2, 3])
@pytest.mark.parametrize("codec", ["zstd", "snappy"])
def test_lds_kernels_decode_the_foreign_corpus(lvkv, gpu, codec, skew):
    """max_ulen = the largest (LVKV_ZSTD_MAX_BLOCK = LVKV_SNAPPY_MAX_BLOCK),
    every room that size: whatever fits is the LDS kernel's, a longer
    content is CAPACITY."""
    items = _corpus(codec)
    cap = lvkv.ZSTD_MAX_BLOCK
    assert cap == lvkv.SNAPPY_MAX_BLOCK
    st = _run_and_check(lvkv, gpu, codec, items, [cap] * len(items), cap, skew,
                        f"{codec} LDS kernel, skew {skew}")
    assert {lvkv.SNAPPY_OK, lvkv.SNAPPY_BAD_CONTENTS, lvkv.SNAPPY_CAPACITY,
            lvkv.SNAPPY_BAD_LENGTH} <= set(st)


@pytest.mark.gpu
@pytest.mark.parametrize("skew", [0, 1, 2, 3])
@pytest.mark.parametrize("max_ulen", [256, 0])
@pytest.mark.parametrize("codec", ["zstd", "snappy"])
def test_hbm_kernels_decode_the_foreign_corpus(lvkv, gpu, codec, max_ulen, skew):
    """A small max_ulen and every room exactly what the stream's header
    claims: what does not fit the small staging (at max_ulen 0 nearly
    everything) is decoded by the HBM-output kernel, the long contents too."""
    items = _corpus(codec)
    caps = [_claim(codec, f) or 0 for f, _ in items]
    st = _run_and_check(lvkv, gpu, codec, items, caps, max_ulen, skew,
                        f"{codec} HBM kernel, max_ulen {max_ulen}, skew {skew}")
    good = 1 if codec == "zstd" else so.OK
    assert [s == lvkv.SNAPPY_OK for s in st] == [e["ok"] == good for _, e in items]


@pytest.mark.gpu
def test_uncompressed_length_over_the_foreign_corpus(lvkv, gpu):
    import torch
    for codec in ("zstd", "snappy"):
        items = _corpus(codec)
        src, soff, slen = _pack(torch, gpu, [f for f, _ in items], 1)
        fn = lvkv.zstd_uncompressed_length if codec == "zstd" else lvkv.snappy_uncompressed_length
        ul, st = fn(src, soff, slen)
        torch.cuda.synchronize()
        ul, st = ul.cpu().tolist(), st.cpu().tolist()
        for k, (f, e) in enumerate(items):
            if codec == "zstd":
                n = zo.frame_content_size(f)
                want = (lvkv.SNAPPY_BAD_LENGTH, 0) if n == 0 else \
                    (lvkv.SNAPPY_TOO_LARGE, 0xFFFFFFFF) if n > 0xFFFFFFFF else (lvkv.SNAPPY_OK, n)
            else:
                n = so.uncompressed_length(f)
                want = (lvkv.SNAPPY_BAD_LENGTH, None) if n is None else (lvkv.SNAPPY_OK, n)
            assert st[k] == want[0], (codec, e["name"], st[k], want)
            if want[1] is not None and want[0] != lvkv.SNAPPY_BAD_LENGTH:
                assert ul[k] & 0xFFFFFFFF == want[1], (codec, e["name"])


@functools.lru_cache(maxsize=None)
def _read_block_image(codec):
    """(image, handles, caps, [(status, bytes)] of so.read_block with and
    without verification) of about 40 accepted and 20 refused streams of at
    most 8 KiB of content as blocks of the codec's type, trailers right."""
    crc = so._crc()
    good = 1 if codec == "zstd" else so.OK
    small = [(f, e) for f, e in _corpus(codec)
             if len(f) <= 6000 and (_claim(codec, f) or 0) <= 8192]
    acc = [x for x in small if x[1]["ok"] == good]
    ref = [x for x in small if x[1]["ok"] != good]
    picked = acc[::max(1, len(acc) // 40)][:40] + ref[::max(1, len(ref) // 20)][:20]
    assert len(picked) >= 50
    t = 2 if codec == "zstd" else 1
    img = bytearray(b"\xa5" * 5)
    handles, caps = [], []
    for f, _ in picked:
        caps.append(_claim(codec, f) or 0)
        handles.append((len(img), len(f)))
        img += f + bytes([t])
        img += crc.mask(crc.extend(crc.value(f), bytes([t]))).to_bytes(4, "little")
    img = bytes(img)
    want = [[so.read_block(img, o, sz, verify) for o, sz in handles] for verify in (False, True)]
    return img, handles, caps, want, [e["name"] for _, e in picked]


@pytest.mark.gpu
@pytest.mark.parametrize("codec", ["zstd", "snappy"])
def test_read_blocks_over_foreign_streams(lvkv, gpu, codec):
    """sst_read_blocks over an image whose blocks hold foreign streams, each
    out-cap what the stream claims: so.read_block's verdict and bytes with
    and without the checksum test, the borders whole."""
    import torch
    from test_codec_reuse_and_bounds import _gapped
    img, handles, caps, wants, names = _read_block_image(codec)
    file = torch.from_numpy(np.frombuffer(img, dtype=np.uint8).copy()).to(gpu)
    ho = _i64(torch, gpu, (h[0] for h in handles))
    hs = _i32(torch, gpu, (h[1] for h in handles))
    for verify, want in zip((False, True), wants):
        assert {so.READ_OK} < {w[0] for w in want}
        out, ooff, check = _gapped(torch, gpu, caps)
        _, _, olen, st = lvkv.sst_read_blocks(file, ho, hs, max_ulen=4096, verify=verify, out=out,
                                              out_offsets=_i64(torch, gpu, ooff),
                                              out_caps=_i32(torch, gpu, caps))
        torch.cuda.synchronize()
        st, olen, h = st.cpu().tolist(), olen.cpu().tolist(), out.cpu().numpy()
        what = f"{codec}, verify={verify}"
        # (every room is the stream's claim; a claim past any block, a malformed
        # zstd header's among them, is so.read_block's READ_CAPACITY too)
        bad = [(names[k], st[k], want[k][0]) for k in range(len(handles)) if st[k] != want[k][0]]
        assert not bad, f"{what}: statuses differ (stream, got, want): {bad[:8]}"
        for k, (w, x) in enumerate(want):
            if w == so.READ_OK:
                assert olen[k] == len(x), (what, names[k])
                assert h[ooff[k]:ooff[k] + len(x)].tobytes() == x, (what, names[k])
        check(h, what)


@pytest.mark.gpu
@pytest.mark.parametrize("codec", ["zstd", "snappy"])
def test_foreign_corpus_twice_in_one_call(lvkv, gpu, codec):
    """The corpus in its order and then reversed in one call at max_ulen 0,
    where all but the shortest streams are the HBM-output kernels': those
    decode their streams one after another in the same workgroup, so a
    windowed, checksummed or multi-frame stream, a refused one or one with
    its own tables is followed by another (and each by a different one the
    second time) and must leave it nothing."""
    items = _corpus(codec)
    items = items + items[::-1]
    caps = [_claim(codec, f) or 0 for f, _ in items]
    _run_and_check(lvkv, gpu, codec, items, caps, 0, 1, f"{codec} twice")
