"""tests/sst_get_model.py against the reference: for every query of every
fixture table (tests/golden/gen_get.cc) what its own Table::InternalGet did --
whether the callback ran, the entry it was handed, the Status, whether a data
block was read -- and where its Block::Iter::Seek lands on the index block and
on every data block directly. Then the damaged blocks of
tests/sst_get_damage.py: that each edit damages what its name says. No device.
"""
from __future__ import annotations

import functools
import json

import pytest

import snappy_oracle as so
import sst_build_model as bm
import sst_get_damage as dmg
import sst_get_model as gm
from conftest import GOLDEN

HAVE = (GOLDEN / "get_cases.json").exists()
TABLES = sorted(json.loads((GOLDEN / "get_cases.json").read_text())) if HAVE else ["(no fixture)"]


@functools.lru_cache(maxsize=None)
def cases():
    return json.loads((GOLDEN / "get_cases.json").read_text())


@functools.lru_cache(maxsize=None)
def table(name):
    """(spec, image, index block, filter block or None, data blocks) decoded."""
    spec = cases()[name]
    img = (GOLDEN / spec["file"]).read_bytes()

    def block(h):
        st, raw = so.read_block(img, h[0], h[1])
        assert st == so.READ_OK
        return raw

    filt = block(spec["filter"]) if spec["filter"] is not None else None
    return spec, img, block(spec["index"]), filt, [block(h) for h in spec["blocks"]]


def seek_string(block, q, key_format):
    s = gm.seek(block, q, key_format)
    if s["verdict"] == gm.VALID:
        return "V:" + s["key"].hex()
    return "E" if s["verdict"] == gm.END else "C:Corruption: bad entry in block"


def get(name, q):
    """The model's whole lookup: (locate's tuple, seek_query's tuple or None,
    the data block sought in or None)."""
    spec, _, index, filt, data = table(name)
    loc = gm.locate(index, filt, q, spec["key_format"])
    if loc[0] != gm.BLOCK:
        return loc, None, None
    at = [h[0] for h in spec["blocks"]].index(loc[2])
    assert spec["blocks"][at][1] == loc[3] and loc[1] == at
    return loc, gm.seek_query(data[at], q, spec["key_format"]), data[at]


def test_fixture_is_small_and_complete():
    files = list(GOLDEN.glob("get_*"))
    assert sum(f.stat().st_size for f in files) < 100_000
    spec = cases()
    assert {c["key_format"] for c in spec.values()} == {0, 1}
    assert {c["compression"] for c in spec.values()} == {0, 1}
    assert {c["restart_interval"] for c in spec.values()} == {1, 2, 16}
    assert {(c["key_format"], c["filter"] is not None) for c in spec.values()} == \
        {(1, True), (1, False), (0, False)}
    assert spec["one_entry"]["entries"] == 1 and len(spec["one_block_r16"]["blocks"]) == 1
    assert max(len(c["blocks"]) for c in spec.values()) >= 4
    # absent keys the filter lets through, and ones it turns away
    for name in ("internal_bloom_r16", "internal_bloom_r1_snappy"):
        absent = [q for q in spec[name]["queries"] if b"~" in bytes.fromhex(q["k"])]
        assert any(q["read"] for q in absent) and not all(q["read"] for q in absent)
    # past the end, a deletion handed out, a version of another user key
    qs = [q for c in spec.values() for q in c["queries"]]
    assert any(q["iseek"] == "E" for q in qs)
    assert any(q["called"] and q["ev"] == "" for q in qs)


@pytest.mark.parametrize("name", TABLES)
def test_seek_lands_where_the_references_does(name):
    spec, _, index, _, data = table(name)
    for q in spec["queries"]:
        k = bytes.fromhex(q["k"])
        assert seek_string(index, k, spec["key_format"]) == q["iseek"], q["k"]
        assert [seek_string(b, k, spec["key_format"]) for b in data] == q["bseek"], q["k"]


@pytest.mark.parametrize("name", TABLES)
def test_lookup_does_what_internal_get_did(name):
    spec, _, _, _, _ = table(name)
    for q in spec["queries"]:
        k = bytes.fromhex(q["k"])
        loc, hit, block = get(name, k)
        assert q["st"] == "OK" and loc[0] in (gm.BLOCK, gm.PAST_END, gm.FILTERED), q["k"]
        assert bool(q["read"]) == (loc[0] == gm.BLOCK), q["k"]
        if q["iseek"] == "E":
            assert loc[0] == gm.PAST_END
        called = hit is not None and hit[1] != gm.NONE
        assert called == bool(q["called"]), q["k"]
        if not called:
            assert hit is None or hit[0] == gm.NOT_FOUND
            continue
        state, off, voff, vlen, tag = hit
        ek, ev = bytes.fromhex(q["ek"]), bytes.fromhex(q["ev"])
        assert block[voff: voff + vlen] == ev, q["k"]
        entries = dict(bm.block_entries(block))
        assert entries[ek] == ev
        if spec["key_format"] == 1:
            # SaveValue on what the callback was handed
            assert tag == gm.tag_of(ek)
            same = ek[:-8] == k[:-8]
            want = gm.NOT_FOUND if not same else gm.FOUND if ek[-8] == 1 else gm.DELETED
            assert state == want, q["k"]
        else:
            assert tag == 0 and state == (gm.FOUND if ek == k else gm.NOT_FOUND), q["k"]


@pytest.mark.skipif(not HAVE, reason="no fixture")
def test_every_state_is_met():
    states, statuses = set(), set()
    for name in TABLES:
        for q in cases()[name]["queries"]:
            loc, hit, _ = get(name, bytes.fromhex(q["k"]))
            statuses.add(loc[0])
            if hit is not None:
                states.add(hit[0])
    assert statuses == {gm.BLOCK, gm.PAST_END, gm.FILTERED}
    assert states == {gm.NOT_FOUND, gm.FOUND, gm.DELETED}


# ---- the damaged blocks: each edit damages what its name says -----------------


def verdicts(block, queries, key_format):
    return {gm.seek(block, q, key_format)["verdict"] for q in queries}


@pytest.mark.skipif(not HAVE, reason="no fixture")
@pytest.mark.parametrize("name", ["internal_plain_r2_snappy", "bytes_r1_snappy"])
def test_block_damage_is_what_it_says(name):
    spec, _, index, _, data = table(name)
    kf = spec["key_format"]
    qs = [bytes.fromhex(q["k"]) for q in spec["queries"]]
    for block in (index, data[0]):
        d = dmg.block_damage(block)
        sound = [gm.seek(block, q, kf) for q in qs]
        assert all(s["verdict"] in (gm.VALID, gm.END) for s in sound)
        assert gm.CORRUPT in verdicts(d["restart shared != 0"], qs, kf)
        # in the bisection such an offset is corrupt, in the walk a clean end
        for near in ("restart at the array", "restart 2 before the array"):
            assert gm.CORRUPT in verdicts(d[near + ", middle"], qs, kf), near
        assert verdicts(d["restart at the array, first"], qs, kf) >= {gm.END}
        assert gm.CORRUPT not in verdicts(d["restart at the array, first"], qs[:1], kf)
        assert verdicts(d["restart count 0"], qs, kf) == {gm.END}
        assert verdicts(d["4 bytes, count 0"], qs, kf) == {gm.END}
        for bad in ("restart count too large", "restart count huge", "3 bytes", "empty"):
            assert verdicts(d[bad], qs, kf) == {gm.BAD}, bad
        assert gm.CORRUPT in verdicts(d["entry varint runs out"], qs, kf)
        above = [n for n in d if n.startswith("shared above")]
        assert (len(above) == 3) == (spec["restart_interval"] > 1 and block is data[0])
        for n in above:
            assert gm.CORRUPT in verdicts(d[n], qs, kf), n
        # a lying array changes where some seek lands, and none crashes the model
        lying = [gm.seek(d["lying restarts, mid-entry"], q, kf) for q in qs]
        assert lying != sound


@pytest.mark.skipif(not HAVE, reason="no fixture")
def test_index_and_key_damage_is_what_it_says():
    spec, _, index, filt, data = table("internal_bloom_r16")
    qs = [bytes.fromhex(q["k"]) for q in spec["queries"]]
    for bad in dmg.index_bad_handles(index).values():
        assert gm.BAD_HANDLE in {gm.locate(bad, filt, q, 1)[0] for q in qs}
    entries = bm.block_entries(data[1])
    short = dmg.short_key_block(entries, 2, 4)  # (entry 4 begins a restart run)
    assert gm.BAD_ENTRY in {gm.seek_query(short, q, 1)[0] for q in qs}
    first = entries[0][0]
    hit = gm.seek_query(dmg.type_byte(data[1], 0, 2), first[:-8] + b"\xff" * 8, 1)
    assert hit[0] == gm.CORRUPT_KEY and hit[1] == 0
    assert gm.seek_query(data[1], b"short", 1)[0] == gm.STATE_BAD_KEY
    assert gm.locate(index, filt, b"short", 1)[0] == gm.BAD_KEY


@pytest.mark.skipif(not HAVE, reason="no fixture")
def test_filter_damage_is_what_it_says():
    spec, _, index, filt, _ = table("internal_bloom_r16")
    qs = [bytes.fromhex(q["k"]) for q in spec["queries"]]
    d = dmg.filter_damage(filt)
    sound = [gm.locate(index, filt, q, 1)[0] for q in qs]
    assert gm.FILTERED in sound

    def statuses(f):
        return [gm.locate(index, f, q, 1)[0] for q in qs]

    nofilter = statuses(None)
    assert gm.FILTERED not in nofilter
    for name in ("4 bytes", "empty", "last_word too large", "last_word huge", "start > limit",
                 "limit past the offsets", "k of 31", "k of 255"):
        assert statuses(d[name]) == nofilter, name  # everything may match
    for name in ("empty filter", "one byte filter"):
        got = statuses(d[name])  # nothing matches
        assert all(g == gm.FILTERED for g, n in zip(got, nofilter) if n == gm.BLOCK), name
    assert statuses(d["k of 30"]) != nofilter
    # with base_lg 0 only the block at offset 0 still has a filter
    got = statuses(d["base_lg 0"])
    first = [gm.locate(index, None, q, 1)[2] == 0 for q in qs]
    assert [g for g, f in zip(got, first) if f] == [s for s, f in zip(sound, first) if f]
    assert [g for g, f in zip(got, first) if not f] == [n for n, f in zip(nofilter, first) if not f]
    assert statuses(d["base_lg 63"]) == sound and statuses(d["base_lg 64"]) == sound
