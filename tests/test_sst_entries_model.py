"""tests/sst_entries_model.py pinned against the reference (CPU).

tests/golden/block_walk.{bin,json} hold blocks the reference's BlockBuilder
wrote, damaged copies of them, and what the reference's own Block::Iter
yielded for each (gen_block_walk.cc): the model must say the same, entry for
entry and status for status. On the data blocks of every golden table it must
agree with sst_build_model.block_entries, the reader the build tests trust.
The one case the generator must never hand the reference -- a non_shared +
value_length that wraps in 32 bits -- is tested on its own.
"""
from __future__ import annotations

import functools
import json

import pytest

import sst_build_model as bm
import sst_entries_model as em
import sst_finish_model as fm
from conftest import GOLDEN
from test_sst_build_blocks import FIXTURES, _fixture


@functools.lru_cache(maxsize=None)
def walk_cases():
    """(name, block, the reference's entries, the reference's status text)."""
    spec = json.loads((GOLDEN / "block_walk.json").read_text())["cases"]
    data = (GOLDEN / "block_walk.bin").read_bytes()
    assert sum(c["size"] for c in spec) == len(data)
    return tuple((c["name"], data[c["offset"]:c["offset"] + c["size"]],
                  [(bytes.fromhex(k), o, n) for k, o, n in c["entries"]], c["status"])
                 for c in spec)


def test_fixture_is_small_and_complete():
    files = [GOLDEN / "block_walk.json", GOLDEN / "block_walk.bin"]
    assert sum(f.stat().st_size for f in files) < 100_000
    names = {c[0] for c in walk_cases()}
    for want in ("clean_r1", "clean_r2", "clean_r16", "len0", "len3", "len4_count1", "count0",
                 "count_too_many", "restart0_second_entry", "restart0_at_end",
                 "restart0_mid_entry", "restart1_mid_entry", "restart_out_of_order",
                 "restart_entry_shares", "shared_too_long", "varint_cut", "varint_five_high",
                 "stray_one", "stray_two", "value_past_limit", "empty_key_first", "empty_values"):
        assert want in names, want
    by = {c[0]: c for c in walk_cases()}
    # the cases are what their names say
    assert len(by["clean_r16"][2]) == 12 and by["clean_r16"][3] == "OK"
    assert by["restart1_mid_entry"][2] == by["clean_r2"][2] == by["restart_out_of_order"][2]
    assert by["restart0_second_entry"][2] == by["clean_r1"][2][1:]
    assert by["restart_entry_shares"][3] == "OK"
    assert by["restart_entry_shares"][2][3][0] == b"wa" + by["clean_r1"][2][3][0]
    assert by["shared_too_long"][3] == "Corruption: bad entry in block"
    assert len(by["shared_too_long"][2]) == 4
    assert by["empty_key_first"][2][0][0] == b""
    assert [n for _, _, n in by["empty_values"][2]].count(0) == 3


@pytest.mark.parametrize("case", walk_cases(), ids=[c[0] for c in walk_cases()])
def test_model_walks_as_the_reference(case):
    _, block, entries, status = case
    st, got = em.walk(block)
    assert em.STATUS_TEXT[st] == status
    assert got == entries


@pytest.mark.parametrize("name", FIXTURES)
def test_model_reads_the_golden_tables(name):
    raws = _fixture(name)[2]
    for raw in raws:
        assert em.walk(raw)[0] == em.OK
        assert em.entries_of(raw) == bm.block_entries(raw)
    out = em.read(raws, [0] * len(raws))
    assert out["report"]["num_entries"] == len(_fixture(name)[3])
    assert out["report"]["nbad"] == 0 and out["report"]["first_bad_block"] == em.NONE


def test_the_stated_difference_a_sum_that_wraps():
    """non_shared = 0xFFFFFFF0 and value_length = 0x20: 32-bit arithmetic
    gives 0x10 and DecodeEntry would accept the entry and hand out a value 4
    GiB away. The model (and the device) refuse it: BAD_ENTRY, with the
    entries before it."""
    good = fm.block_of([(b"a", b"1"), (b"b", b"2")], 16)
    limit = len(good) - 8
    entry = b"\x00" + fm.varint(0xFFFFFFF0) + fm.varint(0x20) + b"x" * 0x10
    block = good[:limit] + entry + good[limit:]
    st, got = em.walk(block)
    assert st == em.BAD_ENTRY
    assert [k for k, _, _ in got] == [b"a", b"b"]


def test_layout_of_the_model():
    blocks = [fm.block_of([(b"abc", b"v"), (b"abcdefghij", b"")], 16), b"\x00\x00\x00",
              fm.block_of([(b"z", b"zz")], 1)]
    out = em.read(blocks, [16, 100, 200], skip=None)
    assert out["key_off"] == [0, 8, 24] and out["key_len"] == [3, 10, 1]
    assert out["block_first"] == [0, 2, 2, 3]
    assert out["block_status"] == [em.OK, em.BAD_BLOCK, em.OK]
    assert out["val_off"] == [16 + 6, 16 + 7 + 3 + 7, 200 + 4]
    assert out["report"] == {"status": 0, "nbad": 1, "first_bad_block": 1, "max_key_len": 10,
                             "num_entries": 3, "key_bytes": 25, "value_bytes": 3}
    assert em.read(blocks, [0, 0, 0], skip=[0, 1, 1])["block_status"] == \
        [em.OK, em.SKIPPED, em.SKIPPED]
    assert em.read(blocks, [0, 0, 0], max_entries=2)["report"]["status"] == em.CAPACITY
    assert em.read(blocks, [0, 0, 0], key_capacity=24)["report"]["status"] == em.CAPACITY
    assert em.read(blocks, [0, 0, 0], max_entries=3, key_capacity=25)["report"]["status"] == em.OK
