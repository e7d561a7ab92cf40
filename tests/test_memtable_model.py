"""tests/memtable_model.py against the reference (tests/golden/gen_memtable.cc):
on every fixture log, with paranoid_checks off and on, the statuses its
WriteBatch::Iterate gave, the order its MemTable iterates in with every
internal key, max_sequence and the final status; and, through vtable_model and
the build and finish models, every byte of the .ldb / .vtb its BuildTable
wrote. No device.
"""
from __future__ import annotations

import functools
import json

import pytest

import memtable_model as mm
import sst_build_model as bm
import sst_finish_model as fm
import vtable_model as vm
from conftest import GOLDEN

FILE_NUMBER = 5


@functools.lru_cache(maxsize=None)
def cases():
    return json.loads((GOLDEN / "memtable_cases.json").read_text())


@functools.lru_cache(maxsize=None)
def log_of(name):
    """(payload, batch offsets, batch lengths) of a fixture log."""
    records = mm.log_records((GOLDEN / cases()[name]["log"]).read_bytes())
    offs, at = [], 0
    for r in records:
        offs.append(at)
        at += len(r)
    return b"".join(records), offs, [len(r) for r in records]


NAMES = sorted(json.loads((GOLDEN / "memtable_cases.json").read_text()))


def test_fixture_is_small_and_complete():
    files = list(GOLDEN.glob("memtable_*"))
    assert sum(f.stat().st_size for f in files) < 300000
    c = cases()
    texts = {t for v in c.values() for t in v["plain"]["batch_status"]}
    assert texts == set(mm.STATUS_TEXT)
    assert {len(v["plain"]["entries"]) for v in c.values()} >= {0, 1}
    ukeys = {len(e[2]) // 2 - 8 for e in c["keys"]["plain"]["entries"]}
    assert {0, 1, 7, 8, 9, 300} <= ukeys
    lens = log_of("sizes")[2]
    assert {0, 11, 12} <= set(lens)
    assert {0, 1, 2, 65} <= set(mm.from_batches(*log_of("sizes"))["batch_entries"])
    assert max(log_of("three_blocks")[2]) > 2 * 32768
    assert c["sequence_wraps"]["plain"]["max_sequence"] > 1 << 56
    assert c["count_negative"]["plain"]["max_sequence"] > 1 << 63
    for kind in ("tag", "put", "delete"):
        for where in ("first", "middle", "last", "all"):
            assert f"bad_{kind}_{where}" in c
    assert sum(v["paranoid"]["writes_table"] for v in c.values()) >= 8
    assert sum(not v["paranoid"]["writes_table"] for v in c.values()) >= 20


@pytest.mark.parametrize("name", NAMES)
def test_model_walks_and_orders_as_the_reference(name):
    spec = cases()[name]
    payload, offs, lens = log_of(name)
    assert len(offs) == spec["nbatches"]
    ref = spec["plain"]
    res = mm.from_batches(payload, offs, lens, max_sequence=spec["max_sequence_in"])
    rep = res["report"]
    assert res["batch_status"] == [mm.STATUS_TEXT[t] for t in ref["batch_status"]]
    assert rep["status"] == mm.OK and ref["status"] == "OK"
    assert rep["max_sequence_out"] == ref["max_sequence"]
    assert rep["n_too_small"] == ref["reports"] and rep["too_small_bytes"] == ref["report_bytes"]
    where = [(b, j) for b, n in enumerate(res["batch_entries"]) for j in range(n)]
    assert [list(where[e]) for e in res["src"]] == [e[:2] for e in ref["entries"]]
    assert [k.hex() for k in res["ikeys"]] == [e[2] for e in ref["entries"]]
    assert rep["nentries"] == len(ref["entries"])
    for i, e in enumerate(res["src"]):
        assert res["keys"][res["key_off"][i]:res["key_off"][i] + res["key_len"][i]] == res["ikeys"][i]


@pytest.mark.parametrize("name", NAMES)
def test_model_stops_where_a_paranoid_recovery_stops(name):
    spec = cases()[name]
    payload, offs, lens = log_of(name)
    ref = spec["paranoid"]
    res = mm.from_batches(payload, offs, lens, max_sequence=spec["max_sequence_in"], paranoid=True)
    rep = res["report"]
    assert rep["status"] == mm.STATUS_TEXT[ref["status"]]
    assert rep["max_sequence_out"] == ref["max_sequence"]
    if ref["status"] == "OK":
        assert rep["first_bad_batch"] == mm.NONE and ref["writes_table"]
        assert [k.hex() for k in res["ikeys"]] == [e[2] for e in ref["entries"]]
    else:
        # the batch the loop ended on is the last whose status was taken down
        assert rep["first_bad_batch"] == len(ref["batch_status"]) - 1
        assert not ref["writes_table"] and "keys" not in res
        # what the memtable held when the loop ended: the entries before that batch, and
        # those Iterate had handed over
        upto = rep["first_bad_batch"]
        assert sum(res["batch_entries"][:upto + 1]) == len(ref["entries"])


@pytest.mark.parametrize("name", NAMES)
def test_model_entries_through_the_build_models_give_the_tables(name):
    spec = cases()[name]
    payload, offs, lens = log_of(name)
    res = mm.from_batches(payload, offs, lens)
    tables = spec["plain"]["tables"]
    if not tables:
        assert all(s == mm.TOO_SMALL for s in res["batch_status"])  # no memtable was made
        return
    assert [t["kv_sep_size"] for t in tables] == [16, 1 << 40]
    entries = [(k, payload[o:o + n]) for k, o, n in zip(res["ikeys"], res["val_off"], res["val_len"])]
    for t in tables:
        if t["ldb"] is None:
            assert not entries and t["vtb"] is None
            continue
        sep = vm.separate(entries, t["kv_sep_size"], FILE_NUMBER)
        assert sep["report"]["status"] == vm.OK
        assert sep["vtb"] == ((GOLDEN / t["vtb"]).read_bytes() if t["vtb"] else b"")
        blocks, _, rep = bm.build([(k, o) for (k, _), o in zip(entries, sep["out_vals"])],
                                  4096, 16, 1)
        assert rep["status"] == bm.OK
        assert fm.finish(blocks, 1, 10, 0).image == (GOLDEN / t["ldb"]).read_bytes()


def test_model_statuses_the_reference_leaves_undefined():
    one = mm.batch(7, 2, mm.put(b"k", b"\x02v") + mm.delete(b"x"))
    two = mm.batch(8, 1, mm.delete(b"x"))  # x at sequence 8, as the first batch's second entry
    res = mm.from_batches(one + two, [0, len(one)], [len(one), len(two)])
    assert res["report"]["status"] == mm.DUPLICATE and res["report"]["first_bad_entry"] == 2
    res = mm.from_batches(one, [0], [len(one)], max_entries=1)
    assert res["report"]["status"] == mm.CAPACITY and res["report"]["nentries"] == 2
    res = mm.from_batches(one, [0], [len(one)], key_capacity=17)
    assert res["report"]["status"] == mm.CAPACITY and res["report"]["key_bytes"] == 18
    long = mm.batch(1, 1, b"\x00" + mm.varint((1 << 32) - 8))
    res = mm.from_batches(long, [0], [len(long)], virtual_len=[len(long) + (1 << 32)])
    assert res["report"]["status"] == mm.KEY_TOO_LONG and res["report"]["first_bad_batch"] == 0
    res = mm.from_batches(long, [0], [len(long)])  # the key does not fit the batch: Iterate's say
    assert res["batch_status"] == [mm.BAD_DELETE]
