"""tests/vtable_model.py against the reference (tests/golden/gen_vtable.cc):
the vTable, the stored values and the VTableMeta its own BuildTable wrote,
the table itself through the build and finish models, and every verdict its
VTableReader::Get and VTableIndex::Decode gave on good and damaged handles,
files and index values. Then the order of the separate call's failures.
No device.
"""
from __future__ import annotations

import functools
import json

import pytest

import sst_build_model as bm
import sst_finish_model as fm
import vtable_model as vm
from conftest import GOLDEN

TABLES = ["sep1", "sep16", "sep1000", "none"]


@functools.lru_cache(maxsize=None)
def cases():
    return json.loads((GOLDEN / "vtable_cases.json").read_text())


@functools.lru_cache(maxsize=None)
def table(name):
    """(spec, entries as (internal key, input value), the .vtb's bytes)."""
    spec = cases()["tables"][name]
    entries = [(bytes.fromhex(e["k"]),
                bytes([e["first"]]) + vm.pattern(e["seed"], e["len"] - 1) if e["len"] else b"")
               for e in spec["entries"]]
    vtb = (GOLDEN / spec["vtb"]).read_bytes() if spec["vtb"] else b""
    return spec, entries, vtb


def get_status(text: str) -> int:
    """A Status of VTableReader::Get as the resolve call's status."""
    if text == "OK":
        return vm.R_OK
    if text.startswith("IO error") or "Read input size not equal" in text:
        return vm.R_PAST_END
    return {"Corruption: Error decode record header": vm.R_BAD_HEADER,
            "Corruption: Error decode VTableRecord": vm.R_BAD_RECORD,
            "Corruption: ": vm.R_TRAILING}[text]


def index_status(text: str) -> int:
    if text == "OK":
        return vm.R_OK
    if "VTableHandle" in text:
        return vm.R_BAD_HANDLE
    assert text == "Corruption: Error decode VTableIndex"
    return vm.R_BAD_INDEX


def test_fixture_is_small_and_complete():
    files = list(GOLDEN.glob("vtable_*"))
    assert sum(f.stat().st_size for f in files) < 131072
    t = cases()["tables"]
    assert sorted(t) == sorted(TABLES)
    assert {c["kv_sep_size"] for c in t.values()} >= {1, 16, 1000}
    assert {c["file_number"] for c in t.values()} == {7, 128, 1 << 35}
    assert t["none"]["vtb"] is None and t["none"]["records_num"] == 0
    ukeys = {len(e["k"]) // 2 - 8 for e in t["sep1"]["entries"]}
    assert {0, 1, 127, 128} <= ukeys
    for name in ("sep1", "sep16", "sep1000"):
        s = t[name]["kv_sep_size"]
        assert {s - 1, s, s + 1} <= {e["len"] for e in t[name]["entries"]}
        assert any(bytes.fromhex(e["k"])[-8] == 0 for e in t[name]["entries"])  # a deletion
    stripped = {e["len"] - 1 for c in t.values() for e in c["entries"] if e["moved"]}
    assert {0, 127, 128, 16383, 16384} <= stripped
    assert any(e["moved"] and e["first"] == 1 for c in t.values() for e in c["entries"])
    offs = [e["get"]["off"] for e in t["sep16"]["entries"] if e["moved"]]
    assert min(offs) < 128 < 16384 < max(offs)
    assert {len(e["stored"]) for e in t["sep16"]["entries"] if e["moved"]} >= {10, 12, 14}


@pytest.mark.parametrize("name", TABLES)
def test_model_reproduces_the_vtable_and_the_stored_values(name):
    spec, entries, vtb = table(name)
    res = vm.separate(entries, spec["kv_sep_size"], spec["file_number"])
    rep = res["report"]
    assert rep["status"] == vm.OK and rep["first_bad_entry"] == vm.NO_ENTRY
    assert res["vtb"] == vtb
    assert (rep["records_num"], rep["table_size"]) == (spec["records_num"], spec["table_size"])
    for e, (_, v), out, off, size in zip(spec["entries"], entries, res["out_vals"],
                                         res["rec_off"], res["rec_size"]):
        if e["moved"]:
            assert out == bytes.fromhex(e["stored"])
            assert (off, size) == (e["get"]["off"], e["get"]["size"])
        else:
            assert out == v and (off, size) == (0, 0)
    assert rep["out_val_bytes"] == sum(map(len, res["out_vals"]))
    assert rep["max_out_val_len"] == max(map(len, res["out_vals"]))


@pytest.mark.parametrize("name", TABLES)
def test_model_values_through_the_build_models_give_the_table(name):
    spec, entries, _ = table(name)
    res = vm.separate(entries, spec["kv_sep_size"], spec["file_number"])
    blocks, _, rep = bm.build([(k, o) for (k, _), o in zip(entries, res["out_vals"])], 4096, 16, 1)
    assert rep["status"] == bm.OK
    image = fm.finish(blocks, 1, 10, 0).image
    assert len(image) == spec["ldb_size"]
    assert image == (GOLDEN / spec["ldb"]).read_bytes()


@pytest.mark.parametrize("name", TABLES)
def test_model_resolves_what_the_reference_stored(name):
    spec, entries, vtb = table(name)
    # as DBImpl::Get sees them: the values the table holds, type 2 before one that stayed
    stored = [bytes.fromhex(e["stored"]) if e["moved"] else b"\x02" + v
              for e, (_, v) in zip(spec["entries"], entries)]
    vals = b"".join(stored)
    lens = list(map(len, stored))
    offs = [sum(lens[:i]) for i in range(len(lens))]
    status, src, off, ln, rep = vm.resolve(vals, offs, lens, vtb, [0], [len(vtb)],
                                           [spec["file_number"]])
    assert status == [vm.R_OK] * len(stored) and rep["count"][vm.R_OK] == len(stored)
    for e, (k, v), s, o, l in zip(spec["entries"], entries, src, off, ln):
        if e["moved"]:
            assert e["get"]["status"] == "OK" and e["get"]["key"] == k[:-8].hex()
            assert s == 1 and vtb[o:o + l] == v[1:] and l == e["get"]["value_len"]
        else:
            assert s == 0 and vals[o:o + l] == v
    dst, dst_off, grep = vm.gather(vals, vtb, status, src, off, ln)
    want = [v[1:] if e["moved"] else v for e, (_, v) in zip(spec["entries"], entries)]
    assert dst == b"".join(want) and grep["dst_bytes"] == len(dst)
    assert [dst[a:b] for a, b in zip(dst_off, dst_off[1:])] == want


def test_model_gives_the_readers_verdicts_on_damaged_handles():
    h = cases()["handles"]
    _, _, vtb = table(h["table"])
    seen = set()
    for c in h["cases"]:
        got = vm.read_record(vtb, c["off"], c["size"])
        assert got[0] == get_status(c["status"]), c
        seen.add(got[0])
    assert seen == {vm.R_BAD_HEADER, vm.R_PAST_END}


def test_model_gives_the_readers_verdicts_on_damaged_files():
    seen = set()
    for c in cases()["crafted"]:
        f = bytes.fromhex(c["file"])
        got = vm.read_record(f, c["off"], c["size"])
        assert got[0] == get_status(c["status"]), c["name"]
        seen.add(got[0])
        if got[0] == vm.R_OK:
            assert f[got[1]:got[1] + got[2]].hex() == c["value"] and got[3].hex() == c["key"]
    assert seen == {vm.R_OK, vm.R_BAD_RECORD, vm.R_TRAILING}


def test_model_gives_the_index_decoders_verdicts():
    seen = set()
    for c in cases()["index"]:
        v = bytes.fromhex(c["value"])
        got = vm.decode_index(v)
        assert got[0] == index_status(c["status"]), c["name"]
        seen.add(got[0])
        if got[0] == vm.R_OK:
            assert got[1:] == (c["file_number"], c["off"], c["size"], c["left"]), c["name"]
        # DecodeValue looks at the type first: only a 1 reaches the decoder
        st = vm.resolve(v, [0], [len(v)], b"", [], [], [])[0][0]
        if not v:
            assert st == vm.R_EMPTY
        elif v[0] == 2:
            assert st == vm.R_OK
        elif v[0] != 1:
            assert st == vm.R_BAD_TYPE
        else:
            assert st == (got[0] if got[0] != vm.R_OK else vm.R_NO_FILE)
    assert seen == {vm.R_OK, vm.R_BAD_INDEX, vm.R_BAD_HANDLE}


def test_overrun_is_refused():
    # (not run in the reference: it builds a Slice past its buffer there)
    f = (7).to_bytes(4, "little") + b"\x03abc\x02xy"
    assert vm.read_record(f, 0, 11)[0] == vm.R_OK
    assert vm.read_record(f, 0, 10)[0] == vm.R_RECORD_OVERRUN
    assert vm.read_record(f, 0, 4)[0] == vm.R_RECORD_OVERRUN


def ikey(user: bytes, seq: int = 5, typ: int = 1) -> bytes:
    return user + ((seq << 8) | typ).to_bytes(8, "little")


def test_failures_come_in_the_references_order():
    good = (ikey(b"a"), b"\x02" + b"v" * 20)
    stays = (b"short", b"\x02v")  # a key that does not parse, but the entry stays
    bad_key, bad_type = (b"short", b"\x02" + b"v" * 20), (ikey(b"b", typ=2), b"\x02" + b"v" * 20)
    assert vm.separate([good, stays], 16, 7)["report"]["status"] == vm.OK
    for at in (0, 1, 2):
        for bad in (bad_key, bad_type):
            es = [good, good, good]
            es[at] = bad
            rep = vm.separate(es, 16, 7)["report"]
            assert (rep["status"], rep["first_bad_entry"]) == (vm.BAD_KEY, at)
            assert rep["table_size"] == rep["records_num"] == rep["out_val_bytes"] == 0
    # an empty value moves only under kv_sep_size 0; the key is looked at first
    rep = vm.separate([good, (ikey(b"b"), b"")], 0, 7)["report"]
    assert (rep["status"], rep["first_bad_entry"]) == (vm.BAD_VALUE, 1)
    rep = vm.separate([good, (b"short", b"")], 0, 7)["report"]
    assert (rep["status"], rep["first_bad_entry"]) == (vm.BAD_KEY, 1)
    # the lowest entry decides, whatever its failure
    rep = vm.separate([good, (ikey(b"b"), b""), bad_key], 0, 7)["report"]
    assert (rep["status"], rep["first_bad_entry"]) == (vm.BAD_VALUE, 1)
    rep = vm.separate([bad_key, (ikey(b"b"), b"")], 0, 7)["report"]
    assert (rep["status"], rep["first_bad_entry"]) == (vm.BAD_KEY, 0)
    # RecordEncoder's assert: user key + stripped value < 2^32 - 1
    assert vm.check_entry(ikey(b"k"), 0xFFFFFFFF, 16) == vm.TOO_LARGE
    assert vm.check_entry(ikey(b""), 0xFFFFFFFF, 16) == vm.OK
    assert vm.check_entry(ikey(b"kk"), 0xFFFFFFFE, 16) == vm.TOO_LARGE
    assert vm.check_entry(b"short", 0xFFFFFFFF, 16) == vm.BAD_KEY


def test_capacity_comes_last_and_says_what_is_needed():
    es = [(ikey(b"a"), b"\x02" + b"v" * 20), (ikey(b"b"), b"\x02v"), (ikey(b"c"), b"\x01" + b"w" * 99)]
    full = vm.separate(es, 16, 7)
    need_vtb, need_out = full["report"]["table_size"], full["report"]["out_val_bytes"]
    assert vm.separate(es, 16, 7, need_vtb, need_out)["report"]["status"] == vm.OK
    for caps in ((need_vtb - 1, need_out), (need_vtb, need_out - 1)):
        res = vm.separate(es, 16, 7, *caps)
        assert res["report"] == dict(full["report"], status=vm.CAPACITY)
        assert res["vtb"] == b"" and res["out_vals"] == []
    rep = vm.separate(es + [(b"short", b"x" * 40)], 16, 7, 0, 0)["report"]
    assert (rep["status"], rep["first_bad_entry"]) == (vm.BAD_KEY, 3)
