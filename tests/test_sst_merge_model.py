"""tests/sst_merge_model.py against the reference: the merged order its own
NewMergingIterator handed out over tables its TableBuilder wrote, the drop
flag of every merged entry from the loop of db/db_impl.cc:1022-1055 restated
with its ParseInternalKey and comparators, and the table its TableBuilder
wrote from the survivors (tests/golden/gen_merge.cc). No device.
"""
from __future__ import annotations

import functools
import json

import pytest

import snappy_oracle as so
import sst_build_model as bm
import sst_finish_model as fm
import sst_merge_model as mm
from conftest import GOLDEN

RESTART = 16  # Options::block_restart_interval of every fixture table


@functools.lru_cache(maxsize=None)
def cases():
    return json.loads((GOLDEN / "merge_cases.json").read_text())


CASES = sorted(json.loads((GOLDEN / "merge_cases.json").read_text())) \
    if (GOLDEN / "merge_cases.json").exists() else ["(no fixture)"]
COMPACTIONS = [(c, k) for c in CASES if c in cases() for k in range(len(cases()[c]["settings"]))] \
    if CASES != ["(no fixture)"] else [("(no fixture)", 0)]


def table_entries(img, blocks):
    out = []
    for b in blocks:
        st, raw = so.read_block(img, b["offset"], b["size"])
        assert st == so.READ_OK
        out += bm.block_entries(raw)
    return out


@functools.lru_cache(maxsize=None)
def case_inputs(name):
    """(spec, input images, the runs' entries) of a case."""
    spec = cases()[name]
    images = tuple((GOLDEN / i["file"]).read_bytes() for i in spec["inputs"])
    runs = tuple(tuple(table_entries(img, i["blocks"])) for img, i in zip(images, spec["inputs"]))
    assert [len(r) for r in runs] == [i["entries"] for i in spec["inputs"]]
    return spec, images, runs


def setting_of(spec, k):
    s = spec["settings"][k]
    deeper = [(bytes.fromhex(a), bytes.fromhex(b)) for a, b in s["deeper"]]
    return s, deeper


def flat(runs):
    """The runs laid end to end: (entries, run_first)."""
    entries, first = [], [0]
    for r in runs:
        entries += r
        first.append(len(entries))
    return entries, first


def test_fixture_is_small_and_complete():
    files = list(GOLDEN.glob("merge_*"))
    assert sum(f.stat().st_size for f in files) < 200_000
    assert max(f.stat().st_size for f in files) < 16_384
    spec = cases()
    assert {len(c["inputs"]) for c in spec.values()} >= {1, 2, 3, 5}
    assert {c["key_format"] for c in spec.values()} == {0, 1}
    for name in ("three_empty_first", "three_empty_middle", "three_empty_last"):
        at = ["first", "middle", "last"].index(name.split("_")[-1])
        assert [i["entries"] == 0 for i in spec[name]["inputs"]].index(True) == at
    # all of one run before all of another, the reverse, strict interleave
    assert spec["two_in_order"]["order"][0::2] == [0] * 20 + [1] * 20
    assert spec["two_reversed"]["order"][0::2] == [1] * 20 + [0] * 20
    assert spec["two_interleaved"]["order"][0::2] == [0, 1] * 30
    assert [i["entries"] for i in spec["one_in_long"]["inputs"]] == [50, 1]
    snaps = {s["smallest_snapshot"] for c in spec.values() for s in c["settings"]}
    assert {0, mm.MAX_SEQUENCE} <= snaps
    flags = "".join(s["drops"] for c in spec.values() for s in c["settings"])
    assert set(flags) == {"0", "1", "2"}


def test_fixture_holds_its_key_cases():
    _, _, runs = case_inputs("five_runs")
    keys = [k for r in runs for k, _ in r]
    users = [k[:-8] for k in keys]
    assert b"" in users and min(map(len, keys)) == 8
    assert users.count(b"five") == 5 and sum(any(k[:-8] == b"five" for k, _ in r) for r in runs) == 3
    seqs = sorted(mm.parse(k)[1] for k in keys if k[:-8] == b"seq")
    assert seqs == [5, 300]  # (300 << 8 has a lower first byte than 5 << 8)
    assert {b"pre", b"pref", b"prefix"} <= set(users)
    assert [mm.parse(k) is None for k in keys].count(True) == 1
    spec, _, runs = case_inputs("five_runs")
    entries, first = flat(runs)
    merged = [entries[first[r] + j][0] for r, j in zip(spec["order"][0::2], spec["order"][1::2])]
    err = [k for k in merged if k[:-8] == b"err"]
    assert [mm.parse(k) is None for k in err] == [False, True, False, False]
    # the error key stays, and the version after it is not hidden by the one
    # before it: under a snapshot of 250 the first version hides the next
    # otherwise. (kMaxSequenceNumber hides whatever parses, first versions too:
    # the loop starts a user key with last_sequence_for_key = kMaxSequenceNumber.)
    at = merged.index(err[1])
    for s in spec["settings"]:
        assert s["drops"][at] == "0"
        if s["smallest_snapshot"] < mm.MAX_SEQUENCE:
            assert s["drops"][at + 1] == "0"
    by_snapshot = {s["smallest_snapshot"]: s["drops"] for s in spec["settings"]}
    assert by_snapshot[250][at - 1:at + 3] == "0001"
    assert set(by_snapshot[mm.MAX_SEQUENCE]) == {"0", "1"}
    assert by_snapshot[mm.MAX_SEQUENCE].count("0") == 1
    # a deletion that is also hidden counts as hidden
    spec, _, runs = case_inputs("deletions")
    entries, first = flat(runs)
    merged = [entries[first[r] + j][0] for r, j in zip(spec["order"][0::2], spec["order"][1::2])]
    at = next(i for i, k in enumerate(merged) if k[:-8] == b"g-hidden" and mm.parse(k)[2] == 0)
    assert spec["settings"][0]["drops"][at] == "1"
    # equal internal keys in three runs: the lowest run first
    spec = cases()["equal_keys"]
    _, _, runs = case_inputs("equal_keys")
    same = [(r, j) for r, j in zip(spec["order"][0::2], spec["order"][1::2])
            if runs[r][j][0][:-8] == b"same"]
    assert [r for r, _ in same] == [1, 2, 3]


@pytest.mark.parametrize("name", CASES)
def test_model_merges_as_the_reference(name):
    spec, _, runs = case_inputs(name)
    want = list(zip(spec["order"][0::2], spec["order"][1::2]))
    fmt = spec["key_format"]
    assert mm.order([[k for k, _ in r] for r in runs], fmt) == want
    entries, first = flat(runs)
    keys = [k for k, _ in entries]
    assert mm.fast_order(keys, first, fmt) == [first[r] + j for r, j in want]
    src, dropped, rep = mm.merge(keys, [len(v) for _, v in entries], first, fmt)
    assert src == [first[r] + j for r, j in want] and dropped == []
    assert rep["status"] == mm.OK and rep["num_out"] == rep["num_in"] == len(entries)


@pytest.mark.parametrize("name,k", COMPACTIONS, ids=[f"{c}-s{k}" for c, k in COMPACTIONS])
def test_model_drops_as_the_reference(name, k):
    spec, _, runs = case_inputs(name)
    s, deeper = setting_of(spec, k)
    entries, first = flat(runs)
    keys = [key for key, _ in entries]
    merged = [first[r] + j for r, j in zip(spec["order"][0::2], spec["order"][1::2])]
    flags = mm.drops([keys[e] for e in merged], s["smallest_snapshot"], deeper)
    assert "".join(map(str, flags)) == s["drops"]
    src, dropped, rep = mm.merge(keys, [len(v) for _, v in entries], first, 1, True,
                                 s["smallest_snapshot"], deeper)
    assert src == [e for e, f in zip(merged, s["drops"]) if f == "0"]
    assert dropped == [e for e, f in zip(merged, s["drops"]) if f != "0"]
    assert (rep["num_hidden"], rep["num_obsolete"]) == (s["drops"].count("1"), s["drops"].count("2"))
    # the reference's table of the survivors, byte for byte
    blocks = [fm.block_of(b, RESTART)
              for b in bm.cut(mm.survivors(entries, src), spec["out_block_size"], RESTART)]
    table = fm.finish(blocks, key_format=1, bits_per_key=spec["bits_per_key"], compression=0)
    assert table.image == (GOLDEN / s["out"]).read_bytes()


def test_statuses_and_their_precedence():
    ik = lambda u, s: u + ((s << 8) | 1).to_bytes(8, "little")
    keys = [ik(b"a", 5), ik(b"b", 5), ik(b"a", 9), ik(b"c", 1)]
    vl = [1, 2, 3, 4]
    assert mm.merge(keys, vl, [0, 2, 4])[2]["status"] == mm.OK  # a descent across the boundary
    for bad in ([1, 2, 4], [0, 2, 3], [0, 3, 2, 4], [0, 2, 5]):
        rep = mm.merge(keys, vl, bad)[2]
        assert (rep["status"], rep["first_bad_entry"], rep["max_key_len"]) == (mm.BAD_RUNS, mm.NONE, 0)
    assert mm.merge(keys, vl, [0, 4])[2] | {"num_in": 0} == \
        {"status": mm.UNSORTED, "first_bad_entry": 2, "num_in": 0, "num_out": 0, "num_hidden": 0,
         "num_obsolete": 0, "max_key_len": 9, "key_bytes": 0, "value_bytes": 0}
    short = [keys[0], keys[0], b"short", keys[3]]
    assert mm.merge(short, vl, [0, 4])[2]["status"] == mm.BAD_KEY  # before UNSORTED at 1
    assert mm.merge(short, vl, [0, 4])[2]["first_bad_entry"] == 2
    assert mm.merge(short, vl, [0, 4], key_format=0)[2]["first_bad_entry"] == 1
    src, dropped, rep = mm.merge(keys, vl, [0, 2, 4], max_out=3)
    assert (src, dropped, rep["status"], rep["num_out"]) == ([], [], mm.CAPACITY, 4)
    assert mm.merge(keys, vl, [0, 0, 2, 2, 4, 4])[0] == [2, 0, 1, 3]
    assert mm.merge([], [], [0])[2]["num_in"] == 0
