"""tests/scan_model.py against the reference: what its own DBIter over its own
NewMergingIterator over tables its TableBuilder wrote yielded (tests/golden/
gen_scan.cc) -- the forward walk, the SeekToLast / Prev walk, Seek followed by
one Prev, and the caller's loop for a list of ranges, each with status().ok()
-- and the C entry point's host-side validation. No device.
"""
from __future__ import annotations

import ctypes
import functools
import json
import re

import pytest

import scan_model as sm
import sst_merge_model as mm
from conftest import GOLDEN, REPO
from test_sst_merge_model import flat, table_entries

FIXTURE = GOLDEN / "scan_cases.json"


@functools.lru_cache(maxsize=None)
def cases():
    return json.loads(FIXTURE.read_text())


CASES = sorted(json.loads(FIXTURE.read_text())) if FIXTURE.exists() else ["(no fixture)"]
WALKS = [(c, k) for c in CASES for k in range(len(cases()[c]["snapshots"]))] \
    if FIXTURE.exists() else [("(no fixture)", 0)]


@functools.lru_cache(maxsize=None)
def case_merged(name):
    """(spec, the entries in MergingIterator's order, the (run, index) of each,
    the runs' entries, the query keys)."""
    spec = cases()[name]
    images = [(GOLDEN / i["file"]).read_bytes() for i in spec["inputs"]]
    runs = tuple(tuple(table_entries(img, i["blocks"])) for img, i in zip(images, spec["inputs"]))
    assert [len(r) for r in runs] == [i["entries"] for i in spec["inputs"]]
    order = mm.order([[k for k, _ in r] for r in runs], 1)  # pinned in test_sst_merge_model.py
    merged = tuple(runs[r][j] for r, j in order)
    return spec, merged, tuple(order), runs, tuple(bytes.fromhex(k) for k in spec["qkeys"])


def pairs(flat_list):
    return list(zip(flat_list[0::2], flat_list[1::2]))


def test_fixture_is_small_and_complete():
    files = list(GOLDEN.glob("scan_*"))
    assert sum(f.stat().st_size for f in files) < 400_000
    assert max(f.stat().st_size for f in files if f.suffix == ".sst") < 4096
    spec = cases()
    assert {len(c["inputs"]) for c in spec.values()} >= {1, 2, 3, 4}
    assert any(i["entries"] == 0 for i in spec["empty_run"]["inputs"])
    for c in spec.values():
        assert c["first_period"] > 4 * c["total_bytes"]  # RecordReadSample was never reached
    snaps = {s["snapshot"] for c in spec.values() for s in c["snapshots"]}
    assert {0, sm.MAX_SEQUENCE} <= snaps
    # a corrupt walk and a clean one over the same entries
    oks = {(name, s["forward_ok"]) for name, c in spec.items() for s in c["snapshots"]}
    assert ("unparsable", False) in oks and ("five_versions", True) in oks
    qs = [q for c in spec.values() for s in c["snapshots"] for q in s["queries"]]
    assert {q[5] for q in qs} == {True, False}
    assert {-1, 0, 1} <= {q[2] for q in qs} and any(q[2] > q[4] > 0 for q in qs)
    assert any(q[1] == -1 for q in qs) and any(q[0] == q[1] for q in qs)


def test_fixture_holds_its_key_cases():
    _, merged, _, runs, _ = case_merged("five_versions")
    five = [sm.parse(k)[1] for k, _ in merged if k[:-8] == b"five"]
    assert five == [500, 400, 300, 200, 100]
    assert sum(any(k[:-8] == b"five" for k, _ in r) for r in runs) == 3
    snaps = [s["snapshot"] for s in cases()["five_versions"]["snapshots"]]
    assert any(s > 500 for s in snaps) and any(100 < s < 500 for s in snaps) and \
        any(s < 100 for s in snaps)
    # a deletion as the newest, a middle and the oldest version
    _, merged, _, _, _ = case_merged("deletions")
    types = lambda user: [sm.parse(k)[2] for k, _ in merged if k[:-8] == user]
    assert types(b"d-new") == [0, 1, 1] and types(b"d-mid") == [1, 0, 1] and \
        types(b"d-old") == [1, 1, 0]
    assert types(b"e-above") == [0, 1]
    # unparsable keys: before the first visible entry, between two versions, after the last
    _, merged, _, _, _ = case_merged("unparsable")
    bad = [i for i, (k, _) in enumerate(merged) if sm.parse(k) is None]
    assert bad[0] == 0 and bad[-1] == len(merged) - 1 and len(bad) == 3
    assert merged[bad[1] - 1][0][:-8] == merged[bad[1]][0][:-8] == merged[bad[1] + 1][0][:-8]
    # the same internal key in three runs
    spec, merged, order, _, _ = case_merged("equal_keys")
    same = [r for (r, _), (k, _) in zip(order, merged) if k == b"same" + ((77 << 8) | 1).to_bytes(8, "little")]
    assert same == [1, 2, 3]
    users = {k[:-8] for k, _ in case_merged("prefixes")[1]}
    assert {b"", b"pre", b"pref", b"prefix"} <= users
    assert len(case_merged("one_run")[3]) == 1 and len(case_merged("no_entries")[1]) == 0


@pytest.mark.parametrize("name,k", WALKS, ids=[f"{c}-s{k}" for c, k in WALKS])
def test_model_walks_as_the_reference(name, k):
    spec, merged, order, _, qkeys = case_merged(name)
    s = spec["snapshots"][k]
    keys = [key for key, _ in merged]
    snapshot = s["snapshot"]
    fwd, fwd_ok = sm.forward_walk(keys, snapshot)
    assert [order[e] for e in fwd] == pairs(s["forward"]) and fwd_ok == s["forward_ok"]
    rev, rev_ok = sm.reverse_walk(keys, snapshot)
    assert [order[e] for e in rev] == pairs(s["reverse"]) and rev_ok == s["reverse_ok"]
    # the reverse walk is the forward list backwards, in the reference and here
    assert pairs(s["reverse"]) == pairs(s["forward"])[::-1] and rev == fwd[::-1]
    for q, at, seek_ok, prev, prev_ok in s["seek_prev"]:
        it = sm.DBIter(keys, snapshot)
        it.seek(qkeys[q])
        assert (fwd.index(it.at()) if it.valid else -1) == at and (not it.corrupt) == seek_ok
        if it.valid:
            it.prev()
            assert (fwd.index(it.at()) if it.valid else -1) == prev, (q, at)
            assert (not it.corrupt) == prev_ok
        else:
            assert prev == -2
    for start, limit, max_count, first, n, ok in s["queries"]:
        counted, end, q_ok = sm.query(keys, snapshot, qkeys[start],
                                      None if limit < 0 else qkeys[limit],
                                      None if max_count < 0 else max_count)
        want_first = fwd.index(counted[0]) if counted else fwd.index(end) if end is not None else -1
        assert (want_first, len(counted), q_ok) == (first, n, ok), (start, limit, max_count)
        assert counted == fwd[first:first + n] if n else True


@pytest.mark.parametrize("name,k", WALKS, ids=[f"{c}-s{k}" for c, k in WALKS])
def test_model_call_matches_the_fixture(name, k):
    """scan(): the whole call's outputs as the device test compares them."""
    spec, merged, order, _, qkeys = case_merged(name)
    s = spec["snapshots"][k]
    keys = [key for key, _ in merged]
    queries = [(qkeys[a], None if b < 0 else qkeys[b], None if c < 0 else c)
               for a, b, c, _, _, _ in s["queries"]]
    src, per_query, rep = sm.scan(keys, [len(v) for _, v in merged], s["snapshot"], queries)
    assert rep["status"] == sm.OK and rep["num_in"] == len(keys)
    if not keys:
        assert (src, per_query) == ([], []) and rep["nqueries"] == 0
        return
    assert [order[e] for e in src] == pairs(s["forward"])
    nvis = len(src)
    for (first, n, status), q in zip(per_query, s["queries"]):
        assert (first if q[3] >= 0 else nvis, n, status == sm.Q_OK) == \
            (q[3] if q[3] >= 0 else nvis, q[4], q[5])
    assert rep["num_visible"] + rep["num_hidden"] + rep["num_deletions"] + \
        rep["num_above_snapshot"] + rep["num_unparsable"] == len(keys)
    assert rep["sum_count"] == sum(q[4] for q in s["queries"])


def test_model_statuses_and_their_precedence():
    ik = lambda u, s, t=1: u + ((s << 8) | t).to_bytes(8, "little")
    keys = [ik(b"a", 9), ik(b"a", 5), ik(b"a", 5), ik(b"b", 7, 0), ik(b"c", 1)]
    vl = [1, 2, 3, 4, 5]
    src, _, rep = sm.scan(keys, vl, 100)
    assert src == [0, 4] and rep["status"] == sm.OK  # equal keys are legal
    assert (rep["num_hidden"], rep["num_deletions"], rep["key_bytes"], rep["value_bytes"]) == \
        (2, 1, 2, 6)
    swapped = [keys[1], keys[0]] + keys[2:]
    assert sm.scan(swapped, vl, 100)[2] | {"num_in": 0} == \
        dict.fromkeys(sm.REPORT_KEYS, 0) | {"status": sm.UNSORTED, "first_bad_entry": 1}
    short = [keys[1], keys[0], b"short!!", keys[4]]
    rep = sm.scan(short, vl[:4], 100)[2]
    assert (rep["status"], rep["first_bad_entry"]) == (sm.BAD_KEY, 2)  # before UNSORTED at 1
    src, per_query, rep = sm.scan(keys, vl, 100, [(b"", None, None)], max_out=1)
    assert (src, per_query, rep["status"], rep["num_visible"]) == ([], [], sm.CAPACITY, 2)
    assert (rep["max_count"], rep["sum_count"], rep["nqueries"]) == (0, 0, 1)
    # a start above the limit
    assert sm.scan(keys, vl, 100, [(b"c", b"a", None)])[1] == [(1, 0, sm.Q_OK)]


# ---- the C ABI without a device ---------------------------------------------------

ARGS = ("keys", "key_off", "key_len", "val_off", "val_len", "n", "snapshot", "qkeys", "start_off",
        "start_len", "limit_off", "limit_len", "q_max", "nq", "scratch", "scratch_bytes",
        "out_key_off", "out_key_len", "out_val_off", "out_val_len", "out_src", "max_out",
        "q_first", "q_count", "q_status", "report", "stream")
ENTRY_POINTERS = ("keys", "key_off", "key_len", "val_off", "val_len", "scratch", "out_key_off",
                  "out_key_len", "out_val_off", "out_val_len", "out_src", "report")
QUERY_POINTERS = ("qkeys", "start_off", "start_len", "limit_off", "limit_len", "q_first",
                  "q_count", "q_status")


def _abi_args(lvkv, **over):
    p = ctypes.c_void_p(0x1000)
    a = dict.fromkeys(ARGS, p)
    a.update(n=100, snapshot=7, nq=10, max_out=100, stream=None,
             scratch_bytes=lvkv.lib.lvkv_sst_scan_entries_scratch_bytes(100, 10))
    a.update(over)
    assert list(a) == list(ARGS)
    return list(a.values())


def test_host_validation_needs_no_device(lvkv):
    L = lvkv.lib
    f = L.lvkv_sst_scan_entries_device
    bad = lvkv.LVKV_ERR_INVALID
    for name in ENTRY_POINTERS + QUERY_POINTERS:
        assert f(*_abi_args(lvkv, **{name: None})) == bad, name
    for name in ENTRY_POINTERS:  # with no query the query arrays may be null, the others not
        nulls = dict.fromkeys(QUERY_POINTERS + ("q_max",))
        assert f(*_abi_args(lvkv, nq=0, **nulls, **{name: None})) == bad, name
    for snapshot in (sm.MAX_SEQUENCE + 1, (1 << 64) - 1):
        assert f(*_abi_args(lvkv, snapshot=snapshot)) == bad, snapshot
    for n in (1 << 31, (1 << 31) + 5):
        big = L.lvkv_sst_scan_entries_scratch_bytes(n, 10)
        assert f(*_abi_args(lvkv, n=n, scratch_bytes=big)) == bad
        big = L.lvkv_sst_scan_entries_scratch_bytes(100, n)
        assert f(*_abi_args(lvkv, nq=n, scratch_bytes=big)) == bad
    short = L.lvkv_sst_scan_entries_scratch_bytes(100, 10) - 1
    assert f(*_abi_args(lvkv, scratch_bytes=short)) == bad
    # nentries == 0 is decided before every other check
    nulls = dict.fromkeys(ENTRY_POINTERS + QUERY_POINTERS + ("q_max",))
    assert f(*_abi_args(lvkv, n=0, snapshot=(1 << 64) - 1, nq=1 << 40, scratch_bytes=0,
                        **nulls)) == lvkv.LVKV_OK


def test_report_mirror_matches_the_header(lvkv):
    R = lvkv.SstScanReport
    assert ctypes.sizeof(R) == 64
    assert [R.key_bytes.offset, R.value_bytes.offset, R.nqueries.offset, R.sum_count.offset] == \
        [32, 40, 48, 56]
    assert [k for k, _ in R._fields_] == sm.REPORT_KEYS
    header = (REPO / "include" / "lvkv_scan.h").read_text()
    struct = header[header.index("typedef struct lvkv_sst_scan_report"):]
    struct = struct[:struct.index("}")]
    assert re.findall(r"^\s+u?int(?:32|64)_t\s+(\w+);", struct, re.M) == sm.REPORT_KEYS
    assert [lvkv.SCAN_OK, lvkv.SCAN_UNSORTED, lvkv.SCAN_BAD_KEY, lvkv.SCAN_CAPACITY] == \
        [sm.OK, sm.UNSORTED, sm.BAD_KEY, sm.CAPACITY]
    for name, value in (("OK", 0), ("UNSORTED", 1), ("BAD_KEY", 2), ("CAPACITY", 3), ("Q_OK", 0),
                        ("Q_CORRUPT", 1)):
        assert re.search(rf"#define LVKV_SCAN_{name} {value}\b", header), name
    assert re.search(r"#define LVKV_SCAN_NO_LIMIT 0xFFFFFFFFu", header)
    assert lvkv.SCAN_NO_LIMIT == sm.NO_LIMIT == 0xFFFFFFFF
    assert lvkv.MAX_SEQUENCE_NUMBER == sm.MAX_SEQUENCE


def test_sizing_function_is_monotone(lvkv):
    f = lvkv.lib.lvkv_sst_scan_entries_scratch_bytes
    ns = [0, 1, 2, 255, 256, 257, 4095, 4096, 4097, 1 << 20, (1 << 31) - 1]
    for nq in ns:
        s = [f(n, nq) for n in ns]
        assert s == sorted(s), (nq, s)
        s = [f(nq, n) for n in ns]
        assert s == sorted(s), (nq, s)
