"""tests/store_model.py against the pinned per-stage models, composed as the
device composes the stages: memtable_model per group, vtable_model.separate,
the build and finish models for the table images, sst_merge_model over the
runs newest first, scan_model and vtable_model.resolve. No device.

Three things are held here so that tests/test_store.py can lean on them:
the histories have what the GPU tests need; the composed models give the
dictionary's answers at every snapshot and range the GPU tests use; and a
compaction at smallest snapshot s changes nothing for a reader at s or later,
in one step or in two.
"""
from __future__ import annotations

import functools

import pytest

import memtable_model as mm
import scan_model as sm
import sst_build_model as bm
import sst_finish_model as fm
import sst_merge_model as gm
import store_model as st
import vtable_model as vm

from test_memtable import T, W  # the sort tile and the parse window, held there to the library's
from test_sst_scan import TILE as SCAN_TILE  # kScanTile, read there from the sources

SEEDS = st.SEEDS


@functools.lru_cache(maxsize=None)
def built(seed):
    """Per group of history(seed), by the models: raw (the sorted entries as
    written), stored (after separation), vtb, image (the table's bytes)."""
    h = st.history(seed)
    out = []
    for g in range(len(h.groups)):
        payload, offs, lens = h.payload(g)
        m = mm.from_batches(payload, offs, lens)
        assert m["report"]["status"] == mm.OK and m["report"]["nentries"] == len(h.ops[g])
        assert m["report"]["max_sequence_out"] == h.last[g]
        raw = [(k, bytes(payload[o:o + n]))
               for k, o, n in zip(m["ikeys"], m["val_off"], m["val_len"])]
        sep = vm.separate(raw, h.kv_sep[g], h.file_numbers[g])
        assert sep["report"]["status"] == vm.OK
        stored = [(k, bytes(v)) for (k, _), v in zip(raw, sep["out_vals"])]
        out.append(dict(raw=raw, stored=stored, vtb=bytes(sep["vtb"]),
                        image=table_image(h, stored, at_least=9)))
    return out


def table_image(h, entries, at_least=1) -> bytes:
    """The table the build and finish models write for sorted entries, of
    at_least so many data blocks (and as many restarts in its index)."""
    blocks, _, rep = bm.build(entries, h.block_size, h.restart_interval, 1)
    assert rep["status"] == bm.OK and len(blocks) >= at_least
    return fm.finish(blocks, 1, 10, 0).image


def laid(runs):
    """Runs of (key, value) end to end: (entries, run_first)."""
    first = [0]
    for r in runs:
        first.append(first[-1] + len(r))
    return [e for r in runs for e in r], first


def runs_of(seed, memtable=True, flushed=False):
    """The runs db_scan merges, newest first: the memtable's entries as
    written (or, flushed, as its table stores them), then the tables'."""
    b = built(seed)
    head = [b[-1]["stored"]] if flushed else [b[-1]["raw"]] if memtable else []
    return head + [g["stored"] for g in b[-2::-1]]


class Files:
    """Every group's vTable as vtable_model.resolve takes them."""

    def __init__(self, seed):
        h, b = st.history(seed), built(seed)
        self.vtb = b"".join(g["vtb"] for g in b)
        self.size = [len(g["vtb"]) for g in b]
        self.off = [sum(self.size[:g]) for g in range(len(b))]
        self.number = h.file_numbers
        assert self.number == sorted(self.number)

    def value(self, stored: bytes):
        """(value, status) DecodeValue leaves of a stored value."""
        s, src, off, ln, _ = vm.resolve(stored, [0], [len(stored)], self.vtb, self.off, self.size,
                                        self.number)
        return ((self.vtb if src[0] else stored)[off[0]:off[0] + ln[0]] if s[0] == vm.R_OK else b"",
                s[0])


def merged(runs):
    entries, first = laid(runs)
    src, _, rep = gm.merge([k for k, _ in entries], [len(v) for _, v in entries], first)
    assert rep["status"] == gm.OK
    return [entries[e] for e in src]


def answers(entries, files, snapshot, ranges, reverse=False):
    """Per range [(user key, value, status)] by scan_model over `entries` (in
    merged order) and vtable_model."""
    keys = [k for k, _ in entries]
    out = []
    for start, limit, mx in ranges:
        counted, _, ok = sm.query(keys, snapshot, start, limit, mx)
        assert ok
        out.append([(keys[e][:-8],) + files.value(entries[e][1]) for e in counted][::-1 if reverse else 1])
    return out


def by_dictionary(store, snapshot, ranges, reverse=False):
    return [[(k, v, vm.R_OK) for k, v in store.scan(a, b, snapshot, mx, reverse)]
            for a, b, mx in ranges]


def compaction_settings(h):
    """(smallest_snapshot, deeper): 0, the middle of a group, a group's last
    sequence and the top, each with no deeper level and with two ranges over
    about half the user keys that end at b"" and at nine 0xff bytes."""
    n = len(h.users)
    deeper = [(b"", h.users[n // 4]), (h.users[3 * n // 4], b"\xff" * 9)]
    return [(s, d) for s in (0, (h.first[1] + h.last[1]) // 2, h.last[0], h.last[-1])
            for d in ((), deeper)]


def compacted(runs, s, deeper):
    """(survivors in order, report) of sst_merge_model's compaction of runs."""
    entries, first = laid(runs)
    src, _, rep = gm.merge([k for k, _ in entries], [len(v) for _, v in entries], first, 1, True,
                           s, deeper)
    assert rep["status"] == gm.OK
    return [entries[e] for e in src], rep


# ---- the histories --------------------------------------------------------------------------

@pytest.mark.parametrize("seed", SEEDS)
def test_history_has_what_the_gpu_tests_need(seed):
    h = st.history(seed)
    assert h is st.history(seed) and len(h.groups) == 4
    whole = h.store()
    seqs = [op[0] for g in h.ops for op in g]
    assert seqs == list(range(h.first[0], h.last[-1] + 1))  # consecutive, ascending
    assert all(300 <= len(g) <= 1200 for g in h.ops) and any(len(g) > T for g in h.ops)
    assert len(set(h.file_numbers)) == len(h.groups)
    assert all(W < len(g[0]) < 2 * W and len(g) > 3 for g in h.groups)
    top = whole.last(st.DELETED_LAST, sm.MAX_SEQUENCE)
    assert top == (h.last[-1], st.DELETED_LAST, None)
    in_group = [{u for _, u, _ in g} for g in h.ops]
    assert all(st.EVERY_GROUP in g for g in in_group)
    assert [st.ONLY_NEWEST in g for g in in_group] == [False, False, False, True]
    assert [st.ONLY_OLDEST in g for g in in_group] == [True, False, False, False]
    for g, ops in enumerate(h.ops):
        stored = [1 + len(v) for _, _, v in ops if v is not None]
        assert min(stored) < 16 <= max(stored) and min(stored) < 64 <= max(stored)
        assert any(v is None for _, _, v in ops)
        assert any(h.first[g] < s < h.last[g] for s in h.snapshots())
    assert {0, h.first[0] - 1, h.last[-1], sm.MAX_SEQUENCE, *h.last} <= set(h.snapshots())
    for k in st.SPECIAL:
        assert any(whole.get(k, s) is not None for s in h.snapshots()), k
    assert len(st.SPECIAL) == 22 and len(set(st.SPECIAL)) == 22 and len(st.LONGS[0]) == 300
    assert not set(st.ABSENT) & set(whole.of) and len(st.ABSENT) >= 12
    assert st.ABSENT[0] > h.users[0] == b"" and max(st.ABSENT) > h.users[-1] == b"\xff" * 9
    # the ranges: the whole store, every key and absent key, empty, backwards, none wanted,
    # one ending on an existing key
    r = h.ranges()
    assert r[0] == (b"", None, None) and len(r) > len(h.users) + len(st.ABSENT)
    assert any(a == b for a, b, _ in r) and any(b is not None and b < a for a, b, _ in r)
    assert any(mx == 0 for _, _, mx in r) and any(b in whole.of and a < b for a, b, _ in r)
    assert all(len(g["image"]) > 8 * h.block_size for g in built(seed))  # many data blocks


def test_one_history_is_longer_than_a_scan_tile():
    assert sorted(sum(map(len, st.history(s).ops)) > SCAN_TILE for s in SEEDS) == [False, False, True]


def test_the_dictionary_on_a_history_written_by_hand():
    s = st.Store([(5, b"k", b"v5"), (7, b"k", None), (9, b"k", b""), (6, b"j", b"w"), (8, b"", b"e")])
    assert [s.get(b"k", q) for q in (4, 5, 6, 7, 8, 9, 1 << 55)] == \
        [None, b"v5", b"v5", None, None, b"", b""]
    assert s.get(b"absent", 9) is None and s.last(b"k", 7) == (7, b"k", None)
    assert s.scan(b"", None, 9) == [(b"", b"e"), (b"j", b"w"), (b"k", b"")]
    assert s.scan(b"", None, 7) == [(b"j", b"w")]
    assert s.scan(b"", b"k", 9, 5, True) == [(b"j", b"w"), (b"", b"e")]
    assert s.scan(b"", None, 9, 2, True) == [(b"j", b"w"), (b"", b"e")]
    assert s.scan(b"j", b"j", 9) == [] and s.scan(b"k", b"j", 9) == [] and s.scan(b"", None, 9, 0) == []


# ---- the composition ------------------------------------------------------------------------

@pytest.mark.parametrize("seed", SEEDS)
def test_composed_models_give_the_dictionary_s_scans(seed):
    h, files = st.history(seed), Files(seed)
    with_mem, tables, flushed = (merged(runs_of(seed, **kw)) for kw in
                                 ({}, dict(memtable=False), dict(flushed=True)))
    assert len(with_mem) == sum(map(len, h.ops))
    whole, below = h.store(), h.store(range(len(h.groups) - 1))
    seen = 0
    for snapshot in h.snapshots():
        for reverse in (False, True):
            want = by_dictionary(whole, snapshot, h.ranges(), reverse)
            assert answers(with_mem, files, snapshot, h.ranges(), reverse) == want
            assert answers(flushed, files, snapshot, h.ranges(), reverse) == want
            assert answers(tables, files, snapshot, h.ranges(), reverse) == \
                by_dictionary(below, snapshot, h.ranges(), reverse)
        seen += bool(want[0])
    assert seen >= len(h.snapshots()) - 2  # (nothing at 0 and below the first write)


@pytest.mark.parametrize("seed", SEEDS)
def test_composed_models_give_the_dictionary_s_lookups(seed):
    """A table alone: Table::InternalGet's entry is the dictionary's last
    operation of that table's group."""
    h, files, b = st.history(seed), Files(seed), built(seed)
    for g in range(len(h.groups) - 1):
        keys = [k for k, _ in b[g]["stored"]]
        group = h.store([g])
        for snapshot in h.snapshots():
            for user in h.users + st.ABSENT:
                it = sm.DBIter(keys, snapshot)
                it.seek(user)  # (the first entry at or after (user, snapshot): seek_pos)
                e = it.seek_pos
                hit = e < len(keys) and keys[e][:-8] == user
                op = group.last(user, snapshot)
                assert hit == (op is not None)
                if hit:
                    assert sm.parse(keys[e])[1:] == (op[0], 0 if op[2] is None else 1)
                    if op[2] is not None:
                        assert files.value(b[g]["stored"][e][1]) == (op[2], vm.R_OK)


# ---- compaction -----------------------------------------------------------------------------

@pytest.mark.parametrize("seed", SEEDS)
def test_compaction_changes_nothing_at_or_above_its_snapshot(seed):
    h, files = st.history(seed), Files(seed)
    runs = runs_of(seed, memtable=False)
    below = h.store(range(len(h.groups) - 1))
    dropped = set()
    for s, deeper in compaction_settings(h):
        kept, rep = compacted(runs, s, deeper)
        dropped |= {bool(rep["num_hidden"]), 2 * bool(rep["num_obsolete"])}
        assert rep["num_out"] + rep["num_hidden"] + rep["num_obsolete"] == rep["num_in"]
        for snapshot in h.snapshots():
            if snapshot >= s:
                assert answers(kept, files, snapshot, h.ranges()) == \
                    by_dictionary(below, snapshot, h.ranges()), (s, snapshot)
        if not deeper:
            # the oldest two first, then their survivors with the newest
            older, _ = compacted(runs[1:], s, ())
            assert compacted([runs[0], older], s, ())[0] == kept
    assert dropped >= {1, 2}
