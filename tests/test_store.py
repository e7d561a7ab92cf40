"""The store end to end on the device, against the dictionary of
tests/store_model.py: seeded histories (tests/test_store_model.py says what
they hold) written through wal_recover_table and memtable_from_batches, then
read through db_scan and sst_get_values, compacted through sst_compact_tables
and flushed through sst_flush_separated. Every result is compared in full.

The seams the histories cross: a group of more than a sort tile (a table's
group or the memtable's, by the seed), a batch a group longer than the parse
window, logs of more than one 32 KiB block, tables of dozens of data blocks
and as many index restarts, three or four runs whose buffers are laid end to
end with padding, for one seed a merged list of more than a scan tile, more
lookups than a workgroup has lanes, values on both sides of each table's
kv_sep_size resolved through three or four value logs.

A store is built once a seed and kept; the scans of the original store are
kept too, since the compaction and the flush are compared with them.
"""
from __future__ import annotations

import numpy as np
import pytest

import scan_model as sm
import store_model as st
import vtable_model as vm
from test_sst_scan import _listed
from test_store_model import (SEEDS, built, by_dictionary, compacted, compaction_settings, runs_of,
                              table_image)
from test_vtable import Packed

_STORES = {}


class DeviceStore:
    """history(seed) on the device: tables[g] / vtbs[number] of the table
    groups (oldest first), mem the live group's memtable_from_batches."""

    def __init__(self, lvkv, gpu, seed):
        import torch
        self.torch, self.lvkv, self.gpu = torch, lvkv, gpu
        self.h = h = st.history(seed)
        self.build = dict(block_size=h.block_size, restart_interval=h.restart_interval,
                          compression=0, filter_bits_per_key=10)
        self.read = dict(filter_policy=lvkv.BLOOM_POLICY, max_ulen=lvkv.SNAPPY_MAX_BLOCK)
        self.tables, self.vtbs, self.sequences = [], {}, []
        for g in range(len(h.groups) - 1):
            image, vimage, _, seq = lvkv.wal_recover_table(
                self.bytes_on_device(h.log(g)), file_number=h.file_numbers[g],
                kv_sep_size=h.kv_sep[g], **self.build)
            self.tables.append(image)
            self.vtbs[h.file_numbers[g]] = vimage
            self.sequences.append(seq)
        payload, offs, lens = h.payload(len(h.groups) - 1)
        i64 = lambda v: torch.tensor(v, dtype=torch.int64, device=gpu)
        self.mem = lvkv.memtable_from_batches(self.bytes_on_device(payload), i64(offs), i64(lens),
                                              max_sequence=h.last[-2])
        self.ranges = h.ranges()
        self.kept = {}
        # Get's queries: every user key and absent key at every snapshot
        self.asked = [(u, s) for s in h.snapshots() for u in h.users + st.ABSENT]
        self.queries = Packed(torch, gpu, [u + ((s << 8) | 1).to_bytes(8, "little")
                                           for u, s in self.asked])

    def bytes_on_device(self, b: bytes):
        return self.torch.tensor(np.frombuffer(b, dtype=np.uint8).copy(), device=self.gpu)

    def scan(self, snapshot, reverse, files=None, vtbs=None, memtable=True):
        """db_scan of every range: (per range [(key, value, status)], q_status)."""
        res = self.lvkv.db_scan(
            self.tables[::-1] if files is None else files, self.vtbs if vtbs is None else vtbs,
            [a for a, _, _ in self.ranges], [b for _, b, _ in self.ranges], snapshot=snapshot,
            memtable=self.mem[1:7] if memtable else None, max_count=[m for _, _, m in self.ranges],
            reverse=reverse, **self.read)
        assert res["merge"]["status"] == self.lvkv.MERGE_OK and res["scan"]["status"] == sm.OK
        return _listed(res), res["q_status"].cpu().tolist()

    def original(self, snapshot, reverse):
        """scan() of the store as it was built, asked once."""
        if (snapshot, reverse) not in self.kept:
            self.kept[snapshot, reverse] = self.scan(snapshot, reverse)
        return self.kept[snapshot, reverse]

    def lookups(self, image):
        """sst_get_values of every query on one table: [(state, status, value)]."""
        n = len(self.asked)
        got = self.lvkv.sst_get_values(image, self.vtbs, self.queries.buf, self.queries.off[:n],
                                       self.queries.len[:n], **self.read)
        values = bytes(got["values"].cpu().numpy())
        offs = got["value_off"].cpu().tolist()
        return list(zip(got["state"].cpu().tolist(), got["status"].cpu().tolist(),
                        [values[a:b] for a, b in zip(offs, offs[1:])]))

    def original_level0(self):
        """level0() over the tables as they were built, asked once."""
        if "level0" not in self.kept:
            self.kept["level0"] = self.level0([self.lookups(t) for t in self.tables[::-1]])
        return self.kept["level0"]

    def level0(self, per_table):
        """The level-0 loop of Version::Get on the host, over lookups() of the
        tables newest first: the newest table in which the key is found or
        deleted decides. [(status, value)]."""
        found, deleted = self.lvkv.GET_STATE_FOUND, self.lvkv.GET_STATE_DELETED
        out = []
        for q in range(len(self.asked)):
            hit = next((t[q] for t in per_table if t[q][0] in (found, deleted)), None)
            out.append((vm.R_SKIPPED, b"") if hit is None else hit[1:])
        return out


def store_of(lvkv, gpu, seed) -> DeviceStore:
    if seed not in _STORES:
        _STORES[seed] = DeviceStore(lvkv, gpu, seed)
    return _STORES[seed]


def image_bytes(t) -> bytes:
    return bytes(t.cpu().numpy())


def asked_of(lvkv, store, user, snapshot):
    """(state, status, value) the dictionary `store` gives one Get, the state
    in sst_get's encoding."""
    op = store.last(user, snapshot)
    if op is None:
        return lvkv.GET_STATE_NOT_FOUND, vm.R_SKIPPED, b""
    if op[2] is None:
        return lvkv.GET_STATE_DELETED, vm.R_SKIPPED, b""
    return lvkv.GET_STATE_FOUND, vm.R_OK, op[2]


# ---- the store as built ---------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("seed", SEEDS)
def test_recovery_writes_the_models_tables_and_memtable(lvkv, gpu, seed):
    """Seams: the log's 32 KiB blocks, the parse window, the sort tile, the
    data blocks."""
    d, b = store_of(lvkv, gpu, seed), built(seed)
    h = d.h
    assert d.sequences == h.last[:-1]
    for g, image in enumerate(d.tables):
        assert image is not None
        assert image_bytes(image) == b[g]["image"], g
        assert image_bytes(d.vtbs[h.file_numbers[g]]) == b[g]["vtb"], g
    rep = d.mem[0]
    assert rep["status"] == lvkv.MEMTABLE_OK and rep["nentries"] == len(h.ops[-1])
    assert rep["max_sequence_out"] == h.last[-1]
    keys, payload = image_bytes(d.mem[1]), image_bytes(d.mem[4])
    entries = [(keys[ko:ko + kl], payload[vo:vo + vl]) for ko, kl, vo, vl in
               zip(*(d.mem[k].cpu().tolist() for k in (2, 3, 5, 6)))]
    assert entries == b[-1]["raw"]


@pytest.mark.gpu
@pytest.mark.parametrize("seed", SEEDS)
def test_scans_at_every_snapshot_give_the_dictionary_s(lvkv, gpu, seed):
    """Seams: the run boundaries of the merge (a memtable and three tables),
    the scan tile and its workgroups, the value logs."""
    d = store_of(lvkv, gpu, seed)
    whole = d.h.store()
    for snapshot in d.h.snapshots():
        for reverse in (False, True):
            got, q_status = d.original(snapshot, reverse)
            assert got == by_dictionary(whole, snapshot, d.ranges, reverse), (snapshot, reverse)
            assert q_status == [sm.Q_OK] * len(d.ranges)


@pytest.mark.gpu
@pytest.mark.parametrize("seed", SEEDS)
def test_point_lookups_give_the_dictionary_s(lvkv, gpu, seed):
    """Seams: the index's restarts and the data blocks of each table, the
    filter, the value logs; then the tables in Version::Get's order."""
    d = store_of(lvkv, gpu, seed)
    h = d.h
    per_table = []
    for g, image in enumerate(d.tables):
        group = h.store([g])
        got = d.lookups(image)
        assert got == [asked_of(lvkv, group, u, s) for u, s in d.asked], g
        per_table.append(got)
    below = h.store(range(len(d.tables)))
    assert d.level0(per_table[::-1]) == [asked_of(lvkv, below, u, s)[1:] for u, s in d.asked]


# ---- compaction -----------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("setting", range(8))
@pytest.mark.parametrize("seed", SEEDS)
def test_compaction_changes_nothing_at_or_above_its_snapshot(lvkv, gpu, seed, setting):
    """Seams: the runs' buffers laid end to end, the drop pass over the merged
    list, the rebuilt table's blocks. Nothing is asserted below the snapshot."""
    d = store_of(lvkv, gpu, seed)
    h = d.h
    s, deeper = compaction_settings(h)[setting]
    assert len(compaction_settings(h)) == 8

    def compact(files):
        out = lvkv.sst_compact_tables(files, smallest_snapshot=s, deeper=list(deeper) or None,
                                      **d.read, **d.build)
        assert out[7]["status"] == lvkv.MERGE_OK
        assert out[6]["status"] == lvkv.BUILD_OK and out[5]["status"] == lvkv.TABLE_OK
        return out[0][:out[5]["file_size"]].clone(), out[7]

    table, rep = compact(d.tables[::-1])
    kept, want = compacted(runs_of(seed, memtable=False), s, deeper)
    assert rep == want  # num_out, num_hidden, num_obsolete and the byte counts
    one_step = image_bytes(table)
    assert one_step == table_image(h, kept)
    for snapshot in h.snapshots():
        if snapshot >= s:
            for reverse in (False, True):
                assert d.scan(snapshot, reverse, files=[table]) == d.original(snapshot, reverse), \
                    (snapshot, reverse)
    asked = [q for q, (_, snapshot) in enumerate(d.asked) if snapshot >= s]
    assert asked
    got, originals = d.level0([d.lookups(table)]), d.original_level0()
    assert [got[q] for q in asked] == [originals[q] for q in asked]
    if not deeper:
        # the oldest two tables first, then their table with the newest
        older, _ = compact(d.tables[1::-1])
        again, _ = compact([d.tables[2], older])
        assert image_bytes(again) == one_step


# ---- the live group flushed ----------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("seed", SEEDS)
def test_the_flushed_memtable_reads_as_the_live_one(lvkv, gpu, seed):
    """Seams: the memtable's entries as a table's blocks, its large values in
    a value log of their own."""
    d, b = store_of(lvkv, gpu, seed), built(seed)
    h = d.h
    table, vtb, reports = lvkv.sst_flush_separated(
        *d.mem[1:7], kv_sep_size=h.kv_sep[-1], file_number=h.file_numbers[-1], **d.build)
    assert table is not None and reports["table"]["status"] == lvkv.TABLE_OK
    assert image_bytes(table) == b[-1]["image"] and image_bytes(vtb) == b[-1]["vtb"]
    vtbs = dict(d.vtbs)
    vtbs[h.file_numbers[-1]] = vtb
    for snapshot in h.snapshots():
        for reverse in (False, True):
            got = d.scan(snapshot, reverse, files=[table] + d.tables[::-1], vtbs=vtbs,
                         memtable=False)
            assert got == d.original(snapshot, reverse), (snapshot, reverse)
