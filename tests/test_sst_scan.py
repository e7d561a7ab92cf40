"""lvkv_sst_scan_entries_device: DBIter over entries in MergingIterator's order
at a snapshot, on the device, and sst_scan_entries / db_scan on top of it.

The expectation is tests/scan_model.py -- the reference's sequential walk,
pinned against the reference in test_scan_model.py. The GPU tests call the C
entry point on buffers that persist over calls, filled and between borders, and
compare the whole of every output array, the three per-query arrays and the
report with the model: what a call does not write must still hold what was
there.

The counts the kernels change path at are read from the sources: the lanes a
workgroup of lvkv_sst_scan.hip (entries and queries alike), and the tile of the
scans that number the eligible and the visible entries.
"""
from __future__ import annotations

import ctypes
import re

import numpy as np
import pytest

import memtable_model as memm
import scan_model as sm
import store_model as st
import vtable_model as vm
from conftest import GOLDEN, REPO
from test_memtable import batches_of, laid_out
from test_memtable_model import FILE_NUMBER, log_of
from test_scan_model import CASES, case_merged, pairs
from test_sst_merge_entries import _pack, ikey, versions
from test_vtable_model import TABLES, table

FILL = 0xC3
BORDER = 4096
SLOT_FILL64 = -0x3C3C3C3C3C3C3C3D
SLOT_FILL32 = -0x3C3C3C3D
CSRC = REPO / "leveldb-kv-separation_amd" / "csrc"
_const = lambda file, name: int(re.search(rf"constexpr uint32_t {name} = (\d+);",
                                          (CSRC / file).read_text()).group(1))
TILE = _const("lvkv_launch.h", "kScanTile")
GROUP = _const("lvkv_sst_scan.hip", "kGroup")
ENTRY_ARRAYS = ("out_key_off", "out_key_len", "out_val_off", "out_val_len", "out_src")
QUERY_ARRAYS = ("q_first", "q_count", "q_status")


class Buffers:
    """The output side of a call, kept over calls, between borders, and on
    the host what it must hold: the fill, with everything an earlier call
    wrote laid over it."""

    def __init__(self, torch, dev, lvkv, max_entries, max_queries=16):
        self.torch, self.dev, self.lvkv = torch, dev, lvkv
        self.max_entries, self.max_queries = max_entries, max_queries
        self.need = lvkv.lib.lvkv_sst_scan_entries_scratch_bytes(max_entries, max_queries)
        full = lambda n, v, t: torch.full((n,), v, dtype=t, device=dev)
        ne, nq = max_entries + 64, max_queries + 64
        self.dev_bufs = {
            "out_key_off": full(ne, SLOT_FILL64, torch.int64),
            "out_key_len": full(ne, SLOT_FILL32, torch.int32),
            "out_val_off": full(ne, SLOT_FILL64, torch.int64),
            "out_val_len": full(ne, SLOT_FILL32, torch.int32),
            "out_src": full(ne, SLOT_FILL32, torch.int32),
            "q_first": full(nq, SLOT_FILL32, torch.int32),
            "q_count": full(nq, SLOT_FILL32, torch.int32),
            "q_status": full(nq, FILL, torch.uint8),
        }
        self.scratch = full(self.need + BORDER, FILL, torch.uint8)
        self.rep = full(ctypes.sizeof(lvkv.SstScanReport), FILL, torch.uint8)
        self.want = {k: v.cpu().numpy().copy() for k, v in self.dev_bufs.items()}


class Call:
    """One call's inputs on the device and its launch; check() compares with
    the model after a synchronize."""

    def __init__(self, buf, entries, snapshot, queries=(), *, max_out=None, aligned=False, gap=1,
                 null_max=False, rep=None):
        torch, dev, lvkv = buf.torch, buf.dev, buf.lvkv
        self.buf, self.snapshot, self.queries = buf, snapshot, list(queries)
        self.keys = [k for k, _ in entries]
        self.vlen = [v if isinstance(v, int) else len(v) for _, v in entries]
        n, nq = len(entries), len(self.queries)
        self.max_out = n if max_out is None else max_out
        assert n <= buf.max_entries and self.max_out <= buf.max_entries and nq <= buf.max_queries
        khost, self.koff = _pack(self.keys, gap, aligned)
        self.voff = [1000 + 3 * i for i in range(n)]  # (no value byte is read)
        qpieces = [s for s, _, _ in self.queries] + [l or b"" for _, l, _ in self.queries]
        qhost, qoff = _pack(qpieces, 3, False)
        i64 = lambda v: torch.tensor(v or [0], dtype=torch.int64, device=dev)
        i32 = lambda v: torch.tensor([x - (1 << 32) if x >= 1 << 31 else x for x in v] or [0],
                                     dtype=torch.int32, device=dev)
        if null_max:
            assert all(m is None for _, _, m in self.queries)
        self.t = [torch.from_numpy(khost).to(dev), i64(self.koff), i32([len(k) for k in self.keys]),
                  i64(self.voff), i32(self.vlen), torch.from_numpy(qhost).to(dev), i64(qoff[:nq]),
                  i32([len(s) for s, _, _ in self.queries]), i64(qoff[nq:]),
                  i32([sm.NO_LIMIT if l is None else len(l) for _, l, _ in self.queries]),
                  i32([0xFFFFFFFF if m is None else m for _, _, m in self.queries])]
        if aligned:
            assert self.t[0].data_ptr() % 8 == 0 and all(o % 8 == 0 for o in self.koff)
        p = lambda t: ctypes.c_void_p(t.data_ptr())
        assert lvkv.lib.lvkv_sst_scan_entries_scratch_bytes(n, nq) <= buf.need
        d = buf.dev_bufs
        self.rep = buf.rep if rep is None else rep
        stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        k, ko, kl, vo, vl, qk, so, sl, lo, ll, qm = self.t
        rc = lvkv.lib.lvkv_sst_scan_entries_device(
            p(k), p(ko), p(kl), p(vo), p(vl), n, snapshot,
            p(qk) if nq else None, p(so) if nq else None, p(sl) if nq else None,
            p(lo) if nq else None, p(ll) if nq else None, None if null_max or not nq else p(qm), nq,
            p(buf.scratch), buf.need, p(d["out_key_off"]), p(d["out_key_len"]),
            p(d["out_val_off"]), p(d["out_val_len"]), p(d["out_src"]), self.max_out,
            p(d["q_first"]), p(d["q_count"]), p(d["q_status"]), p(self.rep), stream)
        assert rc == 0

    def expect(self):
        """The model's outputs laid over what the buffers must hold."""
        src, per_query, want = sm.scan(self.keys, self.vlen, self.snapshot, self.queries,
                                       self.max_out)
        w = self.buf.want
        if want["status"] == sm.OK and self.keys:
            no = len(src)
            w["out_key_off"][:no] = [self.koff[e] for e in src]
            w["out_key_len"][:no] = [len(self.keys[e]) - 8 for e in src]
            w["out_val_off"][:no] = [self.voff[e] for e in src]
            w["out_val_len"][:no] = [self.vlen[e] for e in src]
            w["out_src"][:no] = src
            nq = len(per_query)
            w["q_first"][:nq] = [f for f, _, _ in per_query]
            w["q_count"][:nq] = [c for _, c, _ in per_query]
            w["q_status"][:nq] = [s for _, _, s in per_query]
        return src, per_query, want

    def check(self):
        buf = self.buf
        buf.torch.cuda.synchronize()
        rep = buf.lvkv.SstScanReport.from_buffer_copy(bytes(self.rep.cpu().numpy())).as_dict()
        src, per_query, want = self.expect()
        print("report", rep)
        assert rep == want
        for name in ENTRY_ARRAYS + QUERY_ARRAYS:
            got = buf.dev_bufs[name].cpu().numpy()
            w = buf.want[name]
            wrong = np.nonzero(got != w)[0]
            assert wrong.size == 0, f"{name}[{wrong[0]}] is {got[wrong[0]]}, not {w[wrong[0]]}"
        assert (buf.scratch[buf.need:].cpu().numpy() == FILL).all(), "a write past the scratch"
        return src, per_query, want


def _fresh(lvkv, gpu, n, nq=16):
    import torch
    return Buffers(torch, gpu, lvkv, n, nq)


def some_queries(keys, rng, k=8):
    """k ranges over the user keys of `keys`: on a key, between keys, before
    the first and after the last, with and without a limit and a maximum."""
    users = sorted({key[:-8] for key in keys if len(key) >= 8}) or [b"a"]
    out = [(b"", None, None), (users[-1] + b"\xff", None, 3), (users[0], users[0], None)]
    while len(out) < k:
        a, b = (users[int(i)] for i in rng.integers(0, len(users), 2))
        kind = int(rng.integers(0, 5))
        out.append((a + (b"\x00" if kind == 0 else b""), None if kind == 1 else b,
                    None if kind < 3 else int(rng.integers(0, 6))))
    return out[:k]


# ---- the reference's cases ---------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_fixture_cases(lvkv, gpu, name):
    """Every case, snapshot and query of the reference's."""
    spec, merged, order, _, qkeys = case_merged(name)
    nq = max(len(s["queries"]) for s in spec["snapshots"])
    buf = _fresh(lvkv, gpu, max(1, len(merged)), nq)
    for k, s in enumerate(spec["snapshots"]):
        queries = [(qkeys[a], None if b < 0 else qkeys[b], None if c < 0 else c)
                   for a, b, c, _, _, _ in s["queries"]]
        src, per_query, rep = Call(buf, merged, s["snapshot"], queries, aligned=k % 2 == 1).check()
        if not merged:
            continue
        # the reference's own walk, not only the model's
        assert [order[e] for e in src] == pairs(s["forward"])
        for (first, n, status), q in zip(per_query, s["queries"]):
            assert (n, status == sm.Q_OK) == (q[4], q[5])
            assert first == (q[3] if q[3] >= 0 else len(src))


# ---- entry counts and seams ----------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, GROUP - 1, GROUP, GROUP + 1, TILE - 1, TILE, TILE + 1,
                               2 * TILE + GROUP + 3])
def test_entry_counts(lvkv, gpu, n):
    rng = np.random.default_rng(n)
    entries = versions(n)
    buf = _fresh(lvkv, gpu, n)
    keys = [k for k, _ in entries]
    for snapshot in (sm.MAX_SEQUENCE, 600, 200):
        src, _, rep = Call(buf, entries, snapshot, some_queries(keys, rng, 6)).check()
    assert n < 3 or rep["num_above_snapshot"] > 0


def seam_case(at, nversions=7):
    """Plain keys with one user key in `nversions` versions -- values, a
    deletion in the middle, a value above every snapshot first -- such that
    the versions lie around position `at`."""
    lead = at - nversions // 2
    out = [(ikey(b"a%07d" % i, 50), 5) for i in range(lead)]
    out += [(ikey(b"b-many", 1000 - 100 * v, 0 if v == 3 else 1), 7 + v) for v in range(nversions)]
    out += [(ikey(b"c%07d" % i, 60 + i % 3), 6) for i in range(GROUP + 9)]
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("seam", ["group", "tile"])
def test_versions_of_one_user_key_straddle_a_seam(lvkv, gpu, seam):
    at = GROUP if seam == "group" else TILE
    entries = seam_case(at)
    keys = [k for k, _ in entries]
    assert keys[at - 1][:-8] == keys[at][:-8] == b"b-many"
    buf = _fresh(lvkv, gpu, len(entries))
    queries = [(b"b-many", None, 2), (b"b", b"c", None), (b"b-many", b"b-many\x00", None)]
    for snapshot in (2000, 950, 850, 750, 650, 450, 399):
        src, per_query, _ = Call(buf, entries, snapshot, queries).check()
        # one version at the most, whichever side of the seam it lies on
        assert per_query[1][1] == per_query[2][1] == (0 if 700 <= snapshot < 800 or snapshot < 400 else 1)


@pytest.mark.gpu
def test_more_than_a_tile_of_ineligible_entries_before_the_previous_eligible_one(lvkv, gpu):
    gap = TILE + GROUP + 5
    # one user key: an eligible value, `gap` unparsable keys, a value it hides
    same = [(ikey(b"k", 9000), 3)] + [(ikey(b"k", 8000 - i, 2), 1) for i in range(gap)] + \
        [(ikey(b"k", 10), 4)]
    # other user keys in between, all above the snapshot: the last value is seen
    other = [(ikey(b"m", 5), 3)] + [(ikey(b"n%06d" % i, 9500), 1) for i in range(gap)] + \
        [(ikey(b"o", 7), 4)]
    entries = same + other
    buf = _fresh(lvkv, gpu, len(entries))
    queries = [(b"", None, None), (b"k", b"l", None), (b"m", None, 1), (b"n", None, None)]
    src, per_query, rep = Call(buf, entries, 9000, queries).check()
    assert src == [0, len(same), len(entries) - 1]
    assert (rep["num_unparsable"], rep["num_above_snapshot"], rep["num_hidden"]) == (gap, gap, 1)
    assert [s for _, _, s in per_query] == [sm.Q_CORRUPT, sm.Q_CORRUPT, sm.Q_OK, sm.Q_OK]


@pytest.mark.gpu
def test_none_eligible_and_all_visible(lvkv, gpu):
    n = TILE + 77
    entries = [(ikey(b"u%06d" % i, 5 + i % 3), i % 11) for i in range(n)]
    buf = _fresh(lvkv, gpu, n)
    queries = [(b"", None, None), (b"u000100", b"u000200", None), (b"u000100", b"u000200", 17)]
    src, per_query, rep = Call(buf, entries, 4, queries).check()
    assert src == [] and rep["num_above_snapshot"] == n and [c for _, c, _ in per_query] == [0] * 3
    src, per_query, rep = Call(buf, entries, 7, queries).check()
    assert src == list(range(n)) and [c for _, c, _ in per_query] == [n, 100, 17]
    assert rep["max_count"] == n and rep["sum_count"] == n + 117
    # only deletions and unparsable keys
    dead = [(ikey(b"u%06d" % i, 5, 2 * (i % 2)), 1) for i in range(300)]
    src, per_query, rep = Call(buf, dead, 7, queries[:1]).check()
    assert src == [] and (rep["num_deletions"], rep["num_unparsable"]) == (150, 150)


# ---- key shapes -------------------------------------------------------------------------

# a second alphabet for the seeded user keys: the bytes a signed compare and a compare that
# stops at a zero byte get wrong
WIDE = np.array([0x00, 0x61, 0x7f, 0x80, 0xff], dtype=np.uint8)


def draw(rng, n, alphabet, lo, hi):
    """n bytes of the alphabet, or -- none given -- of lo .. hi - 1 (the
    draws the seeded cases have always made)."""
    if alphabet is None:
        return rng.integers(lo, hi, n, dtype=np.uint8).tobytes()
    return alphabet[rng.integers(0, len(alphabet), n)].tobytes()


def with_prefixes(users):
    """The keys and the first half of each: keys that are prefixes of others."""
    return sorted(set(users) | {u[:len(u) // 2] for u in users})


@pytest.mark.gpu
@pytest.mark.parametrize("aligned,gap", [(True, 0), (False, 0), (False, 1), (False, 3), (False, 7)])
def test_keys_at_odd_and_aligned_offsets(lvkv, gpu, aligned, gap):
    offsets_case(lvkv, gpu, aligned, gap, None)


@pytest.mark.gpu
@pytest.mark.parametrize("aligned,gap", [(True, 0), (False, 0), (False, 3)])
def test_wide_alphabet_keys_at_odd_and_aligned_offsets(lvkv, gpu, aligned, gap):
    offsets_case(lvkv, gpu, aligned, gap, WIDE)


def offsets_case(lvkv, gpu, aligned, gap, alphabet):
    rng = np.random.default_rng(gap + 10 * aligned)
    users = sorted({draw(rng, int(rng.integers(0, 20)), alphabet, 97, 100) for _ in range(120)})
    if alphabet is not None:
        users = with_prefixes(users)
    entries = []
    for i, u in enumerate(users):
        entries += [(ikey(u, s, t), 4) for s, t in ((90, 1), (60, i % 3 and 1), (30, 1))][:1 + i % 3]
    buf = _fresh(lvkv, gpu, len(entries))
    keys = [k for k, _ in entries]
    for snapshot in (100, 70, 40):
        Call(buf, entries, snapshot, some_queries(keys, rng, 12), aligned=aligned, gap=gap).check()


@pytest.mark.gpu
@pytest.mark.parametrize("klen", [300, 2000])
@pytest.mark.parametrize("aligned", [False, True])
def test_long_keys_that_differ_in_their_last_byte(lvkv, gpu, klen, aligned):
    rng = np.random.default_rng(klen)
    stem = rng.integers(0, 256, klen - 1, dtype=np.uint8).tobytes()
    entries = []
    for b in range(0, 40):
        user = stem + bytes([b])
        entries += [(ikey(user, 50, 1), 9), (ikey(user, 40, b % 2), 9), (ikey(user, 30, 1), 9)]
    buf = _fresh(lvkv, gpu, len(entries))
    queries = [(stem + b"\x07", stem + b"\x0b", None), (stem, None, 3), (stem + b"\x27", None, None),
               (stem + b"\x27\x00", None, None), (stem[:-1], stem + b"\x02", None),
               (stem + b"\x10", stem + b"\x10", None), (stem + b"\x10", stem + b"\x0f", None)]
    src, per_query, _ = Call(buf, entries, 45, queries, aligned=aligned, gap=0 if aligned else 1).check()
    assert [c for _, c, _ in per_query] == [2, 3, 1, 0, 1, 0, 0]
    assert len(src) == 20  # (the versions at 40: values for odd b)
    Call(buf, entries, 35, queries, aligned=aligned, gap=0 if aligned else 5).check()


# ---- the store's special keys ---------------------------------------------------------------

def near_misses(k):
    out = [k + b"\x00"]
    if k:
        out.append(k[:-1])
        if k[-1]:
            out.append(k[:-1] + bytes([k[-1] - 1]))
    return out


def special_case(seam, which):
    """Every key of store_model.SPECIAL in several versions (a deletion every
    fourth), the versions of `which` lying around position `seam`. Returns
    (entries, queries, snapshots)."""
    users = sorted(st.SPECIAL)
    before = users[:users.index(which)]
    nv = {u: 5 for u in users}
    nv[which] = 9
    fill = seam - nv[which] // 2 - 5 * len(before)
    assert before and fill >= 0
    for j, u in enumerate(before):
        nv[u] += fill // len(before) + (j < fill % len(before))
    entries = [(ikey(u, 9000 - 3 * v, 0 if v % 4 == 3 else 1), 1 + v % 7)
               for u in users for v in range(nv[u])]
    keys = [k for k, _ in entries]
    assert keys[seam - 1][:-8] == keys[seam][:-8] == which
    pool = sorted(set(users) | {m for u in users for m in near_misses(u)})
    queries = [(p, None, 2) for p in pool] + [(p, q, None) for p, q in zip(pool, pool[1:])] + \
        [(which, None, None), (b"", which, None), (which, which[:-1], None)]
    # (readers that see version 0, 2, 6 and 8 first: values, the last two of the longer keys)
    return entries, queries, (sm.MAX_SEQUENCE, 9000 - 3 * 2, 9000 - 3 * 5 - 1, 9000 - 3 * 8)


@pytest.mark.gpu
@pytest.mark.parametrize("which", [b"a\x00", st.PAIRS[1], b"\xff" * 8],
                         ids=["zero_padded", "pair_at_8", "eight_ff"])
@pytest.mark.parametrize("seam", ["group", "tile"])
def test_order_of_the_special_keys_across_a_seam(lvkv, gpu, seam, which):
    """Order decided past a shared prefix, by a zero byte, by 0x7f against
    0x80 and among 0xff bytes, with one key's versions across a workgroup's
    end or the scan tile's; starts and limits on the keys and on their near
    misses."""
    entries, queries, snapshots = special_case(GROUP if seam == "group" else TILE, which)
    buf = _fresh(lvkv, gpu, len(entries), len(queries))
    for k, snapshot in enumerate(snapshots):
        src, per_query, rep = Call(buf, entries, snapshot, queries, aligned=k == 1,
                                   gap=(1, 0, 3, 7)[k]).check()
        assert rep["num_visible"] and rep["num_hidden"]
    assert rep["num_above_snapshot"] and rep["num_deletions"]


# ---- queries ----------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("nq", [0, 1, GROUP - 1, GROUP, GROUP + 1, 2 * GROUP + 5])
def test_query_counts(lvkv, gpu, nq):
    rng = np.random.default_rng(nq)
    entries = versions(90, every=3)
    keys = [k for k, _ in entries]
    buf = _fresh(lvkv, gpu, len(entries), max(nq, 1))
    queries = some_queries(keys, rng, nq)
    # duplicate and overlapping ranges
    for i in range(5, nq, 7):
        queries[i] = queries[i - 3]
    src, per_query, rep = Call(buf, entries, 600, queries).check()
    assert rep["nqueries"] == nq and len(per_query) == nq
    if nq:
        no_max = [(s, l, None) for s, l, _ in queries]
        Call(buf, entries, 950, no_max, null_max=True).check()


# ---- statuses -----------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("where", ["first", "middle", "last"])
def test_whole_call_statuses_and_their_precedence(lvkv, gpu, where):
    n = TILE + GROUP + 2
    good = [(ikey(b"s%06d" % (i // 2), 9 - i % 2), 2) for i in range(n)]
    at = {"first": 0, "middle": TILE, "last": n - 1}[where]
    buf = _fresh(lvkv, gpu, n)
    queries = [(b"", None, None), (b"s000009", None, 4)]
    Call(buf, good, 100, queries).check()  # (the arrays now hold a good call's words)
    # BAD_KEY: a key under 8 bytes
    for short in (b"", b"1234567"):
        bad = list(good)
        bad[at] = (short, 2)
        _, _, rep = Call(buf, bad, 100, queries).check()
        assert (rep["status"], rep["first_bad_entry"]) == (sm.BAD_KEY, at)
    # UNSORTED: an entry below its predecessor (by the user key, by the trailer)
    un = max(at, 1)
    for lower in (ikey(b"a", 5), good[un - 1][0][:-8] + ((10 << 8) | 1).to_bytes(8, "little")):
        bad = list(good)
        bad[un] = (lower, 2)
        _, _, rep = Call(buf, bad, 100, queries).check()
        assert (rep["status"], rep["first_bad_entry"]) == (sm.UNSORTED, un)
    # BAD_KEY wins over an UNSORTED before it, and the lowest of each kind is reported
    bad = list(good)
    bad[1] = (ikey(b"a", 5), 2)
    bad[un] = (ikey(b"a", 4), 2) if un > 1 else bad[un]
    bad[n - 2] = (b"short", 2)
    bad[n // 2] = (b"short", 2)
    _, _, rep = Call(buf, bad, 100, queries, max_out=1).check()
    assert (rep["status"], rep["first_bad_entry"]) == (sm.BAD_KEY, n // 2)
    bad[n // 2], bad[n - 2] = good[n // 2], good[n - 2]
    _, _, rep = Call(buf, bad, 100, queries, max_out=1).check()
    assert (rep["status"], rep["first_bad_entry"]) == (sm.UNSORTED, 1)
    # equal keys are legal
    eq = list(good)
    eq[un] = eq[un - 1]
    assert Call(buf, eq, 100, queries).check()[2]["status"] == sm.OK


@pytest.mark.gpu
def test_capacity_one_short_then_the_repeat(lvkv, gpu):
    entries = versions(TILE + 300)
    buf = _fresh(lvkv, gpu, len(entries))
    queries = [(b"", None, None), ((7).to_bytes(8, "big"), None, 9)]
    nvis = len(sm.forward_walk([k for k, _ in entries], 600)[0])
    for max_out in (0, nvis - 1):
        src, per_query, rep = Call(buf, entries, 600, queries, max_out=max_out).check()
        assert (src, per_query, rep["status"], rep["num_visible"]) == ([], [], sm.CAPACITY, nvis)
    src, _, rep = Call(buf, entries, 600, queries, max_out=rep["num_visible"]).check()
    assert rep["status"] == sm.OK and len(src) == nvis


# ---- seeded cases, reuse -----------------------------------------------------------------------

def random_case(rng, alphabet=None):
    nusers = int(rng.integers(1, 14))
    users = sorted({draw(rng, int(rng.integers(0, 5)), alphabet, 97, 99) for _ in range(nusers)})
    if alphabet is not None:
        users = with_prefixes(users)
    entries = []
    for u in users:
        tags = sorted({(int(rng.integers(0, 12)) << 8) | int(rng.choice([0, 1, 1, 1, 2]))
                       for _ in range(int(rng.integers(1, 6)))}, reverse=True)
        for t in tags:
            entries += [(u + t.to_bytes(8, "little"), int(rng.integers(0, 9)))] * \
                (2 if rng.integers(0, 8) == 0 else 1)  # (the same key from two runs)
    snapshot = int(rng.choice([0, 3, 6, 9, 12, sm.MAX_SEQUENCE]))
    pool = users + [u + b"\x00" for u in users] + [b"", b"zz", b"a", b"b"]
    pick = lambda: pool[int(rng.integers(0, len(pool)))]
    queries = [(pick(), None if rng.integers(0, 3) == 0 else pick(),
                None if rng.integers(0, 2) == 0 else int(rng.integers(0, 5)))
               for _ in range(int(rng.integers(0, 7)))]
    return entries, snapshot, queries


@pytest.mark.gpu
def test_random_cases_on_one_set_of_dirty_buffers(lvkv, gpu):
    random_cases(lvkv, gpu, 2025, None)


@pytest.mark.gpu
def test_random_cases_over_the_wide_alphabet(lvkv, gpu):
    random_cases(lvkv, gpu, 2027, WIDE)


def random_cases(lvkv, gpu, seed, alphabet):
    rng = np.random.default_rng(seed)
    buf = _fresh(lvkv, gpu, 200)
    seen = set()
    for i in range(300):
        entries, snapshot, queries = random_case(rng, alphabet)
        max_out = None if i % 9 else int(rng.integers(0, 4))
        _, per_query, rep = Call(buf, entries, snapshot, queries, max_out=max_out,
                                 aligned=i % 4 == 0, gap=i % 3).check()
        seen |= {("status", rep["status"])} | {("q", s) for _, _, s in per_query}
    assert seen >= {("status", sm.OK), ("status", sm.CAPACITY), ("q", sm.Q_OK), ("q", sm.Q_CORRUPT)}


@pytest.mark.gpu
def test_three_calls_back_to_back_on_one_scratch(lvkv, gpu):
    """No synchronize between them: the stream orders the calls on the scratch.
    Each has outputs and a report of its own."""
    import torch
    rng = np.random.default_rng(7)
    cases = [(versions(TILE + 50), 600), (seam_case(GROUP), 850), (versions(700, every=2), 950)]
    bufs = [_fresh(lvkv, gpu, TILE + 50) for _ in cases]
    for b in bufs[1:]:
        b.scratch, b.need = bufs[0].scratch, bufs[0].need
    calls = [Call(b, e, s, some_queries([k for k, _ in e], rng, 9))
             for b, (e, s) in zip(bufs, cases)]
    for c in calls:
        c.check()


# ---- end to end ------------------------------------------------------------------------------------

def _resolved(stored, vtb, number):
    """(value, status) DecodeValue leaves of a stored value, by the model."""
    st, src, off, ln, _ = vm.resolve(stored, [0], [len(stored)], vtb, [0], [len(vtb)], [number])
    return ((vtb if src[0] else stored)[off[0]:off[0] + ln[0]] if st[0] == vm.R_OK else b"", st[0])


def _listed(res):
    """db_scan's lists on the host: per range [(user key, value, status)]."""
    q = res["query_off"].cpu().tolist()
    ko, vo = res["key_off"].cpu().tolist(), res["value_off"].cpu().tolist()
    keys, values = bytes(res["keys"].cpu().numpy()), bytes(res["values"].cpu().numpy())
    st = res["status"].cpu().tolist()
    items = [(keys[ko[e]:ko[e + 1]], values[vo[e]:vo[e + 1]], st[e]) for e in range(q[-1])]
    return [items[a:b] for a, b in zip(q, q[1:])]


@pytest.mark.gpu
@pytest.mark.parametrize("name", TABLES)
def test_db_scan_over_the_vtable_fixtures(lvkv, gpu, name):
    """Every original value in key order, through the table and the value log
    the reference wrote, forward and reversed."""
    import torch
    spec, entries, vtb = table(name)
    image = torch.tensor(np.fromfile(GOLDEN / spec["ldb"], dtype=np.uint8), device=gpu)
    vimage = torch.tensor(np.frombuffer(vtb, dtype=np.uint8).copy(), device=gpu) if vtb else \
        torch.zeros(0, dtype=torch.uint8, device=gpu)
    keys = [k for k, _ in entries]
    fwd, _ = sm.forward_walk(keys, sm.MAX_SEQUENCE)
    stored = vm.separate(entries, spec["kv_sep_size"], spec["file_number"])["out_vals"]
    want = [(keys[e][:-8],) + _resolved(stored[e], vtb, spec["file_number"]) for e in fwd]
    assert sum(st == vm.R_OK and v == entries[e][1][1:] for e, (_, v, st) in zip(fwd, want)) >= \
        len(fwd) - 3  # (an empty value and a kept value whose first byte is 1 do not decode)
    assert len(want) >= 2
    mid = want[len(want) // 2][0]
    starts, limits = [b"", mid, mid, b"\xff\xff"], [None, None, mid + b"\x00", None]
    for reverse in (False, True):
        res = lvkv.db_scan([image], {spec["file_number"]: vimage}, starts, limits,
                           snapshot=sm.MAX_SEQUENCE, max_ulen=32768, reverse=reverse,
                           filter_policy=lvkv.BLOOM_POLICY)
        assert res["merge"]["status"] == 0 and res["scan"]["status"] == sm.OK
        step = -1 if reverse else 1
        assert _listed(res) == [want[::step], want[len(want) // 2:][::step],
                                [want[len(want) // 2]], []]
        assert res["q_status"].cpu().tolist() == [sm.Q_OK] * 4
    # a reader before the last writes, with a maximum
    snapshot = sorted(sm.parse(k)[1] for k in keys)[len(keys) // 2]
    fwd, _ = sm.forward_walk(keys, snapshot)
    res = lvkv.db_scan([image], {spec["file_number"]: vimage}, [b""], [None], snapshot=snapshot,
                       max_count=3, max_ulen=32768, filter_policy=lvkv.BLOOM_POLICY)
    assert [k for k, _, _ in _listed(res)[0]] == [keys[e][:-8] for e in fwd[:3]]


@pytest.mark.gpu
def test_db_scan_over_a_recovered_table_and_a_memtable(lvkv, gpu):
    """A level-0 table and its vTable from one log, newer writes from another
    as the memtable's run: what Version::Get over both amounts to."""
    import torch
    name = "sorted"
    payload, offs, lens = log_of(name)
    log = torch.tensor(np.fromfile(GOLDEN / f"memtable_{name}.log", dtype=np.uint8), device=gpu)
    image, vimage, reports, seq = lvkv.wal_recover_table(
        log, file_number=FILE_NUMBER, kv_sep_size=16, compression=0, filter_bits_per_key=10)
    old = memm.from_batches(payload, offs, lens, max_sequence=0)
    assert image is not None and old["report"]["status"] == memm.OK
    old_entries = [(k, bytes(payload[o:o + n]))
                   for k, o, n in zip(old["ikeys"], old["val_off"], old["val_len"])]
    sep = vm.separate(old_entries, 16, FILE_NUMBER)
    assert bytes(vimage.cpu().numpy()) == bytes(sep["vtb"])
    old_entries = [(k, bytes(v)) for (k, _), v in zip(old_entries, sep["out_vals"])]  # as stored
    users = sorted({k[:-8] for k, _ in old_entries})
    # newer writes: puts and deletions over some of those keys, and keys of their own
    rng = np.random.default_rng(3)
    pick = [users[i % len(users)] if i % 3 else b"new%03d" % i for i in range(40)]
    new_payload, new_offs, new_lens = laid_out(
        batches_of(rng, [7, 1, 20, 12], lambda i: pick[i], seq0=seq + 1, vlen=lambda i: 3 + i % 30))
    new = memm.from_batches(new_payload, new_offs, new_lens, max_sequence=seq)
    new_entries = [(k, bytes(new_payload[o:o + n]))
                   for k, o, n in zip(new["ikeys"], new["val_off"], new["val_len"])]
    assert any(k[-8] == 0 for k, _ in new_entries)
    p = torch.tensor(np.frombuffer(new_payload, dtype=np.uint8).copy(), device=gpu)
    m = lvkv.memtable_from_batches(p, torch.tensor(new_offs, dtype=torch.int64, device=gpu),
                                   torch.tensor(new_lens, dtype=torch.int64, device=gpu),
                                   max_sequence=seq)
    assert m[0]["status"] == lvkv.MEMTABLE_OK and m[0]["nentries"] == len(new_entries)

    merged = sorted(new_entries + old_entries,
                    key=lambda e: (e[0][:-8], -int.from_bytes(e[0][-8:], "little")))
    keys = [k for k, _ in merged]
    top = m[0]["max_sequence_out"]
    starts = [b"", users[len(users) // 2], b"new", users[3], users[3]]
    limits = [None, None, b"nex", users[3] + b"\x00", users[2]]
    for snapshot, reverse in ((top, False), (top, True), (seq, False), ((seq + top) // 2, False)):
        res = lvkv.db_scan([image], {FILE_NUMBER: vimage}, starts, limits, snapshot=snapshot,
                           memtable=m[1:7], max_count=[None, 5, None, 1, None], reverse=reverse,
                           max_ulen=lvkv.SNAPPY_MAX_BLOCK, filter_policy=lvkv.BLOOM_POLICY)
        assert res["merge"]["status"] == 0 and res["scan"]["status"] == sm.OK
        assert res["merge"]["num_out"] == len(merged)
        want = []
        for start, limit, mx in zip(starts, limits, [None, 5, None, 1, None]):
            counted, _, ok = sm.query(keys, snapshot, start, limit, mx)
            assert ok
            want.append([(keys[e][:-8],) + _resolved(merged[e][1], bytes(sep["vtb"]), FILE_NUMBER)
                         for e in counted][::-1 if reverse else 1])
        assert _listed(res) == want
        assert len(want[0]) > len(want[1]) == 5 and want[4] == []
