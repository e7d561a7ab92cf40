"""lvkv_sst_read_entries_device: Block::Iter's forward walk on the device, and
sst_read_entries / sst_read_table on top of it.

The expectation is tests/sst_entries_model.py, pinned against the reference
in test_sst_entries_model.py. The GPU tests call the C entry point on buffers
filled with a byte and bordered, and compare the *whole* output buffers with
the model's result laid over that fill: the keys, the four entry arrays,
block_first, the statuses, the report, and every byte and slot the call must
leave alone (the gaps between keys, what follows the counts, the borders).

The call's device-wide scans run over the blocks (the entries of a block are
placed inside it by the wave that counts them), so the sizes at which it
changes path are block counts: 64 runs a round of the count kernel, and the
scan's tile, read from the code as the build test reads kBuildTile.
"""
from __future__ import annotations

import ctypes
import functools
import json
import re

import numpy as np
import pytest

import sst_build_model as bm
import sst_entries_model as em
import sst_finish_model as fm
import test_sst_build_blocks as tb
from conftest import GOLDEN, REPO
from test_sst_entries_model import walk_cases

FILL = 0xC3
BORDER = 4096
SLOT_FILL64 = -0x3C3C3C3C3C3C3C3D
SLOT_FILL32 = -0x3C3C3C3D
REPORT_KEYS = ["status", "nbad", "first_bad_block", "max_key_len", "num_entries", "key_bytes",
               "value_bytes"]
# blocks a workgroup of the device-wide scan, from the code
TILE = int(re.search(r"constexpr uint32_t kScanTile = (\d+);",
                     (REPO / "leveldb-kv-separation_amd" / "csrc" / "lvkv_launch.h").read_text())
           .group(1))


# ---- inputs ---------------------------------------------------------------------

def _blocks_of(entries, block_size, restart):
    return [fm.block_of(c, restart) for c in bm.cut(list(entries), block_size, restart)]


@functools.lru_cache(maxsize=None)
def _tiny_blocks(n):
    """n blocks of one to three entries, intervals 1 and 16 in turn."""
    out = []
    for b in range(n):
        ents = [((b * 4 + j).to_bytes(8, "big"), b"xyz"[:(b + j) % 4]) for j in range(1 + b % 3)]
        out.append(fm.block_of(ents, 1 if b % 2 else 16))
    return tuple(out)


def _damage(rng, block):
    """One of the fixture's damage kinds on a block BlockBuilder wrote."""
    b = bytearray(block)
    nr = int.from_bytes(b[-4:], "little")
    limit = len(b) - 4 - 4 * nr
    kind = int(rng.integers(0, 10))
    if kind == 0:    # restart[0] anywhere up to a little past the entries
        b[limit:limit + 4] = int(rng.integers(0, limit + 8)).to_bytes(4, "little")
    elif kind == 1 and nr > 1:  # another restart anywhere
        at = limit + 4 * int(rng.integers(1, nr))
        b[at:at + 4] = int(rng.integers(0, 1 << 32)).to_bytes(4, "little")
    elif kind == 2:  # a count that does not fit
        b[-4:] = ((len(b) - 4) // 4 + 1).to_bytes(4, "little")
    elif kind == 3:  # no restarts
        b[-4:] = bytes(4)
    elif kind == 4:  # too short for a count
        b = b[:int(rng.integers(0, 4))]
    elif kind == 5:  # stray bytes before the restart array
        b[limit:limit] = bytes(rng.integers(0, 256, size=int(rng.integers(1, 4)), dtype=np.uint8))
    elif kind == 6:  # a five-byte varint with a high bit, cut or not
        b[limit:limit] = b"\x80" * int(rng.integers(3, 7)) + b"\x01\x00\x00"
    else:            # a byte of the entries changed: shared, a length, a key byte
        at = int(rng.integers(0, max(1, limit)))
        b[at] = int(rng.integers(0, 256))
    return bytes(b)


@functools.lru_cache(maxsize=None)
def _random_batch(seed):
    """The blocks of tb._random_case(seed), a seeded tenth of them damaged."""
    entries, block_size, restart, _ = tb._random_case(seed)
    blocks = _blocks_of(entries, block_size, restart)
    rng = np.random.default_rng(10_000 + seed)
    hit = rng.integers(0, 10, size=len(blocks)) == 0
    return tuple(_damage(rng, b) if h else b for b, h in zip(blocks, hit))


# ---- the C ABI without a device ---------------------------------------------------

def _abi_args(lvkv, **over):
    p = ctypes.c_void_p(0x1000)
    need = lvkv.lib.lvkv_sst_read_entries_scratch_bytes(100, 0)
    a = dict(raw=p, raw_off=p, raw_len=p, skip=p, n=100, scratch=p, scratch_bytes=need, keys=p,
             key_capacity=1 << 20, key_off=p, key_len=p, val_off=p, val_len=p, max_entries=1000,
             block_first=p, block_status=p, report=p, stream=None)
    a.update(over)
    return list(a.values())


def test_host_validation_needs_no_device(lvkv):
    L = lvkv.lib
    bad = lvkv.LVKV_ERR_INVALID
    names = ("raw", "raw_off", "raw_len", "scratch", "keys", "key_off", "key_len", "val_off",
             "val_len", "block_first", "block_status", "report")
    for name in names:
        assert L.lvkv_sst_read_entries_device(*_abi_args(lvkv, **{name: None})) == bad, name
    for n in (1 << 31, (1 << 31) + 5):
        big = L.lvkv_sst_read_entries_scratch_bytes(n, 0)
        assert L.lvkv_sst_read_entries_device(*_abi_args(lvkv, n=n, scratch_bytes=big)) == bad
    short = _abi_args(lvkv)[6] - 1
    assert L.lvkv_sst_read_entries_device(*_abi_args(lvkv, scratch_bytes=short)) == bad
    nulls = {k: None for k in names + ("skip",)}
    assert L.lvkv_sst_read_entries_device(*_abi_args(lvkv, n=0, scratch_bytes=0, **nulls)) == \
        lvkv.LVKV_OK


def test_report_mirror_matches_the_header(lvkv):
    assert ctypes.sizeof(lvkv.SstEntriesReport) == 40
    assert [lvkv.SstEntriesReport.num_entries.offset, lvkv.SstEntriesReport.key_bytes.offset,
            lvkv.SstEntriesReport.value_bytes.offset] == [16, 24, 32]
    assert [k for k, _ in lvkv.SstEntriesReport._fields_] == REPORT_KEYS
    assert [lvkv.ENTRIES_OK, lvkv.ENTRIES_BAD_BLOCK, lvkv.ENTRIES_BAD_ENTRY,
            lvkv.ENTRIES_SKIPPED] == [em.OK, em.BAD_BLOCK, em.BAD_ENTRY, em.SKIPPED]
    assert lvkv.ENTRIES_CAPACITY == em.CAPACITY
    header = (REPO / "include" / "lvkv_snappy.h").read_text()
    for name, value in (("OK", 0), ("BAD_BLOCK", 1), ("BAD_ENTRY", 2), ("SKIPPED", 3),
                        ("CAPACITY", 1)):
        assert re.search(rf"#define LVKV_ENTRIES_{name} {value}\b", header), name


def test_sizing_function_is_monotone(lvkv):
    f = lvkv.lib.lvkv_sst_read_entries_scratch_bytes
    ns = [0, 1, 2, 63, 64, 65, TILE - 1, TILE, TILE + 1, 1 << 20, (1 << 31) - 1]
    totals = [0, 1, 6, 7, 8, 4096, 4097, 1 << 20, 1 << 33]
    for t in totals:
        s = [f(n, t) for n in ns]
        assert s == sorted(s), (t, s)
    for n in ns:
        s = [f(n, t) for t in totals]
        assert s == sorted(s), (n, s)


# ---- on the device -----------------------------------------------------------------

class Buffers:
    """The output side of a call, kept over calls, between borders, and on
    the host what it must hold: the fill, with everything an earlier call
    wrote laid over it."""

    def __init__(self, torch, dev, lvkv, key_cap, max_entries, max_blocks, total_raw):
        self.torch, self.dev, self.lvkv = torch, dev, lvkv
        self.key_cap, self.max_entries, self.max_blocks = key_cap, max_entries, max_blocks
        self.need = lvkv.lib.lvkv_sst_read_entries_scratch_bytes(max_blocks, total_raw)
        full = lambda n, v, t: torch.full((n,), v, dtype=t, device=dev)
        ne, nb = max_entries + 64, max_blocks + 64
        self.dev_bufs = {
            "keys": full(key_cap + BORDER, FILL, torch.uint8),
            "key_off": full(ne, SLOT_FILL64, torch.int64),
            "key_len": full(ne, SLOT_FILL32, torch.int32),
            "val_off": full(ne, SLOT_FILL64, torch.int64),
            "val_len": full(ne, SLOT_FILL32, torch.int32),
            "block_first": full(nb + 1, SLOT_FILL64, torch.int64),
            "block_status": full(nb, FILL, torch.uint8),
        }
        self.scratch = full(self.need + BORDER, FILL, torch.uint8)
        self.rep = full(ctypes.sizeof(lvkv.SstEntriesReport), FILL, torch.uint8)
        self.want = {k: v.cpu().numpy().copy() for k, v in self.dev_bufs.items()}


def _pack_blocks(blocks, gap):
    """The blocks `gap` bytes apart (every alignment) behind a border."""
    offs, p = [], 64 + gap
    for b in blocks:
        offs.append(p)
        p += len(b) + gap
    host = np.full(p + 64, 0x5A, dtype=np.uint8)
    for o, b in zip(offs, blocks):
        host[o:o + len(b)] = np.frombuffer(b, dtype=np.uint8)
    return host, offs


def _call(buf, blocks, *, skip=None, max_entries=None, key_capacity=None, gap=1,
          scratch_bytes=None):
    """One call of the C entry point into buf, checked in full against the
    model. Returns the model's result (the report checked equal)."""
    torch, dev, lvkv = buf.torch, buf.dev, buf.lvkv
    max_entries = buf.max_entries if max_entries is None else max_entries
    key_capacity = buf.key_cap if key_capacity is None else key_capacity
    n = len(blocks)
    assert n <= buf.max_blocks and max_entries <= buf.max_entries and key_capacity <= buf.key_cap
    host, offs = _pack_blocks(blocks, gap)
    raw = torch.from_numpy(host).to(dev)
    off_t = torch.tensor(offs, dtype=torch.int64, device=dev)
    len_t = torch.tensor([len(b) for b in blocks], dtype=torch.int32, device=dev)
    skip_t = None if skip is None else torch.tensor(skip, dtype=torch.uint8, device=dev)
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
    scratch_bytes = buf.need if scratch_bytes is None else scratch_bytes
    assert lvkv.lib.lvkv_sst_read_entries_scratch_bytes(n, 0) <= scratch_bytes <= buf.need
    d = buf.dev_bufs
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    rc = lvkv.lib.lvkv_sst_read_entries_device(
        p(raw), p(off_t), p(len_t), p(skip_t), n, p(buf.scratch), scratch_bytes, p(d["keys"]),
        key_capacity, p(d["key_off"]), p(d["key_len"]), p(d["val_off"]), p(d["val_len"]),
        max_entries, p(d["block_first"]), p(d["block_status"]), p(buf.rep), stream)
    assert rc == 0
    torch.cuda.synchronize()
    rep = lvkv.SstEntriesReport.from_buffer_copy(bytes(buf.rep.cpu().numpy())).as_dict()
    m = em.read(blocks, offs, skip, max_entries, key_capacity)
    print("report", rep)
    assert rep == m["report"]
    w = buf.want
    w["block_first"][:n + 1] = m["block_first"]
    w["block_status"][:n] = m["block_status"]
    if m["report"]["status"] == em.OK:
        ne = len(m["keys"])
        for name in ("key_off", "key_len", "val_off", "val_len"):
            w[name][:ne] = m[name]
        for o, k in zip(m["key_off"], m["keys"]):
            w["keys"][o:o + len(k)] = np.frombuffer(k, dtype=np.uint8)
    got = {k: v.cpu().numpy() for k, v in d.items()}
    assert got["block_status"][:n].tolist() == m["block_status"]
    assert got["block_first"][:n + 1].tolist() == m["block_first"]
    for name in ("block_first", "block_status", "key_off", "key_len", "val_off", "val_len"):
        wrong = np.nonzero(got[name] != w[name])[0]
        assert wrong.size == 0, f"{name}[{wrong[0]}] is {got[name][wrong[0]]}, not " \
                                f"{w[name][wrong[0]]}"
    wrong = np.nonzero(got["keys"] != w["keys"])[0]
    assert wrong.size == 0, f"key byte {wrong[0]} of {m['report']['key_bytes']} is wrong"
    assert (buf.scratch[buf.need:].cpu().numpy() == FILL).all(), "a write past the scratch"
    return m


def _fresh(lvkv, gpu, blocks, spare=0):
    import torch
    m = em.read(blocks, [0] * len(blocks))["report"]
    total = sum(len(b) for b in blocks)
    return Buffers(torch, gpu, lvkv, m["key_bytes"] + 8 + spare, m["num_entries"] + spare,
                   len(blocks), total)


@pytest.mark.gpu
@pytest.mark.parametrize("case", walk_cases(), ids=[c[0] for c in walk_cases()])
def test_fixture_blocks_alone(lvkv, gpu, case):
    name, block, entries, status = case
    buf = _fresh(lvkv, gpu, [block], spare=4)
    m = _call(buf, [block])
    # the reference's own verdict and entries, not only the model's
    assert em.STATUS_TEXT[m["block_status"][0]] == status
    assert m["keys"] == [k for k, _, _ in entries]
    assert [v - 65 for v in m["val_off"]] == [o for _, o, _ in entries]


@pytest.mark.gpu
def test_fixture_blocks_in_one_batch(lvkv, gpu):
    blocks = [c[1] for c in walk_cases()]
    buf = _fresh(lvkv, gpu, blocks)
    m = _call(buf, blocks)
    assert [em.STATUS_TEXT[s] for s in m["block_status"]] == [c[3] for c in walk_cases()]
    assert m["report"]["nbad"] == sum(c[3] != "OK" for c in walk_cases())
    _call(buf, blocks[::-1], gap=0)


@pytest.mark.gpu
@pytest.mark.parametrize("name", tb.FIXTURES)
def test_golden_table_blocks(lvkv, gpu, name):
    raws, entries = tb._fixture(name)[2:]
    buf = _fresh(lvkv, gpu, raws)
    m = _call(buf, list(raws))
    assert m["report"]["nbad"] == 0
    assert m["keys"] == [k for k, _ in entries]


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 63, 64, 65, 1025])
def test_block_counts(lvkv, gpu, n):
    blocks = list(_tiny_blocks(n))
    _call(_fresh(lvkv, gpu, blocks), blocks)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [TILE - 1, TILE, TILE + 1, 2 * TILE + 3],
                         ids=["T-1", "T", "T+1", "2T+3"])
def test_block_counts_around_the_scan_tile(lvkv, gpu, n):
    """The scans that place entries and key bytes pass one tile and carry
    into the next; a bad block sits on either side of the boundary."""
    blocks = list(_tiny_blocks(n))
    for b in (TILE - 2, TILE - 1, TILE, n - 1):
        if b < n:
            blocks[b] = blocks[b][:-4] + (1 << 20).to_bytes(4, "little")
    m = _call(_fresh(lvkv, gpu, blocks), blocks)
    assert m["report"]["nbad"] >= 1 and m["report"]["num_entries"] > n


@pytest.mark.gpu
@pytest.mark.parametrize("n", [TILE - 1, TILE, TILE + 1, 3 * TILE + 5],
                         ids=["T-1", "T", "T+1", "3T+5"])
def test_entry_counts_around_the_scan_tile(lvkv, gpu, n):
    """One-entry blocks: the entry count is the block count, so the scan of
    the entries' places passes one tile and one carry at exactly n entries."""
    blocks = [fm.block_of([((7 * b).to_bytes(5, "big"), b"v" * (b % 3))], 16) for b in range(n)]
    m = _call(_fresh(lvkv, gpu, blocks), blocks, gap=0)
    assert m["report"]["num_entries"] == n and m["block_first"][-1] == n


@pytest.mark.gpu
def test_run_shapes(lvkv, gpu):
    """More runs than a wave has lanes (two rounds of the count kernel, the
    second partly filled), and runs far longer than any interval suggests."""
    seventy = [(b"run%04d" % i, b"v" * (i % 5)) for i in range(70)]
    many = fm.block_of(seventy, 1)
    assert int.from_bytes(many[-4:], "little") == 70
    exactly = fm.block_of(seventy[:64], 1)
    more = fm.block_of(seventy + [(b"s%05d" % i, b"") for i in range(70)], 1)
    long_run = fm.block_of([(b"long/%06d" % i, b"%d" % i) for i in range(1000)], 1000)
    assert int.from_bytes(long_run[-4:], "little") == 1
    two_long = fm.block_of([(b"long/%06d" % i, b"%d" % i) for i in range(1500)], 1000)
    blocks = [many, long_run, exactly, two_long, more]
    m = _call(_fresh(lvkv, gpu, blocks), blocks)
    assert m["block_first"] == [0, 70, 1070, 1134, 2634, 2774]
    rbig = tb._fixture("cuts_rbig")
    assert rbig[1]["restart_interval"] == 1000
    _call(_fresh(lvkv, gpu, rbig[2]), list(rbig[2]))


@pytest.mark.gpu
@pytest.mark.parametrize("key_format", [0, 1])
@pytest.mark.parametrize("key_len", [300, 2000])
def test_long_keys(lvkv, gpu, key_len, key_format):
    """300 bytes lie inside the write kernel's window of the running key,
    2,000 past it (their shared bytes are traced back to their deltas); a
    40-byte key stands between long ones. Clean blocks, and the same entries
    in a block one lane walks (a restart array that lies)."""
    window = int(re.search(r"kEntriesKeyWindow = (\d+);", (
        REPO / "leveldb-kv-separation_amd" / "csrc" / "lvkv_launch.h").read_text()).group(1))
    assert 300 < window < 2000
    entries = tb._long_key_entries(key_len, key_format)
    assert max(len(k) for k, _ in entries) == key_len
    blocks = _blocks_of(entries, 1 << 16, 4) + _blocks_of(entries, 4096, 16)
    lying = bytearray(blocks[0])
    limit = len(lying) - 4 - 4 * int.from_bytes(lying[-4:], "little")
    lying[limit + 4:limit + 8] = (7).to_bytes(4, "little")
    blocks.append(bytes(lying))
    m = _call(_fresh(lvkv, gpu, blocks), blocks)
    assert m["report"]["max_key_len"] == key_len and m["report"]["nbad"] == 0
    assert m["keys"][-len(entries):] == [k for k, _ in entries]


@pytest.mark.gpu
def test_skip(lvkv, gpu):
    blocks = list(tb._fixture("cuts_r3")[2])
    n = len(blocks)
    assert n > 4
    buf = _fresh(lvkv, gpu, blocks)
    whole = _call(buf, blocks)  # null
    assert _call(buf, blocks, skip=[0] * n)["report"] == whole["report"]
    some = [0] * n
    some[0] = some[n - 1] = 1
    some[2] = 0xFF
    m = _call(buf, blocks, skip=some)
    assert m["block_status"][0] == m["block_status"][2] == m["block_status"][-1] == em.SKIPPED
    assert m["report"]["nbad"] == 0 and m["block_first"][1] == 0
    # a skipped block is not read: its length may say anything
    blocks[2] = b""
    _call(buf, blocks, skip=some)
    assert _call(buf, blocks, skip=[1] * n)["report"]["num_entries"] == 0


@pytest.mark.gpu
def test_mixed_batch(lvkv, gpu):
    """Clean blocks, blocks one lane walks, and bad ones side by side: what
    follows a partly emitted block lands right after its last good entry."""
    by = {c[0]: c[1] for c in walk_cases()}
    clean = list(tb._fixture("cuts_r2")[2])
    blocks = [clean[0], by["shared_too_long"], clean[1], by["restart_entry_shares"], by["len3"],
              by["stray_two"], clean[2], by["restart0_second_entry"], by["count0"],
              by["value_past_limit"], by["count_too_many"], clean[3], by["restart0_mid_entry"]]
    buf = _fresh(lvkv, gpu, blocks)
    m = _call(buf, blocks)
    assert m["block_status"].count(em.BAD_ENTRY) == 4 and m["block_status"].count(em.BAD_BLOCK) == 2
    assert m["report"]["first_bad_block"] == 1
    assert m["block_first"][2] - m["block_first"][1] == 4  # partly emitted
    # a scratch with room for few runs or none (the alignment slack it did not
    # need): the blocks past them by one lane, the same result
    floor = lvkv.lib.lvkv_sst_read_entries_scratch_bytes(len(blocks), 0)
    assert _call(buf, blocks, scratch_bytes=floor)["report"] == m["report"]
    assert _call(buf, blocks, scratch_bytes=floor + 16 * 9)["report"] == m["report"]


@pytest.mark.gpu
def test_random_batches_on_dirty_buffers(lvkv, gpu):
    """Separate calls into one set of buffers nobody cleans in between."""
    import torch
    batches = [_random_batch(s) for s in tb.RANDOM_SEEDS]
    reports = [em.read(b, [0] * len(b))["report"] for b in batches]
    assert sum(r["nbad"] for r in reports) > 100
    buf = Buffers(torch, gpu, lvkv, max(r["key_bytes"] for r in reports) + 8,
                  max(r["num_entries"] for r in reports), max(map(len, batches)),
                  max(sum(map(len, b)) for b in batches))
    for seed, blocks in zip(tb.RANDOM_SEEDS, batches):
        try:
            _call(buf, list(blocks), gap=seed % 3)
        except AssertionError as e:
            raise AssertionError(f"seed {seed} ({len(blocks)} blocks): {e}") from e
    _call(buf, list(batches[0]))


@pytest.mark.gpu
def test_capacity(lvkv, gpu):
    blocks = list(tb._fixture("table")[2])
    need = em.read(blocks, [0] * len(blocks))["report"]
    assert need["num_entries"] == 1400
    buf = _fresh(lvkv, gpu, blocks)
    for over in (dict(max_entries=1399), dict(key_capacity=need["key_bytes"] - 1),
                 dict(max_entries=1399, key_capacity=need["key_bytes"] - 1),
                 dict(max_entries=0, key_capacity=0)):
        m = _call(buf, blocks, **over)  # (compares every buffer: nothing but the per-block arrays)
        assert m["report"]["status"] == em.CAPACITY
        assert (m["report"]["num_entries"], m["report"]["key_bytes"]) == \
            (1400, need["key_bytes"])
    rep = m["report"]
    m = _call(buf, blocks, max_entries=rep["num_entries"], key_capacity=rep["key_bytes"])
    assert m["report"]["status"] == em.OK


# ---- the wrappers --------------------------------------------------------------------

def _table_options(name):
    bits = 10 if name == "table" else 0
    return tb._fixture(name)[1], bits


@pytest.mark.gpu
def test_read_entries_wrapper(lvkv, gpu):
    import torch
    raws, entries = tb._fixture("cuts_internal")[2:]
    host, offs = _pack_blocks(raws, 3)
    raw = torch.from_numpy(host).to(gpu)
    off = torch.tensor(offs, dtype=torch.int64, device=gpu)
    ln = torch.tensor([len(r) for r in raws], dtype=torch.int32, device=gpu)
    keys, koff, klen, vals, voff, vlen, first, status, rep = lvkv.sst_read_entries(raw, off, ln)
    m = em.read(raws, offs)
    assert rep == m["report"] and koff.tolist() == m["key_off"] and klen.tolist() == m["key_len"]
    assert voff.tolist() == m["val_off"] and vlen.tolist() == m["val_len"]
    assert first.tolist() == m["block_first"] and status.tolist() == m["block_status"]
    kh = keys.cpu().numpy()
    assert [bytes(kh[o:o + n]) for o, n in zip(m["key_off"], m["key_len"])] == \
        [k for k, _ in entries]
    assert vals is raw
    # too few key bytes at first: asked again with what the report says
    small = lvkv.sst_read_entries(raw, off, ln, key_capacity=64)
    assert small[8]["status"] == lvkv.ENTRIES_CAPACITY and small[1].numel() == 0
    assert small[8]["key_bytes"] == rep["key_bytes"]
    none = lvkv.sst_read_entries(raw, off[:0], ln[:0])
    assert none[8] == em.read([], [])["report"] and none[6].tolist() == [0]


@pytest.mark.gpu
@pytest.mark.parametrize("name", tb.FIXTURES)
def test_round_trip_of_a_reference_table(lvkv, gpu, name):
    """image -> handles -> blocks -> entries -> blocks -> image: the
    reference's own file comes back byte for byte, with the values read from
    where the decoded blocks left them."""
    import torch
    img, opts, raws, entries = tb._fixture(name)
    opts, bits = _table_options(name)
    file = torch.from_numpy(np.frombuffer(img, dtype=np.uint8).copy()).to(gpu)
    out = lvkv.sst_read_table(file, filter_policy=lvkv.BLOOM_POLICY if bits else None,
                              max_ulen=max(map(len, raws)))
    table, rstatus, rep = out[6:]
    assert table["status"] == 0 and table["ndata"] == len(raws)
    assert not rstatus.cpu().numpy().any()
    assert rep["status"] == 0 and rep["nbad"] == 0 and rep["num_entries"] == len(entries)
    built = lvkv.sst_build_table(*out[:6], compression=0, filter_bits_per_key=bits, **opts)
    assert built[6]["status"] == lvkv.BUILD_OK and built[5]["status"] == lvkv.TABLE_OK
    assert built[5]["file_size"] == len(img)
    assert bytes(built[0][:len(img)].cpu().numpy()) == img


@pytest.mark.gpu
def test_round_trip_through_snappy(lvkv, gpu):
    """sst_read_blocks' decoded output feeds the walk: a Snappy-compressed
    image, read back into entries and built again, is the same image."""
    import torch
    entries = tb._round_trip_entries()
    opts = dict(block_size=2048, restart_interval=16, key_format=1, compression=1)
    first = lvkv.sst_build_table(*tb._device_entries(torch, gpu, entries), **opts)
    assert first[5]["status"] == lvkv.TABLE_OK and set(first[3].tolist()) == {1}
    img = first[0][:first[5]["file_size"]].clone()
    out = lvkv.sst_read_table(img, filter_policy=lvkv.BLOOM_POLICY,
                              max_ulen=first[6]["max_block_len"])
    assert out[8]["num_entries"] == len(entries) and out[8]["nbad"] == 0
    kh, koff, klen = out[0].cpu().numpy(), out[1].tolist(), out[2].tolist()
    assert [bytes(kh[o:o + n]) for o, n in zip(koff, klen)] == [k for k, _ in entries]
    again = lvkv.sst_build_table(*out[:6], **opts)
    assert again[5]["status"] == lvkv.TABLE_OK
    assert bytes(again[0][:again[5]["file_size"]].cpu().numpy()) == bytes(img.cpu().numpy())
