"""lvkv_memtable_from_batches_device against tests/memtable_model.py, which
tests/test_memtable_model.py holds to the reference's own recovery: every
output array, d_keys and the report. The calls write into filled buffers with
a border on either side of every output; what a call must not touch has to
still hold the fill. The payload ends where its buffer ends. The fixtures go
end to end: wal_recover_table gives the reference's .ldb and .vtb byte for
byte, and sst_get_values on them the newest version of every user key.

T is the sort's tile and W the parse window: the sizes at which the call
changes path.
"""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

import memtable_model as mm
import vtable_model as vm
from conftest import GOLDEN
from test_memtable_model import FILE_NUMBER, NAMES, cases, log_of
from test_vtable import BORDER, FILL, PAD, Out, Packed, _stream, report, vp

T = 1024
W = 8192


def test_constants_are_the_library_s(lvkv):
    assert (lvkv.MEMTABLE_SORT_TILE, lvkv.MEMTABLE_WINDOW) == (T, W)
    assert ctypes.sizeof(lvkv.MemtableReport) == 64
    assert [getattr(lvkv, "MEMTABLE_" + n) for n in
            ("OK", "TOO_SMALL", "UNKNOWN_TAG", "BAD_PUT", "BAD_DELETE", "WRONG_COUNT",
             "KEY_TOO_LONG", "CAPACITY", "DUPLICATE")] == list(range(9))


def test_scratch_size_never_decreases(lvkv):
    f = lvkv.lib.lvkv_memtable_scratch_bytes
    sizes = [0, 1, 2, 255, 256, 257, 4095, 4096, 4097, 100000, (1 << 31) - 1]
    for a in sizes:
        for b in sizes:
            assert f(a, b) <= f(a + 1, b) and f(a, b) <= f(a, b + 1)
    assert f(0, 0) >= 256


class Mem:
    """One call's buffers; call() launches (any number of times on the same
    buffers), check() compares with the model."""

    def __init__(self, lvkv, dev, payload, offs, lens, *, max_sequence=0, paranoid=False,
                 max_entries=None, key_capacity=None, batch_arrays=True, lead=0, shift=0,
                 virtual_len=None, scratch=None):
        import torch
        self.lvkv, self.dev = lvkv, dev
        self.args = dict(max_sequence=max_sequence, paranoid=paranoid, virtual_len=virtual_len)
        self.payload, self.offs, self.lens = payload, list(offs), list(lens)
        self.free = mm.from_batches(payload, offs, lens, **self.args)  # no capacity in the way
        rep = self.free["report"]
        self.me = rep["nentries"] if max_entries is None else max_entries
        self.kc = rep["key_bytes"] if key_capacity is None else key_capacity
        self.want = mm.from_batches(payload, offs, lens, max_entries=self.me, key_capacity=self.kc,
                                    **self.args)
        nb = self.nb = len(offs)
        # the payload's last byte is its buffer's last
        self.buf = torch.tensor(np.frombuffer(bytes(lead) + bytes(payload), dtype=np.uint8).copy(),
                                device=dev) if len(payload) + lead else \
            torch.zeros(1, dtype=torch.uint8, device=dev)
        self.lead = lead
        claimed = [v if v is not None else l for v, l in
                   zip(virtual_len or [None] * nb, self.lens)]
        self.boff = torch.tensor(self.offs or [0], dtype=torch.int64, device=dev)
        self.blen = torch.tensor(claimed or [0], dtype=torch.int64, device=dev)
        self.keys = Out(torch, dev, self.kc, torch.uint8, BORDER, shift)
        self.koff = Out(torch, dev, self.me, torch.int64, PAD)
        self.klen = Out(torch, dev, self.me, torch.int32, PAD)
        self.voff = Out(torch, dev, self.me, torch.int64, PAD)
        self.vlen = Out(torch, dev, self.me, torch.int32, PAD)
        self.src = Out(torch, dev, self.me, torch.int32, PAD)
        self.bst = Out(torch, dev, nb, torch.uint8, PAD) if batch_arrays else None
        self.bent = Out(torch, dev, nb, torch.int32, PAD) if batch_arrays else None
        self.need = int(lvkv.lib.lvkv_memtable_scratch_bytes(nb, self.me))
        self.scratch = scratch if scratch is not None else \
            torch.full((self.need + BORDER,), FILL, dtype=torch.uint8, device=dev)
        assert self.scratch.numel() >= self.need
        self.rep = torch.full((ctypes.sizeof(lvkv.MemtableReport) + 64,), FILL, dtype=torch.uint8,
                              device=dev)

    def call(self, rc=0):
        got = self.lvkv.lib.lvkv_memtable_from_batches_device(
            vp(self.buf, self.lead), vp(self.boff), vp(self.blen), self.nb,
            self.args["max_sequence"], 1 if self.args["paranoid"] else 0, vp(self.scratch),
            self.need, self.keys.ptr(), self.kc, self.koff.ptr(), self.klen.ptr(), self.voff.ptr(),
            self.vlen.ptr(), self.src.ptr(), self.me,
            self.bst.ptr() if self.bst else None, self.bent.ptr() if self.bent else None,
            vp(self.rep), _stream(self.dev))
        assert got == rc
        return self

    def check(self, own_scratch=True):
        lvkv, want = self.lvkv, self.want
        rep = report(self.rep, lvkv.MemtableReport)
        assert rep == want["report"]
        if own_scratch:
            assert (self.scratch[self.need:].cpu().numpy() == FILL).all(), "a write past the scratch"
        keys, c0 = self.keys.read()
        arrays = [a.read() for a in (self.koff, self.klen, self.voff, self.vlen, self.src)]
        assert c0 and all(c for _, c in arrays), "a write into a border"
        if self.bst:
            bst, c1 = self.bst.read()
            bent, c2 = self.bent.read()
            assert c1 and c2
            assert bst.tolist() == want["batch_status"]
            assert bent.tolist() == want["batch_entries"]
        if rep["status"] != mm.OK:
            assert (keys == FILL).all()
            assert all((a.view(np.uint8) == FILL).all() for a, _ in arrays)
            return rep
        n, kb = rep["nentries"], rep["key_bytes"]
        assert bytes(keys[:kb]) == want["keys"] and (keys[kb:] == FILL).all()
        names = ("key_off", "key_len", "val_off", "val_len", "src")
        for (a, _), name in zip(arrays, names):
            assert (a[:n] == np.array(want[name], dtype=np.int64).astype(a.dtype)).all(), name
            assert (a[n:].view(np.uint8) == FILL).all(), name
        return rep


# ---- workloads ------------------------------------------------------------------------------

def value(rng, n):
    return b"" if n == 0 else b"\x02" + rng.integers(0, 256, n - 1, dtype=np.uint8).tobytes()


def batches_of(rng, counts, key, seq0=1, vlen=lambda i: 5, deletes=True):
    """len(counts) batches of counts[b] entries: entry i has user key key(i);
    the sequences ascend, so no two internal keys are equal."""
    out, i, seq = [], 0, seq0
    for c in counts:
        body = b""
        for _ in range(c):
            body += mm.delete(key(i)) if deletes and i % 5 == 3 else \
                mm.put(key(i), value(rng, vlen(i)))
            i += 1
        out.append(mm.batch(seq, c, body))
        seq += c
    return out


def laid_out(batches, gap=lambda b: 0):
    offs, at, parts = [], 0, []
    for b, x in enumerate(batches):
        offs.append(at)
        g = gap(b) if b + 1 < len(batches) else 0
        parts.append(x + bytes(g))
        at += len(x) + g
    return b"".join(parts), offs, [len(x) for x in batches]


def split(rng, n, nb):
    cuts = sorted(rng.integers(0, n + 1, nb - 1).tolist())
    return [b - a for a, b in zip([0] + cuts, cuts + [n])]


# a second alphabet: the bytes a signed compare, a zero-padded prefix and the tile's padding
# (prefix ~0) get wrong
WIDE = np.array([0x00, 0x61, 0x7f, 0x80, 0xff], dtype=np.uint8)


def random_key(rng, alphabet=None):
    n = int(rng.choice([0, 1, 3, 7, 8, 9, 12, 16, 24, 40]))
    if alphabet is None:
        return rng.integers(97, 100, n, dtype=np.uint8).tobytes()
    return alphabet[rng.integers(0, len(alphabet), n)].tobytes()


# ---- sizes ----------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 255, 256, 257, T - 1, T, T + 1, 2 * T + 1, 4 * T + 3])
@pytest.mark.parametrize("nb", [1, 2, 257])
def test_entry_and_batch_counts(lvkv, gpu, n, nb):
    rng = np.random.default_rng(1000 * nb + n)
    keys = [random_key(rng) for _ in range(n)]
    b = batches_of(rng, split(rng, n, nb), lambda i: keys[i], vlen=lambda i: i % 23)
    m = Mem(lvkv, gpu, *laid_out(b, gap=lambda b: b % 3), max_sequence=n // 2, shift=n % 16)
    rep = m.call().check()
    assert rep["nentries"] == n and rep["status"] == mm.OK


@pytest.mark.gpu
@pytest.mark.parametrize("nb", [4095, 4096, 4097])
def test_batch_counts_around_the_scan_tile(lvkv, gpu, nb):
    rng = np.random.default_rng(nb)
    b = batches_of(rng, [1 + (i % 97 == 0) for i in range(nb)], lambda i: b"k%06d" % (i * 7919 % nb))
    assert Mem(lvkv, gpu, *laid_out(b)).call().check()["nentries"] == nb + (nb + 96) // 97


@pytest.mark.gpu
@pytest.mark.parametrize("lead", [0, 1, 2, 5])
def test_three_byte_records_straddle_every_window_edge(lvkv, gpu, lead):
    # one batch of 3 W bytes of deletions of one-byte keys: with the window's edges 16-byte
    # aligned and W % 3 == 2, the edges fall at every residue of a record over the leads
    nrec = (3 * W - 12) // 3
    body = b"".join(mm.delete(bytes([97 + i % 5])) for i in range(nrec))
    batch = mm.batch(9, nrec, body)
    assert 3 * W - 3 < len(batch) <= 3 * W
    m = Mem(lvkv, gpu, batch, [0], [len(batch)], lead=lead)
    assert m.call().check()["nentries"] == nrec


@pytest.mark.gpu
def test_varints_split_across_the_window_edge(lvkv, gpu):
    # a put whose tag, two-byte key length and two-byte value length fall around batch
    # offset W (the buffer is 16-byte aligned: the first window ends there) in every way
    rng = np.random.default_rng(3)
    for extra in range(8):
        nfill = (W - 12 - 8) // 3
        fill = b"".join(mm.delete(b"f") for _ in range(nfill)) + mm.delete(b"g" * (1 + extra))
        at = 12 + len(fill)  # where the put's tag lies
        assert at == W - 5 + extra
        body = fill + mm.put(b"K" * 200, value(rng, 300)) + mm.put(b"L" * (W - 207), value(rng, 131))
        batch = mm.batch(1 << 40, nfill + 3, body)
        m = Mem(lvkv, gpu, batch, [0], [len(batch)])
        assert m.buf.data_ptr() % 16 == 0
        assert m.call().check()["nentries"] == nfill + 3


# ---- spare capacity, the tile's padding, the other tiles --------------------------------------

def spare_capacity_case(lvkv, gpu, n, max_entries, nb):
    """n entries over nb batches into max_entries slots: the grids are sized by
    max_entries, the true count is the control words'. check() holds the order
    and the fill past nentries."""
    rng = np.random.default_rng(100000 * nb + 10 * n + max_entries % 7)
    keys = [random_key(rng, WIDE if i % 2 else None) for i in range(n)]
    laid = laid_out(batches_of(rng, split(rng, n, nb), lambda i: keys[i], vlen=lambda i: i % 23),
                    gap=lambda b: b % 3)
    need = mm.from_batches(*laid)["report"]["key_bytes"]
    m = Mem(lvkv, gpu, *laid, max_entries=max_entries, key_capacity=need + 300 + n % 9,
            max_sequence=n // 2, shift=n % 16)
    rep = m.call().check()
    assert rep["nentries"] == n and rep["status"] == mm.OK and m.me == max_entries > n


@pytest.mark.gpu
@pytest.mark.parametrize("n,max_entries", [(1, 2 * T + 1), (T - 1, T + 1), (T + 1, 4 * T + 3),
                                           (2 * T + 1, 8 * T)])
@pytest.mark.parametrize("nb", [1, 9])
def test_spare_capacity_across_tiles(lvkv, gpu, n, max_entries, nb):
    spare_capacity_case(lvkv, gpu, n, max_entries, nb)


@pytest.mark.gpu
@pytest.mark.parametrize("nb", [1, 9])
def test_spare_capacity_and_no_entry_at_all(lvkv, gpu, nb):
    b = [mm.batch(50 + i, 0, b"") for i in range(nb)]
    m = Mem(lvkv, gpu, *laid_out(b, gap=lambda b: b % 3), max_entries=2 * T, key_capacity=300)
    rep = m.call().check()
    assert (rep["status"], rep["nentries"], rep["key_bytes"]) == (mm.OK, 0, 0)
    assert rep["max_sequence_out"] == 50 + nb - 2  # (sequence + count - 1 of the last batch)


# (eight 0xff and a ninth byte of 0xff is the key of nine: 22 keys)
TIE_KEYS = sorted({b"\xff" * l for l in range(7, 13)} |
                  {b"\xff" * 8 + bytes([x]) for x in (0, 1, 0x7f, 0x80, 0xfe, 0xff)} |
                  {b"a" + b"\0" * j for j in range(10)} | {b""})


def padding_case(lvkv, gpu, n, tile):
    """Keys whose prefix word ties with the padding's (eight 0xff bytes and
    more) or with one another's through the zero padding of a short key, each
    in three versions: two in the first tile, one in the last; random keys over
    every byte value around them."""
    rng = np.random.default_rng(n)
    step = (tile - 40) // len(TIE_KEYS)
    assert step >= 2 and n - len(TIE_KEYS) >= tile
    at = {}
    for j, k in enumerate(TIE_KEYS):
        at[3 + step * j] = at[3 + step * j + step // 2] = at[n - 1 - j] = k
    assert len(at) == 3 * len(TIE_KEYS)
    full = np.arange(256, dtype=np.uint8)
    keys = [at[i] if i in at else random_key(rng, full) for i in range(n)]
    laid = laid_out(batches_of(rng, split(rng, n, 5), lambda i: keys[i], vlen=lambda i: i % 11))
    m = Mem(lvkv, gpu, *laid)
    rep = m.call().check()
    assert rep["nentries"] == n and rep["status"] == mm.OK
    # the model's order has what the case is for: the 0xff keys last, after every random key
    ties = [k for k in TIE_KEYS if k[:8] == b"\xff" * 8]
    assert [k[:-8] for k in m.want["ikeys"][-3 * len(ties):]] == [k for k in ties for _ in range(3)]


@pytest.mark.gpu
@pytest.mark.parametrize("n", [T + 37, 2 * T])
def test_keys_that_tie_with_the_padding_and_with_zero_padded_prefixes(lvkv, gpu, n):
    """n = T + 37: the second tile is mostly padding; n = 2 T: there is none."""
    padding_case(lvkv, gpu, n, T)


def test_the_debug_tile_is_one_of_three(lvkv):
    f = lvkv.lib.lvkv_debug_set_memtable_tile
    try:
        for bad in (-1, 1, 2, 256, 511, 513, 1023, 1025, 2047, 2049, 4096, 1 << 20, -512):
            assert f(bad) != 0, bad
        for good in (512, 1024, 2048, 0):
            assert f(good) == 0
    finally:
        assert f(0) == 0


@pytest.mark.gpu
@pytest.mark.parametrize("tile", [512, 2048])
def test_the_other_sort_tiles(lvkv, gpu, tile):
    assert lvkv.lib.lvkv_debug_set_memtable_tile(tile) == 0
    try:
        for n in (tile - 1, tile + 1, 2 * tile + 1):
            spare_capacity_case(lvkv, gpu, n, n + tile + 3, 9)
        padding_case(lvkv, gpu, tile + 37, tile)
        padding_case(lvkv, gpu, 2 * tile, tile)
    finally:
        assert lvkv.lib.lvkv_debug_set_memtable_tile(0) == 0


# ---- keys -----------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("klen", [300, 2000])
def test_long_keys_that_differ_in_their_last_byte(lvkv, gpu, klen):
    rng = np.random.default_rng(klen)
    stem = rng.integers(0, 256, klen - 1, dtype=np.uint8).tobytes()
    last = rng.permutation(256).tolist()
    b = batches_of(rng, [100, 156], lambda i: stem + bytes([last[i]]))
    rep = Mem(lvkv, gpu, *laid_out(b, gap=lambda b: 5)).call().check()
    assert rep["max_key_len"] == klen + 8


@pytest.mark.gpu
def test_versions_of_one_user_key_cross_a_tile_and_a_merge_boundary(lvkv, gpu):
    rng = np.random.default_rng(8)
    n = 2 * T + 7  # T + 1 versions of "same", spread over three tiles
    which = set(rng.permutation(n)[:T + 1].tolist())
    b = batches_of(rng, split(rng, n, 9), lambda i: b"same" if i in which else b"k%05d" % (i % 50))
    assert Mem(lvkv, gpu, *laid_out(b)).call().check()["nentries"] == n


@pytest.mark.gpu
@pytest.mark.parametrize("shift", [0, 7, 15])
def test_keys_at_every_source_residue(lvkv, gpu, shift):
    rng = np.random.default_rng(shift)
    lens = [0, 1, 7, 8, 9, 15, 16, 17, 31, 33, 48, 64, 100, 255, 256, 257]
    keys = [bytes([65 + i % 26]) * lens[i % len(lens)] + b"%04d" % i for i in range(16 * len(lens))]
    b = batches_of(rng, [len(keys)], lambda i: keys[i], vlen=lambda i: 2 + i % 7, deletes=False)
    m = Mem(lvkv, gpu, *laid_out(b), lead=shift, shift=shift)
    es = mm.walk(m.payload, 0, len(m.payload))[1]
    assert {(e[0] + shift) % 16 for e in es} == set(range(16))
    m.call().check()


@pytest.mark.gpu
@pytest.mark.parametrize("order", ["sorted", "reversed", "equal_prefixes"])
def test_input_orders(lvkv, gpu, order):
    rng = np.random.default_rng(5)
    n = 3 * T + 11
    key = {"sorted": lambda i: b"%08d" % i, "reversed": lambda i: b"%08d" % (n - i),
           "equal_prefixes": lambda i: b"prefix__" + b"%06d" % (i * 7919 % n)}[order]
    assert Mem(lvkv, gpu, *laid_out(batches_of(rng, split(rng, n, 5), key))).call().check()


# ---- the fixtures ---------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("paranoid", [False, True])
@pytest.mark.parametrize("name", NAMES)
def test_fixture(lvkv, gpu, name, paranoid):
    payload, offs, lens = log_of(name)
    m = Mem(lvkv, gpu, payload, offs, lens, max_sequence=cases()[name]["max_sequence_in"],
            paranoid=paranoid)
    rep = m.call().check()
    ref = cases()[name]["paranoid" if paranoid else "plain"]
    assert rep["status"] == mm.STATUS_TEXT[ref["status"]]
    assert rep["max_sequence_out"] == ref["max_sequence"]


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_fixture_end_to_end(lvkv, gpu, name):
    import torch
    spec = cases()[name]
    log = torch.tensor(np.fromfile(GOLDEN / spec["log"], dtype=np.uint8), device=gpu)
    model = mm.from_batches(*log_of(name), max_sequence=0)
    payload = log_of(name)[0]
    for t in spec["plain"]["tables"] or [dict(kv_sep_size=16, ldb=None, vtb=None)]:
        image, vimage, reports, seq = lvkv.wal_recover_table(
            log, file_number=FILE_NUMBER, kv_sep_size=t["kv_sep_size"], compression=0,
            filter_bits_per_key=10)
        assert seq == model["report"]["max_sequence_out"]
        if t["ldb"] is None:
            assert image is None and vimage is None
            continue
        assert bytes(image.cpu().numpy()) == (GOLDEN / t["ldb"]).read_bytes()
        assert bytes(vimage.cpu().numpy()) == ((GOLDEN / t["vtb"]).read_bytes() if t["vtb"] else b"")
        # DBImpl::Get at the newest sequence, for every user key: its newest put, or nothing
        newest = {}
        for k, o, n in zip(model["ikeys"], model["val_off"], model["val_len"]):
            newest.setdefault(k[:-8], (vm.R_OK, payload[o + 1:o + n]) if k[-8] == 1
                              else (vm.R_SKIPPED, b""))
        users = sorted(newest)
        q = Packed(torch, gpu, [u + ((((1 << 56) - 1) << 8) | 1).to_bytes(8, "little") for u in users])
        got = lvkv.sst_get_values(image, {FILE_NUMBER: vimage}, q.buf, q.off[:len(users)],
                                  q.len[:len(users)], filter_policy=lvkv.BLOOM_POLICY,
                                  max_ulen=lvkv.SNAPPY_MAX_BLOCK)
        values = bytes(got["values"].cpu().numpy())
        offs = got["value_off"].cpu().tolist()
        assert got["status"].cpu().tolist() == [newest[u][0] for u in users]
        assert [values[a:b] for a, b in zip(offs, offs[1:])] == [newest[u][1] for u in users]
    # a paranoid recovery writes tables where the reference's does
    image, vimage, reports, seq = lvkv.wal_recover_table(
        log, file_number=FILE_NUMBER, kv_sep_size=16, paranoid=True,
        max_sequence=spec["max_sequence_in"], compression=0, filter_bits_per_key=10)
    wrote = spec["paranoid"]["writes_table"] and bool(spec["paranoid"]["entries"])
    assert (image is not None) == wrote
    assert seq == spec["paranoid"]["max_sequence"]


# ---- statuses -------------------------------------------------------------------------------

BAD = {mm.TOO_SMALL: bytes(11), mm.UNKNOWN_TAG: mm.batch(1, 2, mm.put(b"a", b"\x02v") + b"\x07"),
       mm.BAD_PUT: mm.batch(1, 2, mm.delete(b"a") + b"\x01\x01k\x09v"),
       mm.BAD_DELETE: mm.batch(1, 1, b"\x00\x80"),
       mm.WRONG_COUNT: mm.batch(1, 3, mm.put(b"a", b"\x02v") + mm.delete(b"b"))}


@pytest.mark.gpu
@pytest.mark.parametrize("batch_arrays", [True, False])
@pytest.mark.parametrize("where", [0, 3, 6])
@pytest.mark.parametrize("status", sorted(BAD))
def test_batch_statuses(lvkv, gpu, status, where, batch_arrays):
    rng = np.random.default_rng(status)
    good = batches_of(rng, [4] * 7, lambda i: b"key%03d" % (i * 5 % 28), seq0=100)
    b = good[:where] + [BAD[status]] + good[where + 1:]
    for paranoid in (False, True):
        m = Mem(lvkv, gpu, *laid_out(b), paranoid=paranoid, batch_arrays=batch_arrays,
                max_sequence=7)
        assert m.free["batch_status"][where] == status
        rep = m.call().check()
        assert rep["status"] == (status if paranoid else mm.OK)
        assert rep["first_bad_batch"] == (where if paranoid else mm.NONE)


@pytest.mark.gpu
@pytest.mark.parametrize("copies,apart", [(2, 1), (3, 1), (2, 2 * T), (3, 2 * T)])
def test_duplicate(lvkv, gpu, copies, apart):
    rng = np.random.default_rng(copies + apart)
    n = 2 * T * copies + 50
    spots = [40 + c * apart for c in range(copies)]
    # one entry a batch; the copies share user key, sequence and type
    b = [mm.batch(7 if i in spots else 1000 + i, 1,
                  mm.put(b"dup" if i in spots else b"k%06d" % (i * 31 % n), b"\x02" + bytes([i % 251])))
         for i in range(n)]
    m = Mem(lvkv, gpu, *laid_out(b))
    rep = m.call().check()
    assert rep["status"] == mm.DUPLICATE and rep["first_bad_entry"] == spots[1]


@pytest.mark.gpu
def test_key_too_long_is_decided_before_its_bytes_are_looked_at(lvkv, gpu):
    import torch
    klen = (1 << 32) - 8
    head = mm.batch(5, 1, b"\x01" + mm.varint(klen))
    claimed = len(head) + klen
    good = mm.batch(9, 1, mm.put(b"a", b"\x02v"))
    payload = good + head
    for paranoid in (False, True):
        m = Mem(lvkv, gpu, payload, [0, len(good)], [len(good), len(head)],
                virtual_len=[None, claimed], paranoid=paranoid)
        # the bytes the descriptor claims exist, untouched and never written
        m.buf = torch.empty(len(payload) + klen, dtype=torch.uint8, device=gpu)
        m.buf[:len(payload)] = torch.tensor(np.frombuffer(payload, dtype=np.uint8).copy(), device=gpu)
        rep = m.call().check()
        assert rep["status"] == mm.KEY_TOO_LONG and rep["first_bad_batch"] == 1
        del m
    # one byte shorter is a key like any other, which the batch then does not hold
    short = mm.batch(5, 1, b"\x01" + mm.varint(klen - 1) + b"k")
    m = Mem(lvkv, gpu, short, [0], [len(short)])
    assert m.call().check()["status"] == mm.OK and m.free["batch_status"] == [mm.BAD_PUT]


@pytest.mark.gpu
def test_capacity_one_short_then_the_repeat(lvkv, gpu):
    rng = np.random.default_rng(2)
    laid = laid_out(batches_of(rng, [300, 1, 811], lambda i: b"k%05d" % (i * 13 % 1112)))
    free = mm.from_batches(*laid)["report"]
    for short in (dict(max_entries=free["nentries"] - 1), dict(key_capacity=free["key_bytes"] - 1),
                  dict(max_entries=0), dict(key_capacity=0)):
        rep = Mem(lvkv, gpu, *laid, **short).call().check()
        assert rep["status"] == mm.CAPACITY
        again = Mem(lvkv, gpu, *laid, max_entries=rep["nentries"], key_capacity=rep["key_bytes"])
        assert again.call().check()["status"] == mm.OK


@pytest.mark.gpu
def test_invalid_arguments_and_the_empty_call(lvkv, gpu):
    import torch
    rng = np.random.default_rng(4)
    m = Mem(lvkv, gpu, *laid_out(batches_of(rng, [3, 2], lambda i: b"k%d" % i)))
    f = lvkv.lib.lvkv_memtable_from_batches_device
    base = [vp(m.buf), vp(m.boff), vp(m.blen), m.nb, 0, 0, vp(m.scratch), m.need, m.keys.ptr(),
            m.kc, m.koff.ptr(), m.klen.ptr(), m.voff.ptr(), m.vlen.ptr(), m.src.ptr(), m.me,
            m.bst.ptr(), m.bent.ptr(), vp(m.rep), _stream(gpu)]
    for null in (0, 1, 2, 6, 8, 10, 11, 12, 13, 14, 18):
        assert f(*[None if i == null else a for i, a in enumerate(base)]) == -1
    for at, v in ((3, 1 << 31), (15, 1 << 31), (7, m.need - 1)):
        assert f(*[v if i == at else a for i, a in enumerate(base)]) == -1
    torch.cuda.synchronize()
    assert (m.rep.cpu().numpy() == FILL).all() and (m.scratch.cpu().numpy() == FILL).all()
    m.call().check()  # the same arguments, whole
    # nbatches == 0, before every other check
    rep = torch.full((ctypes.sizeof(lvkv.MemtableReport) + 64,), FILL, dtype=torch.uint8, device=gpu)
    none = [None] * 20
    assert f(*[0 if i in (3, 4, 5, 7, 9, 15) else None for i in range(20)]) == 0
    none[3], none[4], none[5], none[7], none[9], none[15] = 0, 77, 1, 0, 0, 1 << 40
    none[18], none[19] = vp(rep), _stream(gpu)
    assert f(*none) == 0
    want = mm.from_batches(b"", [], [], max_sequence=77, paranoid=True)["report"]
    assert report(rep, lvkv.MemtableReport) == want
    out = lvkv.memtable_from_batches(torch.zeros(1, dtype=torch.uint8, device=gpu),
                                     torch.zeros(0, dtype=torch.int64, device=gpu),
                                     torch.zeros(0, dtype=torch.int64, device=gpu), max_sequence=77)
    assert out[0] == want and out[2].numel() == 0


# ---- random cases, and calls back to back ---------------------------------------------------

def random_case(rng, alphabet=None):
    nb = int(rng.integers(1, 9))
    keys = [random_key(rng, alphabet) for _ in range(12)]
    b = batches_of(rng, [int(rng.integers(0, 30)) for _ in range(nb)],
                   lambda i: keys[int(rng.integers(0, len(keys)))], seq0=int(rng.integers(0, 1 << 40)),
                   vlen=lambda i: int(rng.integers(0, 50)))
    for k in range(nb):  # damage: a flipped byte, a cut, a wrong count
        r = rng.random()
        x = bytearray(b[k])
        if r < 0.15 and len(x) > 12:
            x[int(rng.integers(8, len(x)))] ^= 1 << int(rng.integers(0, 8))
        elif r < 0.25:
            x = x[:int(rng.integers(0, len(x) + 1))]
        b[k] = bytes(x)
    return laid_out(b, gap=lambda b: int(rng.integers(0, 4)))


@pytest.mark.gpu
def test_random_cases_on_one_set_of_dirty_buffers(lvkv, gpu):
    random_cases(lvkv, gpu, 2024, None)


@pytest.mark.gpu
def test_random_cases_over_the_wide_alphabet(lvkv, gpu):
    random_cases(lvkv, gpu, 2026, WIDE)


def random_cases(lvkv, gpu, seed, alphabet):
    import torch
    rng = np.random.default_rng(seed)
    cap, kcap, nbmax = 512, 1 << 16, 8
    scratch = torch.full((int(lvkv.lib.lvkv_memtable_scratch_bytes(nbmax, cap)),), FILL,
                         dtype=torch.uint8, device=gpu)
    keys = torch.full((kcap,), FILL, dtype=torch.uint8, device=gpu)
    arr = {n: torch.full((cap,), -1, dtype=dt, device=gpu) for n, dt in
           (("key_off", torch.int64), ("key_len", torch.int32), ("val_off", torch.int64),
            ("val_len", torch.int32), ("src", torch.int32))}
    bst = torch.zeros(nbmax, dtype=torch.uint8, device=gpu)
    bent = torch.zeros(nbmax, dtype=torch.int32, device=gpu)
    rep = torch.zeros(ctypes.sizeof(lvkv.MemtableReport), dtype=torch.uint8, device=gpu)
    seen = set()
    for case in range(200):
        payload, offs, lens = random_case(rng, alphabet)
        paranoid = bool(case % 3 == 0)
        want = mm.from_batches(payload, offs, lens, max_sequence=case, paranoid=paranoid,
                               max_entries=cap, key_capacity=kcap)
        # (a duplicate is possible: equal keys at equal sequences after a flipped header byte)
        buf = torch.tensor(np.frombuffer(payload + b"", dtype=np.uint8).copy(), device=gpu) \
            if payload else torch.zeros(1, dtype=torch.uint8, device=gpu)
        boff = torch.tensor(offs, dtype=torch.int64, device=gpu)
        blen = torch.tensor(lens, dtype=torch.int64, device=gpu)
        rc = lvkv.lib.lvkv_memtable_from_batches_device(
            vp(buf), vp(boff), vp(blen), len(offs), case, int(paranoid), vp(scratch),
            scratch.numel(), vp(keys), kcap, vp(arr["key_off"]), vp(arr["key_len"]),
            vp(arr["val_off"]), vp(arr["val_len"]), vp(arr["src"]), cap, vp(bst), vp(bent),
            vp(rep), _stream(gpu))
        assert rc == 0
        got = lvkv.MemtableReport.from_buffer_copy(bytes(rep.cpu().numpy())).as_dict()
        assert got == want["report"], case
        assert bst[:len(offs)].cpu().tolist() == want["batch_status"], case
        assert bent[:len(offs)].cpu().tolist() == want["batch_entries"], case
        seen.add(got["status"])
        seen.update(want["batch_status"])
        if got["status"] != mm.OK:
            continue
        n = got["nentries"]
        assert bytes(keys[:got["key_bytes"]].cpu().numpy()) == want["keys"], case
        for name, t in arr.items():
            assert t[:n].cpu().tolist() == want[name], (case, name)
    assert seen >= {mm.OK, mm.TOO_SMALL, mm.UNKNOWN_TAG, mm.BAD_PUT, mm.WRONG_COUNT}


@pytest.mark.gpu
def test_three_calls_back_to_back_on_one_scratch(lvkv, gpu):
    import torch
    rng = np.random.default_rng(6)
    laid = [laid_out(batches_of(rng, split(rng, n, nb), lambda i: random_key(rng) + b"%d" % (i % 3)))
            for n, nb in ((T + 5, 3), (3 * T, 17), (40, 2))]
    need = max(int(lvkv.lib.lvkv_memtable_scratch_bytes(len(l[1]), mm.from_batches(*l)["report"]["nentries"]))
               for l in laid)
    scratch = torch.full((need + BORDER,), FILL, dtype=torch.uint8, device=gpu)
    ms = [Mem(lvkv, gpu, *l, scratch=scratch, paranoid=bool(i == 1)) for i, l in enumerate(laid)]
    for m in ms:
        m.call()
    for m in ms:
        m.check(own_scratch=False)
    assert (scratch[need:].cpu().numpy() == FILL).all()
