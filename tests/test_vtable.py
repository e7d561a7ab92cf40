"""KV separation on the device (include/lvkv_vtable.h) against
tests/vtable_model.py, which tests/test_vtable_model.py pins to the reference.

Every output array and report of lvkv_vtable_separate_device,
lvkv_vtable_resolve_device and lvkv_vtable_gather_device is compared with the
model's. The calls write into filled buffers with a border on either side of
every array and after the scratch; whatever the model does not name must
still hold the fill. The fixtures go end to end: sst_flush_separated gives
the reference's own .ldb and .vtb byte for byte, and sst_get_values hands
every original value back.
"""
from __future__ import annotations

import ctypes
import json
import subprocess

import numpy as np
import pytest

import vtable_model as vm
from conftest import GOLDEN, REPO
from test_vtable_model import TABLES, cases, ikey, table

FILL = 0xC3
PAD = 64        # slots of border before and after every per-entry array
BORDER = 4096   # bytes of border before and after every image, and after the scratch
U64 = (1 << 64) - 1


def s64(v):
    return v - (1 << 64) if v >= 1 << 63 else v


def vp(t, off=0):
    return ctypes.c_void_p(t.data_ptr() + off)


def _stream(dev):
    import torch
    return ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


class Packed:
    """Byte strings in one device buffer behind `lead` bytes, `gap(i)` bytes
    apart, with their offsets and lengths."""

    def __init__(self, torch, dev, pieces, lead=0, gap=lambda i: 0, lens=None):
        offs, at, parts = [], lead, [bytes(lead)]
        for i, p in enumerate(pieces):
            offs.append(at)
            g = gap(i)
            parts.append(p + bytes(g))
            at += len(p) + g
        self.host = b"".join(parts) + bytes(16)
        self.buf = torch.tensor(np.frombuffer(self.host, dtype=np.uint8).copy(), device=dev)
        self.offs, self.lens = offs, lens if lens is not None else [len(p) for p in pieces]
        self.off = torch.tensor(offs or [0], dtype=torch.int64, device=dev)
        self.len = torch.tensor([l - (1 << 32) if l >= 1 << 31 else l for l in self.lens] or [0],
                                dtype=torch.int32, device=dev)


class Out:
    """A filled device array of n items behind and before a border."""

    def __init__(self, torch, dev, n, dtype, pad, shift=0):
        self.n, self.pad, self.shift = n, pad, shift
        self.size = torch.empty(0, dtype=dtype).element_size()
        self.t = torch.full((pad + n + pad + (16 if shift else 0),), 0, dtype=dtype, device=dev)
        self.t.view(torch.uint8).fill_(FILL)
        self.at = (pad + shift) * self.size

    def ptr(self):
        return vp(self.t, self.at)

    def read(self):
        """(the n items, True when both borders still hold the fill)."""
        raw = self.t.cpu().numpy()
        b = raw.view(np.uint8)
        lo, hi = self.at, self.at + self.n * self.size
        clean = bool((b[:lo] == FILL).all() and (b[hi:] == FILL).all())
        return b[lo:hi].view(raw.dtype), clean


def report(buf, cls):
    raw = bytes(buf.cpu().numpy())
    n = ctypes.sizeof(cls)
    assert set(raw[n:]) == {FILL}, "a write past the report"
    return cls.from_buffer_copy(raw[:n]).as_dict()


class Separate:
    """One lvkv_vtable_separate_device call's buffers; call() launches (any
    number of times on the same buffers), check() compares with the model."""

    def __init__(self, lvkv, dev, entries, sep, number, *, vtb_cap=None, out_cap=None, lead=0,
                 gap=lambda i: 0, shift=0, val_lens=None, vals_buf=None):
        import torch
        self.lvkv, self.dev, self.entries, self.sep, self.number = lvkv, dev, entries, sep, number
        n = self.n = len(entries)
        self.model = vm.separate(entries, sep, number) if val_lens is None else None
        self.keys = Packed(torch, dev, [k for k, _ in entries], lead, gap)
        if vals_buf is None:
            self.vals = Packed(torch, dev, [v for _, v in entries], lead + 3, gap)
        else:
            self.vals = vals_buf
        rep = self.model["report"] if self.model else None
        self.vtb_cap = vtb_cap if vtb_cap is not None else rep["table_size"]
        self.out_cap = out_cap if out_cap is not None else rep["out_val_bytes"]
        self.vtb = Out(torch, dev, self.vtb_cap, torch.uint8, BORDER, shift)
        self.out = Out(torch, dev, self.out_cap, torch.uint8, BORDER, (shift * 7) % 16)
        self.ooff = Out(torch, dev, n, torch.int64, PAD)
        self.olen = Out(torch, dev, n, torch.int32, PAD)
        self.roff = Out(torch, dev, n, torch.int64, PAD)
        self.rsize = Out(torch, dev, n, torch.int64, PAD)
        self.need = int(lvkv.lib.lvkv_vtable_separate_scratch_bytes(n))
        self.scratch = torch.full((self.need + BORDER,), FILL, dtype=torch.uint8, device=dev)
        self.rep = torch.full((ctypes.sizeof(lvkv.VtableSeparateReport) + 64,), FILL,
                              dtype=torch.uint8, device=dev)

    def call(self):
        rc = self.lvkv.lib.lvkv_vtable_separate_device(
            vp(self.keys.buf), vp(self.keys.off), vp(self.keys.len), vp(self.vals.buf),
            vp(self.vals.off), vp(self.vals.len), self.n, self.sep, self.number, vp(self.scratch),
            self.need, self.vtb.ptr(), self.vtb_cap, self.out.ptr(), self.out_cap, self.ooff.ptr(),
            self.olen.ptr(), self.roff.ptr(), self.rsize.ptr(), vp(self.rep), _stream(self.dev))
        assert rc == 0
        return self

    def check(self, want=None, status=None):
        """want: the model's result (default: the unbounded call's, with
        `status` in place of its own when the capacities do not hold it)."""
        lvkv = self.lvkv
        want = want or self.model
        rep = report(self.rep, lvkv.VtableSeparateReport)
        wrep = dict(want["report"]) if status is None else dict(want["report"], status=status)
        assert rep == wrep
        assert (self.scratch[self.need:].cpu().numpy() == FILL).all(), "a write past the scratch"
        vtb, c0 = self.vtb.read()
        out, c1 = self.out.read()
        arrays = [a.read() for a in (self.ooff, self.olen, self.roff, self.rsize)]
        assert c0 and c1 and all(c for _, c in arrays), "a write into a border"
        if rep["status"] != vm.OK:
            assert (vtb == FILL).all() and (out == FILL).all()
            assert all((a.view(np.uint8) == FILL).all() for a, _ in arrays)
            return rep
        ts, ob = rep["table_size"], rep["out_val_bytes"]
        assert bytes(vtb[:ts]) == want["vtb"]
        assert bytes(out[:ob]) == b"".join(want["out_vals"])
        assert (vtb[ts:] == FILL).all() and (out[ob:] == FILL).all(), "a write past an image"
        lens = [len(v) for v in want["out_vals"]]
        assert arrays[1][0].tolist() == lens
        assert arrays[0][0].tolist() == np.concatenate([[0], np.cumsum(lens)[:-1]]).tolist()
        assert arrays[2][0].tolist() == want["rec_off"]
        assert arrays[3][0].tolist() == want["rec_size"]
        return rep


def seeded_entries(rng, n, lens, first=(2,)):
    """n entries, ascending user keys of 1 to 24 bytes, values of the lengths
    lens(i) (the whole value)."""
    out = []
    for i in range(n):
        user = b"%08d" % i + bytes(rng.integers(97, 123, int(rng.integers(0, 17)), dtype=np.uint8))
        ln = lens(i)
        v = bytes([first[i % len(first)]]) + rng.integers(0, 256, ln - 1, dtype=np.uint8).tobytes() \
            if ln else b""
        out.append((ikey(user, 1000 + i), v))
    return out


# ---- the host's checks: no device ----------------------------------------------------

def test_exported_symbols(lvkv):
    out = subprocess.run(["nm", "-D", "--defined-only", str(lvkv.LIB_PATH)], capture_output=True,
                         text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
    assert {"lvkv_vtable_separate_device", "lvkv_vtable_separate_scratch_bytes",
            "lvkv_vtable_separate_vtb_bound", "lvkv_vtable_separate_vals_bound",
            "lvkv_vtable_resolve_device", "lvkv_vtable_resolve_scratch_bytes",
            "lvkv_vtable_gather_device", "lvkv_vtable_gather_scratch_bytes"} <= exported


def test_report_mirrors_match_the_header(lvkv):
    text = (REPO / "include" / "lvkv_vtable.h").read_text()
    assert "#define LVKV_VRES_NSTATUS 12" in text
    assert ctypes.sizeof(lvkv.VtableSeparateReport) == 40
    assert ctypes.sizeof(lvkv.VtableResolveReport) == 64
    assert ctypes.sizeof(lvkv.VtableGatherReport) == 16
    for i, name in enumerate(("OK", "BAD_KEY", "BAD_VALUE", "TOO_LARGE", "CAPACITY")):
        assert f"#define LVKV_VTABLE_{name} {i}" in text and getattr(lvkv, "VTABLE_" + name) == i
    for i, name in enumerate(("OK", "SKIPPED", "EMPTY", "BAD_TYPE", "BAD_INDEX", "BAD_HANDLE",
                              "NO_FILE", "PAST_END", "BAD_HEADER", "BAD_RECORD", "TRAILING",
                              "RECORD_OVERRUN")):
        assert f"#define LVKV_VRES_{name} {i}" in text and getattr(lvkv, "VRES_" + name) == i


def test_host_validation_needs_no_device(lvkv):
    L = lvkv.lib
    p = ctypes.c_void_p(4096)  # (never dereferenced: the call is refused on the host)
    big = 1 << 20
    # n == 0 comes before every other check
    assert L.lvkv_vtable_separate_device(*([None] * 6), 0, 0, 0, None, 0, None, 0, None, 0,
                                         *([None] * 6)) == 0
    assert L.lvkv_vtable_resolve_device(*([None] * 4), 0, *([None] * 4), 0, None, 0,
                                        *([None] * 6)) == 0
    assert L.lvkv_vtable_gather_device(*([None] * 6), 0, None, 0, None, 0, None, None, None) == 0
    sep = [p] * 6 + [4, 16, 7, p, big, p, 100, p, 100, p, p, p, p, p, None]
    assert L.lvkv_vtable_separate_device(*sep[:9], p, 0, *sep[11:]) == -1  # scratch too small
    need = L.lvkv_vtable_separate_scratch_bytes(4)
    assert L.lvkv_vtable_separate_device(*sep[:9], p, need - 1, *sep[11:]) == -1
    assert L.lvkv_vtable_separate_device(*sep[:6], 1 << 31, *sep[7:9], p, 1 << 40, *sep[11:]) == -1
    for i in (0, 1, 2, 3, 4, 5, 9, 11, 13, 15, 16, 19):  # every pointer but rec_off / rec_size
        a = list(sep)
        a[i] = None
        assert L.lvkv_vtable_separate_device(*a) == -1, i
    res = [p, p, p, None, 4, p, p, p, p, 1, p, big, p, p, p, p, p, None]
    for i in (0, 1, 2, 5, 6, 7, 8, 10, 12, 13, 14, 15, 16):
        a = list(res)
        a[i] = None
        assert L.lvkv_vtable_resolve_device(*a) == -1, i
    a = list(res)
    a[11] = L.lvkv_vtable_resolve_scratch_bytes(4) - 1
    assert L.lvkv_vtable_resolve_device(*a) == -1
    a = list(res)
    a[4] = 1 << 31
    a[11] = 1 << 40
    assert L.lvkv_vtable_resolve_device(*a) == -1
    a = list(res)
    a[9] = 1 << 31
    assert L.lvkv_vtable_resolve_device(*a) == -1
    gat = [p, p, p, p, p, p, 4, p, big, p, 100, p, p, None]
    for i in (0, 1, 2, 3, 4, 5, 7, 9, 11, 12):
        a = list(gat)
        a[i] = None
        assert L.lvkv_vtable_gather_device(*a) == -1, i
    a = list(gat)
    a[8] = L.lvkv_vtable_gather_scratch_bytes(4) - 1
    assert L.lvkv_vtable_gather_device(*a) == -1
    a = list(gat)
    a[6], a[8] = 1 << 31, 1 << 40
    assert L.lvkv_vtable_gather_device(*a) == -1


def test_sizing_functions_are_monotone_and_bound_the_fixtures(lvkv):
    L = lvkv.lib
    ns = [0, 1, 2, 255, 256, 257, 4095, 4096, 4097, 8192, 8193, 100000, (1 << 31) - 1]
    for f in (L.lvkv_vtable_separate_scratch_bytes, L.lvkv_vtable_resolve_scratch_bytes,
              L.lvkv_vtable_gather_scratch_bytes):
        got = [f(n) for n in ns]
        assert got == sorted(got) and got[0] > 0
    assert L.lvkv_vtable_separate_vtb_bound(3, 10, 20) == 10 + 20 + 3 * 14
    assert L.lvkv_vtable_separate_vals_bound(3, 20) == 20 + 3 * 31
    for name in TABLES:
        spec, entries, _ = table(name)
        kb, vb = sum(len(k) for k, _ in entries), sum(len(v) for _, v in entries)
        for sep in (0 if all(v for _, v in entries) else 1, 1, 16, spec["kv_sep_size"]):
            rep = vm.separate(entries, sep, U64)["report"]
            assert rep["status"] == vm.OK
            assert rep["table_size"] <= L.lvkv_vtable_separate_vtb_bound(len(entries), kb, vb)
            assert rep["out_val_bytes"] <= L.lvkv_vtable_separate_vals_bound(len(entries), vb)


# ---- the fixtures, end to end ------------------------------------------------------------

def _device_entries(torch, dev, entries):
    k = Packed(torch, dev, [k for k, _ in entries])
    v = Packed(torch, dev, [v for _, v in entries])
    n = len(entries)
    return k.buf, k.off[:n], k.len[:n], v.buf, v.off[:n], v.len[:n]


@pytest.mark.gpu
@pytest.mark.parametrize("name", TABLES)
def test_fixture_end_to_end(lvkv, gpu, name):
    import torch
    spec, entries, vtb = table(name)
    image, vimage, reports = lvkv.sst_flush_separated(
        *_device_entries(torch, gpu, entries), kv_sep_size=spec["kv_sep_size"],
        file_number=spec["file_number"], compression=0, filter_bits_per_key=10)
    assert reports["separate"]["status"] == lvkv.VTABLE_OK
    assert (reports["separate"]["records_num"], reports["separate"]["table_size"]) == \
        (spec["records_num"], spec["table_size"])
    assert bytes(vimage.cpu().numpy()) == vtb
    assert bytes(image.cpu().numpy()) == (GOLDEN / spec["ldb"]).read_bytes()

    # what DBImpl::Get hands back for every entry's own key, by the model
    model = vm.separate(entries, spec["kv_sep_size"], spec["file_number"])
    want = []
    for (k, _), stored in zip(entries, model["out_vals"]):
        if k[-8] == 0:
            want.append((vm.R_SKIPPED, b""))
            continue
        st, src, off, ln, _ = vm.resolve(stored, [0], [len(stored)], vtb, [0], [len(vtb)],
                                         [spec["file_number"]])
        want.append((st[0], (vtb if src[0] else stored)[off[0]:off[0] + ln[0]]))
    assert sum(st == vm.R_OK for st, _ in want) >= len(entries) - 4
    rng = np.random.default_rng(11)
    n = len(entries)
    for order in (list(range(n)), rng.integers(0, n, 3 * n).tolist()):
        q = Packed(torch, gpu, [entries[i][0] for i in order])
        got = lvkv.sst_get_values(image, {spec["file_number"]: vimage}, q.buf, q.off[:len(order)],
                                  q.len[:len(order)], filter_policy=lvkv.BLOOM_POLICY,
                                  max_ulen=8192)
        values = bytes(got["values"].cpu().numpy())
        offs = got["value_off"].cpu().tolist()
        assert got["status"].cpu().tolist() == [want[i][0] for i in order]
        assert [values[a:b] for a, b in zip(offs, offs[1:])] == [want[i][1] for i in order]
        assert got["gather"]["nvalues"] == sum(want[i][0] == vm.R_OK for i in order)
        assert got["resolve"]["total_len"] == offs[-1] == got["gather"]["dst_bytes"]


# ---- the copy kernel's shapes ------------------------------------------------------------

STRIPPED = [0, 1, 15, 16, 17, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097]


@pytest.mark.gpu
@pytest.mark.parametrize("shift", [0, 5, 15])
def test_lengths_at_every_source_and_destination_residue(lvkv, gpu, shift):
    rng = np.random.default_rng(100 + shift)
    lens = [s + 1 for s in STRIPPED for _ in range(16)] + [300001, 7, 300001]
    entries = seeded_entries(rng, len(lens), lambda i: lens[i], first=(2, 1, 0, 255))
    # every piece starts one residue after the one before it
    sep = Separate(lvkv, gpu, entries, 1, 7, lead=shift, shift=shift,
                   gap=lambda i: (1 - len(entries[i][1])) % 16)
    assert {o % 16 for o in sep.vals.offs[:16 * len(STRIPPED)]} == set(range(16))
    assert {o % 16 for o in sep.model["rec_off"]} == set(range(16))
    rep = sep.call().check()
    assert rep["records_num"] == len(lens)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 63, 64, 65, 1023, 1024, 1025, 4097, 9001])
def test_entry_counts(lvkv, gpu, n):
    rng = np.random.default_rng(n)
    entries = seeded_entries(rng, n, lambda i: int(rng.integers(0, 40)))
    Separate(lvkv, gpu, entries, 16, 128, gap=lambda i: i % 3, shift=n % 16).call().check()


@pytest.mark.gpu
@pytest.mark.parametrize("pattern", ["all", "none", "alternating"])
def test_which_entries_move(lvkv, gpu, pattern):
    rng = np.random.default_rng(5)
    big = lambda i: pattern == "all" or (pattern == "alternating" and i % 2 == 0)
    entries = seeded_entries(rng, 700, lambda i: int(rng.integers(100, 400)) if big(i)
                             else int(rng.integers(0, 100)))
    rep = Separate(lvkv, gpu, entries, 100, 1 << 32, gap=lambda i: 1).call().check()
    assert rep["records_num"] == {"all": 700, "none": 0, "alternating": 350}[pattern]


@pytest.mark.gpu
@pytest.mark.parametrize("where", [0, 10, 20])
def test_a_long_record_first_in_the_middle_and_last(lvkv, gpu, where):
    rng = np.random.default_rng(where)
    entries = seeded_entries(rng, 21, lambda i: 300001 if i == where else int(rng.integers(1, 60)))
    Separate(lvkv, gpu, entries, 30, 127, gap=lambda i: 5, shift=where % 16).call().check()


@pytest.mark.gpu
@pytest.mark.parametrize("number", [0, 127, 128, 1 << 32, U64])
def test_file_numbers(lvkv, gpu, number):
    rng = np.random.default_rng(9)
    entries = seeded_entries(rng, 300, lambda i: int(rng.integers(1, 200)))
    sep = Separate(lvkv, gpu, entries, 64, number).call()
    sep.check()
    assert any(v.startswith(b"\x01" + vm.varint(number)) for v in sep.model["out_vals"])


# ---- failures ------------------------------------------------------------------------------

def _good(rng, n=9):
    return seeded_entries(rng, n, lambda i: 40 + i)


@pytest.mark.gpu
@pytest.mark.parametrize("at", [0, 4, 8])
@pytest.mark.parametrize("kind", ["short_key", "bad_type", "empty_value", "too_large"])
def test_each_failure_at_the_first_a_middle_and_the_last_entry(lvkv, gpu, kind, at):
    import torch
    rng = np.random.default_rng(3)
    entries = _good(rng)
    want = {"short_key": vm.BAD_KEY, "bad_type": vm.BAD_KEY, "empty_value": vm.BAD_VALUE,
            "too_large": vm.TOO_LARGE}[kind]
    sepsize, lens = 16, None
    if kind == "short_key":
        entries[at] = (b"seven..", entries[at][1])
    elif kind == "bad_type":
        entries[at] = (entries[at][0][:-8] + bytes([2]) + entries[at][0][-7:], entries[at][1])
    elif kind == "empty_value":
        entries[at], sepsize = (entries[at][0], b""), 0
    if kind == "too_large":
        # a descriptor of 2^32 - 1 bytes: nothing of the value may be read
        vals = Packed(torch, gpu, [v for _, v in entries])
        vals.lens[at] = 0xFFFFFFFF
        vals.len = torch.tensor([l if l < 1 << 31 else -1 for l in vals.lens], dtype=torch.int32,
                                device=gpu)
        sep = Separate(lvkv, gpu, entries, sepsize, 7, vtb_cap=4096, out_cap=4096,
                       val_lens=vals.lens, vals_buf=vals)
        rep = {"status": want, "first_bad_entry": at, "records_num": 0, "table_size": 0,
               "out_val_bytes": 0, "max_out_val_len": 0}
        sep.call().check(want={"report": rep})
        return
    model = vm.separate(entries, sepsize, 7)["report"]
    assert (model["status"], model["first_bad_entry"]) == (want, at)
    Separate(lvkv, gpu, entries, sepsize, 7, vtb_cap=4096, out_cap=4096).call().check()


@pytest.mark.gpu
def test_too_large_over_four_gib_that_are_never_touched(lvkv, gpu):
    import torch
    free, _ = torch.cuda.mem_get_info(gpu)
    if free < 6 << 30:
        pytest.fail("the device has no 4 GiB to allocate")
    rng = np.random.default_rng(4)
    entries = _good(rng, 3)
    vals = Packed(torch, gpu, [v for _, v in entries])
    vals.buf = torch.empty(1 << 32, dtype=torch.uint8, device=gpu)  # uninitialised
    vals.lens = [40, 0xFFFFFFFF, 42]
    vals.offs = [0, 0, 100]
    vals.off = torch.tensor(vals.offs, dtype=torch.int64, device=gpu)
    vals.len = torch.tensor([40, -1, 42], dtype=torch.int32, device=gpu)
    sep = Separate(lvkv, gpu, entries, 16, 7, vtb_cap=4096, out_cap=4096, val_lens=vals.lens,
                   vals_buf=vals)
    rep = {"status": vm.TOO_LARGE, "first_bad_entry": 1, "records_num": 0, "table_size": 0,
           "out_val_bytes": 0, "max_out_val_len": 0}
    sep.call().check(want={"report": rep})


@pytest.mark.gpu
def test_the_lower_of_two_failures_wins(lvkv, gpu):
    rng = np.random.default_rng(6)
    for first, second, want in (("value", "key", vm.BAD_VALUE), ("key", "value", vm.BAD_KEY)):
        entries = _good(rng, 600)  # (more than one workgroup)
        bad = {"value": lambda e: (e[0], b""), "key": lambda e: (b"short", e[1])}
        entries[70], entries[400] = bad[first](entries[70]), bad[second](entries[400])
        rep = Separate(lvkv, gpu, entries, 0, 7, vtb_cap=1 << 16, out_cap=1 << 16).call().check()
        assert (rep["status"], rep["first_bad_entry"]) == (want, 70)


@pytest.mark.gpu
@pytest.mark.parametrize("short", ["vtb", "out"])
def test_capacity_one_byte_short(lvkv, gpu, short):
    rng = np.random.default_rng(8)
    entries = seeded_entries(rng, 500, lambda i: int(rng.integers(0, 300)))
    full = vm.separate(entries, 100, 7)["report"]
    caps = dict(vtb_cap=full["table_size"] - (short == "vtb"),
                out_cap=full["out_val_bytes"] - (short == "out"))
    sep = Separate(lvkv, gpu, entries, 100, 7, **caps).call()
    rep = sep.check(status=vm.CAPACITY)
    assert (rep["table_size"], rep["out_val_bytes"]) == (full["table_size"], full["out_val_bytes"])
    # and the exact capacities hold it, on the same buffers' sizes plus the byte
    Separate(lvkv, gpu, entries, 100, 7).call().check()


# ---- resolve and gather --------------------------------------------------------------------

class Resolve:
    def __init__(self, lvkv, dev, values, files, state=None, lead=1, gap=lambda i: i % 5):
        import torch
        self.lvkv, self.dev, n = lvkv, dev, len(values)
        self.n, self.values, self.state_host = n, values, state
        self.vals = Packed(torch, dev, values, lead, gap)
        files = sorted(files, key=lambda f: f[0])
        self.fimg = Packed(torch, dev, [img for _, img in files], 7, lambda i: 3)
        self.fnum = [num for num, _ in files]
        self.nf = len(files)
        self.fnum_t = torch.tensor([s64(x) for x in self.fnum] or [0], dtype=torch.int64, device=dev)
        self.fsize_t = self.fimg.len.to(torch.int64)
        self.state = torch.tensor(state, dtype=torch.uint8, device=dev) if state is not None else None
        self.status = Out(torch, dev, n, torch.uint8, PAD)
        self.src = Out(torch, dev, n, torch.uint8, PAD)
        self.off = Out(torch, dev, n, torch.int64, PAD)
        self.len = Out(torch, dev, n, torch.int32, PAD)
        self.need = int(lvkv.lib.lvkv_vtable_resolve_scratch_bytes(n))
        self.scratch = torch.full((self.need + BORDER,), FILL, dtype=torch.uint8, device=dev)
        self.rep = torch.full((ctypes.sizeof(lvkv.VtableResolveReport) + 64,), FILL,
                              dtype=torch.uint8, device=dev)

    def call(self):
        nf = self.nf
        rc = self.lvkv.lib.lvkv_vtable_resolve_device(
            vp(self.vals.buf), vp(self.vals.off), vp(self.vals.len),
            vp(self.state) if self.state is not None else None, self.n,
            vp(self.fimg.buf) if nf else None, vp(self.fimg.off) if nf else None,
            vp(self.fsize_t) if nf else None, vp(self.fnum_t) if nf else None, nf,
            vp(self.scratch), self.need, self.status.ptr(), self.src.ptr(), self.off.ptr(),
            self.len.ptr(), vp(self.rep), _stream(self.dev))
        assert rc == 0
        return self

    def check(self):
        want = vm.resolve(self.vals.host, self.vals.offs, self.vals.lens, self.fimg.host,
                          self.fimg.offs, self.fimg.lens, self.fnum, self.state_host)
        got = [a.read() for a in (self.status, self.src, self.off, self.len)]
        assert all(c for _, c in got), "a write into a border"
        assert (self.scratch[self.need:].cpu().numpy() == FILL).all(), "a write past the scratch"
        for g, w in zip(got, want[:4]):
            assert g[0].tolist() == w
        assert report(self.rep, self.lvkv.VtableResolveReport) == want[4]
        return want


def damaged_values(rng, entries, model, number):
    """Stored values and vTable files with seeded damage of every kind, and
    the files: [(number, image)]."""
    vtb = bytearray(model["vtb"])
    recs = [(o, s) for o, s in zip(model["rec_off"], model["rec_size"]) if s]
    ix = vm.index_value
    values = [b"\x02" + v if len(v) < 16 else o for (_, v), o in zip(entries, model["out_vals"])]
    o0, s0 = recs[0]
    values += [b"", b"\x02", b"\x00abc", b"\x03", b"\xff" + ix(number, o0, s0)[1:],
               b"\x01", b"\x01\x80", b"\x01" + b"\x80" * 10 + b"\x01", ix(number, o0, s0)[:-1],
               b"\x01\x07", b"\x01\x07\x05", b"\x01\x07\x05\x80",
               ix(number + 1, o0, s0), ix(number - 1, o0, s0), ix(U64, o0, s0), ix(0, o0, s0),
               ix(number, len(vtb), 0), ix(number, len(vtb), 4), ix(number, len(vtb) + 1, 0),
               ix(number, o0, len(vtb) - o0 + 1), ix(number, U64, 2), ix(number, 2, U64),
               ix(number, U64, U64), ix(number, o0, 0), ix(number, o0, 3), ix(number, o0, 4),
               ix(number, o0, s0 - 1), ix(number, o0, s0 + 1) + b"trailing", ix(number, o0 + 1, s0)]
    # records edited in place: the header one less and one more, a key that passes the record
    o1, s1 = recs[1]
    vtb[o1:o1 + 4] = (s1 - 4 - 1).to_bytes(4, "little")
    o2, s2 = recs[2]
    vtb[o2:o2 + 4] = (s2 - 4 + 1).to_bytes(4, "little")
    o3, s3 = recs[3]
    vtb[o3 + 4] = 0xFF
    o4, s4 = recs[4]
    vtb[o4 + 4:o4 + 9] = b"\xff\xff\xff\xff\x7f"
    values += [ix(number, o2, s2 + 1)]  # (the lengthened record reaches into the next: trailing)
    return values, bytes(vtb)


@pytest.mark.gpu
@pytest.mark.parametrize("nfiles", [1, 2, 17])
@pytest.mark.parametrize("with_state", [False, True])
def test_resolve_every_status_on_seeded_damage(lvkv, gpu, nfiles, with_state):
    rng = np.random.default_rng(20 + nfiles)
    number = 1000
    entries = seeded_entries(rng, 300, lambda i: int(rng.integers(1, 120)))
    model = vm.separate(entries, 16, number)
    values, vtb = damaged_values(rng, entries, model, number)
    # the other files: real images under other numbers, among them the neighbours
    others = [number + d for d in (2, -2, 5, -5, 100, 1 << 40, -900, 3, 7, 9, 11, 13, 15, 17, 19, 21)]
    files = [(number, vtb)] + [(x, model["vtb"][:200 + 13 * i]) for i, x in enumerate(others)]
    files = files[:nfiles]
    state = None
    if with_state:
        # (the entries' own values: some not FOUND; the damaged ones are all looked at)
        state = [int(s) for s in rng.choice([1, 1, 1, 0, 2, 3, 7], len(entries))]
        state += [1] * (len(values) - len(entries))
    res = Resolve(lvkv, gpu, values, files, state).call()
    want = res.check()
    seen = set(want[0])
    assert seen >= set(range(vm.NSTATUS)) - ({vm.R_SKIPPED} if not with_state else set())
    # gather what it found, exactly and one byte short
    _gather_and_check(lvkv, gpu, res, want)


def _gather_and_check(lvkv, dev, res, want, repeat=1):
    import torch
    status, src, off, ln, _ = want
    dst_w, off_w, rep_w = vm.gather(res.vals.host, res.fimg.host, status, src, off, ln)
    for cap in (len(dst_w), len(dst_w) - 1):
        for shift in (0, 9):
            dst = Out(torch, dev, cap, torch.uint8, BORDER, shift)
            doff = Out(torch, dev, res.n + 1, torch.int64, PAD)
            need = int(lvkv.lib.lvkv_vtable_gather_scratch_bytes(res.n))
            scratch = torch.full((need + BORDER,), FILL, dtype=torch.uint8, device=dev)
            rep = torch.full((16 + 64,), FILL, dtype=torch.uint8, device=dev)
            for _ in range(repeat):
                rc = lvkv.lib.lvkv_vtable_gather_device(
                    vp(res.vals.buf), vp(res.fimg.buf), res.status.ptr(), res.src.ptr(),
                    res.off.ptr(), res.len.ptr(), res.n, vp(scratch), need, dst.ptr(), cap,
                    doff.ptr(), vp(rep), _stream(dev))
                assert rc == 0
            got = report(rep, lvkv.VtableGatherReport)
            d, c0 = dst.read()
            o, c1 = doff.read()
            assert c0 and c1 and (scratch[need:].cpu().numpy() == FILL).all()
            if cap == len(dst_w):
                assert got == rep_w and bytes(d) == dst_w and o.tolist() == off_w
            else:
                assert got == dict(rep_w, status=vm.CAPACITY)
                assert (d == FILL).all() and (o.view(np.uint8) == FILL).all()


@pytest.mark.gpu
def test_unknown_file_numbers_and_no_files(lvkv, gpu):
    rng = np.random.default_rng(31)
    entries = seeded_entries(rng, 40, lambda i: 30 + i)
    model = vm.separate(entries, 16, 50)
    for files in ([], [(49, model["vtb"])], [(49, model["vtb"]), (51, model["vtb"])]):
        want = Resolve(lvkv, gpu, model["out_vals"] + [b"\x02plain"], files).call().check()
        assert want[4]["count"][vm.R_NO_FILE] == 40 and want[4]["count"][vm.R_OK] == 1
    # a list that does not ascend may miss a file, and stays inside the list
    res = Resolve(lvkv, gpu, model["out_vals"], [(50, model["vtb"])])
    res.nf, res.fnum = 3, [90, 50, 10]
    import torch
    res.fnum_t = torch.tensor(res.fnum, dtype=torch.int64, device=gpu)
    res.fimg.off = res.fimg.off.repeat(3)
    res.fsize_t = res.fsize_t.repeat(3)
    res.fimg.offs, res.fimg.lens = res.fimg.offs * 3, res.fimg.lens * 3
    res.call().check()


# ---- reuse -----------------------------------------------------------------------------------

@pytest.mark.gpu
def test_three_calls_back_to_back_and_thrice_on_dirty_outputs(lvkv, gpu):
    import torch
    rng = np.random.default_rng(40)
    entries = seeded_entries(rng, 1500, lambda i: int(rng.integers(1, 90)))
    seps = [Separate(lvkv, gpu, entries, s, 77, shift=s % 16) for s in (16, 40, 1000)]
    short = Separate(lvkv, gpu, entries, 16, 77, vtb_cap=100, out_cap=1 << 20)
    for s in seps:  # no wait between them
        s.call()
    for s in seps:
        s.check()
    for s in seps:  # each three times on what the last call left
        s.call().call().call()
    short.call().call().call()
    torch.cuda.synchronize(gpu)
    for s in seps:
        s.check()
    short.check(status=vm.CAPACITY)
    # resolve and gather: three times each on the same outputs
    model = seps[0].model
    res = Resolve(lvkv, gpu, model["out_vals"], [(77, model["vtb"])])
    res.call().call().call()
    want = res.check()
    assert want[4]["count"][vm.R_OK] == len(entries)
    _gather_and_check(lvkv, gpu, res, want, repeat=3)


@pytest.mark.gpu
def test_wrappers_take_an_empty_batch(lvkv, gpu):
    import torch
    e8 = torch.zeros(0, dtype=torch.uint8, device=gpu)
    e64 = torch.zeros(0, dtype=torch.int64, device=gpu)
    e32 = torch.zeros(0, dtype=torch.int32, device=gpu)
    sep = lvkv.vtable_separate(e8, e64, e32, e8, e64, e32, file_number=7)
    assert sep["report"] == {"status": 0, "first_bad_entry": lvkv.VTABLE_NO_ENTRY,
                             "records_num": 0, "table_size": 0, "out_val_bytes": 0,
                             "max_out_val_len": 0}
    st, src, off, ln, rep = lvkv.vtable_resolve(e8, e64, e32, e8, e64, e64, e64)
    assert rep == {"nqueries": 0, "count": [0] * 12, "max_len": 0, "total_len": 0}
    dst, dst_off, grep = lvkv.vtable_gather(e8, e8, st, src, off, ln)
    assert grep == {"status": 0, "nvalues": 0, "dst_bytes": 0} and dst_off.cpu().tolist() == [0]
