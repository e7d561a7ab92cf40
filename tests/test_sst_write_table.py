"""lvkv_sst_write_table_device: TableBuilder::Flush + Finish on the device.

The expectation is tests/sst_finish_model.py, and the model is pinned first
(CPU tests): from the data blocks alone it rebuilds, byte for byte, five
tables the reference's TableBuilder wrote -- tests/golden/table.sst
(oracle/gen_golden.cc) and the four finish_*.sst of
tests/golden/gen_table_finish.cc (internal keys under snappy with filters
that blocks share and one user key on both sides of a block boundary; the
separator edge cases with a 10 KiB block that leaves empty filters; no filter
policy; no entries).

The GPU tests compare the whole image file[:file_size], the handles, types
and report of one call with the model's (or the fixture itself), and give the
call damaged blocks, a file one byte short, and dirty buffers twice in a row.
"""
from __future__ import annotations

import ctypes
import functools
import json

import numpy as np
import pytest

import snappy_oracle as so
import sst_finish_model as fm
from conftest import GOLDEN

FIXTURES = ["finish_internal_snappy", "finish_edges", "finish_nofilter", "finish_empty"]
REPORT_KEYS = ["status", "first_bad_block", "num_entries", "nfilters", "meta_type", "index_type",
               "meta_status", "index_status", "data_end", "filter_offset", "filter_size",
               "meta_offset", "meta_size", "index_offset", "index_size", "file_size"]
FILL = 0xC3
BORDER = 4096


# ---- inputs ---------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _fixture(name):
    """(image, options, data blocks' contents, handles, types) of a table the
    reference wrote."""
    if name == "table":
        img = (GOLDEN / "table.sst").read_bytes()
        # (every block of the file: the last three are filter, metaindex, index)
        blocks = json.loads((GOLDEN / "table_blocks.json").read_text())["blocks"][:-3]
        assert len(blocks) == 49
        opts = {"key_format": 0, "bits_per_key": 10, "compression": 0}
    else:
        img = (GOLDEN / f"{name}.sst").read_bytes()
        spec = json.loads((GOLDEN / "finish_tables.json").read_text())[name]
        assert spec["file_bytes"] == len(img)
        blocks = spec["blocks"]
        opts = {k: spec[k] for k in ("key_format", "bits_per_key", "compression")}
    raws = []
    for b in blocks:
        st, raw = so.read_block(img, b["offset"], b["size"])
        assert st == so.READ_OK and img[b["offset"] + b["size"]] == b["type"]
        raws.append(raw)
    return (img, opts, tuple(raws), [(b["offset"], b["size"]) for b in blocks],
            [b["type"] for b in blocks])


def _ikey(user: bytes, seq: int) -> bytes:
    return user + ((seq << 8) | 1).to_bytes(8, "little")


@functools.lru_cache(maxsize=None)
def _bench_blocks():
    """64 blocks of 1-6 KiB, internal keys, db_bench-like half-compressible
    values, restart interval 16."""
    rng = np.random.default_rng(7)
    blocks, i = [], 0
    for b in range(64):
        want, entries, size = 1024 + int(rng.integers(0, 5 * 1024)), [], 0
        while size < want:
            piece = rng.integers(32, 127, size=50, dtype=np.uint8).tobytes()
            entries.append((_ikey(b"%016d" % (i * 3), 1000 + i), piece * 2))
            size += 130
            i += 1
        blocks.append(fm.block_of(entries, 16))
    return tuple(blocks)


@functools.lru_cache(maxsize=None)
def _tiny_blocks(n, key_len=16):
    """n one-entry blocks: a key of key_len bytes and a value that brings the
    block to about 40 bytes."""
    return tuple(fm.block_of([(b"%0*d" % (key_len, i * 5), b"v" * (40 - 11 - key_len))], 16)
                 for i in range(n))


@functools.lru_cache(maxsize=None)
def _model(blocks, key_format, bits, compression, level=1):
    return fm.finish(blocks, key_format, bits, compression, level, device_limits=True)


# ---- the model against the reference's tables (CPU) -----------------------------

@pytest.mark.parametrize("name", ["table"] + FIXTURES)
def test_model_reproduces_reference_table(name):
    img, opts, raws, handles, types = _fixture(name)
    t = fm.finish(raws, opts["key_format"], opts["bits_per_key"], opts["compression"])
    assert t.handles == handles and t.types == types
    assert t.report["file_size"] == len(img)
    assert t.image == img


def test_fixtures_hold_their_cases():
    """What the generator was written to produce is in the files."""
    img, _, raws, handles, _ = _fixture("finish_internal_snappy")
    ends = [(o + s + 5) >> 11 for o, s in handles]
    assert max(ends.count(e) for e in set(ends)) >= 3  # blocks sharing a filter
    keys = [fm.block_keys(r) for r in raws]
    twice = [i for i in range(len(keys) - 1) if keys[i][-1][:-8] == keys[i + 1][0][:-8]]
    assert twice  # one user key on both sides of a boundary
    i = twice[0]
    assert fm.index_key(keys[i][-1], keys[i + 1][0], 1) == keys[i][-1]
    _, _, raws, handles, _ = _fixture("finish_edges")
    keys = [fm.block_keys(r) for r in raws]
    seps = [fm.index_key(keys[i][-1], keys[i + 1][0] if i + 1 < len(keys) else None, 0)
            for i in range(len(keys))]
    assert seps[:6] == [b"aa\x01", b"ab\x02", b"abc", b"a\xffz", b"b", b"c"]
    assert seps[-1] == b"\xff\xff\xff" and len(keys[4]) == 1
    t = fm.finish(raws, 0, 10, 0)
    fb = t.image[t.report["filter_offset"]:][:t.report["filter_size"]]
    arr = int.from_bytes(fb[-5:-1], "little")
    offs = [int.from_bytes(fb[arr + 4 * i:][:4], "little") for i in range(t.report["nfilters"])]
    assert max(offs.count(o) for o in set(offs)) >= 5  # four or more empty filters
    img, *_ = _fixture("finish_empty")
    assert img[:5] == bytes([0, 0, 0, 0, 11])
    img, _, _, handles, _ = _fixture("finish_nofilter")
    t = fm.finish(_fixture("finish_nofilter")[2], 0, 0, 0)
    assert t.meta_contents == bytes([0, 0, 0, 0, 1, 0, 0, 0]) and t.report["filter_size"] == 0


# ---- the C ABI without a device ---------------------------------------------------

def _abi_args(lvkv, **over):
    """A call's arguments with made-up non-null pointers (never dereferenced:
    every case here is rejected before a launch)."""
    L = lvkv.lib
    p = ctypes.c_void_p(0x1000)
    need = L.lvkv_sst_write_table_scratch_bytes(4, 0, 4096, 64, 10)
    a = dict(raw=p, off=p, len=p, n=4, compression=1, level=1, max_len=4096, key_format=1,
             bits=10, max_key_len=64, scratch=p, scratch_bytes=need, file=p, cap=1 << 20, hoff=p,
             hsize=p, type=p, status=p, report=p, stream=None)
    a.update(over)
    return list(a.values())


def test_host_validation_needs_no_device(lvkv):
    L = lvkv.lib
    bad = lvkv.LVKV_ERR_INVALID
    for name in ("raw", "off", "len", "scratch", "file", "hoff", "hsize", "type", "status",
                 "report"):
        assert L.lvkv_sst_write_table_device(*_abi_args(lvkv, **{name: None})) == bad, name
    for over in (dict(compression=3), dict(compression=-1), dict(key_format=2),
                 dict(key_format=-1), dict(compression=2, level=0), dict(compression=2, level=3),
                 dict(bits=-1), dict(max_key_len=(1 << 20) + 1)):
        assert L.lvkv_sst_write_table_device(*_abi_args(lvkv, **over)) == bad, over
    short = _abi_args(lvkv)[11] - 1
    assert L.lvkv_sst_write_table_device(*_abi_args(lvkv, scratch_bytes=short)) == bad


def test_sizing_functions_are_monotone(lvkv):
    L = lvkv.lib
    base = dict(n=100, total=400_000, max_len=4096, mkl=64, bits=10)

    def scratch(**o):
        a = {**base, **o}
        return L.lvkv_sst_write_table_scratch_bytes(a["n"], a["total"], a["max_len"], a["mkl"],
                                                    a["bits"])

    def bound(**o):
        a = {**base, **o}
        return L.lvkv_sst_table_file_bound(a["n"], a["total"], a["mkl"], a["bits"])

    steps = dict(n=[0, 1, 2, 99, 100, 101, 5000], total=[0, 1, 4096, 400_000, 400_001, 1 << 30],
                 max_len=[0, 1, 4096, 20480, 20481, 65536, 131072, 1 << 20],
                 mkl=[0, 1, 8, 64, 65, 1024], bits=[0, 1, 10, 11, 40])
    for arg, values in steps.items():
        s = [scratch(**{arg: v}) for v in values]
        assert s == sorted(s), (arg, s)
        if arg != "max_len":
            f = [bound(**{arg: v}) for v in values]
            assert f == sorted(f), (arg, f)


def test_sizing_functions_answer_as_recorded(lvkv):
    """tests/golden/scratch_sizes.json (gen_scratch_sizes.py): every value of
    the write path's seven sizing functions over a grid that crosses their
    branches. Callers allocate by these; no layout change may move one."""
    calls = json.loads((GOLDEN / "scratch_sizes.json").read_text())["calls"]
    assert sorted(calls) == [
        "lvkv_sst_build_blocks_raw_bound", "lvkv_sst_build_blocks_scratch_bytes",
        "lvkv_sst_table_file_bound", "lvkv_sst_write_scratch_bytes",
        "lvkv_sst_write_scratch_bytes_v2", "lvkv_sst_write_table_scratch_bytes",
        "lvkv_zstd_compress_big_scratch_bytes"]
    assert sum(len(rows) for rows in calls.values()) > 700
    for fn, rows in calls.items():
        f = getattr(lvkv.lib, fn)
        for *args, want in rows:
            assert f(*args) == want, (fn, args)


def _cases():
    """(name, blocks, key_format, bits) of every table the GPU tests build."""
    for name in ["table"] + FIXTURES:
        _, opts, raws, _, _ = _fixture(name)
        yield name, raws, opts["key_format"], opts["bits_per_key"]
    yield "bench", _bench_blocks(), 1, 10
    yield "tiny4101", _tiny_blocks(4101), 0, 10
    yield "tiny6000", _tiny_blocks(6000), 0, 10
    yield "single", _fixture("table")[2][:1], 0, 10


def test_file_bound_covers_every_case(lvkv):
    for name, raws, key_format, bits in _cases():
        t = fm.finish(raws, key_format, bits, 0)  # (raw: the longest image)
        mkl = max((len(k) for r in raws for k in fm.block_keys(r)), default=0)
        bound = lvkv.lib.lvkv_sst_table_file_bound(len(raws), sum(map(len, raws)), mkl, bits)
        assert bound >= len(t.image), name
    for name in ["table"] + FIXTURES:
        img, opts, raws, _, _ = _fixture(name)
        assert lvkv.lib.lvkv_sst_table_file_bound(len(raws), sum(map(len, raws)), 64,
                                                  opts["bits_per_key"]) >= len(img)


# ---- on the device -----------------------------------------------------------------

def _pack(torch, dev, blocks):
    """The blocks one byte apart (every alignment) between borders."""
    offs, p = [], BORDER
    for b in blocks:
        offs.append(p)
        p += len(b) + 1
    host = np.full(p + BORDER, FILL, dtype=np.uint8)
    for o, b in zip(offs, blocks):
        host[o:o + len(b)] = np.frombuffer(b, dtype=np.uint8)
    return (torch.from_numpy(host).to(dev), torch.tensor(offs, dtype=torch.int64, device=dev),
            torch.tensor([len(b) for b in blocks], dtype=torch.int32, device=dev))


def _max_key(blocks):
    return max((len(k) for b in blocks for k in fm.block_keys(b)), default=8)


def _write(lvkv, gpu, blocks, *, key_format, bits, compression, level=1, max_key_len=None,
           capacity=None, max_len=None):
    """One call between borders: the file and the scratch are views of
    tensors whose last BORDER bytes must stay FILL. Returns the wrapper's
    tuple with the file as host bytes."""
    import torch
    raw, off, ln = _pack(torch, gpu, blocks)
    mkl = _max_key(blocks) if max_key_len is None else max_key_len
    total = sum(map(len, blocks))
    if max_len is None:
        max_len = max(map(len, blocks), default=0)
    need = lvkv.lib.lvkv_sst_write_table_scratch_bytes(len(blocks), total, max_len, mkl, bits)
    cap = capacity if capacity is not None else \
        lvkv.lib.lvkv_sst_table_file_bound(len(blocks), total, mkl, bits)
    file = torch.full((cap + BORDER,), FILL, dtype=torch.uint8, device=gpu)
    scratch = torch.full((need + BORDER,), FILL, dtype=torch.uint8, device=gpu)
    out = lvkv.sst_write_table(raw, off, ln, compression=compression, zstd_level=level,
                               max_len=max_len, key_format=key_format, filter_bits_per_key=bits,
                               max_key_len=mkl, file=file, file_capacity=cap,
                               scratch=scratch[:need])
    host = file.cpu().numpy()
    assert (host[cap:] == FILL).all(), "a write past file_capacity"
    assert (scratch[need:].cpu().numpy() == FILL).all(), "a write past the scratch"
    return (bytes(host[:cap]),) + tuple(out[1:])


def _expect(out, t):
    """The call's outputs against a model table."""
    file, hoff, hsize, typ, status, rep = out
    assert {k: rep[k] for k in REPORT_KEYS} == {k: t.report[k] for k in REPORT_KEYS}
    assert list(zip(hoff.tolist(), hsize.tolist())) == t.handles
    assert typ.tolist() == t.types
    assert not status.any()
    got = file[:rep["file_size"]]
    if got != t.image:
        first = next(i for i, (a, b) in enumerate(zip(got, t.image)) if a != b)
        raise AssertionError(f"image differs from byte {first} of {len(t.image)} "
                             f"(data_end {rep['data_end']}, report {rep})")


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["table"] + FIXTURES)
def test_reference_tables_from_their_data_blocks(lvkv, gpu, name):
    img, opts, raws, handles, types = _fixture(name)
    out = _write(lvkv, gpu, raws, key_format=opts["key_format"], bits=opts["bits_per_key"],
                 compression=opts["compression"])
    file, hoff, hsize, typ, status, rep = out
    assert rep["status"] == lvkv.TABLE_OK and rep["file_size"] == len(img)
    assert file[:len(img)] == img
    assert list(zip(hoff.tolist(), hsize.tolist())) == handles and typ.tolist() == types
    _expect(out, _model(raws, opts["key_format"], opts["bits_per_key"], opts["compression"]))


@pytest.mark.gpu
@pytest.mark.parametrize("compression,level", [(1, 1), (2, 1), (2, -1)],
                         ids=["snappy", "zstd1", "zstd-1"])
def test_table_blocks_compressed(lvkv, gpu, compression, level):
    raws = _fixture("table")[2]
    _expect(_write(lvkv, gpu, raws, key_format=0, bits=10, compression=compression, level=level),
            _model(raws, 0, 10, compression, level))


@pytest.mark.gpu
@pytest.mark.parametrize("compression", [0, 1, 2])
def test_bench_blocks_internal_keys(lvkv, gpu, compression):
    raws = _bench_blocks()
    _expect(_write(lvkv, gpu, raws, key_format=1, bits=10, compression=compression),
            _model(raws, 1, 10, compression))


@pytest.mark.gpu
@pytest.mark.parametrize("compression", [0, 1])
@pytest.mark.parametrize("nblocks", [1024, 1025, 4101])
def test_many_small_blocks_share_filters(lvkv, gpu, compression, nblocks):
    """The scans that carry a total from one pass of 1,024 blocks to the next
    (the slot scan, the finisher's three), at exactly one pass, at one block
    past it, and at 4,101 blocks: five passes of those, two of the writer's
    layout; some fifty blocks a filter."""
    raws = _tiny_blocks(nblocks)
    t = _model(raws, 0, 10, compression)
    assert t.report["nfilters"] < nblocks // 40
    _expect(_write(lvkv, gpu, raws, key_format=0, bits=10, compression=compression), t)


@pytest.mark.gpu
@pytest.mark.parametrize("compression", [1, 2], ids=["snappy", "zstd1"])
def test_index_block_past_128k(lvkv, gpu, compression):
    raws = _tiny_blocks(6000)
    t = _model(raws, 0, 10, compression)
    assert len(t.index_contents) > 128 << 10
    out = _write(lvkv, gpu, raws, key_format=0, bits=10, compression=compression)
    rep = out[5]
    if compression == 1:
        assert rep["index_status"] == 0 and rep["index_type"] == 1
    else:
        assert rep["index_status"] == lvkv.ZSTD_TOO_LARGE and rep["index_type"] == 0
        assert rep["status"] == lvkv.TABLE_OK
    _expect(out, t)


@pytest.mark.gpu
@pytest.mark.parametrize("bits", [10, 0])
def test_no_blocks(lvkv, gpu, bits):
    t = _model((), 0, bits, 0)
    if bits:
        assert t.image == _fixture("finish_empty")[0]
    _expect(_write(lvkv, gpu, (), key_format=0, bits=bits, compression=0), t)
    _expect(_write(lvkv, gpu, (), key_format=1, bits=bits, compression=1),
            _model((), 1, bits, 1))


@pytest.mark.gpu
def test_single_block(lvkv, gpu):
    raws = _fixture("table")[2][:1]
    for compression in (0, 1):
        _expect(_write(lvkv, gpu, raws, key_format=0, bits=10, compression=compression),
                _model(raws, 0, 10, compression))


@pytest.mark.gpu
@pytest.mark.parametrize("max_key_len", [512, 513, 600])
def test_long_keys_on_either_side_of_the_lds_bound(lvkv, gpu, max_key_len):
    """The bit-setting kernel rebuilds keys in LDS up to max_key_len 512 and
    in the scratch past it: a key of exactly max_key_len bytes, sharing a
    prefix with its neighbours, under both."""
    long_user = b"9" * (max_key_len - 8 - 3)
    entries = [(_ikey(long_user + b"%03d" % i, 7 + i), b"v%d" % i) for i in range(40)]
    raws = _bench_blocks()[:20] + (fm.block_of(entries[:25], 16), fm.block_of(entries[25:], 16))
    assert _max_key(raws) == max_key_len
    for compression in (0, 1):
        _expect(_write(lvkv, gpu, raws, key_format=1, bits=10, compression=compression),
                _model(raws, 1, 10, compression))


@pytest.mark.gpu
def test_round_trip_on_the_device(lvkv, gpu):
    import torch
    raws = _bench_blocks()
    for bits in (10, 0):
        t = _model(raws, 1, bits, 0)
        out = _write(lvkv, gpu, raws, key_format=1, bits=bits, compression=0)
        rep = out[5]
        img = torch.frombuffer(bytearray(out[0][:rep["file_size"]]), dtype=torch.uint8).to(gpu)
        v = lvkv.sst_verify_table(img, filter_policy=lvkv.BLOOM_POLICY if bits else None)[0]
        assert v["status"] == 0 and v["nbad"] == 0 and v["ndata"] == len(raws)
        assert v["has_filter"] == (1 if bits else 0)
        assert (v["index_offset"], v["meta_offset"]) == (rep["index_offset"], rep["meta_offset"])
        assert (v["index_offset"], v["meta_offset"]) == (t.report["index_offset"],
                                                         t.report["meta_offset"])
    t = _model(raws, 1, 10, 1)
    out = _write(lvkv, gpu, raws, key_format=1, bits=10, compression=1)
    rep = out[5]
    assert rep["index_type"] == 1
    img = torch.frombuffer(bytearray(out[0][:rep["file_size"]]), dtype=torch.uint8).to(gpu)
    ho = torch.tensor([rep["index_offset"]], dtype=torch.int64, device=gpu)
    hs = torch.tensor([rep["index_size"]], dtype=torch.int32, device=gpu)
    data, _, ln, st = lvkv.sst_read_blocks(img, ho, hs, max_ulen=len(t.index_contents))
    assert st.tolist() == [0]
    assert bytes(data[:int(ln[0])].cpu().numpy()) == t.index_contents


# ---- damaged blocks ---------------------------------------------------------------

def _entry_offsets(block):
    nr = int.from_bytes(block[-4:], "little")
    limit, p, offs = len(block) - 4 - 4 * nr, 0, []
    while p < limit:
        offs.append(p)
        _, q = fm._get_varint32(block, p, limit)
        ns, q = fm._get_varint32(block, q, limit)
        vl, q = fm._get_varint32(block, q, limit)
        p = q + ns + vl
    return offs


def _sound_batch(key_format):
    tag = (lambda k, i: _ikey(k, 50 + i)) if key_format else (lambda k, i: k)
    return [fm.block_of([(tag(b"key%02d-%03d" % (b, i), i), b"value%d" % i) for i in range(7)], 3)
            for b in range(5)]


def _restart_count(b):
    return b[:-4] + b"\xff\xff\xff\xff"


def _restart_offset(b):
    nr = int.from_bytes(b[-4:], "little")
    at = len(b) - 4 - 4 * nr + 4  # the second restart
    return b[:at] + (len(b) + 100).to_bytes(4, "little") + b[at + 4:]


def _non_shared(b):
    return b[:1] + b"\x7f" + b[2:]


def _endless_varint(b):
    return b"\x80" * 5 + b[5:]


def _shared_too_long(b):
    at = _entry_offsets(b)[1]
    return b[:at] + b"\x64" + b[at + 1:]


def _empty(b):
    return b""


def _short_internal_key(b):
    return fm.block_of([(b"short", b"v")], 16)


DAMAGE = [(_restart_count, 0), (_restart_offset, 0), (_non_shared, 0), (_endless_varint, 0),
          (_shared_too_long, 0), (_empty, 0), (_short_internal_key, 1), (_restart_count, 1),
          (_shared_too_long, 1)]


@pytest.mark.gpu
@pytest.mark.parametrize("damage,key_format", DAMAGE,
                         ids=[f"{d.__name__[1:]}-fmt{k}" for d, k in DAMAGE])
@pytest.mark.parametrize("which", [0, 2, 4])
def test_damaged_block_is_a_verdict(lvkv, gpu, damage, key_format, which):
    blocks = _sound_batch(key_format)
    mkl = _max_key(blocks)
    blocks[which] = damage(blocks[which])
    for compression in (0, 1):
        out = _write(lvkv, gpu, blocks, key_format=key_format, bits=10, compression=compression,
                     max_key_len=mkl)
        rep = out[5]
        assert rep["status"] == lvkv.TABLE_BAD_BLOCK and rep["first_bad_block"] == which
        assert rep["file_size"] == 0
        # the data blocks are the block writer's all the same
        _, handles, types = so.write_blocks(blocks, compression)[0:3]
        assert list(zip(out[1].tolist(), out[2].tolist())) == handles
        assert out[0][:rep["data_end"]] == so.write_blocks(blocks, compression)[0]


@pytest.mark.gpu
def test_key_longer_than_promised(lvkv, gpu):
    blocks = _sound_batch(0)
    blocks[3] = fm.block_of([(b"key03-000", b"v"), (b"key03-001-long", b"v")], 16)
    mkl = len(b"key03-001-long")
    ok = _write(lvkv, gpu, blocks, key_format=0, bits=10, compression=0, max_key_len=mkl)
    _expect(ok, _model(tuple(blocks), 0, 10, 0))
    rep = _write(lvkv, gpu, blocks, key_format=0, bits=10, compression=0, max_key_len=mkl - 1)[5]
    assert rep["status"] == lvkv.TABLE_KEY_TOO_LONG and rep["first_bad_block"] == 3
    assert rep["file_size"] == 0


@pytest.mark.gpu
@pytest.mark.parametrize("compression", [0, 1])
def test_capacity(lvkv, gpu, compression):
    raws = _bench_blocks()[:9]
    t = _model(raws, 1, 10, compression)
    size = len(t.image)
    _expect(_write(lvkv, gpu, raws, key_format=1, bits=10, compression=compression,
                   capacity=size), t)
    # one byte short, and short of each part in turn (the borders are checked in _write)
    for cap in (size - 1, size - 48, t.report["index_offset"] + 3, t.report["meta_offset"],
                t.report["filter_offset"] + 7, t.report["data_end"] - 1, 100, 0):
        rep = _write(lvkv, gpu, raws, key_format=1, bits=10, compression=compression,
                     capacity=cap)[5]
        assert rep["status"] == lvkv.TABLE_CAPACITY and rep["file_size"] == 0, cap


# ---- dirty buffers, two calls in a row ------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("compression", [0, 1, 2])
def test_second_call_on_dirty_buffers(lvkv, gpu, compression):
    """Two calls of different shapes into the same scratch, file, arrays and
    report, back to back on one stream with no synchronisation between them,
    every buffer poisoned before: the second result is a fresh run's."""
    import torch
    L = lvkv.lib
    first, second = _bench_blocks()[:40], _tiny_blocks(300)
    shapes = [(first, 1, 10), (second, 0, 7)]
    mkl = 24
    need = max(L.lvkv_sst_write_table_scratch_bytes(len(b), sum(map(len, b)), 8192, mkl, bits)
               for b, _, bits in shapes)
    cap = max(L.lvkv_sst_table_file_bound(len(b), sum(map(len, b)), mkl, bits)
              for b, _, bits in shapes)
    scratch = torch.full((need + BORDER,), 0xA5, dtype=torch.uint8, device=gpu)
    file = torch.full((cap + BORDER,), 0xA5, dtype=torch.uint8, device=gpu)
    nmax = max(len(b) for b, _, _ in shapes)
    hoff = torch.full((nmax,), -1, dtype=torch.int64, device=gpu)
    hsize = torch.full((nmax,), -1, dtype=torch.int32, device=gpu)
    typ = torch.full((nmax,), 0xA5, dtype=torch.uint8, device=gpu)
    status = torch.full((nmax,), 0xA5, dtype=torch.uint8, device=gpu)
    rep = torch.full((ctypes.sizeof(lvkv.SstTableReport),), 0xA5, dtype=torch.uint8, device=gpu)
    packed = [_pack(torch, gpu, b) for b, _, _ in shapes]
    stream = ctypes.c_void_p(torch.cuda.current_stream(gpu).cuda_stream)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    for (blocks, key_format, bits), (raw, off, ln) in zip(shapes, packed):
        rc = L.lvkv_sst_write_table_device(
            p(raw), p(off), p(ln), len(blocks), compression, 1, 8192, key_format, bits, mkl,
            p(scratch), need, p(file), cap, p(hoff), p(hsize), p(typ), p(status), p(rep), stream)
        assert rc == 0
    torch.cuda.synchronize()
    r = lvkv.SstTableReport.from_buffer_copy(bytes(rep.cpu().numpy())).as_dict()
    n = len(second)
    out = (bytes(file.cpu().numpy()[:cap]), hoff[:n], hsize[:n], typ[:n], status[:n], r)
    _expect(out, _model(second, 0, 7, compression))
    assert (file.cpu().numpy()[cap:] == 0xA5).all() and (scratch.cpu().numpy()[need:] == 0xA5).all()
