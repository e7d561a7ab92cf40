"""The write path for blocks of any size: the device Zstd compressor for
blocks of 20,481-131,072 bytes (one Zstd block a frame, ZSTD_fast: levels
<= 2 except 0) and the block writer with ragged scratch and a per-block
status (lvkv_zstd_compress_big_device, lvkv_sst_write_blocks_status_device).

Every expectation is byte-exact: frames from oracle/zstd_encoder.py, which
test 1 pins to libzstd 1.4.9 driven as port::Zstd_Compress on these very
blocks (tests/golden/gen_zstd_write_big.py), images from
snappy_oracle.write_blocks (TableBuilder::WriteBlock).
"""
from __future__ import annotations

import ctypes
import functools
import hashlib
import json
import subprocess
import sys

import numpy as np
import pytest

import zstd_encoder as ze
import snappy_oracle as so
import zstd_big_inputs as zb
from conftest import GOLDEN, REPO

BIG = 131072


# ---- CPU -----------------------------------------------------------------------

def test_oracle_matches_library_on_large_blocks():
    spec = json.loads((GOLDEN / "zstd_write_big.json").read_text())
    blocks = dict(zb.edge_blocks())
    rows = spec["frames"]
    assert {(r["name"], r["level"]) for r in rows} == {(n, l) for n in blocks for l in zb.LEVELS}
    bad = []
    for r in rows:
        x = blocks[r["name"]]
        assert len(x) == r["input_len"] and hashlib.sha256(x).hexdigest() == r["input_sha256"], \
            f"{r['name']}: the input rebuilt from its seed is not the pinned one"
        f = zb.frame(x, r["level"])
        if len(f) != r["frame_len"] or hashlib.sha256(f).hexdigest() != r["frame_sha256"]:
            bad.append((r["name"], r["level"]))
    assert not bad, f"oracle differs from libzstd 1.4.9 on {bad}"


def test_scratch_does_not_scale_with_blocks_times_max_len(lvkv):
    L = lvkv.lib
    T = 10000 * 4096 + BIG
    f = L.lvkv_sst_write_scratch_bytes_v2
    assert f(20001, 2 * T, BIG) - f(10001, T, BIG) <= 2 * T
    # the old sizing, for contrast: 10,001 slots of 128 KiB
    assert L.lvkv_sst_write_scratch_bytes(10001, BIG) > 10001 * BIG
    assert f(10001, T, BIG) < 2 * T + L.lvkv_zstd_compress_big_scratch_bytes(BIG)
    # the compressor's pool: a function of max_len alone
    g = L.lvkv_zstd_compress_big_scratch_bytes
    assert g(20480) == 0 and g(20481) > 0 and g(65536) > 0 and g(BIG) == g(1 << 30)


def test_validation_without_a_device_call(lvkv):
    """The checks that come before the first HIP call."""
    L = lvkv.lib
    one = ctypes.c_uint64(1)  # stands for any non-null pointer: the checks fail first
    p = ctypes.addressof(one)
    args = lambda level, status: (p, p, p, 1, 2, level, BIG, p, p, 0, p, p, p, p, 1 << 30, status,
                                  None)
    assert L.lvkv_sst_write_blocks_status_device(*args(3, p)) == lvkv.LVKV_ERR_INVALID
    assert L.lvkv_sst_write_blocks_status_device(*args(0, p)) == lvkv.LVKV_ERR_INVALID
    assert L.lvkv_sst_write_blocks_status_device(*args(1, None)) == lvkv.LVKV_ERR_INVALID
    # the compressor: a null or short scratch where a block can need it
    z = lambda max_len, scratch, nbytes: L.lvkv_zstd_compress_big_device(
        p, p, p, p, p, p, p, 1, max_len, 1, scratch, nbytes, None)
    assert z(BIG, None, 0) == lvkv.LVKV_ERR_INVALID
    assert z(BIG, p, L.lvkv_zstd_compress_big_scratch_bytes(BIG) - 1) == lvkv.LVKV_ERR_INVALID
    assert z(20481, None, 0) == lvkv.LVKV_ERR_INVALID


@pytest.fixture(scope="module")
def emu():
    """The kernels compiled for the CPU, once for the tests that run them."""
    r = subprocess.run(["bash", str(REPO / "tools/simt_emu/emu_build.sh")], capture_output=True,
                       text=True)
    assert r.returncode == 0, r.stderr[-3000:]


def test_emulated_kernel_on_edge_blocks(emu):
    """The kernels compiled for the CPU (tools/simt_emu: 64 threads a wave,
    AddressSanitizer and UBSan, the scratch and the input allocated exactly)
    on three edge blocks: a match and a literal run past 65,535, and the
    first size the second kernel takes."""
    r = subprocess.run([sys.executable, str(REPO / "tools/simt_emu/zstdc_check.py"), "big",
                        "long_match,long_literals,bench20481", "1"], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert "3 blocks, 0 differ from the oracle" in r.stdout, r.stdout


@pytest.mark.parametrize("level", [2, -5])
def test_emulated_workgroup_takes_many_blocks(emu, level):
    """One emulated workgroup over zstd_big_inputs.reuse_sequence(): every
    block after the first is compressed in the slot and the LDS its
    predecessor left (longer, shorter, raw-exit, all-zero; blocks of the first
    kernel skipped in between), under AddressSanitizer and UBSan, at the
    levels the edge-block test does not run. The emulator's barriers are real
    ones: this holds the carry-over, not the device's ordering
    (tests/test_codec_reuse_and_bounds.py)."""
    nb = len(zb.reuse_sequence())
    r = subprocess.run([sys.executable, str(REPO / "tools/simt_emu/zstdc_check.py"), "reuse",
                        str(level)], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert f"{nb} blocks, 0 differ from the oracle" in r.stdout, r.stdout
    assert "Sanitizer" not in r.stdout + r.stderr and "runtime error" not in r.stdout + r.stderr, \
        (r.stdout + r.stderr)[-3000:]


def test_emulated_first_kernel_on_the_fixtures(emu):
    """The first kernel alone over every committed input it takes (at most
    20,480 bytes; tests/test_zstd_write.py::test_fixtures_reach_the_rare_paths
    says which paths they reach), at level 1: block_body is the body both
    kernels run, and most of its paths are reached by small blocks only."""
    spec = json.loads((GOLDEN / "zstd_write.json").read_text())
    nb = sum(1 for n in spec["inputs"] if n <= 20480)
    assert nb > 0
    r = subprocess.run([sys.executable, str(REPO / "tools/simt_emu/zstdc_check.py"), "fixtures",
                        "1"], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert f"{nb} blocks, 0 differ from the oracle" in r.stdout, r.stdout
    assert "Sanitizer" not in r.stdout + r.stderr and "runtime error" not in r.stdout + r.stderr, \
        (r.stdout + r.stderr)[-3000:]


# ---- GPU -----------------------------------------------------------------------

def _pack(torch, dev, blobs, skew=0):
    """Blocks one byte apart: every alignment."""
    offs, p = [], skew
    for b in blobs:
        offs.append(p)
        p += len(b) + 1
    buf = np.zeros(max(1, p), dtype=np.uint8)
    for o, b in zip(offs, blobs):
        buf[o:o + len(b)] = np.frombuffer(b, dtype=np.uint8)
    return (torch.from_numpy(buf).to(dev), torch.tensor(offs, dtype=torch.int64, device=dev),
            torch.tensor([len(b) for b in blobs], dtype=torch.int32, device=dev))


def _unpack(dst, offs, lens):
    d = dst.cpu().numpy()
    return [d[o:o + n].tobytes() for o, n in zip(offs.cpu().tolist(), lens.cpu().tolist())]


@pytest.mark.gpu
def test_validation_and_empty_batch(lvkv, gpu):
    """nblocks == 0 comes before every other check; level 3 and a null status
    are LVKV_ERR_INVALID for a batch that has blocks."""
    import torch
    for level in (3, 1):
        file, hoff, hsize, typ, end, st = lvkv.sst_write_blocks_status(
            torch.zeros(1, dtype=torch.uint8, device=gpu),
            torch.zeros(0, dtype=torch.int64, device=gpu),
            torch.zeros(0, dtype=torch.int32, device=gpu), compression=2, zstd_level=level,
            file_offset=321)
        torch.cuda.synchronize()
        assert int(end.item()) == 321 and st.numel() == 0
    end = torch.zeros(1, dtype=torch.int64, device=gpu)
    rc = lvkv.lib.lvkv_sst_write_blocks_status_device(None, None, None, 0, 7, 3, 0, None, None, 99,
                                                      None, None, None, end.data_ptr(), 0, None,
                                                      None)
    torch.cuda.synchronize()
    assert rc == 0 and int(end.item()) == 99
    src, off, ln = _pack(torch, gpu, [b"x" * 100])
    with pytest.raises(RuntimeError):
        lvkv.sst_write_blocks_status(src, off, ln, compression=2, zstd_level=3)


@pytest.mark.gpu
@pytest.mark.parametrize("level", [1, 2, -1, -5])
def test_edge_blocks(lvkv, gpu, level):
    import torch
    names, blobs = zip(*zb.edge_blocks())
    src, off, ln = _pack(torch, gpu, blobs, skew=3)
    dst, doff, dlen, st = lvkv.zstd_compress_big(src, off, ln, level=level, max_len=BIG)
    torch.cuda.synchronize()
    assert st.cpu().tolist() == [lvkv.ZSTD_OK] * len(blobs)
    got = _unpack(dst, doff, dlen)
    bad = [n for n, x, g in zip(names, blobs, got) if g != zb.frame(x, level)]
    assert not bad, f"level {level}: device frame differs from the oracle on {bad}"
    # the blocks of the first kernel: the bytes zstd_compress gives
    small = [k for k, x in enumerate(blobs) if len(x) <= lvkv.ZSTD_COMPRESS_MAX_BLOCK]
    assert len(small) == 4
    s2, o2, l2 = _pack(torch, gpu, [blobs[k] for k in small], skew=3)
    d2, do2, dl2, st2 = lvkv.zstd_compress(s2, o2, l2, level=level, max_len=20480)
    torch.cuda.synchronize()
    assert _unpack(d2, do2, dl2) == [got[k] for k in small]


@pytest.mark.gpu
def test_edge_statuses(lvkv, gpu):
    import torch
    b = zb.bench()
    blobs = [b[:BIG + 1], b[:BIG], b[:4096], b[:30000]]
    src, off, ln = _pack(torch, gpu, blobs, skew=3)
    for level in (1, 2):  # (level 2 is not ZSTD_fast past 128 KiB: still TOO_LARGE here)
        dst, doff, dlen, st = lvkv.zstd_compress_big(src, off, ln, level=level, max_len=1 << 30)
        torch.cuda.synchronize()
        assert st.cpu().tolist() == [lvkv.ZSTD_TOO_LARGE] + [lvkv.ZSTD_OK] * 3
        assert _unpack(dst, doff, dlen)[1:] == [zb.frame(x, level) for x in blobs[1:]]
    # max_len below the kernel's own bound
    _, _, _, st = lvkv.zstd_compress_big(src, off, ln, level=1, max_len=30000)
    torch.cuda.synchronize()
    assert st.cpu().tolist() == [lvkv.ZSTD_TOO_LARGE, lvkv.ZSTD_TOO_LARGE, lvkv.ZSTD_OK,
                                 lvkv.ZSTD_OK]
    for level in (3, 0, 19):
        _, _, _, st = lvkv.zstd_compress_big(src, off, ln, level=level, max_len=BIG)
        torch.cuda.synchronize()
        assert set(st.cpu().tolist()) == {lvkv.ZSTD_UNSUPPORTED}


@pytest.mark.gpu
def test_no_dependence_on_neighbouring_bytes(lvkv, gpu):
    """The same block followed by 0x00s and by 0xFFs, and once more ending
    the tensor: the same frame, the oracle's."""
    import torch
    x = zb.bench()[:70001]
    n = len(x)
    buf = np.zeros(3 + (n + 64) * 2 + n, dtype=np.uint8)
    offs = [3, 3 + n + 64, 3 + 2 * (n + 64)]
    for o in offs:
        buf[o:o + n] = np.frombuffer(x, dtype=np.uint8)
    buf[offs[1] + n: offs[1] + n + 64] = 0xFF
    assert offs[2] + n == buf.size
    src = torch.from_numpy(buf).to(gpu)
    off = torch.tensor(offs, dtype=torch.int64, device=gpu)
    ln = torch.tensor([n] * 3, dtype=torch.int32, device=gpu)
    for level in (1, -1):
        dst, doff, dlen, st = lvkv.zstd_compress_big(src, off, ln, level=level, max_len=BIG)
        torch.cuda.synchronize()
        assert st.cpu().tolist() == [lvkv.ZSTD_OK] * 3
        got = _unpack(dst, doff, dlen)
        assert got[0] == got[1] == got[2] == zb.frame(x, level)


@functools.lru_cache(maxsize=1)
def _ragged_blocks():
    """24 blocks for level 1, 8 each for 2, -1, -5: one draw from one stream."""
    rng = np.random.default_rng(7)
    return {level: zb.fuzz_inputs(rng, count, 20481, BIG)
            for level, count in [(1, 24), (2, 8), (-1, 8), (-5, 8)]}


@pytest.mark.gpu
@pytest.mark.parametrize("level", [1, 2, -1, -5])
def test_ragged_batch(lvkv, gpu, level):
    import torch
    blobs = _ragged_blocks()[level]
    count = len(blobs)
    src, off, ln = _pack(torch, gpu, blobs, skew=1)
    dst, doff, dlen, st = lvkv.zstd_compress_big(src, off, ln, level=level, max_len=BIG)
    torch.cuda.synchronize()
    assert st.cpu().tolist() == [lvkv.ZSTD_OK] * count
    got = _unpack(dst, doff, dlen)
    bad = [(k, len(x)) for k, (x, g) in enumerate(zip(blobs, got)) if g != ze.compress(x, level)]
    assert not bad, f"level {level}: device frame differs from the oracle on {bad}"
    # the device decoder reads them back
    s2, o2, l2 = _pack(torch, gpu, got)
    caps = torch.tensor([len(x) for x in blobs], dtype=torch.int32, device=gpu)
    ooff = torch.tensor(np.concatenate([[0], np.cumsum([len(x) for x in blobs])[:-1]]),
                        dtype=torch.int64, device=gpu)
    out = torch.empty(sum(len(x) for x in blobs), dtype=torch.uint8, device=gpu)
    out, ooff, olen, st2 = lvkv.zstd_uncompress(s2, o2, l2, max_ulen=lvkv.ZSTD_MAX_BLOCK,
                                                dst=out, dst_offsets=ooff, dst_caps=caps)
    torch.cuda.synchronize()
    assert st2.cpu().tolist() == [lvkv.ZSTD_OK] * count
    assert _unpack(out, ooff, olen) == blobs


def _writer_raws():
    b = zb.bench()
    rng = np.random.default_rng(7)

    def rand(n):
        return rng.integers(0, 256, n, dtype=np.uint8).tobytes()

    r3000 = rand(3000)
    straddler = rng.integers(0, 256, 40000, dtype=np.uint8)
    straddler[: 40000 // 7] = 7
    mixed = b[:30000] + rand(66000) + b[:30000]
    return [b[:5000], b[7:70007], b[100:4196], b[:65536], b[:30000], r3000, b"", b[:BIG],
            straddler.tobytes(), bytes(100000), mixed, zb.edge("skewed")]


def _read_back(lvkv, torch, gpu, file, hoff, hsize, raws):
    caps = torch.tensor([max(1, len(x)) for x in raws], dtype=torch.int32, device=gpu)
    ooff = torch.tensor(np.concatenate([[0], np.cumsum([max(1, len(x)) for x in raws])[:-1]]),
                        dtype=torch.int64, device=gpu)
    out = torch.empty(int(caps.sum().item()), dtype=torch.uint8, device=gpu)
    out, ooff, olen, st = lvkv.sst_read_blocks(file, hoff, hsize, max_ulen=lvkv.SNAPPY_MAX_BLOCK,
                                               out=out, out_offsets=ooff, out_caps=caps)
    torch.cuda.synchronize()
    assert st.cpu().tolist() == [lvkv.READ_OK] * len(raws)
    assert _unpack(out, ooff, olen) == raws


@pytest.mark.gpu
@pytest.mark.parametrize("compression,level,file_offset",
                         [(1, 1, 0), (2, 1, 777), (2, 2, 0), (2, -1, 5), (0, 1, 17)])
def test_writer_image(lvkv, gpu, compression, level, file_offset):
    """A 70 KB snappy block and 30-128 KiB zstd blocks give the oracle's
    WriteBlock image."""
    import torch
    raws = _writer_raws()
    src, off, ln = _pack(torch, gpu, raws, skew=1)
    file, hoff, hsize, typ, end, st = lvkv.sst_write_blocks_status(
        src, off, ln, compression=compression, zstd_level=level, max_len=BIG,
        file_offset=file_offset)
    torch.cuda.synchronize()
    img, handles, types = so.write_blocks(raws, compression, file_offset, zstd_level=level)
    if compression == 1:
        assert types == [1, 1, 1, 1, 1, 0, 0, 1, 1, 1, 0, 1]
    elif compression == 2 and level == 1:
        assert types == [2, 2, 2, 2, 2, 0, 0, 2, 2, 2, 2, 2]
    assert st.cpu().tolist() == [lvkv.ZSTD_OK] * len(raws)
    assert typ.cpu().tolist() == types
    assert hoff.cpu().tolist() == [h[0] for h in handles]
    assert hsize.cpu().tolist() == [h[1] for h in handles]
    assert int(end.item()) == file_offset + len(img)
    assert file.cpu().numpy()[file_offset:file_offset + len(img)].tobytes() == img
    _read_back(lvkv, torch, gpu, file, hoff, hsize, raws)


@pytest.mark.gpu
def test_reported_raw_block(lvkv, gpu):
    """A zstd block past 128 KiB is written raw and says so."""
    import torch
    b = zb.bench()
    raws = [b[:5000], b[:BIG + 1], b[:4096]]
    src, off, ln = _pack(torch, gpu, raws, skew=1)
    file, hoff, hsize, typ, end, st = lvkv.sst_write_blocks_status(src, off, ln, compression=2,
                                                                   zstd_level=1, max_len=1 << 20)
    torch.cuda.synchronize()
    assert st.cpu().tolist() == [lvkv.ZSTD_OK, lvkv.ZSTD_TOO_LARGE, lvkv.ZSTD_OK]
    assert typ.cpu().tolist() == [2, 0, 2]
    img = file.cpu().numpy()
    for k in (0, 2):
        o, n = int(hoff[k].item()), int(hsize[k].item())
        assert img[o:o + n].tobytes() == zb.frame(raws[k], 1)
    _read_back(lvkv, torch, gpu, file, hoff, hsize, raws)


@pytest.mark.gpu
def test_scratch_too_small_for_a_block_is_reported(lvkv, gpu):
    """A caller whose total was too small: the blocks without room are
    written raw and reported, nothing lands past the scratch."""
    import torch
    b = zb.bench()
    raws = [b[:4096], b[:8000], b[:4096]]
    src, off, ln = _pack(torch, gpu, raws)
    n = len(raws)
    L = lvkv.lib
    # room for the first block's slot only, then a canary
    need = int(L.lvkv_sst_write_scratch_bytes_v2(n, 4096, 0))
    scratch = torch.full((need + 4096,), 0xAB, dtype=torch.uint8, device=gpu)
    file = torch.zeros(sum(map(len, raws)) + 5 * n, dtype=torch.uint8, device=gpu)
    hoff = torch.empty(n, dtype=torch.int64, device=gpu)
    hsize = torch.empty(n, dtype=torch.int32, device=gpu)
    typ = torch.empty(n, dtype=torch.uint8, device=gpu)
    st = torch.empty(n, dtype=torch.uint8, device=gpu)
    end = torch.empty(1, dtype=torch.int64, device=gpu)
    rc = L.lvkv_sst_write_blocks_status_device(
        src.data_ptr(), off.data_ptr(), ln.data_ptr(), n, 1, 1, 0, scratch.data_ptr(),
        file.data_ptr(), 0, hoff.data_ptr(), hsize.data_ptr(), typ.data_ptr(), end.data_ptr(),
        need, st.data_ptr(), None)
    torch.cuda.synchronize()
    assert rc == 0
    assert st.cpu().tolist()[0] == lvkv.ZSTD_OK and typ.cpu().tolist()[0] == 1
    assert st.cpu().tolist()[1] == lvkv.ZSTD_TOO_LARGE and typ.cpu().tolist()[1] == 0
    assert (scratch[need:] == 0xAB).all().item()
    _read_back(lvkv, torch, gpu, file, hoff, hsize, raws)


N_PASSES = 4101  # past the slots scan's pass (1,024 blocks) and the layout scan's (4,096)


@functools.lru_cache(maxsize=1)
def _many_small_raws():
    """4,101 blocks of 0-96 bytes: odd indices random bytes (kept raw), even
    ones a repeated byte (compressed)."""
    rng = np.random.default_rng(4101)
    out = []
    for k in range(N_PASSES):
        n = int(rng.integers(0, 97))
        if k % 2:
            out.append(rng.integers(0, 256, n, dtype=np.uint8).tobytes())
        else:
            out.append(bytes([int(rng.integers(0, 256))]) * n)
    return out


@functools.lru_cache(maxsize=None)
def _many_small_image(compression):
    return so.write_blocks(_many_small_raws(), compression, 123, zstd_level=1)


@pytest.mark.gpu
@pytest.mark.parametrize("compression", [0, 1, 2])
@pytest.mark.parametrize("with_status", [False, True])
def test_writer_image_across_scan_passes(lvkv, gpu, with_status, compression):
    """Both writers on a batch that takes the slots scan through five passes
    and the layout scan through two: the carry from pass to pass puts every
    handle where WriteBlock does, for raw and compressed blocks on both sides
    of both boundaries."""
    import torch
    raws = _many_small_raws()
    img, handles, types = _many_small_image(compression)
    if compression:
        for lo, hi in [(0, 1024), (1024, 4096), (4096, N_PASSES)]:
            assert set(types[lo:hi]) == {0, compression}
    src, off, ln = _pack(torch, gpu, raws, skew=1)
    if with_status:
        file, hoff, hsize, typ, end, st = lvkv.sst_write_blocks_status(
            src, off, ln, compression=compression, zstd_level=1, file_offset=123)
    else:
        file, hoff, hsize, typ, end = lvkv.sst_write_blocks(
            src, off, ln, compression=compression, zstd_level=1, file_offset=123)
    torch.cuda.synchronize()
    if with_status:
        assert st.cpu().tolist() == [lvkv.ZSTD_OK] * len(raws)
    assert typ.cpu().tolist() == types
    assert hoff.cpu().tolist() == [h[0] for h in handles]
    assert hsize.cpu().tolist() == [h[1] for h in handles]
    assert int(end.item()) == 123 + len(img)
    assert file.cpu().numpy()[123:123 + len(img)].tobytes() == img
