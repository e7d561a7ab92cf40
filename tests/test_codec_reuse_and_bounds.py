"""What one work item of the codecs leaves behind for, or does to, its
neighbours: reuse and bounds.

Reuse. zstd_compress_big_kernel is a persistent grid of at most
2 * kBigCus = 512 workgroups (csrc/lvkv_zstd_compress.hip, zstd_big_grid);
each pulls block indices off a counter and reuses its HBM slot and its LDS
from block to block. Section A hands it more than twice that many big
blocks, so that most are compressed by a workgroup that has compressed
another one before, and a second call on the same dirty scratch. Section B
hands the block writers a scratch a different batch left dirty, through the
C ABI as a C caller does.

Bounds. Every destination here lies in one allocation between borders of a
fill byte, at every alignment, and the tensor ends with 1 MiB of it
(_gapped): a kernel that writes outside its room fails an assertion instead
of corrupting a neighbour or faulting. Section C gives the HBM-output
decoders streams whose header claims fewer bytes than they decode to;
section D gives the compressors exactly their bound.

Every expectation is an oracle's (oracle/zstd_encoder.py,
oracle/zstd_oracle.py, oracle/snappy_oracle.py). Their cost, measured on one
core of the build machine: 12.5 s for the frames of section A's five cases
together (4.9 s the dearest, level 1 at 128 KiB; 3.0 s of that are the edge
blocks' frames, which test_edge_blocks needs anyway and finds in
zstd_big_inputs.frame's cache), 1.8 s for section B's images, 8.7 s for the
verdicts on section C's 128 zstd streams (0.11 s an intact 64 KiB one, computed
once for both max_ulen cases and the ReadBlock test) and 0.5 s for its 136
snappy streams. On the MI355X host every test here took under 2.5 s.
"""
from __future__ import annotations

import functools
import json

import numpy as np
import pytest

import snappy_oracle as so
import zstd_big_inputs as zb
import zstd_oracle as zo
from conftest import GOLDEN

BIG = 131072
TAIL = 1 << 20


# ---- destinations between borders ------------------------------------------------

def _gapped(torch, dev, rooms, gap=256, fill=0xC3):
    """One tensor of destinations of rooms[i] bytes, `gap` bytes of `fill`
    before and after each, start offsets going through every alignment mod 4,
    a 1 MiB tail of `fill`. Returns (tensor, offsets, check); check() raises
    when a byte outside the rooms is no longer `fill`, naming the destination
    the first such byte belongs to and how far outside it lies."""
    offs, p = [], 0
    for i, r in enumerate(rooms):
        p += gap
        p += (i - p) % 4
        offs.append(p)
        p += int(r)
    total = p + gap + TAIL
    buf = torch.full((total,), fill, dtype=torch.uint8, device=dev)

    def check(host=None, what=""):
        h = buf.cpu().numpy() if host is None else host
        assert h.size == total
        prev = 0
        for i in range(len(rooms) + 1):
            hi = offs[i] if i < len(rooms) else total
            seg = h[prev:hi]
            if seg.size and (seg != fill).any():
                j = prev + int(np.argmax(seg != fill))
                past, before = j - prev, hi - j
                if i == len(rooms) or (i > 0 and past < before):
                    where = f"{past + 1} byte(s) past the end of destination {i - 1}"
                else:
                    where = f"{before} byte(s) before destination {i}"
                raise AssertionError(f"{what}: byte {j} is {int(h[j]):#x}, not the border's "
                                     f"{fill:#x}: a write {where}")
            if i < len(rooms):
                prev = offs[i] + int(rooms[i])

    return buf, offs, check


def test_gapped_checker_names_the_destination():
    """The helper itself: intact borders pass whatever the rooms hold; a byte
    past a room and a byte before one are reported with the right index."""
    import torch
    cpu = torch.device("cpu")
    rooms = [10, 0, 7, 4096, 33]
    buf, offs, check = _gapped(torch, cpu, rooms)
    assert [o % 4 for o in offs] == [0, 1, 2, 3, 0]
    assert buf.numel() >= offs[-1] + rooms[-1] + TAIL
    for o, r in zip(offs, rooms):
        buf[o:o + r] = 0x11
    check()
    buf[offs[2] + rooms[2]] = 0
    with pytest.raises(AssertionError, match=r"1 byte\(s\) past the end of destination 2"):
        check()
    buf[offs[2] + rooms[2]] = 0xC3
    buf[offs[3] - 1] = 0
    with pytest.raises(AssertionError, match=r"1 byte\(s\) before destination 3"):
        check()
    buf[offs[3] - 1] = 0xC3
    buf[offs[1]] = 0xC2  # (a room of no bytes owns none)
    with pytest.raises(AssertionError, match=r"destination 1"):
        check()
    buf[offs[1]] = 0xC3
    buf[-1] = 0
    with pytest.raises(AssertionError, match=r"past the end of destination 4"):
        check()
    buf[-1] = 0xC3
    check()


def _pack(torch, dev, blobs, skew=0):
    """Inputs one byte apart: every alignment."""
    offs, p = [], skew
    for b in blobs:
        offs.append(p)
        p += len(b) + 1
    buf = np.zeros(max(1, p), dtype=np.uint8)
    for o, b in zip(offs, blobs):
        buf[o:o + len(b)] = np.frombuffer(b, dtype=np.uint8)
    return torch.from_numpy(buf).to(dev), offs, [len(b) for b in blobs]


def _i64(torch, dev, v):
    return torch.tensor(list(v), dtype=torch.int64, device=dev)


def _i32(torch, dev, v):
    return torch.tensor(list(v), dtype=torch.int32, device=dev)


# ---- A. more big blocks than workgroups ----------------------------------------

MAX_GRID = 512  # 2 * kBigCus (csrc/lvkv_zstd_compress.hip): the persistent grid's bound
N_BIG = 1100


@functools.lru_cache(maxsize=None)
def _reuse_batch(max_len):
    """[(name, bytes)] for section A at this cap. The first 512 entries are
    the largest blocks the cap allows, so that every workgroup's later blocks
    follow a maximal one; then seeded draws from the whole pool until 1,100
    entries in all are the second kernel's, with riders for the loop's skip
    paths (counted from the end of the head): every 7th a block of the first
    kernel, every 53rd a block one byte over the cap."""
    pool = zb.reuse_pool()
    b = zb.bench()
    head = [(f"bench{n}", b[:n]) for n in (max_len - 1, max_len)]
    assert all(dict(pool)[n] == x for n, x in head)
    small = [(n, zb.edge(n)) for n in ("empty", "abc", "bench4096", "bench20480")]
    over = (f"bench{max_len + 1}", b[:max_len + 1])
    out = [head[k % 2] for k in range(MAX_GRID)]
    rng = np.random.default_rng(max_len)
    nbig = MAX_GRID
    k = 0
    while nbig < N_BIG + 4:
        k += 1
        if k % 53 == 0:
            e = over
        elif k % 7 == 0:
            e = small[(k // 7) % 4]
        else:
            e = pool[int(rng.integers(0, len(pool)))]
        out.append(e)
        nbig += 20480 < len(e[1]) <= max_len
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("level,max_len",
                         [(1, BIG), (2, BIG), (-5, BIG), (1, 65536), (-1, 65536)])
def test_more_big_blocks_than_workgroups(lvkv, gpu, level, max_len):
    """At least 1,100 blocks of the second kernel in one call: the grid is at
    most 512 workgroups, so at least 588 of them are compressed in a slot and
    an LDS that already held another block (a maximal one first, so stale
    literals, sequences, codes and table entries lie past the new lengths).
    Then the same blocks in reverse on the same stream, no synchronize, the
    same scratch: the counter and the pool are reused dirty and each workgroup
    sees another (previous, current) pairing. Frames are the oracle's, byte
    for byte; rooms are lvkv_zstd_compress_bound, between borders."""
    import torch
    batch = _reuse_batch(max_len)
    names, blobs = zip(*batch)
    n = len(blobs)
    big = [20480 < len(x) <= max_len for x in blobs]
    assert sum(big) >= N_BIG and sum(big) - MAX_GRID >= 588
    assert all(big[:MAX_GRID]) and all(len(x) >= max_len - 1 for x in blobs[:MAX_GRID])
    want_st = [lvkv.ZSTD_TOO_LARGE if len(x) > max_len else lvkv.ZSTD_OK for x in blobs]
    assert want_st.count(lvkv.ZSTD_TOO_LARGE) >= 10 and sum(len(x) <= 20480 for x in blobs) >= 50
    want = [zb.frame(x, level) if s == lvkv.ZSTD_OK else None for x, s in zip(blobs, want_st)]

    src, soff, slen = _pack(torch, gpu, blobs, skew=3)
    rooms = [lvkv.zstd_compress_bound(len(x)) for x in blobs]
    need = lvkv.zstd_compress_big_scratch_bytes(max_len)
    assert need > 0
    scratch = torch.full((need,), 0xFF, dtype=torch.uint8, device=gpu)
    runs = []
    for order in (list(range(n)), list(range(n - 1, -1, -1))):
        dst, doff, check = _gapped(torch, gpu, [rooms[k] for k in order])
        _, _, dlen, st = lvkv.zstd_compress_big(
            src, _i64(torch, gpu, (soff[k] for k in order)),
            _i32(torch, gpu, (slen[k] for k in order)), level=level, max_len=max_len, dst=dst,
            dst_offsets=_i64(torch, gpu, doff), scratch=scratch)
        runs.append((order, dst, doff, check, dlen, st))
    torch.cuda.synchronize()
    for call, (order, dst, doff, check, dlen, st) in enumerate(runs):
        what = f"level {level}, max_len {max_len}, call {call}"
        st, dlen, h = st.cpu().tolist(), dlen.cpu().tolist(), dst.cpu().numpy()
        bad_st = [(j, names[k], st[j], want_st[k]) for j, k in enumerate(order)
                  if st[j] != want_st[k]]
        assert not bad_st, f"{what}: {len(bad_st)} statuses differ (entry, block, got, want): " \
                           f"{bad_st[:6]}"
        bad = [(j, names[k], len(blobs[k])) for j, k in enumerate(order) if want[k] is not None
               and h[doff[j]:doff[j] + dlen[j]].tobytes() != want[k]]
        assert not bad, f"{what}: {len(bad)} frames differ from the oracle (entry, block, " \
                        f"length): {bad[:6]}"
        check(h, what)


# ---- B. the writers on a reused scratch, with borders ---------------------------

@functools.lru_cache(maxsize=None)
def _snappy(x: bytes) -> bytes:
    return so.compress(x)


def _expected_image(lvkv, raws, compression, level, max_len, file_offset):
    """TableBuilder::WriteBlock's rule over cached compressed forms: (image,
    handles, types, statuses). A zstd block past min(max_len, 128 KiB) is the
    device's TOO_LARGE: raw, type 0."""
    crc = so._crc()
    out = bytearray()
    handles, types, status = [], [], []
    for raw in raws:
        contents, typ, st = raw, 0, lvkv.ZSTD_OK
        if compression == 2 and len(raw) > min(max_len, BIG):
            st = lvkv.ZSTD_TOO_LARGE
        elif compression:
            c = _snappy(raw) if compression == 1 else zb.frame(raw, level)
            if len(c) < len(raw) - len(raw) // 8:
                contents, typ = c, compression
        handles.append((file_offset + len(out), len(contents)))
        types.append(typ)
        status.append(st)
        out += contents
        out.append(typ)
        out += crc.mask(crc.extend(crc.value(contents), bytes([typ]))).to_bytes(4, "little")
    return bytes(out), handles, types, status


@functools.lru_cache(maxsize=1)
def _writer_batches():
    """Batch 1 (zstd, about 700 blocks) and batch 2 (snappy, shorter, other
    blocks) of test_writer_reuses_a_dirty_scratch."""
    b = zb.bench()
    rng = np.random.default_rng(17)

    def rand(n):
        return rng.integers(0, 256, n, dtype=np.uint8).tobytes()

    mid = [x for _, x in zb.reuse_pool() if len(x) <= 40000]
    assert len(mid) == 27
    small = [b[s:s + n] for s, n in [(0, 4096), (4096, 4096), (100, 100), (9000, 1), (5, 8191),
                                     (12288, 2048), (333, 777), (20000, 6000), (1, 15), (7, 16)]]
    raw = [rand(n) for n in (3000, 17, 4096, 25000)]
    # the first 40 (re-compressed by so.write_blocks to pin the assembly): cheap ones
    first = [mid[0], mid[5]] + small * 3 + raw[:3] + [b"", mid[13], small[0], small[4], raw[1],
                                                      small[2]]
    assert len(first) == 41
    rest = [mid[int(rng.integers(0, 27))] for _ in range(298)]
    rest += [small[int(rng.integers(0, 10))] for _ in range(320)]
    rest += [raw[int(rng.integers(0, 4))] for _ in range(40)]
    rest.append(b[:BIG + 1])
    rest = [rest[k] for k in rng.permutation(len(rest))]
    one = first + rest
    two = [b[50:70050], b[11:30011], rand(5000), b""] + \
          [b[int(s):int(s) + int(n)] for s, n in zip(rng.integers(0, 100000, 12),
                                                     rng.integers(0, 8192, 12))]
    two = [two[int(rng.integers(0, len(two)))] for _ in range(180)] + two
    return one, two


_SPARE = {"hoff": -0x0101010101010102, "hsize": -0x01010102, "typ": 0xEE, "st": 0xEE,
          "end": -0x0101010101010102}


def _writer_outputs(torch, dev, n, total_raw, file_offset):
    """The outputs of one writer call: the image prefilled with 0xCD and a
    1 MiB tail, every per-block array with 8 spare entries of its canary."""
    return dict(
        file=torch.full((file_offset + total_raw + 5 * n + TAIL,), 0xCD, dtype=torch.uint8,
                        device=dev),
        hoff=torch.full((n + 8,), _SPARE["hoff"], dtype=torch.int64, device=dev),
        hsize=torch.full((n + 8,), _SPARE["hsize"], dtype=torch.int32, device=dev),
        typ=torch.full((n + 8,), _SPARE["typ"], dtype=torch.uint8, device=dev),
        st=torch.full((n + 8,), _SPARE["st"], dtype=torch.uint8, device=dev),
        end=torch.full((1 + 8,), _SPARE["end"], dtype=torch.int64, device=dev))


def _check_writer(lvkv, o, n, file_offset, want, what, with_status=True):
    img, handles, types, status = want
    assert int(o["end"][0].item()) == file_offset + len(img), what
    if with_status:
        assert o["st"][:n].cpu().tolist() == status, what
    assert o["typ"][:n].cpu().tolist() == types, what
    assert o["hoff"][:n].cpu().tolist() == [h[0] for h in handles], what
    assert o["hsize"][:n].cpu().tolist() == [h[1] for h in handles], what
    f = o["file"].cpu().numpy()
    got = f[file_offset:file_offset + len(img)]
    if got.tobytes() != img:
        j = int(np.argmax(got != np.frombuffer(img, dtype=np.uint8)))
        k = max(i for i, h in enumerate(handles) if h[0] - file_offset <= j)
        raise AssertionError(f"{what}: the image differs from WriteBlock's at byte {j} (block {k}, "
                             f"{handles[k][1]} bytes, type {types[k]})")
    assert (f[:file_offset] == 0xCD).all(), f"{what}: a write before file_offset"
    after = f[file_offset + len(img):]
    assert (after == 0xCD).all(), \
        f"{what}: a write {int(np.argmax(after != 0xCD)) + 1} byte(s) past the image's end"
    for name, canary in _SPARE.items():
        spare = o[name][(1 if name == "end" else n):].cpu().tolist()
        assert spare == [canary] * 8, f"{what}: a write past the entries of {name}"
    if not with_status:
        assert o["st"].cpu().tolist() == [0xEE] * (n + 8), what
    return f[:file_offset + len(img)].tobytes()


@pytest.mark.gpu
def test_writer_reuses_a_dirty_scratch(lvkv, gpu):
    """lvkv_sst_write_blocks_status_device three times on one stream, no
    synchronize, one scratch filled with 0xFF: a zstd batch (blocks of the
    second compress kernel, small ones, raw-kept ones, an empty one and one
    past 128 KiB), a shorter snappy batch of other blocks, the first batch
    again. Each image is WriteBlock's, nothing outside [file_offset, end) or
    past an output array's entries is touched, images 1 and 3 are equal."""
    import torch
    L = lvkv.lib
    one, two = _writer_batches()
    calls = [(one, 2, 1, BIG, 777), (two, 1, 1, 0, 12345), (one, 2, 1, BIG, 9)]
    wants = [_expected_image(lvkv, raws, comp, lvl, ml, fo) for raws, comp, lvl, ml, fo in calls]
    # the assembly above is snappy_oracle.write_blocks': pinned on the first 40 blocks
    img40, h40, t40 = so.write_blocks(one[:40], 2, 777, zstd_level=1)
    assert wants[0][0][:len(img40)] == img40 and wants[0][1][:40] == h40 and wants[0][2][:40] == t40
    assert {0, 2} <= set(t40)
    assert wants[0][3].count(lvkv.ZSTD_TOO_LARGE) == 1 and set(wants[1][2]) == {0, 1}
    assert sum(20480 < len(x) <= BIG for x in one) >= 300

    need = max(int(L.lvkv_sst_write_scratch_bytes_v2(len(one), sum(map(len, one)), BIG)),
               int(L.lvkv_sst_write_scratch_bytes_v2(len(two), sum(map(len, two)), 0)))
    scratch = torch.full((need + 4096,), 0xFF, dtype=torch.uint8, device=gpu)
    scratch[need:] = 0xAB
    packed = {id(one): _pack(torch, gpu, one, skew=1), id(two): _pack(torch, gpu, two, skew=2)}
    ins = {k: (s, _i64(torch, gpu, o), _i32(torch, gpu, ln)) for k, (s, o, ln) in packed.items()}
    outs = [_writer_outputs(torch, gpu, len(raws), sum(map(len, raws)), fo)
            for raws, _, _, _, fo in calls]
    stream = torch.cuda.current_stream(gpu).cuda_stream
    for (raws, comp, lvl, ml, fo), o in zip(calls, outs):
        src, off, ln = ins[id(raws)]
        rc = L.lvkv_sst_write_blocks_status_device(
            src.data_ptr(), off.data_ptr(), ln.data_ptr(), len(raws), comp, lvl, ml,
            scratch.data_ptr(), o["file"].data_ptr(), fo, o["hoff"].data_ptr(),
            o["hsize"].data_ptr(), o["typ"].data_ptr(), o["end"].data_ptr(), need,
            o["st"].data_ptr(), stream)
        assert rc == 0
    torch.cuda.synchronize()
    imgs = [_check_writer(lvkv, o, len(c[0]), c[4], w, f"call {k + 1}")
            for k, (c, o, w) in enumerate(zip(calls, outs, wants))]
    assert imgs[0][777:] == imgs[2][9:]
    assert (scratch[need:] == 0xAB).all().item(), "a write past the scratch"


@pytest.mark.gpu
def test_strided_writer_reuses_a_dirty_scratch(lvkv, gpu):
    """lvkv_sst_write_blocks_level_device and its nblocks x stride scratch:
    300 blocks of 0-8,192 bytes, snappy and then zstd (max_len 20480) on one
    scratch filled with 0xFF, one stream, no synchronize."""
    import torch
    import test_zstd_write as tzw
    L = lvkv.lib
    raws = tzw._fuzz_inputs(np.random.default_rng(23), 300, 8193)
    raws[0], raws[1] = raws[0][:0], zb.bench()[:8192]
    n = len(raws)
    calls = [(1, 8192, 4321), (2, 20480, 1)]
    wants = []
    for comp, _, fo in calls:
        img, handles, types = so.write_blocks(raws, comp, fo, zstd_level=1)
        assert set(types) == {0, comp}
        wants.append((img, handles, types, None))
    need = max(int(L.lvkv_sst_write_scratch_bytes(n, ml)) for _, ml, _ in calls)
    scratch = torch.full((need + 4096,), 0xFF, dtype=torch.uint8, device=gpu)
    scratch[need:] = 0xAB
    src, off, ln = _pack(torch, gpu, raws, skew=1)
    off, ln = _i64(torch, gpu, off), _i32(torch, gpu, ln)
    outs = [_writer_outputs(torch, gpu, n, sum(map(len, raws)), fo) for _, _, fo in calls]
    stream = torch.cuda.current_stream(gpu).cuda_stream
    for (comp, ml, fo), o in zip(calls, outs):
        rc = L.lvkv_sst_write_blocks_level_device(
            src.data_ptr(), off.data_ptr(), ln.data_ptr(), n, comp, 1, ml, scratch.data_ptr(),
            o["file"].data_ptr(), fo, o["hoff"].data_ptr(), o["hsize"].data_ptr(),
            o["typ"].data_ptr(), o["end"].data_ptr(), stream)
        assert rc == 0
    torch.cuda.synchronize()
    for k, (c, o, w) in enumerate(zip(calls, outs, wants)):
        _check_writer(lvkv, o, n, c[2], w, f"call {k + 1} (compression {c[0]})", with_status=False)
    assert (scratch[need:] == 0xAB).all().item(), "a write past the scratch"


# ---- C. decoders: damaged big streams stay inside their destination -------------

def _split(blob: bytes, lengths):
    out, p = [], 0
    for n in lengths:
        out.append(blob[p:p + n])
        p += n
    assert p == len(blob)
    return out


def _zstd_claim(f: bytes, n: int) -> bytes:
    """Frame f with its content-size field rewritten to n."""
    h = zo.frame_header(f)
    fcs = [1 if (f[4] >> 5) & 1 else 0, 2, 4, 8][f[4] >> 6]
    assert fcs and zo.frame_header(f).content_size != n
    v = n - 256 if fcs == 2 else n
    assert 0 <= v < 1 << (8 * fcs)
    g = f[:h.size - fcs] + v.to_bytes(fcs, "little") + f[h.size:]
    assert zo.frame_header(g).content_size == n
    return g


def _snappy_claim(s: bytes, n: int) -> bytes:
    """Stream s with its varint preamble rewritten to n."""
    g = so._varint32(n) + s[so._preamble_len(s):]
    assert so.uncompressed_length(g) == n
    return g


def _damage(rng, base, count):
    """1-3 bytes flipped or replaced in the second half, and cuts."""
    out = []
    for k in range(count):
        d = bytearray(base[k % len(base)])
        if k % 6 == 5:
            keep = rng.integers(1, len(d)) if k % 12 == 5 else len(d) - rng.integers(1, 200)
            out.append(bytes(d[:int(keep)]))
            continue
        for _ in range(int(rng.integers(1, 4))):
            j = int(rng.integers(len(d) // 2, len(d)))
            d[j] = int(rng.integers(0, 256)) if k % 2 else d[j] ^ (1 << int(rng.integers(0, 8)))
        out.append(bytes(d))
    return out


@functools.lru_cache(maxsize=None)
def _zstd_verdict(f: bytes):
    return zo.uncompress(f)


@functools.lru_cache(maxsize=1)
def _decoder_cases():
    """{"zstd" | "snappy": [(stream, dst_cap)]} from the 64 KiB-class big
    fixtures: intact copies; overrun attempts by construction (the header
    claims 1, 1,000 and 40,000 bytes less than the stream decodes to, the
    room is the claim: both oracles and both libraries refuse them); rooms
    below an honest claim and of no bytes; random damage and cuts, the room
    the (intact) header's claim."""
    from test_big_blocks import _with_checksum
    import sys
    sys.path.insert(0, str(GOLDEN))
    import gen_big
    spec = json.loads((GOLDEN / "big.json").read_text())
    ins = gen_big.inputs()
    snap = _split((GOLDEN / "big_snappy.bin").read_bytes(), spec["snappy"])
    zst = _split((GOLDEN / "big_zstd.bin").read_bytes(), spec["zstd"])
    zbase = [(zst[0], ins[0]), (zst[4], ins[2])]
    zbase += [(_with_checksum(f, x), x) for f, x in zbase]
    sbase = [(snap[0], ins[0]), (snap[2], ins[2])]
    cases = {}
    for codec, base, claim, ulen, seed in (
            ("zstd", zbase, _zstd_claim, zo.get_uncompressed_length, 61),
            ("snappy", sbase, _snappy_claim, so.uncompressed_length, 62)):
        rng = np.random.default_rng(seed)
        c = []
        for f, x in base:
            assert ulen(f) == len(x)
            c += [(f, len(x)), (f, len(x) + 5)]
            for less in (1, 1000, 40000):
                c.append((claim(f, len(x) - less), len(x) - less))
            c += [(f, len(x) - 1), (f, len(x) // 2), (f, 0)]
        for d in _damage(rng, [f for f, _ in base], 128 - len(c) if codec == "zstd" else 120):
            n = ulen(d)
            c.append((d, n if n is not None and n <= 70000 else 0))
        assert len(c) >= 120
        cases[codec] = c
    return cases


def _decoder_want(lvkv, codec, f, cap):
    """(status, bytes): the oracle's verdict as tests/test_zstd.py's _want and
    tests/test_big_blocks.py map it."""
    if codec == "zstd":
        n = zo.get_uncompressed_length(f)
        if n is None:
            return lvkv.SNAPPY_BAD_LENGTH, b""
        if n > cap:
            return lvkv.SNAPPY_CAPACITY, b""
        ok, out = _zstd_verdict(f)
        return (lvkv.SNAPPY_OK, out) if ok else (lvkv.SNAPPY_BAD_CONTENTS, b"")
    st, out = so.uncompress(f)
    n = so.uncompressed_length(f)
    if st != so.BAD_LENGTH and n is not None and n > cap:
        return lvkv.SNAPPY_CAPACITY, b""
    return st, out


def test_overrun_attempts_are_refused_by_the_oracles():
    """The deterministic part of section C, on the CPU: a header that claims
    less than the stream decodes to is BAD_CONTENTS for both oracles (and for
    the libraries, where present)."""
    zlib, slib = zo.system_zstd(), so.system_snappy()
    for codec, ulen in (("zstd", zo.get_uncompressed_length), ("snappy", so.uncompressed_length)):
        cases = _decoder_cases()[codec]
        short = [(f, cap) for f, cap in cases[:8 * (4 if codec == "zstd" else 2)]
                 if ulen(f) == cap and cap not in (65536, 65600)]
        assert len(short) == 3 * (4 if codec == "zstd" else 2)
        for f, cap in short:
            if codec == "zstd":
                assert _zstd_verdict(f) == (False, b"")
                if zlib is not None:
                    assert zo.lib_uncompress(zlib, f) == (False, b"")
            else:
                assert so.uncompress(f) == (so.BAD_CONTENTS, b"")
                if slib is not None:
                    assert so.lib_uncompress(slib, f) == (so.BAD_CONTENTS, b"")


@pytest.mark.gpu
@pytest.mark.parametrize("max_ulen", [4096, 49152])
def test_hbm_decoders_stay_inside_their_destination(lvkv, gpu, max_ulen):
    """The decoders that write straight into the caller's buffer
    (snappy_uncompress_big_kernel, zstd_stream<true>: every stream here at
    max_ulen 4096) and the LDS-staged ones (what fits at 49152) on intact,
    lying and damaged 64 KiB streams: the oracle's status, the oracle's bytes
    where it decodes, and not a byte outside dst_cap."""
    import torch
    for codec, fn in (("snappy", lvkv.snappy_uncompress), ("zstd", lvkv.zstd_uncompress)):
        cases = _decoder_cases()[codec]
        streams, caps = zip(*cases)
        want = [_decoder_want(lvkv, codec, f, cap) for f, cap in cases]
        seen = {w[0] for w in want}
        assert {lvkv.SNAPPY_OK, lvkv.SNAPPY_BAD_CONTENTS, lvkv.SNAPPY_CAPACITY} <= seen
        src, soff, slen = _pack(torch, gpu, streams, skew=1)
        dst, doff, check = _gapped(torch, gpu, caps)
        _, _, olen, st = fn(src, _i64(torch, gpu, soff), _i32(torch, gpu, slen), max_ulen=max_ulen,
                            dst=dst, dst_offsets=_i64(torch, gpu, doff),
                            dst_caps=_i32(torch, gpu, caps))
        torch.cuda.synchronize()
        st, olen, h = st.cpu().tolist(), olen.cpu().tolist(), dst.cpu().numpy()
        what = f"{codec}, max_ulen {max_ulen}"
        bad = [(k, len(streams[k]), caps[k], st[k], want[k][0]) for k in range(len(cases))
               if st[k] != want[k][0]]
        assert not bad, f"{what}: statuses differ (stream, length, cap, got, want): {bad[:6]}"
        for k, (ws, out) in enumerate(want):
            if ws == lvkv.SNAPPY_OK:
                assert olen[k] == len(out), (what, k)
                assert h[doff[k]:doff[k] + len(out)].tobytes() == out, (what, k)
        check(h, what)


@pytest.mark.gpu
def test_read_blocks_stays_inside_out(lvkv, gpu):
    """ReadBlock over one image whose blocks' contents are 60 of the same
    streams (types 1 and 2, the trailers right for the bytes as they are),
    each out-cap what its header claims: so.read_block's verdicts, with and
    without the checksum test, and not a byte outside the caps."""
    import torch
    crc = so._crc()
    picked = [(1, f) for f, _ in _decoder_cases()["snappy"][::4][:30]] + \
             [(2, f) for f, _ in _decoder_cases()["zstd"][::4][:30]]
    assert len(picked) == 60
    img = bytearray(b"\x5a" * 3)
    handles, caps = [], []
    for t, f in picked:
        n = so.uncompressed_length(f) if t == 1 else zo.get_uncompressed_length(f)
        caps.append(n if n is not None and n <= 70000 else 0)
        handles.append((len(img), len(f)))
        img += f + bytes([t])
        img += crc.mask(crc.extend(crc.value(f), bytes([t]))).to_bytes(4, "little")
    img = bytes(img)
    want = []
    for (t, f), (o, sz), cap in zip(picked, handles, caps):
        if t == 2:  # (so.read_block's zstd case, through the cached verdict)
            n = zo.get_uncompressed_length(f)
            ok, out = (False, b"") if n is None else _zstd_verdict(f)
            ws = so.READ_ZSTD_LENGTH if n is None else so.READ_CAPACITY if ok is None else \
                so.READ_OK if ok else so.READ_ZSTD_CONTENTS
        else:
            ws, out = so.read_block(img, o, sz, True)
            n = so.uncompressed_length(f)
        if ws in (so.READ_OK, so.READ_SNAPPY_CONTENTS, so.READ_ZSTD_CONTENTS) and n is not None \
                and n > cap:
            ws = lvkv.READ_CAPACITY
        want.append((ws, out if ws == so.READ_OK else b""))
    # the zstd shortcut above is read_block's own answer
    k2 = next(k for k, (t, _) in enumerate(picked) if t == 2)
    assert so.read_block(img, *handles[k2], True)[0] == want[k2][0]
    assert {so.READ_OK, so.READ_SNAPPY_CONTENTS, so.READ_ZSTD_CONTENTS} <= {w[0] for w in want}
    file = torch.from_numpy(np.frombuffer(img, dtype=np.uint8).copy()).to(gpu)
    ho = _i64(torch, gpu, (h[0] for h in handles))
    hs = _i32(torch, gpu, (h[1] for h in handles))
    for verify in (False, True):
        out, ooff, check = _gapped(torch, gpu, caps)
        _, _, olen, st = lvkv.sst_read_blocks(file, ho, hs, max_ulen=8192, verify=verify, out=out,
                                              out_offsets=_i64(torch, gpu, ooff),
                                              out_caps=_i32(torch, gpu, caps))
        torch.cuda.synchronize()
        st, olen, h = st.cpu().tolist(), olen.cpu().tolist(), out.cpu().numpy()
        what = f"verify={verify}"
        bad = [(k, picked[k][0], st[k], want[k][0]) for k in range(60) if st[k] != want[k][0]]
        assert not bad, f"{what}: statuses differ (block, type, got, want): {bad[:6]}"
        for k, (ws, x) in enumerate(want):
            if ws == so.READ_OK:
                assert olen[k] == len(x), (what, k)
                assert h[ooff[k]:ooff[k] + len(x)].tobytes() == x, (what, k)
        check(h, what)


# ---- D. compressors stay inside their bound ----------------------------------

@pytest.mark.gpu
def test_compressors_stay_inside_their_bound(lvkv, gpu):
    """2,000 blocks of 0-20,480 bytes through zstd_compress and 500 of
    0-70,000 through snappy_compress, each destination exactly
    lvkv_zstd_compress_bound / lvkv_snappy_max_compressed_length between
    borders: every status OK, the borders intact, each frame decoded back to
    its block on the device. (An empty block's zstd frame has content size 0:
    port::Zstd_GetUncompressedLength's false, BAD_LENGTH.)"""
    import torch
    import test_zstd_write as tzw
    for codec, count, top in (("zstd", 2000, 20480), ("snappy", 500, 70000)):
        blobs = tzw._fuzz_inputs(np.random.default_rng(top), count, top + 1)
        blobs[0], blobs[1] = blobs[0][:0], zb.bench()[:top]
        src, soff, slen = _pack(torch, gpu, blobs, skew=1)
        soff, slen = _i64(torch, gpu, soff), _i32(torch, gpu, slen)
        if codec == "zstd":
            rooms = [lvkv.zstd_compress_bound(len(x)) for x in blobs]
        else:
            rooms = [lvkv.snappy_max_compressed_length(len(x)) for x in blobs]
        dst, doff, check = _gapped(torch, gpu, rooms)
        d_doff = _i64(torch, gpu, doff)
        if codec == "zstd":
            _, _, dlen, st = lvkv.zstd_compress(src, soff, slen, level=1, max_len=top, dst=dst,
                                                dst_offsets=d_doff)
        else:
            _, _, dlen, st = lvkv.snappy_compress(src, soff, slen, max_len=top, dst=dst,
                                                  dst_offsets=d_doff)
        torch.cuda.synchronize()
        assert st.cpu().tolist() == [0] * count, codec
        assert all(0 < n <= r for n, r in zip(dlen.cpu().tolist(), rooms)), codec
        check(what=codec)
        # back through the device decoder, out of the gapped buffer
        out, ooff, check2 = _gapped(torch, gpu, [len(x) for x in blobs])
        fn = lvkv.zstd_uncompress if codec == "zstd" else lvkv.snappy_uncompress
        _, _, olen, st2 = fn(dst, d_doff, dlen, max_ulen=lvkv.SNAPPY_MAX_BLOCK, dst=out,
                             dst_offsets=_i64(torch, gpu, ooff),
                             dst_caps=_i32(torch, gpu, (len(x) for x in blobs)))
        torch.cuda.synchronize()
        want_st = [lvkv.SNAPPY_BAD_LENGTH if codec == "zstd" and not x else lvkv.SNAPPY_OK
                   for x in blobs]
        assert st2.cpu().tolist() == want_st, codec
        h = out.cpu().numpy()
        bad = [k for k, (x, o) in enumerate(zip(blobs, ooff)) if h[o:o + len(x)].tobytes() != x]
        assert not bad, f"{codec}: blocks {bad[:6]} do not decode back to themselves"
        check2(h, f"{codec} read-back")
