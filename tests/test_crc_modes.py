"""Every KernelArgs mode of the batch CRC kernels (csrc/crc32c_modes.h: SST
verify / fill, WAL verify / fill) through every kernel that serves it, on one
small image per family. Which bytes are covered, from which init, against
which stored value and what is stored: table/format.cc:92-99,
table/table_builder.cc:199-203, db/log_reader.cc:243-257,
db/log_writer.cc:94-96. Expected values come from the oracle over the covered
ranges (init 0) and Mask.

Paths: "persistent" = crc32c_kernel.hip plus crc32c_long_kernel
(lvkv_debug_set_general_kernel(-1)); "ragged" = the default (WAL records on
log cfg 8); "ragged_wide" = WAL records on the 8 x 2 x 24 shape
(lvkv_debug_set_log_kernel(0)) with its in-kernel long pass at 8 KiB;
"engine" = the Engine methods of the same names with default flags."""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# content lengths: covered 1-5 (bitwise up to covered 3), a row edge, the 16-
# and 24-row chunk edges, the 64 KiB split (covered > 65536), one long block
SST_LENS = ([0, 1, 2, 3, 4] + list(range(251, 258)) + [4095, 4096, 4097, 6143, 6144, 6145,
                                                        65534, 65535, 65536, 100003])
# payload lengths: covered 1-5, a row edge, the 8 KiB split (covered > 8192),
# a full 32 KiB block's fragment, the largest a header can state
LOG_LENS = [0, 1, 2, 3, 4, 255, 256, 8190, 8191, 8192, 32761, 65535]
SST_SPLIT, LOG_SPLIT = 65536, 8192


def _le32(v):
    return np.frombuffer(np.uint32(v).tobytes(), np.uint8)


def _image(oracle, lens, log, seed):
    """Blocks of every length at every start alignment (the SST block's first
    byte, the WAL record's header), random bytes between them, each CRC field
    holding Mask(crc) of its covered range. `crc_at`: the CRC field; `cov`,
    `clen`: the covered range; `offs`: what the API takes."""
    rng = np.random.default_rng(seed)
    L = np.repeat(np.array(lens, np.uint32), 4)
    align = np.tile(np.arange(4), len(lens))
    offs, at = [], 16
    for n, k in zip(L, align):
        at = (at + 3) // 4 * 4 + int(k)
        offs.append(at)
        at += int(n) + (7 if log else 5) + int(rng.integers(1, 9))
    offs = np.array(offs, np.int64)
    img = rng.integers(0, 256, at + 16, dtype=np.uint8)
    if log:
        for o, n in zip(offs, L):
            img[o + 4] = n & 0xFF
            img[o + 5] = n >> 8
            img[o + 6] = rng.integers(1, 5)  # kFullType..kLastType
        cov, crc_at = offs + 6, offs
    else:
        cov, crc_at = offs, offs + L.astype(np.int64) + 1
    clen = L + np.uint32(1)
    crc = oracle.batch(img, cov.astype(np.uint64), clen, threads=8)
    for p, c in zip(crc_at, crc):
        img[p:p + 4] = _le32(oracle.mask(int(c)))
    return SimpleNamespace(img=img, offs=offs, sizes=L.view(np.int32), cov=cov, clen=clen,
                           crc_at=crc_at, crc=crc, log=log)


@pytest.fixture(scope="module")
def images(oracle):
    sst = _image(oracle, SST_LENS, False, 11)
    log = _image(oracle, LOG_LENS, True, 12)
    assert sst.offs.size < 100 and sst.img.size < (2 << 20)
    return {"sst": sst, "log": log}


@pytest.fixture(scope="module")
def eng(lvkv, gpu):
    e = lvkv.Engine(gpu)
    yield e
    e.close()


CASES = [(p, f) for p in ("persistent", "ragged", "engine") for f in ("sst", "log")]
CASES.append(("ragged_wide", "log"))


@pytest.fixture(params=CASES, ids=["%s-%s" % c for c in CASES])
def path(request, lvkv, gpu, eng):
    """(verify, fill, image family) of one path; the knobs go back to their
    defaults (general kernel 0, log cfg 8) afterwards."""
    import torch
    name, family = request.param
    L_ = lvkv.lib

    def dev(a):
        return torch.from_numpy(np.ascontiguousarray(a)).to(gpu)

    def call(fn_sst, fn_log, wait):
        def run(im, img):
            buf = dev(img)
            args = (dev(im.offs),) if im.log else (dev(im.offs), dev(im.sizes))
            out = (fn_log if im.log else fn_sst)(buf, *args)
            wait()
            return buf, out
        return run

    if name == "engine":
        v = call(eng.sst_verify, eng.log_verify, eng.wait)
        f = call(eng.sst_fill_trailers, eng.log_fill_headers, eng.wait)
        yield v, f, family
        return
    assert L_.lvkv_debug_set_general_kernel(-1 if name == "persistent" else 0) == 0
    assert L_.lvkv_debug_set_log_kernel(0 if name == "ragged_wide" else 8) == 0
    try:
        v = call(lvkv.sst_verify, lvkv.log_verify, torch.cuda.synchronize)
        f = call(lvkv.sst_fill_trailers, lvkv.log_fill_headers, torch.cuda.synchronize)
        yield v, f, family
    finally:
        L_.lvkv_debug_set_general_kernel(0)
        L_.lvkv_debug_set_log_kernel(8)


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


def _describe(im, idx):
    return [(int(im.clen[i]), int(im.offs[i] % 4)) for i in idx[:10]]


def _check_verify(im, out, want_crc, want_bad):
    actual, status = _u32(out[0]), out[1].cpu().numpy()
    wrong = np.nonzero(actual != want_crc)[0]
    assert wrong.size == 0, ("actual (covered, align)", _describe(im, wrong))
    assert set(np.unique(status).tolist()) <= {0, 1}
    got = np.nonzero(status)[0].tolist()
    assert got == sorted(want_bad), ("status (covered, align)",
                                    _describe(im, sorted(set(got) ^ set(want_bad))))


def test_verify(oracle, images, path):
    verify, _, family = path
    im = images[family]
    n = im.offs.size
    # clean: every status 0, every actual the oracle's
    _, out = verify(im, im.img)
    _check_verify(im, out, im.crc, [])
    # one byte flipped in the first block, every fifth and every block past
    # the split bound: in the covered range, then in the stored CRC
    split = LOG_SPLIT if im.log else SST_SPLIT
    hit = sorted(set(range(0, n, 5)) | set(np.nonzero(im.clen > split)[0].tolist()))
    assert any(im.clen[i] > split for i in hit) and any(im.clen[i] < 4 for i in hit)
    bad = im.img.copy()
    for i in hit:
        bad[int(im.cov[i]) + int(im.clen[i]) // 2] ^= 0x20
    _, out = verify(im, bad)
    _check_verify(im, out, oracle.batch(bad, im.cov.astype(np.uint64), im.clen, threads=8), hit)
    bad = im.img.copy()
    for j, i in enumerate(hit):
        bad[int(im.crc_at[i]) + j % 4] ^= 0x01
    _, out = verify(im, bad)
    _check_verify(im, out, im.crc, hit)


def test_fill(images, path):
    _, fill, family = path
    im = images[family]
    wiped = im.img.copy()
    for p in im.crc_at:
        wiped[p:p + 4] = 0xEE
    buf, crc = fill(im, wiped)
    wrong = np.nonzero(_u32(crc) != im.crc)[0]  # the returned CRCs are unmasked
    assert wrong.size == 0, ("crc (covered, align)", _describe(im, wrong))
    # the whole buffer: the four CRC bytes of each block and nothing else moved
    got = buf.cpu().numpy()
    diff = np.nonzero(got != im.img)[0]
    assert diff.size == 0, ("first differing bytes", diff[:10].tolist())
