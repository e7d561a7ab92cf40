"""The kernels only the AQL engine runs (csrc/lvkv_engine_kernels.hip, a code
object of its own) against the CPU oracle, at the shapes where they differ
from their HIP-path siblings.

A. The two burst kernels of crc32c_burst.h (lvkv_ek_uniform: 8 waves x 5
   chains, lvkv_ek_uniform_pair: 8 x 3, chain-pipelined) and their timestamp
   builds, each as the overlapped, the ordered and the LVKV_FLAG_FINAL kernel:
   every length 4..4096 (every (rows, s0l, delta) of uni_geo /
   fix_first_chunk, with a non-zero init), every burst_body<NV, FULL> on
   short and on 16-row blocks with dead waves beside live ones, and the
   strides the contract allows (gaps, overlaps, 0).
B. The four ragged_run shapes (<8,2,24>, <8,4,8>, <8,4,17>, <8,6,8>), each
   forced in turn: lengths around R*256 and 2R*256 bytes at every start
   alignment in the offset and the uniform layout, both sides of the routing
   seams of submit_general, and the cuts of a one-round batch into dispatches.

Every expected value is the oracle's (util/crc32c.cc:276-377 restated on the
CPU); every comparison is exact equality of 32-bit values."""
from __future__ import annotations

import contextlib
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

WAVES = 8                       # waves per workgroup of every engine kernel
KERNELS = [0, 1]                # 0: lvkv_ek_uniform, 1: lvkv_ek_uniform_pair
KERNEL_IDS = ["uniform", "pair"]
ROLES = ["overlapped", "ordered", "final"]
SPECS = [2, 3, 4, 5]            # ragged_run<8,2,24>, <8,4,8>, <8,4,17>, <8,6,8>
INITS = [0, 0xFFFFFFFF, 0x9E3779B1]


@pytest.fixture(scope="module")
def eng(lvkv, gpu):
    L = lvkv.lib
    L.lvkv_engine_set_variant.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int]
    L.lvkv_engine_set_final_variant.argtypes = [ctypes.c_void_p, ctypes.c_int]
    L.lvkv_engine_set_stamps.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64]
    L.lvkv_debug_engine_ragged_spec.argtypes = [ctypes.c_void_p, ctypes.c_int]
    e = lvkv.Engine(gpu)
    yield e
    e.close()


def _device_bytes(torch, gpu, n, seed):
    """n random bytes written by a kernel of this device (so a submit needs no
    system-scope acquire), and their host copy."""
    g = torch.Generator(device=gpu).manual_seed(seed)
    d = torch.randint(0, 256, (n,), dtype=torch.uint8, device=gpu, generator=g)
    torch.cuda.synchronize()
    assert d.data_ptr() % 4 == 0
    return d, d.cpu().numpy()


def _shape_of(lvkv, eng, kernel):
    """(chains per wave, workgroups per dispatch) of a burst kernel: the
    engine's own figures, with that kernel set as the overlapped one."""
    assert lvkv.lib.lvkv_engine_set_variant(eng.handle, kernel, 1 - kernel) == 0
    waves, chains, groups = eng.shape()
    assert lvkv.lib.lvkv_engine_set_variant(eng.handle, 0, 1) == 0
    assert waves == WAVES
    return chains, groups


@contextlib.contextmanager
def _role(lvkv, eng, kernel, role):
    """Burst kernel `kernel` as the kernel of overlapped, of ordered or of
    LVKV_FLAG_FINAL dispatches (the other kernel everywhere else); yields the
    submit's keywords. Defaults restored afterwards."""
    L, h = lvkv.lib, eng.handle
    try:
        if role == "overlapped":
            assert L.lvkv_engine_set_variant(h, kernel, 1 - kernel) == 0
            yield {}
        elif role == "ordered":
            assert L.lvkv_engine_set_variant(h, 1 - kernel, kernel) == 0
            yield {"ordered": True}
        else:
            assert L.lvkv_engine_set_variant(h, 1 - kernel, 1 - kernel) == 0
            assert L.lvkv_engine_set_final_variant(h, kernel) == 0
            yield {"final": True}
    finally:
        L.lvkv_engine_set_variant(h, 0, 1)  # waits for outstanding work first
        L.lvkv_engine_set_final_variant(h, -1)
        eng._inflight.clear()


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


def _first_bad(got, want):
    bad = np.nonzero(got != want)[0]
    return f"{bad.size} of {want.size} wrong, first at block {bad[:4].tolist()}"


# ---------------------------------------------------------------------------
# A.1 every length 4..4096

@pytest.fixture(scope="module")
def every_length(oracle, gpu):
    """Three blocks of every length 4..4096, ends 4-byte aligned, stride the
    length rounded up to 4 (so a block's front padding is its predecessor's
    tail, or the buffer's first bytes), init a hash of the length, Mask on
    odd lengths; the oracle's values, computed once."""
    import torch
    d, host = _device_bytes(torch, gpu, 3 + 3 * 4096 + 16, 0xB0057)
    lengths = np.arange(4, 4097, dtype=np.int64)
    shift = (-lengths) % 4
    stride = lengths + shift
    inits = (lengths * 2654435761) & 0xFFFFFFFF
    offs = (shift[:, None] + np.arange(3)[None, :] * stride[:, None]).ravel()
    lens, ini = np.repeat(lengths, 3), np.repeat(inits, 3)
    plain = oracle.batch(host, offs, lens, ini, threads=8)
    masked = oracle.batch(host, offs, lens, ini, mask=True, threads=8)
    want = np.where(np.repeat(lengths & 1, 3) == 1, masked, plain).reshape(-1, 3)
    return d, lengths, shift, stride, inits, want


@pytest.mark.parametrize("role", ROLES)
@pytest.mark.parametrize("kernel", KERNELS, ids=KERNEL_IDS)
def test_burst_every_length(lvkv, eng, gpu, every_length, kernel, role):
    """One submit of three blocks per length 4..4096: one workgroup, one chain
    in three waves, five dead waves; every (rows, s0l, delta), the init spill
    into the next word and into row 1 (s0l == 63). All submits in flight
    before one wait (the engine fences itself when its kernarg ring fills)."""
    import torch
    d, lengths, shift, stride, inits, want = every_length
    out = torch.zeros(want.shape, dtype=torch.int32, device=gpu)
    torch.cuda.synchronize()
    with _role(lvkv, eng, kernel, role) as kw:
        for i, L in enumerate(lengths.tolist()):
            eng.crc32c_uniform(d[int(shift[i]):], 3, L, int(stride[i]), init=int(inits[i]),
                               mask=bool(L & 1), fresh=False, out=out[i], **kw)
        eng.wait()
    got = out.cpu().numpy().view(np.uint32)
    bad = lengths[(got != want).any(axis=1)]
    assert bad.size == 0, f"{bad.size} lengths wrong, first {bad[:8].tolist()}"


# ---------------------------------------------------------------------------
# A.2 chain counts x block shape

CHAIN_LENGTHS = ([5, 6, 7, 8] + list(range(253, 261)) + list(range(2049, 2053)) +
                 list(range(3837, 3845)) + list(range(4093, 4097)))


def _rows(length):
    return ((length + 3) // 4 + 63) // 64


def _bodies(n, groups, chains, length):
    """The burst_body<NV, FULL>(live) instantiations a submit of n blocks
    runs, by the engine's cut into dispatches (lvkv_engine_crc32c_uniform)
    and the kernel's work map (burst_kernel_body)."""
    full = _rows(length) == 16
    cap = groups * WAVES * chains
    nd = -(-n // cap)
    out = set()
    for m in {n // nd, -(-n // nd)}:                 # the dispatches' sizes
        ngroups = min(groups, (m + 2) // 3)
        per, extra = divmod(m, ngroups)
        for items in ({per, per + 1} if extra else {per}):   # the first `extra` get one more
            for w in range(WAVES):
                nv = sum(1 for c in range(chains) if c * WAVES + w < items)
                out.add((max(nv, 1), full, nv != 0))
    return out


def _chain_counts(groups, chains):
    """Block counts that give k chains to every wave but one (8kG - 1), one
    wave of k chains beside seven of k - 1 in half of the workgroups
    (8(k-1)G + ceil(G/2); k = 1: dead waves), and two dispatches of unequal
    size (capacity + 1)."""
    ns = []
    for k in range(1, chains + 1):
        ns += [8 * k * groups - 1, 8 * (k - 1) * groups + (groups + 1) // 2]
    return ns + [groups * WAVES * chains + 1]


@pytest.fixture(scope="module")
def chain_blocks(lvkv, oracle, eng, gpu):
    """One random buffer (about 50 MB on a 256-CU device: the pair kernel's
    capacity + 1 blocks of 4 KiB) for every case of A.2, A.3, A.4, B.2 and
    B.3, and a memo of the oracle's values over it."""
    import torch
    shapes = {k: _shape_of(lvkv, eng, k) for k in KERNELS}
    nmax = max(g * WAVES * c for c, g in shapes.values()) + 1
    d, host = _device_bytes(torch, gpu, nmax * 4096 + 64, 0xC4A1)
    memo = {}

    def want(nblocks, length, stride, shift, init=0, mask=False):
        key = (length, stride, shift, init, mask)
        if key not in memo or memo[key].size < nblocks:
            memo[key] = oracle.uniform(host[shift:], nblocks, length, stride, init=init,
                                       mask=mask, threads=8)
        return memo[key][:nblocks]

    return d, shapes, nmax, want


@pytest.mark.parametrize("role", ROLES)
@pytest.mark.parametrize("kernel", KERNELS, ids=KERNEL_IDS)
def test_burst_chain_counts(lvkv, eng, gpu, chain_blocks, kernel, role):
    """Every burst_body<NV, FULL>: NV = 1..NCH valid chains on short and on
    16-row blocks, workgroups mixing waves of k and of k - 1 chains, dead
    waves, at the lengths where rows, s0l == 63 and delta change; three inits,
    Mask off and on. The reach is computed from the work map first."""
    import torch
    d, shapes, nmax, want = chain_blocks
    chains, groups = shapes[kernel]
    ns = _chain_counts(groups, chains)
    assert max(ns) <= nmax
    reach = set()
    for L in CHAIN_LENGTHS:
        for n in ns:
            reach |= _bodies(n, groups, chains, L)
    live = {(nv, full) for nv, full, alive in reach if alive}
    assert live == {(nv, full) for nv in range(1, chains + 1) for full in (False, True)}
    assert {full for nv, full, alive in reach if not alive} == {False, True}  # dead waves
    # k chains beside k - 1 in one workgroup, short and full blocks
    for k in range(2, chains + 1):
        for L in (2049, 3841):
            assert {k, k - 1} <= {nv for nv, _, _ in _bodies(8 * (k - 1) * groups +
                                                            (groups + 1) // 2, groups, chains, L)}

    out = torch.zeros(6 * sum(ns), dtype=torch.int32, device=gpu)
    torch.cuda.synchronize()
    with _role(lvkv, eng, kernel, role) as kw:
        for L in CHAIN_LENGTHS:
            shift = -L % 4
            stride = L + shift
            cases, at = [], 0
            for init in INITS:
                for mask in (False, True):
                    for n in ns:
                        eng.crc32c_uniform(d[shift:], n, L, stride, init=init, mask=mask,
                                           fresh=False, out=out[at:at + n], **kw)
                        cases.append((init, mask, n, at))
                        at += n
            eng.wait()
            got = _u32(out)
            for init, mask, n, at in cases:
                w = want(nmax, L, stride, shift, init, mask)[:n]
                assert np.array_equal(got[at:at + n], w), \
                    (L, hex(init), mask, n, _first_bad(got[at:at + n], w))


# ---------------------------------------------------------------------------
# A.3 strides

@pytest.mark.parametrize("role", ROLES)
@pytest.mark.parametrize("kernel", KERNELS, ids=KERNEL_IDS)
def test_burst_strides(lvkv, eng, gpu, chain_blocks, kernel, role):
    """Any stride that is a multiple of 4 (include/lvkv_crc32c.h): a gap
    between the blocks, overlapping blocks 4 bytes apart, and stride 0 (every
    block the same bytes, every output equal); a short (4 rows, delta 3) and a
    16-row (delta 2) length, waves of 2 and of 3 chains."""
    import torch
    d, shapes, nmax, want = chain_blocks
    chains, groups = shapes[kernel]
    n = 16 * groups + (groups + 1) // 2
    nvs = {nv for nv, _, alive in _bodies(n, groups, chains, 1021) if alive}
    assert nvs == {2, 3}
    init = 0x1234ABCD
    with _role(lvkv, eng, kernel, role) as kw:
        for L in (1021, 4090):
            shift = -L % 4
            strides = [L + shift + 260, 4, 0]
            assert (n - 1) * strides[0] + L + shift <= d.numel()
            outs = [eng.crc32c_uniform(d[shift:], n, L, s, init=init, mask=(s == 4),
                                       fresh=False, **kw) for s in strides]
            eng.wait()
            for s, o in zip(strides, outs):
                w = want(n, L, s, shift, init, s == 4)
                assert np.array_equal(_u32(o), w), (L, s, _first_bad(_u32(o), w))
                if s == 0:
                    assert np.unique(_u32(o)).size == 1


# ---------------------------------------------------------------------------
# A.4 the timestamp builds

@pytest.mark.parametrize("kernel", KERNELS, ids=KERNEL_IDS)
def test_burst_stamp_builds(lvkv, eng, gpu, chain_blocks, kernel):
    """lvkv_ek_uniform_stamps / lvkv_ek_uniform_pair_stamps (separate
    kernels): the same CRCs on a short and a 16-row length with delta != 0,
    over two dispatches; stamps land inside areas x G x waves x 8 u64 and
    nowhere after it."""
    import torch
    d, shapes, nmax, want = chain_blocks
    L_, h = lvkv.lib, eng.handle
    chains, groups = shapes[kernel]
    areas, guard, pattern = 3, 4096, 0x5A5AA5A55A5AA5A5
    words = areas * groups * WAVES * 8
    st = torch.zeros(words + guard, dtype=torch.int64, device=gpu)
    st[words:] = pattern
    torch.cuda.synchronize()
    n = groups * WAVES * chains + 1          # two dispatches, two areas
    try:
        # every role dispatches the kernel under test: the area size the
        # engine uses is that kernel's
        assert L_.lvkv_engine_set_variant(h, kernel, kernel) == 0
        assert eng.shape() == (WAVES, chains, groups)
        assert L_.lvkv_engine_set_stamps(h, ctypes.c_void_p(st.data_ptr()), areas) == 0
        for L in (1022, 3842):
            shift = -L % 4
            stride = L + shift
            a = eng.crc32c_uniform(d[shift:], n, L, stride, init=0xFEEDF00D, fresh=False)
            b = eng.crc32c_uniform(d[shift:], n, L, stride, init=0xFEEDF00D, fresh=False,
                                   ordered=True, mask=True)
            eng.wait()
            w = want(n, L, stride, shift, 0xFEEDF00D, False)
            assert np.array_equal(_u32(a), w), (L, _first_bad(_u32(a), w))
            w = want(n, L, stride, shift, 0xFEEDF00D, True)
            assert np.array_equal(_u32(b), w), (L, _first_bad(_u32(b), w))
    finally:
        L_.lvkv_engine_set_stamps(h, None, 0)  # waits for outstanding work first
        L_.lvkv_engine_set_variant(h, 0, 1)
        eng._inflight.clear()
    host = st.cpu().numpy()
    assert (host[words:] == pattern).all(), "a stamp was written past the stamp areas"
    assert host[:words].any()


# ---------------------------------------------------------------------------
# B.1 the ragged_run shapes at their chunk edges

EDGE_LENGTHS = sorted({r * 256 + dd for r in (1, 7, 8, 9, 15, 16, 17, 18, 23, 24, 25, 33, 34, 35,
                                             47, 48, 49) for dd in range(-4, 5)} |
                      set(range(9)) | {65535, 65536, 65537, 70001})


@contextlib.contextmanager
def _spec(lvkv, eng, spec):
    try:
        assert lvkv.lib.lvkv_debug_engine_ragged_spec(eng.handle, spec) == 0
        yield
    finally:
        try:
            eng.wait()
        finally:
            lvkv.lib.lvkv_debug_engine_ragged_spec(eng.handle, -1)


@pytest.fixture(scope="module")
def edge_offsets(oracle, gpu):
    """Every edge length at every start alignment 0..3, shuffled (one round
    holds chains of different chunk counts), a few bytes between the blocks,
    per-block inits; the oracle's values."""
    import torch
    rng = np.random.default_rng(0xED6E)
    L = np.repeat(np.array(EDGE_LENGTHS, np.int64), 4)
    align = np.tile(np.arange(4), len(EDGE_LENGTHS))
    order = rng.permutation(L.size)
    L, align = L[order], align[order]
    offs = np.empty(L.size, np.int64)
    at = 4
    for i in range(L.size):
        at = (at + 3) // 4 * 4 + int(align[i])
        offs[i] = at
        at += int(L[i]) + int(rng.integers(1, 8))
    d, host = _device_bytes(torch, gpu, at + 8, 0xED6E)
    inits = rng.integers(0, 2**32, L.size, dtype=np.uint64).astype(np.uint32)
    L32 = L.astype(np.uint32)
    o64 = offs.astype(np.uint64)
    want = oracle.batch(host, o64, L32, inits, threads=8)
    want_m = oracle.batch(host, o64, L32, np.full(L.size, 0x0BADF00D, np.uint32), mask=True,
                          threads=8)
    dev = (d, torch.from_numpy(offs).to(gpu), torch.from_numpy(L32.view(np.int32)).to(gpu),
           torch.from_numpy(inits.view(np.int32)).to(gpu))
    torch.cuda.synchronize()
    return dev, L, align, want, want_m


@pytest.mark.parametrize("spec", SPECS)
def test_ragged_shapes_edge_lengths_offsets(lvkv, eng, gpu, edge_offsets, spec):
    """Offset layout: the whole list, batches of 1, 5, 17 and 33 blocks (idle
    chains) taken at several places of it, and the list repeated past two
    rounds per workgroup; compute with per-block inits, masked with one init,
    and ordered."""
    import torch
    (d, do, dl, di), L, align, want, want_m = edge_offsets
    assert {(int(a), int(x)) for a, x in zip(align, L)} == \
        {(a, x) for a in range(4) for x in EDGE_LENGTHS}
    rng = np.random.default_rng(spec)
    cuts = [(0, L.size)] + [(int(s), size) for size in (1, 5, 17, 33)
                            for s in rng.integers(0, L.size - size, 4)]
    # The list over and over, past two rounds of every workgroup of the
    # persistent shapes (2 per CU x 8 waves x 4 chains) and past two
    # dispatches of the one-round ones: a batch under workgroups x one round
    # gives every workgroup a single round, whatever its size.
    cus = _shape_of(lvkv, eng, 0)[1]
    rep = np.resize(np.arange(L.size), 2 * 2 * cus * 32 + 77)
    ri = torch.from_numpy(rep).to(gpu)
    ro, rl, rin = do[ri], dl[ri], di[ri]
    torch.cuda.synchronize()
    with _spec(lvkv, eng, spec):
        runs = []
        for s, size in cuts:
            sl = slice(s, s + size)
            runs.append((sl, eng.crc32c_batch(d, do[sl], dl[sl], inits=di[sl]),
                         eng.crc32c_batch(d, do[sl], dl[sl], init=0x0BADF00D, mask=True),
                         eng.crc32c_batch(d, do[sl], dl[sl], inits=di[sl], ordered=True)))
        runs.append((rep, eng.crc32c_batch(d, ro, rl, inits=rin),
                     eng.crc32c_batch(d, ro, rl, init=0x0BADF00D, mask=True),
                     eng.crc32c_batch(d, ro, rl, inits=rin, ordered=True)))
        eng.wait()
    for sl, a, m, o in runs:
        for name, got, w in (("compute", a, want[sl]), ("masked", m, want_m[sl]),
                             ("ordered", o, want[sl])):
            bad = np.nonzero(_u32(got) != w)[0]
            assert bad.size == 0, (name, got.numel(),
                                   [(int(L[sl][i]), int(align[sl][i])) for i in bad[:6]])


def _unaligned_stride(length):
    """The smallest stride over `length` that is no multiple of 4: with it a
    uniform submit of any length and base goes to the general walk."""
    s = length + 1
    return s if s % 4 else s + 1


@pytest.fixture(scope="module")
def edge_uniform(oracle, gpu):
    """70 blocks (more than two rounds of the 8 x 4 shapes) of every edge
    length at base shifts 1..3, a gap of one or two bytes between them (the
    blocks' alignments differ); the oracle's values, plain and masked."""
    import torch
    nb = 70
    d, host = _device_bytes(torch, gpu, 3 + nb * _unaligned_stride(EDGE_LENGTHS[-1]) + 8, 0x0E1F)
    cases = [(L, shift) for L in EDGE_LENGTHS for shift in (1, 2, 3)]
    init = 0x600DCAFE
    want = np.stack([oracle.uniform(host[s:], nb, L, _unaligned_stride(L), init=init, threads=8)
                     for L, s in cases])
    want_m = np.stack([oracle.uniform(host[s:], nb, L, _unaligned_stride(L), init=init, mask=True,
                                      threads=8) for L, s in cases])
    return d, nb, cases, init, want, want_m


@pytest.mark.parametrize("spec", SPECS)
def test_ragged_shapes_edge_lengths_uniform(lvkv, eng, gpu, edge_uniform, spec):
    """Uniform layout (offsets == nullptr) through each shape: one submit per
    edge length and base shift; compute, masked and ordered."""
    import torch
    d, nb, cases, init, want, want_m = edge_uniform
    out = torch.zeros((3, len(cases), nb), dtype=torch.int32, device=gpu)
    torch.cuda.synchronize()
    with _spec(lvkv, eng, spec):
        for i, (L, shift) in enumerate(cases):
            stride = _unaligned_stride(L)
            assert stride % 4 != 0  # never the burst kernel
            for j, kw in enumerate(({}, {"mask": True}, {"ordered": True})):
                eng.crc32c_uniform(d[shift:], nb, L, stride, init=init, fresh=False,
                                   out=out[j, i], **kw)
        eng.wait()
    got = out.cpu().numpy().view(np.uint32)
    for j, (name, w) in enumerate((("compute", want), ("masked", want_m), ("ordered", want))):
        bad = np.nonzero((got[j] != w).any(axis=1))[0]
        assert bad.size == 0, (name, [cases[i] for i in bad[:8]])


# ---------------------------------------------------------------------------
# B.2 the routing seams of submit_general, by the engine's own choice

@pytest.mark.parametrize("length,shift", [
    (2045, 1), (2046, 1),      # 8 rows | 9: persistent 8 x 4 x 8 | one-round 8 x 4 x 17
    (4349, 1), (4350, 1),      # 17 rows | 18: one-round 8 x 4 x 17 | persistent 8 x 2 x 24
    (4096, 1),                 # the burst kernel's length, ends unaligned
    (4097, 3), (4098, 2), (4099, 1), (4100, 0),  # aligned ends, past the burst kernel
])
def test_engine_routing_seams(lvkv, eng, gpu, chain_blocks, length, shift):
    """Both sides of each seam, overlapped and ordered (an ordered batch of
    the one-round shape falls back to the persistent walk); enough blocks for
    two dispatches of the one-round shape."""
    d, shapes, nmax, want = chain_blocks
    cus = shapes[0][1]                      # lvkv_ek_uniform: one workgroup per CU
    n = 32 * cus + 7
    stride = length + (-length % 4) if (shift + length) % 4 == 0 else length
    assert (n - 1) * stride + length + shift <= d.numel()
    assert lvkv.lib.lvkv_debug_engine_ragged_spec(eng.handle, -1) == 0
    a = eng.crc32c_uniform(d[shift:], n, length, stride, init=0x7E57AB1E, fresh=False)
    b = eng.crc32c_uniform(d[shift:], n, length, stride, init=0x7E57AB1E, fresh=False,
                           ordered=True)
    eng.wait()
    w = want(n, length, stride, shift, 0x7E57AB1E)
    assert np.array_equal(_u32(a), w), ("overlapped", _first_bad(_u32(a), w))
    assert np.array_equal(_u32(b), w), ("ordered", _first_bad(_u32(b), w))


# ---------------------------------------------------------------------------
# B.3 a one-round batch cut into dispatches of cus x 32 blocks

def test_one_round_dispatch_cuts(lvkv, oracle, eng, gpu, chain_blocks):
    """ragged_run<8,4,17> forced, 2100-byte blocks, one block under, at and
    over one dispatch and one over two: every block of every dispatch (its
    offsets, lengths, inits and outputs start where the previous dispatch
    ended), in the offset and in the uniform layout."""
    import torch
    d, shapes, nmax, want = chain_blocks
    cus = shapes[0][1]
    L, stride = 2100, 2101
    nbig = 2 * 32 * cus + 1
    assert nbig * 2104 + 8 <= d.numel()
    host = d.cpu().numpy()
    rng = np.random.default_rng(0xC075)
    offs = np.arange(nbig, dtype=np.int64) * 2104 + rng.integers(0, 4, nbig)
    lens = np.full(nbig, L, np.uint32)
    inits = rng.integers(0, 2**32, nbig, dtype=np.uint64).astype(np.uint32)
    w_off = oracle.batch(host, offs.astype(np.uint64), lens, inits, threads=8)
    do, dl = torch.from_numpy(offs).to(gpu), torch.from_numpy(lens.view(np.int32)).to(gpu)
    di = torch.from_numpy(inits.view(np.int32)).to(gpu)
    torch.cuda.synchronize()
    with _spec(lvkv, eng, 4):
        runs = []
        for n in (32 * cus - 1, 32 * cus, 32 * cus + 1, nbig):
            runs.append((n, eng.crc32c_batch(d, do[:n], dl[:n], inits=di[:n]),
                         eng.crc32c_uniform(d[1:], n, L, stride, init=0xD15BA7C4, mask=True,
                                            fresh=False)))
        eng.wait()
    for n, a, u in runs:
        assert np.array_equal(_u32(a), w_off[:n]), (n, _first_bad(_u32(a), w_off[:n]))
        w = want(n, L, stride, 1, 0xD15BA7C4, True)
        assert np.array_equal(_u32(u), w), (n, _first_bad(_u32(u), w))
