"""Device time of lvkv_memtable_from_batches_device on the table build
benchmark's entries (tools/table_build_bench.py): 253,952 user keys of 16
bytes with 100-byte values, shuffled, written as puts into batches of one
entry, of 100, of 1 MiB, and into one batch of everything. HIP events around
one call, 5 timed calls after 3. The answers are checked before anything is
timed: the report, the key image, every per-entry array. Beside it, in the
same run on the same buffers: lvkv_sst_build_blocks_device on the call's
result, and torch.sort of as many int64 (a device sort with no key bytes
behind it). Then the sort's tile (lvkv_debug_set_memtable_tile: 512, 1024,
2048 pairs) at batches of 100. One JSON line (profiles/memtable_time.json).

  --only SHAPE   one shape (one, 100, 1MiB, all), two calls, nothing else:
                 the run a kernel trace is taken of."""
import ctypes
import json
import sys
from pathlib import Path

import numpy as np
import torch

REPO = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(REPO), str(REPO / "oracle"), str(REPO / "tests")]
import __graft_entry__ as g

lvkv = g.load_package()
L = lvkv.lib
dev = torch.device("cuda:0")
N, KLEN, VLEN = 253952, 16, 100
REC = 1 + 1 + KLEN + 1 + VLEN  # tag, varint, key, varint, value
p = lambda t: ctypes.c_void_p(t.data_ptr())
stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
u8 = lambda n: torch.empty(n, dtype=torch.uint8, device=dev)
i64 = lambda n: torch.empty(n, dtype=torch.int64, device=dev)
i32 = lambda n: torch.empty(n, dtype=torch.int32, device=dev)

rng = np.random.default_rng(7)
perm = rng.permutation(N)
records = np.empty((N, REC), dtype=np.uint8)
records[:, 0] = 1
records[:, 1] = KLEN
digits = np.char.zfill(perm.astype(str), KLEN)
records[:, 2:2 + KLEN] = np.frombuffer("".join(digits).encode(), dtype=np.uint8).reshape(-1, KLEN)
records[:, 2 + KLEN] = VLEN
records[:, 3 + KLEN] = 2  # the type byte the fork's Put leaves
records[:, 4 + KLEN:] = rng.integers(0, 256, (N, VLEN - 1), dtype=np.uint8)


def timed(fn, calls=8, warm=3):
    times = []
    for _ in range(calls):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        rc = fn()
        b.record()
        torch.cuda.synchronize()
        assert rc in (0, None), rc
        times.append(a.elapsed_time(b))
    return [round(t, 4) for t in times[warm:]]


def layout(per_batch):
    """The payload of batches of per_batch entries (sequence 1 + the first
    entry's index), the batches' places, and every entry's place."""
    first = np.arange(0, N, per_batch)
    counts = np.minimum(per_batch, N - first)
    boff = first * REC + 12 * np.arange(len(first))
    blen = counts * REC + 12
    total = int(boff[-1] + blen[-1])
    payload = np.zeros(total, dtype=np.uint8)
    entry_at = np.arange(N) * REC + 12 * (np.arange(N) // per_batch + 1)
    payload[(entry_at[:, None] + np.arange(REC)[None, :]).reshape(-1)] = records.reshape(-1)
    heads = np.zeros((len(first), 12), dtype=np.uint8)
    heads[:, :8] = (first + 1).astype("<u8").reshape(-1, 1).view(np.uint8)
    heads[:, 8:] = counts.astype("<u4").reshape(-1, 1).view(np.uint8)
    payload[(boff[:, None] + np.arange(12)[None, :]).reshape(-1)] = heads.reshape(-1)
    return payload, boff, blen, entry_at


def measure(name, per_batch, only=False, tiles=False):
    payload, boff, blen, entry_at = layout(per_batch)
    nb = len(boff)
    d_payload = torch.from_numpy(payload).to(dev)
    d_boff, d_blen = torch.from_numpy(boff).to(dev), torch.from_numpy(blen).to(dev)
    kcap = N * (KLEN + 8)
    need = L.lvkv_memtable_scratch_bytes(nb, N)
    scratch, keys = u8(need), u8(kcap)
    koff, klen, voff, vlen, src = i64(N), i32(N), i64(N), i32(N), i32(N)
    rep = torch.zeros(ctypes.sizeof(lvkv.MemtableReport), dtype=torch.uint8, device=dev)

    def call():
        return L.lvkv_memtable_from_batches_device(
            p(d_payload), p(d_boff), p(d_blen), nb, 0, 0, p(scratch), need, p(keys), kcap, p(koff),
            p(klen), p(voff), p(vlen), p(src), N, None, None, p(rep), stream)

    assert call() == 0
    torch.cuda.synchronize()
    r = lvkv.MemtableReport.from_buffer_copy(bytes(rep.cpu().numpy())).as_dict()
    assert r == dict(status=0, first_bad_batch=0xFFFFFFFF, first_bad_entry=0xFFFFFFFF, nentries=N,
                     key_bytes=kcap, val_bytes=N * VLEN, max_key_len=KLEN + 8, n_too_small=0,
                     too_small_bytes=0, max_sequence_out=N, n_bad_batches=0), r
    order = np.argsort(perm)  # the log index of the entry with the i-th smallest key
    assert np.array_equal(src.cpu().numpy(), order.astype(np.int32))
    assert np.array_equal(koff.cpu().numpy(), order * (KLEN + 8))
    assert np.array_equal(voff.cpu().numpy(), entry_at[order] + 3 + KLEN)
    assert bool((klen == KLEN + 8).all()) and bool((vlen == VLEN).all())
    rows = keys.cpu().numpy().reshape(N, KLEN + 8)
    assert np.array_equal(rows[:, :KLEN], records[:, 2:2 + KLEN])
    trailer = (((np.arange(N, dtype=np.uint64) + np.uint64(1)) << np.uint64(8)) | np.uint64(1))
    assert np.array_equal(rows[:, KLEN:].copy().view("<u8").reshape(-1), trailer)
    res = {"batches": nb, "payload_bytes": int(payload.size)}
    if only:
        timed(call, calls=2, warm=0)
        return res
    res["memtable_ms"] = timed(call)
    if tiles:
        res["memtable_ms_by_tile"] = {}
        for t in (512, 1024, 2048):
            assert L.lvkv_debug_set_memtable_tile(t) == 0
            assert call() == 0
            torch.cuda.synchronize()
            assert np.array_equal(src.cpu().numpy(), order.astype(np.int32))
            res["memtable_ms_by_tile"][str(t)] = timed(call)
        assert L.lvkv_debug_set_memtable_tile(0) == 0

    # the build call on the result
    vbytes = int(payload.size)
    bcap = int(L.lvkv_sst_build_blocks_raw_bound(N, kcap, vbytes, 16))
    bneed = L.lvkv_sst_build_blocks_scratch_bytes(N, 16)
    raw, bscratch, raw_off, raw_len = u8(bcap), u8(bneed), i64(N), i32(N)
    brep = torch.zeros(ctypes.sizeof(lvkv.SstBuildReport), dtype=torch.uint8, device=dev)

    def build():
        return L.lvkv_sst_build_blocks_device(
            p(keys), p(koff), p(klen), p(d_payload), p(voff), p(vlen), N, 4096, 16, 1, p(bscratch),
            bneed, p(raw), bcap, p(raw_off), p(raw_len), N, p(brep), stream)

    assert build() == 0
    torch.cuda.synchronize()
    br = lvkv.SstBuildReport.from_buffer_copy(bytes(brep.cpu().numpy())).as_dict()
    assert br["status"] == 0, br
    res["build_blocks_ms"] = timed(build)
    med = lambda xs: float(np.median(xs))
    res["memtable_over_build"] = round(med(res["memtable_ms"]) / med(res["build_blocks_ms"]), 2)
    return res


SHAPES = {"one": 1, "100": 100, "1MiB": (1 << 20) // REC, "all": N}
if "--only" in sys.argv:
    name = sys.argv[sys.argv.index("--only") + 1]
    print(json.dumps({name: measure(name, SHAPES[name], only=True)}))
    sys.exit(0)
out = {"entries": N, "user_key_bytes": KLEN, "value_bytes": VLEN}
for name, per in SHAPES.items():
    out[name] = measure(name, per, tiles=name == "100")
    torch.cuda.empty_cache()
x = torch.from_numpy(rng.integers(0, 1 << 62, N)).to(dev)
out["torch_sort_int64_ms"] = timed(lambda: (torch.sort(x), None)[1])
print(json.dumps(out))
