"""Device time of lvkv_sst_read_entries_device on the 7,055 blocks
tools/table_build_bench.py cuts from its 253,952 entries (internal keys of 24
bytes, half-compressible values of 100, block_size 4096, interval 16), and in
the same run on the same buffers its two yardsticks: lvkv_sst_build_blocks_device
on the entries just produced (the values read from the blocks where the walk
left them), and a device-to-device copy of the blocks' bytes. HIP events
around one call, 5 timed calls after 3. One JSON line
(profiles/table_read_time.json). --check compares the entries with the input
and the rebuilt blocks with the first ones before timing."""
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
rng = np.random.default_rng(11)
N, KLEN, VLEN, BLOCK_SIZE, RESTART = 253952, 24, 100, 4096, 16
keys = np.empty((N, KLEN), dtype=np.uint8)
for i in range(N):
    keys[i] = np.frombuffer(b"%016d" % (i * 3) + ((1000 + i) << 8 | 1).to_bytes(8, "little"),
                            dtype=np.uint8)
half = rng.integers(32, 127, size=(N, VLEN // 2), dtype=np.uint8)
vals = np.concatenate([half, half], axis=1)
d_keys, d_vals = torch.from_numpy(keys.reshape(-1)).to(dev), torch.from_numpy(vals.reshape(-1)).to(dev)
d_koff = torch.arange(N, dtype=torch.int64, device=dev) * KLEN
d_voff = torch.arange(N, dtype=torch.int64, device=dev) * VLEN
d_klen = torch.full((N,), KLEN, dtype=torch.int32, device=dev)
d_vlen = torch.full((N,), VLEN, dtype=torch.int32, device=dev)

p = lambda t: ctypes.c_void_p(t.data_ptr())
stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
u8 = lambda n: torch.empty(n, dtype=torch.uint8, device=dev)
i64 = lambda n: torch.empty(n, dtype=torch.int64, device=dev)
i32 = lambda n: torch.empty(n, dtype=torch.int32, device=dev)
bneed = L.lvkv_sst_build_blocks_scratch_bytes(N, RESTART)
bound = L.lvkv_sst_build_blocks_raw_bound(N, N * KLEN, N * VLEN, RESTART)
bscratch = u8(bneed)
brep = torch.zeros(ctypes.sizeof(lvkv.SstBuildReport), dtype=torch.uint8, device=dev)


def build(k, ko, kl, v, vo, vl, raw, raw_off, raw_len):
    return L.lvkv_sst_build_blocks_device(
        p(k), p(ko), p(kl), p(v), p(vo), p(vl), N, BLOCK_SIZE, RESTART, 1, p(bscratch), bneed,
        p(raw), bound, p(raw_off), p(raw_len), N, p(brep), stream)


def timed(fn):
    times = []
    for _ in range(8):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        assert fn() == 0
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b))
    return [round(t, 3) for t in times[3:]]


# the blocks the read side starts from
raw, raw_off, raw_len = u8(bound), i64(N), i32(N)
assert build(d_keys, d_koff, d_klen, d_vals, d_voff, d_vlen, raw, raw_off, raw_len) == 0
torch.cuda.synchronize()
r = lvkv.SstBuildReport.from_buffer_copy(bytes(brep.cpu().numpy())).as_dict()
assert r["status"] == 0, r
nb, total = r["nblocks"], r["raw_bytes"]
out = {"entries": N, "nblocks": nb, "raw_bytes": total}

eneed = L.lvkv_sst_read_entries_scratch_bytes(nb, total)
escratch = u8(eneed)
e_keys, e_koff, e_klen, e_voff, e_vlen = u8(N * KLEN), i64(N), i32(N), i64(N), i32(N)
first, bstatus = i64(nb + 1), u8(nb)
erep = torch.zeros(ctypes.sizeof(lvkv.SstEntriesReport), dtype=torch.uint8, device=dev)


def read():
    return L.lvkv_sst_read_entries_device(
        p(raw), p(raw_off), p(raw_len), None, nb, p(escratch), eneed, p(e_keys), N * KLEN,
        p(e_koff), p(e_klen), p(e_voff), p(e_vlen), N, p(first), p(bstatus), p(erep), stream)


assert read() == 0
torch.cuda.synchronize()
e = lvkv.SstEntriesReport.from_buffer_copy(bytes(erep.cpu().numpy())).as_dict()
assert e["status"] == 0 and e["nbad"] == 0 and e["num_entries"] == N, e
out["scratch_bytes"] = eneed

# the yardsticks' buffers: the rebuilt blocks, the copy
raw2, raw_off2, raw_len2 = u8(bound), i64(N), i32(N)
copy_dst = u8(total)


def rebuild():
    return build(e_keys, e_koff, e_klen, raw, e_voff, e_vlen, raw2, raw_off2, raw_len2)


def copy():
    copy_dst.copy_(raw[:total])
    return 0


if "--check" in sys.argv:
    assert torch.equal(e_keys, d_keys) and torch.equal(e_koff, d_koff)
    assert torch.equal(e_klen, d_klen) and torch.equal(e_vlen, d_vlen)
    host = raw.cpu().numpy()
    voff = e_voff.cpu().numpy()
    for i in range(0, N, 997):
        assert host[voff[i]:voff[i] + VLEN].tobytes() == vals[i].tobytes(), i
    assert rebuild() == 0
    torch.cuda.synchronize()
    r2 = lvkv.SstBuildReport.from_buffer_copy(bytes(brep.cpu().numpy())).as_dict()
    assert r2 == r, (r2, r)
    assert torch.equal(raw_off2[:nb], raw_off[:nb]) and torch.equal(raw_len2[:nb], raw_len[:nb])
    host2, offs, lens = raw2.cpu().numpy(), raw_off[:nb].tolist(), raw_len[:nb].tolist()
    assert all((host[o:o + n] == host2[o:o + n]).all() for o, n in zip(offs, lens))
    out["checked"] = True

out["read_entries_ms"] = timed(read)
out["build_ms"] = timed(rebuild)
out["copy_d2d_ms"] = timed(copy)
print(json.dumps(out))
