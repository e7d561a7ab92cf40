"""Device time of lvkv_sst_build_blocks_device next to lvkv_sst_write_table_device
(uncompressed) on the blocks it cut, same run, same buffers: 253,952 entries
(internal keys of 24 bytes, half-compressible values of 100), block_size 4096,
restart interval 16 (about 8,192 blocks), Bloom 10 bits a key; HIP events
around one call, 5 timed calls after 3. One JSON line
(profiles/table_build_time.json). --check compares the blocks with the CPU
model's before timing."""
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
need = L.lvkv_sst_build_blocks_scratch_bytes(N, RESTART)
bound = L.lvkv_sst_build_blocks_raw_bound(N, N * KLEN, N * VLEN, RESTART)
scratch = torch.empty(need, dtype=torch.uint8, device=dev)
raw = torch.empty(bound, dtype=torch.uint8, device=dev)
raw_off = torch.empty(N, dtype=torch.int64, device=dev)
raw_len = torch.empty(N, dtype=torch.int32, device=dev)
brep = torch.zeros(ctypes.sizeof(lvkv.SstBuildReport), dtype=torch.uint8, device=dev)


def build():
    return L.lvkv_sst_build_blocks_device(
        p(d_keys), p(d_koff), p(d_klen), p(d_vals), p(d_voff), p(d_vlen), N, BLOCK_SIZE, RESTART,
        1, p(scratch), need, p(raw), bound, p(raw_off), p(raw_len), N, p(brep), stream)


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


assert build() == 0
torch.cuda.synchronize()
r = lvkv.SstBuildReport.from_buffer_copy(bytes(brep.cpu().numpy())).as_dict()
assert r["status"] == 0, r
nb, max_len, mkl, total = r["nblocks"], r["max_block_len"], r["max_key_len"], r["raw_bytes"]
out = {"entries": N, "nblocks": nb, "raw_bytes": total, "max_block_len": max_len}

if "--check" in sys.argv:
    import sst_build_model as bm
    entries = [(keys[i].tobytes(), vals[i].tobytes()) for i in range(N)]
    blocks, offs, want = bm.build(entries, BLOCK_SIZE, RESTART, 1)
    assert r == want, (r, want)
    host = raw.cpu().numpy()
    assert raw_off[:nb].tolist() == offs and raw_len[:nb].tolist() == list(map(len, blocks))
    assert all(host[o:o + len(b)].tobytes() == b for o, b in zip(offs, blocks))
    out["checked"] = True

out["build_ms"] = timed(build)

tneed = L.lvkv_sst_write_table_scratch_bytes(nb, total, max_len, mkl, 10)
cap = L.lvkv_sst_table_file_bound(nb, total, mkl, 10)
tscratch = torch.empty(tneed, dtype=torch.uint8, device=dev)
file = torch.empty(cap, dtype=torch.uint8, device=dev)
hoff = torch.empty(nb, dtype=torch.int64, device=dev)
hsize = torch.empty(nb, dtype=torch.int32, device=dev)
typ = torch.empty(nb, dtype=torch.uint8, device=dev)
st = torch.empty(nb, dtype=torch.uint8, device=dev)
trep = torch.zeros(ctypes.sizeof(lvkv.SstTableReport), dtype=torch.uint8, device=dev)


def table():
    return L.lvkv_sst_write_table_device(
        p(raw), p(raw_off), p(raw_len), nb, 0, 1, max_len, 1, 10, mkl, p(tscratch), tneed,
        p(file), cap, p(hoff), p(hsize), p(typ), p(st), p(trep), stream)


out["table_c0_ms"] = timed(table)
t = lvkv.SstTableReport.from_buffer_copy(bytes(trep.cpu().numpy())).as_dict()
assert t["status"] == 0 and t["num_entries"] == N, t
out["file_size"] = t["file_size"]
print(json.dumps(out))
