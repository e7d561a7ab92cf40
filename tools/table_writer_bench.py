"""Device time of lvkv_sst_write_table_device next to the data blocks' writer
alone (lvkv_sst_write_blocks_status_device), same blocks, same buffers:
8,192 blocks of 31 entries (internal keys of 24 bytes, half-compressible
values of 100), restart interval 16, Bloom 10 bits a key; compression 0, 1 and
2 (level 1); HIP events around one call, 5 timed calls after 3. One JSON line
(profiles/table_writer_time.json)."""
import ctypes
import json
import sys
from pathlib import Path

import numpy as np
import torch

REPO = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(REPO), str(REPO / "oracle"), str(REPO / "tests")]
import __graft_entry__ as g
import sst_finish_model as fm

lvkv = g.load_package()
L = lvkv.lib
dev = torch.device("cuda:0")
rng = np.random.default_rng(11)
N = 8192
blocks, i = [], 0
for b in range(N):
    entries = []
    for _ in range(31):
        piece = rng.integers(32, 127, size=50, dtype=np.uint8).tobytes()
        entries.append((b"%016d" % (i * 3) + ((1000 + i) << 8 | 1).to_bytes(8, "little"), piece * 2))
        i += 1
    blocks.append(fm.block_of(entries, 16))
lens = np.array([len(b) for b in blocks], dtype=np.int32)
offs = np.concatenate([[0], np.cumsum(lens[:-1], dtype=np.int64)]).astype(np.int64)
raw = torch.from_numpy(np.frombuffer(b"".join(blocks), dtype=np.uint8).copy()).to(dev)
d_off, d_len = torch.from_numpy(offs).to(dev), torch.from_numpy(lens).to(dev)
total, max_len, mkl = int(lens.sum()), int(lens.max()), 24
p = lambda t: ctypes.c_void_p(t.data_ptr())
stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
out = {"nblocks": N, "total_raw_bytes": total, "entries": i}
for compression in (0, 1, 2):
    need = L.lvkv_sst_write_table_scratch_bytes(N, total, max_len, mkl, 10)
    cap = L.lvkv_sst_table_file_bound(N, total, mkl, 10)
    scratch = torch.empty(need, dtype=torch.uint8, device=dev)
    file = torch.empty(cap, dtype=torch.uint8, device=dev)
    hoff = torch.empty(N, dtype=torch.int64, device=dev)
    hsize = torch.empty(N, dtype=torch.int32, device=dev)
    typ = torch.empty(N, dtype=torch.uint8, device=dev)
    st = torch.empty(N, dtype=torch.uint8, device=dev)
    end = torch.empty(1, dtype=torch.int64, device=dev)
    rep = torch.zeros(ctypes.sizeof(lvkv.SstTableReport), dtype=torch.uint8, device=dev)

    def blocks_only():
        return L.lvkv_sst_write_blocks_status_device(
            p(raw), p(d_off), p(d_len), N, compression, 1, max_len, p(scratch), p(file), 0, p(hoff),
            p(hsize), p(typ), p(end), need, p(st), stream)

    def table():
        return L.lvkv_sst_write_table_device(
            p(raw), p(d_off), p(d_len), N, compression, 1, max_len, 1, 10, mkl, p(scratch), need,
            p(file), cap, p(hoff), p(hsize), p(typ), p(st), p(rep), stream)

    for name, fn in (("blocks", blocks_only), ("table", table)):
        times = []
        for it in range(8):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            assert fn() == 0
            b.record()
            torch.cuda.synchronize()
            times.append(a.elapsed_time(b))
        out[f"c{compression}_{name}_ms"] = [round(t, 3) for t in times[3:]]
    r = lvkv.SstTableReport.from_buffer_copy(bytes(rep.cpu().numpy())).as_dict()
    assert r["status"] == 0, r
    out[f"c{compression}_file_size"] = r["file_size"]
print(json.dumps(out))
