"""Device time of lvkv_sst_merge_entries_device on the workload of
tools/table_build_bench.py (253,952 internal keys of 24 bytes,
half-compressible values of 100) split into 2 and into 5 sorted runs, by
residue (entry i in run i % K: every bisection ends deep) and by contiguous
ranges (every bisection ends at a run's edge), with LVKV_MERGE_COMPACT (a
user key a hundred has an older version, which the snapshot hides). The runs
are laid out run after run, keys and values moved with them, so the merged
order is not the order of the bytes. In the same run on the same buffers the
two yardsticks: lvkv_sst_build_blocks_device on the merge's output (keys and
values read in merged order from where the runs left them), and
lvkv_sst_read_entries_device on the blocks that gives. HIP events around one
call, 5 timed calls after 3. One JSON line (profiles/table_merge_time.json).
--check compares the merged order and the drops with the input before timing;
--split NAME --once runs one split's three calls once each after a warm-up,
for a kernel trace."""
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
SNAPSHOT = 1 << 30
# entry i: user key i - (i % 100 == 1), so that entries 100j and 100j + 1 are
# two versions of one user key, the newer first
keys = np.empty((N, KLEN), dtype=np.uint8)
for i in range(N):
    user = i - 1 if i % 100 == 1 else i
    keys[i] = np.frombuffer(b"%016d" % (user * 3) + ((1000 + N - i) << 8 | 1).to_bytes(8, "little"),
                            dtype=np.uint8)
hidden = np.arange(N) % 100 == 1
half = rng.integers(32, 127, size=(N, VLEN // 2), dtype=np.uint8)
vals = np.concatenate([half, half], axis=1)

p = lambda t: ctypes.c_void_p(t.data_ptr())
stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
u8 = lambda n: torch.empty(n, dtype=torch.uint8, device=dev)
i64 = lambda n: torch.empty(n, dtype=torch.int64, device=dev)
i32 = lambda n: torch.empty(n, dtype=torch.int32, device=dev)
d_koff = torch.arange(N, dtype=torch.int64, device=dev) * KLEN
d_voff = torch.arange(N, dtype=torch.int64, device=dev) * VLEN
d_klen = torch.full((N,), KLEN, dtype=torch.int32, device=dev)
d_vlen = torch.full((N,), VLEN, dtype=torch.int32, device=dev)

mneed = L.lvkv_sst_merge_entries_scratch_bytes(N, 5)
mscratch = u8(mneed)
o_koff, o_klen, o_voff, o_vlen, o_src, o_drop = i64(N), i32(N), i64(N), i32(N), i32(N), i32(N)
mrep = torch.zeros(ctypes.sizeof(lvkv.SstMergeReport), dtype=torch.uint8, device=dev)
bneed = L.lvkv_sst_build_blocks_scratch_bytes(N, RESTART)
bound = L.lvkv_sst_build_blocks_raw_bound(N, N * KLEN, N * VLEN, RESTART)
bscratch = u8(bneed)
raw, raw_off, raw_len = u8(bound), i64(N), i32(N)
brep = torch.zeros(ctypes.sizeof(lvkv.SstBuildReport), dtype=torch.uint8, device=dev)
e_keys, e_koff, e_klen, e_voff, e_vlen = u8(N * KLEN), i64(N), i32(N), i64(N), i32(N)
erep = torch.zeros(ctypes.sizeof(lvkv.SstEntriesReport), dtype=torch.uint8, device=dev)


def split(k, by_residue):
    """The input index of each entry of the runs laid end to end, and run_first."""
    idx = np.arange(N)
    run = idx % k if by_residue else idx * k // N
    perm = np.argsort(run, kind="stable")
    first = np.concatenate([[0], np.cumsum(np.bincount(run, minlength=k))])
    return perm, first


def timed(fn, once):
    times = []
    for _ in range(2 if once else 8):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        assert fn() == 0
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b))
    return [round(t, 3) for t in times[1 if once else 3:]]


def measure(k, by_residue, check, once):
    perm, first = split(k, by_residue)
    d_keys = torch.from_numpy(keys[perm].reshape(-1)).to(dev)
    d_vals = torch.from_numpy(vals[perm].reshape(-1)).to(dev)
    d_first = torch.from_numpy(first.astype(np.int64)).to(dev)

    def merge():
        return L.lvkv_sst_merge_entries_device(
            p(d_keys), p(d_koff), p(d_klen), p(d_vals), p(d_voff), p(d_vlen), N, p(d_first), k, 1,
            lvkv.MERGE_COMPACT, SNAPSHOT, None, None, None, 0, p(mscratch), mneed, p(o_koff),
            p(o_klen), p(o_voff), p(o_vlen), p(o_src), N, p(o_drop), p(mrep), stream)

    assert merge() == 0
    torch.cuda.synchronize()
    m = lvkv.SstMergeReport.from_buffer_copy(bytes(mrep.cpu().numpy())).as_dict()
    assert m["status"] == 0 and m["num_hidden"] == int(hidden.sum()) and m["num_obsolete"] == 0, m
    no = m["num_out"]
    assert no == N - m["num_hidden"]
    if check:
        src, drop = o_src[:no].cpu().numpy(), o_drop[:N - no].cpu().numpy()
        assert (perm[src] == np.nonzero(~hidden)[0]).all()
        assert (perm[drop] == np.nonzero(hidden)[0]).all()
        assert (o_koff[:no].cpu().numpy() == src.astype(np.int64) * KLEN).all()

    def build():
        return L.lvkv_sst_build_blocks_device(
            p(d_keys), p(o_koff), p(o_klen), p(d_vals), p(o_voff), p(o_vlen), no, BLOCK_SIZE,
            RESTART, 1, p(bscratch), bneed, p(raw), bound, p(raw_off), p(raw_len), N, p(brep),
            stream)

    assert build() == 0
    torch.cuda.synchronize()
    b = lvkv.SstBuildReport.from_buffer_copy(bytes(brep.cpu().numpy())).as_dict()
    assert b["status"] == 0 and b["num_entries"] == no, b
    nb, total = b["nblocks"], b["raw_bytes"]
    eneed = L.lvkv_sst_read_entries_scratch_bytes(nb, total)
    escratch = u8(eneed)
    e_first, e_status = i64(nb + 1), u8(nb)

    def read():
        return L.lvkv_sst_read_entries_device(
            p(raw), p(raw_off), p(raw_len), None, nb, p(escratch), eneed, p(e_keys), N * KLEN,
            p(e_koff), p(e_klen), p(e_voff), p(e_vlen), N, p(e_first), p(e_status), p(erep),
            stream)

    assert read() == 0
    torch.cuda.synchronize()
    e = lvkv.SstEntriesReport.from_buffer_copy(bytes(erep.cpu().numpy())).as_dict()
    assert e["status"] == 0 and e["nbad"] == 0 and e["num_entries"] == no, e
    if check:
        got = e_keys[:no * KLEN].cpu().numpy().reshape(no, KLEN)
        assert (got == keys[~hidden]).all()
    return {"runs": k, "by": "residue" if by_residue else "ranges", "num_out": no, "nblocks": nb,
            "merge_ms": timed(merge, once), "build_on_merged_ms": timed(build, once),
            "read_entries_ms": timed(read, once)}


SPLITS = {"2_residue": (2, True), "2_ranges": (2, False), "5_residue": (5, True),
          "5_ranges": (5, False)}
once = "--once" in sys.argv
names = [sys.argv[sys.argv.index("--split") + 1]] if "--split" in sys.argv else list(SPLITS)
out = {"entries": N, "scratch_bytes": mneed, "checked": "--check" in sys.argv}
for name in names:
    out[name] = measure(*SPLITS[name], "--check" in sys.argv, once)
print(json.dumps(out))
