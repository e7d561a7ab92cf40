"""Device time of lvkv_sst_scan_entries_device on the workload of
tools/table_merge_bench.py (253,952 internal keys of 24 bytes in order, a user
key a hundred with an older version, which the newer one hides from a reader
at the snapshot), with 1, 1,024 and 262,144 ranges: a start on a seeded user
key, or just past one, a limit sixteen user keys on (one range in four has
none and a maximum of 16 instead). In the same run on the same buffers the
yardstick: lvkv_sst_merge_entries_device with LVKV_MERGE_COMPACT over them as
one run. The answers are checked against numpy before anything is timed. HIP
events around one call, 5 timed calls after 3. One JSON line, also written to
--out (default profiles/scan_time.json). --once NQ runs the scan with NQ
ranges and the merge once each after a warm-up, for a kernel trace."""
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
N, KLEN, VLEN, ULEN = 253952, 24, 100, 16
SNAPSHOT = 1 << 30
# entry i: user key i - (i % 100 == 1), so that entries 100j and 100j + 1 are
# two versions of one user key, the newer first
users = np.arange(N) - (np.arange(N) % 100 == 1)
keys = np.empty((N, KLEN), dtype=np.uint8)
for i in range(N):
    keys[i] = np.frombuffer(b"%016d" % (users[i] * 3) + ((1000 + N - i) << 8 | 1).to_bytes(8, "little"),
                            dtype=np.uint8)
hidden = np.arange(N) % 100 == 1
visible = np.nonzero(~hidden)[0]
vis_users = users[visible] * 3  # the visible entries' user keys as numbers, ascending

p = lambda t: ctypes.c_void_p(t.data_ptr())
stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
u8 = lambda n: torch.empty(n, dtype=torch.uint8, device=dev)
i64 = lambda n: torch.empty(n, dtype=torch.int64, device=dev)
i32 = lambda n: torch.empty(n, dtype=torch.int32, device=dev)
d_keys = torch.from_numpy(keys.reshape(-1)).to(dev)
d_vals = u8(N * VLEN)
d_koff = torch.arange(N, dtype=torch.int64, device=dev) * KLEN
d_voff = torch.arange(N, dtype=torch.int64, device=dev) * VLEN
d_klen = torch.full((N,), KLEN, dtype=torch.int32, device=dev)
d_vlen = torch.full((N,), VLEN, dtype=torch.int32, device=dev)
o_koff, o_klen, o_voff, o_vlen, o_src, o_drop = i64(N), i32(N), i64(N), i32(N), i32(N), i32(N)
d_first = torch.tensor([0, N], dtype=torch.int64, device=dev)
mneed = L.lvkv_sst_merge_entries_scratch_bytes(N, 1)
mscratch = u8(mneed)
mrep = torch.zeros(ctypes.sizeof(lvkv.SstMergeReport), dtype=torch.uint8, device=dev)
srep = torch.zeros(ctypes.sizeof(lvkv.SstScanReport), dtype=torch.uint8, device=dev)


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


def merge():
    return L.lvkv_sst_merge_entries_device(
        p(d_keys), p(d_koff), p(d_klen), p(d_vals), p(d_voff), p(d_vlen), N, p(d_first), 1, 1,
        lvkv.MERGE_COMPACT, SNAPSHOT, None, None, None, 0, p(mscratch), mneed, p(o_koff),
        p(o_klen), p(o_voff), p(o_vlen), p(o_src), N, p(o_drop), p(mrep), stream)


def scan_with(nq):
    """(the call, a check of its answers) for nq seeded ranges."""
    rng = np.random.default_rng(nq)
    at = rng.integers(0, N, nq)
    past = rng.integers(0, 2, nq).astype(np.int64)  # 1: the start lies just past the user key
    start = users[at] * 3 + past
    no_limit = np.arange(nq) % 4 == 3
    limit = start + 48
    qk = np.empty((nq, 2, ULEN), dtype=np.uint8)
    for q in range(nq):
        qk[q, 0] = np.frombuffer(b"%016d" % start[q], dtype=np.uint8)
        qk[q, 1] = np.frombuffer(b"%016d" % limit[q], dtype=np.uint8)
    d_qk = torch.from_numpy(qk.reshape(-1)).to(dev)
    d_soff = torch.arange(nq, dtype=torch.int64, device=dev) * (2 * ULEN)
    d_loff = d_soff + ULEN
    d_slen = torch.full((nq,), ULEN, dtype=torch.int32, device=dev)
    d_llen = torch.from_numpy(np.where(no_limit, -1, ULEN).astype(np.int32)).to(dev)
    d_max = torch.from_numpy(np.where(no_limit, 16, -1).astype(np.int32)).to(dev)
    need = L.lvkv_sst_scan_entries_scratch_bytes(N, nq)
    scratch = u8(need)
    q_first, q_count, q_status = i32(nq), i32(nq), u8(nq)

    def call():
        return L.lvkv_sst_scan_entries_device(
            p(d_keys), p(d_koff), p(d_klen), p(d_voff), p(d_vlen), N, SNAPSHOT, p(d_qk), p(d_soff),
            p(d_slen), p(d_loff), p(d_llen), p(d_max), nq, p(scratch), need, p(o_koff), p(o_klen),
            p(o_voff), p(o_vlen), p(o_src), N, p(q_first), p(q_count), p(q_status), p(srep), stream)

    def check():
        assert call() == 0
        torch.cuda.synchronize()
        r = lvkv.SstScanReport.from_buffer_copy(bytes(srep.cpu().numpy())).as_dict()
        assert r["status"] == 0 and r["num_visible"] == visible.size, r
        assert r["num_hidden"] == int(hidden.sum()) and r["nqueries"] == nq, r
        assert (o_src[:visible.size].cpu().numpy() == visible).all()
        assert (o_klen[:visible.size].cpu().numpy() == ULEN).all()
        first = np.searchsorted(vis_users, start, side="left")
        end = np.where(no_limit, np.minimum(first + 16, visible.size),
                       np.searchsorted(vis_users, limit, side="left"))
        assert (q_first.cpu().numpy() == first).all()
        assert (q_count.cpu().numpy() == end - first).all()
        assert (q_status.cpu().numpy() == 0).all()
        assert r["sum_count"] == int((end - first).sum()) and r["max_count"] == int((end - first).max())
        return need

    return call, check


out_path = Path(sys.argv[sys.argv.index("--out") + 1]) if "--out" in sys.argv else \
    REPO / "profiles" / "scan_time.json"
once = int(sys.argv[sys.argv.index("--once") + 1]) if "--once" in sys.argv else None
out = {"entries": N, "visible": int(visible.size), "checked": True}
assert merge() == 0
torch.cuda.synchronize()
m = lvkv.SstMergeReport.from_buffer_copy(bytes(mrep.cpu().numpy())).as_dict()
assert m["status"] == 0 and m["num_hidden"] == int(hidden.sum()) and m["num_out"] == visible.size, m
assert (o_src[:visible.size].cpu().numpy() == visible).all()
for nq in [once] if once is not None else [1, 1024, 262144]:
    call, check = scan_with(nq)
    out[f"scan_{nq}_scratch_bytes"] = check()
    out[f"scan_{nq}_ms"] = timed(call, once is not None)
out["merge_compact_1_run_ms"] = timed(merge, once is not None)
out["merge_scratch_bytes"] = mneed
print(json.dumps(out))
if once is None:
    out_path.parent.mkdir(parents=True, exist_ok=True)
    out_path.write_text(json.dumps(out) + "\n")
