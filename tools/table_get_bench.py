"""Device time of lvkv_sst_get_locate_device and lvkv_sst_get_seek_device on
the table of tools/table_build_bench.py (253,952 internal keys of 24 bytes,
half-compressible values of 100, block size 4096, restart interval 16, bloom
filter of 10 bits a key): batches of 1,024 and 262,144 lookups, all present,
all absent and half each, the keys drawn by seed and asked for in random order
and sorted; the all-absent batches without the filter block as well, where
every query goes on to a data block. The decoded blocks are all resident (the
build call's output is the read call's), so the seek call's time is the seek
alone. In the same run lvkv_sst_read_entries_device over the whole table: the
only way to answer a lookup without these calls. HIP events around one call,
5 timed calls after 3. One JSON line (profiles/table_get_time.json). --check
compares every answer with the keys the table was built from before timing;
--case NAME --once runs one case's two calls once each after a warm-up, for a
kernel trace."""
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
N, KLEN, VLEN, BLOCK_SIZE, RESTART, BITS = 253952, 24, 100, 4096, 16, 10
MAX_TAG = ((1 << 56) - 1) << 8 | 1  # LookupKey at kMaxSequenceNumber
rng = np.random.default_rng(11)


def key_rows(users, tags):
    """24-byte internal keys: 16 decimal digits, then the tag."""
    rows = np.empty((len(users), KLEN), dtype=np.uint8)
    digits = np.char.zfill(users.astype(str), 16)
    rows[:, :16] = np.frombuffer("".join(digits).encode(), dtype=np.uint8).reshape(-1, 16)
    rows[:, 16:] = np.asarray(tags, dtype="<u8").reshape(-1, 1).view(np.uint8)
    return rows


entry = np.arange(N, dtype=np.int64)
keys = key_rows(entry * 3, ((1000 + N - entry) << 8) | 1)
half = rng.integers(32, 127, size=(N, VLEN // 2), dtype=np.uint8)
vals = np.concatenate([half, half], axis=1)

p = lambda t: ctypes.c_void_p(t.data_ptr())
stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
u8 = lambda n: torch.empty(n, dtype=torch.uint8, device=dev)
i64 = lambda n: torch.empty(n, dtype=torch.int64, device=dev)
i32 = lambda n: torch.empty(n, dtype=torch.int32, device=dev)

# the table: data blocks by the build call, then the image for its index and filter
d_keys = torch.from_numpy(keys.reshape(-1)).to(dev)
d_vals = torch.from_numpy(vals.reshape(-1)).to(dev)
d_koff = torch.arange(N, dtype=torch.int64, device=dev) * KLEN
d_voff = torch.arange(N, dtype=torch.int64, device=dev) * VLEN
d_klen = torch.full((N,), KLEN, dtype=torch.int32, device=dev)
d_vlen = torch.full((N,), VLEN, dtype=torch.int32, device=dev)
raw, raw_off, raw_len, build = lvkv.sst_build_blocks(
    d_keys, d_koff, d_klen, d_vals, d_voff, d_vlen, block_size=BLOCK_SIZE,
    restart_interval=RESTART, key_format=1)
assert build["status"] == 0, build
nb = build["nblocks"]
raw_off, raw_len = raw_off[:nb].contiguous(), raw_len[:nb].contiguous()
file, hoff, hsize, _, _, table = lvkv.sst_write_table(
    raw, raw_off, raw_len, compression=0, max_len=build["max_block_len"], key_format=1,
    filter_bits_per_key=BITS, max_key_len=build["max_key_len"])
assert table["status"] == 0, table
file = file[:table["file_size"]].contiguous()
opened, v_off, v_size, _, v_status = lvkv.sst_verify_table(file, filter_policy=lvkv.BLOOM_POLICY)
assert opened["status"] == 0 and opened["ndata"] == nb and opened["has_filter"] == 1, opened
at, size = opened["index_offset"], opened["index_size"]
index = file[at:at + size].clone()
at, size = int(v_off[nb].cpu()), int(v_size[nb].cpu())
filt = file[at:at + size].clone()
hoff = hoff[:nb].contiguous()

MAXQ = 262144
lneed = L.lvkv_sst_get_locate_scratch_bytes(index.numel(), MAXQ)
sneed = L.lvkv_sst_get_seek_scratch_bytes(MAXQ)
lscratch, sscratch = u8(lneed), u8(sneed)
lrep = torch.zeros(ctypes.sizeof(lvkv.SstGetLocateReport), dtype=torch.uint8, device=dev)
srep = torch.zeros(ctypes.sizeof(lvkv.SstGetSeekReport), dtype=torch.uint8, device=dev)


def timed(fn, once):
    times = []
    for _ in range(2 if once else 8):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        assert fn() == 0
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b))
    return [round(t, 4) for t in times[1 if once else 3:]]


def measure(nq, mix, in_order, with_filter, check, once):
    r = np.random.default_rng(nq + 7 * len(mix))
    which = r.integers(0, N, size=nq)
    present = {"present": np.ones(nq, bool), "absent": np.zeros(nq, bool),
               "half": np.arange(nq) % 2 == 0}[mix]
    r.shuffle(present)
    if in_order:
        which = np.sort(which)
    q = key_rows(which * 3 + ~present, np.full(nq, MAX_TAG, dtype=np.uint64))
    d_q = torch.from_numpy(q.reshape(-1)).to(dev)
    q_off = torch.arange(nq, dtype=torch.int64, device=dev) * KLEN
    q_len = torch.full((nq,), KLEN, dtype=torch.int32, device=dev)
    q_block, q_hoff, q_hsize, q_status = i32(nq), i64(nq), i32(nq), u8(nq)
    hit, voff, vlen, tag, state = i32(nq), i64(nq), i32(nq), i64(nq), u8(nq)

    def locate():
        return L.lvkv_sst_get_locate_device(
            p(index), index.numel(), p(filt) if with_filter else None, filt.numel(), p(d_q),
            p(q_off), p(q_len), nq, 1, p(lscratch), lneed, p(q_block), p(q_hoff), p(q_hsize),
            p(q_status), p(lrep), stream)

    assert locate() == 0
    torch.cuda.synchronize()
    lr = lvkv.SstGetLocateReport.from_buffer_copy(bytes(lrep.cpu().numpy())).as_dict()
    # the caller's mapping: every block is resident, block b in slot b
    slot = torch.where(q_status == lvkv.GET_BLOCK, q_block, torch.full_like(q_block, -1))
    assert bool((hoff[q_block[q_status == lvkv.GET_BLOCK].long()] ==
                 q_hoff[q_status == lvkv.GET_BLOCK]).all())

    def seek():
        return L.lvkv_sst_get_seek_device(
            p(raw), p(raw_off), p(raw_len), None, nb, p(d_q), p(q_off), p(q_len), p(slot), nq, 1,
            p(sscratch), sneed, p(hit), p(voff), p(vlen), p(tag), p(state), p(srep), stream)

    assert seek() == 0
    torch.cuda.synchronize()
    sr = lvkv.SstGetSeekReport.from_buffer_copy(bytes(srep.cpu().numpy())).as_dict()
    assert sr["count"][lvkv.GET_STATE_FOUND] == int(present.sum()), (sr, int(present.sum()))
    assert sr["count"][lvkv.GET_STATE_NOT_FOUND] == nq - int(present.sum()), sr
    assert lr["count"][lvkv.GET_BLOCK] >= int(present.sum()), lr
    if check:
        st, vo = state.cpu().numpy(), voff.cpu().numpy()
        assert ((st == lvkv.GET_STATE_FOUND) == present).all()
        got = raw[torch.from_numpy(vo[present][:, None] + np.arange(VLEN)).to(dev)].cpu().numpy()
        assert (got == vals[which[present]]).all()
        assert (tag.cpu().numpy()[present] == ((1000 + N - which[present]) << 8 | 1)).all()
    return {"queries": nq, "mix": mix, "order": "sorted" if in_order else "random",
            "filter": with_filter, "to_block": lr["count"][lvkv.GET_BLOCK],
            "filtered": lr["count"][lvkv.GET_FILTERED], "found": sr["count"][lvkv.GET_STATE_FOUND],
            "locate_ms": timed(locate, once), "seek_ms": timed(seek, once)}


def read_whole_table(once):
    eneed = L.lvkv_sst_read_entries_scratch_bytes(nb, build["raw_bytes"])
    escratch = u8(eneed)
    e_keys, e_koff, e_klen, e_voff, e_vlen = u8(N * KLEN), i64(N), i32(N), i64(N), i32(N)
    e_first, e_status = i64(nb + 1), u8(nb)
    erep = torch.zeros(ctypes.sizeof(lvkv.SstEntriesReport), dtype=torch.uint8, device=dev)

    def read():
        return L.lvkv_sst_read_entries_device(
            p(raw), p(raw_off), p(raw_len), None, nb, p(escratch), eneed, p(e_keys), N * KLEN,
            p(e_koff), p(e_klen), p(e_voff), p(e_vlen), N, p(e_first), p(e_status), p(erep),
            stream)

    assert read() == 0
    torch.cuda.synchronize()
    e = lvkv.SstEntriesReport.from_buffer_copy(bytes(erep.cpu().numpy())).as_dict()
    assert e["status"] == 0 and e["nbad"] == 0 and e["num_entries"] == N, e
    return timed(read, once)


CASES = {}
for nq in (1024, 262144):
    for mix in ("present", "absent", "half"):
        for in_order in (False, True):
            CASES[f"{nq}_{mix}_{'sorted' if in_order else 'random'}"] = (nq, mix, in_order, True)
for in_order in (False, True):
    CASES[f"262144_absent_{'sorted' if in_order else 'random'}_nofilter"] = \
        (262144, "absent", in_order, False)
once = "--once" in sys.argv
names = [sys.argv[sys.argv.index("--case") + 1]] if "--case" in sys.argv else list(CASES)
out = {"entries": N, "nblocks": nb, "index_bytes": index.numel(), "filter_bytes": filt.numel(),
       "locate_scratch_bytes": lneed, "seek_scratch_bytes": sneed, "checked": "--check" in sys.argv}
for name in names:
    out[name] = measure(*CASES[name], "--check" in sys.argv, once)
out["read_entries_whole_table_ms"] = read_whole_table(once)
print(json.dumps(out))
