"""Device time of lvkv_vtable_separate_device, lvkv_vtable_resolve_device and
lvkv_vtable_gather_device on 1 GiB of values cut three ways at the same total
bytes: 1 KiB values, 64 KiB values, and a seeded mix of 1 KiB to 4 MiB
(log-uniform). Keys are 24-byte internal keys; kv_sep_size is 1000, so every
value moves. Beside each cut, in the same run: a device-to-device copy of
table_size bytes (the floor: the call reads and writes every byte once), and
the parent's own way of moving the same value bytes, lvkv_sst_build_blocks_device
on the same entries, unseparated. HIP events around one call, 5 timed calls
after 3. The answers are checked before anything is timed: the whole image
against the inputs for the two uniform cuts, the report's sizes and 256
seeded records and index values against tests/vtable_model.py for the mix.
Then the copy kernel's tile (lvkv_debug_set_vtable_copy_rows: 1, 2, 4, 8
stores a lane) on the 1 KiB cut and the mix, lvkv_vtable_gather_device on the
three cuts, and lvkv_vtable_resolve_device for 1,024 and 262,144 queries. One
JSON line (profiles/vtable_time.json)."""
import ctypes
import json
import sys
from pathlib import Path

import numpy as np
import torch

REPO = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(REPO), str(REPO / "oracle"), str(REPO / "tests")]
import __graft_entry__ as g
import vtable_model as vm

lvkv = g.load_package()
L = lvkv.lib
dev = torch.device("cuda:0")
TOTAL, KLEN, SEP, NUMBER = 1 << 30, 24, 1000, 123456
p = lambda t: ctypes.c_void_p(t.data_ptr())
stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
u8 = lambda n: torch.empty(n, dtype=torch.uint8, device=dev)
i64 = lambda n: torch.empty(n, dtype=torch.int64, device=dev)
i32 = lambda n: torch.empty(n, dtype=torch.int32, device=dev)

d_vals = torch.randint(0, 256, (TOTAL,), dtype=torch.uint8, device=dev,
                       generator=torch.Generator(device=dev).manual_seed(5))


def cut_lengths(name):
    if name == "1KiB":
        return np.full(TOTAL >> 10, 1 << 10, dtype=np.int64)
    if name == "64KiB":
        return np.full(TOTAL >> 16, 1 << 16, dtype=np.int64)
    rng = np.random.default_rng(17)
    lens, left = [], TOTAL
    while left:
        n = min(left, int(2 ** rng.uniform(10, 22)))
        if left - n < 1024:
            n = left
        lens.append(n)
        left -= n
    return np.asarray(lens, dtype=np.int64)


def key_rows(n):
    rows = np.empty((n, KLEN), dtype=np.uint8)
    digits = np.char.zfill(np.arange(n).astype(str), 16)
    rows[:, :16] = np.frombuffer("".join(digits).encode(), dtype=np.uint8).reshape(-1, 16)
    rows[:, 16:] = (((1000 + n - np.arange(n, dtype=np.uint64)) << np.uint64(8)) |
                    np.uint64(1)).astype("<u8").reshape(-1, 1).view(np.uint8)
    return rows


def timed(fn):
    times = []
    for _ in range(8):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        rc = fn()
        b.record()
        torch.cuda.synchronize()
        assert rc in (0, None), rc
        times.append(a.elapsed_time(b))
    return [round(t, 4) for t in times[3:]]


def measure(name, rows_too):
    lens = cut_lengths(name)
    n = len(lens)
    assert int(lens.sum()) == TOTAL
    offs = np.concatenate([[0], np.cumsum(lens)[:-1]])
    keys = key_rows(n)
    d_keys = torch.from_numpy(keys.reshape(-1)).to(dev)
    d_koff = torch.arange(n, dtype=torch.int64, device=dev) * KLEN
    d_klen = torch.full((n,), KLEN, dtype=torch.int32, device=dev)
    d_voff = torch.from_numpy(offs).to(dev)
    d_vlen = torch.from_numpy(lens.astype(np.int32)).to(dev)
    vcap = int(L.lvkv_vtable_separate_vtb_bound(n, n * KLEN, TOTAL))
    ocap = 31 * n + 16
    need = L.lvkv_vtable_separate_scratch_bytes(n)
    vtb, out, scratch = u8(vcap), u8(ocap), u8(need)
    ooff, olen, roff, rsize = i64(n), i32(n), i64(n), i64(n)
    rep = torch.zeros(ctypes.sizeof(lvkv.VtableSeparateReport), dtype=torch.uint8, device=dev)

    def separate():
        return L.lvkv_vtable_separate_device(
            p(d_keys), p(d_koff), p(d_klen), p(d_vals), p(d_voff), p(d_vlen), n, SEP, NUMBER,
            p(scratch), need, p(vtb), vcap, p(out), ocap, p(ooff), p(olen), p(roff), p(rsize),
            p(rep), stream)

    # the answers, before anything is timed
    assert separate() == 0
    torch.cuda.synchronize()
    r = lvkv.VtableSeparateReport.from_buffer_copy(bytes(rep.cpu().numpy())).as_dict()
    sizes = np.asarray([4 + 1 + 16 + len(vm.varint(int(l) - 1)) for l in np.unique(lens)])
    per_len = dict(zip(np.unique(lens).tolist(), sizes.tolist()))
    want_size = int(sum(per_len[int(l)] + int(l) - 1 for l in lens)) if name == "mix" else \
        n * (per_len[int(lens[0])] + int(lens[0]) - 1)
    assert r["status"] == 0 and r["records_num"] == n and r["table_size"] == want_size, r
    ts = r["table_size"]
    if name != "mix":
        vl, rec = int(lens[0]), want_size // n
        hdr = rec - (vl - 1)
        rows = vtb[:ts].view(n, rec)
        assert torch.equal(rows[:, hdr:], d_vals.view(n, vl)[:, 1:])
        head = vm.record(bytes(keys[0, :16]), bytes(vl - 1))[:hdr]
        assert torch.equal(rows[:, 5:21], d_keys.view(n, KLEN)[:, :16])
        for c in list(range(5)) + list(range(21, hdr)):
            assert bool((rows[:, c] == head[c]).all())
    ro, rs = roff.cpu().numpy(), rsize.cpu().numpy()
    oo, ol = ooff.cpu().numpy(), olen.cpu().numpy()
    for i in np.random.default_rng(3).integers(0, n, 256).tolist() + [0, n - 1]:
        v = bytes(d_vals[int(offs[i]):int(offs[i] + lens[i])].cpu().numpy())
        assert bytes(vtb[int(ro[i]):int(ro[i] + rs[i])].cpu().numpy()) == \
            vm.record(bytes(keys[i, :16]), v[1:]), i
        assert bytes(out[int(oo[i]):int(oo[i] + ol[i])].cpu().numpy()) == \
            vm.index_value(NUMBER, int(ro[i]), int(rs[i])), i
    res = {"entries": n, "table_size": ts, "out_val_bytes": r["out_val_bytes"],
           "separate_ms": timed(separate)}

    # the floor: a device-to-device copy of table_size bytes
    src = u8(ts)

    def d2d():
        vtb[:ts].copy_(src)

    res["d2d_copy_ms"] = timed(d2d)
    del src
    if rows_too:
        res["separate_ms_by_rows"] = {}
        for rows_ in (1, 2, 4, 8):
            assert L.lvkv_debug_set_vtable_copy_rows(rows_) == 0
            res["separate_ms_by_rows"][str(rows_)] = timed(separate)
        assert L.lvkv_debug_set_vtable_copy_rows(0) == 0
    assert separate() == 0  # (the copy above overwrote the image)

    # resolve every stored value and gather what it finds
    rneed, gneed = L.lvkv_vtable_resolve_scratch_bytes(n), L.lvkv_vtable_gather_scratch_bytes(n)
    rscratch, gscratch = u8(rneed), u8(gneed)
    st, sr, of, ln = u8(n), u8(n), i64(n), i32(n)
    foff = torch.zeros(1, dtype=torch.int64, device=dev)
    fsize = torch.tensor([ts], dtype=torch.int64, device=dev)
    fnum = torch.tensor([NUMBER], dtype=torch.int64, device=dev)
    rrep = torch.zeros(ctypes.sizeof(lvkv.VtableResolveReport), dtype=torch.uint8, device=dev)

    def resolve(nq):
        return L.lvkv_vtable_resolve_device(
            p(out), p(ooff), p(olen), None, nq, p(vtb), p(foff), p(fsize), p(fnum), 1, p(rscratch),
            rneed, p(st), p(sr), p(of), p(ln), p(rrep), stream)

    assert resolve(n) == 0
    torch.cuda.synchronize()
    rr = lvkv.VtableResolveReport.from_buffer_copy(bytes(rrep.cpu().numpy())).as_dict()
    assert rr["count"][0] == n and rr["total_len"] == TOTAL - n, rr
    res["resolve_all_ms"] = timed(lambda: resolve(n))
    for nq in (1024, 262144):
        if nq <= n:
            res[f"resolve_{nq}_ms"] = timed(lambda: resolve(nq))
    assert resolve(n) == 0
    dst, doff = u8(TOTAL), i64(n + 1)
    grep = torch.zeros(ctypes.sizeof(lvkv.VtableGatherReport), dtype=torch.uint8, device=dev)

    def gather():
        return L.lvkv_vtable_gather_device(
            p(out), p(vtb), p(st), p(sr), p(of), p(ln), n, p(gscratch), gneed, p(dst), TOTAL,
            p(doff), p(grep), stream)

    assert gather() == 0
    torch.cuda.synchronize()
    gr = lvkv.VtableGatherReport.from_buffer_copy(bytes(grep.cpu().numpy())).as_dict()
    assert gr == {"status": 0, "nvalues": n, "dst_bytes": TOTAL - n}, gr
    if name != "mix":
        assert torch.equal(dst[:TOTAL - n].view(n, -1), d_vals.view(n, -1)[:, 1:])
    i = n // 2
    a, b = int(doff[i].cpu()), int(doff[i + 1].cpu())
    assert torch.equal(dst[a:b], d_vals[int(offs[i]) + 1:int(offs[i] + lens[i])])
    res["gather_ms"] = timed(gather)
    del dst, vtb

    # the parent's way of moving the same value bytes: the block builder, unseparated
    bcap = int(L.lvkv_sst_build_blocks_raw_bound(n, n * KLEN, TOTAL, 16))
    bneed = L.lvkv_sst_build_blocks_scratch_bytes(n, 16)
    raw, bscratch, raw_off, raw_len = u8(bcap), u8(bneed), i64(n), i32(n)
    brep = torch.zeros(ctypes.sizeof(lvkv.SstBuildReport), dtype=torch.uint8, device=dev)

    def build():
        return L.lvkv_sst_build_blocks_device(
            p(d_keys), p(d_koff), p(d_klen), p(d_vals), p(d_voff), p(d_vlen), n, 4096, 16, 1,
            p(bscratch), bneed, p(raw), bcap, p(raw_off), p(raw_len), n, p(brep), stream)

    assert build() == 0
    torch.cuda.synchronize()
    br = lvkv.SstBuildReport.from_buffer_copy(bytes(brep.cpu().numpy())).as_dict()
    assert br["status"] == 0, br
    res["build_blocks_unseparated_ms"] = timed(build)
    med = lambda xs: float(np.median(xs))
    res["separate_over_d2d"] = round(med(res["separate_ms"]) / med(res["d2d_copy_ms"]), 3)
    res["build_over_separate"] = round(med(res["build_blocks_unseparated_ms"]) /
                                       med(res["separate_ms"]), 3)
    res["separate_gb_s"] = round((TOTAL + ts) / med(res["separate_ms"]) / 1e6, 1)
    return res


out = {"total_value_bytes": TOTAL, "kv_sep_size": SEP}
for name in ("1KiB", "64KiB", "mix"):
    out[name] = measure(name, name != "64KiB")
    torch.cuda.empty_cache()
spans = {k: (min(out[k]["separate_ms"]), max(out[k]["separate_ms"])) for k in ("1KiB", "64KiB", "mix")}
out["cuts_agree_within_their_spread"] = bool(
    max(lo for lo, _ in spans.values()) <= min(hi for _, hi in spans.values()))
print(json.dumps(out))
