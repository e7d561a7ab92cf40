"""MI355X batched CRC32C engine for ArcueidType/LevelDB-KV-Separation.

Host-side mirror of the reference's checksum interface (util/crc32c.h:17-38)
over the C-ABI in include/lvkv_crc32c.h, plus the batched device API that the
SST writer/reader (table/table_builder.cc:199-203, table/format.cc:92-99) and
WAL writer/reader (db/log_writer.cc:94-95, db/log_reader.cc:243-257) checksum
paths map onto.

The package directory name contains dashes, so import it through
``load()`` (or ``importlib``); it registers itself as
``leveldb_kv_separation_amd``. Every call goes to the native library
``liblvkv_crc32c.so``; if it is missing, importing fails loudly — there is no
Python or CPU fallback for the batch (GPU) path.
"""
from __future__ import annotations

import ctypes
from pathlib import Path
from typing import Optional, Tuple

__all__ = [
    "Extend", "Value", "Mask", "Unmask", "kMaskDelta",
    "crc32c_batch", "crc32c_uniform", "sst_verify", "log_verify",
    "crc32c_batch_host", "LvkvError", "lib", "LIB_PATH", "device_groups", "Engine",
]

LIB_PATH = Path(__file__).resolve().parent / "liblvkv_crc32c.so"
kMaskDelta = 0xA282EAD8  # util/crc32c.h:22

LVKV_OK = 0
LVKV_ERR_INVALID = -1
LVKV_FLAG_MASK = 1
LVKV_FLAG_ORDERED = 2
LVKV_FLAG_SYSTEM_ACQUIRE = 4
LVKV_FLAG_FINAL = 8
LVKV_FLAG_SMALL_BLOCKS = 16


class LvkvError(RuntimeError):
    """A C-ABI call returned a negative code (see lvkv_strerror)."""

    def __init__(self, fn: str, code: int):
        msg = _lib.lvkv_strerror(code).decode()
        if code in (-2, -3):
            msg += f" (hipError_t {_lib.lvkv_last_hip_error()})"
        super().__init__(f"{fn}: {msg} [{code}]")
        self.code = code


def _load() -> ctypes.CDLL:
    # One HIP runtime per process: torch bundles its own libamdhip64.so.7.
    # Loading torch FIRST makes this library's NEEDED libamdhip64.so.7 bind to
    # that same (already loaded) runtime, so device pointers and streams are
    # shared. Loading this library first would map /opt/rocm's runtime and
    # torch would then map a second one (device enumeration then fails).
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    if not LIB_PATH.exists():
        raise ImportError(
            f"{LIB_PATH} is not built; run `python -c 'import __graft_entry__ as g; g.build()'` "
            "(the GPU path has no fallback)")
    L = ctypes.CDLL(str(LIB_PATH))
    u32, u64, sz, vp, i32 = (ctypes.c_uint32, ctypes.c_uint64, ctypes.c_size_t,
                             ctypes.c_void_p, ctypes.c_int)
    L.lvkv_crc32c_extend.argtypes = [u32, ctypes.c_char_p, sz]
    L.lvkv_crc32c_extend.restype = u32
    L.lvkv_crc32c_value.argtypes = [ctypes.c_char_p, sz]
    L.lvkv_crc32c_value.restype = u32
    L.lvkv_crc32c_mask.argtypes = [u32]
    L.lvkv_crc32c_mask.restype = u32
    L.lvkv_crc32c_unmask.argtypes = [u32]
    L.lvkv_crc32c_unmask.restype = u32
    L.lvkv_crc32c_batch_device.argtypes = [vp, vp, vp, vp, u32, vp, sz, u32, vp]
    L.lvkv_crc32c_batch_device.restype = i32
    L.lvkv_crc32c_uniform_device.argtypes = [vp, u64, u32, u32, vp, sz, u32, vp]
    L.lvkv_crc32c_uniform_device.restype = i32
    L.lvkv_sst_verify_device.argtypes = [vp, vp, vp, vp, vp, sz, vp]
    L.lvkv_sst_verify_device.restype = i32
    L.lvkv_sst_verify_table_device.argtypes = [vp, u64, vp, vp, vp, vp, sz, ctypes.c_char_p,
                                               vp, vp]
    L.lvkv_sst_verify_table_device.restype = i32
    L.lvkv_sst_verify_tables_device.argtypes = [vp, vp, vp, sz, vp, vp, vp, vp, sz,
                                                ctypes.c_char_p, vp, vp]
    L.lvkv_sst_verify_tables_device.restype = i32
    L.lvkv_sst_fill_trailers_device.argtypes = [vp, vp, vp, vp, sz, vp]
    L.lvkv_sst_fill_trailers_device.restype = i32
    L.lvkv_log_fill_headers_device.argtypes = [vp, vp, vp, sz, vp]
    L.lvkv_log_fill_headers_device.restype = i32
    L.lvkv_log_verify_blocks_device.argtypes = [vp, u64, vp, vp, vp, sz, vp, vp, vp, vp]
    L.lvkv_log_verify_blocks_device.restype = i32
    L.lvkv_log_read_device.argtypes = [vp, u64, vp, vp, vp, sz, vp, vp, vp, vp, sz, vp, sz, u64,
                                       vp, vp]
    L.lvkv_log_read_device.restype = i32
    L.lvkv_log_gather_device.argtypes = [vp, vp, sz, vp, vp, sz, vp, vp, u64, vp, vp]
    L.lvkv_log_gather_device.restype = i32
    L.lvkv_debug_set_sst_form.argtypes = [i32]
    L.lvkv_debug_set_sst_form.restype = i32
    L.lvkv_log_verify_device.argtypes = [vp, vp, vp, vp, sz, vp]
    L.lvkv_log_verify_device.restype = i32
    L.lvkv_crc32c_batch_host.argtypes = [vp, vp, vp, vp, u32, vp, sz, u32]
    L.lvkv_crc32c_batch_host.restype = i32
    L.lvkv_engine_create.argtypes = [i32, ctypes.POINTER(vp)]
    L.lvkv_engine_create.restype = i32
    L.lvkv_engine_destroy.argtypes = [vp]
    L.lvkv_engine_destroy.restype = None
    L.lvkv_engine_crc32c_uniform.argtypes = [vp, vp, u64, u32, u32, vp, sz, u32]
    L.lvkv_engine_crc32c_uniform.restype = i32
    L.lvkv_engine_crc32c_batch.argtypes = [vp, vp, vp, vp, vp, u32, vp, sz, u32]
    L.lvkv_engine_crc32c_batch.restype = i32
    L.lvkv_engine_sst_verify.argtypes = [vp, vp, vp, vp, vp, vp, sz, u32]
    L.lvkv_engine_sst_verify.restype = i32
    L.lvkv_engine_log_verify.argtypes = [vp, vp, vp, vp, vp, sz, u32]
    L.lvkv_engine_log_verify.restype = i32
    L.lvkv_engine_sst_fill_trailers.argtypes = [vp, vp, vp, vp, vp, sz, u32]
    L.lvkv_engine_sst_fill_trailers.restype = i32
    L.lvkv_engine_log_fill_headers.argtypes = [vp, vp, vp, vp, sz, u32]
    L.lvkv_engine_log_fill_headers.restype = i32
    L.lvkv_engine_wait.argtypes = [vp]
    L.lvkv_engine_wait.restype = i32
    L.lvkv_engine_queues.argtypes = [vp, i32]
    L.lvkv_engine_queues.restype = i32
    L.lvkv_engine_shape.argtypes = [vp, ctypes.POINTER(u32), ctypes.POINTER(u32),
                                    ctypes.POINTER(u32)]
    L.lvkv_engine_shape.restype = i32
    L.lvkv_debug_engine_kernarg_cache.argtypes = [vp, ctypes.POINTER(u64), ctypes.POINTER(u64)]
    L.lvkv_debug_engine_kernarg_cache.restype = i32
    L.lvkv_engine_profile.argtypes = [vp, i32]
    L.lvkv_engine_profile.restype = i32
    L.lvkv_engine_profile_read.argtypes = [vp, ctypes.POINTER(ctypes.c_double),
                                           ctypes.POINTER(ctypes.c_double), sz]
    L.lvkv_engine_profile_read.restype = ctypes.c_long
    L.lvkv_engine_load_probe.argtypes = [vp, ctypes.c_char_p, sz, ctypes.c_char_p, u32, u32,
                                         u32, i32]
    L.lvkv_engine_load_probe.restype = i32
    L.lvkv_debug_engine_stall.argtypes = [vp, i32, ctypes.c_double]
    L.lvkv_debug_engine_stall.restype = i32
    L.lvkv_snappy_max_compressed_length.argtypes = [sz]
    L.lvkv_snappy_max_compressed_length.restype = sz
    L.lvkv_snappy_compress_device.argtypes = [vp, vp, vp, vp, vp, vp, vp, sz, u32, vp]
    L.lvkv_snappy_compress_device.restype = i32
    L.lvkv_snappy_uncompressed_length_device.argtypes = [vp, vp, vp, vp, vp, sz, vp]
    L.lvkv_snappy_uncompressed_length_device.restype = i32
    L.lvkv_snappy_uncompress_device.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, sz, u32, vp]
    L.lvkv_snappy_uncompress_device.restype = i32
    L.lvkv_zstd_uncompressed_length_device.argtypes = [vp, vp, vp, vp, vp, sz, vp]
    L.lvkv_zstd_uncompressed_length_device.restype = i32
    L.lvkv_zstd_uncompress_device.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, sz, u32, vp]
    L.lvkv_zstd_uncompress_device.restype = i32
    L.lvkv_debug_zstd_uncompress_device.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, vp, sz, u32,
                                                    vp]
    L.lvkv_debug_zstd_uncompress_device.restype = i32
    L.lvkv_sst_write_scratch_bytes.argtypes = [sz, u32]
    L.lvkv_sst_write_scratch_bytes.restype = sz
    L.lvkv_sst_write_blocks_device.argtypes = [vp, vp, vp, sz, i32, u32, vp, vp, u64, vp, vp, vp,
                                               vp, vp]
    L.lvkv_sst_write_blocks_device.restype = i32
    L.lvkv_sst_write_blocks_level_device.argtypes = [vp, vp, vp, sz, i32, i32, u32, vp, vp, u64,
                                                     vp, vp, vp, vp, vp]
    L.lvkv_sst_write_blocks_level_device.restype = i32
    L.lvkv_zstd_compress_bound.argtypes = [sz]
    L.lvkv_zstd_compress_bound.restype = sz
    L.lvkv_zstd_compress_device.argtypes = [vp, vp, vp, vp, vp, vp, vp, sz, u32, i32, vp]
    L.lvkv_zstd_compress_device.restype = i32
    L.lvkv_zstd_compress_big_scratch_bytes.argtypes = [u32]
    L.lvkv_zstd_compress_big_scratch_bytes.restype = sz
    L.lvkv_zstd_compress_big_device.argtypes = [vp, vp, vp, vp, vp, vp, vp, sz, u32, i32, vp, sz,
                                                vp]
    L.lvkv_zstd_compress_big_device.restype = i32
    L.lvkv_sst_write_scratch_bytes_v2.argtypes = [sz, u64, u32]
    L.lvkv_sst_write_scratch_bytes_v2.restype = sz
    L.lvkv_sst_write_blocks_status_device.argtypes = [vp, vp, vp, sz, i32, i32, u32, vp, vp, u64,
                                                      vp, vp, vp, vp, sz, vp, vp]
    L.lvkv_sst_write_blocks_status_device.restype = i32
    L.lvkv_sst_write_table_scratch_bytes.argtypes = [sz, u64, u32, u32, i32]
    L.lvkv_sst_write_table_scratch_bytes.restype = sz
    L.lvkv_sst_table_file_bound.argtypes = [sz, u64, u32, i32]
    L.lvkv_sst_table_file_bound.restype = u64
    L.lvkv_sst_write_table_device.argtypes = [vp, vp, vp, sz, i32, i32, u32, i32, i32, u32, vp, sz,
                                              vp, u64, vp, vp, vp, vp, vp, vp]
    L.lvkv_sst_write_table_device.restype = i32
    L.lvkv_sst_build_blocks_scratch_bytes.argtypes = [sz, u32]
    L.lvkv_sst_build_blocks_scratch_bytes.restype = sz
    L.lvkv_sst_build_blocks_raw_bound.argtypes = [sz, u64, u64, u32]
    L.lvkv_sst_build_blocks_raw_bound.restype = u64
    L.lvkv_sst_build_blocks_device.argtypes = [vp, vp, vp, vp, vp, vp, sz, u32, u32, i32, vp, sz,
                                               vp, u64, vp, vp, sz, vp, vp]
    L.lvkv_sst_build_blocks_device.restype = i32
    L.lvkv_sst_read_blocks_device.argtypes = [vp, vp, vp, sz, i32, vp, vp, vp, vp, vp, u32, vp]
    L.lvkv_sst_read_blocks_device.restype = i32
    L.lvkv_sst_read_entries_scratch_bytes.argtypes = [sz, u64]
    L.lvkv_sst_read_entries_scratch_bytes.restype = sz
    L.lvkv_sst_read_entries_device.argtypes = [vp, vp, vp, vp, sz, vp, sz, vp, u64, vp, vp, vp, vp,
                                               sz, vp, vp, vp, vp]
    L.lvkv_sst_read_entries_device.restype = i32
    L.lvkv_sst_merge_entries_scratch_bytes.argtypes = [sz, u32]
    L.lvkv_sst_merge_entries_scratch_bytes.restype = sz
    L.lvkv_sst_merge_entries_device.argtypes = [vp, vp, vp, vp, vp, vp, sz, vp, u32, i32, u32, u64,
                                                vp, vp, vp, sz, vp, sz, vp, vp, vp, vp, vp, sz,
                                                vp, vp, vp]
    L.lvkv_sst_merge_entries_device.restype = i32
    L.lvkv_sst_get_locate_scratch_bytes.argtypes = [u32, sz]
    L.lvkv_sst_get_locate_scratch_bytes.restype = sz
    L.lvkv_sst_get_seek_scratch_bytes.argtypes = [sz]
    L.lvkv_sst_get_seek_scratch_bytes.restype = sz
    L.lvkv_sst_get_locate_device.argtypes = [vp, u32, vp, u32, vp, vp, vp, sz, i32, vp, sz, vp, vp,
                                             vp, vp, vp, vp]
    L.lvkv_sst_get_locate_device.restype = i32
    L.lvkv_sst_get_seek_device.argtypes = [vp, vp, vp, vp, sz, vp, vp, vp, vp, sz, i32, vp, sz, vp,
                                           vp, vp, vp, vp, vp, vp]
    L.lvkv_sst_get_seek_device.restype = i32
    L.lvkv_debug_set_vtable_copy_rows.argtypes = [i32]
    L.lvkv_debug_set_vtable_copy_rows.restype = i32
    L.lvkv_vtable_separate_scratch_bytes.argtypes = [sz]
    L.lvkv_vtable_separate_scratch_bytes.restype = sz
    L.lvkv_vtable_separate_vtb_bound.argtypes = [sz, u64, u64]
    L.lvkv_vtable_separate_vtb_bound.restype = u64
    L.lvkv_vtable_separate_vals_bound.argtypes = [sz, u64]
    L.lvkv_vtable_separate_vals_bound.restype = u64
    L.lvkv_vtable_separate_device.argtypes = [vp, vp, vp, vp, vp, vp, sz, u64, u64, vp, sz, vp, u64,
                                              vp, u64, vp, vp, vp, vp, vp, vp]
    L.lvkv_vtable_separate_device.restype = i32
    L.lvkv_vtable_resolve_scratch_bytes.argtypes = [sz]
    L.lvkv_vtable_resolve_scratch_bytes.restype = sz
    L.lvkv_vtable_resolve_device.argtypes = [vp, vp, vp, vp, sz, vp, vp, vp, vp, sz, vp, sz, vp, vp,
                                             vp, vp, vp, vp]
    L.lvkv_vtable_resolve_device.restype = i32
    L.lvkv_vtable_gather_scratch_bytes.argtypes = [sz]
    L.lvkv_vtable_gather_scratch_bytes.restype = sz
    L.lvkv_vtable_gather_device.argtypes = [vp, vp, vp, vp, vp, vp, sz, vp, sz, vp, u64, vp, vp, vp]
    L.lvkv_vtable_gather_device.restype = i32
    L.lvkv_memtable_scratch_bytes.argtypes = [sz, sz]
    L.lvkv_memtable_scratch_bytes.restype = sz
    L.lvkv_memtable_from_batches_device.argtypes = [vp, vp, vp, sz, u64, u32, vp, sz, vp, u64, vp,
                                                    vp, vp, vp, vp, sz, vp, vp, vp, vp]
    L.lvkv_memtable_from_batches_device.restype = i32
    L.lvkv_debug_set_memtable_tile.argtypes = [i32]
    L.lvkv_debug_set_memtable_tile.restype = i32
    L.lvkv_sst_scan_entries_scratch_bytes.argtypes = [sz, sz]
    L.lvkv_sst_scan_entries_scratch_bytes.restype = sz
    L.lvkv_sst_scan_entries_device.argtypes = [vp, vp, vp, vp, vp, sz, u64, vp, vp, vp, vp, vp, vp,
                                               sz, vp, sz, vp, vp, vp, vp, vp, sz, vp, vp, vp, vp,
                                               vp]
    L.lvkv_sst_scan_entries_device.restype = i32
    L.lvkv_strerror.argtypes = [i32]
    L.lvkv_strerror.restype = ctypes.c_char_p
    L.lvkv_last_hip_error.argtypes = []
    L.lvkv_last_hip_error.restype = i32
    L.lvkv_cpu_impl.argtypes = []
    L.lvkv_cpu_impl.restype = ctypes.c_char_p
    L.lvkv_device_groups.argtypes = []
    L.lvkv_device_groups.restype = i32
    # Link-level drop-ins (C++ / Google ABI) — resolved to check they exist.
    L.crc32c_extend.argtypes = [u32, ctypes.c_char_p, sz]
    L.crc32c_extend.restype = u32
    L.crc32c_value.argtypes = [ctypes.c_char_p, sz]
    L.crc32c_value.restype = u32
    return L


_lib = _load()
lib = _lib


def _check(fn: str, rc: int) -> None:
    if rc != LVKV_OK:
        raise LvkvError(fn, rc)


# --------------------------------------------------------------------------
# util/crc32c.h mirror (per call, host)


def _as_bytes(data) -> bytes:
    if isinstance(data, (bytes, bytearray)):
        return bytes(data)
    if isinstance(data, str):
        return data.encode()
    return memoryview(data).tobytes()


def Extend(init_crc: int, data, n: Optional[int] = None) -> int:
    """leveldb::crc32c::Extend (util/crc32c.h:17): crc32c of A||data given
    init_crc = crc32c(A)."""
    b = _as_bytes(data)
    if n is None:
        n = len(b)
    if n > len(b):
        raise ValueError("n exceeds data length")
    return int(_lib.lvkv_crc32c_extend(init_crc & 0xFFFFFFFF, b, n))


def Value(data, n: Optional[int] = None) -> int:
    """leveldb::crc32c::Value (util/crc32c.h:20)."""
    return Extend(0, data, n)


def Mask(crc: int) -> int:
    """leveldb::crc32c::Mask (util/crc32c.h:29-32)."""
    return int(_lib.lvkv_crc32c_mask(crc & 0xFFFFFFFF))


def Unmask(masked_crc: int) -> int:
    """leveldb::crc32c::Unmask (util/crc32c.h:35-38)."""
    return int(_lib.lvkv_crc32c_unmask(masked_crc & 0xFFFFFFFF))


def cpu_impl() -> str:
    return _lib.lvkv_cpu_impl().decode()


def device_groups() -> int:
    g = int(_lib.lvkv_device_groups())
    _check("lvkv_device_groups", g if g < 0 else 0)
    return g


# --------------------------------------------------------------------------
# batched device API (torch tensors are only device-memory plumbing)


def _torch():
    import torch
    return torch


def _dev_ptr(t, name: str, dtype=None, numel: Optional[int] = None):
    torch = _torch()
    if not isinstance(t, torch.Tensor) or t.device.type != "cuda":
        raise TypeError(f"{name} must be a CUDA (HIP) tensor")
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous")
    if dtype is not None and t.dtype not in dtype:
        raise TypeError(f"{name} must have dtype in {dtype}, got {t.dtype}")
    if numel is not None and t.numel() < numel:
        raise ValueError(f"{name} has {t.numel()} elements, need {numel}")
    return ctypes.c_void_p(t.data_ptr())


def _stream_handle(stream, device):
    torch = _torch()
    s = stream if stream is not None else torch.cuda.current_stream(device)
    return ctypes.c_void_p(s.cuda_stream)


def _u32_out(torch, n, device, out):
    if out is None:
        return torch.empty(n, dtype=torch.int32, device=device)
    return out


def crc32c_batch(buf, offsets, lengths, *, init: int = 0, inits=None,
                 mask: bool = False, out=None, stream=None):
    """Batched Extend over block i = buf[offsets[i] : offsets[i]+lengths[i]].

    buf: uint8/int8 CUDA tensor; offsets: int64 CUDA tensor; lengths, inits:
    int32 CUDA tensors (bit patterns of u32). Returns an int32 tensor of CRC
    bit patterns (Mask()ed if mask=True)."""
    torch = _torch()
    n = offsets.numel()
    if lengths.numel() != n:
        raise ValueError("offsets and lengths differ in length")
    out = _u32_out(torch, n, buf.device, out)
    with torch.cuda.device(buf.device):
        rc = _lib.lvkv_crc32c_batch_device(
            _dev_ptr(buf, "buf", (torch.uint8, torch.int8)),
            _dev_ptr(offsets, "offsets", (torch.int64,)),
            _dev_ptr(lengths, "lengths", (torch.int32,)),
            _dev_ptr(inits, "inits", (torch.int32,), n) if inits is not None else None,
            init & 0xFFFFFFFF,
            _dev_ptr(out, "out", (torch.int32,), n), n,
            LVKV_FLAG_MASK if mask else 0, _stream_handle(stream, buf.device))
    _check("lvkv_crc32c_batch_device", rc)
    return out


def crc32c_uniform(buf, nblocks: int, length: int, stride: Optional[int] = None, *,
                   init: int = 0, mask: bool = False, out=None, stream=None):
    """Batched Extend over nblocks blocks of `length` bytes at buf + i*stride."""
    torch = _torch()
    stride = length if stride is None else stride
    if nblocks and (nblocks - 1) * stride + length > buf.numel():
        raise ValueError("blocks exceed the buffer")
    out = _u32_out(torch, nblocks, buf.device, out)
    with torch.cuda.device(buf.device):
        rc = _lib.lvkv_crc32c_uniform_device(
            _dev_ptr(buf, "buf", (torch.uint8, torch.int8)), stride, length,
            init & 0xFFFFFFFF, _dev_ptr(out, "out", (torch.int32,), nblocks),
            nblocks, LVKV_FLAG_MASK if mask else 0,
            _stream_handle(stream, buf.device))
    _check("lvkv_crc32c_uniform_device", rc)
    return out


def sst_verify(file_buf, offsets, sizes, *, stream=None) -> Tuple["object", "object"]:
    """Batched ReadBlock checksum test (table/format.cc:92-99) over the
    BlockHandles {offsets[i], sizes[i]} of an SST image. Returns (actual crc
    int32 tensor, status uint8 tensor: 0 ok / 1 'block checksum mismatch')."""
    torch = _torch()
    n = offsets.numel()
    actual = torch.empty(n, dtype=torch.int32, device=file_buf.device)
    status = torch.empty(n, dtype=torch.uint8, device=file_buf.device)
    with torch.cuda.device(file_buf.device):
        rc = _lib.lvkv_sst_verify_device(
            _dev_ptr(file_buf, "file_buf", (torch.uint8, torch.int8)),
            _dev_ptr(offsets, "offsets", (torch.int64,)),
            _dev_ptr(sizes, "sizes", (torch.int32,), n),
            _dev_ptr(actual, "actual"), _dev_ptr(status, "status"), n,
            _stream_handle(stream, file_buf.device))
    _check("lvkv_sst_verify_device", rc)
    return actual, status


class SstReport(ctypes.Structure):
    """lvkv_sst_report (include/lvkv_crc32c.h)."""
    _fields_ = [("status", ctypes.c_int32), ("nblocks", ctypes.c_uint32),
                ("ndata", ctypes.c_uint32), ("has_filter", ctypes.c_uint32),
                ("nbad", ctypes.c_uint32), ("first_bad", ctypes.c_uint32),
                ("index_crc", ctypes.c_uint32), ("meta_crc", ctypes.c_uint32),
                ("index_status", ctypes.c_uint8), ("meta_status", ctypes.c_uint8),
                ("reserved0_", ctypes.c_uint8 * 2), ("first", ctypes.c_uint32),
                ("index_offset", ctypes.c_uint64), ("index_size", ctypes.c_uint64),
                ("meta_offset", ctypes.c_uint64), ("meta_size", ctypes.c_uint64),
                ("link_", ctypes.c_uint64), ("total_", ctypes.c_uint32),
                ("done_", ctypes.c_uint32)]

    def as_dict(self) -> dict:
        return {k: getattr(self, k) for k, _ in self._fields_
                if not k.endswith("_")}


SST_STATUS = {0: "OK", 1: "file is too short to be an sstable",
              2: "not an sstable (bad magic number)", 3: "bad block handle",
              4: "truncated block read (index)", 5: "block checksum mismatch (index)",
              6: "index block type not readable here", 7: "bad index block contents",
              8: "capacity too small"}
BLOCK_STATUS = {0: "OK", 1: "block checksum mismatch", 2: "truncated block read",
                3: "bad block type", 4: "bad block handle", 5: "bad entry in block",
                6: "compressed block (no codec as built)", 7: "not read"}
# FilterPolicy::Name() of leveldb::NewBloomFilterPolicy (util/bloom.cc)
BLOOM_POLICY = "leveldb.BuiltinBloomFilter2"


def _policy(filter_policy):
    return None if filter_policy is None else filter_policy.encode()


def sst_verify_table(file_buf, *, capacity: Optional[int] = None,
                     filter_policy: Optional[str] = BLOOM_POLICY, stream=None):
    """Whole-SSTable verify on the device (lvkv_sst_verify_table_device):
    footer, index, metaindex, filter and every data block of the SST image
    in `file_buf` (uint8 CUDA tensor). filter_policy: the reader's
    FilterPolicy::Name() (None: no policy, no filter block). Returns (report
    dict, offsets int64, sizes int32, actual int32, status uint8) — the
    per-block tensors cut to report['nblocks'] entries (data blocks in index
    order, then the filter). With capacity=None a first guess is retried once
    at the index's size."""
    torch = _torch()
    dev = file_buf.device
    size = file_buf.numel()
    cap = capacity if capacity is not None else max(64, size // 2048 + 2)
    for attempt in range(2):
        off = torch.empty(cap, dtype=torch.int64, device=dev)
        sizes = torch.empty(cap, dtype=torch.int32, device=dev)
        actual = torch.empty(cap, dtype=torch.int32, device=dev)
        status = torch.empty(cap, dtype=torch.uint8, device=dev)
        rep = torch.zeros(ctypes.sizeof(SstReport), dtype=torch.uint8, device=dev)
        with torch.cuda.device(dev):
            rc = _lib.lvkv_sst_verify_table_device(
                _dev_ptr(file_buf, "file_buf", (torch.uint8, torch.int8)), size,
                _dev_ptr(off, "offsets"), _dev_ptr(sizes, "sizes"), _dev_ptr(actual, "actual"),
                _dev_ptr(status, "status"), cap, _policy(filter_policy), _dev_ptr(rep, "report"),
                _stream_handle(stream, dev))
        _check("lvkv_sst_verify_table_device", rc)
        r = SstReport.from_buffer_copy(bytes(rep.cpu().numpy()))
        if r.status == 8 and capacity is None and attempt == 0:
            cap = r.ndata + 1
            continue
        break
    n = r.nblocks
    return r.as_dict(), off[:n], sizes[:n], actual[:n], status[:n]


def sst_verify_tables(file_buf, table_offsets, table_sizes, *, capacity=None,
                      filter_policy: Optional[str] = BLOOM_POLICY, stream=None):
    """Many SST images in one device buffer (lvkv_sst_verify_tables_device):
    two launches for all of them. Returns one (report dict, offsets, sizes,
    actual, status) per table as sst_verify_table would for that image alone,
    except that offsets are into file_buf. capacity (shared by all tables)
    defaults to file_buf.numel() // 2048 + 64 per table; a table that does
    not fit reports LVKV_SST_CAPACITY (8)."""
    torch = _torch()
    dev = file_buf.device
    T = len(table_offsets)
    toff = torch.tensor([int(x) for x in table_offsets], dtype=torch.int64, device=dev)
    tsz = torch.tensor([int(x) for x in table_sizes], dtype=torch.int64, device=dev)
    cap = capacity if capacity is not None else file_buf.numel() // 2048 + 64 * T
    o = torch.empty(cap, dtype=torch.int64, device=dev)
    sz = torch.empty(cap, dtype=torch.int32, device=dev)
    act = torch.empty(cap, dtype=torch.int32, device=dev)
    st = torch.empty(cap, dtype=torch.uint8, device=dev)
    rsz = ctypes.sizeof(SstReport)
    reps = torch.zeros(T * rsz, dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        rc = _lib.lvkv_sst_verify_tables_device(
            _dev_ptr(file_buf, "file_buf", (torch.uint8, torch.int8)), _dev_ptr(toff, "toff"),
            _dev_ptr(tsz, "tsize"), T, _dev_ptr(o, "offsets"), _dev_ptr(sz, "sizes"),
            _dev_ptr(act, "actual"), _dev_ptr(st, "status"), cap, _policy(filter_policy),
            _dev_ptr(reps, "reports"), _stream_handle(stream, dev))
    _check("lvkv_sst_verify_tables_device", rc)
    host = bytes(reps.cpu().numpy())
    out = []
    for t in range(T):
        r = SstReport.from_buffer_copy(host[t * rsz:(t + 1) * rsz])
        f, n = r.first, r.nblocks
        out.append((r.as_dict(), o[f:f + n], sz[f:f + n], act[f:f + n], st[f:f + n]))
    return out


def log_verify(file_buf, hdr_offsets, *, stream=None):
    """Batched ReadPhysicalRecord checksum test (db/log_reader.cc:243-257)
    over physical records whose 7-byte headers start at hdr_offsets[i]."""
    torch = _torch()
    n = hdr_offsets.numel()
    actual = torch.empty(n, dtype=torch.int32, device=file_buf.device)
    status = torch.empty(n, dtype=torch.uint8, device=file_buf.device)
    with torch.cuda.device(file_buf.device):
        rc = _lib.lvkv_log_verify_device(
            _dev_ptr(file_buf, "file_buf", (torch.uint8, torch.int8)),
            _dev_ptr(hdr_offsets, "hdr_offsets", (torch.int64,)),
            _dev_ptr(actual, "actual"), _dev_ptr(status, "status"), n,
            _stream_handle(stream, file_buf.device))
    _check("lvkv_log_verify_device", rc)
    return actual, status


def sst_fill_trailers(file_buf, offsets, sizes, *, stream=None):
    """Batched TableBuilder::WriteRawBlock checksum (table_builder.cc:192-209):
    for each block handle (offsets int64, sizes int32 CUDA tensors) whose type
    byte is already in file_buf, writes Mask(CRC32C(contents + type)) into
    the trailer in place. Returns the unmasked CRCs (int32 tensor)."""
    torch = _torch()
    n = offsets.numel()
    crc = torch.empty(n, dtype=torch.int32, device=file_buf.device)
    with torch.cuda.device(file_buf.device):
        rc = _lib.lvkv_sst_fill_trailers_device(
            _dev_ptr(file_buf, "file_buf", (torch.uint8, torch.int8)),
            _dev_ptr(offsets, "offsets", (torch.int64,)),
            _dev_ptr(sizes, "sizes", (torch.int32,), n), _dev_ptr(crc, "crc"), n,
            _stream_handle(stream, file_buf.device))
    _check("lvkv_sst_fill_trailers_device", rc)
    return crc


def log_fill_headers(file_buf, hdr_offsets, *, stream=None):
    """Batched log::Writer::EmitPhysicalRecord checksum (log_writer.cc:82-108):
    fills header bytes 0..3 of every record in place. Returns the unmasked
    CRCs (int32 tensor)."""
    torch = _torch()
    n = hdr_offsets.numel()
    crc = torch.empty(n, dtype=torch.int32, device=file_buf.device)
    with torch.cuda.device(file_buf.device):
        rc = _lib.lvkv_log_fill_headers_device(
            _dev_ptr(file_buf, "file_buf", (torch.uint8, torch.int8)),
            _dev_ptr(hdr_offsets, "hdr_offsets", (torch.int64,)), _dev_ptr(crc, "crc"), n,
            _stream_handle(stream, file_buf.device))
    _check("lvkv_log_fill_headers_device", rc)
    return crc


# --------------------------------------------------------------------------
# Snappy block codec (include/lvkv_snappy.h; port/port_stdcxx.h:90-133)

SNAPPY_OK, SNAPPY_BAD_LENGTH, SNAPPY_BAD_CONTENTS, SNAPPY_CAPACITY, SNAPPY_TOO_LARGE = range(5)
SNAPPY_MAX_BLOCK = 49152


def snappy_max_compressed_length(n: int) -> int:
    """snappy::MaxCompressedLength (32 + n + n/6)."""
    return int(_lib.lvkv_snappy_max_compressed_length(n))


def _packed_offsets(torch, sizes, device):
    """Exclusive prefix sum of sizes (int64, on device)."""
    off = torch.zeros(sizes.numel(), dtype=torch.int64, device=device)
    if sizes.numel() > 1:
        off[1:] = torch.cumsum(sizes[:-1].to(torch.int64), 0)
    return off


def _snappy_bound(lens):
    """snappy::MaxCompressedLength of each of an int64 tensor's lengths."""
    return 32 + lens + lens // 6


def _device_call(fn_name, dev, stream, *args, report: Optional[str] = None):
    """One C-ABI call on dev's stream (the call's last argument); a failure is
    raised under the name `report` (default: the function's own)."""
    with _torch().cuda.device(dev):
        rc = getattr(_lib, fn_name)(*args, _stream_handle(stream, dev))
    _check(report or fn_name, rc)


def _compress_outputs(src, offsets, lengths, max_len, dst, dst_offsets, bound, floor):
    """What the three compressors share before their call: the length check,
    the default max_len, a packed dst of bound(lengths) bytes a block (at
    least `floor` bytes in all) unless one is given, the outputs. Returns
    (max_len, (dst, dst_offsets, out_len, status), the call's first eight
    arguments -- None for an empty batch, which makes no call). Every tensor
    those point at is the caller's or among the outputs: it outlives the call."""
    torch = _torch()
    n = offsets.numel()
    dev = src.device
    if lengths.numel() != n:
        raise ValueError("offsets and lengths differ in length")
    if max_len is None:
        max_len = int(lengths.max().item()) if n else 0
    if dst is None:
        room = bound(lengths.to(torch.int64))
        dst_offsets = _packed_offsets(torch, room, dev)
        dst = torch.empty(max(floor, int(room.sum().item())) if n else floor, dtype=torch.uint8,
                          device=dev)
    elif dst_offsets is None:
        raise ValueError("dst needs dst_offsets")
    out_len = torch.empty(n, dtype=torch.int32, device=dev)
    status = torch.empty(n, dtype=torch.uint8, device=dev)
    args = None
    if n:
        args = [_dev_ptr(src, "src", (torch.uint8, torch.int8)),
                _dev_ptr(offsets, "offsets", (torch.int64,)),
                _dev_ptr(lengths, "lengths", (torch.int32,)),
                _dev_ptr(dst, "dst", (torch.uint8, torch.int8)),
                _dev_ptr(dst_offsets, "dst_offsets", (torch.int64,), n),
                _dev_ptr(out_len, "out_len"), _dev_ptr(status, "status"), n]
    return max_len, (dst, dst_offsets, out_len, status), args


def _ulen_call(fn_name, src, offsets, lengths, stream):
    """Both codecs' GetUncompressedLength: (lengths int32, status uint8)."""
    torch = _torch()
    n = offsets.numel()
    dev = src.device
    ulen = torch.zeros(n, dtype=torch.int32, device=dev)
    status = torch.empty(n, dtype=torch.uint8, device=dev)
    if n:
        _device_call(fn_name, dev, stream,
                     _dev_ptr(src, "src", (torch.uint8, torch.int8)),
                     _dev_ptr(offsets, "offsets", (torch.int64,)),
                     _dev_ptr(lengths, "lengths", (torch.int32,), n),
                     _dev_ptr(ulen, "ulen"), _dev_ptr(status, "status"), n)
    return ulen, status


def _uncompress_call(fn_name, src, offsets, lengths, max_ulen, dst, dst_offsets, dst_caps, stream,
                     *extra, report=None):
    """Both decoders: the bound on max_ulen, a dst of max_ulen bytes a stream
    unless one is given, the outputs, the call (`extra`: the debug entry's
    arguments between status and n; made here, while the default dst_caps is
    alive). Returns (dst, dst_offsets, out_len, status)."""
    torch = _torch()
    n = offsets.numel()
    dev = src.device
    if not 0 <= max_ulen <= SNAPPY_MAX_BLOCK:
        raise ValueError(f"max_ulen must be in [0, {SNAPPY_MAX_BLOCK}]")
    if dst is None:
        dst_caps = torch.full((n,), max_ulen, dtype=torch.int32, device=dev)
        dst_offsets = torch.arange(n, dtype=torch.int64, device=dev) * max_ulen
        dst = torch.empty(max(1, n * max_ulen), dtype=torch.uint8, device=dev)
    elif dst_offsets is None or dst_caps is None:
        raise ValueError("dst needs dst_offsets and dst_caps")
    out_len = torch.zeros(n, dtype=torch.int32, device=dev)
    status = torch.empty(n, dtype=torch.uint8, device=dev)
    if n:
        _device_call(fn_name, dev, stream,
                     _dev_ptr(src, "src", (torch.uint8, torch.int8)),
                     _dev_ptr(offsets, "offsets", (torch.int64,)),
                     _dev_ptr(lengths, "lengths", (torch.int32,), n),
                     _dev_ptr(dst, "dst", (torch.uint8, torch.int8)),
                     _dev_ptr(dst_offsets, "dst_offsets", (torch.int64,), n),
                     _dev_ptr(dst_caps, "dst_caps", (torch.int32,), n),
                     _dev_ptr(out_len, "out_len"), _dev_ptr(status, "status"), *extra, n, max_ulen,
                     report=report)
    return dst, dst_offsets, out_len, status


def snappy_compress(src, offsets, lengths, *, max_len: Optional[int] = None, dst=None,
                    dst_offsets=None, stream=None):
    """Batched port::Snappy_Compress (port/port_stdcxx.h:90-106) of block
    i = src[offsets[i] : offsets[i] + lengths[i]]: snappy 1.1.8's bytes.

    Without dst, every block gets MaxCompressedLength bytes, packed. Returns
    (dst uint8, dst_offsets int64, compressed lengths int32, status uint8:
    SNAPPY_OK or SNAPPY_TOO_LARGE for a block longer than max_len)."""
    max_len, outs, args = _compress_outputs(src, offsets, lengths, max_len, dst, dst_offsets,
                                            _snappy_bound, 0)
    if args:
        _device_call("lvkv_snappy_compress_device", src.device, stream, *args,
                     max(0, min(int(max_len), 0xFFFFFFFF)))
    return outs


def snappy_uncompressed_length(src, offsets, lengths, *, stream=None):
    """Batched port::Snappy_GetUncompressedLength (port/port_stdcxx.h:108-119).
    Returns (lengths int32 as u32 bit patterns, status uint8: SNAPPY_OK /
    SNAPPY_BAD_LENGTH)."""
    return _ulen_call("lvkv_snappy_uncompressed_length_device", src, offsets, lengths, stream)


def snappy_uncompress(src, offsets, lengths, *, max_ulen: int, dst=None, dst_offsets=None,
                      dst_caps=None, stream=None):
    """Batched port::Snappy_Uncompress (port/port_stdcxx.h:121-133) as
    ReadBlock runs it (table/format.cc:120-135). Without dst, every stream
    gets max_ulen bytes. max_ulen sizes the LDS staging; a longer stream is
    decoded from HBM by the call's second kernel. Returns (dst uint8,
    dst_offsets int64, uncompressed lengths int32, status uint8: SNAPPY_OK /
    BAD_LENGTH / BAD_CONTENTS / CAPACITY)."""
    return _uncompress_call("lvkv_snappy_uncompress_device", src, offsets, lengths, max_ulen, dst,
                            dst_offsets, dst_caps, stream)


ZSTD_OK, ZSTD_BAD_LENGTH, ZSTD_BAD_CONTENTS, ZSTD_CAPACITY, ZSTD_TOO_LARGE, \
    ZSTD_UNSUPPORTED = range(6)
ZSTD_MAX_BLOCK = 49152
ZSTD_COMPRESS_MAX_BLOCK = 20480


def zstd_compress_bound(n: int) -> int:
    """ZSTD_compressBound (libzstd 1.4.9)."""
    return int(_lib.lvkv_zstd_compress_bound(n))


def _zstd_bound(lens):
    """ZSTD_compressBound of each of an int64 tensor's lengths."""
    return lens + (lens >> 8) + _torch().clamp((131072 - lens) >> 11, min=0)


def zstd_compress(src, offsets, lengths, *, level: int = 1, max_len: Optional[int] = None,
                  dst=None, dst_offsets=None, stream=None):
    """Batched port::Zstd_Compress(level, block) (port/port_stdcxx.h:133-161) of
    block i = src[offsets[i] : offsets[i] + lengths[i]]: libzstd 1.4.9's frame
    as ZSTD_compress2 writes it after getCParams(level, max(n, 1)) +
    setCParams. Without dst, every block gets ZSTD_compressBound bytes,
    packed. Returns (dst uint8, dst_offsets int64, frame lengths int32,
    status uint8: ZSTD_OK / ZSTD_TOO_LARGE / ZSTD_UNSUPPORTED)."""
    # (max_len past ZSTD_COMPRESS_MAX_BLOCK: the C-ABI's LVKV_ERR_INVALID)
    max_len, outs, args = _compress_outputs(src, offsets, lengths, max_len, dst, dst_offsets,
                                            _zstd_bound, 1)
    if args:
        _device_call("lvkv_zstd_compress_device", src.device, stream, *args, int(max_len),
                     int(level))
    return outs


ZSTD_COMPRESS_BIG_MAX_BLOCK = 131072


def zstd_compress_big_scratch_bytes(max_len: int) -> int:
    """The scratch zstd_compress_big's second kernel works in: a fixed pool,
    the same for every batch (0 for max_len <= ZSTD_COMPRESS_MAX_BLOCK)."""
    return int(_lib.lvkv_zstd_compress_big_scratch_bytes(max(0, min(int(max_len), 0xFFFFFFFF))))


def zstd_compress_big(src, offsets, lengths, *, level: int = 1, max_len: Optional[int] = None,
                      dst=None, dst_offsets=None, scratch=None, stream=None):
    """zstd_compress for blocks of any length up to ZSTD_COMPRESS_BIG_MAX_BLOCK
    (one Zstd block a frame): identical to libzstd 1.4.9 driven as
    port::Zstd_Compress. Blocks up to ZSTD_COMPRESS_MAX_BLOCK take the kernel
    of zstd_compress (the same bytes); the longer ones a second kernel on the
    same stream. max_len may be anything: a block longer than min(max_len,
    ZSTD_COMPRESS_BIG_MAX_BLOCK) is ZSTD_TOO_LARGE (the host library's), a
    level that is not ZSTD_fast (0, >= 3) ZSTD_UNSUPPORTED. The scratch is
    allocated here unless given (zstd_compress_big_scratch_bytes(max_len)
    bytes; it belongs to the call until the stream has run it). Returns the
    same 4-tuple as zstd_compress."""
    torch = _torch()
    max_len, outs, args = _compress_outputs(src, offsets, lengths, max_len, dst, dst_offsets,
                                            _zstd_bound, 1)
    max_len = max(0, min(int(max_len), 0xFFFFFFFF))
    if args:
        dev = src.device
        need = zstd_compress_big_scratch_bytes(max_len)
        if scratch is None and need:
            scratch = torch.empty(need, dtype=torch.uint8, device=dev)
        _device_call("lvkv_zstd_compress_big_device", dev, stream, *args, max_len, int(level),
                     _dev_ptr(scratch, "scratch", (torch.uint8, torch.int8))
                     if scratch is not None else None,
                     scratch.numel() if scratch is not None else 0)
    return outs


READ_OK, READ_CHECKSUM, READ_BAD_TYPE, READ_SNAPPY_LENGTH, READ_SNAPPY_CONTENTS, \
    READ_ZSTD_LENGTH, READ_CAPACITY, READ_TOO_LARGE, READ_ZSTD_CONTENTS = range(9)


def zstd_uncompressed_length(src, offsets, lengths, *, stream=None):
    """Batched port::Zstd_GetUncompressedLength (port/port_stdcxx.h:163-177):
    (lengths int32 as u32, status uint8: SNAPPY_OK / SNAPPY_BAD_LENGTH (0) /
    SNAPPY_TOO_LARGE (unknown, malformed, > 32 bits))."""
    return _ulen_call("lvkv_zstd_uncompressed_length_device", src, offsets, lengths, stream)


def zstd_uncompress(src, offsets, lengths, *, max_ulen: int, dst=None, dst_offsets=None,
                    dst_caps=None, detail: bool = False, stream=None):
    """Batched port::Zstd_Uncompress (port/port_stdcxx.h:179-199) as ReadBlock
    runs it (table/format.cc:138-155). Statuses as snappy_uncompress. With
    detail=True also returns the failure site per stream (a debug hook)."""
    if not detail:
        return _uncompress_call("lvkv_zstd_uncompress_device", src, offsets, lengths, max_ulen, dst,
                                dst_offsets, dst_caps, stream)
    torch = _torch()
    why = torch.zeros(max(1, offsets.numel()), dtype=torch.int32, device=src.device)
    return _uncompress_call("lvkv_debug_zstd_uncompress_device", src, offsets, lengths, max_ulen,
                            dst, dst_offsets, dst_caps, stream, _dev_ptr(why, "detail"),
                            report="lvkv_zstd_uncompress_device") + (why,)


def _sst_write(raw, offsets, lengths, compression, zstd_level, max_len, file, file_offset, stream,
               with_status):
    """Both writers: the outputs, the scratch by the public sizing function of
    the call (fixed stride, or ragged with a status), the call."""
    torch = _torch()
    n = offsets.numel()
    dev = raw.device
    total_raw = 0
    if n and (file is None or with_status):  # (sizes the file image and the ragged scratch)
        total_raw = int(lengths.to(torch.int64).sum().item())
    if max_len is None:
        max_len = int(lengths.max().item()) if n else 0
    if with_status:
        max_len = max(0, min(int(max_len), 0xFFFFFFFF))
    if file is None:
        file = torch.zeros(max(1, file_offset + total_raw + 5 * n), dtype=torch.uint8, device=dev)
    hoff = torch.empty(n, dtype=torch.int64, device=dev)
    hsize = torch.empty(n, dtype=torch.int32, device=dev)
    typ = torch.empty(n, dtype=torch.uint8, device=dev)
    end = torch.empty(1, dtype=torch.int64, device=dev)
    status = torch.empty(n, dtype=torch.uint8, device=dev) if with_status else None
    scratch = None
    if compression in (1, 2) and n:
        if with_status:  # (the zstd compressor's pool is part of it only for compression 2)
            need = _lib.lvkv_sst_write_scratch_bytes_v2(n, total_raw,
                                                        max_len if compression == 2 else 0)
        else:
            need = _lib.lvkv_sst_write_scratch_bytes(n, max_len)
        scratch = torch.empty(int(need), dtype=torch.uint8, device=dev)
    args = [_dev_ptr(raw, "raw", (torch.uint8, torch.int8)) if n else None,
            _dev_ptr(offsets, "offsets", (torch.int64,)) if n else None,
            _dev_ptr(lengths, "lengths", (torch.int32,), n) if n else None, n, compression,
            int(zstd_level), max_len, _dev_ptr(scratch, "scratch") if scratch is not None else None,
            _dev_ptr(file, "file", (torch.uint8, torch.int8)), file_offset,
            _dev_ptr(hoff, "hoff") if n else None, _dev_ptr(hsize, "hsize") if n else None,
            _dev_ptr(typ, "type") if n else None, _dev_ptr(end, "end")]
    if with_status:
        name = "lvkv_sst_write_blocks_status_device"
        args += [scratch.numel() if scratch is not None else 0,
                 _dev_ptr(status, "status") if n else None]
    else:
        name = "lvkv_sst_write_blocks_level_device"
    with torch.cuda.device(dev):
        rc = getattr(_lib, name)(*args, _stream_handle(stream, dev))
    _check(name, rc)
    return (file, hoff, hsize, typ, end) + ((status,) if with_status else ())


def sst_write_blocks(raw, offsets, lengths, *, compression: int = 1, max_len: Optional[int] = None,
                     file=None, file_offset: int = 0, zstd_level: int = 1, stream=None):
    """Batched TableBuilder::WriteBlock + WriteRawBlock (table/table_builder.cc:
    141-209): blocks raw[offsets[i] : offsets[i] + lengths[i]] written in order
    from file_offset of the file image `file` (allocated when None: file_offset
    + sum(lengths + 5) bytes). Returns (file, handle offsets int64, handle
    sizes int32, types uint8, end offset int64 tensor of one)."""
    return _sst_write(raw, offsets, lengths, compression, zstd_level, max_len, file, file_offset,
                      stream, False)


def sst_write_blocks_status(raw, offsets, lengths, *, compression: int = 1, zstd_level: int = 1,
                            max_len: Optional[int] = None, file=None, file_offset: int = 0,
                            stream=None):
    """sst_write_blocks for blocks of any size, with the codec's verdict per
    block: snappy compresses every block; zstd (levels <= 2 except 0) every
    block up to min(max_len, ZSTD_COMPRESS_BIG_MAX_BLOCK). status[i] is
    ZSTD_OK, or ZSTD_TOO_LARGE for a block the device left raw (type 0) that
    TableBuilder::WriteBlock would have compressed: a zstd block past that
    bound. A block the 12.5% rule kept raw has status OK. The scratch grows
    with the bytes written, not with the block count times max_len. Returns
    (file, handle offsets int64, handle sizes int32, types uint8, end offset
    int64 tensor of one, status uint8)."""
    return _sst_write(raw, offsets, lengths, compression, zstd_level, max_len, file, file_offset,
                      stream, True)


TABLE_OK, TABLE_BAD_BLOCK, TABLE_KEY_TOO_LONG, TABLE_CAPACITY = range(4)


class SstTableReport(ctypes.Structure):
    """lvkv_sst_table_report (include/lvkv_snappy.h)."""
    _fields_ = [("status", ctypes.c_int32), ("first_bad_block", ctypes.c_uint32),
                ("num_entries", ctypes.c_uint64), ("nfilters", ctypes.c_uint32),
                ("meta_type", ctypes.c_uint8), ("index_type", ctypes.c_uint8),
                ("meta_status", ctypes.c_uint8), ("index_status", ctypes.c_uint8),
                ("data_end", ctypes.c_uint64), ("filter_offset", ctypes.c_uint64),
                ("filter_size", ctypes.c_uint64), ("meta_offset", ctypes.c_uint64),
                ("meta_size", ctypes.c_uint64), ("index_offset", ctypes.c_uint64),
                ("index_size", ctypes.c_uint64), ("file_size", ctypes.c_uint64)]

    def as_dict(self) -> dict:
        return {k: getattr(self, k) for k, _ in self._fields_}


def sst_write_table(raw, offsets, lengths, *, compression: int = 1, zstd_level: int = 1,
                    max_len: Optional[int] = None, key_format: int = 1,
                    filter_bits_per_key: int = 10, max_key_len: int = 256, file=None,
                    file_capacity: Optional[int] = None, scratch=None, stream=None):
    """TableBuilder::Flush per block and TableBuilder::Finish (table/
    table_builder.cc) in one stream-ordered call (lvkv_sst_write_table_device):
    the finished data blocks raw[offsets[i] : offsets[i] + lengths[i]], in key
    order, become the whole table image -- data blocks as
    sst_write_blocks_status writes them, filter block (filter_bits_per_key > 0:
    the built-in Bloom policy; 0: none), metaindex block, index block, footer.
    key_format 1: internal keys (db/builder.cc's tables), 0: plain byte
    strings. `file` (allocated by lvkv_sst_table_file_bound when None) holds
    the image from offset 0; at most file_capacity (default: all) of its bytes
    are written. Returns (file, handle offsets int64, handle sizes int32,
    types uint8, status uint8, report dict); report['status'] is TABLE_*, and
    the image is file[:report['file_size']] when it is TABLE_OK. The report is
    the one thing read back."""
    torch = _torch()
    n = offsets.numel()
    dev = raw.device
    if lengths.numel() != n:
        raise ValueError("offsets and lengths differ in length")
    total_raw = int(lengths.to(torch.int64).sum().item()) if n else 0
    if max_len is None:
        max_len = int(lengths.max().item()) if n else 0
    max_len = max(0, min(int(max_len), 0xFFFFFFFF))
    if file is None:
        file = torch.zeros(int(_lib.lvkv_sst_table_file_bound(n, total_raw, max_key_len,
                                                              filter_bits_per_key)),
                           dtype=torch.uint8, device=dev)
    if file_capacity is None:
        file_capacity = file.numel()
    if file_capacity > file.numel():
        raise ValueError("file_capacity exceeds the file tensor")
    if scratch is None:
        scratch = torch.empty(int(_lib.lvkv_sst_write_table_scratch_bytes(
            n, total_raw, max_len, max_key_len, filter_bits_per_key)), dtype=torch.uint8,
            device=dev)
    hoff = torch.empty(n, dtype=torch.int64, device=dev)
    hsize = torch.empty(n, dtype=torch.int32, device=dev)
    typ = torch.empty(n, dtype=torch.uint8, device=dev)
    status = torch.empty(n, dtype=torch.uint8, device=dev)
    rep = torch.zeros(ctypes.sizeof(SstTableReport), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        rc = _lib.lvkv_sst_write_table_device(
            _dev_ptr(raw, "raw", (torch.uint8, torch.int8)) if n else None,
            _dev_ptr(offsets, "offsets", (torch.int64,)) if n else None,
            _dev_ptr(lengths, "lengths", (torch.int32,)) if n else None, n, int(compression),
            int(zstd_level), max_len, int(key_format), int(filter_bits_per_key), int(max_key_len),
            _dev_ptr(scratch, "scratch", (torch.uint8, torch.int8)), scratch.numel(),
            _dev_ptr(file, "file", (torch.uint8, torch.int8)), int(file_capacity),
            _dev_ptr(hoff, "hoff") if n else None, _dev_ptr(hsize, "hsize") if n else None,
            _dev_ptr(typ, "type") if n else None, _dev_ptr(status, "status") if n else None,
            _dev_ptr(rep, "report"), _stream_handle(stream, dev))
    _check("lvkv_sst_write_table_device", rc)
    if stream is not None:
        stream.synchronize()
    report = SstTableReport.from_buffer_copy(bytes(rep.cpu().numpy())).as_dict()
    return file, hoff, hsize, typ, status, report


BUILD_OK, BUILD_UNSORTED, BUILD_BAD_KEY, BUILD_CAPACITY, BUILD_TOO_LARGE = range(5)


class SstBuildReport(ctypes.Structure):
    """lvkv_sst_build_report (include/lvkv_snappy.h)."""
    _fields_ = [("status", ctypes.c_int32), ("first_bad_entry", ctypes.c_uint32),
                ("nblocks", ctypes.c_uint32), ("max_block_len", ctypes.c_uint32),
                ("max_key_len", ctypes.c_uint32), ("num_entries", ctypes.c_uint64),
                ("raw_bytes", ctypes.c_uint64)]

    def as_dict(self) -> dict:
        return {k: getattr(self, k) for k, _ in self._fields_}


def sst_build_blocks(keys, key_off, key_len, vals, val_off, val_len, *, block_size: int = 4096,
                     restart_interval: int = 16, key_format: int = 1, raw=None,
                     max_blocks: Optional[int] = None, scratch=None, stream=None):
    """TableBuilder::Add over sorted entries (lvkv_sst_build_blocks_device):
    entry i is keys[key_off[i] : key_off[i] + key_len[i]] -> vals[val_off[i] :
    val_off[i] + val_len[i]], in comparator order (key_format 1: internal
    keys, 0: plain byte strings). The data blocks BlockBuilder builds, cut as
    TableBuilder cuts them at block_size, land in `raw` (allocated by
    lvkv_sst_build_blocks_raw_bound when None; all of it may be written) at
    raw_off[b], raw_len[b] for b < report['nblocks'] (arrays of max_blocks,
    default: an entry a block). Returns (raw, raw_off int64, raw_len int32,
    report dict); report['status'] is BUILD_*, and nothing is written unless
    it is BUILD_OK. The report is the one thing read back."""
    torch = _torch()
    n = key_off.numel()
    dev = keys.device
    if not (key_len.numel() == val_off.numel() == val_len.numel() == n):
        raise ValueError("the entry arrays differ in length")
    if max_blocks is None:
        max_blocks = n
    if raw is None:
        kb = int(key_len.to(torch.int64).sum().item()) if n else 0
        vb = int(val_len.to(torch.int64).sum().item()) if n else 0
        raw = torch.empty(max(1, int(_lib.lvkv_sst_build_blocks_raw_bound(
            n, kb, vb, restart_interval))), dtype=torch.uint8, device=dev)
    if scratch is None:
        scratch = torch.empty(int(_lib.lvkv_sst_build_blocks_scratch_bytes(n, restart_interval)),
                              dtype=torch.uint8, device=dev)
    raw_off = torch.empty(max(1, max_blocks), dtype=torch.int64, device=dev)[:max_blocks]
    raw_len = torch.empty(max(1, max_blocks), dtype=torch.int32, device=dev)[:max_blocks]
    rep = torch.zeros(ctypes.sizeof(SstBuildReport), dtype=torch.uint8, device=dev)
    b8 = (torch.uint8, torch.int8)
    with torch.cuda.device(dev):
        rc = _lib.lvkv_sst_build_blocks_device(
            _dev_ptr(keys, "keys", b8) if n else None,
            _dev_ptr(key_off, "key_off", (torch.int64,)) if n else None,
            _dev_ptr(key_len, "key_len", (torch.int32,)) if n else None,
            _dev_ptr(vals, "vals", b8) if n else None,
            _dev_ptr(val_off, "val_off", (torch.int64,)) if n else None,
            _dev_ptr(val_len, "val_len", (torch.int32,)) if n else None,
            n, int(block_size), int(restart_interval), int(key_format),
            _dev_ptr(scratch, "scratch", b8), scratch.numel(), _dev_ptr(raw, "raw", b8),
            raw.numel(), _dev_ptr(raw_off, "raw_off", (torch.int64,)),
            _dev_ptr(raw_len, "raw_len", (torch.int32,)), int(max_blocks),
            _dev_ptr(rep, "report"), _stream_handle(stream, dev))
    _check("lvkv_sst_build_blocks_device", rc)
    if stream is not None:
        stream.synchronize()
    report = SstBuildReport.from_buffer_copy(bytes(rep.cpu().numpy())).as_dict()
    return raw, raw_off, raw_len, report


def sst_build_table(keys, key_off, key_len, vals, val_off, val_len, *, block_size: int = 4096,
                    restart_interval: int = 16, key_format: int = 1, compression: int = 1,
                    zstd_level: int = 1, filter_bits_per_key: int = 10, file=None,
                    file_capacity: Optional[int] = None, stream=None):
    """Sorted entries -> the whole table image: sst_build_blocks, then
    sst_write_table on the blocks it cut, with max_len and max_key_len from
    the build's report. Returns sst_write_table's tuple and the build report:
    (file, handle offsets, handle sizes, types, status, table report, build
    report). When the build's status is not BUILD_OK no table is written and
    the first six are None."""
    raw, raw_off, raw_len, build = sst_build_blocks(
        keys, key_off, key_len, vals, val_off, val_len, block_size=block_size,
        restart_interval=restart_interval, key_format=key_format, stream=stream)
    if build["status"] != BUILD_OK:
        return (None,) * 6 + (build,)
    nb = build["nblocks"]
    out = sst_write_table(raw, raw_off[:nb], raw_len[:nb], compression=compression,
                          zstd_level=zstd_level, max_len=build["max_block_len"],
                          key_format=key_format, filter_bits_per_key=filter_bits_per_key,
                          max_key_len=build["max_key_len"], file=file,
                          file_capacity=file_capacity, stream=stream)
    return out + (build,)


def sst_read_blocks(file, handle_off, handle_size, *, max_ulen: int, verify: bool = True,
                    out=None, out_offsets=None, out_caps=None, stream=None):
    """Batched ReadBlock (table/format.cc:69-162): checksum, then contents by
    type (raw copied, snappy decoded). Without out, each block gets max_ulen
    bytes. Returns (out uint8, out_offsets int64, lengths int32, status uint8
    READ_*)."""
    torch = _torch()
    n = handle_off.numel()
    dev = file.device
    if not 0 <= max_ulen <= SNAPPY_MAX_BLOCK:
        raise ValueError(f"max_ulen must be in [0, {SNAPPY_MAX_BLOCK}]")
    if out is None:
        out_caps = torch.full((n,), max_ulen, dtype=torch.int32, device=dev)
        out_offsets = torch.arange(n, dtype=torch.int64, device=dev) * max_ulen
        out = torch.empty(max(1, n * max_ulen), dtype=torch.uint8, device=dev)
    elif out_offsets is None or out_caps is None:
        raise ValueError("out needs out_offsets and out_caps")
    out_len = torch.zeros(n, dtype=torch.int32, device=dev)
    status = torch.empty(n, dtype=torch.uint8, device=dev)
    if n:
        with torch.cuda.device(dev):
            rc = _lib.lvkv_sst_read_blocks_device(
                _dev_ptr(file, "file", (torch.uint8, torch.int8)),
                _dev_ptr(handle_off, "handle_off", (torch.int64,)),
                _dev_ptr(handle_size, "handle_size", (torch.int32,), n), n, 1 if verify else 0,
                _dev_ptr(out, "out", (torch.uint8, torch.int8)),
                _dev_ptr(out_offsets, "out_offsets", (torch.int64,), n),
                _dev_ptr(out_caps, "out_caps", (torch.int32,), n),
                _dev_ptr(out_len, "out_len"), _dev_ptr(status, "status"), max_ulen,
                _stream_handle(stream, dev))
        _check("lvkv_sst_read_blocks_device", rc)
    return out, out_offsets, out_len, status


ENTRIES_OK, ENTRIES_BAD_BLOCK, ENTRIES_BAD_ENTRY, ENTRIES_SKIPPED = range(4)
ENTRIES_CAPACITY = 1


class SstEntriesReport(ctypes.Structure):
    """lvkv_sst_entries_report (include/lvkv_snappy.h)."""
    _fields_ = [("status", ctypes.c_int32), ("nbad", ctypes.c_uint32),
                ("first_bad_block", ctypes.c_uint32), ("max_key_len", ctypes.c_uint32),
                ("num_entries", ctypes.c_uint64), ("key_bytes", ctypes.c_uint64),
                ("value_bytes", ctypes.c_uint64)]

    def as_dict(self) -> dict:
        return {k: getattr(self, k) for k, _ in self._fields_}


def sst_read_entries(raw, raw_off, raw_len, *, skip=None, keys=None,
                     key_capacity: Optional[int] = None, max_entries: Optional[int] = None,
                     stream=None):
    """Block::Iter's forward walk over decoded data blocks
    (lvkv_sst_read_entries_device): blocks raw[raw_off[b] : raw_off[b] +
    raw_len[b]] -- sst_read_blocks' out, out_offsets and lengths; skip: its
    status, a block with a non-zero byte is not walked -- become their
    entries, in block order, laid out as sst_build_blocks takes them: the
    restored keys in `keys` 8 bytes apart, the values left in `raw`.
    max_entries defaults to the most the bytes can hold (an entry takes three).
    Without key_capacity the keys get a first guess of the blocks' bytes and
    the call is repeated once with what the report asks for. Returns (keys,
    key_off int64, key_len int32, raw, val_off int64, val_len int32 -- the
    build's inputs, cut to report['num_entries'] -- block_first int64 of
    nblocks + 1, block_status uint8 ENTRIES_*, report dict). report['status']
    is 0 or ENTRIES_CAPACITY, and nothing of the entries is written unless it
    is 0. The report is the one thing read back."""
    torch = _torch()
    n = raw_off.numel()
    dev = raw.device
    if raw_len.numel() != n or (skip is not None and skip.numel() != n):
        raise ValueError("the block arrays differ in length")
    total = int(raw_len.to(torch.int64).sum().item()) if n else 0
    if max_entries is None:
        max_entries = total // 3
    guess = key_capacity is None and keys is None
    if key_capacity is None:
        key_capacity = keys.numel() if keys is not None else 2 * total + 64
    scratch = torch.empty(int(_lib.lvkv_sst_read_entries_scratch_bytes(n, total)),
                          dtype=torch.uint8, device=dev)
    slots = max(1, max_entries)
    key_off = torch.empty(slots, dtype=torch.int64, device=dev)
    key_len = torch.empty(slots, dtype=torch.int32, device=dev)
    val_off = torch.empty(slots, dtype=torch.int64, device=dev)
    val_len = torch.empty(slots, dtype=torch.int32, device=dev)
    first = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    status = torch.empty(max(1, n), dtype=torch.uint8, device=dev)[:n]
    rep = torch.zeros(ctypes.sizeof(SstEntriesReport), dtype=torch.uint8, device=dev)
    b8 = (torch.uint8, torch.int8)
    for attempt in range(2):
        if keys is None or keys.numel() < key_capacity:
            keys = torch.empty(max(8, key_capacity), dtype=torch.uint8, device=dev)
        with torch.cuda.device(dev):
            rc = _lib.lvkv_sst_read_entries_device(
                _dev_ptr(raw, "raw", b8) if n else None,
                _dev_ptr(raw_off, "raw_off", (torch.int64,)) if n else None,
                _dev_ptr(raw_len, "raw_len", (torch.int32,)) if n else None,
                _dev_ptr(skip, "skip", (torch.uint8,)) if skip is not None and n else None, n,
                _dev_ptr(scratch, "scratch", b8), scratch.numel(), _dev_ptr(keys, "keys", b8),
                int(key_capacity), _dev_ptr(key_off, "key_off"), _dev_ptr(key_len, "key_len"),
                _dev_ptr(val_off, "val_off"), _dev_ptr(val_len, "val_len"), int(max_entries),
                _dev_ptr(first, "block_first"), _dev_ptr(status, "block_status") if n else None,
                _dev_ptr(rep, "report"), _stream_handle(stream, dev))
        _check("lvkv_sst_read_entries_device", rc)
        if stream is not None:
            stream.synchronize()
        report = SstEntriesReport.from_buffer_copy(bytes(rep.cpu().numpy())).as_dict()
        if not (guess and attempt == 0 and report["status"] == ENTRIES_CAPACITY and
                report["num_entries"] <= max_entries):
            break
        key_capacity, keys = report["key_bytes"], None
    ne = report["num_entries"] if report["status"] == 0 else 0
    return (keys, key_off[:ne], key_len[:ne], raw, val_off[:ne], val_len[:ne], first, status,
            report)


def sst_read_table(file, *, filter_policy: Optional[str] = None, max_ulen: int,
                   verify: bool = True, stream=None):
    """A table image -> its entries, ready for sst_build_table: sst_verify_table
    (footer, index: the data blocks' handles), sst_read_blocks over them
    (max_ulen: the longest decoded block), sst_read_entries over what that
    decoded. The reports are read on the host between the calls. Returns
    (keys, key_off, key_len, vals, val_off, val_len, table report, block
    status uint8 READ_*, entries report); the first six are None when the
    table's status is not 0 (nothing to list the blocks from). A block
    ReadBlock refused is skipped (ENTRIES_SKIPPED is not among the entries
    report's nbad: look at the block status)."""
    table, off, size, _, _ = sst_verify_table(file, filter_policy=filter_policy, stream=stream)
    if table["status"] != 0:
        return (None,) * 6 + (table, None, None)
    nd = table["ndata"]
    out, out_off, out_len, rstatus = sst_read_blocks(file, off[:nd], size[:nd], max_ulen=max_ulen,
                                                     verify=verify, stream=stream)
    e = sst_read_entries(out, out_off, out_len, skip=rstatus, stream=stream)
    return e[:6] + (table, rstatus, e[8])


MERGE_OK, MERGE_UNSORTED, MERGE_BAD_KEY, MERGE_CAPACITY, MERGE_BAD_RUNS = range(5)
MERGE_MAX_RUNS = 64
MERGE_COMPACT = 1


class SstMergeReport(ctypes.Structure):
    """lvkv_sst_merge_report (include/lvkv_snappy.h)."""
    _fields_ = [("status", ctypes.c_int32), ("first_bad_entry", ctypes.c_uint32),
                ("num_in", ctypes.c_uint32), ("num_out", ctypes.c_uint32),
                ("num_hidden", ctypes.c_uint32), ("num_obsolete", ctypes.c_uint32),
                ("max_key_len", ctypes.c_uint32), ("reserved_", ctypes.c_uint32),
                ("key_bytes", ctypes.c_uint64), ("value_bytes", ctypes.c_uint64)]

    def as_dict(self) -> dict:
        return {k: getattr(self, k) for k, _ in self._fields_ if not k.endswith("_")}


def _pack_deeper(torch, dev, deeper):
    """[(smallest, largest) user keys] -> (keys uint8, offsets int64, lengths
    int32) on the device, range g at 2g and 2g + 1."""
    flat = [bytes(k) for pair in deeper for k in pair]
    offs, at = [], 0
    for k in flat:
        offs.append(at)
        at += len(k)
    keys = torch.tensor(list(b"".join(flat)) or [0], dtype=torch.uint8, device=dev)
    return (keys, torch.tensor(offs, dtype=torch.int64, device=dev),
            torch.tensor([len(k) for k in flat], dtype=torch.int32, device=dev))


def sst_merge_entries(keys, key_off, key_len, vals, val_off, val_len, run_first, *,
                      key_format: int = 1, compact: bool = False, smallest_snapshot: int = 0,
                      deeper=None, max_out: Optional[int] = None, stream=None):
    """MergingIterator's forward walk over sorted runs of entries, with
    DoCompactionWork's drops when compact (lvkv_sst_merge_entries_device). The
    six entry arrays are sst_build_blocks'; they hold the runs laid end to
    end, run r being entries run_first[r] .. run_first[r + 1] (int64 CUDA
    tensor of nruns + 1, or a list). deeper: [(smallest, largest)] user keys
    of the files in levels level + 2 and deeper, as bytes. Returns (out_key_off
    int64, out_key_len int32, out_val_off int64, out_val_len int32 -- with keys
    and vals, sst_build_blocks' inputs -- src int32, dropped_src int32, report
    dict): the survivors in merged order, cut to report['num_out'], each the
    input entry src[j]; dropped_src the dropped entries' input indices in
    merged order. report['status'] is MERGE_*, and the arrays are empty unless
    it is MERGE_OK. The report is the one thing read back."""
    torch = _torch()
    n = key_off.numel()
    dev = keys.device
    if not (key_len.numel() == val_off.numel() == val_len.numel() == n):
        raise ValueError("the entry arrays differ in length")
    if not isinstance(run_first, torch.Tensor):
        run_first = torch.tensor(list(run_first), dtype=torch.int64, device=dev)
    nruns = run_first.numel() - 1
    if max_out is None:
        max_out = n
    deeper = list(deeper or [])
    dkeys, doff, dlen = _pack_deeper(torch, dev, deeper) if deeper else (None, None, None)
    scratch = torch.empty(int(_lib.lvkv_sst_merge_entries_scratch_bytes(n, max(nruns, 0))),
                          dtype=torch.uint8, device=dev)
    slots = max(1, max_out)
    out_key_off = torch.empty(slots, dtype=torch.int64, device=dev)
    out_key_len = torch.empty(slots, dtype=torch.int32, device=dev)
    out_val_off = torch.empty(slots, dtype=torch.int64, device=dev)
    out_val_len = torch.empty(slots, dtype=torch.int32, device=dev)
    src = torch.empty(slots, dtype=torch.int32, device=dev)
    dropped = torch.empty(max(1, n), dtype=torch.int32, device=dev)
    rep = torch.zeros(ctypes.sizeof(SstMergeReport), dtype=torch.uint8, device=dev)
    b8 = (torch.uint8, torch.int8)
    with torch.cuda.device(dev):
        rc = _lib.lvkv_sst_merge_entries_device(
            _dev_ptr(keys, "keys", b8) if n else None,
            _dev_ptr(key_off, "key_off", (torch.int64,)) if n else None,
            _dev_ptr(key_len, "key_len", (torch.int32,)) if n else None,
            _dev_ptr(vals, "vals", b8) if n else None,
            _dev_ptr(val_off, "val_off", (torch.int64,)) if n else None,
            _dev_ptr(val_len, "val_len", (torch.int32,)) if n else None, n,
            _dev_ptr(run_first, "run_first", (torch.int64,)), max(nruns, 0), int(key_format),
            MERGE_COMPACT if compact else 0, int(smallest_snapshot),
            _dev_ptr(dkeys, "deeper keys") if deeper else None,
            _dev_ptr(doff, "deeper offsets") if deeper else None,
            _dev_ptr(dlen, "deeper lengths") if deeper else None, len(deeper),
            _dev_ptr(scratch, "scratch", b8), scratch.numel(),
            _dev_ptr(out_key_off, "out_key_off"), _dev_ptr(out_key_len, "out_key_len"),
            _dev_ptr(out_val_off, "out_val_off"), _dev_ptr(out_val_len, "out_val_len"),
            _dev_ptr(src, "src"), int(max_out), _dev_ptr(dropped, "dropped_src"),
            _dev_ptr(rep, "report"), _stream_handle(stream, dev))
    _check("lvkv_sst_merge_entries_device", rc)
    if stream is not None:
        stream.synchronize()
    report = SstMergeReport.from_buffer_copy(bytes(rep.cpu().numpy())).as_dict()
    ok = report["status"] == MERGE_OK
    no = report["num_out"] if ok else 0
    nd = report["num_hidden"] + report["num_obsolete"] if ok else 0
    return (out_key_off[:no], out_key_len[:no], out_val_off[:no], out_val_len[:no], src[:no],
            dropped[:nd], report)


GET_BLOCK, GET_PAST_END, GET_FILTERED, GET_INDEX_CORRUPT, GET_BAD_HANDLE, GET_BAD_KEY = range(6)
(GET_STATE_NOT_FOUND, GET_STATE_FOUND, GET_STATE_DELETED, GET_STATE_CORRUPT_KEY,
 GET_STATE_BAD_BLOCK, GET_STATE_BAD_ENTRY, GET_STATE_UNREADABLE, GET_STATE_BAD_KEY) = range(8)
GET_NO_SLOT = -1  # d_q_slot 0xFFFFFFFF as int32


class SstGetLocateReport(ctypes.Structure):
    """lvkv_sst_get_locate_report (include/lvkv_snappy.h)."""
    _fields_ = [("nqueries", ctypes.c_uint32), ("count", ctypes.c_uint32 * 6),
                ("reserved_", ctypes.c_uint32)]

    def as_dict(self) -> dict:
        return {"nqueries": self.nqueries, "count": list(self.count)}


class SstGetSeekReport(ctypes.Structure):
    """lvkv_sst_get_seek_report (include/lvkv_snappy.h)."""
    _fields_ = [("nqueries", ctypes.c_uint32), ("count", ctypes.c_uint32 * 8)]

    def as_dict(self) -> dict:
        return {"nqueries": self.nqueries, "count": list(self.count)}


def sst_get_locate(index, filter, qkeys, qkey_off, qkey_len, *, key_format: int = 1,
                   stream=None):
    """The index seek and the filter of Table::InternalGet for a batch of keys
    (lvkv_sst_get_locate_device). index: the decoded index block (uint8 CUDA
    tensor, all of it); filter: the decoded filter block, or None for no
    policy; query q is qkeys[qkey_off[q] : qkey_off[q] + qkey_len[q]]
    (key_format 1: LookupKey::internal_key(), 0: plain bytes). Returns (block
    int32 -- the index entry's ordinal, -1 for none --, handle offsets int64,
    handle sizes int32, status uint8 GET_*, report dict). The report is the
    one thing read back."""
    torch = _torch()
    n = qkey_off.numel()
    dev = index.device
    if qkey_len.numel() != n:
        raise ValueError("the query arrays differ in length")
    scratch = torch.empty(int(_lib.lvkv_sst_get_locate_scratch_bytes(index.numel(), n)),
                          dtype=torch.uint8, device=dev)
    slots = max(1, n)
    block = torch.empty(slots, dtype=torch.int32, device=dev)
    hoff = torch.empty(slots, dtype=torch.int64, device=dev)
    hsize = torch.empty(slots, dtype=torch.int32, device=dev)
    status = torch.empty(slots, dtype=torch.uint8, device=dev)
    rep = torch.zeros(ctypes.sizeof(SstGetLocateReport), dtype=torch.uint8, device=dev)
    b8 = (torch.uint8, torch.int8)
    with torch.cuda.device(dev):
        rc = _lib.lvkv_sst_get_locate_device(
            _dev_ptr(index, "index", b8), index.numel(),
            _dev_ptr(filter, "filter", b8) if filter is not None else None,
            filter.numel() if filter is not None else 0,
            _dev_ptr(qkeys, "qkeys", b8) if n else None,
            _dev_ptr(qkey_off, "qkey_off", (torch.int64,)) if n else None,
            _dev_ptr(qkey_len, "qkey_len", (torch.int32,)) if n else None, n, int(key_format),
            _dev_ptr(scratch, "scratch", b8), scratch.numel(), _dev_ptr(block, "block"),
            _dev_ptr(hoff, "handle_off"), _dev_ptr(hsize, "handle_size"),
            _dev_ptr(status, "status"), _dev_ptr(rep, "report"), _stream_handle(stream, dev))
    _check("lvkv_sst_get_locate_device", rc)
    if stream is not None:
        stream.synchronize()
    report = SstGetLocateReport.from_buffer_copy(bytes(rep.cpu().numpy())).as_dict()
    return block[:n], hoff[:n], hsize[:n], status[:n], report


def sst_get_seek(raw, raw_off, raw_len, qkeys, qkey_off, qkey_len, q_slot, *, skip=None,
                 key_format: int = 1, stream=None):
    """The data block seek and SaveValue of Table::InternalGet for a batch of
    keys (lvkv_sst_get_seek_device). The blocks are sst_read_blocks' out,
    out_offsets and lengths (skip: its status); q_slot[q] (int32) is the block
    query q seeks in, GET_NO_SLOT for none. Returns (state uint8 GET_STATE_*,
    hit_off int32 -- -1 for none --, val_off int64 into raw, val_len int32,
    tag int64, report dict). The report is the one thing read back."""
    torch = _torch()
    n = qkey_off.numel()
    nb = raw_off.numel()
    dev = qkeys.device
    if qkey_len.numel() != n or q_slot.numel() != n:
        raise ValueError("the query arrays differ in length")
    if raw_len.numel() != nb or (skip is not None and skip.numel() != nb):
        raise ValueError("the block arrays differ in length")
    if nb == 0:  # (no block to seek in: the pointers still have to be some)
        raw = torch.zeros(8, dtype=torch.uint8, device=dev)
        raw_off = torch.zeros(1, dtype=torch.int64, device=dev)
        raw_len = torch.zeros(1, dtype=torch.int32, device=dev)
        skip = None
    slots = max(1, n)
    scratch = torch.empty(int(_lib.lvkv_sst_get_seek_scratch_bytes(n)), dtype=torch.uint8,
                          device=dev)
    state = torch.empty(slots, dtype=torch.uint8, device=dev)
    hit = torch.empty(slots, dtype=torch.int32, device=dev)
    voff = torch.empty(slots, dtype=torch.int64, device=dev)
    vlen = torch.empty(slots, dtype=torch.int32, device=dev)
    tag = torch.empty(slots, dtype=torch.int64, device=dev)
    rep = torch.zeros(ctypes.sizeof(SstGetSeekReport), dtype=torch.uint8, device=dev)
    b8 = (torch.uint8, torch.int8)
    with torch.cuda.device(dev):
        rc = _lib.lvkv_sst_get_seek_device(
            _dev_ptr(raw, "raw", b8), _dev_ptr(raw_off, "raw_off", (torch.int64,)),
            _dev_ptr(raw_len, "raw_len", (torch.int32,)),
            _dev_ptr(skip, "skip", (torch.uint8,)) if skip is not None else None, nb,
            _dev_ptr(qkeys, "qkeys", b8) if n else None,
            _dev_ptr(qkey_off, "qkey_off", (torch.int64,)) if n else None,
            _dev_ptr(qkey_len, "qkey_len", (torch.int32,)) if n else None,
            _dev_ptr(q_slot, "q_slot", (torch.int32,)) if n else None, n, int(key_format),
            _dev_ptr(scratch, "scratch", b8), scratch.numel(), _dev_ptr(hit, "hit_off"), _dev_ptr(voff, "val_off"), _dev_ptr(vlen, "val_len"),
            _dev_ptr(tag, "tag"), _dev_ptr(state, "state"), _dev_ptr(rep, "report"),
            _stream_handle(stream, dev))
    _check("lvkv_sst_get_seek_device", rc)
    if stream is not None:
        stream.synchronize()
    report = SstGetSeekReport.from_buffer_copy(bytes(rep.cpu().numpy())).as_dict()
    return state[:n], hit[:n], voff[:n], vlen[:n], tag[:n], report


def _read_one_block(file, off: int, size: int, *, max_ulen: int, verify: bool, stream):
    """One block of the image, whatever its decoded length: a first guess of
    the room, once more with what ReadBlock says it needs. Returns (contents
    uint8 or None, READ_* status)."""
    torch = _torch()
    dev = file.device
    if off + size + 5 > file.numel():
        return None, READ_BAD_TYPE
    cap = max(4 * size, 4096)
    for _ in range(2):
        out, _, out_len, status = sst_read_blocks(
            file, torch.tensor([off], dtype=torch.int64, device=dev),
            torch.tensor([size], dtype=torch.int32, device=dev), max_ulen=max_ulen, verify=verify,
            out=torch.empty(cap, dtype=torch.uint8, device=dev),
            out_offsets=torch.zeros(1, dtype=torch.int64, device=dev),
            out_caps=torch.tensor([cap], dtype=torch.int32, device=dev), stream=stream)
        if stream is not None:
            stream.synchronize()
        st, ln = int(status.cpu()[0]), int(out_len.cpu()[0])
        if st != READ_CAPACITY:
            break
        cap = ln
    return (out[:ln] if st == READ_OK else None), st


def _meta_filter_handle(file, table, filter_policy: str, **read):
    """Table::ReadMeta (table/table.cc:81-105): the handle under the exact key
    "filter." + policy in the metaindex block, or None -- the lookup is a
    seek with plain keys in that one block."""
    torch = _torch()
    dev = file.device
    meta, _ = _read_one_block(file, table["meta_offset"], table["meta_size"], **read)
    if meta is None:
        return None
    key = b"filter." + filter_policy.encode()
    state, _, voff, vlen, _, _ = sst_get_seek(
        meta, torch.zeros(1, dtype=torch.int64, device=dev),
        torch.tensor([meta.numel()], dtype=torch.int32, device=dev),
        torch.tensor(list(key), dtype=torch.uint8, device=dev),
        torch.zeros(1, dtype=torch.int64, device=dev),
        torch.tensor([len(key)], dtype=torch.int32, device=dev),
        torch.zeros(1, dtype=torch.int32, device=dev), key_format=0, stream=read["stream"])
    if int(state.cpu()[0]) != GET_STATE_FOUND:
        return None
    at, n = int(voff.cpu()[0]), int(vlen.cpu()[0])
    value, out, p = bytes(meta[at:at + n].cpu().numpy()), [], 0
    for _ in range(2):  # BlockHandle::DecodeFrom
        v, shift = 0, 0
        while True:
            if p >= len(value) or shift > 63:
                return None
            b = value[p]
            p += 1
            v |= (b & 127) << shift
            shift += 7
            if not b & 128:
                break
        out.append(v)
    return out[0], out[1]


def sst_get(file, qkeys, qkey_off, qkey_len, *, filter_policy: Optional[str] = None,
            key_format: int = 1, max_ulen: int, verify: bool = True, stream=None):
    """Table::InternalGet for a batch of keys on one table image in device
    memory: sst_verify_table (the footer's handles, the filter's), the index
    and filter blocks through sst_read_blocks, sst_get_locate, one
    sst_read_blocks over the distinct data blocks the GET_BLOCK queries name
    (max_ulen: the longest decoded data block) and sst_get_seek in them. The
    reports are read on the host between the steps; a batch whose every query
    is filtered or past the end decodes no data block. Returns a dict: state
    (uint8 GET_STATE_*), val_off / val_len into `values` (the decoded blocks),
    tag, hit_off, status (uint8 GET_*: the locate verdicts), block, raw_off /
    raw_len / read_status (the decoded blocks, one a distinct block), and the
    reports table, locate, seek. When the table does not open (table['status']
    != 0) or its index block cannot be read, only the reports are there (index
    status under 'index_read'). One exception: sst_verify_table stops at a
    compressed index block (status 6 with a sound checksum); the index is
    decoded here all the same, and the filter block is then found through the
    metaindex block. Which table of a version a key is looked up in, and in
    what order, stays the caller's."""
    torch = _torch()
    dev = file.device
    n = qkey_off.numel()
    table, off, size, _, vstatus = sst_verify_table(file, filter_policy=filter_policy,
                                                    stream=stream)
    res = {"table": table}
    # (the verifier has no codec for a compressed index block: it reports the
    # footer's handles and stops; the index is decoded here all the same)
    packed_index = table["status"] == 6 and table["index_status"] == 6
    if table["status"] != 0 and not packed_index:
        return res
    small = min(max_ulen, SNAPPY_MAX_BLOCK)
    read = dict(max_ulen=small, verify=verify, stream=stream)
    index, ist = _read_one_block(file, table["index_offset"], table["index_size"], **read)
    res["index_read"] = ist
    if index is None:
        return res
    filt = None
    if filter_policy is not None:
        # (a filter block that cannot be read is no filter: Table::ReadFilter)
        nd = table["ndata"]
        if packed_index:
            h = _meta_filter_handle(file, table, filter_policy, **read)
        elif table["has_filter"] and int(vstatus[nd].cpu()) == 0:
            h = int(off[nd].cpu()), int(size[nd].cpu()) & 0xFFFFFFFF
        else:
            h = None
        if h is not None:
            filt, _ = _read_one_block(file, h[0], h[1], **read)
    block, hoff, hsize, status, locate = sst_get_locate(index, filt, qkeys, qkey_off, qkey_len,
                                                        key_format=key_format, stream=stream)
    slot = torch.full((n,), GET_NO_SLOT, dtype=torch.int32, device=dev)
    raw = raw_off = raw_len = rstatus = None
    if locate["count"][GET_BLOCK] != 0:
        wanted = status == GET_BLOCK
        pairs = torch.stack([hoff[wanted], hsize[wanted].to(torch.int64) & 0xFFFFFFFF], dim=1)
        uniq, inverse = torch.unique(pairs, dim=0, return_inverse=True)
        # a handle that leaves the image is not read: its queries get a slot past the blocks
        inside = (uniq[:, 0] >= 0) & (uniq[:, 0] + uniq[:, 1] + 5 <= file.numel())
        place = torch.cumsum(inside.to(torch.int32), 0, dtype=torch.int32) - 1
        place = torch.where(inside, place, torch.full_like(place, 0x7FFFFFFF))
        slot[wanted] = place[inverse]
        uniq = uniq[inside]
        if uniq.shape[0] != 0:
            raw, raw_off, raw_len, rstatus = sst_read_blocks(
                file, uniq[:, 0].contiguous(), uniq[:, 1].to(torch.int32).contiguous(),
                max_ulen=max_ulen, verify=verify, stream=stream)
    if raw is None:
        raw = torch.zeros(8, dtype=torch.uint8, device=dev)
        raw_off = torch.zeros(0, dtype=torch.int64, device=dev)
        raw_len = torch.zeros(0, dtype=torch.int32, device=dev)
        rstatus = torch.zeros(0, dtype=torch.uint8, device=dev)
    state, hit, voff, vlen, tag, seek = sst_get_seek(raw, raw_off, raw_len, qkeys, qkey_off,
                                                     qkey_len, slot, skip=rstatus,
                                                     key_format=key_format, stream=stream)
    res.update(state=state, val_off=voff, val_len=vlen, values=raw, tag=tag, hit_off=hit,
               status=status, block=block, raw_off=raw_off, raw_len=raw_len, read_status=rstatus,
               locate=locate, seek=seek)
    return res


# --------------------------------------------------------------------------
# KV separation: the vTable (include/lvkv_vtable.h)

VTABLE_OK, VTABLE_BAD_KEY, VTABLE_BAD_VALUE, VTABLE_TOO_LARGE, VTABLE_CAPACITY = range(5)
VTABLE_NO_ENTRY = 0xFFFFFFFF
(VRES_OK, VRES_SKIPPED, VRES_EMPTY, VRES_BAD_TYPE, VRES_BAD_INDEX, VRES_BAD_HANDLE, VRES_NO_FILE,
 VRES_PAST_END, VRES_BAD_HEADER, VRES_BAD_RECORD, VRES_TRAILING, VRES_RECORD_OVERRUN) = range(12)


class VtableSeparateReport(ctypes.Structure):
    """lvkv_vtable_separate_report (include/lvkv_vtable.h)."""
    _fields_ = [("status", ctypes.c_int32), ("first_bad_entry", ctypes.c_uint32),
                ("records_num", ctypes.c_uint64), ("table_size", ctypes.c_uint64),
                ("out_val_bytes", ctypes.c_uint64), ("max_out_val_len", ctypes.c_uint32),
                ("reserved_", ctypes.c_uint32)]

    def as_dict(self) -> dict:
        return {k: getattr(self, k) for k, _ in self._fields_ if k != "reserved_"}


class VtableResolveReport(ctypes.Structure):
    """lvkv_vtable_resolve_report (include/lvkv_vtable.h)."""
    _fields_ = [("nqueries", ctypes.c_uint32), ("count", ctypes.c_uint32 * 12),
                ("max_len", ctypes.c_uint32), ("total_len", ctypes.c_uint64)]

    def as_dict(self) -> dict:
        return {"nqueries": self.nqueries, "count": list(self.count), "max_len": self.max_len,
                "total_len": self.total_len}


class VtableGatherReport(ctypes.Structure):
    """lvkv_vtable_gather_report (include/lvkv_vtable.h)."""
    _fields_ = [("status", ctypes.c_int32), ("nvalues", ctypes.c_uint32),
                ("dst_bytes", ctypes.c_uint64)]

    def as_dict(self) -> dict:
        return {k: getattr(self, k) for k, _ in self._fields_}


def _read_report(cls, rep, stream):
    if stream is not None:
        stream.synchronize()
    return cls.from_buffer_copy(bytes(rep.cpu().numpy())).as_dict()


def vtable_separate(keys, key_off, key_len, vals, val_off, val_len, *, kv_sep_size: int = 1000,
                    file_number: int, vtb=None, out_vals=None, scratch=None, stream=None):
    """BuildTable's loop (lvkv_vtable_separate_device): every entry whose value
    has kv_sep_size bytes or more moves into the vTable image `vtb` as a
    VTableRecord (user key, the value without its first byte) and gets a
    VTableIndex for a value; the others keep theirs. Entries as for
    sst_build_blocks, keys internal keys. vtb / out_vals: allocated by the
    bounds when None. Returns a dict: vtb, out_vals, out_val_off (int64),
    out_val_len (int32) -- with the key arrays, sst_build_blocks' arguments --,
    rec_off / rec_size (int64; 0 / 0 for an entry that stays) and report
    (status VTABLE_*; nothing is written unless it is VTABLE_OK; on
    VTABLE_CAPACITY table_size and out_val_bytes say what is needed). The
    report is the one thing read back."""
    torch = _torch()
    n = key_off.numel()
    dev = keys.device
    if not (key_len.numel() == val_off.numel() == val_len.numel() == n):
        raise ValueError("the entry arrays differ in length")
    if vtb is None or out_vals is None:
        kb = int(key_len.to(torch.int64).sum().item()) if n else 0
        vb = int((val_len.to(torch.int64) & 0xFFFFFFFF).sum().item()) if n else 0
        if vtb is None:
            vtb = torch.empty(max(1, int(_lib.lvkv_vtable_separate_vtb_bound(n, kb, vb))),
                              dtype=torch.uint8, device=dev)
        if out_vals is None:
            out_vals = torch.empty(max(1, int(_lib.lvkv_vtable_separate_vals_bound(n, vb))),
                                   dtype=torch.uint8, device=dev)
    if scratch is None:
        scratch = torch.empty(int(_lib.lvkv_vtable_separate_scratch_bytes(n)), dtype=torch.uint8,
                              device=dev)
    slots = max(1, n)
    ooff = torch.empty(slots, dtype=torch.int64, device=dev)
    olen = torch.empty(slots, dtype=torch.int32, device=dev)
    roff = torch.empty(slots, dtype=torch.int64, device=dev)
    rsize = torch.empty(slots, dtype=torch.int64, device=dev)
    rep = torch.zeros(ctypes.sizeof(VtableSeparateReport), dtype=torch.uint8, device=dev)
    b8 = (torch.uint8, torch.int8)
    with torch.cuda.device(dev):
        rc = _lib.lvkv_vtable_separate_device(
            _dev_ptr(keys, "keys", b8) if n else None,
            _dev_ptr(key_off, "key_off", (torch.int64,)) if n else None,
            _dev_ptr(key_len, "key_len", (torch.int32,)) if n else None,
            _dev_ptr(vals, "vals", b8) if n else None,
            _dev_ptr(val_off, "val_off", (torch.int64,)) if n else None,
            _dev_ptr(val_len, "val_len", (torch.int32,)) if n else None,
            n, int(kv_sep_size), int(file_number), _dev_ptr(scratch, "scratch", b8),
            scratch.numel(), _dev_ptr(vtb, "vtb", b8), vtb.numel(),
            _dev_ptr(out_vals, "out_vals", b8), out_vals.numel(), _dev_ptr(ooff, "out_val_off"),
            _dev_ptr(olen, "out_val_len"), _dev_ptr(roff, "rec_off"), _dev_ptr(rsize, "rec_size"),
            _dev_ptr(rep, "report"), _stream_handle(stream, dev))
    _check("lvkv_vtable_separate_device", rc)
    return dict(vtb=vtb, out_vals=out_vals, out_val_off=ooff[:n], out_val_len=olen[:n],
                rec_off=roff[:n], rec_size=rsize[:n],
                report=_read_report(VtableSeparateReport, rep, stream))


def _pack_vtables(torch, dev, vtables):
    """{file number: image} or [(file number, image)] -> one buffer and the
    three file arrays, ascending by number. An 8-byte buffer for no file."""
    items = sorted(vtables.items() if isinstance(vtables, dict) else vtables, key=lambda kv: kv[0])
    sizes = [img.numel() for _, img in items]
    offs = [0]
    for sz_ in sizes:
        offs.append(offs[-1] + sz_)
    vtb = (torch.cat([img for _, img in items]) if len(items) > 1 else
           items[0][1] if items else torch.zeros(8, dtype=torch.uint8, device=dev))
    if vtb.numel() == 0:
        vtb = torch.zeros(8, dtype=torch.uint8, device=dev)
    def arr(xs):
        # (file numbers are u64: two's complement into int64)
        return torch.tensor([x - (1 << 64) if x >= 1 << 63 else x for x in xs] or [0],
                            dtype=torch.int64, device=dev)[:len(xs)]
    return vtb, arr(offs[:-1]), arr(sizes), arr([k for k, _ in items])


def vtable_resolve(vals, val_off, val_len, vtb, file_off, file_size, file_number, *, state=None,
                   stream=None):
    """DecodeValue and VTableReader::Get for a batch of values
    (lvkv_vtable_resolve_device): value q is vals[val_off[q] : + val_len[q]];
    the vTable images lie in `vtb` at file_off / file_size under file_number
    (int64 tensors, ascending by number; empty for none). state: sst_get_seek's
    -- only GET_STATE_FOUND queries are looked at. Returns (status uint8
    VRES_*, src uint8 -- 0: vals, 1: vtb --, off int64, len int32, report
    dict). No value byte is copied; the report is the one thing read back."""
    torch = _torch()
    n = val_off.numel()
    nf = file_number.numel()
    dev = vals.device
    if val_len.numel() != n or (state is not None and state.numel() != n):
        raise ValueError("the query arrays differ in length")
    if file_off.numel() != nf or file_size.numel() != nf:
        raise ValueError("the file arrays differ in length")
    scratch = torch.empty(int(_lib.lvkv_vtable_resolve_scratch_bytes(n)), dtype=torch.uint8,
                          device=dev)
    slots = max(1, n)
    status = torch.empty(slots, dtype=torch.uint8, device=dev)
    src = torch.empty(slots, dtype=torch.uint8, device=dev)
    off = torch.empty(slots, dtype=torch.int64, device=dev)
    ln = torch.empty(slots, dtype=torch.int32, device=dev)
    rep = torch.zeros(ctypes.sizeof(VtableResolveReport), dtype=torch.uint8, device=dev)
    b8 = (torch.uint8, torch.int8)
    i64 = (torch.int64,)
    with torch.cuda.device(dev):
        rc = _lib.lvkv_vtable_resolve_device(
            _dev_ptr(vals, "vals", b8) if n else None,
            _dev_ptr(val_off, "val_off", i64) if n else None,
            _dev_ptr(val_len, "val_len", (torch.int32,)) if n else None,
            _dev_ptr(state, "state", (torch.uint8,)) if state is not None and n else None, n,
            _dev_ptr(vtb, "vtb", b8) if nf else None,
            _dev_ptr(file_off, "file_off", i64) if nf else None,
            _dev_ptr(file_size, "file_size", i64) if nf else None,
            _dev_ptr(file_number, "file_number", i64) if nf else None, nf,
            _dev_ptr(scratch, "scratch", b8), scratch.numel(), _dev_ptr(status, "status"),
            _dev_ptr(src, "src"), _dev_ptr(off, "off"), _dev_ptr(ln, "len"),
            _dev_ptr(rep, "report"), _stream_handle(stream, dev))
    _check("lvkv_vtable_resolve_device", rc)
    return status[:n], src[:n], off[:n], ln[:n], _read_report(VtableResolveReport, rep, stream)


def vtable_gather(vals, vtb, status, src, off, ln, *, dst=None, stream=None):
    """The values vtable_resolve found, end to end (lvkv_vtable_gather_device):
    query q's is dst[dst_off[q] : dst_off[q + 1]], empty unless its status is
    VRES_OK. dst: allocated to fit when None (the resolve report's total_len
    is not needed: the lengths are added up here). Returns (dst, dst_off int64
    of n + 1, report dict); on VTABLE_CAPACITY nothing is written."""
    torch = _torch()
    n = status.numel()
    dev = vals.device
    if not (src.numel() == off.numel() == ln.numel() == n):
        raise ValueError("the query arrays differ in length")
    if dst is None:
        need = int(((ln.to(torch.int64) & 0xFFFFFFFF) * (status == VRES_OK)).sum().item()) if n else 0
        dst = torch.empty(max(1, need), dtype=torch.uint8, device=dev)
    scratch = torch.empty(int(_lib.lvkv_vtable_gather_scratch_bytes(n)), dtype=torch.uint8,
                          device=dev)
    dst_off = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    rep = torch.zeros(ctypes.sizeof(VtableGatherReport), dtype=torch.uint8, device=dev)
    b8 = (torch.uint8, torch.int8)
    with torch.cuda.device(dev):
        rc = _lib.lvkv_vtable_gather_device(
            _dev_ptr(vals, "vals", b8) if n else None, _dev_ptr(vtb, "vtb", b8) if n else None,
            _dev_ptr(status, "status", (torch.uint8,)) if n else None,
            _dev_ptr(src, "src", (torch.uint8,)) if n else None,
            _dev_ptr(off, "off", (torch.int64,)) if n else None,
            _dev_ptr(ln, "len", (torch.int32,)) if n else None, n,
            _dev_ptr(scratch, "scratch", b8), scratch.numel(), _dev_ptr(dst, "dst", b8),
            dst.numel(), _dev_ptr(dst_off, "dst_off"), _dev_ptr(rep, "report"),
            _stream_handle(stream, dev))
    _check("lvkv_vtable_gather_device", rc)
    return dst, dst_off, _read_report(VtableGatherReport, rep, stream)


def sst_flush_separated(keys, key_off, key_len, vals, val_off, val_len, *,
                        kv_sep_size: int = 1000, file_number: int, stream=None, **table_options):
    """BuildTable on the device: vtable_separate, then sst_build_table on the
    values it left (table_options: sst_build_table's). Returns (table image,
    vTable image, reports): the images cut to their sizes (the vTable image
    empty when nothing moved, where the reference removes the file; the table
    None when a step failed), reports = {'separate', 'build', 'table'}."""
    sep = vtable_separate(keys, key_off, key_len, vals, val_off, val_len,
                          kv_sep_size=kv_sep_size, file_number=file_number, stream=stream)
    reports = {"separate": sep["report"], "build": None, "table": None}
    if sep["report"]["status"] != VTABLE_OK:
        return None, None, reports
    out = sst_build_table(keys, key_off, key_len, sep["out_vals"], sep["out_val_off"],
                          sep["out_val_len"], key_format=1, stream=stream, **table_options)
    reports["build"], reports["table"] = out[6], out[5]
    vtb = sep["vtb"][:sep["report"]["table_size"]]
    if out[0] is None or out[5]["status"] != 0:
        return None, vtb, reports
    return out[0][:out[5]["file_size"]], vtb, reports


def sst_get_values(file, vtables, qkeys, qkey_off, qkey_len, *, stream=None, **get_options):
    """Keys to values through the value log: sst_get on the table image `file`
    (get_options: sst_get's, key_format 1), vtable_resolve on what it found
    against `vtables` ({file number: vTable image}), vtable_gather. Returns a
    dict: values, value_off (int64 of n + 1: query q's value is values[
    value_off[q] : value_off[q + 1]]), status (uint8 VRES_*; VRES_SKIPPED for a
    key that is not there), state (sst_get's), and the reports get, resolve,
    gather. When the table does not open only 'get' is there."""
    torch = _torch()
    dev = file.device
    got = sst_get(file, qkeys, qkey_off, qkey_len, key_format=1, stream=stream, **get_options)
    res = {"get": got}
    if "state" not in got:
        return res
    vtb, foff, fsize, fnum = _pack_vtables(torch, dev, vtables)
    status, src, off, ln, rrep = vtable_resolve(got["values"], got["val_off"], got["val_len"], vtb,
                                                foff, fsize, fnum, state=got["state"],
                                                stream=stream)
    values, value_off, grep = vtable_gather(got["values"], vtb, status, src, off, ln,
                                            stream=stream)
    res.update(values=values, value_off=value_off, status=status, state=got["state"],
               resolve=rrep, gather=grep)
    return res


(MEMTABLE_OK, MEMTABLE_TOO_SMALL, MEMTABLE_UNKNOWN_TAG, MEMTABLE_BAD_PUT, MEMTABLE_BAD_DELETE,
 MEMTABLE_WRONG_COUNT, MEMTABLE_KEY_TOO_LONG, MEMTABLE_CAPACITY, MEMTABLE_DUPLICATE) = range(9)
MEMTABLE_NONE = 0xFFFFFFFF
MEMTABLE_PARANOID = 1
# where the device call changes path with the sizes (csrc/lvkv_launch.h)
MEMTABLE_WINDOW = 8192    # bytes of a batch its wave holds in LDS at a time
MEMTABLE_SORT_TILE = 1024  # pairs a workgroup sorts in LDS


class MemtableReport(ctypes.Structure):
    """lvkv_memtable_report (include/lvkv_memtable.h)."""
    _fields_ = [("status", ctypes.c_int32), ("first_bad_batch", ctypes.c_uint32),
                ("first_bad_entry", ctypes.c_uint32), ("nentries", ctypes.c_uint32),
                ("key_bytes", ctypes.c_uint64), ("val_bytes", ctypes.c_uint64),
                ("max_key_len", ctypes.c_uint32), ("n_too_small", ctypes.c_uint32),
                ("too_small_bytes", ctypes.c_uint64), ("max_sequence_out", ctypes.c_uint64),
                ("n_bad_batches", ctypes.c_uint32), ("reserved_", ctypes.c_uint32)]

    def as_dict(self) -> dict:
        return {k: getattr(self, k) for k, _ in self._fields_ if k != "reserved_"}


def memtable_from_batches(payload, batch_off, batch_len, *, max_sequence: int = 0,
                          paranoid: bool = False, max_entries: Optional[int] = None,
                          key_capacity: Optional[int] = None, scratch=None, stream=None):
    """RecoverLogFile's loop over the write batches of a WAL
    (lvkv_memtable_from_batches_device): batch b is payload[batch_off[b] :
    + batch_len[b]] (int64 tensors; log_read(gather=True)'s payload, its
    positions and its records' lengths). Every batch is walked as
    WriteBatch::Iterate walks it, every entry met gets MemTable::Add's internal
    key, and the entries come out in the memtable's iteration order.

    Returns (report dict, keys, key_off int64, key_len int32, vals, val_off
    int64, val_len int32, src int32, batch_status uint8, batch_entries int32):
    the six entry arrays are sst_build_blocks' and vtable_separate's arguments
    (vals is `payload`: no value byte is copied; keys holds the internal keys
    in log order), src[i] the log-order index of sorted entry i. The per-entry
    arrays are cut to the report's nentries, and are empty unless its status is
    MEMTABLE_OK. The default capacities always fit: entries <= payload bytes /
    2, key bytes <= payload bytes + 8 * entries. The report is the one thing
    read back."""
    torch = _torch()
    nb = batch_off.numel()
    dev = payload.device
    if batch_len.numel() != nb:
        raise ValueError("batch_off and batch_len differ in length")
    if max_entries is None or key_capacity is None:
        pb = min(int(batch_len.sum().item()), payload.numel()) if nb else 0
        if max_entries is None:
            max_entries = pb // 2
        if key_capacity is None:
            key_capacity = pb + 8 * max_entries
    if scratch is None:
        scratch = torch.empty(int(_lib.lvkv_memtable_scratch_bytes(nb, max_entries)),
                              dtype=torch.uint8, device=dev)
    slots = max(1, max_entries)
    keys = torch.empty(max(1, key_capacity), dtype=torch.uint8, device=dev)
    key_off = torch.empty(slots, dtype=torch.int64, device=dev)
    key_len = torch.empty(slots, dtype=torch.int32, device=dev)
    val_off = torch.empty(slots, dtype=torch.int64, device=dev)
    val_len = torch.empty(slots, dtype=torch.int32, device=dev)
    src = torch.empty(slots, dtype=torch.int32, device=dev)
    bst = torch.empty(max(1, nb), dtype=torch.uint8, device=dev)
    bent = torch.empty(max(1, nb), dtype=torch.int32, device=dev)
    rep = torch.zeros(ctypes.sizeof(MemtableReport), dtype=torch.uint8, device=dev)
    b8 = (torch.uint8, torch.int8)
    i64 = (torch.int64,)
    with torch.cuda.device(dev):
        rc = _lib.lvkv_memtable_from_batches_device(
            _dev_ptr(payload, "payload", b8) if nb else None,
            _dev_ptr(batch_off, "batch_off", i64) if nb else None,
            _dev_ptr(batch_len, "batch_len", i64) if nb else None, nb,
            int(max_sequence), MEMTABLE_PARANOID if paranoid else 0,
            _dev_ptr(scratch, "scratch", b8), scratch.numel(), _dev_ptr(keys, "keys"),
            int(key_capacity), _dev_ptr(key_off, "key_off"), _dev_ptr(key_len, "key_len"),
            _dev_ptr(val_off, "val_off"), _dev_ptr(val_len, "val_len"), _dev_ptr(src, "src"),
            int(max_entries), _dev_ptr(bst, "batch_status"), _dev_ptr(bent, "batch_entries"),
            _dev_ptr(rep, "report"), _stream_handle(stream, dev))
    _check("lvkv_memtable_from_batches_device", rc)
    report = _read_report(MemtableReport, rep, stream)
    n = report["nentries"] if report["status"] == MEMTABLE_OK else 0
    return (report, keys, key_off[:n], key_len[:n], payload, val_off[:n], val_len[:n], src[:n],
            bst[:nb], bent[:nb])


def wal_recover_table(log_image, *, file_number: int, kv_sep_size: int, paranoid: bool = False,
                      max_sequence: int = 0, stream=None, **build_options):
    """A WAL image in device memory -> the level-0 table and vTable images
    DBImpl::RecoverLogFile writes for it (one memtable: the reference's switch
    to a new one at write_buffer_size is the caller's), no entry crossing to
    the host: log_read(gather=True), memtable_from_batches on its records,
    sst_flush_separated on the sorted entries (build_options: its
    table_options). Returns (table image, vTable image, reports, max_sequence);
    reports = {'log', 'log_corruptions', 'memtable', 'separate', 'build',
    'table'}. Both images are None when nothing is written: no entry was
    inserted (BuildTable removes the file), or -- paranoid -- a batch was bad
    or the log reader reported a corruption (max_sequence is then None: the
    reference stops at the report, and which batches came before it is not
    looked at here). The vTable image is empty when no value moved. The
    reports of the calls are read on the host in between."""
    torch = _torch()
    dev = log_image.device
    rd, records, corruptions, _, (payload, pos) = log_read(log_image, gather=True, stream=stream)
    reports = {"log": rd, "log_corruptions": corruptions, "memtable": None, "separate": None,
               "build": None, "table": None}
    if rd["status"] != 0:
        raise ValueError(f"the log does not read: {rd}")
    if paranoid and corruptions:
        return None, None, reports, None
    lens = torch.tensor([r[1] for r in records], dtype=torch.int64, device=dev)
    m = memtable_from_batches(payload, pos, lens, max_sequence=max_sequence, paranoid=paranoid,
                              stream=stream)
    reports["memtable"] = m[0]
    if m[0]["status"] != MEMTABLE_OK or m[0]["nentries"] == 0:
        return None, None, reports, m[0]["max_sequence_out"]
    table, vtb, flush = sst_flush_separated(*m[1:7], kv_sep_size=kv_sep_size,
                                            file_number=file_number, stream=stream,
                                            **build_options)
    reports.update(flush)
    return table, vtb, reports, m[0]["max_sequence_out"]


def sst_compact_tables(files, *, smallest_snapshot: int, deeper=None,
                       filter_policy: Optional[str] = None, max_ulen: int, verify: bool = True,
                       block_size: int = 4096, restart_interval: int = 16, compression: int = 1,
                       zstd_level: int = 1, filter_bits_per_key: int = 10, file=None,
                       file_capacity: Optional[int] = None, stream=None):
    """Table images in device memory -> one compacted table image in device
    memory, no entry crossing to the host: sst_read_table's steps on each image (a run
    an image, in the order given: for equal keys the earlier image's entry
    comes first), the key and value buffers laid end to end with their offsets
    shifted, sst_merge_entries(compact=True) with smallest_snapshot and the
    deeper levels' ranges, then sst_build_table over the survivors. The tables
    hold internal keys. Returns sst_build_table's tuple and the merge report:
    (file, handle offsets, handle sizes, types, status, table report, build
    report, merge report); the first seven are None when the merge's status is
    not MERGE_OK. An image that does not open, or a block of one that does not
    read or walk, raises ValueError: a compaction does not go on past a bad
    input. The reports of the calls are read on the host in between.

    One output table: cutting the output into several files (ShouldStopBefore,
    MaxOutputFileSize) and rewriting the vTable indices of the values are the
    caller's."""
    torch = _torch()
    parts, run_first = [], [0]
    key_base = val_base = 0
    dev = None
    for i, img in enumerate(files):
        dev = img.device
        # sst_read_table's three steps, with the table nothing was added to
        # taken for what it is: its index block is one restart point and no
        # entry (8 bytes), which the verifier, counting restart points, lists
        # as one handle that does not decode
        table, off, size, _, _ = sst_verify_table(img, filter_policy=filter_policy, stream=stream)
        if table["status"] != 0:
            raise ValueError(f"input table {i} does not open: status {table['status']}")
        nd = 0 if table["ndata"] == 1 and table["index_size"] == 8 else table["ndata"]
        out, out_off, out_len, rstatus = sst_read_blocks(img, off[:nd], size[:nd],
                                                         max_ulen=max_ulen, verify=verify,
                                                         stream=stream)
        t = sst_read_entries(out, out_off, out_len, skip=rstatus, stream=stream)
        erep = t[8]
        if erep["status"] != 0 or erep["nbad"] != 0 or bool(rstatus.any().item()):
            raise ValueError(f"input table {i} has a block that does not read: block status "
                             f"{rstatus.tolist()}, entries report {erep}")
        keys, key_off, key_len, vals, val_off, val_len = t[:6]
        kb = (erep["key_bytes"] + 7) & ~7  # the next run's keys stay 8 bytes apart
        parts.append((keys[:kb] if keys.numel() >= kb else
                      torch.cat([keys, keys.new_zeros(kb - keys.numel())]),
                      key_off + key_base, key_len, vals, val_off + val_base, val_len))
        key_base += kb
        val_base += vals.numel()
        run_first.append(run_first[-1] + key_off.numel())
    if not parts:
        raise ValueError("no input tables")
    keys, key_off, key_len, vals, val_off, val_len = (torch.cat([p[k] for p in parts])
                                                      for k in range(6))
    m = sst_merge_entries(keys, key_off, key_len, vals, val_off, val_len,
                          torch.tensor(run_first, dtype=torch.int64, device=dev), key_format=1,
                          compact=True, smallest_snapshot=smallest_snapshot, deeper=deeper,
                          stream=stream)
    if m[6]["status"] != MERGE_OK:
        return (None,) * 7 + (m[6],)
    built = sst_build_table(keys, m[0], m[1], vals, m[2], m[3], block_size=block_size,
                            restart_interval=restart_interval, key_format=1,
                            compression=compression, zstd_level=zstd_level,
                            filter_bits_per_key=filter_bits_per_key, file=file,
                            file_capacity=file_capacity, stream=stream)
    return built + (m[6],)


SCAN_OK, SCAN_UNSORTED, SCAN_BAD_KEY, SCAN_CAPACITY = range(4)
SCAN_Q_OK, SCAN_Q_CORRUPT = range(2)
SCAN_NONE = 0xFFFFFFFF
SCAN_NO_LIMIT = 0xFFFFFFFF
MAX_SEQUENCE_NUMBER = (1 << 56) - 1  # kMaxSequenceNumber (db/dbformat.h:69)


class SstScanReport(ctypes.Structure):
    """lvkv_sst_scan_report (include/lvkv_scan.h)."""
    _fields_ = [("status", ctypes.c_int32), ("first_bad_entry", ctypes.c_uint32),
                ("num_in", ctypes.c_uint32), ("num_visible", ctypes.c_uint32),
                ("num_above_snapshot", ctypes.c_uint32), ("num_unparsable", ctypes.c_uint32),
                ("num_deletions", ctypes.c_uint32), ("num_hidden", ctypes.c_uint32),
                ("key_bytes", ctypes.c_uint64), ("value_bytes", ctypes.c_uint64),
                ("nqueries", ctypes.c_uint32), ("max_count", ctypes.c_uint32),
                ("sum_count", ctypes.c_uint64)]

    def as_dict(self) -> dict:
        return {k: getattr(self, k) for k, _ in self._fields_}


def _pack_user_keys(torch, dev, keys):
    """[bytes] -> (buffer uint8, offsets, lengths as lists) end to end."""
    offs, at = [], 0
    for k in keys:
        offs.append(at)
        at += len(k)
    buf = torch.tensor(list(b"".join(bytes(k) for k in keys)) or [0], dtype=torch.uint8, device=dev)
    return buf, offs, [len(k) for k in keys]


def sst_scan_entries(keys, key_off, key_len, val_off, val_len, *, snapshot: int, qkeys=None,
                     start_off=None, start_len=None, limit_off=None, limit_len=None, q_max=None,
                     max_out: Optional[int] = None, stream=None):
    """DBIter over entries in MergingIterator's order at `snapshot`
    (lvkv_sst_scan_entries_device): which of them a reader sees, and for a
    batch of ranges where Seek lands and how many entries the loop `for
    (it->Seek(start); it->Valid() && n < max && it->key() < limit; it->Next())`
    counts. The entry arrays are sst_merge_entries' outputs without compact (or
    one sorted run); keys internal keys. Query q: start qkeys[start_off[q] : +
    start_len[q]], limit qkeys[limit_off[q] : + limit_len[q]] (user keys;
    limit_len -1, SCAN_NO_LIMIT as int32: none), q_max[q] (int32 tensor or
    None: unbounded). Returns a dict: key_off int64 / key_len int32 -- the
    visible entries' USER keys in `keys` --, val_off / val_len -- their values
    as stored --, src int32, cut to report['num_visible']; q_first / q_count
    int32 and q_status uint8 (SCAN_Q_*) per query: its entries are first ..
    first + count of that list; report. report['status'] is SCAN_*, and the
    arrays are empty unless it is SCAN_OK. The report is the one thing read
    back."""
    torch = _torch()
    n = key_off.numel()
    dev = keys.device
    if not (key_len.numel() == val_off.numel() == val_len.numel() == n):
        raise ValueError("the entry arrays differ in length")
    nq = start_off.numel() if start_off is not None else 0
    if nq and not (start_len.numel() == limit_off.numel() == limit_len.numel() == nq and
                   (q_max is None or q_max.numel() == nq)):
        raise ValueError("the query arrays differ in length")
    if max_out is None:
        max_out = n
    scratch = torch.empty(int(_lib.lvkv_sst_scan_entries_scratch_bytes(n, nq)), dtype=torch.uint8,
                          device=dev)
    slots = max(1, max_out)
    out_key_off = torch.empty(slots, dtype=torch.int64, device=dev)
    out_key_len = torch.empty(slots, dtype=torch.int32, device=dev)
    out_val_off = torch.empty(slots, dtype=torch.int64, device=dev)
    out_val_len = torch.empty(slots, dtype=torch.int32, device=dev)
    src = torch.empty(slots, dtype=torch.int32, device=dev)
    # (with no entry the call writes no per-query word: every count is 0)
    q_first = torch.zeros(max(1, nq), dtype=torch.int32, device=dev)
    q_count = torch.zeros(max(1, nq), dtype=torch.int32, device=dev)
    q_status = torch.zeros(max(1, nq), dtype=torch.uint8, device=dev)
    rep = torch.zeros(ctypes.sizeof(SstScanReport), dtype=torch.uint8, device=dev)
    b8 = (torch.uint8, torch.int8)
    i64, i32 = (torch.int64,), (torch.int32,)
    with torch.cuda.device(dev):
        rc = _lib.lvkv_sst_scan_entries_device(
            _dev_ptr(keys, "keys", b8) if n else None,
            _dev_ptr(key_off, "key_off", i64) if n else None,
            _dev_ptr(key_len, "key_len", i32) if n else None,
            _dev_ptr(val_off, "val_off", i64) if n else None,
            _dev_ptr(val_len, "val_len", i32) if n else None, n, int(snapshot),
            _dev_ptr(qkeys, "qkeys", b8) if nq else None,
            _dev_ptr(start_off, "start_off", i64) if nq else None,
            _dev_ptr(start_len, "start_len", i32) if nq else None,
            _dev_ptr(limit_off, "limit_off", i64) if nq else None,
            _dev_ptr(limit_len, "limit_len", i32) if nq else None,
            _dev_ptr(q_max, "q_max", i32) if nq and q_max is not None else None, nq,
            _dev_ptr(scratch, "scratch", b8), scratch.numel(),
            _dev_ptr(out_key_off, "out_key_off"), _dev_ptr(out_key_len, "out_key_len"),
            _dev_ptr(out_val_off, "out_val_off"), _dev_ptr(out_val_len, "out_val_len"),
            _dev_ptr(src, "src"), int(max_out), _dev_ptr(q_first, "q_first"),
            _dev_ptr(q_count, "q_count"), _dev_ptr(q_status, "q_status"), _dev_ptr(rep, "report"),
            _stream_handle(stream, dev))
    _check("lvkv_sst_scan_entries_device", rc)
    report = _read_report(SstScanReport, rep, stream)
    ok = report["status"] == SCAN_OK
    nv = report["num_visible"] if ok else 0
    nq = nq if ok else 0
    return dict(key_off=out_key_off[:nv], key_len=out_key_len[:nv], val_off=out_val_off[:nv],
                val_len=out_val_len[:nv], src=src[:nv], q_first=q_first[:nq], q_count=q_count[:nq],
                q_status=q_status[:nq], report=report)


def _read_run(img, i, *, filter_policy, max_ulen, verify, stream):
    """The entries of table image i as sst_read_table lists them, with the
    table nothing was added to taken for what it is (sst_compact_tables says
    why). An image or a block that does not read raises ValueError."""
    table, off, size, _, _ = sst_verify_table(img, filter_policy=filter_policy, stream=stream)
    if table["status"] != 0:
        raise ValueError(f"input table {i} does not open: status {table['status']}")
    nd = 0 if table["ndata"] == 1 and table["index_size"] == 8 else table["ndata"]
    out, out_off, out_len, rstatus = sst_read_blocks(img, off[:nd], size[:nd], max_ulen=max_ulen,
                                                     verify=verify, stream=stream)
    t = sst_read_entries(out, out_off, out_len, skip=rstatus, stream=stream)
    if t[8]["status"] != 0 or t[8]["nbad"] != 0 or bool(rstatus.any().item()):
        raise ValueError(f"input table {i} has a block that does not read: block status "
                         f"{rstatus.tolist()}, entries report {t[8]}")
    return t[:6]


def db_scan(files, vtables, starts, limits, *, snapshot: int, memtable=None, max_count=None,
            reverse: bool = False, filter_policy: Optional[str] = None, max_ulen: int,
            verify: bool = True, stream=None):
    """DB::NewIterator at `snapshot` and, per range, the loop `for
    (it->Seek(start); it->Valid() && n < max && it->key() < limit; it->Next())`
    with DBIter::fields()' DecodeValue on each value, over table images in
    device memory and no entry crossing to the host: sst_read_table's steps on
    each image (a run an image, in the order given: newer files first, as
    Version::AddIterators lists level 0), before them as run 0 the `memtable`
    entries (memtable_from_batches' six entry arrays), sst_merge_entries
    without compact, sst_scan_entries, then vtable_resolve and vtable_gather on
    the selected entries' values against `vtables` ({file number: vTable
    image}) and vtable_gather again on the key buffer for the user keys.
    starts / limits: user keys as bytes, a limit of None for no limit;
    max_count: None, one int, or one int or None a range. A Get of key k across
    the runs is the range (k, k + b'\\0', 1).

    Returns a dict: query_off (int64 of nq + 1: range q's entries are
    query_off[q] .. query_off[q + 1] of the lists), keys / key_off (int64 of
    total + 1: entry e's user key is keys[key_off[e] : key_off[e + 1]]), values
    / value_off likewise (the value DecodeValue leaves: empty unless status[e]
    is VRES_OK), status (uint8 VRES_* an entry), q_status (uint8 SCAN_Q_* a
    range), and the reports merge, scan, resolve, gather. With reverse=True a
    range's entries come last first (the slice the SeekToLast / Prev walk
    crosses: over sorted entries that walk yields the forward list backwards).
    When the merge or the scan does not end OK only the reports are there.
    The per-range index lists are built on the device; the reports are read on
    the host in between."""
    torch = _torch()
    if len(starts) != len(limits):
        raise ValueError("starts and limits differ in length")
    nq = len(starts)
    if max_count is None or isinstance(max_count, int):
        max_count = [max_count] * nq
    if len(max_count) != nq:
        raise ValueError("max_count and starts differ in length")
    parts, run_first = [], [0]
    key_base = val_base = 0
    runs = ([tuple(memtable[:6])] if memtable is not None else []) + \
        [_read_run(img, i, filter_policy=filter_policy, max_ulen=max_ulen, verify=verify,
                   stream=stream) for i, img in enumerate(files)]
    if not runs:
        raise ValueError("no input runs")
    for keys, key_off, key_len, vals, val_off, val_len in runs:
        kb = (keys.numel() + 7) & ~7  # the next run's keys stay 8 bytes apart
        parts.append((torch.cat([keys, keys.new_zeros(kb - keys.numel())]), key_off + key_base,
                      key_len, vals, val_off + val_base, val_len))
        key_base += kb
        val_base += vals.numel()
        run_first.append(run_first[-1] + key_off.numel())
    keys, key_off, key_len, vals, val_off, val_len = (torch.cat([p[k] for p in parts])
                                                      for k in range(6))
    dev = keys.device
    m = sst_merge_entries(keys, key_off, key_len, vals, val_off, val_len,
                          torch.tensor(run_first, dtype=torch.int64, device=dev), key_format=1,
                          stream=stream)
    res = {"merge": m[6]}
    if m[6]["status"] != MERGE_OK:
        return res
    qbuf, offs, lens = _pack_user_keys(torch, dev, list(starts) + [l or b"" for l in limits])
    i64 = lambda v: torch.tensor(v, dtype=torch.int64, device=dev)
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=dev)
    s = sst_scan_entries(
        keys, m[0], m[1], m[2], m[3], snapshot=snapshot, qkeys=qbuf,
        start_off=i64(offs[:nq]), start_len=i32(lens[:nq]), limit_off=i64(offs[nq:]),
        limit_len=i32([-1 if l is None else len(l) for l in limits]),
        q_max=i32([-1 if c is None else min(int(c), 0x7FFFFFFF) for c in max_count]),
        stream=stream) if nq else None
    if nq == 0:
        res["scan"] = None
        total = 0
    else:
        res["scan"] = s["report"]
        if s["report"]["status"] != SCAN_OK:
            return res
        total = s["report"]["sum_count"]
    query_off = torch.zeros(nq + 1, dtype=torch.int64, device=dev)
    empty8 = torch.zeros(0, dtype=torch.uint8, device=dev)
    res.update(query_off=query_off, keys=empty8, key_off=query_off[:1].clone(), values=empty8,
               value_off=query_off[:1].clone(), status=empty8,
               q_status=s["q_status"] if nq else empty8, resolve=None, gather=None)
    if total == 0:
        return res
    # the entries of range q: slots first[q] .. first[q] + count[q] of the
    # visible list, end to end (last first with reverse)
    count = s["q_count"].to(torch.int64)
    query_off[1:] = torch.cumsum(count, 0)
    q_of = torch.repeat_interleave(torch.arange(nq, device=dev), count, output_size=total)
    within = torch.arange(total, device=dev) - query_off[q_of]
    if reverse:
        within = count[q_of] - 1 - within
    sel = s["q_first"].to(torch.int64)[q_of] + within
    vtb, foff, fsize, fnum = _pack_vtables(torch, dev, vtables)
    status, src, off, ln, rrep = vtable_resolve(vals, s["val_off"][sel].contiguous(),
                                                s["val_len"][sel].contiguous(), vtb, foff, fsize,
                                                fnum, stream=stream)
    values, value_off, grep = vtable_gather(vals, vtb, status, src, off, ln, stream=stream)
    # the user keys: a gather from the key buffer, every entry in it
    zeros = torch.zeros(total, dtype=torch.uint8, device=dev)
    ukeys, ukey_off, _ = vtable_gather(keys, keys, zeros, zeros, s["key_off"][sel].contiguous(),
                                       s["key_len"][sel].contiguous(), stream=stream)
    res.update(keys=ukeys, key_off=ukey_off, values=values, value_off=value_off, status=status,
               resolve=rrep, gather=grep)
    return res


class LogReport(ctypes.Structure):
    """lvkv_log_report (include/lvkv_crc32c.h)."""
    _fields_ = [("status", ctypes.c_int32), ("nblocks", ctypes.c_uint32),
                ("nrecords", ctypes.c_uint32), ("ngood", ctypes.c_uint32),
                ("ncorrupt", ctypes.c_uint32), ("first_bad_block", ctypes.c_uint32),
                ("dropped_bytes", ctypes.c_uint64), ("count_", ctypes.c_uint32),
                ("reserved_", ctypes.c_uint32)]

    def as_dict(self) -> dict:
        return {k: getattr(self, k) for k, _ in self._fields_ if not k.endswith("_")}


def log_verify_blocks(file_buf, *, capacity: Optional[int] = None, stream=None):
    """Every physical record of the log image in `file_buf` (uint8 CUDA
    tensor), walked and verified on the device (lvkv_log_verify_blocks_device).
    Returns (report dict, hdr_offsets int64, actual int32, rec_status uint8 —
    cut to report['nrecords'] — block_status uint8, block_drop int32)."""
    torch = _torch()
    dev = file_buf.device
    size = file_buf.numel()
    nblocks = (size + 32767) // 32768
    cap = capacity if capacity is not None else max(64, size // 256)
    for attempt in range(2):
        hdr = torch.empty(cap, dtype=torch.int64, device=dev)
        actual = torch.empty(cap, dtype=torch.int32, device=dev)
        rst = torch.empty(cap, dtype=torch.uint8, device=dev)
        bst = torch.empty(max(1, nblocks), dtype=torch.uint8, device=dev)
        bdrop = torch.empty(max(1, nblocks), dtype=torch.int32, device=dev)
        rep = torch.zeros(ctypes.sizeof(LogReport), dtype=torch.uint8, device=dev)
        with torch.cuda.device(dev):
            rc = _lib.lvkv_log_verify_blocks_device(
                _dev_ptr(file_buf, "file_buf", (torch.uint8, torch.int8)), size,
                _dev_ptr(hdr, "hdr"), _dev_ptr(actual, "actual"), _dev_ptr(rst, "rec_status"),
                cap, _dev_ptr(bst, "block_status"), _dev_ptr(bdrop, "block_drop"),
                _dev_ptr(rep, "report"), _stream_handle(stream, dev))
        _check("lvkv_log_verify_blocks_device", rc)
        r = LogReport.from_buffer_copy(bytes(rep.cpu().numpy()))
        if r.status == 1 and capacity is None and attempt == 0:
            cap = r.nrecords
            continue
        break
    n = r.nrecords if r.status == 0 else 0
    return r.as_dict(), hdr[:n], actual[:n], rst[:n], bst[:nblocks], bdrop[:nblocks]


class LogReadReport(ctypes.Structure):
    """lvkv_log_read_report (include/lvkv_crc32c.h)."""
    _fields_ = [("status", ctypes.c_int32), ("nrecords", ctypes.c_uint32),
                ("nreports", ctypes.c_uint32), ("stopped", ctypes.c_uint32),
                ("bytes", ctypes.c_uint64)]

    def as_dict(self) -> dict:
        return {k: getattr(self, k) for k, _ in self._fields_}


# Reporter::Corruption reasons (LVKV_LOGR_*) as the reference words them
# (db/log_reader.cc); an unknown type carries its number.
LOG_REASONS = {1: "checksum mismatch", 2: "bad record length",
               3: "partial record without end(1)", 4: "partial record without end(2)",
               5: "missing start of fragmented record(1)",
               6: "missing start of fragmented record(2)", 7: "error in middle of record",
               8: "unknown record type {}"}


def log_read(file_buf, *, initial_offset: int = 0, capacity: Optional[int] = None,
             record_capacity: Optional[int] = None, report_capacity: Optional[int] = None,
             gather: bool = False, stream=None):
    """log::Reader(reporter, checksum=True, initial_offset) over the log image
    in `file_buf` (uint8 CUDA tensor), all on the device
    (lvkv_log_read_device): ReadRecord until it returns false.

    Returns (read report dict, records, reports, physical):
      records  list of (LastRecordOffset, length, first fragment, fragments)
      reports  list of (bytes, reason text) — every Reporter::Corruption call
      physical the log_verify_blocks tuple of the same call
    With gather=True a fifth element: (payload, positions), the records'
    bytes as lvkv_log_gather_device lays them end to end on the device
    (uint8 tensor) and each record's offset in it (int64 tensor).
    Capacities default to sizes that always fit; a LVKV_LOG_CAPACITY result
    from smaller ones is returned as is."""
    import numpy as np
    if initial_offset < 0:
        raise ValueError("initial_offset must be >= 0")
    torch = _torch()
    dev = file_buf.device
    size = file_buf.numel()
    nblocks = (size + 32767) // 32768
    cap = capacity if capacity is not None else max(64, size // 7 + nblocks)
    rcap = record_capacity if record_capacity is not None else cap
    pcap = report_capacity if report_capacity is not None else cap + nblocks
    hdr = torch.empty(cap, dtype=torch.int64, device=dev)
    actual = torch.empty(cap, dtype=torch.int32, device=dev)
    rst = torch.empty(cap, dtype=torch.uint8, device=dev)
    bst = torch.empty(max(1, nblocks), dtype=torch.uint8, device=dev)
    bdrop = torch.empty(max(1, nblocks), dtype=torch.int32, device=dev)
    rep = torch.zeros(ctypes.sizeof(LogReport), dtype=torch.uint8, device=dev)
    recs = torch.zeros(max(1, rcap) * 24, dtype=torch.uint8, device=dev)
    reps = torch.zeros(max(1, pcap) * 16, dtype=torch.uint8, device=dev)
    rd = torch.zeros(ctypes.sizeof(LogReadReport), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        rc = _lib.lvkv_log_read_device(
            _dev_ptr(file_buf, "file_buf", (torch.uint8, torch.int8)), size,
            _dev_ptr(hdr, "hdr"), _dev_ptr(actual, "actual"), _dev_ptr(rst, "rec_status"), cap,
            _dev_ptr(bst, "block_status"), _dev_ptr(bdrop, "block_drop"), _dev_ptr(rep, "report"),
            _dev_ptr(recs, "records"), rcap, _dev_ptr(reps, "reports"), pcap,
            int(initial_offset), _dev_ptr(rd, "read"), _stream_handle(stream, dev))
    _check("lvkv_log_read_device", rc)
    if gather:
        payload = torch.empty(max(1, size), dtype=torch.uint8, device=dev)
        pos = torch.zeros(max(1, rcap), dtype=torch.int64, device=dev)
        with torch.cuda.device(dev):
            rc = _lib.lvkv_log_gather_device(
                _dev_ptr(file_buf, "file_buf", (torch.uint8, torch.int8)), _dev_ptr(hdr, "hdr"),
                cap, _dev_ptr(rep, "report"), _dev_ptr(recs, "records"), rcap,
                _dev_ptr(rd, "read"), _dev_ptr(payload, "payload"), payload.numel(),
                _dev_ptr(pos, "positions"), _stream_handle(stream, dev))
        _check("lvkv_log_gather_device", rc)
    r = LogReport.from_buffer_copy(bytes(rep.cpu().numpy()))
    o = LogReadReport.from_buffer_copy(bytes(rd.cpu().numpy()))
    nrec = min(o.nrecords, rcap)
    nrep = min(o.nreports, pcap)
    rv = recs.cpu().numpy()[: nrec * 24].view(np.uint64).reshape(-1, 3)
    records = [(int(x[0]), int(x[1]), int(x[2]) & 0xFFFFFFFF, int(x[2]) >> 32) for x in rv]
    pv = reps.cpu().numpy()[: nrep * 16].view(np.uint64).reshape(-1, 2)
    reports = []
    for x in pv:
        reason, typ = int(x[1]) & 0xFFFFFFFF, int(x[1]) >> 32
        text = LOG_REASONS.get(reason, "?")
        reports.append((int(x[0]), text.format(typ) if reason == 8 else text))
    n = r.nrecords if r.status == 0 else 0
    physical = (r.as_dict(), hdr[:n], actual[:n], rst[:n], bst[:nblocks], bdrop[:nblocks])
    if gather:
        return o.as_dict(), records, reports, physical, (payload, pos[:nrec])
    return o.as_dict(), records, reports, physical


def crc32c_batch_host(data, offsets, lengths, *, init: int = 0, inits=None,
                      mask: bool = False):
    """Host-resident batch: numpy uint8 buffer + numpy offsets/lengths; the
    library stages through pinned memory to the current device and back.
    Returns a numpy uint32 array."""
    import numpy as np
    data = np.ascontiguousarray(data, dtype=np.uint8)
    offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
    lengths = np.ascontiguousarray(lengths, dtype=np.uint32)
    n = offsets.size
    if lengths.size != n:
        raise ValueError("offsets and lengths differ in length")
    if n and int((offsets + lengths).max()) > data.size:
        raise ValueError("blocks exceed the buffer")
    out = np.empty(n, dtype=np.uint32)
    ip = None
    if inits is not None:
        inits = np.ascontiguousarray(inits, dtype=np.uint32)
        ip = ctypes.c_void_p(inits.ctypes.data)
    rc = _lib.lvkv_crc32c_batch_host(
        ctypes.c_void_p(data.ctypes.data), ctypes.c_void_p(offsets.ctypes.data),
        ctypes.c_void_p(lengths.ctypes.data), ip, init & 0xFFFFFFFF,
        ctypes.c_void_p(out.ctypes.data), n, LVKV_FLAG_MASK if mask else 0)
    _check("lvkv_crc32c_batch_host", rc)
    return out


# --------------------------------------------------------------------------
# the AQL engine (lvkv_engine_*): batches dispatched into hardware queues


class Engine:
    """Per-device batch engine (include/lvkv_crc32c.h, lvkv_engine_*): a
    submit writes AQL dispatch packets into the engine's own hardware queues
    (no HIP launch), consecutive batches overlap on the device, ``wait()``
    fences every queue. Inputs must be complete before a submit (synchronize
    the stream that produced them); results are valid after ``wait()``.

    Same results as ``crc32c_uniform`` / ``crc32c_batch`` / ``sst_verify``
    / ``log_verify`` / the fill calls, for any block layout."""

    def __init__(self, device=None):
        torch = _torch()
        dev = torch.device("cuda", torch.cuda.current_device() if device is None else
                           (device.index if isinstance(device, torch.device) else int(device)))
        h = ctypes.c_void_p()
        _check("lvkv_engine_create", _lib.lvkv_engine_create(dev.index, ctypes.byref(h)))
        self.device = dev
        self.handle = h
        # the raw entry, for callers that pass pointers themselves (bench.py)
        self.submit_ptr = _lib.lvkv_engine_crc32c_uniform
        # inputs and outputs of submitted batches, held until the wait() that
        # covers them: the engine reads and writes them outside any torch
        # stream, so the caching allocator must not hand their memory out
        self._inflight = []

    def crc32c_uniform(self, buf, nblocks: int, length: int, stride: Optional[int] = None, *,
                       init: int = 0, mask: bool = False, ordered: bool = False,
                       fresh: bool = True, final: bool = False, out=None):
        """fresh: the input may have been written by a copy engine or the host
        (LVKV_FLAG_SYSTEM_ACQUIRE); False when a kernel on this device wrote it.
        final: a wait follows (LVKV_FLAG_FINAL)."""
        torch = _torch()
        stride = length if stride is None else stride
        if nblocks and (nblocks - 1) * stride + length > buf.numel():
            raise ValueError("blocks exceed the buffer")
        out = _u32_out(torch, nblocks, buf.device, out)
        flags = self._flags(mask, ordered, fresh, final)
        # the engine does not follow HIP streams: the inputs must be complete
        torch.cuda.current_stream(buf.device).synchronize()
        rc = _lib.lvkv_engine_crc32c_uniform(
            self.handle, _dev_ptr(buf, "buf", (torch.uint8, torch.int8)), stride, length,
            init & 0xFFFFFFFF, _dev_ptr(out, "out", (torch.int32,), nblocks), nblocks, flags)
        _check("lvkv_engine_crc32c_uniform", rc)
        self._inflight.append((buf, out))
        return out

    def _flags(self, mask=False, ordered=False, fresh=True, final=False):
        return ((LVKV_FLAG_MASK if mask else 0) | (LVKV_FLAG_ORDERED if ordered else 0) |
                (LVKV_FLAG_SYSTEM_ACQUIRE if fresh else 0) | (LVKV_FLAG_FINAL if final else 0))

    def crc32c_batch(self, buf, offsets, lengths, *, init: int = 0, inits=None,
                     mask: bool = False, ordered: bool = False, fresh: bool = True,
                     final: bool = False, small: bool = False, out=None):
        """lvkv_engine_crc32c_batch: crc32c_batch's contract on the engine.
        small: the blocks are mostly under ~2 KiB (LVKV_FLAG_SMALL_BLOCKS)."""
        torch = _torch()
        n = offsets.numel()
        if lengths.numel() != n:
            raise ValueError("offsets and lengths differ in length")
        out = _u32_out(torch, n, buf.device, out)
        torch.cuda.current_stream(buf.device).synchronize()
        rc = _lib.lvkv_engine_crc32c_batch(
            self.handle, _dev_ptr(buf, "buf", (torch.uint8, torch.int8)),
            _dev_ptr(offsets, "offsets", (torch.int64,)),
            _dev_ptr(lengths, "lengths", (torch.int32,)),
            _dev_ptr(inits, "inits", (torch.int32,), n) if inits is not None else None,
            init & 0xFFFFFFFF, _dev_ptr(out, "out", (torch.int32,), n), n,
            self._flags(mask, ordered, fresh, final) | (LVKV_FLAG_SMALL_BLOCKS if small else 0))
        _check("lvkv_engine_crc32c_batch", rc)
        self._inflight.append((buf, offsets, lengths, inits, out))
        return out

    def sst_verify(self, file_buf, offsets, sizes, *, ordered=False, fresh=True, final=False):
        """lvkv_engine_sst_verify: (actual int32, status uint8) as sst_verify."""
        torch = _torch()
        n = offsets.numel()
        actual = torch.empty(n, dtype=torch.int32, device=file_buf.device)
        status = torch.empty(n, dtype=torch.uint8, device=file_buf.device)
        torch.cuda.current_stream(file_buf.device).synchronize()
        rc = _lib.lvkv_engine_sst_verify(
            self.handle, _dev_ptr(file_buf, "file_buf", (torch.uint8, torch.int8)),
            _dev_ptr(offsets, "offsets", (torch.int64,)), _dev_ptr(sizes, "sizes", (torch.int32,), n),
            _dev_ptr(actual, "actual"), _dev_ptr(status, "status"), n,
            self._flags(False, ordered, fresh, final))
        _check("lvkv_engine_sst_verify", rc)
        self._inflight.append((file_buf, offsets, sizes, actual, status))
        return actual, status

    def log_verify(self, file_buf, hdr_offsets, *, ordered=False, fresh=True, final=False):
        """lvkv_engine_log_verify: (actual int32, status uint8) as log_verify."""
        torch = _torch()
        n = hdr_offsets.numel()
        actual = torch.empty(n, dtype=torch.int32, device=file_buf.device)
        status = torch.empty(n, dtype=torch.uint8, device=file_buf.device)
        torch.cuda.current_stream(file_buf.device).synchronize()
        rc = _lib.lvkv_engine_log_verify(
            self.handle, _dev_ptr(file_buf, "file_buf", (torch.uint8, torch.int8)),
            _dev_ptr(hdr_offsets, "hdr_offsets", (torch.int64,)), _dev_ptr(actual, "actual"),
            _dev_ptr(status, "status"), n, self._flags(False, ordered, fresh, final))
        _check("lvkv_engine_log_verify", rc)
        self._inflight.append((file_buf, hdr_offsets, actual, status))
        return actual, status

    def sst_fill_trailers(self, file_buf, offsets, sizes, *, ordered=False, fresh=True, final=False):
        """lvkv_engine_sst_fill_trailers: sst_fill_trailers on the engine."""
        torch = _torch()
        n = offsets.numel()
        crc = torch.empty(n, dtype=torch.int32, device=file_buf.device)
        torch.cuda.current_stream(file_buf.device).synchronize()
        rc = _lib.lvkv_engine_sst_fill_trailers(
            self.handle, _dev_ptr(file_buf, "file_buf", (torch.uint8, torch.int8)),
            _dev_ptr(offsets, "offsets", (torch.int64,)), _dev_ptr(sizes, "sizes", (torch.int32,), n),
            _dev_ptr(crc, "crc"), n, self._flags(False, ordered, fresh, final))
        _check("lvkv_engine_sst_fill_trailers", rc)
        self._inflight.append((file_buf, offsets, sizes, crc))
        return crc

    def log_fill_headers(self, file_buf, hdr_offsets, *, ordered=False, fresh=True, final=False):
        """lvkv_engine_log_fill_headers: log_fill_headers on the engine."""
        torch = _torch()
        n = hdr_offsets.numel()
        crc = torch.empty(n, dtype=torch.int32, device=file_buf.device)
        torch.cuda.current_stream(file_buf.device).synchronize()
        rc = _lib.lvkv_engine_log_fill_headers(
            self.handle, _dev_ptr(file_buf, "file_buf", (torch.uint8, torch.int8)),
            _dev_ptr(hdr_offsets, "hdr_offsets", (torch.int64,)), _dev_ptr(crc, "crc"), n,
            self._flags(False, ordered, fresh, final))
        _check("lvkv_engine_log_fill_headers", rc)
        self._inflight.append((file_buf, hdr_offsets, crc))
        return crc

    def wait(self) -> None:
        _check("lvkv_engine_wait", _lib.lvkv_engine_wait(self.handle))
        self._inflight.clear()

    def kernarg_cache(self) -> Tuple[int, int]:
        """(hits, misses) of the engine's kernel-argument cache."""
        h, m = ctypes.c_uint64(), ctypes.c_uint64()
        _check("lvkv_debug_engine_kernarg_cache",
               _lib.lvkv_debug_engine_kernarg_cache(self.handle, ctypes.byref(h), ctypes.byref(m)))
        return int(h.value), int(m.value)

    def queues(self, n: int = 0) -> int:
        r = int(_lib.lvkv_engine_queues(self.handle, n))
        _check("lvkv_engine_queues", r if r < 0 else 0)
        return r

    def shape(self):
        w, c, g = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint32()
        _check("lvkv_engine_shape", _lib.lvkv_engine_shape(self.handle, ctypes.byref(w),
                                                            ctypes.byref(c), ctypes.byref(g)))
        return w.value, c.value, g.value

    def profile(self, enable: bool) -> None:
        _check("lvkv_engine_profile", _lib.lvkv_engine_profile(self.handle, int(enable)))

    def profile_read(self, n: int = 4096):
        """[(start_us, end_us)] of the most recent profiled dispatches, in
        submission order (HSA system clock)."""
        t0, t1 = (ctypes.c_double * n)(), (ctypes.c_double * n)()
        k = int(_lib.lvkv_engine_profile_read(self.handle, t0, t1, n))
        _check("lvkv_engine_profile_read", k if k < 0 else 0)
        return list(zip(t0[:k], t1[:k]))

    def load_probe(self, code_object: Optional[bytes], kernel: str = "", waves: int = 8,
                   chains: int = 5, per_cu: int = 1, overlapped: bool = True) -> None:
        """Measurement only (lvkv_engine_load_probe): overlapped (or ordered)
        uniform submits dispatch `kernel` from a separate gfx950 code object
        instead of the engine's own; None restores them."""
        if code_object is None:
            rc = _lib.lvkv_engine_load_probe(self.handle, None, 0, None, 0, 0, 0, 0)
        else:
            rc = _lib.lvkv_engine_load_probe(self.handle, code_object, len(code_object),
                                             (kernel + ".kd").encode(), waves, chains, per_cu,
                                             int(overlapped))
        _check("lvkv_engine_load_probe", rc)

    def close(self) -> None:
        if self.handle:
            _lib.lvkv_engine_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # interpreter shutdown
            pass
