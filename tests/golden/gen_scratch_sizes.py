"""Generates tests/golden/scratch_sizes.json: what the seven sizing functions
of the write path answer over a grid that crosses every branch of theirs (the
scan passes of 1,024 and tiles of 4,096 items, the bit-setting kernel's keys
in LDS up to 512 bytes, the Zstd compressor's pool from 20,481 bytes a block
and its step down on the way to 128 KiB). Callers size buffers they allocate
once with these values, and the scratch layouts behind them are listed in one
place each: a change of any value is a change of the contract.
tests/test_sst_write_table.py::test_sizing_functions_answer_as_recorded asserts
every row. Needs the built library and no device.

    python tests/golden/gen_scratch_sizes.py
"""
from __future__ import annotations

import json
import sys
from pathlib import Path

HERE = Path(__file__).resolve().parent
REPO = HERE.parent.parent
sys.path.insert(0, str(REPO))
import __graft_entry__ as g  # noqa: E402

COUNTS = [0, 1, 7, 8, 9, 1023, 1024, 1025, 4095, 4096, 4097, 8192, 253952]
KEY_LENS = [0, 1, 24, 512, 513, 600, 1 << 20]  # the last with up to 9 blocks
BITS = [0, 10]
MAX_LENS = [0, 16, 4096, 20480, 20481, 65536, 131072]


def grid():
    """(function, arguments) of every recorded call."""
    for n in COUNTS:
        totals = sorted({0, 4096 * n})
        for max_len in MAX_LENS:
            yield "lvkv_sst_write_scratch_bytes", (n, max_len)
            for total in totals:
                yield "lvkv_sst_write_scratch_bytes_v2", (n, total, max_len)
            # (the finisher's part does not depend on max_len: one key length)
            yield "lvkv_sst_write_table_scratch_bytes", (n, 4096 * n, max_len, 24, 10)
        for mkl in KEY_LENS:
            if mkl == 1 << 20 and n > 9:
                continue
            for bits in BITS:
                yield "lvkv_sst_write_table_scratch_bytes", (n, 0, 4096, mkl, bits)
                yield "lvkv_sst_table_file_bound", (n, 4096 * n, mkl, bits)
        for restart in (1, 16):
            yield "lvkv_sst_build_blocks_scratch_bytes", (n, restart)
            yield "lvkv_sst_build_blocks_raw_bound", (n, 0, 0, restart)
            yield "lvkv_sst_build_blocks_raw_bound", (n, 24 * n, 4096 * n, restart)
    for max_len in MAX_LENS:
        yield "lvkv_zstd_compress_big_scratch_bytes", (max_len,)


def main():
    lib = g.load_package().lib
    calls = {}
    for fn, args in grid():
        rows = calls.setdefault(fn, [])
        row = list(args) + [int(getattr(lib, fn)(*args))]
        if row not in rows:
            rows.append(row)
    blob = {"layout": "per function: rows of its arguments in order, then the value",
            "calls": calls}
    text = json.dumps(blob, separators=(",", ":")).replace('],[', '],\n[')
    (HERE / "scratch_sizes.json").write_text(text + "\n")
    print(sum(len(r) for r in calls.values()), "values recorded")


if __name__ == "__main__":
    main()
