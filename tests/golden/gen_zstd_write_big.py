"""Generates tests/golden/zstd_write_big.json from libzstd 1.4.9
(/opt/conda/lib) driven the way port::Zstd_Compress drives it
(oracle/zstd_encoder.lib_port_compress; tests/golden/gen_zstd_write.py has the
call sequence): for each edge block of tests/zstd_big_inputs.py -- blocks of
20,481 to 131,072 bytes at every place where a 16-bit field of the <= 20 KiB
compressor would overflow, and the small blocks that ride along -- at levels
1, 2, -1 and -5, the input's length and sha256 and the library frame's length
and sha256. The inputs are not committed: the test rebuilds them from the
same seeds.

    python tests/golden/gen_zstd_write_big.py
"""
from __future__ import annotations

import hashlib
import json
import sys
from pathlib import Path

HERE = Path(__file__).resolve().parent
REPO = HERE.parent.parent
sys.path.insert(0, str(REPO))
sys.path.insert(0, str(REPO / "tests"))
from oracle import zstd_encoder as ze  # noqa: E402
import zstd_big_inputs as zb  # noqa: E402


def main():
    lib = ze.system_zstd_writer()
    if lib is None:
        raise SystemExit("libzstd 1.4.9 not found")
    rows = []
    for name, x in zb.edge_blocks():
        for lvl in zb.LEVELS:
            f = ze.lib_port_compress(lib, x, lvl)
            rows.append({"name": name, "level": lvl, "input_len": len(x),
                         "input_sha256": hashlib.sha256(x).hexdigest(), "frame_len": len(f),
                         "frame_sha256": hashlib.sha256(f).hexdigest()})
    blob = {"frames": rows,
            "source": "libzstd 1.4.9 (/opt/conda/lib/libzstd.so.1.4.9): ZSTD_createCCtx, "
                      "ZSTD_getCParams(level, max(n,1), 0), seven ZSTD_CCtx_setParameter "
                      "(= ZSTD_CCtx_setCParams), ZSTD_compress2"}
    (HERE / "zstd_write_big.json").write_text(json.dumps(blob, indent=0))
    print(len(rows), "frames pinned")


if __name__ == "__main__":
    main()
