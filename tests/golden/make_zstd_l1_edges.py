"""Generate tests/golden/zstd_l1_edges.json: libzstd 1.4.9 ZSTD_compress(level 1)
frames (sha256 + size) of the directed inputs in tests/zstd_l1_edges.py, and
the format features tests/zstd_frame_census.py reads from each frame (counted
only when the census decodes the frame back to the input).

libzstd 1.4.9 is /opt/conda/lib/libzstd.so.1, as for make_zstd_l1_golden.py.
Data only: names, sizes, hashes and feature names.
Run from the repo root: python tests/golden/make_zstd_l1_edges.py
"""
from __future__ import annotations

import ctypes
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests.zstd_frame_census import FEATURES, census  # noqa: E402
from tests.zstd_l1_edges import CASES, UNREACHABLE, make  # noqa: E402

ZS = ctypes.CDLL("/opt/conda/lib/libzstd.so.1")
ZS.ZSTD_compress.restype = ctypes.c_size_t
ZS.ZSTD_compress.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
ZS.ZSTD_compressBound.restype = ctypes.c_size_t
ZS.ZSTD_compressBound.argtypes = [ctypes.c_size_t]
ZS.ZSTD_isError.restype = ctypes.c_uint
ZS.ZSTD_isError.argtypes = [ctypes.c_size_t]


def main():
    out = {"version": ZS.ZSTD_versionNumber(), "level": 1, "cases": []}
    seen = set()
    for name in CASES:
        src = make(name)
        cap = ZS.ZSTD_compressBound(len(src))
        dst = ctypes.create_string_buffer(cap)
        c = ZS.ZSTD_compress(dst, cap, src, len(src), 1)
        assert not ZS.ZSTD_isError(c)
        back, feats = census(dst.raw[:c])
        assert back == src, name
        seen |= feats
        out["cases"].append({"name": name, "size": len(src), "csize": c,
                             "src_sha": hashlib.sha256(src).hexdigest(),
                             "comp_sha": hashlib.sha256(dst.raw[:c]).hexdigest(),
                             "features": sorted(feats)})
    assert seen == set(FEATURES) - set(UNREACHABLE), sorted(set(FEATURES) - set(UNREACHABLE) - seen)
    with open(os.path.join(HERE, "zstd_l1_edges.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
