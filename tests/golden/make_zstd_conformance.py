#!/usr/bin/env python3
"""Generate tests/golden/zstd_conformance.json: libzstd's verdict on every
hand-assembled frame of tests/zstd_conformance_cases.py.

Run in the build container (not on the GPU box):
    python tests/golden/make_zstd_conformance.py

Source of truth: libzstd 1.4.9 (/opt/conda/lib/libzstd.so.1), ZSTD_decompress,
as in make_golden.py.  Per case the fixture holds the sha256 of the frame and,
per dst cap, the result (size, or the category -1/-2/-3 of make_golden.zstd_err),
libzstd's error name and the sha256 of the output.  Frame bytes are not
stored: the tests rebuild them from the descriptions and check the sha first.
"""
from __future__ import annotations

import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, HERE)
from make_golden import ZS, sha, zstd_decompress_cat  # noqa: E402
from tests import zstd_conformance_cases as K  # noqa: E402
from tests import zstd_frames as Z  # noqa: E402


def main():
    rows = []
    for c in K.CASES:
        src = Z.write(c["desc"])
        caps = {}
        for cap in K.caps(c):
            r, err, o = zstd_decompress_cat(src, cap)
            caps[str(cap)] = [r, err, sha(o) if r >= 0 else None]
        rows.append(json.dumps({"name": c["name"], "frame_sha": sha(src), "caps": caps}, separators=(",", ":")))
    path = os.path.join(HERE, "zstd_conformance.json")
    with open(path, "w") as f:  # one case per line
        f.write('{"version":%d,"cases":[\n%s\n]}\n' % (ZS.ZSTD_versionNumber(), ",\n".join(rows)))
    print(path, os.path.getsize(path), len(rows))


if __name__ == "__main__":
    main()
