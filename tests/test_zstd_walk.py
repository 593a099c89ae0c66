"""The Zstd decoder's shared frame / block walk and its stop rule
(juicefs_amd/csrc/zstd_walk.h) on a CPU.  tests/zstd_walk_check.cc is a
stand-alone program built against the header with AddressSanitizer + UBSan (a
plain build where the toolchain has no sanitizers) and run here on frames from
tests/zstd_frames.py and the golden frames:

  - frames of raw and RLE blocks, where the walk's lower bound is exact: the
    walk stops after ceil(want / bsize) blocks, for want = 0, 1, bsize - 1,
    bsize, bsize + 1, total, total + 1 (and a negative want, and want above the
    capacity);
  - a frame whose last block ends exactly at want is not stopped and runs its
    frame end;
  - two frames back to back and a skippable frame in front;
  - want = INT32_MAX gives the scratch totals jfs_zstd_plan_host gave before
    the rule existed (tests/golden/zstd_plan_totals.json, recorded from it)."""
import json
import os
import struct
import subprocess
import warnings

from tests import zstd_frames as Z

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
INT32_MAX = 2**31 - 1


def _case(src, cap, want, blocks=-1, stopped=-1, fends=-1, totals=None):
    t = totals or (0, 0, 0, 0)
    return struct.pack("<Iiiiii I 4I", len(src), cap, want, blocks, stopped, fends, 1 if totals else 0, *t) + src


def _stop_cases():
    """Raw / RLE frames: (source, cap, want, blocks walked, stopped, frame ends)."""
    out = []
    bsize, nb = 1000, 5
    total = bsize * nb
    data = bytes((i * 7 + 3) & 0xFF for i in range(total))
    raws = [Z.raw(data[i * bsize:(i + 1) * bsize]) for i in range(nb)]
    rles = [Z.rle(0x41 + i, bsize) for i in range(nb)]
    mixed = [raws[0], rles[1], raws[2], rles[3], raws[4]]
    for blocks in (raws, rles, mixed):
        for kw in (dict(), dict(checksum="ok"), dict(fcs_size=4)):
            src = Z.write([Z.frame(blocks, **kw)])
            for want in (0, 1, bsize - 1, bsize, bsize + 1, 2 * bsize, total - 1, total, total + 1, -5, INT32_MAX):
                w = max(0, min(want, total))  # cap = total
                k = -(-w // bsize)
                if k >= nb:  # the last block was walked: the frame ends with its checks, the rule never fires
                    out.append(_case(src, total, want, nb, 0, 1))
                else:
                    out.append(_case(src, total, want, k, 1, 0))
            # want above a capacity smaller than the content acts as the capacity
            out.append(_case(src, 2 * bsize, total, 2, 1, 0))
    # two frames back to back, a skippable frame in front
    fa = Z.frame(raws[:2], fcs_size=4)
    fb = Z.frame(rles[2:4], checksum="ok")
    src = Z.write([Z.skip(b"skipme"), fa, fb])
    for want, k, stopped, fends in ((0, 0, 1, 0), (1, 1, 1, 0),
                                     # frame 1 ended with its checks; the rule fires in front of frame 2's first block
                                     (bsize + 1, 2, 1, 1), (2 * bsize, 2, 1, 1),
                                     (2 * bsize + 1, 3, 1, 1), (3 * bsize, 3, 1, 1), (3 * bsize + 1, 4, 0, 2),
                                     (4 * bsize, 4, 0, 2), (4 * bsize + 1, 4, 0, 2)):
        out.append(_case(src, 4 * bsize, want, k, stopped, fends))
    # an empty frame (one empty raw block): nothing to stop in front of but the block itself
    src = Z.write([Z.frame([Z.raw(b"")])])
    out.append(_case(src, 0, 0, 0, 1, 0))
    out.append(_case(src, 16, 1, 1, 0, 1))
    # a truncated source: the walk reports its error however small want is past the first block
    src = Z.write([Z.frame(raws)])[:-10]
    out.append(_case(src, total, bsize, 1, 1, 0))
    out.append(_case(src, total, total, -1, 0, 0))
    return out


def _golden_cases():
    g = json.load(open(os.path.join(GOLD, "zstd_golden.json")))
    blob = open(os.path.join(GOLD, g["bin"]), "rb").read()
    rec = json.load(open(os.path.join(GOLD, "zstd_plan_totals.json")))["totals"]
    out = []
    for r in rec:
        f = g["frames"][r["frame"]]
        src = blob[f["off"]:f["off"] + f["csize"]]
        tot = (r["n_items"], r["lit_bytes"], r["n_cblk"], r["n_blk"])
        # the stop itself at a few wants (the walk's own consistency checks), the recorded totals at INT32_MAX
        for want in (INT32_MAX, 4096, f["size"] // 2):
            out.append(_case(src, r["cap"], want, totals=tot))
    return out


def test_zstd_walk_stop_rule_and_totals(tmp_path):
    cases = _stop_cases() + _golden_cases()
    dump = tmp_path / "cases.bin"
    dump.write_bytes(struct.pack("<I", len(cases)) + b"".join(cases))
    src = os.path.join(ROOT, "tests", "zstd_walk_check.cc")
    exe = str(tmp_path / "zstd_walk_check")
    base = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", src, "-o", exe]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]
    r = subprocess.run(base + san, capture_output=True, text=True)
    sanitized = r.returncode == 0
    if not sanitized:  # no sanitizer runtime: the checks still run, and the run says so
        warnings.warn("zstd_walk_check built WITHOUT ASan/UBSan: " + r.stderr[-300:])
        r = subprocess.run(base, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    print("zstd_walk_check build:", "ASan+UBSan" if sanitized else "plain")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, str(dump)], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0 and "zstd walk check OK" in r.stdout, (r.stdout[-3000:], r.stderr[-3000:])
    print(r.stdout.strip())
