"""Host check of the LZ4 lift (juicefs_amd/csrc/lz4_lift.h: the interior test,
the host plan, the per-sequence rule and its serial restatement) and of its
switch's row in juicefs_amd/csrc/host_modes.h.  tests/lz4_lift_main.cc, built
with AddressSanitizer and UBSan, runs the header and the fast encoder's host twin
(juicefs_amd/csrc/lz4_fast_host.cc).  Nothing is loaded into Python under a
sanitizer.

The claim the feature rests on comes first: the fast parse is deterministic in a
chunk's content, so records lifted from the stored stream of block A, with the
other chunks parsed, give the bytes the encoder gives for B, an overwrite of A."""
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

from juicefs_amd import _lib as L
from juicefs_amd import compress as C
from juicefs_amd.blockgen import gen_block
from tests import lz4_chase_cases as K
from tests import lz4_fast_cases as F
from tests.test_modes import H, _check_setter, _children, _mixed

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CH = F.CHUNK
MAX_REC = CH // 4


def _rand(seed, n):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


def interior(c, n):
    return (c + 1) * CH + 12 <= n


def run_driver(tmp, blob):
    """blob: the records -> the driver's lines"""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    exe, data = str(tmp / "lz4_lift"), str(tmp / "cases.bin")
    if not os.path.exists(exe):
        r = subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "juicefs_amd", "csrc"),
                            os.path.join(ROOT, "tests", "lz4_lift_main.cc"), "-o", exe], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
    with open(data, "wb") as f:
        f.write(blob)
    r = subprocess.run([exe, data], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    return r.stdout.strip().splitlines()


def lift_rec(stream, chunk):
    return struct.pack("<IIi", 1, len(stream), chunk) + stream


def lift_rows(lines):
    keys = ("case", "total", "ok", "nrec", "tail", "lit0", "body", "pos", "mlen", "off", "lit", "valid")
    return [dict(zip(keys, map(int, m))) for m in re.findall(
        r"^lift (\d+) total (\d+) ok (\d+) nrec (\d+) tail (\d+) lit0 (\d+) body (\d+) first (\d+):(\d+):(\d+):(\d+) valid (\d+)$",
        "\n".join(lines), re.M)]


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    return tmp_path_factory.mktemp("lz4_lift")


def test_lifted_records_give_the_reparse_bytes(built):
    """every fast-parse input of two chunks or more, 4 KiB overwritten inside one chunk: the other interior chunks'
    records come from A's stream, the rest is parsed, and the block is B's own encoding"""
    blob, expect = b"", []
    for name, a in F.cases():
        n = len(a)
        if n <= CH:
            continue
        start = CH + 1000 if n >= 2 * CH else (CH if n - CH >= 4096 else 1000)
        b = a[:start] + _rand(n, 4096) + a[start + 4096:]
        assert len(b) == n and start // CH == (start + 4095) // CH
        blob += struct.pack("<II", 2, n) + a + b
        # (a chunk the overwrite left as it was counts too: random bytes over random bytes never do that)
        same = [c for c in range(n // CH) if interior(c, n) and a[c * CH:(c + 1) * CH] == b[c * CH:(c + 1) * CH]]
        assert start // CH not in same
        expect.append((name, n, len(same)))
    assert len(expect) >= 20 and any(k >= 2 for _, _, k in expect) and any(nm.startswith("T-") for nm, _, _ in expect)
    lines = run_driver(built, blob)
    rows = re.findall(r"^det \d+ n (\d+) chunks (\d+) lifted (\d+) refused (\d+) same (\d+)$", "\n".join(lines), re.M)
    assert len(rows) == len(expect)
    for (name, n, k), row in zip(expect, rows):
        assert tuple(map(int, row)) == (n, (n + CH - 1) // CH, k, 0, 1), (name, row)


def plan_rec(caps, outs):
    """outs: [(total, [(src, src_off, dst_off, len)])]"""
    b = struct.pack("<III", 3, len(outs), len(caps)) + struct.pack(f"<{len(caps)}i", *caps)
    for total, segs in outs:
        b += struct.pack("<iI", total, len(segs))
        for s in segs:
            b += struct.pack("<4i", *s)
    return b


def test_host_plan_directed(built):
    caps = [300000, 300000, 2 * CH + 11]
    t = 2 * CH + 100
    cases = [
        ("exact-cover", [(t, [(0, 0, 0, CH), (1, 5, CH, CH + 100)])], "0:0:0:0", "0", "1"),
        ("shifted-by-one", [(t, [(0, 1, 0, t)])], "-", "-", "0"),
        # by the stated rule: chunk 0 lies in two segments that continue each other; chunk 1 in the second alone
        ("two-segments-continue", [(t, [(0, 0, 0, 30000), (0, 30000, 30000, t - 30000)])], "0:1:0:1", "0", "1"),
        ("hole", [(t, [(-1, 0, 0, CH), (0, CH, CH, CH + 100)])], "0:1:0:1", "0", "1"),
        ("eleven-bytes-follow", [(2 * CH + 11, [(0, 0, 0, 2 * CH + 11)])], "0:0:0:0", "0", "1"),
        ("twelve-bytes-follow", [(2 * CH + 12, [(0, 0, 0, 2 * CH + 12)])], "0:0:0:0,0:1:0:1", "0", "2"),
        ("moved-chunk", [(t, [(1, 2 * CH, 0, CH), (1, 0, CH, CH + 100)])], "0:0:1:2,0:1:1:0", "1", "2"),
        ("source-chunk-not-interior-in-its-capacity", [(t, [(2, CH, 0, CH), (2, 0, CH, CH + 100)])], "0:1:2:0", "2", "1"),
        ("source-out-of-range", [(t, [(7, 0, 0, t)])], "-", "-", "0"),
        ("segment-ends-inside-the-chunk", [(t, [(0, 0, 0, CH - 1), (1, 0, CH - 1, t - CH + 1)])], "-", "-", "0"),
        ("two-outputs-flat-order", [(t, [(0, 0, 0, CH), (1, 5, CH, CH + 100)]), (t, [(1, 2 * CH, 0, CH), (1, 0, CH, CH + 100)])],
         "0:0:0:0,1:0:1:2,1:1:1:0", "0,1", "1,2"),
        ("empty-output", [(0, []), (2 * CH + 12, [(0, CH, 0, 2 * CH + 12)])], "1:0:0:1,1:1:0:2", "0", "0,2"),
    ]
    lines = run_driver(built, b"".join(plan_rec(caps, outs) for _, outs, *_ in cases))
    rows = re.findall(r"^plan \d+ cand (\S+) srcs (\S+) per_out (\S+)$", "\n".join(lines), re.M)
    assert len(rows) == len(cases)
    for (name, _, cand, srcs, per), row in zip(cases, rows):
        assert row == (cand, srcs, per), (name, row)


def fill(seed, upto, at, ml=30, off=9):
    """one sequence from output position `at` whose match ends exactly at `upto`"""
    return K.seq(_rand(seed, upto - at - ml), ml, off)


def directed():
    """[(name, stream, chunk, ok, expected fields or None)]"""
    out = []
    tail = K.last(_rand(99, 100))
    ends = K.seq(_rand(1, CH - 20), 20, 100) + K.seq(_rand(2, CH - 50), 50, 30) + tail
    out.append(("match-ends-on-E", ends, 1, 1, dict(nrec=1, tail=0, lit0=CH - 50, pos=CH - 50, mlen=50, off=30, lit=CH - 50)))
    out.append(("match-ends-on-E-chunk-0", ends, 0, 1, dict(nrec=1, tail=0, lit0=CH - 20, pos=CH - 20, mlen=20, off=100)))
    cross = K.seq(_rand(3, CH - 6), 20, 10) + fill(4, 2 * CH, CH + 14) + tail
    out.append(("match-straddles-F", cross, 1, 0, None))
    out.append(("match-straddles-E", cross, 0, 0, None))
    on = K.seq(_rand(5, CH), 300, 1) + fill(6, 2 * CH, CH + 300) + tail
    out.append(("overlap-off1-on-F", on, 1, 0, None))
    behind = K.seq(_rand(7, CH + 1), 300, 1) + fill(8, 2 * CH, CH + 301) + tail
    out.append(("overlap-off1-behind-one-literal", behind, 1, 1, dict(nrec=2, tail=0, lit0=1, pos=1, mlen=300, off=1, lit=1)))
    lits = K.seq(_rand(9, 65000), 8, 50) + K.seq(_rand(10, 1000), 10, 20) + fill(11, 2 * CH, 66018) + tail
    out.append(("literals-across-F", lits, 1, 1, dict(nrec=2, tail=0, lit0=472, pos=472, mlen=10, off=20, lit=472)))
    none = K.seq(_rand(12, 100), 8, 50) + K.seq(_rand(13, 2 * CH + 500), 12, 9) + tail
    out.append(("no-match", none, 1, 1, dict(nrec=0, tail=CH, lit0=0, body=0)))
    far = K.seq(_rand(14, CH + 100), 16, 300) + fill(15, 2 * CH, CH + 116) + tail
    out.append(("offset-reaches-below-F", far, 1, 0, None))
    # kMaxRec four-byte matches tile a chunk only with the first on F, which copies from below it: refused by the
    # offset rule (the count rule cannot be met with more, matches being four bytes at least); behind four literals
    # the chunk holds kMaxRec - 1 of them and is lifted
    head = K.seq(_rand(16, CH - 8), 8, 20)
    out.append(("kMaxRec-matches", head + K.seq(b"", 4, 4) * MAX_REC + tail, 1, 0, None))
    out.append(("kMaxRec-less-one", head + K.seq(_rand(17, 4), 4, 4) + K.seq(b"", 4, 4) * (MAX_REC - 2) + tail, 1, 1,
                dict(nrec=MAX_REC - 1, tail=0, lit0=4, pos=4, mlen=4, off=4, lit=4)))
    # the source's true length: the chunk must be interior in it
    short = K.seq(_rand(18, CH - 20), 20, 100) + K.last(_rand(19, 11))
    out.append(("eleven-bytes-follow", short, 0, 0, None))
    out.append(("twelve-bytes-follow", K.seq(_rand(18, CH - 20), 20, 100) + K.last(_rand(19, 12)), 0, 1, dict(nrec=1, tail=0)))
    out.append(("chunk-past-the-end", ends, 2, 0, None))
    out.append(("negative-chunk", ends, -1, 0, None))
    return out


def test_rule_on_hand_made_streams(built):
    cases = directed()
    rows = lift_rows(run_driver(built, b"".join(lift_rec(s, c) for _, s, c, _, _ in cases)))
    assert len(rows) == len(cases)
    for (name, s, c, ok, want), row in zip(cases, rows):
        assert c < 0 or row["total"] == sum(ll + ml for ll, _, ml, _ in K.sequences(s)), name
        assert row["ok"] == ok, (name, row)
        # a lifted chunk's records describe the bytes the interpreter decodes, and the counts are parse_kernel's sums
        assert row["valid"] == ok, (name, row)
        for k, v in (want or {}).items():
            assert row[k] == v, (name, k, row)
    # the streams are what their names say
    by = {name: K.sequences(s) for name, s, *_ in cases}
    ll, _, ml, _ = by["match-straddles-F"][0]
    assert ll < CH < ll + ml
    ll, _, ml, off = by["overlap-off1-on-F"][0]
    assert ll == CH and off == 1
    (l0, _, m0, _), (l1, _, _, _) = by["literals-across-F"][:2]
    assert l0 + m0 < CH < l0 + m0 + l1
    assert len(by["kMaxRec-matches"]) == MAX_REC + 2


def test_exact_encoder_block_has_a_refused_chunk(built, oracle):
    """liblz4's parse matches across chunk boundaries: the rule refuses such chunks, and what it does lift is valid"""
    src = gen_block("T", 21, 300000)
    exact = oracle.lz4_compress(src)[1]
    fast = C.lz4_fast_host(src)
    rows = lift_rows(run_driver(built, b"".join(lift_rec(exact, c) for c in range(4)) + b"".join(lift_rec(fast, c) for c in range(5))))
    assert len(rows) == 9 and all(r["total"] == len(src) for r in rows)
    assert any(r["ok"] == 0 for r in rows[:4]), rows[:4]
    assert all(r["valid"] == r["ok"] for r in rows)
    # the fast encoder's own block: every interior chunk lifts, the ragged one does not
    assert [r["ok"] for r in rows[4:]] == [1, 1, 1, 1, 0], rows[4:]


def test_mode_row_parses(built):
    last = run_driver(built, lift_rec(K.last(b"twelve bytes"), 0))[-1]
    assert last == "cases=1 modes_bad=0", last


def test_switch_environment_setter_and_default():
    """JFS_COMPACT_LZ4_LIFT as tests/test_modes.py checks the other switches: spellings in any case, no prefix match,
    no trimming; the setter answers the previous value, or -1 and no change"""
    var, getter, setter = "JFS_COMPACT_LZ4_LIFT", "jfs_compact_lz4_lift_mode", "jfs_set_compact_lz4_lift_mode"
    words = {"off": H["JFS_COMPACT_LZ4_LIFT_OFF"], "on": H["JFS_COMPACT_LZ4_LIFT_ON"]}
    assert list(words.values()) == [0, 1]
    expect = {None: 0, "bogus": 0, "1": 0, "": 0, "all": 0}
    for w, val in words.items():
        expect[w] = expect[w.upper()] = expect[_mixed(w)] = val
        expect[w + "x"] = expect[" " + w] = 0
    tries = [-1, 0, 1, 2, 3, 1, 0, 7, 2**31 - 1, -2**31]
    got = _children(var, getter, expect, [[setter, tries]])
    assert {v: g["get"] for v, g in got.items()} == expect
    _check_setter(got[None]["sets"], setter, [0, 1])
    rows = [r for r in got[None]["sets"] if r[1] == 2]
    assert rows and all((ans, after) == (-1, before) for _, _, before, ans, after in rows)
    assert C.compact_lz4_lift_mode() in ("off", "on")
    with pytest.raises(ValueError):
        C.set_compact_lz4_lift_mode("all")


def test_new_symbols_exported(lib):
    inc = os.path.join(ROOT, "include")
    header = open(os.path.join(inc, "jfs_gpucodec.h")).read()
    for name in ("jfs_lz4_compress_fast_lift_device", "jfs_compact_lz4_lift_mode", "jfs_set_compact_lz4_lift_mode",
                 "jfs_compact_lz4_lift_counts"):
        assert name in L.EXPORTS and hasattr(lib, name) and name + "(" in header, name
    # the launch-group size is a test hook in the fast encoder's test header, outside the public ABI
    hook = "jfs_test_set_lz4_fast_group_chunks"
    assert L.LZ4_LIFT_TEST_EXPORTS == [hook] and hasattr(lib, hook) and hook not in L.EXPORTS
    assert hook + "(" in open(os.path.join(inc, "jfs_gpucodec_lz4_fast_test.h")).read() and hook not in header
    assert "typedef struct jfs_lz4_lift {" in header
