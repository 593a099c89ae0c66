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
import zlib

import numpy as np
import pytest

from juicefs_amd import _lib as L
from juicefs_amd import compress as C
from juicefs_amd.blockgen import gen_block
from tests import lz4_chase_cases as K
from tests import lz4_fast_cases as F
from tests import lz4_lift_cases as LC
from tests.lz4_lift_cases import directed, fill  # noqa: F401  (the streams, shared with the device's tests)
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


def test_new_streams_are_what_their_names_say():
    by = {name: (s, K.sequences(s), LC.token_starts(s)) for name, s, *_ in directed()}
    assert all(len(s) < 4 * CH for s, _, _ in by.values())
    _, seqs, _ = by["longest-match"]
    assert seqs[0] == (CH + 1, seqs[0][1], 65535, 1) and len(K.seq(b"", 65535, 1)) == 1 + 2 + 257
    _, seqs, _ = by["longest-literal-run"]
    assert seqs[0][0] + seqs[0][2] == CH and seqs[1][0] == 65532 and seqs[1][2] == 4 and seqs[1][3] <= 65532
    _, seqs, _ = by["literals-begin-below-F"]
    assert seqs[0][0] + seqs[0][2] == CH - 200 and seqs[1][0] == 300
    # the tokens of the sequences whose matches lie in chunk 1 start in 257 segments: rounds 0 to 3 take 256
    _, seqs, starts = by["records-in-the-fifth-round"]
    segs = [pos // LC.SEG for (pos, op), (ll, _, ml, _) in zip(starts, seqs) if ml and CH <= op + ll < 2 * CH]
    assert len(segs) == CH // 64 and segs[-1] - segs[0] == 256
    # the chunk's first token: at 253 mod 256, three literal-length bytes on both sides of the edge, and 238
    # match-length bytes across another
    s, seqs, starts = by["token-spans-a-segment-edge"]
    (pos, op), (ll, lit, ml, off) = starts[1], seqs[1]
    assert op == CH and pos % LC.SEG == 253 and lit - pos == 4 and ll == 530 and off <= ll
    mlb = lit + ll + 2
    assert starts[2][0] - mlb == 238 and mlb // LC.SEG != (starts[2][0] - 1) // LC.SEG


def emit_rec(out, lift, streams, caps):
    b = struct.pack("<III", 4, len(out), len(streams))
    for s, cap in zip(streams, caps):
        b += struct.pack("<ii", len(s), cap) + s
    return b + out + b"".join(struct.pack("<ii", *c) for c in lift)


def emit_rows(lines):
    return [(int(n), int(size), int(crc), int(lifted), int(valid), [int(x) for x in nrec.split(",")])
            for n, size, crc, lifted, valid, nrec in re.findall(
                r"^emit \d+ n (\d+) size (\d+) crc (\d+) lifted (\d+) valid (\d+) nrec (\S+)$", "\n".join(lines), re.M)]


def real_encoder_blocks():
    return [LC.unshared_block(40 + i) for i in range(4)]


def zero_record_blocks():
    """(outs, lift, stored streams): the overwrite in the last whole chunk, and in chunk 0"""
    raws = [LC.zero_record_block(50), LC.zero_record_block(60)]
    outs, lift = LC.overwritten(raws, [3 * CH + 1000, 1000])
    return outs, lift, [C.lz4_fast_host(r) for r in raws]


def test_real_encoder_leaves_chunks_liftable(built, oracle):
    """the condition tests/test_lz4_lift_foreign_gpu.py rests on: of a block whose chunks share no content, liblz4's
    parse (which the exact encoder restates byte for byte) leaves three of the four interior chunks liftable at least"""
    raws = real_encoder_blocks()
    streams = [oracle.lz4_compress(r)[1] for r in raws]
    rows = lift_rows(run_driver(built, b"".join(lift_rec(s, c) for s in streams for c in range(4))))
    assert len(rows) == 16 and all(r["total"] == LC.N and r["valid"] == r["ok"] for r in rows)
    per = [sum(r["ok"] for r in rows[4 * k:4 * k + 4]) for k in range(4)]
    assert min(per) >= 3, per
    # and its records are none the fast parse would leave: the hook's block differs from the fast encoder's
    got, lifted, _ = C.lz4_fast_lift_host(raws[0], [(0, j) for j in range(4)] + [(-1, 0)], streams[:1], [LC.N])
    assert lifted == per[0] and got != C.lz4_fast_host(raws[0])


def test_hook_equals_the_driver(built, oracle):
    """jfs_test_lz4_fast_lift_host as the library exports it against the sanitizer-built driver's copy of the same
    source: size, CRC-32 of the bytes, lifted count and per-chunk record counts, over every hand-made stream, the
    real encoder's blocks and the zero-record blocks; the driver also decodes each block back to its content"""
    jobs = []  # (name, out, lift, streams, caps, expected lifted count or None)
    for name, s, c, ok, _ in directed():
        total = sum(ll + ml for ll, _, ml, _ in K.sequences(s))
        out = oracle.lz4_decompress(s, total)[1]
        assert len(out) == total, name
        jobs.append((name, out, LC.candidates(c, total), [s], [total], ok))
    raws = real_encoder_blocks()
    streams = [oracle.lz4_compress(r)[1] for r in raws]
    outs, lift = LC.overwritten(raws)
    assert [sum(s >= 0 for s, _ in l) for l in lift] == LC.PLANNED
    jobs += [(f"liblz4-{k}", o, l, streams, [LC.N] * 4, None) for k, (o, l) in enumerate(zip(outs, lift))]
    outs, lift, streams = zero_record_blocks()
    jobs += [(f"zero-record-{k}", o, l, streams, [LC.N] * 2, 3) for k, (o, l) in enumerate(zip(outs, lift))]
    rows = emit_rows(run_driver(built, b"".join(emit_rec(o, l, s, c) for _, o, l, s, c, _ in jobs)))
    assert len(rows) == len(jobs)
    for (name, out, lift, streams, caps, want), (n, size, crc, lifted, valid, nrec) in zip(jobs, rows):
        got, glifted, gnrec = C.lz4_fast_lift_host(out, lift, streams, caps)
        assert (n, valid) == (len(out), 1), name
        assert (len(got), zlib.crc32(got), glifted, gnrec) == (size, crc, lifted, nrec), name
        assert want is None or lifted == want, (name, lifted)
        assert lifted == sum(r >= 0 for r in nrec), name
        if lifted == 0:
            assert got == C.lz4_fast_host(out), name
    # the zero-record blocks: two of the three lifted chunks hold no record
    for (name, *_), row in zip(jobs[-2:], rows[-2:]):
        assert sum(r == 0 for r in row[5]) == 2, (name, row[5])


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
    # the launch-group size and the host twin's lift form are test hooks in the fast encoder's test header, outside
    # the public ABI
    hooks = ["jfs_test_set_lz4_fast_group_chunks", "jfs_test_lz4_fast_lift_host"]
    assert L.LZ4_LIFT_TEST_EXPORTS == hooks
    test_header = open(os.path.join(inc, "jfs_gpucodec_lz4_fast_test.h")).read()
    for hook in hooks:
        assert hasattr(lib, hook) and hook not in L.EXPORTS
        assert hook + "(" in test_header and hook not in header
    assert "typedef struct jfs_lz4_lift {" in header
