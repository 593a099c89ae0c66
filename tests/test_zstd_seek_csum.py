"""Host checks of checksummed seek tables and ranged-GET planning (DESIGN.md
12f): the stand-alone table parser of juicefs_amd/csrc/zstd_seek.h, both
layouts, against a pure-Python parser (tests/zstd_seek_csum_cases.py) on
hand-built tables, every damaged field and every other descriptor value;
prefixes, suffixes, random strings and planted tables with one bit flipped under
AddressSanitizer + UBSan (tests/zstd_seek_csum_main.cc, a stand-alone program
whose fetch counts every index outside the table); jfs_zstd_seek_plan through
ctypes, which needs no device; the size bound of the 12-byte layout; the new
switch."""
import os
import shutil
import struct
import subprocess
import sys

import pytest

from juicefs_amd import _lib as L
from juicefs_amd import compress as C
from tests import zstd_seek_cases as S
from tests import zstd_seek_csum_cases as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [300, 1, 255, 256, 70000, 5]
CONTENTS = [bytes((i * 7 + k) & 255 for i in range(n)) for k, n in enumerate(SIZES)]
TOTAL = sum(SIZES)
EDGES = [sum(SIZES[:k]) for k in range(len(SIZES) + 1)]
RANGES = sorted({(lo, hi) for e in EDGES for lo in (e - 1, e, e + 1) for hi in (lo, lo + 1, lo + 2, e + 1, TOTAL, TOTAL + 9)}
                | {(0, TOTAL), (-5, 3), (-5, -1), (TOTAL, TOTAL + 5), (TOTAL - 1, 1 << 40), (556, 557),
                   (-(1 << 40), 1 << 40), (300, 557)})


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    out = str(tmp_path_factory.mktemp("zseekx") / "zstd_seek_csum_main")
    r = subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "juicefs_amd", "csrc"),
                        os.path.join(ROOT, "tests", "zstd_seek_csum_main.cc"), "-o", out], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return out


def run_cases(exe, tmp_path, cases):
    """cases = [(table, object_len, cap (-1: D), lo, hi)] -> [None | dict]"""
    path = str(tmp_path / "cases.bin")
    with open(path, "wb") as f:
        for t, olen, cap, lo, hi in cases:
            f.write(struct.pack("<Iqqqq", len(t), olen, cap, lo, hi) + t)
    r = subprocess.run([exe, "cases", path], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = r.stdout.split("\n")
    assert lines[len(cases)] == "oob=0"
    out = []
    for ln in lines[:len(cases)]:
        t, x, nf, total, first, count, coff, cend, doff, dend = map(int, ln.split())
        out.append(dict(checksums=x, nf=nf, content=total, first=first, count=count, get_off=coff, get_len=cend - coff,
                        first_off=doff, flo=doff, fhi=dend) if t else None)
    return out


@pytest.mark.parametrize("checksums", [False, True])
def test_selections_at_every_frame_edge(exe, tmp_path, checksums):
    obj, t, ent = X.build(CONTENTS, checksums)
    assert X.parse(t, len(obj)) == (ent, checksums)
    cases = [(t, len(obj), cap, lo, hi) for lo, hi in RANGES for cap in (-1, TOTAL + 100, 400)]
    got = run_cases(exe, tmp_path, cases)
    for (_, olen, cap, lo, hi), g in zip(cases, got):
        w = X.plan(t, olen, lo, hi, None if cap < 0 else cap)
        assert g is not None and {k: g[k] for k in g} == {k: w[k] for k in g}, (cap, lo, hi, g, w)
    w = X.plan(t, len(obj), 300, 557)
    assert (w["first"], w["count"], w["first_off"], w["fhi"], w["get_off"]) == (1, 3, 300, 812, ent[0][0])
    if not checksums:  # the 8-byte layout selects what the in-object parser selects
        for lo, hi in RANGES:
            if -(1 << 31) <= lo and hi < 1 << 31:
                a, b = S.select(obj, TOTAL, lo, hi), X.plan(t, len(obj), lo, hi)
                assert (a["first"], a["count"], a["coff"], a["doff"]) == (b["first"], b["count"], b["get_off"], b["first_off"])


def variants(checksums):
    obj, t, ent = X.build(CONTENTS, checksums)
    e, nf, olen = 12 if checksums else 8, len(ent), len(obj)
    out = []
    for name, off in [("skip magic", 0), ("skip magic top", 3), ("frame size", 4), ("frame size top", 7),
                      ("entry c", 8 + e * 2), ("entry c top", 8 + e * 2 + 3), ("nf", len(t) - 9), ("nf top", len(t) - 6),
                      ("seek magic", len(t) - 4), ("seek magic top", len(t) - 1)]:
        b = bytearray(t)
        b[off] ^= 0x40
        out.append((name, bytes(b), olen))
    for desc in range(256):  # every other descriptor value, under either entry size
        if desc not in (0, 0x80):
            out.append((f"descriptor {desc:#x}", X.table(ent, descriptor=desc), olen))
    out.append(("the other layout's descriptor", X.table(ent, descriptor=0 if checksums else 0x80), olen))
    for k, dc in ((0, 1), (0, -1), (nf - 1, 1), (nf - 1, -1)):
        e2 = list(ent)
        e2[k] = (e2[k][0] + dc,) + e2[k][1:]
        out.append((f"compressed sum {dc:+d} at {k}", X.table(e2), olen))
    out.append(("object one longer", t, olen + 1))
    out.append(("object one shorter", t, olen - 1))
    out.append(("object shorter than the table", t, len(t) - 1))
    out.append(("object beyond int32", t, 1 << 31))
    out.append(("a frame of no bytes", X.table([(0,) + ent[0][1:], (ent[0][0] + ent[1][0],) + ent[1][1:]] + ent[2:]), olen))
    out.append(("content sum 2^32", X.table([(x[0], 0xFFFFFFFF) + x[2:] if k == 0 else x for k, x in enumerate(ent)]), olen))
    out.append(("nf one more", X.table(ent, nf=nf + 1), olen))
    out.append(("nf one less", X.table(ent, nf=nf - 1), olen))
    out.append(("nf zero", X.table(ent, nf=0), olen))
    out.append(("nf huge", X.table(ent, nf=0x20000000), olen))
    out.append(("size field of the other layout", X.table(ent, size=(8 if checksums else 12) * nf + 9), olen))
    out.append(("too short", t[-16:], olen))
    out.append(("no entry", X.table([]), 17))
    out.append(("a byte in front", b"\0" + t, olen + 1))
    return out, (t, olen, ent)


@pytest.mark.parametrize("checksums", [False, True])
def test_damaged_tables_are_no_table(exe, tmp_path, checksums):
    vs, (t, olen, ent) = variants(checksums)
    for name, b, n in vs:
        assert X.parse(b, n) is None, name
    got = run_cases(exe, tmp_path, [(b, n, -1, 0, 1 << 20) for _, b, n in vs] + [(t, olen, -1, 0, 1 << 20)])
    assert [v[0] for v, g in zip(vs, got) if g is not None] == []
    assert got[-1] is not None and got[-1]["count"] == len(SIZES) and got[-1]["checksums"] == int(checksums)
    # a damaged decompressed size or checksum is still a table: the decode of that frame is what notices
    for off in (8 + (12 if checksums else 8) * 2 + 5,) + ((8 + 12 * 2 + 9,) if checksums else ()):
        lie = bytearray(t)
        lie[off] ^= 0x40
        assert run_cases(exe, tmp_path, [(bytes(lie), olen, -1, 0, 10)])[0] is not None
    # 16,384 frames are a table, one more is not; the content sum may reach 2^32 - 1
    e1 = (1, 0, 0) if checksums else (1, 0)
    for nf, ok in ((S.MAX_FRAMES, True), (S.MAX_FRAMES + 1, False)):
        many = X.table([e1] * (nf - 1) + [(1, 7) + e1[2:]])
        g = run_cases(exe, tmp_path, [(many, len(many) + nf, -1, 0, 100)])[0]
        assert (X.parse(many, len(many) + nf) is not None) == ok and (g is not None) == ok
        assert not ok or (g["content"], g["first"], g["count"], g["get_off"], g["get_len"]) == (7, nf - 1, 1, nf - 1, 1)
    top = X.table([(x[0], 0xFFFFFFFF - (TOTAL - x[1])) + x[2:] if k == 0 else x for k, x in enumerate(ent)])
    g = run_cases(exe, tmp_path, [(top, olen, -1, 0, 10)])[0]
    assert g is not None and g["content"] == 0xFFFFFFFF


@pytest.mark.parametrize("checksums", [False, True])
def test_fuzz_stays_inside_the_table(exe, tmp_path, checksums):
    _, t, _ = X.build(CONTENTS[:3] + [b"x" * 40] * 70, checksums)  # more than 64 entries
    path = str(tmp_path / "table.bin")
    open(path, "wb").write(t)
    r = subprocess.run([exe, "fuzz", path, "20000"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    f = dict(kv.split("=") for kv in r.stdout.split())
    assert int(f["oob"]) == 0 and int(f["bad"]) == 0
    assert int(f["cuts"]) == 2 * (len(t) + 1) and int(f["random"]) == 20000
    assert 5000 < int(f["accepted"]) < 20000  # the whole table and the planted ones whose flip does no harm, nothing random


def c_plan(lib, tail, olen, lo, hi):
    p = L.JfsSeekPlan()
    rc = lib.jfs_zstd_seek_plan(tail, len(tail), olen, lo, hi, p)
    assert rc == 0
    return p


@pytest.mark.parametrize("checksums", [False, True])
def test_planner(lib, checksums):
    obj, t, ent = X.build(CONTENTS, checksums)
    olen, tl = len(obj), len(t)
    fields = ("checksums", "nf", "first", "count", "table_off", "table_len", "get_off", "get_len", "content", "first_off")
    for tail_len in (0, 8, 9, tl - 1, tl, tl + 1, olen):
        tail = obj[olen - tail_len:]
        for lo, hi in RANGES:
            p = c_plan(lib, tail, olen, lo, hi)
            if tail_len < 9:
                assert p.status == L.SEEK_PLAN_NONE
            elif tail_len < tl:
                assert (p.status, p.table_off, p.table_len, p.nf, p.checksums) == (L.SEEK_PLAN_MORE, olen - tl, tl, len(ent),
                                                                                   int(checksums))
                assert (p.get_off, p.get_len, p.count) == (0, 0, 0)
            else:
                w = X.plan(t, olen, lo, hi)
                assert p.status == L.SEEK_PLAN_OK and {k: getattr(p, k) for k in fields} == {k: w[k] for k in fields}, (lo, hi)
                if w["count"]:
                    assert obj[p.get_off:p.get_off + p.get_len] == b"".join(
                        S.raw_frame(c) for c in CONTENTS[p.first:p.first + p.count])
    # no frame, one frame, all frames
    assert C.seek_plan(obj[-tl:], olen, TOTAL, TOTAL + 5)["count"] == 0
    assert C.seek_plan(obj[-tl:], olen, -9, 0)["get_len"] == 0
    d = C.seek_plan(obj[-tl:], olen, 300, 301)
    assert (d["status"], d["first"], d["count"], d["get_off"], d["get_len"]) == ("ok", 1, 1, ent[0][0], ent[1][0])
    d = C.seek_plan(obj[-tl:], olen, -(1 << 40), 1 << 40)
    assert (d["first"], d["count"], d["get_off"], d["get_len"], d["content"]) == (0, len(ent), 0, olen - tl, TOTAL)
    assert C.seek_plan(obj[-64:], olen, 0, 1)["status"] == "more"
    # NONE: a footer that is not one, and every table that fails a check
    for name, b, n in variants(checksums)[0]:
        if n <= 0x7FFFFFFF and len(b) <= n:
            p = c_plan(lib, b, n, 0, 1 << 20)
            # (a footer whose damaged count places a longer table asks for those bytes first)
            assert p.status == L.SEEK_PLAN_NONE or (p.status == L.SEEK_PLAN_MORE and len(b) < p.table_len <= n), name
    assert c_plan(lib, obj[:olen - tl], olen - tl, 0, 10).status == L.SEEK_PLAN_NONE  # frames without a table
    # JFS_ERR_INVALID
    p = L.JfsSeekPlan()
    assert lib.jfs_zstd_seek_plan(t, tl, olen, 0, 1, None) == L.JFS_ERR_INVALID
    assert lib.jfs_zstd_seek_plan(None, tl, olen, 0, 1, p) == L.JFS_ERR_INVALID
    assert lib.jfs_zstd_seek_plan(t, -1, olen, 0, 1, p) == L.JFS_ERR_INVALID
    assert lib.jfs_zstd_seek_plan(t, tl, -1, 0, 1, p) == L.JFS_ERR_INVALID
    assert lib.jfs_zstd_seek_plan(t, tl, tl - 1, 0, 1, p) == L.JFS_ERR_INVALID
    assert lib.jfs_zstd_seek_plan(t, tl, 1 << 31, 0, 1, p) == L.JFS_ERR_INVALID
    assert lib.jfs_zstd_seek_plan(None, 0, olen, 0, 1, p) == 0 and p.status == L.SEEK_PLAN_NONE
    with pytest.raises(ValueError):
        C.seek_plan(t, tl - 1, 0, 1)


def test_layout_stays_within_compress_bound(lib):
    """worst case, every block raw: n + 25 nb + 17 (header 9 + block header 3 + entry 12 <= 25 per frame, with the one
    extra byte per frame the 8-byte layout's 21 already carries)"""
    B = S.FRAME
    ns = set()
    for k in range(1, 129):
        ns.update((k * B - 1, k * B, k * B + 1))
    ns.add((16 << 20) + 1)
    ns = sorted(n for n in ns if n > B)
    assert ns[0] == B + 1 and ns[-1] == (16 << 20) + 1
    for n in ns:
        nb = -(-n // B)
        assert n + 25 * nb + 17 <= lib.jfs_compress_bound(L.ALGO_ZSTD, n), n
    obj, t, ent = X.build([bytes(B), bytes(1)], True)
    assert len(obj) == (B + 1) + (9 + 3 + 12) + (6 + 3 + 12) + 17


def test_switch(lib):
    assert lib.jfs_zstd_seek_csum_mode() == L.ZSTD_SEEK_CSUM_OFF and C.zstd_seek_csum_mode() == "off"
    try:
        for bad in (2, -1, 0x80):
            assert lib.jfs_set_zstd_seek_csum_mode(bad) == -1
        assert lib.jfs_zstd_seek_csum_mode() == L.ZSTD_SEEK_CSUM_OFF
        assert lib.jfs_set_zstd_seek_csum_mode(L.ZSTD_SEEK_CSUM_ON) == L.ZSTD_SEEK_CSUM_OFF
        assert lib.jfs_zstd_seek_csum_mode() == L.ZSTD_SEEK_CSUM_ON and C.zstd_seek_csum_mode() == "on"
        assert C.set_zstd_seek_csum_mode("off") == "on" and C.set_zstd_seek_csum_mode("on") == "off"
        with pytest.raises(ValueError):
            C.set_zstd_seek_csum_mode("ON")
        assert lib.jfs_zstd_parse_mode() == L.ZSTD_PARSE_EXACT  # the parse mode is its own switch
        assert lib.jfs_set_zstd_parse_mode_ext(3) == -1
    finally:
        lib.jfs_set_zstd_seek_csum_mode(L.ZSTD_SEEK_CSUM_OFF)


def test_environment_and_no_device():
    code = ("from juicefs_amd import _lib as L; lib = L.load();"
            "print(lib.jfs_zstd_seek_csum_mode(), lib.jfs_zstd_parse_mode(),"
            " lib.jfs_xxh64_device(None, 1, None, None, None),"
            " lib.jfs_zstd_compress_seekable_csum_device(None, 1, None, None),"
            " lib.jfs_zstd_decompress_frames_device(None, None, None, 1, None, None))")

    def child(env):
        e = dict(os.environ, JFS_GPU_CODEC="off", **env)
        r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=ROOT, env=e, timeout=120)
        assert r.returncode == 0, r.stderr[-2000:]
        return [int(x) for x in r.stdout.split()]
    nd = L.JFS_ERR_NO_DEVICE
    assert child({"JFS_ZSTD_SEEK_CSUM": "On"}) == [1, 0, nd, nd, nd]
    assert child({"JFS_ZSTD_SEEK_CSUM": "on", "JFS_ZSTD_PARSE": "seekable"})[:2] == [1, 2]
    assert child({"JFS_ZSTD_SEEK_CSUM": "1"})[0] == 0
    assert child({})[0] == 0


def test_new_symbols_are_declared_and_exported(lib):
    header = open(os.path.join(ROOT, "include", "jfs_gpucodec.h")).read()
    for name in ("jfs_xxh64_device", "jfs_zstd_compress_seekable_csum_device", "jfs_zstd_seek_csum_mode",
                 "jfs_set_zstd_seek_csum_mode", "jfs_zstd_seek_plan", "jfs_zstd_decompress_frames_device",
                 "jfs_zstd_load_range_batch"):
        assert name in L.EXPORTS and hasattr(lib, name) and name + "(" in header, name
    for text in ("#define JFS_ZSTD_SEEK_CSUM_ON 1", "#define JFS_SEEK_PLAN_MORE 1", "#define JFS_SEEK_PLAN_NONE 2",
                 "typedef struct jfs_seek_plan", "typedef struct jfs_seek_frag", "typedef struct jfs_range_read"):
        assert text in header, text
