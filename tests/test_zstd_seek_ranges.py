"""Host checks of the several-ranges selection: ranges_select
and the either-layout table check of juicefs_amd/csrc/zstd_seek.h against a
pure-Python restatement written here, on tables of both layouts and of 1 to 130
frames, lists whose ends sit on every frame edge, empty, clamped, negative and
bad lists, and 20,000 seeded random tables with random lists, under
AddressSanitizer + UBSan (tests/zstd_seek_ranges_main.cc, a stand-alone program
whose fetch counts every index outside the object); the third value of the
read calls' seek switch and the new names."""
import os
import random
import shutil
import struct
import subprocess
import sys

import pytest

from juicefs_amd import _lib as L
from juicefs_amd import compress as C
from tests import zstd_seek_csum_cases as X
from tests.zstd_seek_cases import MAX_FRAMES, SEEK_MAGIC, SKIP_MAGIC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CYCLE = [0, 1, 777, 131072]
COUNTS = [1, 2, 63, 64, 65, 130]


# ---- the restatement ---------------------------------------------------------
def parse_any(obj: bytes):
    """(entries, entry size, table position) of a valid table of either layout at the end of obj, else None"""
    n = len(obj)
    if n < 25 or struct.unpack_from("<I", obj, n - 4)[0] != SEEK_MAGIC or obj[n - 5] not in (0, 0x80):
        return None
    e = 12 if obj[n - 5] else 8
    nf = struct.unpack_from("<I", obj, n - 9)[0]
    if nf < 1 or nf > MAX_FRAMES or e * nf + 17 > n:
        return None
    t = n - (e * nf + 17)
    if struct.unpack_from("<II", obj, t) != (SKIP_MAGIC, e * nf + 9):
        return None
    ent = [struct.unpack_from("<III" if e == 12 else "<II", obj, t + 8 + e * k) for k in range(nf)]
    if any(x[0] < 1 for x in ent) or sum(x[0] for x in ent) != t or sum(x[1] for x in ent) >= 1 << 32:
        return None
    return ent, e, t


def rule(obj: bytes, cap: int, ranges):
    """the issue's rule, by brute force: what ranges_select must answer"""
    r = dict(bad=0, live=0, top=0, table=0, checksums=0, nf=0, total=0, sel=[])
    for q, (lo, hi) in enumerate(ranges):
        if hi < lo or (q > 0 and ranges[q - 1][1] > lo):
            r["bad"] = 1
            return r
    live = [(max(lo, 0), min(hi, cap)) for lo, hi in ranges if min(hi, cap) > max(lo, 0)]
    r["live"] = len(live)
    r["top"] = max((h for _, h in live), default=0)
    p = parse_any(obj)
    if p is None:
        return r
    ent, e, _ = p
    r.update(table=1, checksums=int(e == 12), nf=len(ent), total=sum(x[1] for x in ent))
    cpos = dpos = 0
    for k, x in enumerate(ent):
        c, d = x[0], x[1]
        if d > 0 and any(lo < dpos + d and hi > dpos for lo, hi in live):
            r["sel"].append((k, cpos, dpos, c, d, x[2] if e == 12 else 0))
        cpos, dpos = cpos + c, dpos + d
    return r


def entries(nf, wide, start=0, rng=None):
    """nf entries whose content sizes cycle through CYCLE from `start`; compressed sizes of 1 to 3 bytes"""
    out = []
    for k in range(nf):
        d = CYCLE[(start + k) % 4]
        out.append((1 + (k * 5) % 3, d) + (((k * 2654435761 + 12345) & 0xFFFFFFFF,) if wide else ()))
    return out


def obj_of(ent, filler=b"\x28") -> bytes:
    """an object as the selection sees it: as many bytes as the frames take (never read) and the table"""
    return filler * sum(x[0] for x in ent) + X.table(ent)


def edges(ent):
    out, pos = [0], 0
    for x in ent:
        pos += x[1]
        out.append(pos)
    return out


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    out = str(tmp_path_factory.mktemp("zranges") / "zstd_seek_ranges_main")
    r = subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "juicefs_amd", "csrc"),
                        os.path.join(ROOT, "tests", "zstd_seek_ranges_main.cc"), "-o", out], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return out


def run_cases(exe, tmp_path, cases):
    """cases = [(object, dst_cap, [(lo, hi)])] -> [dict as rule()]"""
    path = str(tmp_path / "cases.bin")
    with open(path, "wb") as f:
        for obj, cap, ranges in cases:
            f.write(struct.pack("<IiI", len(obj), cap, len(ranges)) + b"".join(struct.pack("<ii", *r) for r in ranges) + obj)
    r = subprocess.run([exe, "cases", path], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = r.stdout.split("\n")
    assert lines[len(cases)] == "oob=0"
    out = []
    for ln in lines[:len(cases)]:
        w = ln.split()
        bad, live, top, table, x, nf, total, count = map(int, w[:8])
        sel = [tuple(int(v) for v in s.split(":")) for s in w[8:]]
        assert len(sel) == count
        out.append(dict(bad=bad, live=live, top=top, table=table, checksums=x, nf=nf, total=total, sel=sel))
    return out


def check(exe, tmp_path, cases):
    got = run_cases(exe, tmp_path, cases)
    for (obj, cap, ranges), g in zip(cases, got):
        assert g == rule(obj, cap, ranges), (len(obj), cap, ranges[:6], g["sel"][:4])
    return got


def edge_lists(ent):
    """lists whose ends sit on every frame edge"""
    ed = edges(ent)
    total = ed[-1]
    out = []
    for e in sorted(set(ed)):
        out += [[(e - 1, e)], [(e, e + 1)], [(e - 1, e + 1)], [(e, e)], [(0, 1), (e, e + 1)] if e >= 1 else [(0, 1)],
                [(e - 1, e), (total - 1, total)] if e <= total - 1 else [(e - 1, e)],
                [(e - 2, e - 1), (e - 1, e - 1), (e, e + 1), (e + 1, e + 1)]]
    return out


@pytest.mark.parametrize("wide", [False, True])
@pytest.mark.parametrize("nf", COUNTS)
def test_every_frame_edge(exe, tmp_path, nf, wide):
    cases = []
    for start in range(4):
        ent = entries(nf, wide, start)
        obj = obj_of(ent)
        assert parse_any(obj) is not None and parse_any(obj)[1] == (12 if wide else 8)
        total = edges(ent)[-1]
        lists = edge_lists(ent) if (nf <= 65 or start == 0) else edge_lists(ent)[::7]
        cases += [(obj, total + 5, ls) for ls in lists]
        cases += [(obj, total + 5, []), (obj, total + 5, [(0, total)]), (obj, total + 5, [(-7, 1 << 30)])]
    got = check(exe, tmp_path, cases)
    assert all(g["table"] == 1 and g["nf"] == nf and g["bad"] == 0 for g in got)


def test_the_edge_rules_by_hand(exe, tmp_path):
    """sizes 0, 1, 777, 131072, 0, 1, ...: frame k's content starts at D[k]"""
    for wide in (False, True):
        ent = entries(10, wide)
        obj, D = obj_of(ent), edges(ent)
        cap = D[-1]
        assert D[:6] == [0, 0, 1, 778, 131850, 131850]

        def sel(ranges, cap=cap):
            g = check(exe, tmp_path, [(obj, cap, ranges)])[0]
            return [s[0] for s in g["sel"]], g
        assert sel([(0, D[3])])[0] == [1, 2]           # hi == D_3 does not select frame 3; frame 0 has no content
        assert sel([(D[3] - 1, D[3] + 1)])[0] == [2, 3]  # lo == D_3 - 1 selects frame 2
        assert sel([(D[3] - 1, D[3])])[0] == [2]
        assert sel([(D[3], D[3] + 1)])[0] == [3]
        # frames 3 and 5 selected, frame 4 (no content) between them is not; nor is 6, which lies between the ranges
        assert sel([(D[4] - 1, D[4]), (D[5], D[5] + 1)])[0] == [3, 5]
        assert sel([(0, 1), (D[9], D[9] + 1)])[0] == [1, 9]  # first and last frame with content, nothing between
        ks, g = sel([(0, 1), (D[9], D[9] + 1)])
        assert g["top"] == D[9] + 1 and g["live"] == 2 and g["total"] == D[-1]
        assert [s[1:3] for s in g["sel"]] == [(ent[0][0], 0), (sum(x[0] for x in ent[:9]), D[9])]
        # empty ranges anywhere; all empty
        assert sel([(0, 0), (5, 5), (D[3], D[3] + 1), (D[3] + 1, D[3] + 1), (cap, cap)])[0] == [3]
        ks, g = sel([(0, 0), (5, 5), (cap, cap)])
        assert ks == [] and g["live"] == 0 and g["top"] == 0 and g["bad"] == 0
        # clamped by dst_cap (the selection is computed whatever D is; the caller answers -2)
        ks, g = sel([(0, 1), (700, 5000)], cap=779)
        assert ks == [1, 2, 3] and g["top"] == 779
        ks, g = sel([(0, 1), (778, 5000)], cap=778)
        assert ks == [1] and g["top"] == 1 and g["live"] == 1
        # negative ends
        ks, g = sel([(-100, -50), (-5, 1), (2, 3)])
        assert ks == [1, 2] and g["live"] == 2 and g["top"] == 3
        assert sel([(-(1 << 31), -1)])[1]["live"] == 0
        assert sel([(-(1 << 31), (1 << 31) - 1)])[0] == [k for k in range(10) if ent[k][1] > 0]
        # every bad list
        for bad in ([(5, 4)], [(0, 10), (9, 20)], [(10, 20), (0, 5)], [(0, 1), (3, 2)], [(0, 5), (4, 4)],
                    [(3, 3), (2, 2)], [(0, 1), (1, 2), (1, 3), (3, 4)]):
            g = sel(bad)[1]
            assert g["bad"] == 1 and g["sel"] == [] and g["table"] == 0, bad
        assert sel([(0, 1), (1, 2), (2, 2), (2, 3)])[1]["bad"] == 0  # touching is in order


def test_table_check_of_either_layout(exe, tmp_path):
    cases, names = [], []
    for wide in (False, True):
        ent = entries(5, wide, 1)
        obj = obj_of(ent)
        e, nf, n = 12 if wide else 8, 5, len(obj)
        t = n - (e * nf + 17)
        body = obj[:t]
        full = [(0, 1 << 30)]
        for name, off in [("skip magic", t), ("skip magic top", t + 3), ("frame size", t + 4), ("frame size top", t + 7),
                          ("entry c", t + 8 + e * 2), ("entry c top", t + 8 + e * 2 + 3), ("nf", n - 9), ("nf top", n - 6),
                          ("seek magic", n - 4), ("seek magic top", n - 1)]:
            b = bytearray(obj)
            b[off] ^= 0x40
            cases.append((bytes(b), 1 << 30, full))
            names.append(name)
        for desc in range(256):
            if desc not in (0, 0x80):
                cases.append((body + X.table(ent, descriptor=desc), 1 << 30, full))
                names.append(f"descriptor {desc:#x}")
        cases.append((body + X.table(ent, descriptor=0 if wide else 0x80), 1 << 30, full))
        names.append("the other layout's descriptor")
        cases.append((body + X.table(ent, size=(8 if wide else 12) * nf + 9), 1 << 30, full))
        names.append("the other layout's size")
        cases.append((b"\x28" + obj, 1 << 30, full))
        names.append("compressed sum one short")
        cases.append((obj[1:], 1 << 30, full))
        names.append("compressed sum one over")
        z = [(0,) + ent[0][1:], (ent[0][0] + ent[1][0],) + ent[1][1:]] + ent[2:]
        cases.append((body + X.table(z), 1 << 30, full))
        names.append("a frame of no bytes")
        big = [(x[0], 0xFFFFFFFF) + x[2:] if k == 0 else x for k, x in enumerate(ent)]
        cases.append((body + X.table(big), 1 << 30, full))
        names.append("content sum 2^32 or more")
        for nf2 in (0, nf - 1, nf + 1, 0x20000000):
            cases.append((body + X.table(ent, nf=nf2), 1 << 30, full))
            names.append(f"nf {nf2}")
        cases.append((obj[-16:], 1 << 30, full))
        names.append("too short")
        cases.append((X.table(ent)[-(e + 17):], 1 << 30, full))
        names.append("a table alone with a wrong count")
    got = check(exe, tmp_path, cases)
    assert [nm for nm, g in zip(names, got) if g["table"]] == []
    assert all(g["live"] == 1 and g["top"] == 1 << 30 and g["bad"] == 0 for g in got)
    # a lying content size or checksum is still a table; 16,384 frames are one, one more is not; D may reach 2^32 - 1
    ok = []
    for wide in (False, True):
        e1 = (1, 0, 0) if wide else (1, 0)
        for nf, want in ((MAX_FRAMES, 1), (MAX_FRAMES + 1, 0)):
            many = obj_of([e1] * (nf - 1) + [(1, 7) + e1[2:]])
            g = check(exe, tmp_path, [(many, 100, [(0, 100)])])[0]
            assert g["table"] == want and (not want or [s[0] for s in g["sel"]] == [nf - 1])
        ent = entries(5, wide, 1)
        top = [(x[0], 0xFFFFFFFF - (sum(y[1] for y in ent) - x[1])) + x[2:] if k == 0 else x for k, x in enumerate(ent)]
        ok.append((obj_of(top), (1 << 31) - 1, [(0, 1), ((1 << 31) - 2, (1 << 31) - 1)]))
    got = check(exe, tmp_path, ok)
    assert all(g["table"] == 1 and g["total"] == 0xFFFFFFFF for g in got)


def test_random_tables_and_lists(exe, tmp_path):
    rnd = random.Random(20260112)
    cases = []
    for i in range(20000):
        wide = rnd.random() < 0.5
        nf = rnd.choice([1, 2, 3, 5, 8, 13, 63, 64, 65, 70]) if rnd.random() < 0.3 else rnd.randrange(1, 24)
        ent = [(rnd.randrange(1, 4), rnd.choice([0, 0, 1, 2, 7, 100, 777, 4096, 131072])) +
               ((rnd.getrandbits(32),) if wide else ()) for _ in range(nf)]
        obj = obj_of(ent)
        total = sum(x[1] for x in ent)
        if rnd.random() < 0.15:  # a damaged table: one bit of its bytes, or of the frames' last byte
            b = bytearray(obj)
            off = rnd.randrange(max(0, len(obj) - (len(ent[0]) * 4 * nf + 18)), len(obj))
            b[off] ^= 1 << rnd.randrange(8)
            obj = bytes(b)
        cap = rnd.choice([total, total + 9, max(total - 1, 0), rnd.randrange(0, total + 2), 1 << 30])
        ed = edges(ent)
        pts = sorted(rnd.choice(ed) + rnd.choice([-1, 0, 0, 1]) if rnd.random() < 0.7 else rnd.randrange(-5, total + 10)
                     for _ in range(2 * rnd.randrange(0, 7)))
        ranges = [(pts[q], pts[q + 1]) for q in range(0, len(pts), 2)]
        if ranges and rnd.random() < 0.1:  # a bad list
            q = rnd.randrange(len(ranges))
            lo, hi = ranges[q]
            ranges[q] = rnd.choice([(hi + 1, lo), (lo - rnd.randrange(1, 1000), hi) if q > 0 else (hi + 1, lo)])
        cases.append((obj, cap, ranges))
    got = check(exe, tmp_path, cases)
    tables, bad, picked, holes = (sum(1 for g in got if g[k]) for k in ("table", "bad", "sel", "live"))
    assert tables > 15000 and 500 < bad < 3000 and picked > 8000 and holes > 10000
    # lists that leave frames out between two selected ones are common in the draw
    gaps = sum(1 for g in got if len(g["sel"]) >= 2 and g["sel"][-1][0] - g["sel"][0][0] + 1 > len(g["sel"]))
    assert gaps > 1000


# ---- the switch and the names ------------------------------------------------
def test_switch(lib):
    assert lib.jfs_read_seek_mode() == L.READ_SEEK_OFF and C.read_seek_mode() == "off"
    try:
        for bad in (3, -1, 0x80):
            assert lib.jfs_set_read_seek_mode_ext(bad) == -1
        assert lib.jfs_read_seek_mode() == L.READ_SEEK_OFF
        assert lib.jfs_set_read_seek_mode_ext(2) == 0 and lib.jfs_read_seek_mode() == 2 == L.READ_SEEK_SPARSE
        assert C.read_seek_mode() == "sparse"
        assert lib.jfs_set_read_seek_mode(2) == -1 and lib.jfs_read_seek_mode() == 2  # the old setter: unknown, nothing changes
        assert lib.jfs_set_read_seek_mode_ext(1) == 2 and lib.jfs_set_read_seek_mode_ext(0) == 1
        assert lib.jfs_set_read_seek_mode(1) == 0 and lib.jfs_set_read_seek_mode_ext(0) == 1
        assert C.set_read_seek_mode("sparse") == "off" and C.set_read_seek_mode("on") == "sparse"
        assert C.set_read_seek_mode("off") == "on"
        for name in ("ON", "Sparse", "2", ""):
            with pytest.raises(ValueError):
                C.set_read_seek_mode(name)
        assert C.read_seek_mode() == "off"
    finally:
        lib.jfs_set_read_seek_mode_ext(L.READ_SEEK_OFF)


def test_environment_and_no_device():
    code = ("from juicefs_amd import _lib as L; lib = L.load();"
            "print(lib.jfs_read_seek_mode(), lib.jfs_zstd_decompress_ranges_device(None, None, None, 1, None, None))")

    def child(env):
        e = dict(os.environ, JFS_GPU_CODEC="off", **env)
        r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=ROOT, env=e, timeout=120)
        assert r.returncode == 0, r.stderr[-2000:]
        return [int(x) for x in r.stdout.split()]
    nd = L.JFS_ERR_NO_DEVICE
    assert child({"JFS_READ_SEEK": "sparse"}) == [2, nd]
    assert child({"JFS_READ_SEEK": "SPARSE"}) == [2, nd]
    assert child({"JFS_READ_SEEK": "On"})[0] == 1
    assert child({"JFS_READ_SEEK": "2"})[0] == 0
    assert child({})[0] == 0


def test_new_symbols_are_declared_and_exported(lib):
    header = open(os.path.join(ROOT, "include", "jfs_gpucodec.h")).read()
    for name in ("jfs_zstd_decompress_ranges_device", "jfs_zstd_sparse_counts", "jfs_set_read_seek_mode_ext"):
        assert name in L.EXPORTS and hasattr(lib, name) and name + "(" in header, name
    for text in ("#define JFS_READ_SEEK_SPARSE 2", "#define JFS_READ_SEEK_ON 1",
                 "typedef struct jfs_range { int32_t lo, hi; } jfs_range;"):
        assert text in header, text
    from juicefs_amd import device as D
    assert callable(D.zstd_decompress_ranges) and callable(D.zstd_sparse_counts)
