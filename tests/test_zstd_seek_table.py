"""Host checks of the seekable Zstd layout: the seek-table
parser of juicefs_amd/csrc/zstd_seek.h, which the range decoder's scan kernel
shares, against a pure-Python parser on hand-built objects; every way a table
can be wrong; every prefix and 20,000 random and 20,000 nearly valid byte
strings under AddressSanitizer + UBSan (tests/zstd_seek_main.cc, a stand-alone
program whose fetch counts every index outside the buffer); the hand-built
object through two CPU decoders; the size bound of the layout; the new
switches without a device; chain_from on plans with holes, unused and repeated
sources."""
import ctypes
import os
import shutil
import struct
import subprocess

import pytest

from juicefs_amd import _lib as L
from juicefs_amd import compress as C
from juicefs_amd import device as D
from tests import zstd_seek_cases as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [300, 1, 255, 256, 70000, 5]  # frame contents: every FCS width, a one-byte frame
CONTENTS = [bytes((i * 7 + k) & 255 for i in range(n)) for k, n in enumerate(SIZES)]
TOTAL = sum(SIZES)


@pytest.fixture(scope="module")
def seek_exe(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("zseek") / "zstd_seek_main")
    r = subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "juicefs_amd", "csrc"),
                        os.path.join(ROOT, "tests", "zstd_seek_main.cc"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def run_cases(exe, tmp_path, cases):
    """cases = [(object, cap, lo, hi)] -> [None | dict] as tests.zstd_seek_cases.select answers"""
    path = str(tmp_path / "cases.bin")
    with open(path, "wb") as f:
        for obj, cap, lo, hi in cases:
            f.write(struct.pack("<Iiii", len(obj), cap, lo, hi) + obj)
    r = subprocess.run([exe, "cases", path], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = r.stdout.split("\n")
    assert lines[len(cases)] == "oob=0"
    out = []
    for ln in lines[:len(cases)]:
        t, nf, total, first, count, coff, doff = map(int, ln.split())
        out.append(dict(nf=nf, total=total, first=first, count=count, coff=coff, doff=doff) if t else None)
    return out


def test_selections_at_every_frame_edge(seek_exe, tmp_path):
    obj, ent = S.build(CONTENTS)
    assert S.parse_table(obj) == ent
    edges = [0]
    for n in SIZES:
        edges.append(edges[-1] + n)
    ranges = []
    for e in edges:
        for lo in (e - 1, e, e + 1):
            for hi in (lo, lo + 1, lo + 2, e + 1, TOTAL, TOTAL + 9):
                ranges.append((lo, hi))
    ranges += [(0, TOTAL), (-5, 3), (-5, -1), (TOTAL, TOTAL + 5), (TOTAL - 1, 1 << 30), (556, 557), (-(1 << 31), (1 << 31) - 1)]
    cases = [(obj, cap, lo, hi) for lo, hi in ranges for cap in (TOTAL, TOTAL + 100)]
    cases += [(obj, TOTAL - 1, 0, 10), (obj, 0, 0, 10), (obj, 400, 0, 1000)]  # D > dst_cap: the table still parses
    got = run_cases(seek_exe, tmp_path, cases)
    for (o, cap, lo, hi), g in zip(cases, got):
        w = S.select(o, cap, lo, hi)
        assert g is not None and g["nf"] == len(SIZES) and g["total"] == TOTAL, (cap, lo, hi)
        assert {k: g[k] for k in ("count",)} == {"count": w["count"]}, (cap, lo, hi, g, w)
        if w["count"]:
            assert (g["first"], g["coff"], g["doff"]) == (w["first"], w["coff"], w["doff"]), (cap, lo, hi, g, w)
    # what the selection means, on one range: frames 1..3 for bytes [300, 557)
    w = S.select(obj, TOTAL, 300, 557)
    assert (w["first"], w["count"], w["doff"], w["flo"], w["fhi"]) == (1, 3, 300, 300, 812)
    assert w["coff"] == ent[0][0]


def variants():
    obj, ent = S.build(CONTENTS)
    body = obj[:sum(c for c, _ in ent)]
    nf = len(ent)
    t = len(body)
    out = []
    # one byte of every field and both magics
    for name, off in [("skip magic", t), ("skip magic top", t + 3), ("frame size", t + 4), ("frame size top", t + 7),
                      ("entry c", t + 8 + 8 * 2), ("entry c top", t + 8 + 8 * 2 + 3), ("nf", len(obj) - 9),
                      ("nf top", len(obj) - 6), ("seek magic", len(obj) - 4), ("seek magic top", len(obj) - 1)]:
        b = bytearray(obj)
        b[off] ^= 0x40
        out.append((name, bytes(b)))
    for bit in range(8):  # the checksum bit and every reserved / unused bit of the descriptor
        out.append((f"descriptor bit {bit}", body + S.table(ent, descriptor=1 << bit)))
    e = list(ent)
    for k, dc in ((0, 1), (0, -1), (nf - 1, 1), (nf - 1, -1)):
        e2 = list(e)
        e2[k] = (e2[k][0] + dc, e2[k][1])
        out.append((f"compressed sum {dc:+d} at {k}", body + S.table(e2)))
    out.append(("a frame of no bytes", body + S.table([(0, 3)] + [(ent[0][0] + ent[1][0], 1)] + e[2:])))
    out.append(("content sum 2^32", body + S.table([(c, 0xFFFFFFFF if k == 0 else d) for k, (c, d) in enumerate(e)])))
    out.append(("nf one more", body + S.table(ent, nf=nf + 1)))
    out.append(("nf one less", body + S.table(ent, nf=nf - 1)))
    out.append(("nf zero", body + S.table(ent, nf=0)))
    out.append(("nf huge", body + S.table(ent, nf=0x20000000)))
    out.append(("entries with checksums", body + S.table(ent, descriptor=0x80)))
    out.append(("too short", S.table([])[:16]))
    out.append(("table only, no entry", S.table([])))
    out.append(("plain frames, no table", body))
    return out, obj


def test_damaged_tables_are_no_table(seek_exe, tmp_path):
    vs, obj = variants()
    for name, b in vs:
        assert S.parse_table(b) is None, name
    got = run_cases(seek_exe, tmp_path, [(b, 1 << 20, 0, 1 << 20) for _, b in vs] + [(obj, 1 << 20, 0, 1 << 20)])
    assert [n for (n, _), g in zip(vs, got) if g is not None] == []
    assert got[-1] is not None and got[-1]["count"] == len(SIZES)
    # A damaged decompressed size is still a table -- nothing in the table contradicts it until the
    # sum passes 2^32 ("content sum 2^32" above); the decode of that frame is what notices
    lie = bytearray(obj)
    lie[len(obj) - len(S.table(S.parse_table(obj))) + 8 + 8 * 2 + 5] ^= 0x40
    g = run_cases(seek_exe, tmp_path, [(bytes(lie), 1 << 30, 0, 1 << 30)])[0]
    assert g is not None and g["total"] == TOTAL + 0x4000
    # 16,384 frames, the most the encoder writes, are a table; one more is not (the range decoder
    # walks the selected entries, and the table is stored data)
    for nf, ok in ((S.MAX_FRAMES, True), (S.MAX_FRAMES + 1, False)):
        many = bytes(nf) + S.table([(1, 0)] * (nf - 1) + [(1, 7)])
        assert (S.parse_table(many) is not None) == ok
        g = run_cases(seek_exe, tmp_path, [(many, 100, 0, 100)])[0]
        assert (g is not None) == ok and (not ok or (g["total"], g["first"], g["count"]) == (7, nf - 1, 1))
    # the content sum may reach 2^32 - 1
    top = obj[:len(obj) - len(S.table(S.parse_table(obj)))] + S.table(
        [(c, 0xFFFFFFFF - (TOTAL - d) if k == 0 else d) for k, (c, d) in enumerate(S.parse_table(obj))])
    g = run_cases(seek_exe, tmp_path, [(top, (1 << 31) - 1, 0, 10)])[0]
    assert g is not None and g["total"] == 0xFFFFFFFF


def test_prefixes_and_random_strings_stay_in_bounds(seek_exe, tmp_path):
    obj, _ = S.build(CONTENTS[:3] + [b"x" * 40] * 70)  # more than 64 entries
    path = str(tmp_path / "obj.bin")
    open(path, "wb").write(obj)
    r = subprocess.run([seek_exe, "fuzz", path, "20000"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    f = dict(kv.split("=") for kv in r.stdout.split())
    assert int(f["oob"]) == 0 and int(f["bad"]) == 0
    assert int(f["prefixes"]) == len(obj) + 1 and int(f["random"]) == 20000
    assert 5000 < int(f["accepted"]) < 20000  # the whole object and the undamaged planted tables, nothing random


def test_chain_from_and_layout(seek_exe):
    r = subprocess.run([seek_exe, "plan", "-"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "plan bad=0" in r.stdout, r.stdout + r.stderr[-4000:]


def test_hand_built_object_is_an_ordinary_zstd_object(oracle):
    """passes without the feature: concatenated frames and a skippable frame"""
    obj, _ = S.build(CONTENTS)
    whole = b"".join(CONTENTS)
    n, out = oracle.zstd_decompress(obj, TOTAL)
    assert n == TOTAL and out == whole
    z = D._libzstd()
    if z is not None:
        z.ZSTD_decompress.restype = ctypes.c_size_t
        z.ZSTD_decompress.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t]
        buf = ctypes.create_string_buffer(TOTAL)
        m = z.ZSTD_decompress(buf, TOTAL, obj, len(obj))
        assert not z.ZSTD_isError(m) and buf.raw[:m] == whole


def test_layout_stays_within_compress_bound(lib):
    """worst case, every block raw: n + 21 nb + 17 (header 9 + block header 3 + entry 8 <= 21 per frame)"""
    B = S.FRAME
    ns = set()
    for k in range(1, 129):
        ns.update((k * B - 1, k * B, k * B + 1))
    ns.add((16 << 20) + 1)
    ns = sorted(n for n in ns if n > B)
    assert ns[0] == B + 1 and ns[-1] == (16 << 20) + 1
    for n in ns:
        nb = -(-n // B)
        assert n + 21 * nb + 17 <= lib.jfs_compress_bound(L.ALGO_ZSTD, n), n
    # a hand-built raw object of two frames has exactly header + block header + entry per frame
    obj, ent = S.build([bytes(B), bytes(1)])
    assert len(obj) == (B + 1) + (9 + 3 + 8) + (6 + 3 + 8) + 17


def test_mode_setters_without_a_device(lib):
    assert lib.jfs_zstd_parse_mode() == L.ZSTD_PARSE_EXACT and lib.jfs_read_seek_mode() == L.READ_SEEK_OFF
    try:
        assert lib.jfs_set_zstd_parse_mode(L.ZSTD_PARSE_SEEKABLE) == -1  # the first setter keeps its two modes
        assert lib.jfs_set_zstd_parse_mode_ext(3) == -1 and lib.jfs_set_zstd_parse_mode_ext(-1) == -1
        assert lib.jfs_zstd_parse_mode() == L.ZSTD_PARSE_EXACT
        assert lib.jfs_set_zstd_parse_mode_ext(L.ZSTD_PARSE_SEEKABLE) == L.ZSTD_PARSE_EXACT
        assert lib.jfs_zstd_parse_mode() == L.ZSTD_PARSE_SEEKABLE
        assert lib.jfs_set_zstd_parse_mode(L.ZSTD_PARSE_FAST) == L.ZSTD_PARSE_SEEKABLE
        assert C.set_zstd_parse_mode("seekable") == "fast"
        with C.zstd_parse_mode("exact"):
            assert lib.jfs_zstd_parse_mode() == L.ZSTD_PARSE_EXACT
        assert lib.jfs_zstd_parse_mode() == L.ZSTD_PARSE_SEEKABLE
        with pytest.raises(ValueError):
            C.set_zstd_parse_mode("seek")
        assert lib.jfs_set_read_seek_mode(2) == -1 and lib.jfs_set_read_seek_mode(-1) == -1
        assert C.read_seek_mode() == "off"
        assert C.set_read_seek_mode("on") == "off" and lib.jfs_read_seek_mode() == L.READ_SEEK_ON
        assert C.set_read_seek_mode("off") == "on"
        with pytest.raises(ValueError):
            C.set_read_seek_mode("ON")
    finally:
        lib.jfs_set_zstd_parse_mode_ext(L.ZSTD_PARSE_EXACT)
        lib.jfs_set_read_seek_mode(L.READ_SEEK_OFF)


def test_environment_and_no_device():
    import sys
    code = ("from juicefs_amd import _lib as L; lib = L.load();"
            "print(lib.jfs_zstd_parse_mode(), lib.jfs_read_seek_mode(),"
            " lib.jfs_zstd_compress_seekable_device(None, 1, None, None),"
            " lib.jfs_zstd_decompress_range_device(None, None, None, 1, None, None))")
    def child(env):
        e = dict(os.environ, **env)
        r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=ROOT, env=e, timeout=120)
        assert r.returncode == 0, r.stderr[-2000:]
        return [int(x) for x in r.stdout.split()]
    off = {"JFS_GPU_CODEC": "off"}
    assert child(dict(off, JFS_ZSTD_PARSE="Seekable", JFS_READ_SEEK="ON")) == [2, 1, L.JFS_ERR_NO_DEVICE, L.JFS_ERR_NO_DEVICE]
    assert child(dict(off, JFS_ZSTD_PARSE="seek", JFS_READ_SEEK="1"))[:2] == [0, 0]


def test_new_symbols_are_declared_and_exported(lib):
    header = open(os.path.join(ROOT, "include", "jfs_gpucodec.h")).read()
    for name in ("jfs_zstd_compress_seekable_device", "jfs_zstd_decompress_range_device", "jfs_set_zstd_parse_mode_ext",
                 "jfs_read_seek_mode", "jfs_set_read_seek_mode"):
        assert name in L.EXPORTS and hasattr(lib, name) and name + "(" in header, name
    assert "#define JFS_ZSTD_PARSE_SEEKABLE 2" in header and "#define JFS_READ_SEEK_ON 1" in header
