"""Host checks of the spliced compaction's rule:
juicefs_amd/csrc/splice_plan.h against a pure-Python restatement written here,
field by field -- the tables, which pieces pass, the frames of every spliced
output, the units and segments of the derived plan, the lists of ranges it still
reads of every source, the counters -- on hand-built tables of 1 to 130 frames
in both layouts against both output layouts, identity plans, overwrites inside
a frame, at a frame edge and across two, shifted plans, short last frames,
holes, contiguous segments, frames without content, the c = d + 21 limit,
damaged tables, outputs of one piece, and 5,000 seeded random plans, under
AddressSanitizer + UBSan (tests/splice_plan_main.cc, a stand-alone program whose
fetch counts every index outside an object)."""
import json
import os
import random
import shutil
import struct
import subprocess

import pytest

from tests import zstd_seek_csum_cases as X
from tests.zstd_seek_cases import MAX_FRAMES, SEEK_MAGIC, SKIP_MAGIC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = 131072
SLACK = 21


# ---- the restatement ---------------------------------------------------------
def parse_any(obj: bytes):
    """(entries, entry size) of a valid table of either layout at the end of obj, else None"""
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
    return ent, e


def clip(segs, lo, hi):
    out = []
    for src, so, do, n in segs:
        a, b = max(do, lo), min(do + n, hi)
        if b > a:
            out.append([src, 0 if src < 0 else so + a - do, a - lo, b - a])
    return out


def merged(ranges):
    out = []
    for lo, hi in sorted(ranges):
        if out and lo <= out[-1][1]:
            out[-1][1] = max(out[-1][1], hi)
        else:
            out.append([lo, hi])
    return out


def rule(srcs, seg_first, seg, use, csum_out):
    """the issue's rule, by brute force: what splice_plan and splice_ranges must answer"""
    tabs, parsed = [], []
    for obj, cap in srcs:
        p = parse_any(obj)
        if p is not None and sum(x[1] for x in p[0]) > cap:
            p = None
        parsed.append(p)
        tabs.append([1, p[1], len(p[0]), sum(x[1] for x in p[0])] if p else [0, 0, 0, 0])
    frame_first, frames, units, dseg = [], [], [], []
    counts = [0, 0, 0, 0]
    for j in range(len(seg_first) - 1):
        frame_first.append(len(frames))
        if not use[j]:
            continue
        segs = seg[seg_first[j]:seg_first[j + 1]]
        total = sum(s[3] for s in segs)
        kinds = []
        for lo in (range(0, total, F) if total > F else []):
            hi, res = min(lo + F, total), None
            cover = [s for s in segs if s[2] <= lo and s[2] + s[3] >= hi]
            if cover and cover[0][0] >= 0:
                src, so, do, _ = cover[0]
                p = parsed[src]
                if p is not None and (not csum_out or p[1] == 12):
                    at, dpos, cpos = so + lo - do, 0, 0
                    for k, x in enumerate(p[0]):
                        if dpos == at and x[1] == hi - lo and x[1] > 0:
                            if x[0] <= x[1] + SLACK:
                                res = [src, k, cpos, x[0], x[1], x[2] if p[1] == 12 else 0, -1]
                            break
                        cpos, dpos = cpos + x[0], dpos + x[1]
            kinds.append((lo, hi, res))
        if not any(r for _, _, r in kinds):
            first = len(dseg)
            dseg += clip(segs, 0, total)
            units.append([j, -1, total, first, len(dseg)])
            continue
        counts[0] += 1
        for f, (lo, hi, res) in enumerate(kinds):
            if res is None:
                first = len(dseg)
                dseg += clip(segs, lo, hi)
                res = [-1, -1, 0, 0, hi - lo, 0, len(units)]
                units.append([j, f, hi - lo, first, len(dseg)])
                counts[2] += 1
            else:
                counts[1] += 1
                counts[3] += res[3]
            frames.append(res)
    frame_first.append(len(frames))
    ranges = {}
    for i, (obj, cap) in enumerate(srcs):
        if len(obj) == 0:
            continue
        cap = min(cap, 2 ** 31 - 1)
        rr = [(min(max(s[1], 0), cap), min(s[1] + s[3], cap)) for s in dseg if s[0] == i]
        ranges[str(i)] = merged([r for r in rr if r[1] > r[0]])
    return dict(tab=tabs, frame_first=frame_first, frames=frames, units=units, seg=dseg, ranges=ranges, counts=counts,
                oob=0)


# ---- the cases -----------------------------------------------------------------
def entries(ds, wide, cs=None):
    out = []
    for k, d in enumerate(ds):
        c = cs[k] if cs else 1 + (k * 5) % 3
        out.append((c, d) + (((k * 2654435761 + 12345) & 0xFFFFFFFF,) if wide else ()))
    return out


def obj_of(ent, filler=b"\x28") -> bytes:
    """an object as the rule sees it: as many bytes as the frames take (never read) and the table"""
    return filler * sum(x[0] for x in ent) + X.table(ent)


def source(ds, wide, cs=None, cap=None):
    ent = entries(ds, wide, cs)
    return obj_of(ent), sum(ds) if cap is None else cap


def identity(srcs):
    """one output per source, the source whole"""
    seg_first, seg = [0], []
    for i, (obj, cap) in enumerate(srcs):
        if cap > 0:
            seg.append((i, 0, 0, cap))
        seg_first.append(len(seg))
    return seg_first, seg


def case(srcs, seg_first, seg, csum_out, use=None):
    return (srcs, list(seg_first), [tuple(s) for s in seg], use or [1] * (len(seg_first) - 1), int(csum_out))


def hand_cases():
    cases = []
    for nf in (1, 2, 5, 64, 65, 130):
        for wide in (False, True):
            for csum_out in (False, True):
                for tail in (F, 777):  # a short last frame, as source and as output tail
                    s = [source([F] * (nf - 1) + [tail], wide)]
                    cases.append(case(s, *identity(s), csum_out))
    for wide in (False, True):
        for csum_out in (False, True):
            a = source([F] * 4 + [5000], wide)
            b = (b"\x01" * 300, 4096)  # the overwrite: an object without a table
            d = a[1]
            for x in (2 * F + 1000, 2 * F, 2 * F - 2048, 0, 4 * F + 904):  # inside a frame, at an edge, across two
                cases.append(case([a, b], [0, 3] if x else [0, 2],
                                  ([(0, 0, 0, x)] if x else []) + [(1, 0, x, 4096), (0, x + 4096, x + 4096, d - x - 4096)],
                                  csum_out))
            cases.append(case([a], [0, 1], [(0, 1, 0, d - 1)], csum_out))             # shifted by one byte
            cases.append(case([a], [0, 2], [(-1, 0, 0, 1), (0, 0, 1, d)], csum_out))       # pushed by one byte
            cases.append(case([a], [0, 3], [(0, 0, 0, F), (-1, 0, F, F), (0, 2 * F, 2 * F, d - 2 * F)], csum_out))  # a hole
            cases.append(case([a], [0, 2], [(0, 0, 0, F + 100), (0, F + 100, F + 100, d - F - 100)], csum_out))  # contiguous
            cases.append(case([a], [0, 1], [(0, F, 0, d - F)], csum_out))             # frames 1.. as pieces 0..
            cases.append(case([a], [0, 1], [(0, 0, 0, F)], csum_out))                 # total <= F
            cases.append(case([a], [0, 1], [(0, 0, 0, F + 1)], csum_out))             # a one-byte tail
            cases.append(case([a, a], [0, 1, 2], [(0, 0, 0, d), (1, 0, 0, d)], csum_out, use=[0, 1]))
            z = source([F, 0, F, 0, 0, 500, 0], wide)                                  # frames without content
            cases.append(case([z], *identity([z]), csum_out))
            lim = source([F, F, F, 9], wide, cs=[F + 21, F + 22, 3, 9 + 22])          # the encoder's worst case, and past it
            cases.append(case([lim], *identity([lim]), csum_out))
            bad = bytearray(a[0])
            bad[-1] ^= 1                                                               # a damaged table
            cases.append(case([(bytes(bad), d)], [0, 1], [(0, 0, 0, d)], csum_out))
            ent = entries([F] * 3, wide)
            lie = obj_of(ent)[1:]                                                      # compressed sizes that do not add up
            cases.append(case([(lie, 3 * F)], [0, 1], [(0, 0, 0, 3 * F)], csum_out))
            cases.append(case([(a[0], d - 1)], [0, 1], [(0, 0, 0, d - 1)], csum_out))  # the content does not fit the block
            cases.append(case([(b"", 0), a], [0, 1], [(1, 0, 0, d)], csum_out))        # an empty object beside it
    return cases


def random_cases(n, seed):
    rng = random.Random(seed)
    cases = []
    for _ in range(n):
        srcs = []
        for _ in range(rng.randint(1, 3)):
            kind = rng.random()
            if kind < 0.15:
                srcs.append((bytes(rng.randrange(256) for _ in range(rng.randint(0, 40))), rng.choice([0, 4096, F, 3 * F])))
                continue
            ds = [rng.choice([F, F, F, F, 0, rng.randint(1, F)]) for _ in range(rng.randint(1, 6))]
            cs = [rng.choice([1, 2, 3, d + 21, d + 22]) if rng.random() < 0.1 else rng.randint(1, 3) for d in ds]
            obj, cap = source(ds, rng.random() < 0.5, cs)
            if kind < 0.22:
                b = bytearray(obj)
                b[rng.randrange(len(b) - 17 - 8, len(b))] ^= 1 << rng.randrange(8)
                obj = bytes(b)
            srcs.append((obj, cap + rng.choice([0, 0, 0, 1, -1, F])))
        seg_first, seg = [0], []
        for _ in range(rng.randint(1, 3)):
            pos = 0
            for _ in range(rng.randint(0, 5)):
                i = rng.randrange(-1, len(srcs))
                kind = rng.random()
                if kind < 0.6:    # whole frames' worth, from a frame edge of an all-F table
                    so, n = F * rng.randint(0, 3), F * rng.randint(1, 4) + rng.choice([0, 0, 500, 1])
                elif kind < 0.8:  # a small overwrite
                    so, n = rng.randint(0, 9000), rng.choice([1, 4096, F - 4096, 4095])
                else:
                    so, n = rng.randint(0, 5 * F), rng.randint(1, 3 * F)
                seg.append((i, 0 if i < 0 else so, pos, n))
                pos += n
            seg_first.append(len(seg))
        use = [int(rng.random() < 0.9) for _ in range(len(seg_first) - 1)]
        cases.append(case(srcs, seg_first, seg, rng.random() < 0.5, use))
    return cases


# ---- the program ---------------------------------------------------------------
@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    out = str(tmp_path_factory.mktemp("splice") / "splice_plan_main")
    r = subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "juicefs_amd", "csrc"),
                        os.path.join(ROOT, "tests", "splice_plan_main.cc"), "-o", out], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return out


def run_cases(exe, tmp_path, cases):
    path = str(tmp_path / "cases.bin")
    with open(path, "wb") as f:
        for srcs, seg_first, seg, use, csum_out in cases:
            f.write(struct.pack("<i", len(srcs)))
            for obj, cap in srcs:
                f.write(struct.pack("<qi", cap, len(obj)) + obj)
            f.write(struct.pack("<ii", len(seg_first) - 1, csum_out) + bytes(use))
            f.write(struct.pack(f"<{len(seg_first)}i", *seg_first))
            for s in seg:
                f.write(struct.pack("<4i", *s))
    r = subprocess.run([exe, path], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    out = [json.loads(line) for line in r.stdout.splitlines()]
    assert len(out) == len(cases)
    return out


def check(cases, got):
    passed = 0
    for q, (c, g) in enumerate(zip(cases, got)):
        srcs, seg_first, seg, use, csum_out = c
        want = rule(srcs, seg_first, seg, use, csum_out)
        for key in want:
            assert g[key] == want[key], (q, key, c[1:], g[key], want[key])
        assert g["oob"] == 0
        # the derived plan tiles each unit, and a unit is a whole output or one piece
        for out, piece, total, s0, s1 in g["units"]:
            pos = 0
            for src, so, do, n in g["seg"][s0:s1]:
                assert do == pos and n > 0 and (src < 0 or so >= 0)
                pos += n
            assert pos == total and (piece < 0 or 0 < total <= F)
        # the lists: ascending, disjoint, not touching; a source only PASS pieces reference has none
        read = {s[0] for s in g["seg"] if s[0] >= 0}
        for i, lst in g["ranges"].items():
            assert all(lo < hi for lo, hi in lst) and all(a[1] < b[0] for a, b in zip(lst, lst[1:]))
            if int(i) not in read:
                assert lst == []
        passed += g["counts"][1]
    return passed


def test_hand_built_plans(exe, tmp_path):
    cases = hand_cases()
    got = run_cases(exe, tmp_path, cases)
    assert check(cases, got) > 0


def test_layouts_and_limits(exe, tmp_path):
    a8, a12 = source([F] * 4 + [5000], False), source([F] * 4 + [5000], True)
    lim = source([F, F, F], False, cs=[F + 21, F + 22, 3])
    zero = source([F, 0, F], False)
    cases = [case([a8], *identity([a8]), False), case([a8], *identity([a8]), True),
             case([a12], *identity([a12]), False), case([a12], *identity([a12]), True),
             case([a8], [0, 1], [(0, 1, 0, a8[1] - 1)], False), case([lim], *identity([lim]), False),
             case([zero], *identity([zero]), False),
             case([a8, (b"x" * 9, 4096)], [0, 3], [(0, 0, 0, F + 7), (1, 0, F + 7, 4096), (0, F + 4103, F + 4103, a8[1] - F - 4103)], False)]
    got = run_cases(exe, tmp_path, cases)
    check(cases, got)
    assert got[0]["counts"] == [1, 5, 0, sum(x[0] for x in entries([F] * 4 + [5000], False))]
    assert got[1]["counts"] == [0, 0, 0, 0] and got[1]["units"] == [[0, -1, a8[1], 0, 1]]  # 12-byte output, 8-byte source
    assert got[2]["counts"][:3] == [1, 5, 0]                                             # a 12-byte source feeds either layout
    assert got[3]["counts"][:3] == [1, 5, 0] and all(f[5] != 0 for f in got[3]["frames"])
    assert got[4]["counts"] == [0, 0, 0, 0]                                              # shifted by one byte
    assert [f[0] for f in got[5]["frames"]] == [0, -1, 0]                                # c = d + 21 passes, d + 22 does not
    assert [f[1] for f in got[6]["frames"]] == [0, 2]                                    # the frames without content are skipped
    assert got[0]["ranges"] == {"0": []} and got[0]["units"] == []                      # nothing left to decode
    assert got[7]["counts"][:3] == [1, 4, 1]                                             # one overwrite inside frame 1
    assert got[7]["ranges"] == {"0": [[F, F + 7], [F + 4103, 2 * F]], "1": [[0, 4096]]}


def test_random_plans(exe, tmp_path):
    cases = random_cases(5000, 20261020)
    got = run_cases(exe, tmp_path, cases)
    passed = check(cases, got)
    spliced = sum(g["counts"][0] for g in got)
    assert passed > 1000 and spliced > 500, (passed, spliced)  # the generator reaches both sides of the rule
