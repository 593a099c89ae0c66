"""Host check of the LZ4 window decode's rules (juicefs_amd/csrc/lz4_window.h:
the chunk floor, the reach rule, the entry clipping) and of its switch's row in
juicefs_amd/csrc/host_modes.h.  tests/lz4_window_main.cc, built with
AddressSanitizer and UBSan, applies the header to directed streams and to both
encoders' output and compares the bytes a decode from the floor defines with a
serial LZ interpreter's.  Nothing is loaded into Python under a sanitizer.

The property the feature rests on is checked here too: in every block of two
chunks or more from the fast encoder no sequence reaches below any chunk floor,
and the exact encoder's blocks do have such sequences (the probe has something
to find).  tests/test_lz4_window_gpu.py relies on it for its counters."""
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

from juicefs_amd import compress as C
from tests import lz4_chase_cases as K
from tests import lz4_fast_cases as F
from tests.test_modes import H, _check_setter, _children, _mixed

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHUNK = F.CHUNK


def _rand(seed, n):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


def chunked_stream(nfull=2, ragged=5130):
    """nfull chunks of exactly CHUNK output bytes, each literals and one match inside the chunk, then a ragged one"""
    out = b"".join(K.seq(_rand(40 + k, CHUNK - 40), 40, 17) for k in range(nfull))
    return out + K.seq(_rand(50, ragged - 130), 30, 9) + K.last(_rand(51, 100))


def directed():
    """[(name, stream, lo, hi, expected floor, expected below)]"""
    out = []
    # a match ending exactly at the chunk boundary; the next chunk's match stays above it
    ends = K.seq(_rand(1, CHUNK - 20), 20, 100) + K.seq(_rand(2, 50), 10, 30) + K.last(_rand(3, 12))
    out.append(("match-ends-at-boundary", ends, CHUNK + 4, CHUNK + 70, CHUNK, 0))
    out.append(("lo-on-boundary", ends, CHUNK, CHUNK + 72, CHUNK, 0))
    out.append(("lo-one-below-boundary", ends, CHUNK - 1, CHUNK + 72, 0, 0))
    # a literal run across the boundary (65,008 .. 66,008); its match copies from above the boundary
    lits = K.seq(_rand(4, 65000), 8, 50) + K.seq(_rand(5, 1000), 10, 20) + K.last(_rand(6, 12))
    out.append(("literals-straddle", lits, CHUNK + 64, 1 << 20, CHUNK, 0))
    # overlapped matches at the boundary: starting on it they copy byte F - 1 (below); behind `off` literals they do not
    for off in (1, 2, 3):
        on = K.seq(_rand(7, CHUNK), 300, off) + K.last(_rand(8, 12))
        out.append((f"overlap-off{off}-on-boundary", on, CHUNK + 10, CHUNK + 290, 0, 1))
        behind = K.seq(_rand(9, CHUNK + off), 300, off) + K.last(_rand(10, 12))
        out.append((f"overlap-off{off}-behind-literals", behind, CHUNK + 10, CHUNK + 290, CHUNK, 0))
    # a match across the boundary sends the floor to 0 -- for a window in the chunk behind it; a chunk later it is unseen
    cross = K.seq(_rand(11, CHUNK - 6), 20, 10) + K.seq(_rand(12, CHUNK - 14 - 40), 40, 17) + K.seq(_rand(13, 900), 30, 9) \
        + K.last(_rand(14, 100))
    out.append(("match-straddles", cross, CHUNK + 100, CHUNK + 200, 0, 1))
    out.append(("match-straddles-window-ends-in-it", cross, CHUNK + 1, CHUNK + 3, 0, 1))
    out.append(("match-straddles-a-chunk-earlier", cross, 2 * CHUNK + 5, 2 * CHUNK + 500, 2 * CHUNK, 0))
    # a match in the window that copies from the chunk in front (offset across the boundary)
    far = K.seq(_rand(15, CHUNK + 100), 16, 300) + K.last(_rand(16, 12))
    out.append(("offset-crosses", far, CHUNK + 50, CHUNK + 128, 0, 1))
    out.append(("offset-crosses-behind-window", far, CHUNK + 5, CHUNK + 100, CHUNK, 0))  # (the match starts at H)
    # the ragged last chunk, the block's end, windows past it
    rag = chunked_stream()
    total = 2 * CHUNK + 5130
    out.append(("lo-in-ragged-chunk", rag, 2 * CHUNK + 4000, total, 2 * CHUNK, 0))
    out.append(("hi-past-total", rag, CHUNK + 9, total + 500, CHUNK, 0))
    out.append(("lo-in-chunk-0", rag, 77, 3000, 0, 0))
    out.append(("negative-lo", rag, -5, 100, 0, 0))
    out.append(("window-across-two-boundaries", rag, CHUNK - 3, total - 1, 0, 0))
    out.append(("empty-window", rag, CHUNK + 50, CHUNK + 50, CHUNK, 0))
    return out


def run_driver(tmp, records):
    """records: [(stream, lo, hi)] -> the driver's rows as dicts, and its last line"""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    exe, data = str(tmp / "lz4_window"), str(tmp / "cases.bin")
    if not os.path.exists(exe):
        r = subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "juicefs_amd", "csrc"),
                            os.path.join(ROOT, "tests", "lz4_window_main.cc"), "-o", exe], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
    with open(data, "wb") as f:
        for s, lo, hi in records:
            f.write(struct.pack("<Iii", len(s), lo, hi) + s)
    r = subprocess.run([exe, data], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    keys = ("case", "n", "total", "fc", "below", "floor", "wrong", "escape", "forced", "reach")
    rows = [dict(zip(keys, map(int, m))) for m in re.findall(
        r"^case (\d+) n (\d+) total (\d+) fc (\d+) below (\d+) floor (\d+) wrong (\d+) escape (\d+) forced (\d+) reach (\d+)$",
        r.stdout, re.M)]
    assert len(rows) == len(records), r.stdout[-2000:]
    return rows, r.stdout.strip().splitlines()[-1]


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    return tmp_path_factory.mktemp("lz4_window")


def test_floor_and_reach_rule_on_directed_streams(built):
    cases = directed()
    rows, _ = run_driver(built, [(s, lo, hi) for _, s, lo, hi, _, _ in cases])
    for (name, s, lo, hi, floor, below), row in zip(cases, rows):
        assert row["n"] == len(s)
        assert row["fc"] == (max(lo, 0) // CHUNK) * CHUNK, name
        assert (row["floor"], row["below"]) == (floor, below), (name, row)
        # decoded from the floor the rule gives, the window's bytes are the interpreter's and no pointer leaves it
        assert (row["wrong"], row["escape"]) == (0, 0), (name, row)
        # and the probe is what keeps it so: held at Fc against its verdict, a pointer escapes -- exactly then
        assert (row["forced"] > 0) == bool(below), (name, row)
    # the streams are what their names say
    by = {name: K.sequences(s) for name, s, *_ in cases}
    ll, _, ml, off = by["match-ends-at-boundary"][0]
    assert ll + ml == CHUNK
    ll, _, ml, off = by["match-straddles"][0]
    assert ll < CHUNK < ll + ml
    (l0, _, m0, _), (l1, _, _, _) = by["literals-straddle"][:2]
    assert l0 + m0 < CHUNK < l0 + m0 + l1
    for o in (1, 2, 3):
        ll, _, ml, off = by[f"overlap-off{o}-on-boundary"][0]
        assert ll == CHUNK and ml > off == o
    assert sum(ll + ml for ll, _, ml, _ in K.sequences(chunked_stream())) == 2 * CHUNK + 5130


@pytest.fixture(scope="module")
def encoded(oracle):
    """[(name, source, fast stream, exact stream)] for the fast-parse inputs of two chunks or more"""
    out = []
    for name, src in F.cases():
        if len(src) > CHUNK:
            out.append((name, src, C.lz4_fast_host(src), oracle.lz4_compress(src)[1]))
    assert len(out) >= 20 and any(n.startswith("T-") for n, *_ in out)
    return out


def test_fast_blocks_never_reach_below_a_chunk_floor(built, encoded):
    """every chunk floor of every input, H = total (the widest window): no sequence of the fast encoder reaches below"""
    recs = []
    for name, src, fast, _ in encoded:
        for k in range(1, (len(src) + CHUNK - 1) // CHUNK):
            recs.append((fast, k * CHUNK + 1, len(src)))
    rows, _ = run_driver(built, recs)
    i = 0
    for name, src, fast, _ in encoded:
        for k in range(1, (len(src) + CHUNK - 1) // CHUNK):
            row = rows[i]
            i += 1
            assert row["total"] == len(src), name
            assert (row["reach"], row["below"], row["floor"]) == (0, 0, k * CHUNK), (name, k, row)
            assert (row["wrong"], row["escape"]) == (0, 0), (name, k, row)


def test_exact_blocks_do_reach_below(built, encoded):
    """the exact encoder matches across chunk boundaries: the rule sends such windows to floor 0, and decodes them right"""
    recs = [(exact, CHUNK + 1, len(src)) for _, src, _, exact in encoded]
    rows, _ = run_driver(built, recs)
    reaching = []
    for (name, src, _, _), row in zip(encoded, rows):
        assert (row["wrong"], row["escape"]) == (0, 0), (name, row)
        assert row["floor"] == (0 if row["below"] else CHUNK), (name, row)
        assert (row["forced"] > 0) == bool(row["below"]), (name, row)
        if row["reach"] > 0:
            reaching.append(name)
    assert any(n.startswith("T-") for n in reaching), reaching


def test_mode_row_parses(built):
    _, last = run_driver(built, [(K.last(b"twelve bytes"), 0, 12)])
    assert last == "cases=1 modes_bad=0", last


def test_switch_environment_setter_and_default():
    """JFS_READ_LZ4_WINDOW as tests/test_modes.py checks the other switches: spellings in any case, no prefix match,
    no trimming; the setter answers the previous value, or -1 and no change"""
    var, getter, setter = "JFS_READ_LZ4_WINDOW", "jfs_read_lz4_window_mode", "jfs_set_read_lz4_window_mode"
    words = {"off": H["JFS_READ_LZ4_WINDOW_OFF"], "on": H["JFS_READ_LZ4_WINDOW_ON"]}
    assert list(words.values()) == [0, 1]
    expect = {None: 0, "bogus": 0, "1": 0, "": 0}
    for w, val in words.items():
        expect[w] = expect[w.upper()] = expect[_mixed(w)] = val
        expect[w + "x"] = expect[" " + w] = 0
    tries = [-1, 0, 1, 2, 3, 1, 0, 7, 2**31 - 1, -2**31]
    got = _children(var, getter, expect, [[setter, tries]])
    assert {v: g["get"] for v, g in got.items()} == expect
    _check_setter(got[None]["sets"], setter, [0, 1])
    rows = [r for r in got[None]["sets"] if r[1] == 2]
    assert rows and all((ans, after) == (-1, before) for _, _, before, ans, after in rows)
    assert C.read_lz4_window_mode() in ("off", "on")
    with pytest.raises(ValueError):
        C.set_read_lz4_window_mode("sparse")
