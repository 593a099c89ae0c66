"""Host check of the LZ4 decode parser's walk step at both segment lengths
(juicefs_amd/csrc/lz4_walkstep.h: BitSet<SEG>, ws_spec_iter, ws_fix_iter as
SegWalk::advance in lz4_decode.hip calls them, SEG = 128 and 256).  The fix-up
walk records its positions into vt directly (there is no third set): vt is
cleared when the walk starts and a join ORs the speculative chain's suffix in.

tests/walkseg_main.cc, a stand-alone program built with AddressSanitizer and
UBSan, runs for each SEG the speculative and the fix-up walk and plain walks
that ask ws_next_exact at every position, from every entry of pre-roll +
segment, over the crafted streams of tests/walkstep_main.cc's kinds, the same
tokens placed in the last 3 / first 3 bytes around bit 64, 128 and 192 of a
segment, streams truncated inside every field, and seeded random token streams.
It compares visited positions, exits and STOP results, counts fetches outside
[0, n), and checks every BitSet<SEG> operation against std::bitset for every
(d, on) in [0, SEG)."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LINE = re.compile(r"seg=(\d+) crafted=(\d+) random=(\d+) walks=(\d+) fixups=(\d+) redone=(\d+) arrived=(\d+) "
                  r"straddle=(\d+) setops=(\d+) oob=(\d+) bad=(\d+)")


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("walkseg") / "walkseg")
    r = subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "juicefs_amd", "csrc"),
                        os.path.join(ROOT, "tests", "walkseg_main.cc"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe, "3000"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    rows = {int(m.group(1)): tuple(map(int, m.groups()[1:])) for m in LINE.finditer(r.stdout)}
    assert sorted(rows) == [128, 256], r.stdout[-2000:]
    return rows, r.stdout


@pytest.mark.parametrize("seg", [128, 256])
def test_walks_and_sets_match_plain_ones(report, seg):
    rows, out = report
    crafted, random, walks, fixups, redone, arrived, straddle, setops, oob, bad = rows[seg]
    assert bad == 0, out[-4000:]   # same visited positions, exit and STOP results; BitSet == std::bitset
    assert oob == 0                # every fetch index in [0, n)
    assert random >= 3000 and crafted > 1000
    # the cases are really there: slow tokens re-walked, lanes settled past their
    # segment, fix-up walks, tokens across a word of the set, every (d, on)
    assert redone > 30000 and arrived > 30000 and fixups > 300000
    assert straddle > 1000
    assert setops >= 4 * seg * (2 * 3 + 7)
