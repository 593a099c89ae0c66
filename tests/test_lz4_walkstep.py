"""Host check of the LZ4 decode parser's walk step (juicefs_amd/csrc/
lz4_walkstep.h, the code SegWalk::advance in lz4_decode.hip inlines): the step
tests a token's first match-length extension byte one iteration late, so a
match of >= 274 bytes is found after the lane already went on, and the lane has
to drop that step and take the exact rule's.  tests/walkstep_main.cc, built
with AddressSanitizer and UBSan, runs the deferred speculative and fix-up walks
and plain walks that ask the exact rule at every position, from every entry of
a pre-roll + segment, over crafted streams (extension bytes 254 / 255 0 /
255 255 k, a 255 where no extension is read, literal extensions with and
without 255, slow tokens in a row, in the pre-roll, last in a segment, joined
by a fix-up walk, streams truncated inside every field) and 10,000 seeded
random token streams of 300..20,000 bytes.  It compares the visited positions,
the exit and the STOP results and counts fetches outside [0, n).

Without the deferred test (a slow token never re-walked) the driver reports
mismatching visited positions and exits (bad > 0) in both kinds of walk."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_deferred_walk_matches_exact_walk(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    exe = str(tmp_path / "walkstep")
    r = subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "juicefs_amd", "csrc"),
                        os.path.join(ROOT, "tests", "walkstep_main.cc"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe, "10000"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    m = re.search(r"crafted=(\d+) random=(\d+) walks=(\d+) fixups=(\d+) redone=(\d+) arrived=(\d+) oob=(\d+) bad=(\d+)", r.stdout)
    assert m, r.stdout[-2000:]
    crafted, random, walks, fixups, redone, arrived, oob, bad = map(int, m.groups())
    assert bad == 0, r.stdout[-4000:]   # same visited positions, exit and STOP results
    assert oob == 0                     # every fetch index in [0, n)
    assert random >= 10000 and crafted > 1000
    # the cases are really there: slow tokens were re-walked, lanes settled past their segment, fix-up walks ran
    assert redone > 100000 and arrived > 100000 and fixups > 1000000
