"""Host check of the origin-map rules both small-batch decoders share
(juicefs_amd/csrc/origin_map.h: entry writers, jump step, gather step, round
rule).  tests/origin_map_main.cc, built with AddressSanitizer and UBSan, fills
maps with the header's writers from (ll, ml, off) sequences, settles them with
the header's jump step in the synchronous model (every round reads a snapshot
taken before it: the slowest schedule a GPU can produce), gathers with the
header's gather step and compares with a serial interpreter: flat chains at the
round rule's edges for units 3 and 4 (settled after exactly rounds() rounds),
overlapped matches at every residue of p & 3, partial final quads with poisoned
entries behind the map, an unsettled gather, dst misaligned by 1, 2 and 3.

The driver also prints rounds(n, unit) for a list of sizes; the second test
holds tests/split_streams.py jump_rounds, which the GPU tests rely on, to it."""
import os
import re
import shutil
import subprocess

import pytest

from tests import split_streams as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def driver_output(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("origin_map") / "origin_map")
    r = subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "juicefs_amd", "csrc"),
                        os.path.join(ROOT, "tests", "origin_map_main.cc"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    return r.stdout


def test_writers_jump_gather_match_serial_decode(driver_output):
    m = re.search(r"cases=(\d+) unsettled_quads=(\d+) residues=(\d+),(\d+),(\d+),(\d+) bad=(\d+)", driver_output)
    assert m, driver_output[-2000:]
    cases, unsettled, r0, r1, r2, r3, bad = map(int, m.groups())
    assert bad == 0, driver_output[-4000:]
    assert cases > 1000                     # the overlap / residue / cut grid really ran
    assert min(r0, r1, r2, r3) > 0          # every total & 3, partial final quads included
    assert unsettled > 0                    # one round on the k = 3 flat chain leaves pointers, and the gather says so


def test_python_round_rule_is_the_header_rule(driver_output):
    rows = [tuple(map(int, m)) for m in re.findall(r"^rounds (\d+) (\d+) (\d+)$", driver_output, re.M)]
    want = {(n, unit) for unit in (3, 4) for k in range(1, 8) for n in S.bound_edge_sizes(k, unit)}
    assert want <= {(n, unit) for n, unit, _ in rows}
    for n, unit, jr in rows:
        assert S.jump_rounds(n, unit) == jr, (n, unit)
    assert {jr for _, _, jr in rows} >= set(range(1, 9))  # the list crosses every step up to a 4 MiB block's 8 rounds
