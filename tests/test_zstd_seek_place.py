"""Host check of the placement rule the seekable Zstd decode's kernels share
with the CPU: Rounds, rounds_build and place_frame of
juicefs_amd/csrc/zstd_seek.h against the serial selectors seek_select,
table_select and ranges_select, on hand-built tables of both entry sizes with
1, 63, 64, 65, 128, 129 and MAX_FRAMES frames and on seeded random tables and
selections, under AddressSanitizer + UBSan (tests/zstd_seek_place_main.cc, a
stand-alone program whose fetch counts every index outside its buffer)."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RANDOM = 4000


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    out = str(tmp_path_factory.mktemp("zplace") / "zstd_seek_place_main")
    r = subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "juicefs_amd", "csrc"),
                        os.path.join(ROOT, "tests", "zstd_seek_place_main.cc"), "-o", out], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return out


def test_every_placement_is_the_serial_selectors_frame(exe):
    r = subprocess.run([exe, str(RANDOM)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    m = re.fullmatch(r"cases=(\d+) placed=(\d+) oob=0 bad=0", r.stdout.strip().split("\n")[-1])
    assert m, r.stdout[-2000:]
    # 7 counts x 2 layouts x 30 fixed selections and the random ones; the MAX_FRAMES tables alone place 100,000
    assert int(m.group(1)) == 7 * 2 * 30 + RANDOM and int(m.group(2)) > 100000
