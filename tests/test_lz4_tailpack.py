"""Host check of the LZ4 decode copier's ordered-tail descriptor (tail_pack in
juicefs_amd/csrc/lz4_tailpack.h, the code the kernel's batch() inlines): a
stand-alone program packs every (destination slot, source slot, length) of the
stated ranges (4096 x 4095 x 64 cases), unpacks it and compares the direct bit
with the byte-wise definition of the whole-wave copy."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_tail_pack_all_cases(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    exe = str(tmp_path / "tailpack")
    r = subprocess.run([cxx, "-O2", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "juicefs_amd", "csrc"),
                        os.path.join(ROOT, "tests", "tailpack_main.cc"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert f"cases={4096 * 4095 * 64} bad=0" in r.stdout, r.stdout
