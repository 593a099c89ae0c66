"""Host check of the LZ4 decode copier's byte masks (put16_masks in
juicefs_amd/csrc/lz4_put16.h, the code the kernel's put16 inlines): a
stand-alone program compares the five dword masks with the byte-wise
definition for all 4 x 16 (ha, m) cases.  The program is its own executable,
built with the address and undefined-behaviour sanitizers where the host
compiler has them (the shifts are the point: none may reach its width)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_put16_masks_all_cases(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    exe = str(tmp_path / "put16_masks")
    base = [cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "juicefs_amd", "csrc"),
            os.path.join(ROOT, "tests", "put16_masks_main.cc"), "-o", exe]
    r = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True,
                       text=True)
    if r.returncode != 0:  # a compiler without the sanitizer runtimes: the plain program checks the same values
        r = subprocess.run(base, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "cases=64 bad=0" in r.stdout, r.stdout
