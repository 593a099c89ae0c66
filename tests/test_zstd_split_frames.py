"""CPU: the frame limit of the Zstd small-batch decode path
(jfs_set_zstd_split_frames / JFS_ZSTD_SPLIT_FRAMES) -- argument
checks, the Python wrappers and the environment parse, through libjfsgpu.so
without a device."""
import os
import subprocess
import sys

import pytest

from juicefs_amd import _lib as L
from juicefs_amd import compress as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX = 16384


def test_setter_checks_its_argument(lib):
    assert L.ZSTD_SPLIT_FRAMES_MAX == MAX
    assert lib.jfs_get_zstd_split_frames() == MAX
    try:
        for bad in (0, -1, MAX + 1, 1 << 30, -(1 << 31)):
            assert lib.jfs_set_zstd_split_frames(bad) == -1
            assert lib.jfs_get_zstd_split_frames() == MAX
        assert lib.jfs_set_zstd_split_frames(1) == MAX and lib.jfs_get_zstd_split_frames() == 1
        assert lib.jfs_set_zstd_split_frames(0) == -1 and lib.jfs_get_zstd_split_frames() == 1
        assert lib.jfs_set_zstd_split_frames(MAX) == 1
        assert C.set_zstd_split_frames(32) == MAX and C.zstd_split_frames() == 32
        for bad in (0, MAX + 1, "4", 2.0, True, None):
            with pytest.raises(ValueError):
                C.set_zstd_split_frames(bad)
        assert C.zstd_split_frames() == 32
    finally:
        lib.jfs_set_zstd_split_frames(MAX)


def test_environment_is_read_once():
    code = ("import os; from juicefs_amd import _lib as L; lib = L.load();"
            "a = lib.jfs_get_zstd_split_frames(); os.environ['JFS_ZSTD_SPLIT_FRAMES'] = '7';"
            "print(a, lib.jfs_get_zstd_split_frames())")

    def child(value):
        e = dict(os.environ, JFS_GPU_CODEC="off")
        e.pop("JFS_ZSTD_SPLIT_FRAMES", None)
        if value is not None:
            e["JFS_ZSTD_SPLIT_FRAMES"] = value
        r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=ROOT, env=e, timeout=120)
        assert r.returncode == 0, r.stderr[-2000:]
        return [int(x) for x in r.stdout.split()]
    assert child(None) == [MAX, MAX]
    assert child("1") == [1, 1] and child("16384") == [MAX, MAX] and child("40") == [40, 40]
    for junk in ("0", "-3", "16385", "", "12x", "x", "99999999999999999999"):
        assert child(junk) == [MAX, MAX], junk


def test_symbols_are_declared_and_exported(lib):
    header = open(os.path.join(ROOT, "include", "jfs_gpucodec.h")).read()
    for name in ("jfs_get_zstd_split_frames", "jfs_set_zstd_split_frames", "jfs_zstd_split_frame_counts"):
        assert name in L.EXPORTS and hasattr(lib, name) and name + "(" in header, name
    assert "#define JFS_ZSTD_SPLIT_FRAMES_MAX 16384" in header
