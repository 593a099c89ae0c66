"""The splice switch of the Zstd compaction call without a GPU:
its default, setters and environment values, the counters, the new names in the
header and the export list, and the device call's answer without a device."""
import ctypes
import os
import subprocess
import sys

import pytest

from juicefs_amd import _lib as L
from juicefs_amd import compress as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("jfs_zstd_splice_device", "jfs_compact_splice_mode", "jfs_set_compact_splice_mode", "jfs_compact_splice_counts")


def test_switch_is_off_and_settable(lib):
    assert lib.jfs_compact_splice_mode() == L.COMPACT_SPLICE_OFF and C.compact_splice_mode() == "off"
    try:
        assert lib.jfs_set_compact_splice_mode(2) == -1 and lib.jfs_set_compact_splice_mode(-1) == -1
        assert lib.jfs_compact_splice_mode() == L.COMPACT_SPLICE_OFF
        assert C.set_compact_splice_mode("on") == "off" and lib.jfs_compact_splice_mode() == L.COMPACT_SPLICE_ON
        assert C.compact_splice_mode() == "on"
        assert C.set_compact_splice_mode("off") == "on"
        with pytest.raises(ValueError):
            C.set_compact_splice_mode("ON")
    finally:
        lib.jfs_set_compact_splice_mode(L.COMPACT_SPLICE_OFF)


def test_counters(lib):
    assert C.compact_splice_counts(reset=True) is not None
    assert C.compact_splice_counts() == (0, 0, 0, 0)
    assert lib.jfs_compact_splice_counts(None, 0) == -1


def test_environment_and_no_device():
    code = ("from juicefs_amd import _lib as L; lib = L.load();"
            "print(lib.jfs_compact_splice_mode(), lib.jfs_zstd_splice_device(None, 1, None, 0, None, None, None, None))")

    def child(env):
        e = dict(os.environ, **env)
        r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=ROOT, env=e, timeout=120)
        assert r.returncode == 0, r.stderr[-2000:]
        return [int(x) for x in r.stdout.split()]
    off = {"JFS_GPU_CODEC": "off"}
    assert child(dict(off, JFS_COMPACT_SPLICE="On")) == [1, L.JFS_ERR_NO_DEVICE]
    assert child(dict(off, JFS_COMPACT_SPLICE="1"))[0] == 0
    assert child(dict(off, JFS_COMPACT_SPLICE="off"))[0] == 0


def test_new_symbols_are_declared_and_exported(lib):
    header = open(os.path.join(ROOT, "include", "jfs_gpucodec.h")).read()
    for name in NEW:
        assert name in L.EXPORTS and hasattr(lib, name) and name + "(" in header, name
    for text in ("#define JFS_COMPACT_SPLICE_OFF 0", "#define JFS_COMPACT_SPLICE_ON 1", "} jfs_splice_frame;",
                 "} jfs_splice_out;"):
        assert text in header, text
    assert lib.jfs_zstd_splice_device.restype is ctypes.c_int64
    assert ctypes.sizeof(L.JfsSpliceFrame) == 32 and ctypes.sizeof(L.JfsSpliceOut) == 24
    from juicefs_amd import device as D
    assert callable(D.zstd_splice) and D.SPLICE_FRAME_DTYPE.itemsize == 32 and D.SPLICE_OUT_DTYPE.itemsize == 24
