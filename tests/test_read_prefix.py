"""CPU: the read calls' decode mode (jfs_read_decode_mode /
jfs_set_read_decode_mode, JFS_READ_DECODE) and the exported prefix-decode
surface.  No GPU compute is called here."""
import os
import subprocess
import sys

import pytest

from juicefs_amd import _lib as L
from juicefs_amd import compress as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _child(code, **env):
    e = {k: v for k, v in os.environ.items() if k != "JFS_READ_DECODE"}
    e.update(env)
    r = subprocess.run([sys.executable, "-c", code], env=e, cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    return r.stdout.split()


def test_mode_default_and_setter():
    # in a child: the mode is process-wide, and the environment of the test run is not this test's to trust
    code = ("from juicefs_amd import _lib as L\n"
            "lib = L.load()\n"
            "print(lib.jfs_read_decode_mode())\n"
            "for m in (2, -1): print(lib.jfs_set_read_decode_mode(m), lib.jfs_read_decode_mode())\n"
            "print(lib.jfs_set_read_decode_mode(1), lib.jfs_read_decode_mode())\n"
            "for m in (2, -1): print(lib.jfs_set_read_decode_mode(m), lib.jfs_read_decode_mode())\n"
            "print(lib.jfs_set_read_decode_mode(0), lib.jfs_read_decode_mode())\n")
    got = [int(x) for x in _child(code)]
    full, prefix = L.READ_DECODE_FULL, L.READ_DECODE_PREFIX
    assert (full, prefix) == (0, 1)
    assert got == [full, -1, full, -1, full, full, prefix, -1, prefix, -1, prefix, prefix, full]


@pytest.mark.parametrize("value,mode", [("prefix", 1), ("PREFIX", 1), ("Prefix", 1), ("full", 0), ("FULL", 0),
                                        ("", 0), ("partial", 0), ("1", 0), (None, 0)])
def test_mode_from_environment(value, mode):
    code = "from juicefs_amd import _lib as L\nprint(L.load().jfs_read_decode_mode())\n"
    env = {} if value is None else {"JFS_READ_DECODE": value}
    assert _child(code, **env) == [str(mode)]


def test_python_helpers(lib):
    prev = C.read_decode_mode()
    try:
        assert C.set_read_decode_mode("prefix") == prev
        assert C.read_decode_mode() == "prefix" and lib.jfs_read_decode_mode() == L.READ_DECODE_PREFIX
        assert C.set_read_decode_mode("full") == "prefix"
        assert C.read_decode_mode() == "full"
        with pytest.raises(ValueError):
            C.set_read_decode_mode("partial")
        assert C.read_decode_mode() == "full"
    finally:
        C.set_read_decode_mode(prev)


def test_new_symbols_exported(lib):
    for name in ("jfs_lz4_decompress_prefix_device", "jfs_lz4_decompress_prefix_device_small",
                 "jfs_read_decode_mode", "jfs_set_read_decode_mode"):
        assert name in L.EXPORTS
        assert hasattr(lib, name), name


def test_prefix_device_calls_report_no_device():
    """With the engine switched off (JFS_GPU_CODEC=off: no device, as on a
    machine without a GPU) both device calls answer JFS_ERR_NO_DEVICE, in
    either decode mode; the read call still validates first."""
    code = ("import ctypes\n"
            "from tests.test_read import _call, _valid, INVALID_CASES\n"
            "from juicefs_amd import _lib as L\n"
            "lib = L.load()\n"
            "print(lib.jfs_device_count())\n"
            "one = (ctypes.c_int32 * 1)(16)\n"
            "print(lib.jfs_lz4_decompress_prefix_device(None, None, 1, None, None))\n"
            "print(lib.jfs_lz4_decompress_prefix_device_small(None, one, one, None, 1, None, None))\n"
            "print(lib.jfs_read_decode_mode())\n"
            "print(_call(lib, 1, *_valid()))\n"
            "print(_call(lib, 1, *INVALID_CASES['tiling_gap'](*_valid())))\n")
    got = [int(x) for x in _child(code, JFS_GPU_CODEC="off", JFS_READ_DECODE="prefix")]
    nd = L.JFS_ERR_NO_DEVICE
    assert got == [0, nd, nd, L.READ_DECODE_PREFIX, nd, L.JFS_ERR_INVALID]
