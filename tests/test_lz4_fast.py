"""The fast LZ4 encoder without a GPU: its host twin (jfs_test_lz4_fast_host,
the kernels' parse restated in host C++), the parse-mode calls and the new
symbols.  JFS_LZ4_PARSE is matched case-insensitively, like JFS_GPU_CODEC:
"fast" / "FAST" / "bogus" give fast / fast / exact."""
import ctypes
import os
import subprocess
import sys

import pytest

from juicefs_amd import _lib as L
from juicefs_amd import compress as C
from juicefs_amd.blockgen import gen_block
from tests import lz4_fast_cases as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CANARY = 0xA5
PAD = 64


def twin(lib, src: bytes, cap: int):
    """(ret, dst bytes, canary intact) with dst inside a canary-filled buffer"""
    buf = (ctypes.c_uint8 * (cap + 2 * PAD))(*([CANARY] * (cap + 2 * PAD)))
    r = int(lib.jfs_test_lz4_fast_host(ctypes.addressof(buf) + PAD, cap, src, len(src)))
    raw = bytes(buf)
    clean = raw[:PAD] == bytes([CANARY]) * PAD and raw[PAD + cap:] == bytes([CANARY]) * PAD
    return r, raw[PAD:PAD + cap], clean


@pytest.mark.parametrize("name,src", K.cases(), ids=[c[0] for c in K.cases()])
def test_twin_block(lib, oracle, name, src):
    n = len(src)
    bound = oracle.lz4_bound(n)
    r, out, clean = twin(lib, src, bound)
    assert clean
    assert 0 < r <= bound
    comp = out[:r]
    assert out[r:] == bytes([CANARY]) * (bound - r), "bytes past the block were written"
    dn, back = oracle.lz4_decompress(comp, n)
    assert dn == n and back == src
    K.check_end_rules(comp, n)
    # deterministic
    r2, out2, _ = twin(lib, src, bound)
    assert (r2, out2) == (r, out)
    # exactly enough room succeeds with the same bytes
    r3, out3, clean3 = twin(lib, src, r)
    assert clean3 and r3 == r and out3 == comp
    # one byte short, or no room: 0 and not a byte written
    for cap in (r - 1, 0):
        r4, out4, clean4 = twin(lib, src, cap)
        assert r4 == 0 and clean4 and out4 == bytes([CANARY]) * cap


def test_twin_empty_is_one_zero_byte(lib):
    r, out, clean = twin(lib, b"", 1)
    assert (r, out, clean) == (1, b"\x00", True)


def test_twin_refuses_oversize_length(lib):
    d = ctypes.create_string_buffer(16)
    assert lib.jfs_test_lz4_fast_host(ctypes.addressof(d), 16, b"x", 0x7E000001) == 0


def test_carry_spans_chunks():
    # the special blocks do what their names say: a literal run longer than 270
    # bytes across the first chunk boundary, and a match cut at one
    d = dict(K.cases())
    src = d["lits-cross-chunk"]
    seqs = K.walk(C.lz4_fast_host(src), len(src))
    pos, crossing = 0, []
    for lit, mp, ml, off in seqs:
        if pos < K.CHUNK < pos + lit:
            crossing.append(lit)
        pos += lit + ml
    assert crossing and crossing[0] > 270
    src = d["match-cross-chunk"]
    seqs = K.walk(C.lz4_fast_host(src), len(src))
    assert any(mp is not None and mp + ml == K.CHUNK for lit, mp, ml, off in seqs), "no match ends at the chunk cut"


@pytest.mark.parametrize("cls", ["T", "Z"])
def test_size_guard_against_exact(oracle, cls):
    # 4 MiB, seed 1: independent 64 KiB cuts of the exact parse cost 0.99 (T) and
    # 1.04 (Z); a parse without matches costs 2x on text and one without short
    # offsets 255x on zeros.  1.10 separates the two.
    src = gen_block(cls, 1, 4 << 20)
    exact = oracle.lz4_compress(src)[0]
    fast = len(C.lz4_fast_host(src))
    print(f"class {cls}: fast {fast} exact {exact} ratio {fast / exact:.4f}")
    assert 0 < fast <= 1.10 * exact


def test_size_random_within_bound(oracle):
    src = gen_block("R", 1, 4 << 20)
    fast = len(C.lz4_fast_host(src))
    print(f"class R: fast {fast} bound {oracle.lz4_bound(len(src))}")
    assert 0 < fast <= oracle.lz4_bound(len(src))


def test_parse_mode_calls(lib):
    assert lib.jfs_lz4_parse_mode() == L.LZ4_PARSE_EXACT  # the default
    assert lib.jfs_set_lz4_parse_mode(2) == -1
    assert lib.jfs_set_lz4_parse_mode(-1) == -1
    assert lib.jfs_lz4_parse_mode() == L.LZ4_PARSE_EXACT
    try:
        assert lib.jfs_set_lz4_parse_mode(L.LZ4_PARSE_FAST) == L.LZ4_PARSE_EXACT
        assert lib.jfs_lz4_parse_mode() == L.LZ4_PARSE_FAST
    finally:
        assert lib.jfs_set_lz4_parse_mode(L.LZ4_PARSE_EXACT) == L.LZ4_PARSE_FAST
    assert lib.jfs_lz4_parse_mode() == L.LZ4_PARSE_EXACT


def test_parse_mode_context_manager_restores(lib):
    with pytest.raises(RuntimeError):
        with C.lz4_parse_mode("fast"):
            assert lib.jfs_lz4_parse_mode() == L.LZ4_PARSE_FAST
            with C.lz4_parse_mode("exact"):
                assert lib.jfs_lz4_parse_mode() == L.LZ4_PARSE_EXACT
            assert lib.jfs_lz4_parse_mode() == L.LZ4_PARSE_FAST
            raise RuntimeError("leave by exception")
    assert lib.jfs_lz4_parse_mode() == L.LZ4_PARSE_EXACT
    with pytest.raises(ValueError):
        with C.lz4_parse_mode("faster"):
            pass


def _child(env_extra, code):
    env = dict(os.environ)
    env.pop("JFS_LZ4_PARSE", None)
    env.update(env_extra)
    r = subprocess.run([sys.executable, "-c", code], env=env, cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    return [int(x) for x in r.stdout.split()]


def test_parse_mode_env():
    code = "from juicefs_amd import _lib as L; print(L.load().jfs_lz4_parse_mode())"
    assert _child({}, code) == [L.LZ4_PARSE_EXACT]
    assert _child({"JFS_LZ4_PARSE": "fast"}, code) == [L.LZ4_PARSE_FAST]
    assert _child({"JFS_LZ4_PARSE": "FAST"}, code) == [L.LZ4_PARSE_FAST]
    assert _child({"JFS_LZ4_PARSE": "exact"}, code) == [L.LZ4_PARSE_EXACT]
    assert _child({"JFS_LZ4_PARSE": "bogus"}, code) == [L.LZ4_PARSE_EXACT]


def test_fast_device_call_without_device():
    # JFS_GPU_CODEC=off: the library reports no device, with or without a GPU in the machine
    code = ("import ctypes; from juicefs_amd import _lib as L; lib = L.load(); "
            "n = (ctypes.c_int32 * 1)(5); print(lib.jfs_lz4_compress_fast_device(None, n, 1, None, None))")
    assert _child({"JFS_GPU_CODEC": "off"}, code) == [L.JFS_ERR_NO_DEVICE]


def test_new_symbols_exported(lib):
    for name in ("jfs_lz4_compress_fast_device", "jfs_lz4_parse_mode", "jfs_set_lz4_parse_mode"):
        assert name in L.EXPORTS and hasattr(lib, name), name
    # the twin is a test hook with a header of its own, outside the public ABI
    assert L.LZ4_FAST_TEST_EXPORTS == ["jfs_test_lz4_fast_host"] and hasattr(lib, "jfs_test_lz4_fast_host")
    assert "jfs_test_lz4_fast_host" not in L.EXPORTS
    inc = os.path.join(ROOT, "include")
    assert "jfs_test_lz4_fast_host(" in open(os.path.join(inc, "jfs_gpucodec_lz4_fast_test.h")).read()
    assert "jfs_test_lz4_fast_host" not in open(os.path.join(inc, "jfs_gpucodec.h")).read()
