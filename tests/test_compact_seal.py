"""CPU: jfs_compact_seal_batch's host-side validation -- the plan (as
jfs_compact_batch), the cipher, the key arrays and the seal parameters -- which
runs before any device is looked for, and the Python mirror's existence.  No
GPU compute is called here."""
import ctypes
import inspect
import os
import subprocess
import sys

import pytest

from juicefs_amd import _lib as L
from juicefs_amd import encrypt as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

KEY = ctypes.create_string_buffer(b"\x07" * 32, 32)
NONCE = ctypes.create_string_buffer(b"\x09" * 12, 12)
WRAPPED = ctypes.create_string_buffer(b"\x0b" * 256, 256)


def _ptr(buf):
    return ctypes.cast(buf, ctypes.c_void_p) if buf is not None else None


def _call(lib, algo, cipher, srcs, keys, outs, params, seg_first, seg, null=()):
    """jfs_compact_seal_batch over host buffers.  srcs: [(buf, len, block size)],
    keys: [buf or None], outs: [(buf, cap)], params: [(key, nonce, wrapped,
    wrapped_len)]; `null` names pointer arguments to pass as NULL."""
    ns, no = len(srcs), len(outs)
    siov, oiov = (L.JfsIov * max(ns, 1))(), (L.JfsIov * max(no, 1))()
    kp = (ctypes.c_void_p * max(ns, 1))()
    sp = (L.JfsSealParam * max(no, 1))()
    for i, (buf, n, cap) in enumerate(srcs):
        siov[i].src, siov[i].src_len, siov[i].dst_cap = _ptr(buf), n, cap
        kp[i] = _ptr(keys[i])
    for j, (buf, cap) in enumerate(outs):
        oiov[j].dst, oiov[j].dst_cap = _ptr(buf), cap
        key, nonce, wrapped, wl = params[j]
        sp[j].key, sp[j].nonce, sp[j].wrapped, sp[j].wrapped_len = _ptr(key), _ptr(nonce), _ptr(wrapped), wl
    first = (ctypes.c_int32 * max(len(seg_first), 1))(*seg_first)
    segs = (L.JfsCompactSeg * max(len(seg), 1))()
    for k, s in enumerate(seg):
        segs[k].src, segs[k].src_off, segs[k].dst_off, segs[k].len = s
    a_src_n, a_out_n = (ctypes.c_int64 * max(ns, 1))(), (ctypes.c_int64 * max(no, 1))()
    args = {"src": siov, "src_keys": kp, "out": oiov, "out_p": sp, "seg_first": first, "seg": segs, "src_n": a_src_n,
            "out_n": a_out_n}
    for k in null:
        args[k] = None
    return lib.jfs_compact_seal_batch(algo, cipher, ns, args["src"], args["src_keys"], no, args["out"], args["out_p"],
                                      args["seg_first"], args["seg"], args["src_n"], args["out_n"], None, 0)


def _valid():
    """(srcs, keys, outs, params, seg_first, seg): two envelopes, two outputs"""
    src = ctypes.create_string_buffer(b"\x00\x00\x0c" + b"\x10" * 60, 63)
    dst = ctypes.create_string_buffer(512)
    return ([(src, 63, 64), (src, 63, 64)], [KEY, KEY], [(dst, 512), (dst, 512)],
            [(KEY, NONCE, None, 0), (KEY, NONCE, WRAPPED, 256)], [0, 2, 3], [(0, 0, 0, 8), (-1, 0, 8, 4), (1, 3, 0, 5)])


def _with(i, value):
    def f(*a):
        a = list(a)
        a[i] = value(a[i])
        return a
    return f


INVALID_CASES = {
    "null_src_key_entry": _with(1, lambda k: [k[0], None]),
    "null_out_key": _with(3, lambda p: [(None, NONCE, None, 0), p[1]]),
    "null_out_nonce": _with(3, lambda p: [p[0], (KEY, None, WRAPPED, 256)]),
    "wrapped_len_65536": _with(3, lambda p: [p[0], (KEY, NONCE, WRAPPED, 65536)]),
    "wrapped_len_negative": _with(3, lambda p: [(KEY, NONCE, None, -1), p[1]]),
    "null_wrapped_with_len": _with(3, lambda p: [(KEY, NONCE, None, 1), p[1]]),
    "tiling_gap": _with(5, lambda g: [g[0], (-1, 0, 9, 4), g[2]]),
    "tiling_overlap": _with(5, lambda g: [g[0], (-1, 0, 7, 4), g[2]]),
    "first_not_zero": _with(5, lambda g: [g[0], g[1], (1, 3, 1, 5)]),
    "len_zero": _with(5, lambda g: [g[0], g[1], (1, 3, 0, 0)]),
    "src_index_nsrc": _with(5, lambda g: [g[0], g[1], (2, 3, 0, 5)]),
    "src_index_below_hole": _with(5, lambda g: [(-2, 0, 0, 8), g[1], g[2]]),
    "negative_src_off": _with(5, lambda g: [(0, -1, 0, 8), g[1], g[2]]),
    "seg_first_not_monotone": _with(4, lambda f: [0, 3, 2]),
    "negative_src_len": _with(0, lambda s: [(s[0][0], -1, 64), s[1]]),
    "negative_block_size": _with(0, lambda s: [s[0], (s[1][0], 63, -64)]),
    "null_src_bytes": _with(0, lambda s: [(None, 63, 64), s[1]]),
    "negative_dst_cap": _with(2, lambda o: [o[0], (o[1][0], -1)]),
    "null_dst_bytes": _with(2, lambda o: [(None, 512), o[1]]),
}


@pytest.mark.parametrize("algo", [L.ALGO_NONE, L.ALGO_LZ4, L.ALGO_ZSTD])
@pytest.mark.parametrize("name", sorted(INVALID_CASES))
def test_compact_seal_batch_rejects_invalid_arguments(lib, name, algo):
    assert _call(lib, algo, L.CIPHER_AES256GCM, *INVALID_CASES[name](*_valid())) == L.JFS_ERR_INVALID


@pytest.mark.parametrize("null", ["src", "src_keys", "out", "out_p", "seg_first", "seg", "src_n", "out_n"])
def test_compact_seal_batch_rejects_null_arrays(lib, null):
    assert _call(lib, L.ALGO_LZ4, L.CIPHER_SM4GCM, *_valid(), null=(null,)) == L.JFS_ERR_INVALID


def test_compact_seal_batch_rejects_bad_cipher_algo_and_counts(lib):
    for cipher in (-1, 3, 99):
        assert _call(lib, L.ALGO_LZ4, cipher, *_valid()) == L.JFS_ERR_INVALID
    for algo in (-1, 3):
        assert _call(lib, algo, L.CIPHER_AES256GCM, *_valid()) == L.JFS_ERR_INVALID
    none = [None] * 10
    assert lib.jfs_compact_seal_batch(L.ALGO_LZ4, 0, -1, None, None, 0, *none[:7], 0) == L.JFS_ERR_INVALID
    assert lib.jfs_compact_seal_batch(L.ALGO_LZ4, 0, 0, None, None, -1, *none[:7], 0) == L.JFS_ERR_INVALID


def test_compact_seal_batch_validates_then_reports_no_device():
    """With the engine switched off (JFS_GPU_CODEC=off: no device, as on a
    machine without a GPU) valid arguments return JFS_ERR_NO_DEVICE for every
    codec and cipher, and invalid ones still JFS_ERR_INVALID: validation comes
    first."""
    code = (
        "from tests.test_compact_seal import _call, _valid, INVALID_CASES\n"
        "from juicefs_amd import _lib as L\n"
        "lib = L.load()\n"
        "print(lib.jfs_device_count())\n"
        "for a in (0, 1, 2):\n"
        "    for c in (0, 1, 2): print(_call(lib, a, c, *_valid()))\n"
        "for n in sorted(INVALID_CASES): print(_call(lib, 1, 0, *INVALID_CASES[n](*_valid())))\n"
        "print(_call(lib, 1, 7, *_valid()))\n"
        "print(_call(lib, 1, 0, [], [], [], [], [0], []))\n")
    env = dict(os.environ, JFS_GPU_CODEC="off")
    r = subprocess.run([sys.executable, "-c", code], env=env, cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    got = [int(x) for x in r.stdout.split()]
    assert got == ([0] + [L.JFS_ERR_NO_DEVICE] * 9 + [L.JFS_ERR_INVALID] * (len(INVALID_CASES) + 1) +
                   [L.JFS_ERR_NO_DEVICE])


def test_python_mirror_exists_and_checks_its_arguments():
    sig = inspect.signature(E.compact_seal_batch)
    assert list(sig.parameters) == ["codec", "algo", "sources", "keys", "outputs", "params", "plan", "device_mask",
                                    "with_crc"]
    assert sig.parameters["device_mask"].default == 0 and sig.parameters["with_crc"].default is False
    env, key, nonce = b"\x00\x00\x0c" + b"\x10" * 60, b"\x07" * 32, b"\x09" * 12
    with pytest.raises(ValueError):  # seg_first: one entry per output plus one
        E.compact_seal_batch(L.ALGO_LZ4, E.AES256GCM_RSA, [(env, 64)], [key], [bytearray(64)], [(key, nonce, b"")],
                             ([0], []))
    with pytest.raises(ValueError):  # a key per source
        E.compact_seal_batch(L.ALGO_LZ4, E.AES256GCM_RSA, [(env, 64)], [], [bytearray(64)], [(key, nonce, b"")],
                             ([0, 0], []))
    with pytest.raises(ValueError):  # the cipher's key size, before anything reaches the library
        E.compact_seal_batch(L.ALGO_LZ4, E.SM4GCM, [(env, 64)], [key], [bytearray(64)], [(key[:16], nonce, b"")],
                             ([0, 0], []))
    with pytest.raises(ValueError):  # 12-byte nonces
        E.compact_seal_batch(L.ALGO_LZ4, E.AES256GCM_RSA, [(env, 64)], [key], [bytearray(64)], [(key, nonce[:11], b"")],
                             ([0, 0], []))
