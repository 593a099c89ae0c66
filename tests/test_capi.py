"""CPU: libjfsgpu.so loads, exports every symbol include/jfs_gpucodec.h
declares, and its host-only surface behaves like pkg/compress.  No GPU compute
is called here."""
import ctypes
import os
import re

from juicefs_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_functions(names=("jfs_gpucodec.h", "jfs_gpucodec_test.h")):
    """Functions the public header (and the test-hook header) declare."""
    out = set()
    for h in names:
        src = open(os.path.join(ROOT, "include", h)).read()
        src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
        out |= set(re.findall(r"\b(jfs_[a-z0-9_]+)\s*\(", src))
    return sorted(out)


def test_test_hooks_not_in_public_header():
    # the lock-order test hook is not part of the drop-in ABI
    assert "jfs_test_spread_locking" not in header_functions(("jfs_gpucodec.h",))
    # nor is the small-batch decoders' jump-round override
    assert "jfs_test_set_split_jump_rounds" not in header_functions(("jfs_gpucodec.h",))
    assert header_functions(("jfs_gpucodec_test.h",)) == ["jfs_test_set_split_jump_rounds", "jfs_test_spread_locking"]


def test_exports_every_header_symbol(lib):
    names = header_functions()
    assert len(names) >= 14
    assert sorted(L.EXPORTS) == names
    for n in names:
        assert hasattr(lib, n), n


def test_new_compressor_names(lib):
    # compress.go:39-49 (case-insensitive), Name() strings :53,76,109
    for s, a in [(b"zstd", 2), (b"ZSTD", 2), (b"Zstd", 2), (b"lz4", 1), (b"LZ4", 1), (b"none", 0), (b"", 0),
                 (b"NONE", 0), (b"gzip", -1), (b"lz4hc", -1)]:
        assert lib.jfs_codec_from_name(s) == a
    assert lib.jfs_codec_name(0) == b"Noop" and lib.jfs_codec_name(1) == b"LZ4" and lib.jfs_codec_name(2) == b"Zstd"
    assert lib.jfs_codec_name(7) is None


def test_compress_bound(lib):
    # LZ4_compressBound / ZSTD_COMPRESSBOUND
    assert lib.jfs_compress_bound(1, 4 << 20) == 4210768
    assert lib.jfs_compress_bound(1, 64 << 10) == 65809  # liblz4 1.9.3 (SURVEY a4 says 65,808: off by one)
    assert lib.jfs_compress_bound(1, 0) == 16
    assert lib.jfs_compress_bound(1, 0x7E000001) == 0
    assert lib.jfs_compress_bound(2, 4 << 20) == 4210688
    assert lib.jfs_compress_bound(2, 0) == 64
    assert lib.jfs_compress_bound(2, 3) == 66 and lib.jfs_compress_bound(2, 4) == 67
    assert lib.jfs_compress_bound(0, 12345) == 12345


def test_noop_is_copy_with_short_buffer_error(lib):
    # compress.go:55-68
    src = b"Noop"
    dst = ctypes.create_string_buffer(4)
    assert lib.jfs_compress(0, dst, 4, src, 4) == 4 and dst.raw == src
    assert lib.jfs_compress(0, dst, 1, src, 4) == L.JFS_ERR_SHORT_BUFFER
    assert lib.jfs_decompress(0, dst, 1, src, 4) == L.JFS_ERR_SHORT_BUFFER


def test_empty_input_errors_before_device(lib):
    dst = ctypes.create_string_buffer(100)
    # LZ4.Decompress empty -> "decompress an empty input" (compress.go:121-123)
    assert lib.jfs_decompress(1, dst, 100, None, 0) == L.JFS_ERR_EMPTY_INPUT
    # zstd.Decompress empty -> ErrEmptySlice
    assert lib.jfs_decompress(2, dst, 100, None, 0) == L.JFS_ERR_EMPTY_INPUT


def test_version(lib):
    assert b"gfx950" in lib.jfs_version()


def _stats(lib):
    arr = (L.JfsOpStats * L.STATS_N)()
    assert lib.jfs_stats(arr, L.STATS_N) == L.STATS_N
    return arr


def test_stats_count_host_path_blocks(lib):
    # counters behind cachedStore's data-bytes metrics (cached_store.go:931-974);
    # the "none" codec is a host memmove, so this runs without a GPU
    lib.jfs_stats_reset()
    src = b"x" * 1000
    dst = ctypes.create_string_buffer(1000)
    assert lib.jfs_compress(0, dst, 1000, src, 1000) == 1000
    assert lib.jfs_compress(0, dst, 10, src, 1000) == L.JFS_ERR_SHORT_BUFFER
    assert lib.jfs_decompress(0, dst, 1000, src, 600) == 600
    iov = (L.JfsIov * 2)(L.JfsIov(ctypes.cast(src, ctypes.c_void_p), 100, ctypes.addressof(dst), 1000),
                         L.JfsIov(ctypes.cast(src, ctypes.c_void_p), 200, ctypes.addressof(dst), 1000))
    out = (ctypes.c_int64 * 2)()
    assert lib.jfs_compress_batch(0, 2, iov, out, 0) == 0 and list(out) == [100, 200]
    s = _stats(lib)
    c, d = s[0], s[1]  # algo none: compress, decompress
    assert (c.calls, c.blocks, c.bytes_in, c.bytes_out, c.errors) == (3, 4, 1300, 1300, 1)
    assert (d.calls, d.blocks, d.bytes_in, d.bytes_out, d.errors) == (1, 1, 600, 600, 0)
    assert all(s[i].calls == 0 for i in range(2, L.STATS_N))
    lib.jfs_stats_reset()
    assert _stats(lib)[0].calls == 0


def _mode_in_subprocess(env_value, devices=None):
    import subprocess
    import sys
    env = dict(os.environ)
    env["JFS_GPU_CODEC"] = env_value
    if devices is not None:
        env["JFS_GPU_DEVICES"] = devices
    code = ("import ctypes; from juicefs_amd import _lib as L; lib = L.load(); "
            "d = ctypes.create_string_buffer(64); "
            "print(lib.jfs_gpu_mode(), lib.jfs_device_count(), lib.jfs_compress(1, d, 64, b'a' * 20, 20))")
    r = subprocess.run([sys.executable, "-c", code], env=env, cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    return [int(x) for x in r.stdout.split()]


def test_codec_selector_env():
    # JFS_GPU_CODEC=off|auto|force (+ JFS_GPU_DEVICES mask)
    mode, ndev, rc = _mode_in_subprocess("off")
    assert (mode, ndev, rc) == (L.MODE_OFF, 0, L.JFS_ERR_NO_DEVICE)
    assert _mode_in_subprocess("FORCE")[0] == L.MODE_FORCE
    assert _mode_in_subprocess("auto")[0] == L.MODE_AUTO
    assert _mode_in_subprocess("bogus")[0] == L.MODE_AUTO
    # an empty device selection leaves no device (and no CPU fallback)
    mode, ndev, rc = _mode_in_subprocess("force", devices="0x0")
    assert (mode, ndev, rc) == (L.MODE_FORCE, 0, L.JFS_ERR_NO_DEVICE)


def test_seal_and_open_refuse_wrong_key_and_nonce_sizes(lib):
    # dataEncryptor.aead (pkg/object/encrypt.go:182-202) errors on a wrong key
    # size; the batch ABI reads key_size / 12 bytes through plain pointers, so
    # the Python layer refuses short buffers before any library call
    import pytest
    from juicefs_amd import encrypt as E
    raw = b"x" * 100
    dst = bytearray(1024)
    for algo, ks in [(E.AES256GCM_RSA, 32), (E.CHACHA20_RSA, 32), (E.SM4GCM, 16)]:
        assert E.key_size(algo) == ks
        with pytest.raises(ValueError, match="key"):
            E.compress_seal_batch(0, algo, [(dst, raw)], [(b"k" * (ks - 1), b"n" * 12, b"w")])
        with pytest.raises(ValueError, match="key"):
            E.compress_seal_batch(0, algo, [(dst, raw)], [(b"k" * (ks + 1), b"n" * 12, b"w")])
        with pytest.raises(ValueError, match="nonce"):
            E.compress_seal_batch(0, algo, [(dst, raw)], [(b"k" * ks, b"n" * 8, b"w")])
        with pytest.raises(ValueError, match="key"):
            E.open_decompress_batch(0, algo, [(dst, raw)], [b"k" * 16 if ks == 32 else b"k" * 32])


def test_deal_plan_size_balanced(lib):
    """the batch calls deal blocks over devices size-balanced
    (config 4's mixed 64 KiB - 4 MiB blocks), not by count -- checked on the
    policy itself with fake device counts (no GPU needed)."""
    import random
    i64, i32 = ctypes.c_int64, ctypes.c_int32

    def plan(cost, ndev):
        c = (i64 * len(cost))(*cost)
        o = (i32 * len(cost))()
        lib.jfs_deal_plan(c, len(cost), ndev, o)
        return list(o)

    rng = random.Random(8)
    for ndev in (1, 2, 3, 8):
        for n in (1, 5, 64, 500):
            cost = [int(2 ** rng.uniform(16, 22)) for _ in range(n)]  # 64 KiB .. 4 MiB, log-uniform
            w = plan(cost, ndev)
            assert all(0 <= d < ndev for d in w)
            load = [0] * ndev
            for c, d in zip(cost, w):
                load[d] += c
            used = [x for x in load if x > 0]
            assert len(used) == min(ndev, n)
            assert max(load) - min(load) <= max(cost) or n < ndev  # LPT: within one block
            assert plan(cost, ndev) == w  # deterministic
    # count-balanced round robin would put both 4 MiB blocks on device 0 here
    cost = [4 << 20, 64 << 10, 4 << 20, 64 << 10]
    w = plan(cost, 2)
    assert w[0] != w[2]


def test_spread_lock_order_no_deadlock(lib):
    """the coalescer's burst spreading takes the worker's own
    lane first (blocking) and other devices' lanes only by try_lock.  Run that
    acquisition concurrently on fake devices (host only, no GPU): every worker
    of every device spreading at once must finish, and the spread branch (a
    foreign lane taken) must actually be exercised."""
    for ndev in (2, 3, 8):
        r = lib.jfs_test_spread_locking(ndev, 2000, 20000)
        assert r != -1, f"spread lane acquisition deadlocked with {ndev} devices"
        assert r > 0, "no burst took a foreign lane: the multi-device branch did not run"
    assert lib.jfs_test_spread_locking(0, 1, 10) == -2
