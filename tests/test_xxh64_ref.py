"""The pure-Python XXH64 of tests/xxh64_ref.py, pinned: the GPU tests of
jfs_xxh64_device and of the checksummed seek tables compare against it."""
import ctypes

import pytest

from tests.xxh64_ref import xxh64

# seed 0; computed with the xxhash module and libzstd's ZSTD_XXH64
PINNED = [
    (b"", 0xEF46DB3751D8E999),
    (b"a", 0xD24EC4F1A98C6E5B),
    (b"abc", 0x44BC2CF5AD770999),
    (bytes(range(32)), 0xCBF59C5116FF32B4),
    (bytes(range(33)), 0x0C535D1ACAFB8EAD),
    (bytes(i * 7 & 255 for i in range(131072)), 0x0CFEBAB741444537),
]
LENGTHS = [0, 1, 3, 4, 7, 8, 15, 31, 32, 33, 63, 64, 95, 96, 127, 4095]


def test_pinned_values():
    for data, want in PINNED:
        assert xxh64(data) == want, (len(data), hex(xxh64(data)))


def test_against_xxhash_module():
    xxhash = pytest.importorskip("xxhash")
    for n in LENGTHS:
        data = bytes((i * 131 + n) & 255 for i in range(n))
        assert xxh64(data) == xxhash.xxh64(data, seed=0).intdigest(), n


def test_against_libzstd():
    from juicefs_amd import device as D
    z = D._libzstd()
    if z is None or not hasattr(z, "ZSTD_XXH64"):
        pytest.skip("no libzstd with ZSTD_XXH64 to load")
    z.ZSTD_XXH64.restype = ctypes.c_uint64
    z.ZSTD_XXH64.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint64]
    for n in LENGTHS:
        data = bytes((i * 131 + n) & 255 for i in range(n))
        assert xxh64(data) == z.ZSTD_XXH64(data, n, 0), n
