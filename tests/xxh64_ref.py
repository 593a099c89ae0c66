"""XXH64 in plain Python (the xxHash specification, 64-bit variant): the
reference the GPU tests compare jfs_xxh64_device with, so that they depend on
nothing the machine may or may not have installed.  tests/test_xxh64_ref.py
pins it to known values."""
from __future__ import annotations

M = (1 << 64) - 1
P1, P2, P3, P4, P5 = (0x9E3779B185EBCA87, 0xC2B2AE3D27D4EB4F, 0x165667B19E3779F9, 0x85EBCA77C2B2AE63,
                      0x27D4EB2F165667C5)


def _rotl(x, r):
    return ((x << r) | (x >> (64 - r))) & M


def _round(acc, w):
    return (_rotl((acc + w * P2) & M, 31) * P1) & M


def xxh64(data: bytes, seed: int = 0) -> int:
    n, p = len(data), 0
    if n >= 32:
        v = [(seed + P1 + P2) & M, (seed + P2) & M, seed & M, (seed - P1) & M]
        while p + 32 <= n:
            for j in range(4):
                v[j] = _round(v[j], int.from_bytes(data[p + 8 * j:p + 8 * j + 8], "little"))
            p += 32
        h = (_rotl(v[0], 1) + _rotl(v[1], 7) + _rotl(v[2], 12) + _rotl(v[3], 18)) & M
        for x in v:
            h = ((h ^ _round(0, x)) * P1 + P4) & M
    else:
        h = (seed + P5) & M
    h = (h + n) & M
    while p + 8 <= n:
        h = (_rotl(h ^ _round(0, int.from_bytes(data[p:p + 8], "little")), 27) * P1 + P4) & M
        p += 8
    if p + 4 <= n:
        h = (_rotl(h ^ ((int.from_bytes(data[p:p + 4], "little") * P1) & M), 23) * P2 + P3) & M
        p += 4
    while p < n:
        h = (_rotl(h ^ ((data[p] * P5) & M), 11) * P1) & M
        p += 1
    h ^= h >> 33
    h = (h * P2) & M
    h ^= h >> 29
    h = (h * P3) & M
    return h ^ (h >> 32)
