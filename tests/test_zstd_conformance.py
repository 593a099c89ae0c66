"""CPU: the hand-assembled conformance frames (tests/zstd_conformance_cases.py,
written by tests/zstd_frames.py) against libzstd 1.4.9's recorded verdicts
(tests/golden/zstd_conformance.json), the frame writer's own model, and the
CPU oracle (oracle/zstd_oracle.c)."""
import ctypes
import hashlib

import pytest

from tests import zstd_conformance_cases as K
from tests import zstd_frames as Z


def sha(b):
    return hashlib.sha256(b).hexdigest()


@pytest.fixture(scope="module")
def fx():
    return K.fixture()


def of_group(g):
    return [c for c in K.CASES if c["group"] == g]


def test_case_list_is_whole(fx):
    """Every group is present, names are unique, every case and cap is in the
    fixture and the fixture holds nothing else; every reject has its accepted
    twin (or its reason needs none: it is a size or a cut of the input)."""
    assert {c["group"] for c in K.CASES} == set(K.GROUPS)
    want = {(c["name"], cap) for c in K.CASES for cap in K.caps(c)}
    assert want == set(fx)
    for c in K.CASES:
        assert c["intent"] in ("accept", "reject", "verdict") and c["why"]
        if c["twin"]:
            assert K.BY_NAME[c["twin"]]["intent"] == "accept"
    n = {i: sum(1 for c in K.CASES if c["intent"] == i) for i in ("accept", "reject", "verdict")}
    print("cases:", len(K.CASES), n)
    assert n["accept"] >= 200 and n["reject"] >= 80


def test_xxh64_of_the_writer(oracle):
    for n in (0, 1, 3, 4, 7, 8, 31, 32, 33, 100, 1000):
        b = (bytes(range(256)) * 4)[:n]
        assert Z.xxh64(b) == oracle.xxh64(b)


@pytest.mark.parametrize("group", K.GROUPS)
def test_frames_model_and_verdicts(fx, group):
    """The rebuilt frame has the fixture's sha; accept cases decode in the
    fixture to exactly expand(description); every intended reject is a reject
    in the fixture (but for the four libzstd 1.4.9 leaves unchecked, K.LAX_149), as corrupt or wrong source size and never by its cap,
    and its twin an accept; a short cap is dstSize_tooSmall or the frame's own
    error, never a success."""
    for c in of_group(group):
        src, exp = K.built(c)
        for cap in K.caps(c):
            e = fx[(c["name"], cap)]
            assert sha(src) == e["frame_sha"], c["name"]
            if cap < c["size"] and c["intent"] == "accept":
                assert e["ret"] < 0, (c["name"], cap)
        e = fx[(c["name"], c["size"])]
        if c["intent"] == "accept":
            assert e["ret"] == len(exp) == c["size"] and e["out_sha"] == sha(exp), (c["name"], e["ret"], e["err"])
        elif c["intent"] == "reject":
            assert exp is None
            # corrupt or wrong source size, never "too small": the cap is not what rejects it
            assert (e["ret"] in (-1, -3)) != (c["name"] in K.LAX_149), (c["name"], e["ret"])
            assert c["name"] not in K.LAX_149 or e["ret"] >= 0, c["name"]
            if c["twin"]:
                t = K.BY_NAME[c["twin"]]
                assert fx[(t["name"], t["size"])]["ret"] == t["size"], c["name"]
        elif e["ret"] >= 0:
            assert exp is not None and e["ret"] == len(exp) and e["out_sha"] == sha(exp), c["name"]
        else:
            assert exp is None, c["name"]


@pytest.mark.parametrize("group", K.GROUPS)
def test_oracle_agrees(oracle, fx, group):
    """oracle.zstd_decompress gives the fixture's result and bytes; in its
    default (zstd >= 1.5) mode it rejects the K.LAX_149 cases at their exact
    cap as corrupt, in its 1.4.9 mode it accepts those of them whose output is
    defined (no over-read stream)."""
    for c in of_group(group):
        src, _ = K.built(c)
        for cap in K.caps(c):
            want, wsha = K.expected(c, fx[(c["name"], cap)], oracle)
            r, out = oracle.zstd_decompress(src, cap)
            assert r == want and (r < 0 or sha(out) == wsha), (c["name"], cap, r, want)
            assert c["name"] not in K.LAX_149 or cap < c["size"] or r == -1, c["name"]
    oracle.zstd_strict_reserved(False)
    try:
        for c in of_group(group):
            if c["name"] in ("one_spare_bit", "reserved_mode_bits"):
                for cap in K.caps(c):
                    e = fx[(c["name"], cap)]
                    r, out = oracle.zstd_decompress(K.built(c)[0], cap)
                    assert r == e["ret"] and (r < 0 or sha(out) == e["out_sha"]), (c["name"], cap, r)
    finally:
        oracle.zstd_strict_reserved(True)


def test_live_libzstd_agrees(fx):
    """Where a libzstd is installed, it agrees with the fixture (a library of
    another version may differ on K.LAX_149 and on error categories only)."""
    from juicefs_amd import device as D

    def zstd_err(name):  # as tests/golden/make_golden.py
        return -2 if "too small" in name else -3 if "Src size is incorrect" in name else -1

    z = D._libzstd()
    if z is None:
        return
    z.ZSTD_getErrorName.restype = ctypes.c_char_p
    z.ZSTD_getErrorName.argtypes = [ctypes.c_size_t]
    z.ZSTD_versionNumber.restype = ctypes.c_uint
    same = z.ZSTD_versionNumber() == 10409
    for c in K.CASES:
        src, _ = K.built(c)
        for cap in K.caps(c):
            e = fx[(c["name"], cap)]
            dst = ctypes.create_string_buffer(max(cap, 1))
            n = z.ZSTD_decompress(dst, cap, src, len(src))
            if z.ZSTD_isError(n):
                r = zstd_err(z.ZSTD_getErrorName(n).decode())
                assert e["ret"] < 0 or (not same and c["name"] in K.LAX_149), (c["name"], cap)
                assert not same or r == e["ret"], (c["name"], cap, r)
            else:
                assert n == e["ret"] and sha(dst.raw[:n]) == e["out_sha"], (c["name"], cap, n)
