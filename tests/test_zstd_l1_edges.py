"""CPU: the directed edge inputs of the Zstd level-1 encoder (tests/zstd_l1_edges.py)
against tests/golden/zstd_l1_edges.json, libzstd 1.4.9's own frames of them.

  * coverage is a condition: the features the frame census (tests/zstd_frame_census.py)
    reads from the frames are every feature it can name except those listed as
    unreachable at level 1, and no frame shows an unreachable one -- recomputed
    from fresh libzstd frames where /opt/conda/lib/libzstd.so.1 loads, and from
    the oracle's frames, which the fixture ties to libzstd's, everywhere;
  * the census is a decoder of its own: it returns every input from its frame;
  * oracle/zstd_l1_oracle.c is byte-identical to every fixture entry, and to
    ZSTD_compress itself where libzstd loads.
Every comparison is equality of bytes or of sha256 hashes."""
import ctypes
import hashlib
import json
import os

import pytest

from tests import zstd_l1_edges as E
from tests.zstd_frame_census import FEATURES, census

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBZSTD = "/opt/conda/lib/libzstd.so.1"


def sha(b):
    return hashlib.sha256(b).hexdigest()


def fixture():
    with open(os.path.join(ROOT, "tests", "golden", "zstd_l1_edges.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def frames(oracle):
    """name -> (input, the oracle's frame, census features), each computed once"""
    out = {}
    for name in E.CASES:
        src = E.make(name)
        f = oracle.zstd_compress_l1(src)
        back, feats = census(f)
        assert back == src, name  # a census counts only when it decodes the frame back to the input
        out[name] = (src, f, feats)
    return out


def test_fixture_lists_the_cases():
    g = fixture()
    assert g["version"] == 10409 and g["level"] == 1
    assert [c["name"] for c in g["cases"]] == list(E.CASES)
    for c in g["cases"]:
        src = E.make(c["name"])
        assert len(src) == c["size"] and sha(src) == c["src_sha"], c["name"]


def test_features_are_accounted_for():
    assert len(set(FEATURES)) == len(FEATURES)
    assert set(E.UNREACHABLE) <= set(FEATURES)
    for name, (_, want) in E.CASES.items():
        assert set(want) <= set(FEATURES) - set(E.UNREACHABLE), name


def _check_coverage(per_case):
    seen = set()
    for name, feats in per_case.items():
        assert not feats & set(E.UNREACHABLE), (name, sorted(feats & set(E.UNREACHABLE)))
        missing = set(E.CASES[name][1]) - feats
        assert not missing, (name, sorted(missing))  # the case still reaches what it is there for
        seen |= feats
    assert seen == set(FEATURES) - set(E.UNREACHABLE), sorted(set(FEATURES) - set(E.UNREACHABLE) - seen)


def test_coverage_of_the_fixture():
    _check_coverage({c["name"]: set(c["features"]) for c in fixture()["cases"]})


def test_oracle_equals_fixture_and_census_decodes(frames):
    """the oracle's frames are libzstd's (sha256), decode back through the census, and
    show the recorded features; coverage recomputed from them"""
    for c in fixture()["cases"]:
        src, f, feats = frames[c["name"]]
        assert len(f) == c["csize"] and sha(f) == c["comp_sha"], (c["name"], len(f), c["csize"])
        assert sorted(feats) == c["features"], c["name"]
    _check_coverage({name: feats for name, (_, _, feats) in frames.items()})


def test_oracle_decoder_agrees_with_census(oracle, frames):
    for name, (src, f, _) in frames.items():
        n, out = oracle.zstd_decompress(f, len(src))
        assert n == len(src) and out == src, name


def test_libzstd_fresh_frames(frames):
    """ZSTD_compress(.., 1) now: the same bytes as the oracle's, the same census"""
    try:
        z = ctypes.CDLL(LIBZSTD)
    except OSError:
        pytest.skip("libzstd 1.4.9 not loadable here (the committed fixture still pins the oracle)")
    z.ZSTD_compress.restype = ctypes.c_size_t
    z.ZSTD_compress.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    z.ZSTD_compressBound.restype = ctypes.c_size_t
    z.ZSTD_compressBound.argtypes = [ctypes.c_size_t]
    per_case = {}
    for name, (src, f, _) in frames.items():
        cap = z.ZSTD_compressBound(len(src))
        d = ctypes.create_string_buffer(cap)
        m = z.ZSTD_compress(d, cap, src, len(src), 1)
        assert d.raw[:m] == f, name
        back, feats = census(d.raw[:m])
        assert back == src, name
        per_case[name] = feats
    _check_coverage(per_case)


def test_census_rejects_damage(frames):
    """the census checks what it reads: a cut frame, a wrong content size and a flipped
    block-type bit do not decode to the input"""
    from tests.zstd_frame_census import Corrupt
    src, f, _ = frames["size_255"]
    for bad in (f[:-1], f[:5] + bytes([f[5] ^ 1]) + f[6:], f[:6] + bytes([f[6] ^ 2]) + f[7:]):
        try:
            back, _ = census(bad)
        except Corrupt:
            continue
        assert back != src
