"""GPU: the hand-assembled conformance frames (tests/zstd_conformance_cases.py)
through the Zstd decoder's three batch shapes -- a call of its own (the
small-batch path, juicefs_amd/csrc/zstd_split.inc), mixed batches of 7, and
one batch of more than 128 inputs (the one-wave path of zstd_decode.hip) --
and a dozen of them through read assembly and compaction.  Bar: result code
and bytes of libzstd 1.4.9's recorded verdicts (tests/golden/
zstd_conformance.json; K.expected for the four rules it leaves unchecked, K.LAX_149), and
nothing written at or past cap."""
import hashlib

import numpy as np
import pytest

from juicefs_amd import compress as C
from juicefs_amd import device as D
from tests import zstd_conformance_cases as K
from tests.test_zstd_split_gpu import run_device

pytestmark = pytest.mark.gpu


def sha(b):
    return hashlib.sha256(b).hexdigest()


@pytest.fixture(scope="module")
def items(oracle):
    """(case, cap, frame, wanted result, wanted sha) for every case and cap."""
    fx = K.fixture()
    out = []
    for c in K.CASES:
        src, _ = K.built(c)
        for cap in K.caps(c):
            e = fx[(c["name"], cap)]
            assert sha(src) == e["frame_sha"], c["name"]
            out.append((c, cap, src) + K.expected(c, e, oracle))
    return out


def check(part, rets, outs):
    return [(c["name"], cap, r, want) for (c, cap, _, want, wsha), r, o in zip(part, rets, outs)
            if r != want or (r >= 0 and sha(o) != wsha)]


@pytest.mark.parametrize("group", K.GROUPS)
def test_conformance_lone(gpu, items, group):
    """Each case in a call of its own: the small-batch path."""
    D.zstd_split_counts(reset=True)
    bad = []
    part = [it for it in items if it[0]["group"] == group]
    for i, it in enumerate(part):
        r, outs = run_device([it[2]], [it[1]], gpu, src_mis=1 + i % 15, dst_mis=1 + (3 * i) % 15)
        bad += check([it], r, outs)
    print(group, "lone: done/handed", D.zstd_split_counts(), "of", len(part))
    assert not bad, (len(bad), bad[:40])


def test_conformance_batches_of_7(gpu, items):
    """Mixed batches of 7 (small-batch path, several inputs per call)."""
    D.zstd_split_counts(reset=True)
    bad = []
    order = sorted(range(len(items)), key=lambda i: (i * 97) % len(items))  # mixes the groups
    for k in range(0, len(order), 7):
        part = [items[i] for i in order[k:k + 7]]
        r, outs = run_device([p[2] for p in part], [p[1] for p in part], gpu, src_mis=1 + k % 5, dst_mis=2)
        bad += check(part, r, outs)
    print("batches of 7: done/handed", D.zstd_split_counts())
    assert not bad, (len(bad), bad[:40])


def test_conformance_one_wave(gpu, items):
    """Every case once in one batch of more than 128 inputs: the one-wave path."""
    assert len(items) > 128
    D.zstd_split_counts(reset=True)
    r, outs = run_device([p[2] for p in items], [p[1] for p in items], gpu, src_mis=3, dst_mis=5)
    assert D.zstd_split_counts() == (0, 0)
    bad = check(items, r, outs)
    assert not bad, (len(bad), bad[:40])


BLOCK = 4 << 20  # the sources' block size: room for DataDog's size hint of a frame without a content size
CHAIN = ["repeat_after_predefined", "repeat_after_rle", "repeat_after_fse_twice", "mode_of_repeat", "treeless_after_huf",
         "treeless_across_raw_literals", "two_frames", "three_frames", "offset_8191_alone", "offset_8192_alone",
         "offset_8193_alone", "offsets_ml65", "rep_chain_65"]


def test_conformance_read_batch(gpu):
    """Accept cases as stored objects of a full-range read (the chain runner)."""
    cs = [K.BY_NAME[n] for n in CHAIN]
    objs, raws = zip(*[K.built(c) for c in cs])
    seg = [(i, 0, 0, len(r)) for i, r in enumerate(raws)]
    dst = [np.full(len(r) + 32, 0xAB, dtype=np.uint8) for r in raws]
    sres, rres, _ = C.ZStandard().ReadBatch([(o, BLOCK) for o in objs], [d[:len(r)] for d, r in zip(dst, raws)],
                                            (list(range(len(cs) + 1)), seg))
    for c, r, d, s, x in zip(cs, raws, dst, sres, rres):
        assert s == (len(r), None) and x == (len(r), None), (c["name"], s, x)
        assert d[:len(r)].tobytes() == r and (d[len(r):] == 0xAB).all(), c["name"]


def test_conformance_compact_batch(gpu, oracle):
    """The same objects compacted with keep-everything ranges: the re-encoded
    blocks decode (CPU oracle) to the cases' bytes."""
    z = C.ZStandard()
    cs = [K.BY_NAME[n] for n in CHAIN]
    objs, raws = zip(*[K.built(c) for c in cs])
    seg = [(i, 0, 0, len(r)) for i, r in enumerate(raws)]
    outs = [bytearray(z.CompressBound(len(r))) for r in raws]
    sres, ores = z.CompactBatch([(o, BLOCK) for o in objs], outs, (list(range(len(cs) + 1)), seg))
    for c, r, o, s, (n, err) in zip(cs, raws, outs, sres, ores):
        assert s == (len(r), None) and err is None, (c["name"], s, err)
        got, back = oracle.zstd_decompress(bytes(o[:n]), len(r))
        assert got == len(r) and back == r, c["name"]
