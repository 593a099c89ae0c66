"""GPU: the Zstd level-1 encoder on the directed edge inputs (tests/zstd_l1_edges.py):
one input per output decision of libzstd that the frame census
(tests/zstd_frame_census.py) can name -- every literals format and header tier,
every sequence-table mode libzstd can choose, the sequence-count forms, the long
lengths, far offsets, the frame-header tiers.  The bar is
tests/golden/zstd_l1_edges.json, the sha256 of libzstd 1.4.9's own frames:

  a. all cases in one launch, misaligned source and destination;
  b. the reverse order with other misalignments: the same bytes;
  c. every block cut into 1, 4 and 16 segments (JFS_ZL1_SEGS): the same bytes;
  d. the frame-serial parse (a batch of more than JFS_ZL1_SPEC_MAX blocks): the same bytes;
  e. the GPU decoder and the oracle decoder return the inputs from the frames of (a);
  f. the fast and the seekable parse in front of the same entropy stage: every object
     decodes to its input through the oracle, libzstd and the GPU decoder, and the
     fast parse's kernels equal their host twin record for record.
Every comparison is equality of bytes or of hashes."""
import hashlib
import json
import os

import numpy as np
import pytest
import torch

from juicefs_amd import compress as C
from juicefs_amd import device as D
from tests import zstd_l1_edges as E
from tests.test_zstd_encode_gpu import encode_device

pytestmark = pytest.mark.gpu


def _sha(b):
    return hashlib.sha256(b).hexdigest()


def _fixture():
    with open(os.path.join(os.path.dirname(__file__), "golden", "zstd_l1_edges.json")) as f:
        return json.load(f)["cases"]


@pytest.fixture(scope="module")
def first(gpu):
    """(a): (fixture cases, inputs, rets, frames) of one launch over every case"""
    cs = _fixture()
    assert [c["name"] for c in cs] == list(E.CASES)
    srcs = [E.make(c["name"]) for c in cs]
    r, frames = encode_device(srcs, gpu, src_mis=3, dst_mis=5)
    return cs, srcs, r, frames


def _same(first, r, frames, what):
    cs, _, r0, f0 = first
    bad = [c["name"] for c, x, f, x0, g in zip(cs, r, frames, r0, f0) if x != x0 or f != g]
    assert not bad, (what, bad)


def test_edges_equal_libzstd(first):
    cs, srcs, r, frames = first
    bad = [(c["name"], x, c["csize"]) for c, x, f in zip(cs, r, frames) if x != c["csize"] or _sha(f) != c["comp_sha"]]
    assert not bad, bad


def test_edges_reverse_order_other_alignment(gpu, first):
    cs, srcs, _, _ = first
    r, frames = encode_device(srcs[::-1], gpu, src_mis=9, dst_mis=14)
    _same(first, r[::-1], frames[::-1], "reverse order")


@pytest.mark.parametrize("segs", [1, 4, 16])
def test_edges_segment_parse(gpu, first, monkeypatch, segs):
    monkeypatch.setenv("JFS_ZL1_SEGS", str(segs))
    cs, srcs, _, _ = first
    r, frames = encode_device(srcs, gpu, src_mis=1, dst_mis=2)
    _same(first, r, frames, "JFS_ZL1_SEGS=%d" % segs)


def test_edges_frame_serial(gpu, first):
    """behind 64 frames of 32 blocks: more than JFS_ZL1_SPEC_MAX (2,048) blocks in the batch"""
    from tests.zstd_l1_cases import make_case
    g = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "zstd_l1_golden.json")))
    big = [c for c in g["cases"] if c["kind"] == "T" and c["size"] == 4 << 20][0]
    pad = make_case(big["kind"], big["seed"], big["size"])
    cs, srcs, _, _ = first
    batch = srcs + [pad] * 64
    assert sum((len(x) + (128 << 10) - 1) // (128 << 10) for x in batch) > 2048
    r, frames = encode_device(batch, gpu, src_mis=1, dst_mis=4)
    _same(first, r[:len(srcs)], frames[:len(srcs)], "frame-serial parse")
    assert r[-1] == big["csize"] and _sha(frames[-1]) == big["comp_sha"]


def test_edges_decode_back(gpu, oracle, first):
    from tests.test_zstd_gpu import run_device
    cs, srcs, r, frames = first
    for c, s, f in zip(cs, srcs, frames):
        n, out = oracle.zstd_decompress(f, len(s))
        assert n == len(s) and out == s, c["name"]
    r2, outs = run_device(frames, [len(s) for s in srcs], gpu, src_mis=5, dst_mis=3)
    bad = [c["name"] for c, s, x, o in zip(cs, srcs, r2, outs) if x != len(s) or o != s]
    assert not bad, bad


@pytest.mark.parametrize("seekable", [False, True], ids=["fast", "seekable"])
def test_edges_fast_and_seekable_objects(gpu, oracle, first, seekable):
    """the entropy stage behind the other two parses: other sequences, the same writers"""
    from tests.test_zstd_fast_gpu import _libzstd_decode
    from tests.test_zstd_gpu import run_device
    from tests.test_zstd_seekable_gpu import encode, intact
    cs, srcs, _, _ = first
    caps = [D.zstd_bound(len(s)) for s in srcs]
    r, objs, got, doffs = encode(gpu, srcs, caps, seekable=seekable)
    assert all(0 < x <= c for x, c in zip(r, caps)), r
    assert intact(got, doffs, objs), "a byte outside dst[0, ret) was written"
    for c, s, o in zip(cs, srcs, objs):
        n, out = oracle.zstd_decompress(o, len(s))
        assert n == len(s) and out == s, c["name"]
        back = _libzstd_decode(o, len(s))
        assert back is None or back == s, c["name"]
    r2, outs = run_device(objs, [len(s) for s in srcs], gpu, src_mis=3, dst_mis=5)
    bad = [c["name"] for c, s, x, o in zip(cs, srcs, r2, outs) if x != len(s) or o != s]
    assert not bad, bad


def test_edges_fast_kernels_equal_twin(gpu, first):
    """every case in one device buffer, each at its own (odd) address"""
    cs, srcs, _, _ = first
    offs, o = [], 1
    for s in srcs:
        offs.append(o)
        o += len(s) + (3 if len(s) % 2 else 2)
    h = np.full(o + 16, 0xA5, dtype=np.uint8)
    for s, a in zip(srcs, offs):
        h[a:a + len(s)] = np.frombuffer(s, dtype=np.uint8)
    d = torch.from_numpy(h).to(gpu)
    bad = [c["name"] for c, s, a in zip(cs, srcs, offs)
           if C.zstd_fast_seqs(s, device_ptr=d.data_ptr() + a) != C.zstd_fast_seqs(s)]
    assert not bad, bad
