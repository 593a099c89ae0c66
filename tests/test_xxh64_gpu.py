"""GPU: jfs_xxh64_device against the pure-Python XXH64 of tests/xxh64_ref.py
(pinned by tests/test_xxh64_ref.py): every length at which the kernel takes
another path (no stripe, one stripe, the 8-, 4- and 1-byte tail steps, fewer and
more stripes than its prefetch depth, a 128 KiB frame and its neighbours), each
at five source alignments, alone and all in one batch; guard bytes around the
output array; bad descriptors."""
import numpy as np
import pytest
import torch

from juicefs_amd import device as D
from tests.xxh64_ref import xxh64

pytestmark = pytest.mark.gpu
LENGTHS = [0, 1, 3, 4, 7, 8, 15, 31, 32, 33, 63, 64, 95, 96, 127, 4095, 131071, 131072, 131073]
OFFSETS = [0, 1, 3, 5, 7]
GUARD = 0x5A5A5A5A5A5A5A5A
_ref = {}


def data():
    if "buf" not in _ref:
        rng = np.random.default_rng(64)
        _ref["buf"] = rng.integers(0, 256, size=131073 + 16, dtype=np.uint8)
    return _ref["buf"]


def want(off, n):
    if (off, n) not in _ref:
        _ref[(off, n)] = xxh64(data()[off:off + n].tobytes())
    return _ref[(off, n)]


def run(dev, pieces, with_ret=True):
    """pieces = [(offset, length)] of the shared buffer -> (hashes, rets); the
    output array sits between two guard words"""
    src = torch.from_numpy(data()).to(dev)
    n = len(pieces)
    desc = D.make_desc(src, [o for o, _ in pieces], [m for _, m in pieces], src, [0] * n, [0] * n)
    out = torch.full((n + 2,), GUARD, dtype=torch.int64, device=dev)
    ret = torch.full((n + 2,), -77, dtype=torch.int32, device=dev)
    D.xxh64(desc, out[1:], ret[1:] if with_ret else None)
    torch.cuda.synchronize()
    o, r = out.cpu().numpy().view(np.uint64), ret.cpu().tolist()
    assert int(o[0]) == GUARD and int(o[-1]) == GUARD and r[0] == -77 and r[-1] == -77
    assert r[1:-1] == ([0] * n if with_ret else [-77] * n)
    return [int(x) for x in o[1:-1]]


def test_empty_is_the_seed_value(gpu):
    assert run(gpu, [(0, 0)]) == [0xEF46DB3751D8E999]


@pytest.mark.parametrize("off", OFFSETS)
def test_each_length_alone(gpu, off):
    for n in LENGTHS:
        assert run(gpu, [(off, n)], with_ret=n % 2 == 0) == [want(off, n)], (off, n)


def test_one_batch_with_all_of_them(gpu):
    pieces = [(off, n) for n in LENGTHS for off in OFFSETS]  # 95 pieces: six waves, the last one partly filled
    got = run(gpu, pieces)
    for p, g in zip(pieces, got):
        assert g == want(*p), p


def test_bad_descriptors(gpu):
    src = torch.from_numpy(data()).to(gpu)
    a = np.zeros(5, dtype=D.DESC_DTYPE)
    a["src"] = [src.data_ptr(), 0, src.data_ptr() + 1, 0, src.data_ptr()]
    a["src_len"] = [-1, 5, 33, 0, -(1 << 31)]
    desc = torch.from_numpy(a.view(np.uint8).copy()).to(gpu)
    out = torch.full((5,), GUARD, dtype=torch.int64, device=gpu)
    ret = torch.full((5,), -77, dtype=torch.int32, device=gpu)
    D.xxh64(desc, out, ret)
    torch.cuda.synchronize()
    assert ret.cpu().tolist() == [-1, -1, 0, 0, -1]
    assert [int(x) for x in out.cpu().numpy().view(np.uint64)] == [0, 0, want(1, 33), 0xEF46DB3751D8E999, 0]
