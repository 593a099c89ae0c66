"""GPU: the three decode calls on a seek table -- jfs_zstd_decompress_range_device,
_ranges_device and _frames_device -- are one sequence with
three policies, so one range decoded three ways must give one answer: the same
code, the same bytes in the selected frames' spans, the guard pattern everywhere
else.  Hand-built objects of raw frames of 1 to 300 bytes with 1, 64, 65 and 129
frames (the scan works 64 entries a round), both table layouts where the call
takes them; what must be selected comes from the pure-Python plan of
tests/zstd_seek_csum_cases.py."""
import numpy as np
import pytest

from juicefs_amd import device as D
from tests import zstd_seek_cases as S
from tests import zstd_seek_csum_cases as X
from tests.test_zstd_frames_gpu import fetch, run_frames
from tests.test_zstd_ranges_gpu import run_ranges
from tests.test_zstd_seekable_gpu import check_image, run_range

pytestmark = pytest.mark.gpu
COUNTS = [1, 64, 65, 129]
_cache = {}


def built(sizes, checksums):
    """(contents, object, table, content edges, frame edges) of raw frames of the given sizes"""
    key = (tuple(sizes), checksums)
    if key not in _cache:
        rnd = np.random.RandomState(len(sizes) * 1000 + sum(sizes) % 997)
        contents = [rnd.bytes(m) for m in sizes]
        obj, t, ent = X.build(contents, checksums)
        d0 = [sum(e[1] for e in ent[:k]) for k in range(len(ent) + 1)]
        c0 = [sum(e[0] for e in ent[:k]) for k in range(len(ent) + 1)]
        _cache[key] = (contents, obj, t, d0, c0)
    return _cache[key]


def sizes_of(nf):
    return [1 + (k * 37) % 300 for k in range(nf)]


def ranges_of(nf, d0):
    """first selected frame at entry 63, 64 and 128; a run from entry 60 to 70; the whole object"""
    out = [(0, d0[nf]), (d0[nf] - 1, d0[nf])]
    for k in (63, 64, 128):
        if k < nf:
            out += [(d0[k], d0[k] + 1), (d0[k], d0[nf])]
    if nf > 60:
        out.append((d0[60], d0[min(70, nf - 1) + 1]))
    return out


def three_ways(dev, cases, with_range):
    """cases = [(object, table, raw, cap, lo, hi)] -> the rets of the range (or None), ranges and fragment calls,
    every image checked against the plan: the content in [flo, fhi) of the selected run, guard elsewhere"""
    plans = [X.plan(t, len(obj), lo, hi, cap) for obj, t, _, cap, lo, hi in cases]
    writes = [(i, p["flo"], c[2][p["flo"]:p["fhi"]]) for i, (c, p) in enumerate(zip(cases, plans))]
    out = []
    if with_range:
        rets, img, do = run_range(dev, [c[0] for c in cases], [c[3] for c in cases], [c[4] for c in cases],
                                  [c[5] for c in cases])
        check_image(img, do, writes)
        out.append(rets)
    else:
        out.append(None)
    rets, img, do, counts = run_ranges(dev, [(c[0], c[3], [(c[4], c[5])]) for c in cases])
    check_image(img, do, writes)
    out.append(rets)
    items = []
    for obj, t, _, cap, lo, hi in cases:
        t2, frag, off, _ = fetch(obj, 9, lo, hi)
        assert t2 == t
        items.append((t, len(obj), frag, off, cap, lo, hi))
    rets, img, do = run_frames(dev, items)
    check_image(img, do, writes)
    out.append(rets)
    return out, counts


@pytest.mark.parametrize("checksums", [False, True])
def test_three_calls_agree(gpu, checksums):
    cases = []
    for nf in COUNTS:
        contents, obj, t, d0, _ = built(sizes_of(nf), checksums)
        raw = b"".join(contents)
        cases += [(obj, t, raw, d0[nf] + 3, lo, hi) for lo, hi in ranges_of(nf, d0)]
    assert len(cases) == 2 + 5 + 7 + 9
    want = [min(len(c[2]), c[5], c[3]) for c in cases]
    (r_range, r_ranges, r_frames), _ = three_ways(gpu, cases, with_range=not checksums)
    assert r_ranges == want and r_frames == want
    assert r_range is None or r_range == want


def test_contentless_frames(gpu):
    # frames 1 and 3 have no content and lie inside the run of frames 0..4
    contents, obj, t, d0, c0 = built([100, 0, 200, 0, 50, 7], False)
    raw = b"".join(contents)
    cases = [(obj, t, raw, d0[6], 0, d0[5]), (obj, t, raw, d0[6], d0[2] - 1, d0[4] + 1), (obj, t, raw, d0[6], 0, d0[6])]
    rets, _ = three_ways(gpu, cases, with_range=True)
    assert rets[0] == rets[1] == rets[2] == [d0[5], d0[4] + 1, d0[6]]
    # The last frame has no content and the fragment stops in front of it.  With hi' <= D that frame starts at
    # D >= hi', so it is behind the range (frame_from) and the answer is D.  With dst_cap > D and hi > D it starts
    # inside [lo', hi'), so it is the run's last frame (frame_in_run: a frame without content is only ever "before"
    # or "from" by where it starts); its bytes end behind the fragment: -3.  The whole body decodes: D.
    for wide in (False, True):
        contents, obj, t, d0, c0 = built([100, 200, 0], wide)
        raw, n, body = b"".join(contents), d0[3], obj[:c0[3]]
        assert n == 300 and c0[3] > c0[2]
        items = [(t, len(obj), body[:c0[2]], 0, n, 0, n), (t, len(obj), body[:c0[2]], 0, n + 100, 0, n + 50),
                 (t, len(obj), body, 0, n + 100, 0, n + 50)]
        rets, img, do = run_frames(gpu, items)
        assert rets == [300, -3, 300]
        check_image(img, do, [(0, 0, raw), (2, 0, raw)])
        rets, img, do, _ = run_ranges(gpu, [(obj, n + 100, [(0, n + 50)])])
        assert rets == [300]
        check_image(img, do, [(0, 0, raw)])


def test_only_the_ranges_call_moves_the_counters(gpu):
    contents, obj, t, d0, _ = built(sizes_of(65), True)
    _, obj8, t8, _, _ = built(sizes_of(65), False)
    n = d0[65]
    D.zstd_sparse_counts(reset=True)
    rets, _, _ = run_range(gpu, [obj8, obj8], [n, n], [0, d0[63]], [n, d0[64] + 1])
    assert rets == [n, d0[64] + 1]
    items = []
    for o, tt in ((obj, t), (obj8, t8)):
        t2, frag, off, _ = fetch(o, 9, d0[60], n)
        items.append((tt, len(o), frag, off, n, d0[60], n))
    rets, _, _ = run_frames(gpu, items)
    assert rets == [n, n]
    assert D.zstd_sparse_counts() == (0, 0, 0)
    # frames 63 and 64 of the 12-byte object (compared), all 65 of the 8-byte one (not compared)
    rets, _, _, counts = run_ranges(gpu, [(obj, n, [(d0[63], d0[64] + 1)]), (obj8, n, [(0, n)])])
    assert rets == [d0[64] + 1, n] and counts == (2, 67, 2)


def test_a_batch_mixing_kinds_through_the_range_call(gpu):
    """an object with a table, one with a checksummed table and a plain frame (both passed through), an empty input"""
    contents, obj8, _, d0, _ = built(sizes_of(65), False)
    _, obj12, _, _, _ = built(sizes_of(65), True)
    plain = S.raw_frame(contents[7])
    n = d0[65]
    objs, caps = [obj8, obj12, plain, b""], [n, n, len(contents[7]), 16]
    los, his = [d0[63], 5, 0, 0], [d0[64] + 1, d0[10], len(contents[7]), 16]
    alone = [run_range(gpu, [o], [c], [lo], [hi]) for o, c, lo, hi in zip(objs, caps, los, his)]
    check_image(alone[0][1], alone[0][2], [(0, d0[63], b"".join(contents)[d0[63]:d0[65]])])
    rets, img, do = run_range(gpu, objs, caps, los, his)
    assert rets == [a[0][0] for a in alone]
    assert rets[0] == d0[64] + 1 and rets[2] == len(contents[7])
    assert img[do[2]:do[2] + rets[2]].tobytes() == contents[7]
    # a passed-through input is a prefix decode: dst[0, ret) is the content, dst[ret, dst_cap) is unspecified
    for i in (1, 2):
        assert rets[i] > 0
        assert img[do[i]:do[i] + rets[i]].tobytes() == alone[i][1][alone[i][2][0]:alone[i][2][0] + rets[i]].tobytes(), i
    assert img[do[1]:do[1] + rets[1]].tobytes() == b"".join(contents)[:rets[1]]
    a = alone[0]
    check_image(img, do, [(0, 0, a[1][a[2][0]:a[2][0] + n].tobytes())] +
                [(i, 0, img[do[i]:do[i] + caps[i]].tobytes()) for i in (1, 2, 3)])
