"""CPU: the stream builders of tests/split_streams.py decode under the oracle to
the sizes they report, and the host model of the LZ4 fix-up puts them on the
side of the hand-over that tests/test_split_fallback_gpu.py expects."""
import pytest

from tests import split_streams as S


@pytest.fixture(scope="module")
def nonmerging():
    """(nwg, hdr) -> (stream, size), built once"""
    cache = {}

    def get(nwg, hdr):
        if (nwg, hdr) not in cache:
            cache[(nwg, hdr)] = S.nonmerging_stream(nwg, hdr)
        return cache[(nwg, hdr)]
    return get


def test_constants_restate_the_sources():
    import os
    import re
    root = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "juicefs_amd", "csrc")
    hdr = open(os.path.join(root, "jfs_internal.h")).read()
    src = open(os.path.join(root, "lz4_split.hip")).read()
    zs = open(os.path.join(root, "zstd_split.inc")).read()
    om = open(os.path.join(root, "origin_map.h")).read()
    assert int(re.search(r"#define JFS_LZ4_SPLIT_SEG (\d+)", hdr).group(1)) == S.SEG
    assert int(re.search(r"constexpr int FIX_ROUNDS = (\d+);", src).group(1)) == S.FIX_ROUNDS
    # the origin-map constants live in origin_map.h alone; both codecs take them from there
    assert int(re.search(r"constexpr int THREADS = (\d+);", om).group(1)) == S.T
    assert re.search(r"constexpr int T = om::THREADS;", src) and re.search(r"constexpr int ST = om::THREADS;", zs)
    assert int(re.search(r"constexpr int HOPS = (\d+);", om).group(1)) == S.HOPS
    assert int(re.search(r"constexpr int MAX_ROUNDS = (\d+);", om).group(1)) == 12
    assert "jmp[om::MAX_ROUNDS]" in src and "jmp[om::MAX_ROUNDS]" in zs
    assert not re.search(r"constexpr int (HOPS|SJ_HOPS|JUMP_ROUNDS|SJ_ROUNDS)\b", src + zs)


def test_chain_streams_decode(oracle):
    for units in (1, 3, 20000):
        n, _ = oracle.lz4_decompress(S.chain_stream(units), 1 << 20)
        assert n == S.chain_size(units)


def test_nonmerging_streams_decode(oracle, nonmerging):
    for nwg, hdr in ((1, 270), (2, 524), (S.NWG_EDGE, 302), (S.NWG_OVER, 301), (3, 300)):
        s, size = nonmerging(nwg, hdr)
        assert (len(s) + S.SEG - 1) // S.SEG == nwg * S.T  # its last segment is the last lane of workgroup nwg - 1
        assert set(s[3:]) <= set(range(15)) | set(range(16, 31)) | {0xF0}
        assert sum(1 for b in s[3:-18] if b >= 16) == 3 * nwg  # one shifter per span
        for cap in (size, size + 77):
            n, out = oracle.lz4_decompress(s, cap)
            assert n == size, (nwg, hdr, cap, n)
        assert oracle.lz4_decompress(s, size - 1)[0] < 0


def test_fix_rounds_model_finds_the_edge(nonmerging):
    """One round per workgroup boundary while the true chain is not the boundary
    segments' chain: the largest nwg that converges within FIX_ROUNDS and the
    next one up are the pair the GPU test uses."""
    edge = None
    for nwg in range(2, S.FIX_ROUNDS + 4):
        r = S.fix_rounds_needed(nonmerging(nwg, 301)[0])
        assert r == nwg - 1
        if S.converges(r):
            edge = nwg
        else:
            break
    assert (edge, nwg) == (S.NWG_EDGE, S.NWG_OVER)


def test_fix_rounds_of_the_gpu_cases(nonmerging):
    over, edge = nonmerging(S.NWG_OVER, 301)[0], nonmerging(S.NWG_EDGE, 302)[0]
    assert S.fix_rounds_needed(over) >= S.FIX_ROUNDS and not S.converges(S.fix_rounds_needed(over))
    assert S.fix_rounds_needed(edge) <= S.FIX_ROUNDS - 1
    # behind the first block in a batch: the same workgroup alignment, the same count
    assert S.fix_rounds_needed(edge, seg0=S.NWG_OVER * S.T) == S.fix_rounds_needed(edge)
    # two spans more: above FIX_ROUNDS by more than one
    assert S.fix_rounds_needed(nonmerging(S.NWG_OVER + 2, 302)[0]) > S.FIX_ROUNDS
    # the aligned header: the speculative entries are the true ones
    for nwg in (3, S.NWG_OVER + 1):
        assert S.fix_rounds_needed(nonmerging(nwg, 300)[0]) == 0
    # ordinary streams merge at once
    assert S.fix_rounds_needed(S.chain_stream(20000)) <= 1


def test_flat_chain_streams_decode(oracle):
    sizes = [16, 17, 18, 19, 20, 100] + [n for k in (4, 5, 6) for n in S.bound_edge_sizes(k, 4)]
    for nbytes in sizes:
        s = S.flat_chain_stream(nbytes)
        n, out = oracle.lz4_decompress(s, nbytes)
        assert n == nbytes and out[:4] * (S.flat_chain_depth(nbytes) + 1) == out[:4 * S.flat_chain_depth(nbytes) + 4]
    assert max(sizes) < 200_000


def test_bound_edge_sizes_straddle_a_round():
    for unit in (4, 3):
        for k in (4, 5, 6):
            a, b, c = S.bound_edge_sizes(k, unit)
            assert a == max(n for n in range(c - 2 * unit, c + 1) if n / unit + 1 < S.HOPS ** k)
            assert b / unit + 1 == S.HOPS ** k - 1 and c == b + unit
            assert [S.jump_rounds(n, unit) for n in (a, b, c)] == [k, k, k + 1]
    # the deepest chains stay within what the rounds reach
    for k in (4, 5, 6):
        for n in S.bound_edge_sizes(k, 4):
            assert S.flat_chain_depth(n) <= S.HOPS ** S.jump_rounds(n, 4)
        for n in S.bound_edge_sizes(k, 3):
            assert S.zstd_flat_chain_depth(n) <= S.HOPS ** S.jump_rounds(n, 3)


def test_zstd_flat_chain_frames_decode(oracle):
    for nbytes in [6, 7, 8, 100] + S.bound_edge_sizes(4, 3) + S.bound_edge_sizes(6, 3)[2:]:
        f, want = S.zstd_flat_chain_frame(nbytes)
        n, out = oracle.zstd_decompress(f, nbytes)
        assert n == nbytes == len(want) and out == want
        d = S.zstd_flat_chain_depth(nbytes)
        assert want[:3] * (d + 1) == want[:3 * d + 3]
    assert nbytes > S.ZBLOCK  # the largest one spans two blocks


def test_zstd_chain_frames_decode(oracle):
    for units, blocks in ((3, 1), (20000, 2)):
        f, want = S.zstd_chain_frame(units)
        assert len(want) == 11 * units + 10
        n, out = oracle.zstd_decompress(f, len(want))
        assert n == len(want) and out == want
        assert -(-units // 10000) == blocks
