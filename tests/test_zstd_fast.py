"""The fast Zstd encoder without a GPU: its host twin
(jfs_test_zstd_fast_host_seqs, the two kernels' parse restated in host C++),
the parse-mode calls and the new symbols.  JFS_ZSTD_PARSE is matched
case-insensitively: "fast" / "FAST" / "bogus" give fast / fast / exact."""
import os
import subprocess
import sys

import numpy as np
import pytest

from juicefs_amd import _lib as L
from juicefs_amd import compress as C
from tests import zstd_fast_cases as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name,src", K.cases(), ids=[c[0] for c in K.cases()])
def test_twin_replays_to_the_input(lib, name, src):
    blocks = C.zstd_fast_seqs(src)
    K.replay(src, blocks)  # the input again, counts, chunk rule, repeat rule
    for (recs, nl), bsz in zip(blocks, K.block_sizes(len(src))):
        assert sum(ll + ml for ll, ml, _ in recs) + (nl - sum(ll for ll, _, _ in recs)) == bsz
        if bsz < 7:
            assert (recs, nl) == ([], bsz)
    assert C.zstd_fast_seqs(src) == blocks  # deterministic


@pytest.mark.parametrize("name", ["T-13", "T-65537", "period3", "match-ends-chunk", "rep-across-blocks"])
def test_twin_ignores_the_address(lib, name):
    src = dict(K.cases())[name]
    want = C.zstd_fast_seqs(src)
    n = len(src)
    nb = len(K.block_sizes(n))
    for shift in range(4):
        buf = np.full(n + 8, 0xA5, dtype=np.uint8)
        buf[shift:shift + n] = np.frombuffer(src, dtype=np.uint8)
        out = np.zeros(n // 4 + 4 * nb + 4, dtype=np.uint64)
        ns, nl = np.zeros(nb, dtype=np.int32), np.zeros(nb, dtype=np.int32)
        total = lib.jfs_test_zstd_fast_host_seqs(buf.ctypes.data + shift, n, out.ctypes.data, len(out), ns.ctypes.data,
                                                 nl.ctypes.data)
        flat = [x for recs, _ in want for x in recs]
        assert total == len(flat) and ns.tolist() == [len(r) for r, _ in want] and nl.tolist() == [x for _, x in want]
        assert [(int(x) & 0x1FFFF, ((int(x) >> 17) & 0x1FFFF) + 3, int(x) >> 34) for x in out[:total]] == flat


def test_twin_refuses_bad_arguments(lib):
    out = np.zeros(8, dtype=np.uint64)
    ns, nl = np.full(4, -7, dtype=np.int32), np.full(4, -7, dtype=np.int32)
    src = dict(K.cases())["T-65537"]
    args = (out.ctypes.data, ns.ctypes.data, nl.ctypes.data)
    assert lib.jfs_test_zstd_fast_host_seqs(src, -1, args[0], 8, args[1], args[2]) == -1
    assert lib.jfs_test_zstd_fast_host_seqs(src, 0x7FFFFF01, args[0], 8, args[1], args[2]) == -1
    assert lib.jfs_test_zstd_fast_host_seqs(src, len(src), args[0], 8, args[1], args[2]) == -1  # cap too small
    assert not out.any() and (ns == -7).all() and (nl == -7).all()


def test_special_cases_do_what_their_names_say():
    d = dict(K.cases())
    # a literal run of more than 270 bytes across the chunk boundary
    (recs, nl), = C.zstd_fast_seqs(d["lits-cross-chunk"])
    pos, crossing = 0, []
    for ll, ml, _ in recs:
        if pos < K.CHUNK < pos + ll:
            crossing.append(ll)
        pos += ll + ml
    assert crossing and crossing[0] > 270
    # a match longer than a lane extends alone
    (recs, nl), = C.zstd_fast_seqs(d["match-cross-tile"])
    assert recs == [(100 + 300 + 50, 300, 350 + 3)]
    # a match that ends at the chunk's last byte
    (recs, nl), = C.zstd_fast_seqs(d["match-ends-chunk"])
    pos, ends = 0, []
    for ll, ml, _ in recs:
        pos += ll + ml
        ends.append(pos)
    assert K.CHUNK in ends
    # zeros: one match per chunk, each reaching its chunk's end
    for k, (recs, nl) in enumerate(C.zstd_fast_seqs(d["zeros-262144"])):
        # block 0 knows offset 1 from the frame's start values; block 1 learns it from its first match
        assert recs == ([(1, 65535, 1), (1, 65535, 1)] if k == 0 else [(1, 65535, 4), (1, 65535, 1)]) and nl == 2
    # random bytes: no sequence at all
    assert C.zstd_fast_seqs(d["R-65537"]) == [([], 65536), ([], 1)] or \
        all(len(r) < 8 for r, _ in C.zstd_fast_seqs(d["R-65537"]))


def test_repeat_codes_without_literals():
    src = dict(K.cases())["rep-no-literals"]
    blocks = C.zstd_fast_seqs(src)
    used = K.replay(src, blocks)
    (recs, nl), = blocks
    # u at its offset, w without a literal, v without a literal at u's offset
    # again: "repeat 2" is Offset_Value 1 when there is no literal
    assert recs == [(296, 40, 296 + 3), (0, 8, 148 + 3), (0, 40, 1)]
    assert used == [(0, 0, 1)]


def test_repeat_codes_stay_inside_their_block():
    src = dict(K.cases())["rep-across-blocks"]
    blocks = C.zstd_fast_seqs(src)
    K.replay(src, blocks)
    # block 0: chunk 0 learns offset 1000, chunk 1 repeats it after its literals
    # (one long match per chunk; where it starts depends on hash collisions)
    assert [ofv for _, _, ofv in blocks[0][0]] == [1003, 1]
    assert all(ll >= 1000 and ll + ml == K.CHUNK for ll, ml, _ in blocks[0][0])
    # block 1 starts with nothing known: the same offset is coded raw
    assert [ofv for _, _, ofv in blocks[1][0]] == [1003]


def test_replay_catches_a_repeat_code_across_blocks():
    # the checker itself: block 1 naming an entry only block 0 determined is refused
    src = dict(K.cases())["rep-across-blocks"]
    blocks = C.zstd_fast_seqs(src)
    bad = [blocks[0], ([(1000, 4000, 1)], blocks[1][1])]
    with pytest.raises(AssertionError, match="undetermined"):
        K.replay(src, bad)


def test_parse_mode_calls(lib):
    assert lib.jfs_zstd_parse_mode() == L.ZSTD_PARSE_EXACT  # the default
    assert lib.jfs_set_zstd_parse_mode(2) == -1
    assert lib.jfs_set_zstd_parse_mode(-1) == -1
    assert lib.jfs_zstd_parse_mode() == L.ZSTD_PARSE_EXACT
    try:
        assert lib.jfs_set_zstd_parse_mode(L.ZSTD_PARSE_FAST) == L.ZSTD_PARSE_EXACT
        assert lib.jfs_zstd_parse_mode() == L.ZSTD_PARSE_FAST
        assert lib.jfs_lz4_parse_mode() == L.LZ4_PARSE_EXACT  # the two modes are separate
    finally:
        assert lib.jfs_set_zstd_parse_mode(L.ZSTD_PARSE_EXACT) == L.ZSTD_PARSE_FAST
    assert lib.jfs_zstd_parse_mode() == L.ZSTD_PARSE_EXACT


def test_parse_mode_context_manager_restores(lib):
    with pytest.raises(RuntimeError):
        with C.zstd_parse_mode("fast"):
            assert lib.jfs_zstd_parse_mode() == L.ZSTD_PARSE_FAST
            with C.zstd_parse_mode("exact"):
                assert lib.jfs_zstd_parse_mode() == L.ZSTD_PARSE_EXACT
            assert lib.jfs_zstd_parse_mode() == L.ZSTD_PARSE_FAST
            raise RuntimeError("leave by exception")
    assert lib.jfs_zstd_parse_mode() == L.ZSTD_PARSE_EXACT
    with pytest.raises(ValueError):
        with C.zstd_parse_mode("faster"):
            pass


def _child(env_extra, code):
    env = dict(os.environ)
    env.pop("JFS_ZSTD_PARSE", None)
    env.update(env_extra)
    r = subprocess.run([sys.executable, "-c", code], env=env, cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    return [int(x) for x in r.stdout.split()]


def test_parse_mode_env():
    code = "from juicefs_amd import _lib as L; print(L.load().jfs_zstd_parse_mode())"
    assert _child({}, code) == [L.ZSTD_PARSE_EXACT]
    assert _child({"JFS_ZSTD_PARSE": "fast"}, code) == [L.ZSTD_PARSE_FAST]
    assert _child({"JFS_ZSTD_PARSE": "FAST"}, code) == [L.ZSTD_PARSE_FAST]
    assert _child({"JFS_ZSTD_PARSE": "exact"}, code) == [L.ZSTD_PARSE_EXACT]
    assert _child({"JFS_ZSTD_PARSE": "bogus"}, code) == [L.ZSTD_PARSE_EXACT]


def test_fast_device_call_without_device():
    # JFS_GPU_CODEC=off: the library reports no device, with or without a GPU in the machine
    code = ("from juicefs_amd import _lib as L; lib = L.load(); "
            "print(lib.jfs_zstd_compress_fast_device(None, 1, None, None))")
    assert _child({"JFS_GPU_CODEC": "off"}, code) == [L.JFS_ERR_NO_DEVICE]


def test_new_symbols_exported(lib):
    for name in ("jfs_zstd_compress_fast_device", "jfs_zstd_parse_mode", "jfs_set_zstd_parse_mode"):
        assert name in L.EXPORTS and hasattr(lib, name), name
    # the hooks have a header of their own, outside the public ABI
    inc = os.path.join(ROOT, "include")
    hook_h = open(os.path.join(inc, "jfs_gpucodec_zstd_fast_test.h")).read()
    pub_h = open(os.path.join(inc, "jfs_gpucodec.h")).read()
    assert L.ZSTD_FAST_TEST_EXPORTS == ["jfs_test_zstd_fast_host_seqs", "jfs_test_zstd_fast_seqs_device"]
    for name in L.ZSTD_FAST_TEST_EXPORTS:
        assert hasattr(lib, name) and name not in L.EXPORTS
        assert name + "(" in hook_h and name not in pub_h
