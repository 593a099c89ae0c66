"""GPU: the LZ4 lift.  jfs_lz4_compress_fast_lift_device against
jfs_lz4_compress_fast_device on the same gathered blocks -- the feature's exact
oracle is the project's own path without it: d_ret and every byte of the
canary-filled destination are equal, d_lifted is the planned count, and the
blocks decode to the gathered bytes.  Then the compaction calls with
JFS_COMPACT_LZ4_LIFT on against off, and the counters."""
import numpy as np
import pytest
import torch

from juicefs_amd import _lib as L
from juicefs_amd import compress as C
from juicefs_amd import device as D
from juicefs_amd import encrypt as E
from juicefs_amd.blockgen import gen_block
from tests import lz4_chase_cases as K

pytestmark = pytest.mark.gpu
CANARY = 0xA5
CH = 65536
N = 300000  # four whole chunks and a ragged fifth
NCH = 5
# where each output's 4 KiB piece is replaced: at a chunk's start, at a chunk's end, across a boundary, in the ragged tail
CUTS = [CH, 2 * CH - 4096, 2 * CH - 2048, 4 * CH + 1000]
PLANNED = [3, 3, 2, 4]


def interior(c, n):
    return (c + 1) * CH + 12 <= n


@pytest.fixture(scope="module")
def raws():
    return [gen_block("T", 30 + i, N) for i in range(4)]


@pytest.fixture(scope="module")
def fast_streams(raws):
    return [C.lz4_fast_host(r) for r in raws]  # (the device's bytes: tests/test_lz4_fast_gpu.py pins the twin)


def overwritten(raws):
    """the four gathered outputs and their candidates [(src, src_chunk)] per chunk"""
    outs, lift = [], []
    for k, cut in enumerate(CUTS):
        other = raws[(k + 1) % 4]
        outs.append(raws[k][:cut] + other[cut:cut + 4096] + raws[k][cut + 4096:])
        touched = {cut // CH, (cut + 4095) // CH}
        lift.append([(k, j) if interior(j, N) and j not in touched else (-1, 0) for j in range(NCH)])
    assert [sum(s >= 0 for s, _ in l) for l in lift] == PLANNED
    return outs, lift


def pack(dev, blobs, pad=3):
    """blobs at odd offsets inside one canary-filled tensor -> (tensor, offsets)"""
    offs, o = [], 1
    for b in blobs:
        offs.append(o)
        o += len(b) + (pad if len(b) % 2 else pad - 1)
    h = np.full(o + 16, CANARY, dtype=np.uint8)
    for b, at in zip(blobs, offs):
        h[at:at + len(b)] = np.frombuffer(b, dtype=np.uint8)
    return torch.from_numpy(h).to(dev), offs


def run_lift(dev, streams, outs, lift, caps=None, src_cap=N):
    """decode the streams on the device, then both encoders over `outs`; returns (ret, dst) of the plain fast
    encoder, (ret, dst) of the lift call, the lifted counts and the decodes' results.  src_cap: the sources' decode
    capacity, one for all or one each"""
    scaps = list(src_cap) if isinstance(src_cap, (list, tuple)) else [src_cap] * len(streams)
    pitch = max(scaps) + 16
    ddec = torch.full((len(streams) * pitch,), CANARY, dtype=torch.uint8, device=dev)
    dstream, soffs = pack(dev, streams)
    sdesc = D.make_desc(dstream, soffs, [len(s) for s in streams], ddec, [i * pitch for i in range(len(streams))], scaps)
    src_n = torch.full((len(streams),), -9, dtype=torch.int32, device=dev)
    D.lz4_decompress(sdesc, src_n)
    dgat, goffs = pack(dev, outs)
    caps = [D.lz4_bound(len(o)) for o in outs] if caps is None else caps
    doffs, o = [], 3
    for c in caps:
        doffs.append(o)
        o += c + (3 if c % 2 else 2)
    flat = np.array([x for l in lift for x in l], dtype=D.LIFT_DTYPE)
    dlift = torch.from_numpy(flat.view(np.uint8).copy()).to(dev)
    res = []
    for lifted in (None, torch.full((len(outs),), -5, dtype=torch.int32, device=dev)):
        ddst = torch.full((o + 16,), CANARY, dtype=torch.uint8, device=dev)
        desc = D.make_desc(dgat, goffs, [len(x) for x in outs], ddst, doffs, caps)
        ret = torch.full((len(outs),), -7, dtype=torch.int32, device=dev)
        if lifted is None:
            D.lz4_compress_fast(desc, ret, [len(x) for x in outs])
        else:
            D.lz4_compress_fast_lift(desc, ret, [len(x) for x in outs], dlift, sdesc, src_n, [len(s) for s in streams],
                                     scaps, lifted)
        torch.cuda.synchronize()
        res.append((ret.cpu().tolist(), ddst.cpu().numpy()))
    return res[0], res[1], lifted.cpu().tolist(), src_n.cpu().tolist(), doffs


def same_bytes(plain, lift):
    assert lift[0] == plain[0]
    if not np.array_equal(plain[1], lift[1]):
        pytest.fail(f"first difference at dst byte {int(np.flatnonzero(plain[1] != lift[1])[0])}")


@pytest.mark.parametrize("group", [0, 7], ids=["one-group", "groups-of-7-chunks"])
def test_device_call_equals_fast_encode(gpu, oracle, raws, fast_streams, group):
    """group 7: one block per launch group, so the flat candidate array is offset per group"""
    outs, lift = overwritten(raws)
    lib = L.load()
    prev = lib.jfs_test_set_lz4_fast_group_chunks(group)
    try:
        plain, lifted_run, lifted, src_n, doffs = run_lift(gpu, fast_streams, outs, lift)
    finally:
        lib.jfs_test_set_lz4_fast_group_chunks(prev)
    assert src_n == [N] * 4
    same_bytes(plain, lifted_run)
    assert lifted == PLANNED
    for r, at, o in zip(lifted_run[0], doffs, outs):
        assert r > 0 and oracle.lz4_decompress(lifted_run[1][at:at + r].tobytes(), len(o))[1] == o


def test_moved_chunk(gpu, oracle, raws, fast_streams):
    out = raws[0][2 * CH:3 * CH] + raws[0][:CH] + raws[1][2 * CH:2 * CH + 5000]
    plain, lifted_run, lifted, _, doffs = run_lift(gpu, fast_streams, [out], [[(0, 2), (0, 0), (-1, 0)]])
    same_bytes(plain, lifted_run)
    assert lifted == [2]
    r = lifted_run[0][0]
    assert oracle.lz4_decompress(lifted_run[1][doffs[0]:doffs[0] + r].tobytes(), len(out))[1] == out


def py_liftable(stream, i):
    """lz4_lift.h's rule, restated over tests/lz4_chase_cases.sequences"""
    F, Eend, op, total = i * CH, (i + 1) * CH, 0, 0
    ok = True
    for ll, _, ml, off in K.sequences(stream):
        m = op + ll
        if ml and m + ml > F and m < Eend and (m < F or m + ml > Eend or m - off < F):
            ok = False
        op = m + ml
    return ok and interior(i, op)


def test_exact_encoder_sources(gpu, oracle, raws):
    """liblz4's parse matches across chunk boundaries: the device refuses what the rule refuses.  (Chunk 0 of such a
    block is liftable when no match happens to straddle its end; what is lifted then is a valid block all the same,
    and a block with nothing lifted is the fast encoder's byte for byte.)"""
    dsrc, soffs = pack(gpu, raws)
    caps = [D.lz4_bound(N)] * 4
    ddst = torch.zeros(4 * (caps[0] + 16), dtype=torch.uint8, device=gpu)
    ret = torch.zeros(4, dtype=torch.int32, device=gpu)
    D.lz4_compress(D.make_desc(dsrc, soffs, [N] * 4, ddst, [i * (caps[0] + 16) for i in range(4)], caps), ret)
    torch.cuda.synchronize()
    streams = [ddst[i * (caps[0] + 16):i * (caps[0] + 16) + r].cpu().numpy().tobytes() for i, r in enumerate(ret.cpu().tolist())]
    outs, lift = overwritten(raws)
    plain, lifted_run, lifted, src_n, doffs = run_lift(gpu, streams, outs, lift)
    assert src_n == [N] * 4
    want = [sum(py_liftable(streams[s], c) for s, c in l if s >= 0) for l in lift]
    assert lifted == want
    assert sum(PLANNED) - sum(lifted) >= 8  # (chunks 1 to 3 copy from below their floor)
    if sum(want) == 0:
        same_bytes(plain, lifted_run)
    for k, (r, at, o) in enumerate(zip(lifted_run[0], doffs, outs)):
        assert r > 0 and oracle.lz4_decompress(lifted_run[1][at:at + r].tobytes(), len(o))[1] == o
        if want[k] == 0:
            assert r == plain[0][k] and np.array_equal(lifted_run[1][at - 2:at + r + 2], plain[1][at - 2:at + r + 2])


def test_bad_candidates_are_parsed(gpu, raws, fast_streams):
    """src out of range, a negative chunk, a chunk past the source's end, a source that failed to decode: each
    chunk is parsed, and not a byte outside dst[0, ret) is written (the canaries are compared too)"""
    broken = bytearray(fast_streams[3])
    ll, lit, _, _ = K.sequences(fast_streams[3])[0]
    broken[lit + ll:lit + ll + 2] = b"\xff\xff"  # the first match copies from far in front of the block
    streams = fast_streams[:3] + [bytes(broken)]
    outs = list(raws)
    lift = [[(9, j) for j in range(NCH)], [(1, -1)] * NCH, [(2, 100 + j) for j in range(NCH)], [(3, j) for j in range(NCH)]]
    plain, lifted_run, lifted, src_n, _ = run_lift(gpu, streams, outs, lift)
    assert src_n[:3] == [N] * 3 and src_n[3] < 0
    same_bytes(plain, lifted_run)
    assert lifted == [0, 0, 0, 0]
    assert plain[0] == [len(s) for s in fast_streams]


def test_does_not_fit(gpu, raws, fast_streams):
    lift = [[(0, j) if interior(j, N) else (-1, 0) for j in range(NCH)]]
    plain, lifted_run, lifted, _, _ = run_lift(gpu, fast_streams, [raws[0]], lift, caps=[len(fast_streams[0]) - 1])
    assert lifted_run[0] == [0] and plain[0] == [0] and lifted == [4]
    assert (lifted_run[1] == CANARY).all()
    _, fits, lifted, _, doffs = run_lift(gpu, fast_streams, [raws[0]], lift, caps=[len(fast_streams[0])])
    assert fits[0] == [len(fast_streams[0])] and lifted == [4]
    assert fits[1][doffs[0]:doffs[0] + fits[0][0]].tobytes() == fast_streams[0]


Z = C.NewCompressor("lz4")


def overwrite_plan(shift=0):
    """output k: source k with 4 KiB at CUTS[k] taken from source k + 1 (shift: every segment reads `shift` bytes on)"""
    seg_first, seg = [0], []
    for k, cut in enumerate(CUTS):
        n = N - shift
        seg += [(k, shift, 0, cut), ((k + 1) % 4, cut + shift, cut, 4096), (k, cut + 4096 + shift, cut + 4096, n - cut - 4096)]
        seg_first.append(len(seg))
    return seg_first, seg


def store(raws):
    dsts = [bytearray(Z.CompressBound(len(r))) for r in raws]
    res = Z.CompressBatch([(d, r) for d, r in zip(dsts, raws)])
    assert all(e is None for _, e in res), res
    return [bytes(d[:n]) for d, (n, _) in zip(dsts, res)]


def compact(objs, plan):
    totals = [sum(s[3] for s in plan[1][plan[0][j]:plan[0][j + 1]]) for j in range(len(plan[0]) - 1)]
    outs = [bytearray(Z.CompressBound(t)) for t in totals]
    sres, ores, crcs = Z.CompactBatch([(o, N) for o in objs], outs, plan, with_crc=True)
    assert all(e is None for _, e in sres) and all(e is None for _, e in ores), (sres, ores)
    return [n for n, _ in ores], [bytes(o[:n]) for o, (n, _) in zip(outs, ores)], crcs


@pytest.fixture
def switch(gpu):
    prev = C.set_compact_lz4_lift_mode("off")
    C.compact_lz4_lift_counts(reset=True)
    yield
    C.set_compact_lz4_lift_mode(prev)
    C.compact_lz4_lift_counts(reset=True)


def test_compact_batch_on_equals_off(switch, oracle, raws, fast_streams):
    with C.lz4_parse_mode("fast"):
        objs = store(raws)
        assert objs == fast_streams
        off = compact(objs, overwrite_plan())
        assert C.compact_lz4_lift_counts() == (0, 0, 0, 0)
        C.set_compact_lz4_lift_mode("on")
        on = compact(objs, overwrite_plan())
        assert C.compact_lz4_lift_counts(reset=True) == (1, sum(PLANNED), sum(PLANNED), 0)
        assert on == off
        want = C.read_expect(raws, overwrite_plan())
        assert [oracle.lz4_decompress(o, len(w))[1] for o, w in zip(on[1], want)] == want
        # every segment shifted by 4 KiB: no chunk of an output is a chunk of a source
        shifted = compact(objs, overwrite_plan(4096))
        assert C.compact_lz4_lift_counts() == (0, 0, 0, 0)
        C.set_compact_lz4_lift_mode("off")
        assert compact(objs, overwrite_plan(4096)) == shifted


def test_exact_parse_mode_never_lifts(switch, raws):
    objs = store(raws)
    off = compact(objs, overwrite_plan())
    C.set_compact_lz4_lift_mode("on")
    assert compact(objs, overwrite_plan()) == off
    assert C.compact_lz4_lift_counts() == (0, 0, 0, 0)


def test_sealed_compaction_on_equals_off(switch, raws):
    algo = E.CHACHA20_RSA
    rng = np.random.default_rng(5)
    sp = [(rng.bytes(32), rng.bytes(12), b"") for _ in range(4)]
    op = [(rng.bytes(32), rng.bytes(12), b"") for _ in range(4)]
    plan = overwrite_plan()
    want = C.read_expect(raws, plan)
    with C.lz4_parse_mode("fast"):
        pairs = [(bytearray(E.envelope_bound(L.ALGO_LZ4, N, len(p[2]))), r) for r, p in zip(raws, sp)]
        res = E.compress_seal_batch(L.ALGO_LZ4, algo, pairs, sp)
        assert all(e is None for _, e in res)
        envs = [bytes(d[:n]) for (d, _), (n, _) in zip(pairs, res)]
        got = []
        for mode in ("off", "on"):
            C.set_compact_lz4_lift_mode(mode)
            outs = [bytearray(E.envelope_bound(L.ALGO_LZ4, N, 0)) for _ in range(4)]
            sres, ores, crcs = E.compact_seal_batch(L.ALGO_LZ4, algo, [(e, N) for e in envs], [p[0] for p in sp], outs, op, plan,
                                                    with_crc=True)
            assert all(e is None for _, e in sres) and all(e is None for _, e in ores), (sres, ores)
            got.append(([bytes(o[:n]) for o, (n, _) in zip(outs, ores)], crcs))
        assert C.compact_lz4_lift_counts() == (1, sum(PLANNED), sum(PLANNED), 0)
    assert got[0] == got[1]
    dec = [bytearray(N) for _ in range(4)]
    opened = E.open_decompress_batch(L.ALGO_LZ4, algo, list(zip(dec, got[1][0])), [p[0] for p in op])
    assert [(n, e) for n, e, *_ in opened] == [(N, None)] * 4 and [bytes(d) for d in dec] == want
