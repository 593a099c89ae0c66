"""GPU: the LZ4 lift on streams the fast encoder did not write.
lz4_lift.h promises that a chunk the rule accepts is emitted from the source's
own sequences and is still a valid block of the same content.  Here lift_kernel
meets the hand-made streams of tests/lz4_lift_cases.py and a real encoder's
blocks, and stitch and emit meet records the fast parse never leaves: 65,535-byte
matches, 65,532 literals in one record, chunks without a record.  The oracle is
the host expectation jfs_test_lz4_fast_lift_host (tests/test_lz4_lift.py pins it
against the sanitizer-built driver): the device's verdicts, sizes and bytes equal
it, the bytes decode (liblz4) to the gathered content, and not a byte outside
dst[0, ret) is written."""
import numpy as np
import pytest

from juicefs_amd import _lib as L
from juicefs_amd import compress as C
from juicefs_amd import device as D
from juicefs_amd import encrypt as E
from tests import lz4_chase_cases as K
from tests import lz4_lift_cases as LC
from tests.test_lz4_lift_gpu import CANARY, Z, overwrite_plan, pack, run_lift, same_bytes, store, switch  # noqa: F401

pytestmark = pytest.mark.gpu
CH, N = LC.CH, LC.N


def check_blocks(oracle, names, plain, lifted_run, lifted, doffs, outs, lift, streams, scaps, verdicts=None):
    """per block: the verdict, ret and the bytes against the host expectation, the decode, the plain fast encoder's
    bytes where nothing is lifted; then every byte between the blocks"""
    rets, dst = lifted_run
    assert len(rets) == len(lifted) == len(outs) == len(names)
    written = np.zeros(len(dst), dtype=bool)
    hooks = []
    for k, name in enumerate(names):
        want, nlift, nrec = C.lz4_fast_lift_host(outs[k], lift[k], streams, scaps)
        hooks.append((want, nlift, nrec))
        got = dst[doffs[k]:doffs[k] + rets[k]].tobytes()
        print(f"{name}: host lifted {nlift} size {len(want)}; device lifted {lifted[k]} ret {rets[k]}")
        if verdicts is not None:
            assert nlift == verdicts[k], (name, nlift)
        assert lifted[k] == nlift, (name, lifted[k], nlift)
        assert rets[k] == len(want), (name, rets[k], len(want))
        if got != want:
            a, b = np.frombuffer(got, dtype=np.uint8), np.frombuffer(want, dtype=np.uint8)
            pytest.fail(f"{name}: first difference from the host expectation at byte {int(np.flatnonzero(a != b)[0])}")
        assert oracle.lz4_decompress(got, len(outs[k]))[1] == outs[k], name
        if nlift == 0:
            assert rets[k] == plain[0][k] and got == plain[1][doffs[k]:doffs[k] + rets[k]].tobytes(), name
        written[doffs[k]:doffs[k] + rets[k]] = True
    stray = np.flatnonzero((dst != CANARY) & ~written)
    assert stray.size == 0, f"byte {int(stray[0])} outside every dst[0, ret) was written"
    return hooks


@pytest.fixture(scope="module")
def directed_cases(oracle):
    """[(name, stream, chunk, ok, the stream's decode)]"""
    out = []
    for name, s, c, ok, _ in LC.directed():
        total = sum(ll + ml for ll, _, ml, _ in K.sequences(s))
        dec = oracle.lz4_decompress(s, total)[1]
        assert len(dec) == total, name
        out.append((name, s, c, ok, dec))
    return out


@pytest.mark.parametrize("part", [0, 1, 2])
def test_directed_streams_through_lift_kernel(gpu, oracle, directed_cases, part):
    """every hand-made stream: the gathered block is the stream's own decode, the source's capacity its true length,
    and the case's chunk the one candidate"""
    cases = directed_cases[part::3]
    assert len(cases) >= 7
    streams = [s for _, s, *_ in cases]
    outs = [dec for *_, dec in cases]
    scaps = [len(o) for o in outs]
    lift = [LC.candidates(c, len(dec), src=i) for i, (_, _, c, _, dec) in enumerate(cases)]
    plain, lifted_run, lifted, src_n, doffs = run_lift(gpu, streams, outs, lift, src_cap=scaps)
    assert src_n == scaps
    check_blocks(oracle, [c[0] for c in cases], plain, lifted_run, lifted, doffs, outs, lift, streams, scaps,
                 verdicts=[ok for _, _, _, ok, _ in cases])


@pytest.mark.parametrize("group", [0, 1], ids=["one-group", "a-group-per-block"])
def test_moved_foreign_chunks(gpu, oracle, directed_cases, group):
    """[chunk 1 of X | chunk 0 of Y | 5,000 other bytes], and the two the other way round: each chunk is lifted from
    a chunk index other than its own; with a launch group per block the second block's candidates are offset"""
    by = {name: (s, dec) for name, s, _, _, dec in directed_cases}
    (x, xd), (y, yd) = by["overlap-off1-behind-one-literal"], by["match-ends-on-E-chunk-0"]
    other = LC._rand(77, 10000)
    outs = [xd[CH:2 * CH] + yd[:CH] + other[:5000], yd[:CH] + xd[CH:2 * CH] + other[5000:]]
    lift = [[(0, 1), (1, 0), (-1, 0)], [(1, 0), (0, 1), (-1, 0)]]
    scaps = [len(xd), len(yd)]
    lib = L.load()
    prev = lib.jfs_test_set_lz4_fast_group_chunks(group)
    try:
        plain, lifted_run, lifted, src_n, doffs = run_lift(gpu, [x, y], outs, lift, src_cap=scaps)
    finally:
        lib.jfs_test_set_lz4_fast_group_chunks(prev)
    assert src_n == scaps
    check_blocks(oracle, ["X1-Y0", "Y0-X1"], plain, lifted_run, lifted, doffs, outs, lift, [x, y], scaps, verdicts=[2, 2])


@pytest.fixture(scope="module")
def unshared():
    return [LC.unshared_block(40 + i) for i in range(4)]


def exact_streams(dev, raws):
    """the exact encoder's blocks (D.lz4_compress)"""
    import torch
    dsrc, soffs = pack(dev, raws)
    cap = D.lz4_bound(N)
    ddst = torch.zeros(len(raws) * (cap + 16), dtype=torch.uint8, device=dev)
    ret = torch.zeros(len(raws), dtype=torch.int32, device=dev)
    D.lz4_compress(D.make_desc(dsrc, soffs, [N] * len(raws), ddst, [i * (cap + 16) for i in range(len(raws))],
                               [cap] * len(raws)), ret)
    torch.cuda.synchronize()
    return [ddst[i * (cap + 16):i * (cap + 16) + r].cpu().numpy().tobytes() for i, r in enumerate(ret.cpu().tolist())]


def liftable_chunks(raw, stream):
    """the host rule's verdict on the four interior chunks of a block"""
    _, _, nrec = C.lz4_fast_lift_host(raw, [(0, j) for j in range(4)] + [(-1, 0)], [stream], [N])
    return sum(r >= 0 for r in nrec)


@pytest.mark.parametrize("encoder", ["exact", "liblz4"])
def test_real_encoder_chunks_are_lifted(gpu, oracle, unshared, encoder):
    """blocks whose chunks share no content, stored by the exact encoder and by liblz4: most chunks are liftable, and
    what the device lifts and writes is the host expectation's"""
    streams = exact_streams(gpu, unshared) if encoder == "exact" else [oracle.lz4_compress(r)[1] for r in unshared]
    per = [liftable_chunks(r, s) for r, s in zip(unshared, streams)]
    assert min(per) >= 3, per
    outs, lift = LC.overwritten(unshared)
    assert [sum(s >= 0 for s, _ in l) for l in lift] == LC.PLANNED
    plain, lifted_run, lifted, src_n, doffs = run_lift(gpu, streams, outs, lift)
    assert src_n == [N] * 4
    hooks = check_blocks(oracle, [f"{encoder}-{k}" for k in range(4)], plain, lifted_run, lifted, doffs, outs, lift,
                         streams, [N] * 4)
    assert sum(h[1] for h in hooks) >= 8  # (the lift really ran on foreign records)
    assert any(h[0] != plain[1][at:at + r].tobytes() for h, at, r in zip(hooks, doffs, plain[0]))


def test_zero_record_chunks_behind_a_lift(gpu, oracle):
    """text | random | random | text | ragged text, stored by the fast encoder.  The overwrite in the last whole chunk:
    chunks 0 to 2 are lifted, two of them without a record, and their literals join the parsed chunk's first
    sequence.  The overwrite in chunk 0: a parsed chunk's tail runs through two lifted chunks without a record."""
    raws = [LC.zero_record_block(50), LC.zero_record_block(60)]
    streams = [C.lz4_fast_host(r) for r in raws]
    outs, lift = LC.overwritten(raws, [3 * CH + 1000, 1000])
    assert lift == [[(0, 0), (0, 1), (0, 2), (-1, 0), (-1, 0)], [(-1, 0), (1, 1), (1, 2), (1, 3), (-1, 0)]]
    plain, lifted_run, lifted, src_n, doffs = run_lift(gpu, streams, outs, lift)
    assert src_n == [N] * 2
    hooks = check_blocks(oracle, ["cut-in-chunk-3", "cut-in-chunk-0"], plain, lifted_run, lifted, doffs, outs, lift,
                         streams, [N] * 2, verdicts=[3, 3])
    assert [h[2] for h in hooks] == [[hooks[0][2][0], 0, 0, -1, -1], [-1, 0, 0, hooks[1][2][3], -1]]
    assert hooks[0][2][0] > 0 and hooks[1][2][3] > 0
    same_bytes(plain, lifted_run)
    assert lifted == [3, 3]


def hook_sizes(unshared, objs):
    outs, lift = LC.overwritten(unshared)
    hooks = [C.lz4_fast_lift_host(o, l, objs, [N] * 4) for o, l in zip(outs, lift)]
    return outs, [len(h[0]) for h in hooks], sum(h[1] for h in hooks)


def compact_full(objs, plan):
    """tests/test_lz4_lift_gpu.py's compact, with the sources' results"""
    totals = [sum(s[3] for s in plan[1][plan[0][j]:plan[0][j + 1]]) for j in range(len(plan[0]) - 1)]
    outs = [bytearray(Z.CompressBound(t)) for t in totals]
    sres, ores, crcs = Z.CompactBatch([(o, N) for o in objs], outs, plan, with_crc=True)
    assert all(e is None for _, e in ores), ores
    return sres, [n for n, _ in ores], [bytes(o[:n]) for o, (n, _) in zip(outs, ores)], crcs


def test_compaction_over_exact_encoder_objects(switch, oracle, unshared):
    """the mixed deployment: objects stored under the exact parse mode, compacted under the fast one with the switch
    on.  The outputs decode to the planned content, the counters are the host rule's, and every size is the host
    expectation's.  (The payloads' CRC-32C are checked against the payloads, and against the switch-off's wherever the
    payload is the switch-off's: a block emitted from liblz4's sequences is not the fast encoder's block.)"""
    with C.lz4_parse_mode("exact"):
        objs = store(unshared)
    assert objs == [oracle.lz4_compress(r)[1] for r in unshared]
    want, sizes, nlift = hook_sizes(unshared, objs)
    planned = sum(LC.PLANNED)
    assert nlift >= 8 and want == C.read_expect(unshared, overwrite_plan())
    with C.lz4_parse_mode("fast"):
        off = compact_full(objs, overwrite_plan())
        assert C.compact_lz4_lift_counts() == (0, 0, 0, 0)
        C.set_compact_lz4_lift_mode("on")
        on = compact_full(objs, overwrite_plan())
        assert C.compact_lz4_lift_counts(reset=True) == (1, planned, nlift, planned - nlift)
    assert on[0] == off[0] == [(N, None)] * 4
    on, off = on[1:], off[1:]
    for k, (got, w) in enumerate(zip(on[1], want)):
        assert oracle.lz4_decompress(got, len(w))[1] == w, k
        assert oracle.lz4_decompress(off[1][k], len(w))[1] == w, k
        assert on[2][k] == oracle.crc32c(got) and off[2][k] == oracle.crc32c(off[1][k]), k
        assert (on[2][k] == off[2][k]) == (got == off[1][k]), k
    assert on[0] == sizes
    assert on[1] != off[1]  # (foreign records were emitted)


def test_sealed_compaction_over_exact_encoder_objects(switch, unshared):
    algo = E.CHACHA20_RSA
    rng = np.random.default_rng(6)
    sp = [(rng.bytes(32), rng.bytes(12), b"") for _ in range(4)]
    op = [(rng.bytes(32), rng.bytes(12), b"") for _ in range(4)]
    plan = overwrite_plan()
    want = C.read_expect(unshared, plan)
    pairs = [(bytearray(E.envelope_bound(L.ALGO_LZ4, N, len(p[2]))), r) for r, p in zip(unshared, sp)]
    with C.lz4_parse_mode("exact"):
        res = E.compress_seal_batch(L.ALGO_LZ4, algo, pairs, sp)
        objs = store(unshared)  # (the envelopes' payloads)
    assert all(e is None for _, e in res)
    envs = [bytes(d[:n]) for (d, _), (n, _) in zip(pairs, res)]
    _, _, nlift = hook_sizes(unshared, objs)
    with C.lz4_parse_mode("fast"):
        C.set_compact_lz4_lift_mode("on")
        outs = [bytearray(E.envelope_bound(L.ALGO_LZ4, N, 0)) for _ in range(4)]
        sres, ores, _ = E.compact_seal_batch(L.ALGO_LZ4, algo, [(e, N) for e in envs], [p[0] for p in sp], outs, op, plan,
                                             with_crc=True)
        assert all(e is None for _, e in sres) and all(e is None for _, e in ores), (sres, ores)
        assert C.compact_lz4_lift_counts() == (1, sum(LC.PLANNED), nlift, sum(LC.PLANNED) - nlift)
    dec = [bytearray(N) for _ in range(4)]
    opened = E.open_decompress_batch(L.ALGO_LZ4, algo, [(d, bytes(o[:n])) for d, o, (n, _) in zip(dec, outs, ores)],
                                     [p[0] for p in op])
    assert [(n, e) for n, e, *_ in opened] == [(N, None)] * 4 and [bytes(d) for d in dec] == want
