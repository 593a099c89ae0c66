"""GPU parity of the LZ4 decode kernel's copier around the end of its 4 KiB
output ring (lz4_decode.hip: put16 / copy16 / zero_span / far_load / wave_near
and the per-batch choice between wrap-free and masked ring addressing).

Hand-built streams of 8..64 KiB of output (the ring wraps 2..16 times) put one
token case at every wrap, shifted by -20..+20 bytes against the ring's end
(the 20-byte reach of a put16), and end the lane-parallel batch there with a
token longer than the batch limit, so that batches end on, before and after
the boundary.  Every stream is decoded at all 16 values of dst mod 16, which
shifts the ring slots against the output positions (and dst mod 4 for the far
loads that start below dst).  The kernel is called directly
(jfs_lz4_decompress_device, as tests/test_lz4_kernel_gpu.py does), at most 64
blocks per launch.  Bar: the CPU oracle's return value and bytes for every
stream; a stream the oracle rejects fails the test."""
import random

import pytest

from tests.test_lz4_kernel_gpu import _run_device, _tok

pytestmark = pytest.mark.gpu

R = 4096
DELTAS = list(range(-20, 21))
LITS = (1, 3, 4, 15, 16, 17, 63, 64)


class _Stream:
    def __init__(self, seed):
        self.rng = random.Random(seed)
        self.b = bytearray()
        self.pos = 0

    def tok(self, ll, off, ml):
        assert 1 <= off <= min(self.pos + ll, 65535) and ml >= 4, (self.pos, ll, off, ml)
        self.b += _tok(bytes(self.rng.randrange(256) for _ in range(ll)), off, ml)
        self.pos += ll + ml

    def any_off(self, ll):
        top = min(self.pos + ll, 65535)
        k = self.rng.randrange(3)
        return self.rng.randrange(1, min(top, 64 if k == 0 else 3000 if k == 1 else top) + 1)

    def fill_to(self, target):
        """Short text-like tokens (near and far matches) up to exactly `target`."""
        assert target == self.pos or target - self.pos >= 4, (self.pos, target)
        while self.pos < target:
            rem = target - self.pos
            if rem <= 22:
                ml = min(18, rem)
                ll = rem - ml
            else:
                ll, ml = self.rng.randrange(0, 9), self.rng.randrange(4, 11)
            if self.pos == 0:
                ll = max(ll, 1)
            self.tok(ll, self.any_off(ll), ml)

    def end_batch(self):
        """A token over the batch's length limit: the batch before it ends here."""
        self.tok(70, self.any_off(70), 4)

    def finish(self):
        self.fill_to(self.pos + 300 + self.rng.randrange(8))
        self.b += bytes([0xF0, 5]) + bytes(self.rng.randrange(256) for _ in range(20))
        return bytes(self.b)


def _case_batch_end(s, B, d, arg):
    s.fill_to(B + d)


def _case_literal(s, B, d, L):
    s.fill_to(B + d - L // 2 - 40)
    s.fill_to(B + d - L // 2)
    s.tok(L, s.any_off(L), 4)  # the run covers [B + d - L/2, B + d + L - L/2)
    s.fill_to(s.pos + 8)


def _case_near_src(s, B, d, ml):
    """source straddles the ring's end, destination well past it"""
    s.fill_to(B + d + 100)
    s.tok(2, s.pos + 2 - (B + d - ml // 2), ml)
    s.fill_to(s.pos + 8)


def _case_near_dst(s, B, d, ml):
    """destination straddles the ring's end, source well before it"""
    s.fill_to(B + d - ml // 2 - 1)
    s.tok(1, 200 + ml, ml)
    s.fill_to(s.pos + 8)


def _case_period(s, B, d, off):
    s.fill_to(B + d - 9)
    s.tok(2, off, 22 + off)  # period repeat over [B + d - 7, ...)
    s.fill_to(s.pos + 8)


def _case_far_under(s, B, d, msrc):
    """far match (source older than the ring) whose source is output byte 0..3"""
    s.fill_to(B + d - 6)
    s.tok(1, s.pos + 1 - msrc, 4 + (B + d) % 17)
    s.tok(0, s.pos - (msrc ^ 1), 18)
    s.fill_to(s.pos + 8)


def _case_short64(s, B, d, big):
    """64 tokens of 1 literal + 4 match bytes (every ha + m <= 8); big: one 16-byte run among them"""
    s.fill_to(B + d - 200)
    s.end_batch()
    for i in range(64):
        ll = 16 if big and i == 40 else 1
        s.tok(ll, s.rng.randrange(1, 40) if i % 3 else s.any_off(ll), 4)


CASES = ([("end", _case_batch_end, 0)] + [(f"lit{L}", _case_literal, L) for L in LITS] +
         [("nearsrc12", _case_near_src, 12), ("nearsrc40", _case_near_src, 40), ("neardst12", _case_near_dst, 12),
          ("neardst33", _case_near_dst, 33)] + [(f"period{o}", _case_period, o) for o in (1, 2, 3)] +
         [(f"farunder{m}", _case_far_under, m) for m in (0, 1, 2, 3)] +
         [("short64", _case_short64, False), ("short64big", _case_short64, True)])


def _stream(seed, fn, arg, phase, nwrap):
    s = _Stream(seed)
    s.tok(24, 3, 6)
    for w in range(1, nwrap + 1):
        d = DELTAS[(3 * (w - 1) + phase) % len(DELTAS)]
        fn(s, R * w, d, arg)
        s.end_batch()
    return s.finish()


@pytest.fixture(scope="module")
def wrap_streams(oracle):
    """(name, stream, oracle return, oracle bytes): 3 phases x 15 wraps = every shift -20..+20 per case
    (the last stream of a case is 8 KiB: two wraps)"""
    out = []
    for ci, (name, fn, arg) in enumerate(CASES):
        for phase in range(3):
            comp = _stream(7000 + 10 * ci + phase, fn, arg, phase, 15)
            out.append((f"{name}/p{phase}", comp))
        out.append((f"{name}/short", _stream(7900 + ci, fn, arg, 1, 2)))
    res = []
    for name, comp in out:
        want, ref = oracle.lz4_decompress(comp, 1 << 17)
        assert 8192 <= want <= 65535 + 1024, (name, want)  # a rejected stream is a bug of this file
        res.append((name, comp, want, bytes(ref[:want])))
    return res


@pytest.mark.parametrize("mis_d", range(16))
def test_ring_wrap_cases(gpu, wrap_streams, mis_d):
    bad = []
    for i in range(0, len(wrap_streams), 64):
        part = wrap_streams[i:i + 64]
        r, oh, offs_d = _run_device(gpu, [c for _, c, _, _ in part], [w for _, _, w, _ in part], mis_d=mis_d)
        for k, (name, comp, want, ref) in enumerate(part):
            if r[k] != want:
                bad.append((name, r[k], want))
            elif oh[offs_d[k]:offs_d[k] + want].tobytes() != ref:
                got = oh[offs_d[k]:offs_d[k] + want].tobytes()
                first = next(x for x in range(want) if got[x] != ref[x])
                bad.append((name, "bytes", first, first % R))
    assert not bad, f"{len(bad)} of {len(wrap_streams)} mismatch at dst mod 16 = {mis_d}, first: {bad[:4]}"


def test_ring_wrap_short_destination(gpu, oracle, wrap_streams):
    """the same streams into destinations one byte short and 64 bytes long (exact liblz4 returns)"""
    part = wrap_streams[::4][:32]
    comps = [c for _, c, _, _ in part] * 2
    caps = [w - 1 for _, _, w, _ in part] + [w + 64 for _, _, w, _ in part]
    r, oh, offs_d = _run_device(gpu, comps, caps, mis_d=5)
    bad = []
    for k, (comp, cap) in enumerate(zip(comps, caps)):
        want, ref = oracle.lz4_decompress(comp, cap)
        if r[k] != want:
            bad.append((part[k % len(part)][0], cap, r[k], want))
        elif want > 0 and oh[offs_d[k]:offs_d[k] + want].tobytes() != ref[:want]:
            bad.append((part[k % len(part)][0], cap, "bytes"))
    assert not bad, bad[:4]
