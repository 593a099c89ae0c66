"""GPU parity of the LZ4 decode copier's control paths (lz4_decode.hip: the
ordered tail and its packed descriptor, the literal and far step loops, the
per-batch masks, the window and batch shapes).

Hand-built valid streams: a small encoder emits (literal length, match length,
offset) triples.  A literal run longer than the staged window (2,048 bytes)
ends its window, so the tokens after it are tokens 0, 1, ... of a fresh window
and fill its 64-token batches in order; a run of 70 literals (over the
64-byte batch limit) ends a batch.  Streams produce 8..64 KiB, at most 64 per
launch, each decoded at dst mod 16 = 0, 1, 7 and 15.  Bar: the CPU oracle's
return value and bytes for every stream; a stream the oracle rejects fails."""
import random

import pytest

from tests.test_lz4_kernel_gpu import _run_device

pytestmark = pytest.mark.gpu

R = 4096
BSPAN = 2048
LMAX = 64


class Enc:
    """LZ4 block encoder of given triples; literal bytes are seeded noise."""

    def __init__(self, seed):
        self.rng = random.Random(seed)
        self.b = bytearray()
        self.pos = 0

    @staticmethod
    def _ext(b, v):
        while v >= 255:
            b.append(255)
            v -= 255
        b.append(v)

    def tok(self, ll, ml, off):
        assert ml >= 4 and 1 <= off <= min(self.pos + ll, 65535), (self.pos, ll, ml, off)
        self.b.append((min(ll, 15) << 4) | min(ml - 4, 15))
        if ll >= 15:
            self._ext(self.b, ll - 15)
        self.b += bytes(self.rng.randrange(256) for _ in range(ll))
        self.b += off.to_bytes(2, "little")
        if ml - 4 >= 15:
            self._ext(self.b, ml - 4 - 15)
        self.pos += ll + ml

    def new_window(self, upto=None, ml=4):
        """A literal run longer than a window: the next token is token 0 of a window.
        upto: the output position after the token."""
        ll = 2200 if upto is None else upto - ml - self.pos
        assert ll >= 2100, (self.pos, upto)
        self.tok(ll, ml, 7)

    def end_batch(self):
        self.tok(70, 4, 33)

    def back(self, O0, ll, extra=40):
        """offset of a match after ll literals whose source starts `extra` bytes before O0"""
        return self.pos + ll - O0 + extra

    def finish(self):
        for _ in range(40):
            self.tok(3, 6, 11)
        self.b += bytes([0xF0, 5]) + bytes(self.rng.randrange(256) for _ in range(20))
        return bytes(self.b)


def _start(seed, cross):
    """A stream whose next token is token 0 of a window and writes at a ring end
    (cross) or 300 bytes past one."""
    e = Enc(seed)
    e.new_window(upto=2 * R - 150 if cross else 2 * R + 300)
    return e


def _tail(seed, ntail, cross):
    """one 64-token batch with ntail matches left to the ordered tail: a chain
    in which every match reads the match before it"""
    e = _start(seed, cross)
    O0 = e.pos
    free = 64 - ntail
    if ntail == 64:
        e.tok(1, 20, 300)  # first step in the near round, 4 bytes left to the tail
        free = 0
        ntail = 63
    for i in range(free):
        e.tok(2, 6, e.back(O0, 2, 50 + i))
    for i in range(ntail):
        e.tok(1, 8, 9)
    e.end_batch()
    return e.finish()


def _fields(seed, kind):
    e = _start(seed, kind in ("len65x",))
    O0 = e.pos
    if kind.startswith("span"):
        # 63 tokens of 32 bytes, then a tail match ending at span 2047 / 2048 / 2049
        last = {"span2047": 30, "span2048": 31, "span2049": 32}[kind]
        for i in range(63):
            e.tok(28, 4, e.back(O0, 28, 10 + i))
        e.tok(1, last, 3)
    elif kind.startswith("len"):
        ml = 65 if "65" in kind else 64
        for i in range(20):
            e.tok(2, 5, 7)  # chain: the long match below waits for these
        e.tok(1, ml, 6)     # overlapping, source in the chain
        e.tok(1, ml, ml)    # D == length, source = the match before
        e.tok(0, ml, 2 * ml + 40)
    else:
        D = int(kind[1:])
        for i in range(8):
            e.tok(3, 5, 6)
        if D == 0:  # the largest in-batch distance: the source starts at O0
            e.tok(2, 24, e.pos + 2 - O0)
            e.tok(2, 64, e.pos + 2 - O0)
        else:
            for ml in (4, D if D >= 4 else 5, 18, 40, 64):
                e.tok(1, ml, D)
    e.end_batch()
    return e.finish()


def _lits(seed, cross):
    e = _start(seed, cross)
    O0 = e.pos
    for ll in (0, 1, 15, 16, 17, 32, 33, 64):  # each as the longest run of its batch
        for i in range(6):
            e.tok(min(ll, i), 5, e.back(e.pos - 100, min(ll, i)))
        e.tok(ll, 6, e.back(e.pos - 100, ll))
        e.end_batch()
    return e.finish()


def _far(seed, nfar, cross, under=False):
    """a batch of 64 tokens of which nfar are far matches (offset > 4 KiB) of
    4, 16, 17, 32, 33 and 64 bytes in turn; under: one of them from a source
    position < 4 of the block"""
    e = Enc(seed)
    e.new_window()
    e.new_window()
    e.new_window(upto=4 * R - 150 if cross else 4 * R + 300)
    lens = (4, 16, 17, 32, 33, 64)
    for i in range(64):
        if i < nfar:
            ml = lens[i % 6] if nfar > 1 else lens[seed % 6]
            ml = min(ml, 20) if nfar == 64 else ml  # span <= 2,048
            off = 4200 + 37 * i
            if under and i == 1:
                off = e.pos + 1 - (seed % 4)
            e.tok(1, ml, off)
        else:
            e.tok(2, 6, 300 + i)
    e.end_batch()
    return e.finish()


def _window(seed, T):
    """windows of T tokens: T - 1 short tokens, closed by a literal run longer than a window"""
    e = _start(seed, False)
    for rep in range(2):
        if T == 448:  # 3-byte tokens: more than the table holds, the window ends at the cap
            for i in range(700):
                e.tok(0, 4, 5 + (i % 90))
        else:
            for i in range(T - 1):
                e.tok(i % 3, 4 + i % 9, 5 + (i * 7) % 200)
        e.new_window()
    return e.finish()


def _all_streams():
    out = []
    seed = 9100
    for ntail in (0, 1, 2, 63, 64):
        for cross in (False, True):
            seed += 1
            out.append((f"tail{ntail}/{'x' if cross else 'n'}", _tail(seed, ntail, cross), 0))
    for kind in ("span2047", "span2048", "span2049", "len64", "len65", "len65x", "D1", "D15", "D16", "D17", "D0"):
        seed += 1
        out.append((kind, _fields(seed, kind), 0))
    for cross in (False, True):
        seed += 1
        out.append((f"lits/{'x' if cross else 'n'}", _lits(seed, cross), 0))
    for nfar in (0, 1, 64):
        for cross in (False, True):
            for k in range(6 if nfar == 1 else 1):
                seed += 1
                out.append((f"far{nfar}/{'x' if cross else 'n'}/{k}", _far(seed - seed % 6 + k, nfar, cross), 0))
    for k in range(4):
        out.append((f"farunder{k}", _far(9300 + k, 8, False, under=True), 0))
    for T in (1, 63, 64, 65, 448):
        seed += 1
        out.append((f"window{T}", _window(seed, T), 0))
    # an output-side check declines a token: the destination ends 0 / 70 / 200 bytes after the data
    for slack in (0, 70, 200):
        out.append((f"decline{slack}", _tail(9400 + slack, 2, False), slack))
    return out


@pytest.fixture(scope="module")
def path_streams(oracle):
    res = []
    for name, comp, slack in _all_streams():
        want, ref = oracle.lz4_decompress(comp, 1 << 17)
        assert 8192 <= want <= 65536, (name, want)  # a rejected stream is a bug of this file
        cap = want + slack if name.startswith("decline") else want + 64
        w2, ref2 = oracle.lz4_decompress(comp, cap)
        assert w2 == want, (name, w2, want)
        res.append((name, comp, cap, want, bytes(ref[:want])))
    assert len(res) <= 64
    return res


@pytest.mark.parametrize("mis_d", (0, 1, 7, 15))
def test_copier_paths(gpu, path_streams, mis_d):
    r, oh, offs_d = _run_device(gpu, [c for _, c, _, _, _ in path_streams], [cap for _, _, cap, _, _ in path_streams],
                                mis_d=mis_d)
    bad = []
    for k, (name, comp, cap, want, ref) in enumerate(path_streams):
        got = oh[offs_d[k]:offs_d[k] + want].tobytes()
        if r[k] != want:
            bad.append((name, r[k], want))
        elif got != ref:
            bad.append((name, "bytes", next(x for x in range(want) if got[x] != ref[x])))
    assert not bad, f"{len(bad)} of {len(path_streams)} mismatch at dst mod 16 = {mis_d}, first: {bad[:4]}"
