"""Host check of the LZ4 origin chase (juicefs_amd/csrc/lz4_chase.h: locate the
segment, walk its tokens, check the visited token, step through matches down to
a literal).  tests/lz4_chase_main.cc, built with AddressSanitizer and UBSan,
builds the segment index with a serial token walk, runs the header's rule for
every output position -- one position at a time and as quads -- and compares
with a serial LZ interpreter.  Nothing is loaded into Python.

The last tests hold the Python restatement of the rule (tests/lz4_chase_cases.py
hop_depths) to the header and recompute the hop histogram CHASE_HOPS comes from."""
import os
import re
import shutil
import struct
import subprocess

import pytest

from juicefs_amd import compress as C
from juicefs_amd.blockgen import gen_block
from tests import lz4_chase_cases as K
from tests import lz4_fast_cases as F
from tests import split_streams as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def streams(oracle):
    """[(name, stream, expectation)]: 'ok' = every position resolves, 'bad' / 'deep' = some position answers so
    ('deep': the driver asks every 7th position -- chains of thousands of steps at every position take too long)."""
    out = []
    # encoder output, both encoders: the fast-parse inputs up to 70,000 bytes and one large text block
    for name, src in F.cases():
        if 0 < len(src) <= 70000 or name == "T-200003":
            out.append((f"exact-{name}", oracle.lz4_compress(src)[1], "ok"))
            out.append((f"fast-{name}", C.lz4_fast_host(src), "ok"))
    # the small-batch decoders' hand-over streams
    out.append(("chain-40", S.chain_stream(40), "ok"))
    out.append(("flat-chain", S.flat_chain_stream(4000), "ok"))
    out.append(("chain-deep", S.chain_stream(K.CHASE_HOPS + 40), "deep"))
    # hand-built: long runs (overlapped: the period rule), fields across segment edges, empty segments, short finals
    for off in (1, 2, 3, 7):
        out.append((f"run-off{off}", K.long_run_stream(off, 5000 + off), "ok"))
    out.append(("run-off65535", K.long_run_stream(65535, 140000), "ok"))
    out.append(("straddle", K.straddle_stream(), "ok"))
    out.append(("tokenless-segment", K.tokenless_segment_stream(), "ok"))
    out.append(("final-0", K.final_len_stream(0), "ok"))
    out.append(("final-1", K.final_len_stream(1), "ok"))
    out.append(("short-final-0", K.short_final_after_match(0), "bad"))
    out.append(("short-final-1", K.short_final_after_match(1), "bad"))
    for name, s in K.BAD_STREAMS.items():
        out.append((name, s, "bad"))
    return out


@pytest.fixture(scope="module")
def rows(streams, tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    d = tmp_path_factory.mktemp("lz4_chase")
    exe, data = str(d / "lz4_chase"), str(d / "cases.bin")
    r = subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "juicefs_amd", "csrc"),
                        os.path.join(ROOT, "tests", "lz4_chase_main.cc"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    with open(data, "wb") as f:
        for _, s, expect in streams:
            f.write(struct.pack("<II", len(s), 7 if expect == "deep" else 1) + s)
    r = subprocess.run([exe, data], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    got = [tuple(map(int, m)) for m in re.findall(
        r"^case (\d+) n (\d+) total (\d+) ok (\d+) bad (\d+) deep (\d+) wrong (\d+) maxhops (\d+) unseen (\d+)$", r.stdout, re.M)]
    assert len(got) == len(streams), r.stdout[-2000:]
    return got


def test_every_position_matches_the_serial_interpreter(streams, rows):
    for (name, s, expect), (_, n, total, ok, bad, deep, wrong, _, unseen) in zip(streams, rows):
        assert n == len(s)
        assert wrong == 0, name                      # no literal index is ever wrong, quads agree with single positions
        assert ok + bad + deep == total, name
        if expect == "ok":
            assert (bad, deep, unseen) == (0, 0, 0), (name, bad, deep, unseen)


def test_the_directed_streams_are_what_their_names_say(streams, rows, oracle):
    by = {name: (s, row) for (name, s, _), row in zip(streams, rows)}
    # overlapped runs really wrap: the match is longer than its offset
    for off in (1, 2, 3, 7, 65535):
        seqs = K.sequences(by[f"run-off{off}"][0])
        assert seqs[0][2] > seqs[0][3] == off
    # the straddling token: length bytes on both sides of 256, match-length bytes on both sides of 1024
    s = by["straddle"][0]
    assert s[253] >> 4 == 15 and s[254] == 255 and s[256] == 5
    assert s[789] == 255 and s[1026] == 9
    # segments 2 and 3 of it, and 1 of the tokenless one, hold no token start
    for name, empty in (("straddle", (2, 3)), ("tokenless-segment", (1,))):
        s, starts, p = by[name][0], set(), 0
        while p < len(s):
            starts.add(p // K.SEG)
            p = S.parse(s, len(s), p)
        assert not starts & set(empty), (name, starts)
    assert by["final-0"][1][2] == 0 and by["final-1"][1][2] == 1  # totals 0 and 1
    # the encoder streams decode to their sources (the interpreter in the driver agreed byte for byte)
    assert by["exact-T-65536"][1][2] == 65536 and by["fast-T-200003"][1][2] == 200003


def test_faulty_tokens_answer_bad(streams, rows):
    by = {name: row for (name, _, _), row in zip(streams, rows)}
    for name in list(K.BAD_STREAMS) + ["short-final-0", "short-final-1"]:
        _, _, total, ok, bad, deep, wrong, _, _ = by[name]
        assert bad > 0 and deep == 0 and wrong == 0, (name, by[name])
    # offset 0 and an offset beyond the bytes produced sit in the first token: nothing of it resolves
    assert by["offset-zero"][3] <= 12 and by["offset-beyond"][3] <= 12  # (only the tail's literals may)


def test_deep_chain_answers_deep(streams, rows):
    by = {name: row for (name, _, _), row in zip(streams, rows)}
    _, _, total, ok, bad, deep, wrong, maxhops, _ = by["chain-deep"]
    assert deep > 0 and bad == 0 and wrong == 0
    assert maxhops == K.CHASE_HOPS                    # the cap is the number of steps a chain may take
    assert by["chain-40"][5] == 0 and by["chain-40"][7] == 40              # one step per unit


def test_python_restatement_counts_the_headers_hops(streams, rows):
    """hop_depths (the histogram's source) against the driver's step counts."""
    for (name, s, expect), row in zip(streams, rows):
        if expect == "ok" and row[2] > 0:
            assert int(K.hop_depths(s).max()) == row[7], name


def test_chase_hops_covers_generated_inputs(oracle):
    """The cap rule -- the smallest power of two at least twice the deepest
    chain -- on text, mixed and fast-parse inputs of 64 KiB to 1 MiB: the chosen
    CHASE_HOPS exceeds every depth seen, and is a power of two.  (The choice
    itself comes from 4 MiB blocks: scripts/lz4_chase_hops.py)"""
    with open(os.path.join(ROOT, "juicefs_amd", "csrc", "lz4_chase.h")) as f:
        m = re.search(r"constexpr int CHASE_HOPS = (\d+);", f.read())
    assert m and int(m.group(1)) == K.CHASE_HOPS and K.CHASE_HOPS & (K.CHASE_HOPS - 1) == 0
    top = 0
    for i, n in enumerate((64 << 10, 256 << 10, 1 << 20)):
        for src in (gen_block("T", 900 + i, n), K.mixed_block(20 + i, n)):
            for comp in (oracle.lz4_compress(src)[1], C.lz4_fast_host(src)):
                _, mx = K.hop_histogram(comp)
                print(f"n={n} comp={len(comp)} max depth {mx}")
                top = max(top, mx)
    assert top > 0
    assert K.CHASE_HOPS > top
    assert K.hops_cap(top) <= K.CHASE_HOPS            # larger blocks chain deeper, never shallower
