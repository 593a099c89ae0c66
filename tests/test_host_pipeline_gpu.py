"""Host batch path (capi.hip run_batch): many chunks pipelined over two
streams.  A child process with a 16 MiB staging chunk pushes ~60 blocks
through several chunks per call, mixed sizes and codecs; every result must
match a single-chunk run and the CPU oracle (LZ4 and Zstd level-1 bytes exact,
both round trips)."""
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CHILD = r'''
import hashlib, sys
sys.path.insert(0, sys.argv[1])
from juicefs_amd import compress as C
from juicefs_amd.blockgen import gen_block
from tests import oracle_ctypes
o = oracle_ctypes.Oracle(sys.argv[2])
sizes = [(64 << 10) + 37 * i if i % 3 else (3 << 20) + 1001 * i for i in range(60)]
srcs = [gen_block("TZR"[i % 3] if i % 5 else "T", 4000 + i, n) for i, n in enumerate(sizes)]
lz, zs = C.LZ4(), C.ZStandard()
for c in (lz, zs):
    pairs = [(bytearray(c.CompressBound(len(s))), s) for s in srcs]
    res = c.CompressBatch(pairs)
    frames = []
    for (d, s), (n, e) in zip(pairs, res):
        assert e is None and n > 0, e
        frames.append(bytes(d[:n]))
        if c is lz:
            m, ref = o.lz4_compress(s)
            assert bytes(d[:n]) == ref
        else:  # byte-identical to libzstd 1.4.9 level 1 (the restatement the oracle pins)
            assert bytes(d[:n]) == o.zstd_compress_l1(s)
    outs = [bytearray(len(s)) for s in srcs]
    back = c.DecompressBatch(list(zip(outs, frames)))
    for s, b, (n, e) in zip(srcs, outs, back):
        assert e is None and n == len(s) and bytes(b) == s
print("OK", len(srcs))
'''


def test_multi_chunk_pipeline(gpu, oracle):
    env = dict(os.environ, JFS_HOST_CHUNK_MB="16")
    so = os.path.join(ROOT, "oracle", "_build", "liboracle.so")
    r = subprocess.run([sys.executable, "-c", CHILD, ROOT, so], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "OK 60" in r.stdout, (r.stdout[-2000:], r.stderr[-2000:])


# The aead, crc and checksum areas of a chunk's staging across reused slots:
# sealed PUT with envelope CRCs, GET, plain PUT with payload CRCs, decode with
# disk-cache checksums (the calls of test_encrypt_gpu.py / test_batch_gpu.py,
# there within one chunk).  Prints a digest of every result.
CHILD_AREAS = r'''
import hashlib, json, sys
sys.path.insert(0, sys.argv[1])
from juicefs_amd import compress as C, encrypt as E
from juicefs_amd.blockgen import gen_block
from tests import oracle_ctypes
from tests.test_encrypt_gpu import CODECS
o = oracle_ctypes.Oracle(sys.argv[2])
sizes = [(1 << 20) + 1001 * i if i % 2 else (64 << 10) + 37 * i for i in range(48)]
# the 1 MiB blocks are incompressible ("R"), so that the decode calls stage as much as the encode calls
raws = [gen_block("R" if i % 2 else "TZ"[i // 2 % 2], 7000 + i, n) for i, n in enumerate(sizes)]
params = [(bytes((i + j) & 255 for j in range(32)), bytes((3 * i + j) & 255 for j in range(12)), b"w" * (40 + i))
          for i in range(len(raws))]
digest = {}
for name in ("lz4", "zstd"):
    c, h = C.NewCompressor(name), hashlib.sha256()
    pairs = [(bytearray(E.envelope_bound(CODECS[name], len(r), len(p[2]))), r) for r, p in zip(raws, params)]
    crcs = []
    res = E.compress_seal_batch(CODECS[name], E.CHACHA20_RSA, pairs, params, crcs=crcs)
    envs = []
    for (d, _), (n, e), crc in zip(pairs, res, crcs):
        assert e is None and crc == o.crc32c(bytes(d[:n])), (name, "seal", e)
        envs.append(bytes(d[:n]))
        h.update(envs[-1] + crc.to_bytes(4, "little"))
    outs = [bytearray(len(r)) for r in raws]
    back = E.open_decompress_batch(CODECS[name], E.CHACHA20_RSA, list(zip(outs, envs)), [p[0] for p in params])
    for r, b, (n, e) in zip(raws, outs, back):
        assert e is None and n == len(r) and bytes(b) == r, (name, "open", e)
        h.update(bytes(b))
    pairs = [(bytearray(c.CompressBound(len(r))), r) for r in raws]
    comps = []
    for (d, _), (n, e, crc) in zip(pairs, c.CompressBatchChecksum(pairs)):
        assert e is None and crc == o.crc32c(bytes(d[:n])), (name, "compress", e)
        comps.append(bytes(d[:n]))
        h.update(comps[-1] + crc.to_bytes(4, "little"))
    outs = [bytearray(len(r)) for r in raws]
    for r, b, (n, e, cs) in zip(raws, outs, c.DecompressBatchChecksum(list(zip(outs, comps)))):
        assert e is None and n == len(r) and bytes(b) == r and cs == o.crc32c_segments(r), (name, "decode", e)
        h.update(bytes(b) + cs)
    digest[name] = h.hexdigest()
print("DIGEST", json.dumps(digest, sort_keys=True))
'''


def test_multi_chunk_aead_crc_csum_areas(gpu, oracle):
    """48 blocks of 64 KiB / 1 MiB through 16 MiB chunks on one device, with
    encryption, PUT checksums and disk-cache checksums: each of the eight calls
    (seal, open, compress + CRC, decode + checksums; LZ4 and Zstd) runs in at
    least four chunks (counted from the trace), so slot 0's areas are laid out
    anew over a used slot within the call and every slot across calls.  Round
    trips, the oracle's CRCs, and every result equal to a default-chunk run."""
    so = os.path.join(ROOT, "oracle", "_build", "liboracle.so")
    digests = []
    default = {k: v for k, v in os.environ.items() if not k.startswith("JFS_HOST_CHUNK_MB")}
    small = dict(default, JFS_HOST_CHUNK_MB="16", JFS_HOST_CHUNK_MB_LZ4C="16", JFS_HOST_TRACE="1", JFS_GPU_DEVICES="0")
    for env in (small, default):
        r = subprocess.run([sys.executable, "-c", CHILD_AREAS, ROOT, so], env=env, capture_output=True, text=True,
                           timeout=300)
        assert r.returncode == 0 and "DIGEST" in r.stdout, (r.stdout[-2000:], r.stderr[-2000:])
        digests.append(r.stdout[r.stdout.index("DIGEST"):].strip())
        if env is small:  # chunks per call: a call's first chunk starts at block 0
            starts = re.findall(r"algo (\d) dir (\d) chunk (\d+)-\d+ stage-in", r.stderr)
            calls = []
            for algo, d, s in starts:
                if s == "0":
                    calls.append([algo + d, 0])
                calls[-1][1] += 1
            print("chunks per call:", calls)
            assert [k for k, _ in calls] == ["10", "11", "10", "11", "20", "21", "20", "21"], calls
            assert all(n >= 4 for _, n in calls), calls
    assert digests[0] == digests[1]
