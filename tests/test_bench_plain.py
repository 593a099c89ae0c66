"""bench.py's plain run and --dump-outputs.

* dump_outputs writes decoded.npy (float32) and sizes.npy (float64): every
  byte of a small output, a fixed seeded sample of a large one, the same
  sample on every call.
* --full is off by default.
* (GPU) a plain run of a tiny batch prints exactly one JSON result line with
  the headline fields and no sub-record, times the steps it was asked for, and
  dumps the bytes the block generator defines for its seeds.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402
from juicefs_amd.blockgen import gen_block  # noqa: E402


class _Batch:
    def __init__(self, out, ret):
        self.out, self.dec_ret = torch.from_numpy(out), torch.from_numpy(ret)


def test_dump_outputs_small_is_every_byte(tmp_path):
    out = np.random.default_rng(1).integers(0, 256, 5000, dtype=np.uint8)
    ret = np.array([1000, 1000, 1000, 1000, -3], dtype=np.int32)
    d = tmp_path / "a" / "b"  # created on demand
    bench.dump_outputs(_Batch(out, ret), str(d))
    assert sorted(os.listdir(d)) == ["decoded.npy", "sizes.npy"]
    dec, sizes = np.load(d / "decoded.npy"), np.load(d / "sizes.npy")
    assert dec.dtype == np.float32 and np.array_equal(dec, out.astype(np.float32))
    assert sizes.dtype == np.float64 and np.array_equal(sizes, ret.astype(np.float64))


def test_dump_outputs_large_is_a_fixed_sample(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_SAMPLE", 1000)
    out = np.random.default_rng(2).integers(0, 256, 100001, dtype=np.uint8)
    ret = np.full(7, 14286, dtype=np.int32)
    bench.dump_outputs(_Batch(out, ret), str(tmp_path / "x"))
    bench.dump_outputs(_Batch(out, ret), str(tmp_path / "y"))
    x, y = np.load(tmp_path / "x" / "decoded.npy"), np.load(tmp_path / "y" / "decoded.npy")
    assert x.dtype == np.float32 and x.shape == (1000,)
    assert np.array_equal(x, y)
    # the sample follows the output: another output of the same size, sampled
    # at the same offsets, differs where the outputs differ
    idx = np.sort(np.random.default_rng(20240917).integers(0, out.size, 1000, dtype=np.int64))
    assert np.array_equal(x, out[idx].astype(np.float32))
    assert idx[0] < out.size // 10 and idx[-1] > out.size - out.size // 10  # spans the buffer


def test_full_is_off_by_default(monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "3", "--warmup", "1"])
    a = bench.parse()
    assert a.full is False and a.dump_outputs is None and a.steps == 3
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "d"])
    a = bench.parse()
    assert a.full is True and a.dump_outputs == "d"


@pytest.mark.gpu
def test_plain_run_one_line_and_dump(gpu, tmp_path):
    nblk, U, steps = 5, 1 << 16, 3
    d = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps),
                        "--warmup", "1", "--blocks", str(nblk), "--block-bytes", str(U), "--dump-outputs", str(d)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, lines
    out = json.loads(lines[0])
    assert out["metric"] == bench.METRIC and out["unit"] == "GiB/s" and out["dtype"] == "u8"
    assert out["higher_is_better"] is True and out["steps"] == steps and out["n_gpus"] == 1
    assert out["ms_per_step"] > 0
    assert out["value"] == pytest.approx(nblk * U / (out["ms_per_step"] / 1e3) / 2**30, rel=1e-9)
    for k in ("configs_3", "configs_2", "configs_0", "checksum_aead", "lz4_other_classes", "cpu_baseline",
              "cpu_oracle", "compress", "cpu_codecs", "host_path", "oneshot_concurrency", "mixed_host_path"):
        assert k not in out, k
    dec, sizes = np.load(d / "decoded.npy"), np.load(d / "sizes.npy")
    want = np.frombuffer(b"".join(gen_block("T", 1 + i, U) for i in range(nblk)), dtype=np.uint8)
    assert dec.dtype == np.float32 and np.array_equal(dec, want.astype(np.float32))
    assert sizes.dtype == np.float64 and np.array_equal(sizes, np.full(nblk, U, dtype=np.float64))
