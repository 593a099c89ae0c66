"""Measurements of DESIGN.md 5f: whole decodes of seekable Zstd objects, this
build against another build of the library (the parent commit's).

    python scripts/whole_rate.py [--other-root CHECKOUT] [--passes 2]
                                 [--out profiles/seekable/rates_whole.json]

A library is fixed when a process loads it, so every measurement runs in a
child process of this script (--other-root: a built checkout of the other
commit, whose juicefs_amd package and library the child imports instead); the
children of the two builds alternate, `--passes` times.  A child takes medians of 7
repetitions after 2 warm-ups, wall clock around calls that end synchronised,
and compares every decoded byte with the input once, outside the timed region.

Legs: (a) jfs_decompress of one 4 MiB text seekable object; (b) the same
content as one fast frame; (c) DecompressBatch of 64 such seekable objects;
(d) is (a) in a child started with JFS_ZSTD_SPLIT_FRAMES=1 (this build only)."""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.environ.get("JFS_RATE_ROOT") or ROOT)  # (a child of the other build)
MIB4 = 4 << 20
REPS, WARM = 7, 2


def med(samples):
    s = sorted(samples)
    return {"median_ms": round(statistics.median(s) * 1e3, 3), "min_ms": round(s[0] * 1e3, 3),
            "max_ms": round(s[-1] * 1e3, 3)}


def child():
    from juicefs_amd import _lib as L
    from juicefs_amd import compress as C

    def text(seed):
        buf = ctypes.create_string_buffer(MIB4)
        L.load().jfs_gen_block_host(ctypes.addressof(buf), MIB4, b"T", seed)
        return buf.raw
    z = C.ZStandard()
    raws = [text(1 + i) for i in range(64)]

    def stored(mode, rs):
        with C.zstd_parse_mode(mode):
            pairs = [(bytearray(z.CompressBound(MIB4)), r) for r in rs]
            out = z.CompressBatch(pairs)
        assert all(e is None for _, e in out)
        return [bytes(d[:n]) for (d, _), (n, _) in zip(pairs, out)]
    seek, fast = stored("seekable", raws), stored("fast", raws[:1])
    out = bytearray(MIB4)
    pairs = [(bytearray(MIB4), o) for o in seek]

    def one(obj):
        m, err = z.Decompress(out, obj)
        assert err is None and m == MIB4

    def batch():
        assert all(e is None and n == MIB4 for n, e in z.DecompressBatch(pairs))
    one(seek[0])
    assert bytes(out) == raws[0]
    one(fast[0])
    assert bytes(out) == raws[0]
    batch()
    assert all(bytes(d) == r for (d, _), r in zip(pairs, raws))
    fns = {"a seekable, jfs_decompress": lambda: one(seek[0]), "b fast frame, jfs_decompress": lambda: one(fast[0]),
           "c seekable x 64, DecompressBatch": batch}
    t = {k: [] for k in fns}
    for r in range(WARM + REPS):
        for k, f in fns.items():
            t0 = time.perf_counter()
            f()
            if r >= WARM:
                t[k].append(time.perf_counter() - t0)
    print("RESULT " + json.dumps({k: med(v) for k, v in t.items()}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--other-root", default=None)
    ap.add_argument("--passes", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "seekable", "rates_whole.json"))
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child()
    runs = [("this build", None, None), ("this build, JFS_ZSTD_SPLIT_FRAMES=1", None, "1")]
    if a.other_root:
        runs.insert(0, ("other build", os.path.abspath(a.other_root), None))
    res = {"reps": REPS, "warmups": WARM, "passes": []}
    for p in range(a.passes):
        one = {}
        for name, root, frames in runs:
            env = dict(os.environ)
            env.pop("JFS_ZSTD_SPLIT_FRAMES", None)
            env.pop("JFS_RATE_ROOT", None)
            if root:
                env["JFS_RATE_ROOT"] = root
            if frames:
                env["JFS_ZSTD_SPLIT_FRAMES"] = frames
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], env=env, capture_output=True,
                               text=True, timeout=600)
            if r.returncode != 0:
                sys.exit(f"{name}: exit {r.returncode}\n{r.stderr[-3000:]}")
            one[name] = json.loads(next(ln for ln in r.stdout.splitlines() if ln.startswith("RESULT "))[7:])
        res["passes"].append(one)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
