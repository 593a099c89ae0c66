"""The nine run-time switches of the C ABI (juicefs_amd/csrc/host_modes.h has the
table), without a GPU: what the environment gives each getter and what each
setter takes.  Expected values come from include/jfs_gpucodec.h.  A switch reads
its variable once per process, so every environment value gets a fresh child
process (JFS_GPU_CODEC=off: no device is touched); the children of one switch
run side by side."""
import json
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, "include", "jfs_gpucodec.h")) as _f:
    H = {k: int(v) for k, v in re.findall(r"^#define (JFS_\w+) (\d+)\b", _f.read(), re.M)}

# enumerated: variable, getter, setter, _ext setter, {spelling: value} (the first is the default), values the plain
# setter takes (the _ext one takes all)
ENUMS = [
    ("JFS_LZ4_PARSE", "jfs_lz4_parse_mode", "jfs_set_lz4_parse_mode", None,
     {"exact": H["JFS_LZ4_PARSE_EXACT"], "fast": H["JFS_LZ4_PARSE_FAST"]}, 2),
    ("JFS_READ_DECODE", "jfs_read_decode_mode", "jfs_set_read_decode_mode", "jfs_set_read_decode_mode_ext",
     {"full": H["JFS_READ_DECODE_FULL"], "prefix": H["JFS_READ_DECODE_PREFIX"],
      "prefix-all": H["JFS_READ_DECODE_PREFIX_ALL"]}, 2),
    ("JFS_READ_SEEK", "jfs_read_seek_mode", "jfs_set_read_seek_mode", "jfs_set_read_seek_mode_ext",
     {"off": H["JFS_READ_SEEK_OFF"], "on": H["JFS_READ_SEEK_ON"], "sparse": H["JFS_READ_SEEK_SPARSE"]}, 2),
    ("JFS_READ_LZ4_CHASE", "jfs_read_lz4_chase_mode", "jfs_set_read_lz4_chase_mode", None,
     {"off": H["JFS_READ_LZ4_CHASE_OFF"], "on": H["JFS_READ_LZ4_CHASE_ON"]}, 2),
    ("JFS_READ_LZ4_WINDOW", "jfs_read_lz4_window_mode", "jfs_set_read_lz4_window_mode", None,
     {"off": H["JFS_READ_LZ4_WINDOW_OFF"], "on": H["JFS_READ_LZ4_WINDOW_ON"]}, 2),
    ("JFS_ZSTD_PARSE", "jfs_zstd_parse_mode", "jfs_set_zstd_parse_mode", "jfs_set_zstd_parse_mode_ext",
     {"exact": H["JFS_ZSTD_PARSE_EXACT"], "fast": H["JFS_ZSTD_PARSE_FAST"],
      "seekable": H["JFS_ZSTD_PARSE_SEEKABLE"]}, 2),
    ("JFS_ZSTD_SEEK_CSUM", "jfs_zstd_seek_csum_mode", "jfs_set_zstd_seek_csum_mode", None,
     {"off": H["JFS_ZSTD_SEEK_CSUM_OFF"], "on": H["JFS_ZSTD_SEEK_CSUM_ON"]}, 2),
    ("JFS_COMPACT_SPLICE", "jfs_compact_splice_mode", "jfs_set_compact_splice_mode", "jfs_set_compact_splice_mode_ext",
     {"off": H["JFS_COMPACT_SPLICE_OFF"], "on": H["JFS_COMPACT_SPLICE_ON"], "all": H["JFS_COMPACT_SPLICE_ALL"]}, 2),
    ("JFS_COMPACT_LZ4_LIFT", "jfs_compact_lz4_lift_mode", "jfs_set_compact_lz4_lift_mode", None,
     {"off": H["JFS_COMPACT_LZ4_LIFT_OFF"], "on": H["JFS_COMPACT_LZ4_LIFT_ON"]}, 2),
]
# integer: variable, getter, setter, default, closed range
INTS = [
    ("JFS_LZ4_CHASE_MAX", "jfs_lz4_chase_max", "jfs_set_lz4_chase_max", 0, 0, 2**31 - 1),
    ("JFS_ZSTD_SPLIT_FRAMES", "jfs_get_zstd_split_frames", "jfs_set_zstd_split_frames",
     H["JFS_ZSTD_SPLIT_FRAMES_MAX"], 1, H["JFS_ZSTD_SPLIT_FRAMES_MAX"]),
]

# argv[1]: {"get": getter, "sets": [[setter, [values]]]} -> {"get": first value, "sets": [[setter, value, getter
# before, answer, getter after]]}
CHILD = """
import json, sys
from juicefs_amd import _lib as L
lib = L.load()
job = json.loads(sys.argv[1])
get = getattr(lib, job["get"])
out = {"get": get(), "sets": []}
for name, values in job["sets"]:
    for v in values:
        before = get()
        out["sets"].append([name, v, before, getattr(lib, name)(v), get()])
print(json.dumps(out))
"""


def _children(var, getter, values, sets=()):
    """{environment value (None: unset): the child's answer}; the setters run in the child without the variable"""
    procs = {}
    for v in values:
        env = dict(os.environ)
        env.pop(var, None)
        env["JFS_GPU_CODEC"] = "off"
        if v is not None:
            env[var] = v
        job = {"get": getter, "sets": list(sets) if v is None else []}
        procs[v] = subprocess.Popen([sys.executable, "-c", CHILD, json.dumps(job)], env=env, cwd=ROOT,
                                    stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    out = {}
    for v, p in procs.items():
        so, se = p.communicate(timeout=120)
        assert p.returncode == 0, (v, se)
        out[v] = json.loads(so)
    return out


def _mixed(w):
    return "".join(c.upper() if i % 2 else c for i, c in enumerate(w))


def _check_setter(rows, name, accepted):
    """every call of setter `name` in the child: an accepted value answers the previous one and is the new one, any
    other answers -1 and changes nothing"""
    rows = [r for r in rows if r[0] == name]
    assert rows, name
    for _, v, before, ans, after in rows:
        if v in accepted:
            assert (ans, after) == (before, v), (name, v, before, ans, after)
        else:
            assert (ans, after) == (-1, before), (name, v, before, ans, after)
    assert {r[1] for r in rows} >= set(accepted)


def test_parse_functions_under_host_sanitizers(tmp_path):
    """tests/host_modes_main.cc: the table's pure parse functions, ASan + UBSan, nothing loaded into Python"""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    exe = str(tmp_path / "host_modes")
    r = subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "juicefs_amd", "csrc"),
                        os.path.join(ROOT, "tests", "host_modes_main.cc"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    m = re.fullmatch(r"ok (\d+)\n", r.stdout)
    assert m and int(m.group(1)) > 200, r.stdout[-2000:]


@pytest.mark.parametrize("case", ENUMS + INTS, ids=lambda c: c[0])
def test_switch(case):
    if case in ENUMS:
        var, getter, setter, ext, words, nplain = case
        default = next(iter(words.values()))
        every = sorted(words.values())
        assert every == list(range(len(words))) and default == 0
        expect = {None: default, "bogus": default, "1": default, "": default}
        for w, val in words.items():
            assert w == w.lower() and _mixed(w) not in (w, w.upper())
            expect[w] = expect[w.upper()] = expect[_mixed(w)] = val
            expect[w + "x"] = expect[" " + w] = default  # no prefix match, no trimming
        tries = [-1, 0, 1, 2, 3, 1, 0, 7, 2**31 - 1, -2**31]
        sets = [[setter, tries]] + ([[ext, tries]] if ext else [])
        got = _children(var, getter, expect, sets)
        assert {v: g["get"] for v, g in got.items()} == expect
        _check_setter(got[None]["sets"], setter, every[:nplain])
        if ext:
            _check_setter(got[None]["sets"], ext, every)
    else:
        var, getter, setter, default, lo, hi = case
        expect = {None: default, "bogus": default, "": default, "1": 1, str(lo): lo, str(hi): hi, str(lo - 1): default,
                  str(hi + 1): default, "12abc": default, "12 ": default, str(2**70): default}
        mid = (lo + hi) // 2
        tries = [lo - 1, lo, mid, hi, hi + 1, mid, -1, lo]
        got = _children(var, getter, expect, [[setter, tries]])
        assert {v: g["get"] for v, g in got.items()} == expect
        _check_setter(got[None]["sets"], setter, {lo, mid, hi})
