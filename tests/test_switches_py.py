"""The Python names of the run-time switches (juicefs_amd.compress), without a GPU:
what each getter answers by default, what each setter takes, answers and refuses,
and that the context managers put the previous mode back.  The spellings, defaults
and messages are written out here, from include/jfs_gpucodec.h and the functions'
documentation -- not read from the package's table.  The switches are process-wide,
so every case runs this file as a script in a child process of its own
(JFS_GPU_CODEC=off: no device is touched; the switch's variable unset).  The C
getter is the witness throughout, so a Python getter and setter cannot agree on
a wrong answer.  Only the two parse modes have a public context manager."""
import json
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, "include", "jfs_gpucodec.h")) as _f:
    H = {k: int(v) for k, v in re.findall(r"^#define (JFS_\w+) (\d+)\b", _f.read(), re.M)}

# variable, C getter, Python getter / setter / context manager (None: there is none), {spelling: value} (the first is
# the default), what a refusal says after the offending word
ENUMS = [
    ("JFS_LZ4_PARSE", "jfs_lz4_parse_mode", None, None, "lz4_parse_mode",
     {"exact": H["JFS_LZ4_PARSE_EXACT"], "fast": H["JFS_LZ4_PARSE_FAST"]},
     "lz4 parse mode {!r}: expected 'exact' or 'fast'"),
    ("JFS_ZSTD_PARSE", "jfs_zstd_parse_mode", None, "set_zstd_parse_mode", "zstd_parse_mode",
     {"exact": H["JFS_ZSTD_PARSE_EXACT"], "fast": H["JFS_ZSTD_PARSE_FAST"], "seekable": H["JFS_ZSTD_PARSE_SEEKABLE"]},
     "zstd parse mode {!r}: expected 'exact', 'fast' or 'seekable'"),
    ("JFS_READ_DECODE", "jfs_read_decode_mode", "read_decode_mode", "set_read_decode_mode", None,
     {"full": H["JFS_READ_DECODE_FULL"], "prefix": H["JFS_READ_DECODE_PREFIX"],
      "prefix-all": H["JFS_READ_DECODE_PREFIX_ALL"]},
     "read decode mode {!r}: expected 'full', 'prefix' or 'prefix-all'"),
    ("JFS_READ_SEEK", "jfs_read_seek_mode", "read_seek_mode", "set_read_seek_mode", None,
     {"off": H["JFS_READ_SEEK_OFF"], "on": H["JFS_READ_SEEK_ON"], "sparse": H["JFS_READ_SEEK_SPARSE"]},
     "read seek mode {!r}: expected 'off', 'on' or 'sparse'"),
    ("JFS_READ_LZ4_CHASE", "jfs_read_lz4_chase_mode", "read_lz4_chase_mode", "set_read_lz4_chase_mode", None,
     {"off": H["JFS_READ_LZ4_CHASE_OFF"], "on": H["JFS_READ_LZ4_CHASE_ON"]},
     "read lz4 chase mode {!r}: expected 'off' or 'on'"),
    ("JFS_READ_LZ4_WINDOW", "jfs_read_lz4_window_mode", "read_lz4_window_mode", "set_read_lz4_window_mode", None,
     {"off": H["JFS_READ_LZ4_WINDOW_OFF"], "on": H["JFS_READ_LZ4_WINDOW_ON"]},
     "read lz4 window mode {!r}: expected 'off' or 'on'"),
    ("JFS_ZSTD_SEEK_CSUM", "jfs_zstd_seek_csum_mode", "zstd_seek_csum_mode", "set_zstd_seek_csum_mode", None,
     {"off": H["JFS_ZSTD_SEEK_CSUM_OFF"], "on": H["JFS_ZSTD_SEEK_CSUM_ON"]},
     "zstd seek checksum mode {!r}: expected 'off' or 'on'"),
    ("JFS_COMPACT_SPLICE", "jfs_compact_splice_mode", "compact_splice_mode", "set_compact_splice_mode", None,
     {"off": H["JFS_COMPACT_SPLICE_OFF"], "on": H["JFS_COMPACT_SPLICE_ON"], "all": H["JFS_COMPACT_SPLICE_ALL"]},
     "compact splice mode {!r}: expected 'off', 'on' or 'all'"),
    ("JFS_COMPACT_LZ4_LIFT", "jfs_compact_lz4_lift_mode", "compact_lz4_lift_mode", "set_compact_lz4_lift_mode", None,
     {"off": H["JFS_COMPACT_LZ4_LIFT_OFF"], "on": H["JFS_COMPACT_LZ4_LIFT_ON"]},
     "compact lz4 lift mode {!r}: expected 'off' or 'on'"),
]
# variable, C getter, Python getter / setter, default, values it takes, values it refuses, what a refusal says
INTS = [
    ("JFS_LZ4_CHASE_MAX", "jfs_lz4_chase_max", "lz4_chase_max", "set_lz4_chase_max", 0,
     [0, 1, 4096, 2**31 - 1, 0], [-1, 2**31, -2**31],
     "lz4 chase max {!r}: expected 0 .. 2^31 - 1"),
    ("JFS_ZSTD_SPLIT_FRAMES", "jfs_get_zstd_split_frames", "zstd_split_frames", "set_zstd_split_frames",
     H["JFS_ZSTD_SPLIT_FRAMES_MAX"], [1, 2, 8192, H["JFS_ZSTD_SPLIT_FRAMES_MAX"]],
     [0, -1, H["JFS_ZSTD_SPLIT_FRAMES_MAX"] + 1, True, 2.0, "2", None],
     "zstd split frames {!r}: expected an int in [1, %d]" % H["JFS_ZSTD_SPLIT_FRAMES_MAX"]),
]


def _refused(call, arg, message, witness):
    """call(arg) raises ValueError with exactly `message` and leaves the witness's answer alone"""
    before = witness()
    try:
        call(arg)
    except ValueError as e:
        assert str(e) == message.format(arg), (str(e), message.format(arg))
    else:
        raise AssertionError(f"{arg!r} was taken")
    assert witness() == before, (arg, before, witness())


class _Body(Exception):
    pass


def _child_enum(C, lib, cget, get, set_, hold, words, message):
    witness = getattr(lib, cget)
    default = next(iter(words))
    assert words[default] == 0 and witness() == 0, (words, witness())
    bad = ["bogus", default.upper(), default + " ", "", "1"]
    if get:
        assert getattr(C, get)() == default
    if set_:
        prev = default
        for w in list(words) + list(reversed(words)):
            assert getattr(C, set_)(w) == prev, (w, prev)
            assert witness() == words[w], (w, witness())
            if get:
                assert getattr(C, get)() == w
            for b in bad:
                _refused(getattr(C, set_), b, message, witness)
            prev = w
        assert prev == default
    if hold:
        cm = getattr(C, hold)
        for outer in words:
            for inner in words:
                with pytest.raises(_Body):
                    with cm(outer):
                        assert witness() == words[outer]
                        with pytest.raises(_Body):
                            with cm(inner):
                                assert witness() == words[inner]
                                raise _Body()
                        assert witness() == words[outer], (outer, inner, witness())
                        raise _Body()
                assert witness() == 0, (outer, inner, witness())
            with cm(outer):  # and after a body that ends well
                assert witness() == words[outer]
            assert witness() == 0
        for b in bad:
            _refused(lambda m: cm(m).__enter__(), b, message, witness)


def _child_int(C, lib, cget, get, set_, default, good, refused, message):
    witness = getattr(lib, cget)
    assert witness() == default and getattr(C, get)() == default
    prev = default
    for v in good:
        assert getattr(C, set_)(v) == prev, (v, prev)
        assert witness() == v and getattr(C, get)() == v
        for r in refused:
            _refused(getattr(C, set_), r, message, witness)
        prev = v


@pytest.mark.parametrize("case", ENUMS + INTS, ids=lambda c: c[0])
def test_python_switch(case):
    env = dict(os.environ)
    env.pop(case[0], None)
    env["JFS_GPU_CODEC"] = "off"
    r = subprocess.run([sys.executable, os.path.abspath(__file__), json.dumps(case)], env=env, cwd=ROOT,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout == "ok\n", r.stdout[-2000:] + r.stderr[-4000:]


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    from juicefs_amd import _lib, compress
    job = json.loads(sys.argv[1])
    assert job[0] not in os.environ
    (_child_enum if isinstance(job[5], dict) else _child_int)(compress, _lib.load(), *job[1:])
    print("ok")
