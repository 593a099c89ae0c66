"""The run-time switches and counters of libjfsgpu.so, each described once.

ENUMS, INTS and COUNTERS are the Python side of juicefs_amd/csrc/host_modes.h:
``_lib.load()`` declares the C prototypes from them, and the loops below build
the public getters, setters, context managers and counter readers, which
``compress`` and ``device`` re-export under the names they always had.  A new
switch is one record here.
"""
from __future__ import annotations

import contextlib
import ctypes
import inspect
from typing import Callable, NamedTuple

from . import _lib as L


class Enum(NamedTuple):
    """An enumerated switch.  `get`, `set` and `hold` are the Python names of its
    getter, its setter and its context manager (None: not public)."""
    getter: str
    setter: str
    ext: str | None  # the setter that takes every value, where the plain one stops at the first two
    words: dict  # {spelling: value}, the default first
    phrase: str  # in error messages
    get: str | None
    set: str | None
    hold: str | None
    doc: str


class Int(NamedTuple):
    """An integer switch over the closed range [lo, hi]."""
    getter: str
    setter: str
    ctype: type
    lo: int
    hi: int


class Counter(NamedTuple):
    """`words` uint64 counters behind int f(uint64_t *out, int reset)."""
    cname: str
    words: int
    doc: str
    post: Callable = lambda out: tuple(int(x) for x in out)


ENUMS = [
    Enum("jfs_lz4_parse_mode", "jfs_set_lz4_parse_mode", None,
         {"exact": L.LZ4_PARSE_EXACT, "fast": L.LZ4_PARSE_FAST}, "lz4 parse mode",
         None, None, "lz4_parse_mode",
         """The LZ4 parse of the host-buffer compress calls (jfs_lz4_parse_mode):
         "exact" (LZ4_compress_default's bytes) or "fast"
         (jfs_lz4_compress_fast_device's blocks)."""),
    Enum("jfs_zstd_parse_mode", "jfs_set_zstd_parse_mode", "jfs_set_zstd_parse_mode_ext",
         {"exact": L.ZSTD_PARSE_EXACT, "fast": L.ZSTD_PARSE_FAST, "seekable": L.ZSTD_PARSE_SEEKABLE},
         "zstd parse mode", None, "set_zstd_parse_mode", "zstd_parse_mode",
         """The Zstd parse of the host-buffer compress calls (jfs_zstd_parse_mode):
         "exact" (ZSTD_compress level 1's bytes), "fast"
         (jfs_zstd_compress_fast_device's frames), or "seekable" -- the fast parse
         laid out as one frame per 128 KiB block and a seek table
         (jfs_zstd_compress_seekable_device's objects)."""),
    Enum("jfs_read_decode_mode", "jfs_set_read_decode_mode", "jfs_set_read_decode_mode_ext",
         {"full": L.READ_DECODE_FULL, "prefix": L.READ_DECODE_PREFIX, "prefix-all": L.READ_DECODE_PREFIX_ALL},
         "read decode mode", "read_decode_mode", "set_read_decode_mode", None,
         """The decode mode of the read calls (jfs_read_decode_mode): "full", or
         "prefix" -- every LZ4 decode stops at the last byte a read needs, or
         "prefix-all" -- so does every Zstd decode, at the Zstd block that holds it."""),
    Enum("jfs_read_seek_mode", "jfs_set_read_seek_mode", "jfs_set_read_seek_mode_ext",
         {"off": L.READ_SEEK_OFF, "on": L.READ_SEEK_ON, "sparse": L.READ_SEEK_SPARSE},
         "read seek mode", "read_seek_mode", "set_read_seek_mode", None,
         """The seek switch of the read calls (jfs_read_seek_mode): "off", or "on" --
         every Zstd source is decoded through its seek table for the byte range the
         reads ask of it (an object without one: prefix-decoded to their end), or
         "sparse" -- for the list of ranges the reads ask of it, exactly the frames
         they touch, tables with checksums read and verified too."""),
    Enum("jfs_read_lz4_chase_mode", "jfs_set_read_lz4_chase_mode", None,
         {"off": L.READ_LZ4_CHASE_OFF, "on": L.READ_LZ4_CHASE_ON},
         "read lz4 chase mode", "read_lz4_chase_mode", "set_read_lz4_chase_mode", None,
         """The LZ4 chase switch of the read calls (jfs_read_lz4_chase_mode): "off",
         or "on" -- an LZ4 source whose reads ask for at most lz4_chase_max() bytes
         is decoded for exactly those bytes by the origin chase."""),
    Enum("jfs_read_lz4_window_mode", "jfs_set_read_lz4_window_mode", None,
         {"off": L.READ_LZ4_WINDOW_OFF, "on": L.READ_LZ4_WINDOW_ON},
         "read lz4 window mode", "read_lz4_window_mode", "set_read_lz4_window_mode", None,
         """The LZ4 window switch of the read calls (jfs_read_lz4_window_mode):
         "off", or "on" -- an LZ4 source of a small batch is decoded from the 64 KiB
         chunk its reads start in, where the block's sequences allow it."""),
    Enum("jfs_zstd_seek_csum_mode", "jfs_set_zstd_seek_csum_mode", None,
         {"off": L.ZSTD_SEEK_CSUM_OFF, "on": L.ZSTD_SEEK_CSUM_ON},
         "zstd seek checksum mode", "zstd_seek_csum_mode", "set_zstd_seek_csum_mode", None,
         """The checksum switch of the seekable parse mode (jfs_zstd_seek_csum_mode):
         "off", or "on" -- while the Zstd parse mode is "seekable" the compress calls
         write seek tables with a checksum per frame."""),
    Enum("jfs_compact_splice_mode", "jfs_set_compact_splice_mode", "jfs_set_compact_splice_mode_ext",
         {"off": L.COMPACT_SPLICE_OFF, "on": L.COMPACT_SPLICE_ON, "all": L.COMPACT_SPLICE_ALL},
         "compact splice mode", "compact_splice_mode", "set_compact_splice_mode", None,
         """The splice switch of the Zstd compaction call (jfs_compact_splice_mode):
         "off", or "on" -- while the Zstd parse mode is "seekable", a 128 KiB piece
         of an output that is exactly one frame of a seekable source is copied as
         stored bytes, and only the other pieces are decoded and re-encoded; or
         "all" -- "on", and the sealed compaction call splices too, from seek tables
         it lifts out of the sources once they are opened on the device."""),
    Enum("jfs_compact_lz4_lift_mode", "jfs_set_compact_lz4_lift_mode", None,
         {"off": L.COMPACT_LZ4_LIFT_OFF, "on": L.COMPACT_LZ4_LIFT_ON},
         "compact lz4 lift mode", "compact_lz4_lift_mode", "set_compact_lz4_lift_mode", None,
         """The LZ4 lift switch of the compaction calls (jfs_compact_lz4_lift_mode):
         "off", or "on" -- while the LZ4 parse mode is "fast", an output chunk that is
         one whole 64 KiB chunk of one source takes its sequence records from the
         source's stored stream instead of being parsed again; the bytes do not change."""),
]

LZ4_CHASE_MAX = Int("jfs_lz4_chase_max", "jfs_set_lz4_chase_max", ctypes.c_int64, 0, 2**31 - 1)
ZSTD_SPLIT_FRAMES = Int("jfs_get_zstd_split_frames", "jfs_set_zstd_split_frames", ctypes.c_int, 1,
                        L.ZSTD_SPLIT_FRAMES_MAX)
INTS = [LZ4_CHASE_MAX, ZSTD_SPLIT_FRAMES]

COUNTERS = [
    Counter("jfs_lz4_split_counts", 6,
            """(blocks the small-batch path decoded itself, blocks it handed to the
            one-workgroup kernel, ... the reasons: fix-up, jumping, token, no last run)
            on the current device."""),
    Counter("jfs_zstd_split_counts", 2,
            """(inputs the Zstd small-batch path replayed itself, inputs it handed to
            the exact one-wave replay) on the current device."""),
    Counter("jfs_zstd_split_frame_counts", 2,
            """(multi-frame inputs -- two frames or more -- the Zstd small-batch path
            replayed itself, the frames they held) on the current device."""),
    Counter("jfs_lz4_eseg_counts", 17,
            """Segment encoder: {rounds: blocks settled after that many rounds}, with
            0 = blocks handed to the serial kernel.""",
            lambda out: {i: int(x) for i, x in enumerate(out) if x}),
    Counter("jfs_lz4_window_counts", 4,
            """(blocks the window decode took from a floor above 0, blocks whose probe
            sent them to floor 0, blocks handed to the exact kernel, origin entries
            written) on the current device."""),
    Counter("jfs_lz4_chase_counts", 4,
            """(blocks the origin chase resolved, bytes requested of them, chain steps
            taken, blocks handed to the prefix path) on the current device."""),
    Counter("jfs_zstd_sparse_counts", 3,
            """(inputs the ranges decode took through a seek table, frames it selected,
            frames whose checksum it compared) on the current device."""),
    Counter("jfs_compact_splice_counts", 4,
            """(outputs spliced, frames passed, frames re-encoded inside spliced
            outputs, compressed bytes passed) since the last reset."""),
    Counter("jfs_compact_lz4_lift_counts", 4,
            """(calls that took the lift, candidate chunks planned, chunks lifted,
            candidates the device refused and parsed) since the last reset."""),
]


def _enum_api(sw: Enum):
    """(getter, setter, context manager) of one enumerated switch"""
    names = {v: k for k, v in sw.words.items()}
    quoted = [repr(w) for w in sw.words]
    expected = ", ".join(quoted[:-1]) + " or " + quoted[-1]
    via = sw.ext or sw.setter
    doc = inspect.cleandoc(sw.doc)

    def get() -> str:
        return names[getattr(L.load(), sw.getter)()]

    def set_(mode: str) -> str:
        if mode not in sw.words:
            raise ValueError(f"{sw.phrase} {mode!r}: expected {expected}")
        return names[getattr(L.load(), via)(sw.words[mode])]

    @contextlib.contextmanager
    def hold(mode: str):
        prev = set_(mode)
        try:
            yield
        finally:
            set_(prev)

    get.__doc__ = doc
    set_.__doc__ = (f"Set the {sw.phrase} (process-wide, for calls that start afterwards; {via}) and\n"
                    f"return the previous mode's name.\n\n{doc}")
    hold.__doc__ = (f"Hold the {sw.phrase} at `mode` and put the previous mode back on exit, also when\n"
                    f"the body raises.  The mode is process-wide ({via}).\n\n{doc}")
    return get, set_, hold


def _counter_api(c: Counter):
    def counts(reset: bool = False):
        out = (ctypes.c_uint64 * c.words)()
        rc = getattr(L.load(), c.cname)(out, 1 if reset else 0)
        if rc != 0:
            raise RuntimeError(f"{c.cname} failed: {rc}")
        return c.post(out)

    counts.__doc__ = inspect.cleandoc(c.doc)
    return counts


def _publish(name: str, fn):
    fn.__name__ = fn.__qualname__ = name
    globals()[name] = fn


# `from .switches import *` gives compress the switches; the counter readers are imported by name (compress, device)
__all__ = ["lz4_chase_max", "set_lz4_chase_max", "zstd_split_frames", "set_zstd_split_frames"]
for _sw in ENUMS:
    for _name, _fn in zip((_sw.get, _sw.set, _sw.hold), _enum_api(_sw)):
        if _name:
            _publish(_name, _fn)
            __all__.append(_name)
for _c in COUNTERS:
    _publish(_c.cname[len("jfs_"):], _counter_api(_c))


def lz4_chase_max() -> int:
    """The most bytes the reads may ask of one LZ4 source for it to take the
    chase (jfs_lz4_chase_max; JFS_LZ4_CHASE_MAX, default 0)."""
    return int(L.load().jfs_lz4_chase_max())


def set_lz4_chase_max(nbytes: int) -> int:
    """Set it (jfs_set_lz4_chase_max) and return the previous value."""
    prev = int(L.load().jfs_set_lz4_chase_max(int(nbytes)))
    if prev < 0:
        raise ValueError(f"lz4 chase max {nbytes!r}: expected 0 .. 2^31 - 1")
    return prev


def zstd_split_frames() -> int:
    """The most frames a Zstd input may hold for the small-batch decode path to
    replay it block-parallel (jfs_get_zstd_split_frames; default 16384)."""
    return L.load().jfs_get_zstd_split_frames()


def set_zstd_split_frames(n: int) -> int:
    """Set it (process-wide, for launches enqueued afterwards) and return the
    previous value; 1 hands every multi-frame input to the one-wave replay."""
    lo, hi = ZSTD_SPLIT_FRAMES.lo, ZSTD_SPLIT_FRAMES.hi
    if not isinstance(n, int) or isinstance(n, bool) or not lo <= n <= hi:
        raise ValueError(f"zstd split frames {n!r}: expected an int in [{lo}, {hi}]")
    return L.load().jfs_set_zstd_split_frames(n)
