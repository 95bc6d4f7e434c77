#!/usr/bin/env python3
"""The colour adjustment kernel against the pitched device copy of the same bytes on the same
stream (ik_orient_batch_device with orientation 1), arms alternated within each repeat, median
of --repeats after 2 warm-ups, timed with a device synchronise and the host clock.  The kernel
works in place: it reads and writes what the copy reads and writes, so the copy is the
yardstick.

  64 x 512^2 RGB8     the headline's post-resize shape: matrix (grayscale), table, both
  8 x 4096^2 RGBA8    matrix only, table only, both
  8 x 4096^2 RGBA16   the table alone: the global gather

Prints one JSON line per shape.

    python tools/adjust_bench.py [--repeats 7] [--small]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "rust-image-transform_amd"))
from imagekit import _lib  # noqa: E402

ARMS = {
    "matrix": (0, 0, -100, 0, 0.0, 0),
    "table": (10, 20, 0, 0, 2.2, 0),
    "both": (10, 20, 60, 75, 2.2, 0),
}


def timed(ik, fn):
    t0 = time.perf_counter()
    fn()
    assert ik.ik_dev_synchronize() == 0
    return (time.perf_counter() - t0) * 1e3


def alternate(ik, arms, repeats):
    """{name: [ms]}: two warm-ups of every arm, then the arms in turn within each repeat"""
    for fn in arms.values():
        timed(ik, fn)
        timed(ik, fn)
    ms = {k: [] for k in arms}
    for _ in range(repeats):
        for k, fn in arms.items():
            ms[k].append(timed(ik, fn))
    return ms


def stats(v):
    return {"ms_median": round(statistics.median(v), 4), "ms_min": round(min(v), 4), "ms_max": round(max(v), 4)}


def shape(ik, n, S, C, depth, names, repeats):
    pitch = (S * C * depth + 255) // 256 * 256  # as ik_image rows
    total = n * pitch * S
    src, dst = ctypes.c_void_p(), ctypes.c_void_p()
    assert ik.ik_dev_alloc(total, ctypes.byref(src)) == 0, _lib.last_error()
    assert ik.ik_dev_alloc(total, ctypes.byref(dst)) == 0, _lib.last_error()
    # every byte value, in an order that does not repeat along a row (uploaded once, in pieces)
    piece = bytes((i * 151 + (i >> 8) * 7) & 255 for i in range(1 << 20))
    for off in range(0, total, len(piece)):
        assert ik.ik_memcpy_h2d(src.value + off, piece, min(len(piece), total - off)) == 0

    def do_copy():
        assert ik.ik_orient_batch_device(src, S, S, C, depth, pitch, pitch * S, n, 1, dst, pitch, pitch * S, None) == 0

    arms = {"copy": do_copy}
    keep = []
    for name in names:
        a = _lib.Adjust(*ARMS[name])
        keep.append(a)
        arms[name] = (lambda a=a: ik.ik_adjust_batch_device(src, S, S, C, depth, pitch, pitch * S, n, ctypes.byref(a), None))
    c0 = (ctypes.c_ulonglong * 2)()
    ik.ik_adjust_counters(c0)
    ms = alternate(ik, arms, repeats)
    c1 = (ctypes.c_ulonglong * 2)()
    ik.ik_adjust_counters(c1)
    assert c1[0] - c0[0] == len(names) * (repeats + 2), "an adjust arm did not launch"
    moved = 2.0 * n * S * S * C * depth
    res = {"n": n, "W": S, "H": S, "C": C, "depth": depth, "repeats": repeats, "bytes_moved": moved}
    for k in ms:
        res[k] = dict(stats(ms[k]), TBps=round(moved / (statistics.median(ms[k]) * 1e-3) / 1e12, 3))
        if k != "copy":
            res[k]["to_copy"] = round(res[k]["ms_median"] / res["copy"]["ms_median"], 3)
    print(json.dumps(res), flush=True)
    for p in (src, dst):
        ik.ik_dev_free(p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--small", action="store_true", help="a quarter of each side (a rehearsal, not a measurement)")
    a = ap.parse_args()
    ik = _lib.load()
    assert ik.ik_device_count() > 0, "no HIP device"
    assert ik.ik_init(0) == 0, _lib.last_error()
    d = 4 if a.small else 1
    shape(ik, 64, 512 // d, 3, 1, ("matrix", "table", "both"), a.repeats)
    shape(ik, 8, 4096 // d, 4, 1, ("matrix", "table", "both"), a.repeats)
    shape(ik, 8, 4096 // d, 4, 2, ("table",), a.repeats)


if __name__ == "__main__":
    main()
