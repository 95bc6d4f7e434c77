#!/usr/bin/env python3
"""The background flatten measured two ways, arms alternated within each repeat, median of
--repeats after 2 warm-ups, timed with a device synchronise and the host clock:

  copy:    k_flatten 4 -> 3 over n RGBA8 frames against the pitched device copy of the same
           source (ik_orient_batch_device with orientation 1); ms and bytes moved per second
           (the copy reads and writes 4 bytes a pixel, the flatten reads 4 and writes 3).
  resize:  ik_resize_batch_device Triangle and Lanczos3 to --out^2 at C = 4 against
           flatten + resize at C = 3: does the flatten pay for itself?

Prints one JSON line per part.

    python tools/flatten_bench.py [--repeats 7] [--small]
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

TRIANGLE, LANCZOS3 = 1, 4


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
    return {"ms_median": round(statistics.median(v), 3), "ms_min": round(min(v), 3), "ms_max": round(max(v), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--small", action="store_true", help="8 frames of 1024^2 to 128^2 (a rehearsal, not a measurement)")
    a = ap.parse_args()
    ik = _lib.load()
    assert ik.ik_device_count() > 0, "no HIP device"
    assert ik.ik_init(0) == 0, _lib.last_error()
    n, S, out = (8, 1024, 128) if a.small else (64, 4096, 512)
    p4, p3 = S * 4, (S * 3 + 255) // 256 * 256  # as ik_image rows
    po4, po3 = out * 4, (out * 3 + 255) // 256 * 256
    src, flat, dst = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
    assert ik.ik_dev_alloc(n * p4 * S, ctypes.byref(src)) == 0, _lib.last_error()
    assert ik.ik_dev_alloc(n * p4 * S, ctypes.byref(flat)) == 0, _lib.last_error()  # the copy's and the flatten's target
    assert ik.ik_dev_alloc(n * po4 * out, ctypes.byref(dst)) == 0, _lib.last_error()
    # a source with every alpha: bytes 0..255 over and over (uploaded once, in pieces)
    piece = bytes(range(256)) * 4096
    for off in range(0, n * p4 * S, len(piece)):
        assert ik.ik_memcpy_h2d(src.value + off, piece, min(len(piece), n * p4 * S - off)) == 0

    def do_copy():
        assert ik.ik_orient_batch_device(src, S, S, 4, 1, p4, p4 * S, n, 1, flat, p4, p4 * S, None) == 0

    def do_flatten():
        assert ik.ik_flatten_batch_device(src, S, S, 4, 1, p4, p4 * S, n, 0xFFFFFF, 3, flat, p3, p3 * S, None) == 0

    ms = alternate(ik, {"copy": do_copy, "flatten": do_flatten}, a.repeats)
    px = float(n) * S * S
    res = {"part": "copy", "n": n, "W": S, "H": S, "repeats": a.repeats}
    for k, moved in (("copy", 8 * px), ("flatten", 7 * px)):
        res[k] = dict(stats(ms[k]), bytes_moved=moved, TBps=round(moved / (statistics.median(ms[k]) * 1e-3) / 1e12, 3))
    res["flatten_to_copy"] = round(res["flatten"]["ms_median"] / res["copy"]["ms_median"], 3)
    print(json.dumps(res), flush=True)

    for filt, name in ((TRIANGLE, "triangle"), (LANCZOS3, "lanczos3")):
        def resize4():
            assert ik.ik_resize_batch_device(src, S, S, 4, p4, p4 * S, n, out, out, filt, dst, po4, po4 * out, None) == 0

        def resize3():
            assert ik.ik_resize_batch_device(flat, S, S, 3, p3, p3 * S, n, out, out, filt, dst, po3, po3 * out, None) == 0

        def flatten_resize3():
            do_flatten()
            resize3()

        do_flatten()  # (resize3 alone reads what the flatten left)
        assert ik.ik_dev_synchronize() == 0
        ms = alternate(ik, {"resize_c4": resize4, "flatten_then_resize_c3": flatten_resize3, "resize_c3": resize3},
                       a.repeats)
        res = {"part": "resize", "filter": name, "n": n, "W": S, "H": S, "out": out, "repeats": a.repeats}
        for k in ms:
            res[k] = stats(ms[k])
        res["flatten_then_resize_c3_to_resize_c4"] = round(
            res["flatten_then_resize_c3"]["ms_median"] / res["resize_c4"]["ms_median"], 3)
        print(json.dumps(res), flush=True)
    for p in (src, flat, dst):
        ik.ik_dev_free(p)


if __name__ == "__main__":
    main()
