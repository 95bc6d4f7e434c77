#!/usr/bin/env python3
"""The watermark overlay against a device-to-device copy of the same window bytes, arms
alternated within each repeat, median of --repeats after 2 warm-ups, timed with a device
synchronise and the host clock (a launch and its synchronise cost some tens of microseconds,
which is what a small window measures):

  corner:   64 x 512^2 RGB8 under a 128 x 32 RGBA8 mark in the SE corner
  tiled:    the same mark tiled over the same frames
  rgba:     8 x 4096^2 RGBA8 under the mark tiled (the base's alpha: the u32 division by D)
  rgba16:   4 x 2048^2 RGBA16 under the mark tiled (the u64 division by D; reported only)

The copy moves the window's bytes of every frame once (read and write), pitched, from a
second area (ik_orient_batch_device with orientation 1 over the window); the overlay reads
and writes them in place.  Prints one JSON line per case.

    python tools/overlay_bench.py [--repeats 9] [--small]
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

SE, NW = 7, 6


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--small", action="store_true", help="fewer, smaller frames (a rehearsal, not a measurement)")
    a = ap.parse_args()
    ik = _lib.load()
    assert ik.ik_device_count() > 0, "no HIP device"
    assert ik.ik_init(0) == 0, _lib.last_error()
    mw, mh = 128, 32
    mark = ctypes.c_void_p()
    assert ik.ik_dev_alloc(mw * mh * 4, ctypes.byref(mark)) == 0, _lib.last_error()
    mbytes = bytes((i * 37 + (i >> 2)) & 255 for i in range(mw * mh * 4))  # every alpha, fixed
    assert ik.ik_memcpy_h2d(mark, mbytes, len(mbytes)) == 0
    k = 4 if a.small else 1
    cases = [("corner", 64 // k, 512, 3, 1, SE, 0), ("tiled", 64 // k, 512, 3, 1, NW, 1),
             ("rgba", 8 // k, 4096 // k, 4, 1, NW, 1), ("rgba16", 4 // k, 2048 // k, 4, 2, NW, 1)]
    for name, n, S, C, depth, g, tile in cases:
        pitch = (S * C * depth + 255) // 256 * 256  # as ik_image rows
        base, other = ctypes.c_void_p(), ctypes.c_void_p()
        assert ik.ik_dev_alloc(n * pitch * S, ctypes.byref(base)) == 0, _lib.last_error()
        assert ik.ik_dev_alloc(n * pitch * S, ctypes.byref(other)) == 0, _lib.last_error()
        piece = bytes(range(256)) * 4096
        for off in range(0, n * pitch * S, len(piece)):
            assert ik.ik_memcpy_h2d(base.value + off, piece, min(len(piece), n * pitch * S - off)) == 0
        pl = (ctypes.c_int32 * 6)()
        assert ik.ik_overlay_place(S, S, mw, mh, g, 0, 0, tile, pl) == 0
        wx, wy, ww, wh = pl[0], pl[1], pl[2], pl[3]
        woff = wy * pitch + wx * C * depth

        def do_copy():  # the window's bytes of every frame, from the other area into this one
            assert ik.ik_orient_batch_device(other.value + woff, ww, wh, C, depth, pitch, pitch * S, n, 1,
                                             base.value + woff, pitch, pitch * S, None) == 0

        def do_overlay():
            assert ik.ik_overlay_batch_device(base, S, S, C, depth, pitch, pitch * S, n, mark, mw, mh, 4, 1, mw * 4, g,
                                              0, 0, 200, tile, None) == 0, _lib.last_error()

        ms = alternate(ik, {"copy": do_copy, "overlay": do_overlay}, a.repeats)
        moved = 2.0 * n * ww * wh * C * depth
        res = {"case": name, "n": n, "W": S, "H": S, "C": C, "depth": depth, "window": [wx, wy, ww, wh],
               "repeats": a.repeats, "window_bytes_read_and_written": moved}
        for arm in ms:
            res[arm] = dict(stats(ms[arm]), TBps=round(moved / (statistics.median(ms[arm]) * 1e-3) / 1e12, 3))
        res["overlay_to_copy"] = round(res["overlay"]["ms_median"] / res["copy"]["ms_median"], 3)
        print(json.dumps(res), flush=True)
        ik.ik_dev_free(base)
        ik.ik_dev_free(other)
    ik.ik_dev_free(mark)


if __name__ == "__main__":
    main()
