#!/usr/bin/env python3
"""The pad kernel against the pitched device copy of the CANVAS's bytes on the same stream
(ik_orient_batch_device with orientation 1 over canvas-sized areas), arms alternated within
each repeat, median of --repeats after 2 warm-ups, timed with a device synchronise and the
host clock.  The pad writes what the copy writes and reads less (the image, not the canvas;
in colour mode the frame reads nothing), so the copy is the yardstick.

  64 x (512 x 288 -> 512^2) RGB8      the headline's post-resize shape, letterboxed: colour, mirror
  8 x (4096 x 2304 -> 4096^2) RGBA8   colour, mirror
  64 x (288 x 512 -> 511 x 512) RGB8  bars at the sides, the interior off the dword grid; mirror's
  8 x (2304 x 4096 -> 4096^2) RGBA8   frame goes through the index map

Prints one JSON line per shape.

    python tools/pad_bench.py [--repeats 9] [--small]
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

MODES = {"color": 1, "edge": 2, "mirror": 3, "wrap": 4}


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


def shape(ik, n, W, H, cw, ch, C, depth, names, repeats):
    px = C * depth
    sp = (W * px + 255) // 256 * 256  # as ik_image rows
    dp = (cw * px + 255) // 256 * 256
    src, dst, cpy = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
    assert ik.ik_dev_alloc(n * sp * H, ctypes.byref(src)) == 0, _lib.last_error()
    assert ik.ik_dev_alloc(n * dp * ch, ctypes.byref(dst)) == 0, _lib.last_error()
    assert ik.ik_dev_alloc(n * dp * ch, ctypes.byref(cpy)) == 0, _lib.last_error()
    # every byte value, in an order that does not repeat along a row (uploaded once, in pieces)
    piece = bytes((i * 151 + (i >> 8) * 7) & 255 for i in range(1 << 20))
    for base, total in ((src, n * sp * H), (cpy, n * dp * ch)):
        for off in range(0, total, len(piece)):
            assert ik.ik_memcpy_h2d(base.value + off, piece, min(len(piece), total - off)) == 0

    def do_copy():  # the canvas's bytes, from one canvas-sized area to another
        assert ik.ik_orient_batch_device(cpy, cw, ch, C, depth, dp, dp * ch, n, 1, dst, dp, dp * ch, None) == 0

    arms = {"copy": do_copy}
    keep = []
    for name in names:
        p = _lib.Pad(MODES[name], 0, 0, 0, 0xFFFFFF, 255)
        keep.append(p)
        arms[name] = (lambda p=p: ik.ik_pad_batch_device(src, W, H, C, depth, sp, sp * H, n, ctypes.byref(p), cw, ch,
                                                         dst, dp, dp * ch, None))
    c0 = (ctypes.c_ulonglong * 2)()
    ik.ik_pad_counters(c0)
    ms = alternate(ik, arms, repeats)
    c1 = (ctypes.c_ulonglong * 2)()
    ik.ik_pad_counters(c1)
    assert c1[0] - c0[0] == len(names) * (repeats + 2), "a pad arm did not launch"
    written = float(n * cw * ch * px)
    res = {"n": n, "W": W, "H": H, "cw": cw, "ch": ch, "C": C, "depth": depth, "repeats": repeats,
           "canvas_bytes": written}
    for k in ms:
        res[k] = dict(stats(ms[k]), canvas_TBps=round(written / (statistics.median(ms[k]) * 1e-3) / 1e12, 3))
        if k != "copy":
            res[k]["to_copy"] = round(res[k]["ms_median"] / res["copy"]["ms_median"], 3)
    print(json.dumps(res), flush=True)
    for p in (src, dst, cpy):
        ik.ik_dev_free(p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--small", action="store_true", help="a quarter of each side (a rehearsal, not a measurement)")
    a = ap.parse_args()
    ik = _lib.load()
    assert ik.ik_device_count() > 0, "no HIP device"
    assert ik.ik_init(0) == 0, _lib.last_error()
    d = 4 if a.small else 1
    shape(ik, 64, 512 // d, 288 // d, 512 // d, 512 // d, 3, 1, ("color", "mirror"), a.repeats)
    shape(ik, 8, 4096 // d, 2304 // d, 4096 // d, 4096 // d, 4, 1, ("color", "mirror"), a.repeats)
    # bars at the sides: the interior starts off the dword grid in RGB8, and mirror's frame is gathered
    shape(ik, 64, 288 // d, 512 // d, 512 // d - 1, 512 // d, 3, 1, ("color", "mirror"), a.repeats)
    shape(ik, 8, 2304 // d, 4096 // d, 4096 // d, 4096 // d, 4, 1, ("color", "mirror"), a.repeats)


if __name__ == "__main__":
    main()
