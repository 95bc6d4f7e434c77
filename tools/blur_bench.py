#!/usr/bin/env python3
"""Device time of the blur kernel beside the pitched device copy of the same images
(ik_orient_batch_device with orientation 1: the memory floor), arms alternated within each
repeat, median of --repeats after 2 warm-ups of every arm, each timed with a device
synchronise and the host clock (so a figure includes one launch and one synchronise):

  64 x 512^2 RGB    the post-resize shape of the headline batch, sigma 1 and sigma 8
  8 x 4096^2 RGBA   sigma 1

Both the blur and the unsharpen variant are timed.  Prints one JSON line per case.

    python tools/blur_bench.py [--repeats 9] [--small]
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
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--small", action="store_true", help="4 x 256^2 and 2 x 512^2 (a rehearsal, not a measurement)")
    a = ap.parse_args()
    ik = _lib.load()
    assert ik.ik_device_count() > 0, "no HIP device"
    assert ik.ik_init(0) == 0, _lib.last_error()
    cases = [(64, 512, 3, (1.0, 8.0)), (8, 4096, 4, (1.0,))]
    if a.small:
        cases = [(4, 256, 3, (1.0, 8.0)), (2, 512, 4, (1.0,))]
    for n, S, C, sigmas in cases:
        pitch = (S * C + 255) // 256 * 256  # as ik_image rows
        total = n * pitch * S
        src, dst = ctypes.c_void_p(), ctypes.c_void_p()
        assert ik.ik_dev_alloc(total, ctypes.byref(src)) == 0, _lib.last_error()
        assert ik.ik_dev_alloc(total, ctypes.byref(dst)) == 0, _lib.last_error()
        piece = bytes((i * 37 + (i >> 8) * 11) & 0xFF for i in range(1 << 20))
        for off in range(0, total, len(piece)):
            assert ik.ik_memcpy_h2d(src.value + off, piece, min(len(piece), total - off)) == 0

        def do_copy():
            assert ik.ik_orient_batch_device(src, S, S, C, 1, pitch, pitch * S, n, 1, dst, pitch, pitch * S, None) == 0

        arms = {"copy": do_copy}
        for sigma in sigmas:
            for sharpen in (0, 1):
                def do_blur(sigma=sigma, sharpen=sharpen):
                    assert ik.ik_blur_batch_device(src, S, S, C, 1, pitch, pitch * S, n, sigma, sharpen, 2, dst, pitch,
                                                   pitch * S, None) == 0, _lib.last_error()
                arms[("unsharpen" if sharpen else "blur") + "_sigma%g" % sigma] = do_blur
        ms = alternate(ik, arms, a.repeats)
        moved = 2.0 * n * S * S * C  # bytes read plus bytes written, either arm
        res = {"n": n, "W": S, "H": S, "C": C, "repeats": a.repeats, "bytes_moved": moved}
        for k in ms:
            res[k] = dict(stats(ms[k]), TBps=round(moved / (statistics.median(ms[k]) * 1e-3) / 1e12, 3))
            if k != "copy":
                res[k]["to_copy"] = round(statistics.median(ms[k]) / statistics.median(ms["copy"]), 2)
        print(json.dumps(res), flush=True)
        ik.ik_dev_free(src)
        ik.ik_dev_free(dst)


if __name__ == "__main__":
    main()
