#!/usr/bin/env python3
"""The orient kernels against a device-to-device pitched copy of the same bytes
(ik_orient_batch_device with orientation 1 is hipMemcpy2DAsync per image, on the same
stream): ms, achieved TB/s (one read and one write of the images) and the ratio to the
copy, arms alternated within each repeat.  Prints one JSON line per geometry.

    python tools/orient_bench.py [--repeats 7] [--small]
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

KINDS = (1, 2, 3, 6, 7)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--small", action="store_true", help="8 images of 1024^2 (a rehearsal, not a measurement)")
    a = ap.parse_args()
    ik = _lib.load()
    assert ik.ik_device_count() > 0, "no HIP device"
    assert ik.ik_init(0) == 0, _lib.last_error()
    geoms = [(8, 1024, 1024, 4), (8, 1024, 1024, 3)] if a.small else [(64, 4096, 4096, 4), (256, 4096, 4096, 3)]
    for n, W, H, C in geoms:
        pitch = (W * C + 255) // 256 * 256  # as ik_image rows
        stride = pitch * H
        src, dst = ctypes.c_void_p(), ctypes.c_void_p()
        assert ik.ik_dev_alloc(n * stride, ctypes.byref(src)) == 0, _lib.last_error()
        assert ik.ik_dev_alloc(n * stride, ctypes.byref(dst)) == 0, _lib.last_error()
        ms = {k: [] for k in KINDS}

        def run(k):
            t0 = time.perf_counter()
            assert ik.ik_orient_batch_device(src, W, H, C, 1, pitch, stride, n, k, dst, pitch, stride, None) == 0
            assert ik.ik_dev_synchronize() == 0
            return (time.perf_counter() - t0) * 1e3

        for k in KINDS:  # warm-up: code objects, first touch of both areas
            run(k)
            run(k)
        for _ in range(a.repeats):
            for k in KINDS:
                ms[k].append(run(k))
        ik.ik_dev_free(src)
        ik.ik_dev_free(dst)
        moved = 2.0 * n * W * H * C  # bytes: one read and one write of the pixels
        copy = statistics.median(ms[1])
        res = {"n": n, "W": W, "H": H, "C": C, "pitch": pitch, "repeats": a.repeats, "bytes_moved": moved, "kinds": {}}
        for k in KINDS:
            med = statistics.median(ms[k])
            res["kinds"]["copy" if k == 1 else str(k)] = {
                "ms_median": round(med, 3), "ms_min": round(min(ms[k]), 3), "ms_max": round(max(ms[k]), 3),
                "TBps": round(moved / (med * 1e-3) / 1e12, 3), "ratio_to_copy": round(med / copy, 3)}
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
