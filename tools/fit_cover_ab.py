#!/usr/bin/env python3
"""A/B for fit=cover against the only way to get those pixels without it: B RGBA
4096x2304 frames, (a) cover -> 512x512 (the window 199..710 of a virtual 910x512,
ik_resize_window_batch_device) and (b) the whole resize to 910x512
(ik_resize_batch_device), Triangle and Lanczos3.  Kernel alone, HIP events on a stream
of our own, the arms alternated inside each repeat; per arm the median and the range of
the repeats, per repeat the ratio (a)/(b).  Also checks that (a) is (b)'s columns.
Prints one JSON line.  argv[1] = B (default 64), argv[2] = repeats (default 12)."""
import ctypes
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "rust-image-transform_amd"))
from imagekit import _lib  # noqa: E402

W, H, C, TW, TH = 4096, 2304, 4, 512, 512
B = int(sys.argv[1]) if len(sys.argv) > 1 else 64
REPS = int(sys.argv[2]) if len(sys.argv) > 2 else 12
lib = _lib.load()
assert lib.ik_init(0) == 0, _lib.last_error()
win = (ctypes.c_uint32 * 6)()
assert lib.ik_fit_target(W, H, TW, TH, 1, win) == 0
iw, ih, x0, y0, nw, nh = win
assert (iw, ih, x0, y0, nw, nh) == (910, 512, 199, 0, 512, 512)
src = torch.randint(0, 256, (B, H, W * C), dtype=torch.uint8, device="cuda")
da = torch.zeros((B, nh, nw * C), dtype=torch.uint8, device="cuda")
db = torch.zeros((B, ih, iw * C), dtype=torch.uint8, device="cuda")
st = torch.cuda.Stream()
torch.cuda.synchronize()


def arm_a(f):
    return lib.ik_resize_window_batch_device(src.data_ptr(), W, H, C, W * C, H * W * C, B, iw, ih, x0, y0, nw, nh, f,
                                             da.data_ptr(), nw * C, nh * nw * C, st.cuda_stream)


def arm_b(f):
    return lib.ik_resize_batch_device(src.data_ptr(), W, H, C, W * C, H * W * C, B, iw, ih, f, db.data_ptr(), iw * C,
                                      ih * iw * C, st.cuda_stream)


def timed(fn, f):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(st)
    assert fn(f) == 0, _lib.last_error()
    e1.record(st)
    e1.synchronize()
    return e0.elapsed_time(e1)


res = {"B": B, "reps": REPS, "window": [iw, ih, x0, y0, nw, nh], "nw_over_iw": round(nw / iw, 4)}
for f, name in ((1, "triangle"), (4, "lanczos3")):
    info = (ctypes.c_int32 * 13)()
    lib.ik_resize_plan_info_window(W, H, C, iw, ih, x0, y0, nw, nh, f, B, info, 13)
    ns_a, fam_a = info[4], info[12]
    lib.ik_resize_plan_info(W, H, C, iw, ih, f, B, info, 13)
    ns_b, fam_b = info[4], info[12]
    for fn in (arm_a, arm_b):     # warm-up: plan upload, code objects
        timed(fn, f)
    a, b = [], []
    for r in range(REPS):
        order = ((arm_a, a), (arm_b, b)) if r % 2 == 0 else ((arm_b, b), (arm_a, a))
        for fn, sink in order:
            sink.append(timed(fn, f))
    ratios = [x / y for x, y in zip(a, b)]
    same = bool(torch.equal(da.view(B, nh, nw, C), db.view(B, ih, iw, C)[:, y0:y0 + nh, x0:x0 + nw]))
    res[name] = {"family": [fam_a, fam_b], "strips": [ns_a, ns_b], "strips_ratio": round(ns_a / ns_b, 4),
                 "cover_ms": [round(float(np.median(a)), 4), round(min(a), 4), round(max(a), 4)],
                 "exact910_ms": [round(float(np.median(b)), 4), round(min(b), 4), round(max(b), 4)],
                 "ratio": [round(float(np.median(ratios)), 4), round(min(ratios), 4), round(max(ratios), 4)],
                 "cover_equals_crop": same}
print(json.dumps(res))
