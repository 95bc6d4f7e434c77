"""Time the PNG upload's gather + CRC pass (k_png_gather, k_png_crc_check) with nothing
else on the device: the bench's batch (64 requests over 4 distinct 4096^2 RGBA PNG files,
each request its own device allocation) submitted one batch at a time, so no other
batch's kernels run beside it.  The time is the library's own pair of HIP events round
the pass (ik_png_last_timing[14]: the plan tables' copy, k_png_gather, k_png_crc_check),
the rate is over 2 x the PNG bytes (read + written).  Usage:
python tools/png_gather_timing.py [--n 64] [--iters 12] [--host]"""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "rust-image-transform_amd"), os.path.join(ROOT, "tests")]
import ikutil  # noqa: E402

ikutil.use_pillow_codecs()
import bench  # noqa: E402
from imagekit import DeviceBytes, PinnedBytes, _lib, transform_batch_submit, transform_batch_submit_device  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=64)
ap.add_argument("--iters", type=int, default=12)
ap.add_argument("--size", type=int, default=4096)
ap.add_argument("--host", action="store_true", help="inputs in page-locked host memory (the upload-area path)")
args = ap.parse_args()
lib = _lib.load()
assert lib.ik_init(0) == 0, _lib.last_error()
frames = [ikutil.synth(args.size, args.size, 4, seed=sd, pattern="S") for sd in bench.shard_seeds(0, 4)]
pngs = bench.make_pngs(frames)
n = args.n
nbytes = sum(len(pngs[i % 4]) for i in range(n))
reqs = [(PinnedBytes if args.host else DeviceBytes)(pngs[i % 4]) for i in range(n)]
submit = transform_batch_submit if args.host else transform_batch_submit_device
ms = []
for it in range(args.iters + 2):
    out = submit(reqs, [(512, 512)] * n, [1] * n, [80] * n, filter=ikutil.TRIANGLE, threads=16).wait()
    assert all(o for o in out)
    t = (ctypes.c_double * 17)()
    lib.ik_png_last_timing(t, 17)
    ms.append(t[14])
ms = ms[2:]  # (two warm-up batches: allocation, first launches)
med = statistics.median(ms)
print(json.dumps({"inputs": "host" if args.host else "device", "requests": n, "png_bytes": nbytes,
                  "gather_crc_ms": [round(x, 3) for x in ms], "median_ms": round(med, 3), "min_ms": round(min(ms), 3),
                  "GBps_over_2x_png_bytes": round(2 * nbytes / med / 1e6, 1)}))
