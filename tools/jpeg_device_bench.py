"""Dev tool: JPEG request bodies that already lie in device memory, decoded where they
lie (IK_JPEG_DEVICE=inplace: k_jpeg_walk brings back the skeletons, the decoder reads
the scans from the caller's memory) against copied back to the host at submit
(IK_JPEG_DEVICE=copy: the behaviour before in-place decoding), and the same batches
taken from page-locked host memory as the reference point.

  python tools/jpeg_device_bench.py [--shapes configs2,loadtest] [--batch N] [--rounds 3]
                                    [--runs 3] [--distinct 4] [--out FILE.jsonl]

Shapes:
  configs2  256 x 4096^2 q90 4:2:0, half with a restart marker per MCU row and half
            restart-free -> 512^2 Lanczos3 -> JPEG q85
  loadtest  64 x 2000^2 q90 4:2:0 -> w, h drawn from [200, 800) -> JPEG / WebP q80

Each batch is submitted and waited for on its own (nothing else in flight).  Per arm:
ms per batch (submit to the end of wait), the ms submit takes to return, and the
process's CPU ms per batch -- the median of --runs batches, per round; the arms
alternate round by round so their spread is seen on one machine in one session.  The
walk kernel's own device time (HIP events, ik_jpeg_device_walk_ms) is read after an
in-place batch."""
import argparse
import io
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "rust-image-transform_amd"), os.path.join(ROOT, "tests")]
import ikutil  # noqa: E402

ikutil.use_pillow_codecs()


def sources(size, distinct, rst_half):
    from PIL import Image
    out = []
    for k in range(distinct):
        px = ikutil.synth(size, size, 3, seed=3000 + k, pattern="S")
        b = io.BytesIO()
        kw = {"restart_marker_rows": 1} if rst_half and k % 2 == 0 else {}
        Image.fromarray(px, "RGB").save(b, format="JPEG", quality=90, subsampling=2, **kw)
        out.append(b.getvalue())
    return out


def shape(name, batch, distinct):
    from imagekit import ImageFormat
    if name == "configs2":
        n = batch or 256
        src = sources(4096, distinct, True)
        return src, [k % distinct for k in range(n)], [(512, 512)] * n, [ImageFormat.jpeg] * n, [85] * n
    n = batch or 64
    src = sources(2000, distinct, False)
    rng = np.random.default_rng(7)
    sizes = [(int(rng.integers(200, 800)), int(rng.integers(200, 800))) for _ in range(n)]
    fmts = [(ImageFormat.jpeg, ImageFormat.webp)[int(rng.integers(0, 2))] for _ in range(n)]
    return src, [int(rng.integers(0, distinct)) for _ in range(n)], sizes, fmts, [80] * n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="configs2,loadtest")
    ap.add_argument("--batch", type=int, default=0, help="requests per batch (0: the shape's own)")
    ap.add_argument("--distinct", type=int, default=4, help="distinct source files, tiled over the batch")
    ap.add_argument("--rounds", type=int, default=3, help="alternations of the arms")
    ap.add_argument("--runs", type=int, default=3, help="timed batches per arm and round (their median)")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    from imagekit import DeviceBytes, PinnedBytes, _lib, transform_batch_submit, transform_batch_submit_device
    lib = _lib.load()
    assert lib.ik_init(0) == 0, _lib.last_error()
    for name in a.shapes.split(","):
        src, pick, sizes, fmts, qs = shape(name, a.batch, a.distinct)
        # every request its own copy of its file, as request bodies arrive
        dev = [DeviceBytes(src[k]) for k in pick]
        pin = [PinnedBytes(src[k]) for k in pick]
        scan_mb = sum(len(src[k]) for k in pick) / 1e6

        def run(arm):
            c0, t0 = time.process_time(), time.perf_counter()
            if arm == "pinned":
                p = transform_batch_submit(pin, sizes, fmts, qs)
            else:
                p = transform_batch_submit_device(dev, sizes, fmts, qs)
            t1 = time.perf_counter()
            out = p.wait()
            t2, c1 = time.perf_counter(), time.process_time()
            return (t2 - t0) * 1e3, (t1 - t0) * 1e3, (c1 - c0) * 1e3, out

        def set_arm(arm):
            os.environ["IK_JPEG_DEVICE"] = "copy" if arm == "copy" else "inplace"

        arms = ("inplace", "copy", "pinned")
        ref = None
        for arm in arms:  # warm every arm (code objects, pools, pinned areas); the bytes must agree
            set_arm(arm)
            out = run(arm)[3]
            ref = ref or out
            assert out == ref, f"{arm}: outputs differ"
        res = {arm: [] for arm in arms}
        for _ in range(a.rounds):
            for arm in arms:
                set_arm(arm)
                t = [run(arm)[:3] for _ in range(a.runs)]
                res[arm].append(tuple(statistics.median(v[k] for v in t) for k in range(3)))
        set_arm("inplace")
        c = (lib.ik_jpeg_device_counters.argtypes[0]._type_ * 3)()
        lib.ik_jpeg_device_counters(c)
        before = list(c)
        run("inplace")
        lib.ik_jpeg_device_counters(c)
        rec = dict(shape=name, batch=len(pick), distinct=len(src), file_mb=round(scan_mb, 1), rounds=a.rounds,
                   runs=a.runs, walk_kernel_ms=round(lib.ik_jpeg_device_walk_ms(), 4),
                   device_counters_delta=[int(x - y) for x, y in zip(c, before)])
        for arm in arms:
            for k, what in enumerate(("batch_ms", "submit_ms", "cpu_ms")):
                vals = [v[k] for v in res[arm]]
                rec[f"{arm}_{what}"] = round(statistics.median(vals), 2)
                rec[f"{arm}_{what}_rounds"] = [round(v, 2) for v in vals]
        print(json.dumps(rec), flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(json.dumps(rec) + "\n")
        del dev, pin


if __name__ == "__main__":
    main()
