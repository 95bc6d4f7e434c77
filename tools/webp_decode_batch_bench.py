"""Dev tool: time decode_image_batch over batches of lossy q80 WebP files (the batch path
of the GPU WebP decoder, decode_webp_batch) -- wall ms per batch (median of the timed
runs after the warm-ups), ik_webp_last_timing of the last run, process CPU seconds per
batch (every thread: the worker pool's parse + token decode or libwebp).

  python tools/webp_decode_batch_bench.py --mode gpu [--grids 256,512,1024,occ]
                                          [--workloads 512,768,1080,4096,mix] [--cache DIR] [--out FILE]

--mode sets IK_WEBP_DECODE (auto / gpu / host); --grids repeats every workload per
IK_VP8D_GRID value; --cache keeps the encoded files between runs (encoding the 4096^2
frames takes seconds).  Works against a library without ik_webp_last_timing too (an
older build to compare with): those fields are then left out."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "rust-image-transform_amd"), os.path.join(ROOT, "tests")]
import ikutil  # noqa: E402
import webp_tool as wt  # noqa: E402

GEOMETRY = {"512": (512, 512, 64), "768": (1024, 768, 64), "1080": (1920, 1080, 64), "4096": (4096, 4096, 16)}
DISTINCT = 4  # distinct frames per geometry, tiled over the batch


def frames(key, cache):
    w, h, _ = GEOMETRY[key]
    out = []
    for k in range(DISTINCT):
        path = os.path.join(cache, f"q80_{w}x{h}_{k}.webp") if cache else None
        if path and os.path.exists(path):
            out.append(open(path, "rb").read())
            continue
        data = wt.encode(ikutil.synth(w, h, 3, seed=1000 + k, pattern="S"), 80)
        if path:
            os.makedirs(cache, exist_ok=True)
            with open(path, "wb") as f:
                f.write(data)
        out.append(data)
    return out


def workload(key, cache):
    if key == "mix":  # a quarter of each batch
        reqs = []
        for g in GEOMETRY:
            fr = frames(g, cache)
            reqs += [fr[i % DISTINCT] for i in range(GEOMETRY[g][2] // 4)]
        return "mix (16 x 512^2, 16 x 1024x768, 16 x 1920x1080, 4 x 4096^2)", reqs
    w, h, n = GEOMETRY[key]
    fr = frames(key, cache)
    return f"{n} x {w}x{h}", [fr[i % DISTINCT] for i in range(n)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", default="gpu", choices=["auto", "gpu", "host"])
    ap.add_argument("--grids", default="", help="comma-separated IK_VP8D_GRID values (default: the library's grid)")
    ap.add_argument("--workloads", default="512,768,1080,4096,mix")
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--cache", default="")
    ap.add_argument("--encode-only", action="store_true", help="fill --cache and exit (no GPU needed)")
    ap.add_argument("--out", default="", help="append one JSON line per measurement")
    a = ap.parse_args()
    keys = [k for k in a.workloads.split(",") if k]
    if a.encode_only:
        for k in keys:
            workload(k, a.cache)
        return
    from imagekit import _lib, decode_image_batch
    try:
        lib = _lib.load()
    except AttributeError:  # an older library: bind what it has
        _lib.SIGNATURES = [s for s in _lib.SIGNATURES if not s[0].startswith("ik_webp_")
                           or s[0] in ("ik_webp_yuv420_device", "ik_webp_encode_exact_device")]
        lib = _lib.load()
    assert lib.ik_init(0) == 0, _lib.last_error()
    has_timing = hasattr(lib, "ik_webp_last_timing")
    os.environ["IK_WEBP_DECODE"] = a.mode
    for grid in (a.grids.split(",") if a.grids else [""]):
        if grid:
            os.environ["IK_VP8D_GRID"] = grid
        for key in keys:
            name, reqs = workload(key, a.cache)
            wall, cpu = [], []
            for r in range(a.warmup + a.runs):
                c0, t0 = time.process_time(), time.perf_counter()
                out = decode_image_batch(reqs)
                t1, c1 = time.perf_counter(), time.process_time()
                del out
                if r >= a.warmup:
                    wall.append((t1 - t0) * 1e3)
                    cpu.append(c1 - c0)
            rec = dict(workload=name, mode=a.mode, grid=grid or "default", runs=a.runs,
                       wall_ms_median=round(statistics.median(wall), 3), wall_ms_min=round(min(wall), 3),
                       wall_ms_max=round(max(wall), 3), cpu_s_per_batch=round(statistics.median(cpu), 4))
            line = (f"{name:58s} {a.mode:4s} grid {rec['grid']:>7s}: wall {rec['wall_ms_median']:8.2f} ms "
                    f"({rec['wall_ms_min']:.2f} .. {rec['wall_ms_max']:.2f}), cpu {rec['cpu_s_per_batch'] * 1e3:8.1f} ms")
            if has_timing:
                t = (ctypes.c_double * 10)()
                lib.ik_webp_last_timing(t, 10)
                rec["last_timing"] = [round(v, 3) for v in t]
                line += (f" | host half {t[0]:.2f} ms ({t[1]:.1f} core-ms) stage+h2d {t[2]:.2f} recon {t[3]:.2f} "
                         f"rgb {t[4]:.2f} ms, gpu {int(t[5])} host {int(t[6])}, rows {int(t[7])} grid {int(t[8])} "
                         f"launches {int(t[9])}")
            print(line, flush=True)
            if a.out:
                with open(a.out, "a") as f:
                    f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
