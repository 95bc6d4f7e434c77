"""Dev tool: progressive JPEG files without restart markers through decode_image and
decode_image_batch, with the switch at host (every scan on the host entropy decoder:
the behaviour without the switch, the baseline) against gpu (ik_set_jpeg_prog_free: the
Ah = 0 scans through the self-synchronising launches, k_jprog_dc_refine,
k_jprog_ac_chain).

  python tools/jpeg_prog_bench.py [--shapes 2000x2000x64,4096x4096x1,1024x768x256]
                                  [--rounds 3] [--runs 3] [--out FILE.jsonl]

A shape is WxHxN: N Pillow progressive q85 4:2:0 files (two distinct ones, tiled) in one
decode_image_batch call, or, N = 1, one decode_image call.  Per shape: wall ms and process
CPU ms per call for both arms, alternated round by round so that their spread is seen on
the same machine in the same session, and from ik_jpeg_prog_free_ms of the last gpu-arm
call the device ms (HIP events) of the self-synchronising launches, the DC refinement
launches and the AC refinement chains."""
import argparse
import ctypes
import io
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "rust-image-transform_amd"), os.path.join(ROOT, "tests")]
import ikutil  # noqa: E402

DISTINCT = 2  # distinct files per shape, tiled over the batch
HOST, GPU = 0, 1


def files(w, h):
    from PIL import Image
    out = []
    for k in range(DISTINCT):
        b = io.BytesIO()
        Image.fromarray(ikutil.synth(w, h, 3, seed=3000 + k, pattern="S")).save(b, format="JPEG", quality=85,
                                                                                subsampling=2, progressive=True)
        out.append(b.getvalue())
    return out


def timed(fn, runs):
    wall, cpu = [], []
    for _ in range(runs):
        c0, t0 = time.process_time(), time.perf_counter()
        fn()
        t1, c1 = time.perf_counter(), time.process_time()
        wall.append((t1 - t0) * 1e3)
        cpu.append((c1 - c0) * 1e3)
    return statistics.median(wall), statistics.median(cpu)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="2000x2000x64,4096x4096x1,1024x768x256")
    ap.add_argument("--rounds", type=int, default=3, help="host / gpu alternations per shape")
    ap.add_argument("--runs", type=int, default=3, help="timed calls per arm and round (their median)")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    from imagekit import _lib, decode_image, decode_image_batch
    lib = _lib.load()
    assert lib.ik_init(0) == 0, _lib.last_error()
    for shape in a.shapes.split(","):
        w, h, n = (int(v) for v in shape.split("x"))
        fs = files(w, h)
        batch = [fs[i % DISTINCT] for i in range(n)]

        def call():
            out = decode_image(batch[0]) if n == 1 else decode_image_batch(batch)
            del out

        def counts():
            c = (ctypes.c_ulonglong * 2)()
            lib.ik_jpeg_counters(c)
            return c[0], c[1]

        rec = dict(shape=shape, file_kb=round(len(fs[0]) / 1024, 1))
        try:
            for where in (HOST, GPU):  # warm both arms: code objects, pools, pinned areas
                assert lib.ik_set_jpeg_prog_free(where) == 0
                c0 = counts()
                call()
                c1 = counts()
                rec["gpu_counted" if where == GPU else "host_counted"] = [c1[0] - c0[0], c1[1] - c0[1]]
            res = {HOST: [], GPU: []}
            for _ in range(a.rounds):
                for where in (HOST, GPU):
                    assert lib.ik_set_jpeg_prog_free(where) == 0
                    res[where].append(timed(call, a.runs))
            for where, tag in ((HOST, "host"), (GPU, "gpu")):
                ws = [v[0] for v in res[where]]
                rec[f"{tag}_wall_ms"] = round(statistics.median(ws), 3)
                rec[f"{tag}_wall_ms_rounds"] = [round(v, 3) for v in ws]
                rec[f"{tag}_cpu_ms"] = round(statistics.median(v[1] for v in res[where]), 3)
            t = (ctypes.c_double * 3)()
            lib.ik_jpeg_prog_free_ms(t)  # of the last gpu-arm call
            rec["phase_a_ms"], rec["dc_refine_ms"], rec["ac_chain_ms"] = (round(v, 3) for v in t)
        finally:
            lib.ik_set_jpeg_prog_free(-1)
        print(json.dumps(rec), flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
