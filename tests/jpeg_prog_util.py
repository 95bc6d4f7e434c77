"""Progressive JPEG files without restart markers, for tests/test_jpeg_prog_model.py
(CPU) and tests/test_gpu_jpeg_prog_free.py (GPU).

Pillow's progressive=True writes libjpeg's default script: DC first and DC
refinement, AC first scans whose end-of-block runs span many blocks, and AC
refinement scans.  tests/jpeg_writer.py writes the samplings Pillow lacks (4:4:0,
4:1:1, 2x2/2x1/1x1), by spectral selection and with DC successive approximation,
without AC refinement and with no run longer than a block."""
import functools
import io

import numpy as np
from PIL import Image

import ikutil
import jpeg_writer as jw


def pillow(px, mode="RGB", **kw):
    b = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(px), mode).save(b, format="JPEG", progressive=True, **kw)
    return b.getvalue()


@functools.lru_cache(maxsize=None)
def noise_444():
    return pillow(ikutil.synth(203, 141, 3, seed=11, pattern="N"), quality=95, subsampling=0)


@functools.lru_cache(maxsize=None)
def s_420():
    return pillow(ikutil.synth(640, 480, 3, seed=12, pattern="S"), quality=90, subsampling=2)


@functools.lru_cache(maxsize=None)
def s_422():
    return pillow(ikutil.synth(333, 211, 3, seed=13, pattern="S"), quality=75, subsampling=1)


@functools.lru_cache(maxsize=None)
def noise_420_big():
    return pillow(ikutil.synth(1024, 768, 3, seed=14, pattern="N"), quality=85, subsampling=2)


@functools.lru_cache(maxsize=None)
def gray():
    return pillow(ikutil.synth(257, 131, 3, seed=15, pattern="N")[..., 1], "L", quality=88)


@functools.lru_cache(maxsize=None)
def flat_gray():
    """A flat image: every AC-first scan is a handful of end-of-block runs, each
    covering up to 32,767 blocks."""
    return pillow(np.full((512, 512), 120, np.uint8), "L", quality=90)


@functools.lru_cache(maxsize=None)
def flat_gray_noise_rows():
    """The flat image under 64 rows of noise: long end-of-block runs in a file of
    more than 4 KiB (the flat one alone codes to 1.5 KiB)."""
    px = np.full((512, 512), 120, np.uint8)
    px[:64] = ikutil.synth(512, 64, 3, seed=19, pattern="N")[..., 1]
    return pillow(px, "L", quality=90)


@functools.lru_cache(maxsize=None)
def optimised_420():
    return pillow(ikutil.synth(321, 243, 3, seed=16, pattern="N"), quality=90, subsampling=2, optimize=True)


@functools.lru_cache(maxsize=None)
def tiny():
    """Below the 4 KiB the GPU entropy decoders start at."""
    return pillow(ikutil.synth(17, 9, 3, seed=17, pattern="S"), quality=85)


@functools.lru_cache(maxsize=None)
def with_restart_rows():
    return pillow(ikutil.synth(320, 240, 3, seed=18, pattern="N"), quality=85, restart_marker_rows=1)


WRITER_SAMPLINGS = {"440": jw.S440, "411": jw.S411, "221": jw.S221}
WRITER_SCRIPTS = {"spectral": jw.script_spectral, "dc_approx": jw.script_dc_approx}


@functools.lru_cache(maxsize=None)
def writer(sampling: str, script: str, wh=jw.BIG, pattern="N") -> jw.JpegFile:
    """jpeg_writer's progressive scripts without a restart interval."""
    planes = jw.ycbcr(ikutil.synth(wh[0], wh[1], 3, seed=len(sampling + script) + wh[0], pattern=pattern))
    kw = dict(huff="optimal", tables=(0, 1, 2)) if script == "dc_approx" else {}
    return jw.encode(planes, WRITER_SAMPLINGS[sampling], sof=jw.SOF2, scans=WRITER_SCRIPTS[script](), **kw)


@functools.lru_cache(maxsize=None)
def overlapping_first_scans() -> jw.JpegFile:
    """A file no encoder writes: the luma band 1..5 is coded by two Ah = 0 scans.  A
    decoder that applies scans in file order lets the later one win."""
    S = jw.Scan
    script = (S((0, 1, 2), 0, 0), S((0,), 1, 63), S((1,), 1, 63), S((2,), 1, 63), S((0,), 1, 5))
    return jw.encode(jw.ycbcr(ikutil.synth(jw.BIG[0], jw.BIG[1], 3, seed=21, pattern="N")), jw.S440, sof=jw.SOF2,
                     scans=script)


def scan_spans(data: bytes):
    """(start, end) of each scan's entropy-coded bytes in a restart-free file."""
    out, p = [], 2
    while p + 4 <= len(data):
        assert data[p] == 0xFF
        m = data[p + 1]
        if m == 0xD9:
            break
        ln = data[p + 2] << 8 | data[p + 3]
        p += 2 + ln
        if m == 0xDA:
            q = p
            while not (data[q] == 0xFF and data[q + 1] not in (0x00, 0xFF)):
                q += 1
            out.append((p, q))
            p = q
    return out
