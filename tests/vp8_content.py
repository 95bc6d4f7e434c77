"""Chosen inputs for the exact WebP coder -- TEST INFRASTRUCTURE (plain numpy).

ikutil.synth's patterns S and N never give a flat macroblock, a frame one macroblock wide
or high, a frame that ends on an epoch edge of the coder's schedule, or a frame that a
directional intra-4 mode dominates.  patterns() and GEOMETRIES give those;
tests/test_vp8x_inputs.py proves from libwebp's own bytes that they do, and the GPU and
CPU-model tests (tests/test_gpu_vp8x_content.py, tests/test_vp8_modes.py) code them.
"""
import numpy as np

import ikutil

# the content sizes: 12 and 35 macroblocks, the second ragged on both axes
CONTENT_SIZES = [(64, 48), (100, 70)]
# the content qualities: 98 / 99 is the chroma error-diffusion switch; at 10 and 25 the D/SD
# doubling of PickBestIntra16 decides the file on the flat frames (without it the restated
# coder writes other bytes for flat0, flat255, flatcolour, halves and flat_in_noise there,
# and the same bytes at 1, 50 and 98 ... 100)
CONTENT_QUALITIES = [1, 10, 25, 50, 98, 99, 100]

# (w, h): what the frame pins -- number of epochs and the size of the last one follow from
# epoch_bounds(); test_vp8x_inputs.py asserts them
GEOMETRIES = [
    (16, 64),     # 1 x 4: one MB wide
    (64, 16),     # 4 x 1: one MB high
    (32, 33),     # 2 x 3: ragged bottom row
    (192, 128),   # 12 x 8 = 96 MBs: no refresh
    (1536, 16),   # 96 x 1 = 96 MBs: the same count in one row
    (16, 1552),   # 1 x 97 = 97 MBs: a last epoch of one MB; no left or top-right anywhere
    (3088, 16),   # 193 x 1 = 193 MBs: two epochs
    (1552, 32),   # 97 x 2 = 194 MBs: three epochs, the last with one MB
    (1552, 128),  # 97 x 8 = 776 MBs: the first count with M = 97
]

# the strips and epoch edges among them (everything but the 6-MB and 12 x 8 frames)
STRIPS = [g for g in GEOMETRIES if min(g) == 16 or g[0] == 1552]


def mb_dims(w, h):
    return (w + 15) // 16, (h + 15) // 16


def epoch_bounds(w, h):
    """libwebp refreshes its probabilities before macroblocks M, 2M+1, 3M+2, ... with
    M = max(mb_count / 8, 96) (VP8EncTokenLoop: `if (--cnt < 0)` with cnt reset to M).
    Returns [0, those below mb_count ..., mb_count]."""
    mb_w, mb_h = mb_dims(w, h)
    n = mb_w * mb_h
    m = max(n >> 3, 96)
    return [0] + list(range(m, n, m + 1)) + [n]


def _grey(v):
    return np.stack([v, v, v], -1).astype(np.uint8)


def flat_in_noise(w, h, seed=0, grey=128):
    """Pattern N with every second macroblock (a chessboard of 16x16 cells) one constant
    grey: flat and busy macroblocks neighbour each other in both directions."""
    img = ikutil.synth(w, h, 3, seed=seed, pattern="N")
    yy, xx = np.mgrid[0:h, 0:w]
    img[((xx >> 4) + (yy >> 4)) % 2 == 0] = grey
    return img


def _ramp(w, h, yy, xx):
    return np.stack([xx * 255 // max(w - 1, 1), yy * 255 // max(h - 1, 1), (xx + yy) * 255 // max(w + h - 2, 1)], -1)


def _primaries(w, h, yy, xx):
    six = np.array([[255, 0, 0], [255, 255, 0], [0, 255, 0], [0, 255, 255], [0, 0, 255], [255, 0, 255]], np.uint8)
    return six[((xx // 8) + 2 * (yy // 8)) % 6]


def _halves(w, h, yy, xx):
    img = np.zeros((h, w, 3), np.uint8)
    img[:, w // 2:] = 255  # right half white
    img[h // 2:, :w // 2, 0] = 128  # bottom-left quarter dark red
    return img


_MAKERS = {
    "flat0": lambda w, h, yy, xx: np.zeros((h, w, 3)),
    "flat255": lambda w, h, yy, xx: np.full((h, w, 3), 255),
    "flatcolour": lambda w, h, yy, xx: np.broadcast_to(np.array([90, 140, 200]), (h, w, 3)),
    "vstripes": lambda w, h, yy, xx: _grey(((xx // 3) & 1) * 200 + 20),
    "hstripes": lambda w, h, yy, xx: _grey(((yy // 3) & 1) * 200 + 20),
    "diag45": lambda w, h, yy, xx: _grey((((xx + yy) // 5) & 1) * 180 + 30),
    "diag135": lambda w, h, yy, xx: _grey((((xx - yy) // 5) & 1) * 180 + 30),
    "diag_steep": lambda w, h, yy, xx: _grey((((2 * xx + yy) // 7) & 1) * 180 + 30),
    "diag_shallow": lambda w, h, yy, xx: _grey((((xx - 2 * yy) // 7) & 1) * 180 + 30),
    "ramp": _ramp,
    "checker1": lambda w, h, yy, xx: _grey(((xx + yy) & 1) * 255),
    # beyond the issue's list: black and white macroblocks side by side, the largest luma DC
    # step an 8-bit picture has (the census' largest coded level, 1752, comes from it)
    "checker16": lambda w, h, yy, xx: _grey((((xx >> 4) + (yy >> 4)) & 1) * 255),
    "primaries": _primaries,
    "halves": _halves,
    "flat_in_noise": lambda w, h, yy, xx: flat_in_noise(w, h, seed=w + 9 * h),
}
PATTERN_NAMES = list(_MAKERS)


def pattern(name, w, h):
    """One named RGB8 image of w x h."""
    yy, xx = np.mgrid[0:h, 0:w]
    return np.ascontiguousarray(np.asarray(_MAKERS[name](w, h, yy, xx)).astype(np.uint8))


def patterns(w, h):
    """Every named RGB8 image of w x h (a dict, in PATTERN_NAMES' order)."""
    return {name: pattern(name, w, h) for name in PATTERN_NAMES}


def geometry_image(name, w, h):
    """The geometry tests' contents: S and N from ikutil.synth, or a named pattern."""
    if name in ("S", "N"):
        return ikutil.synth(w, h, 3, seed=w ^ (3 * h), pattern=name)
    return pattern(name, w, h)
