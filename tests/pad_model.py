"""The pad of DESIGN section 4 restated in numpy, for the tests: the place rule, the frame
pixel of colour mode, and the four modes as np.pad's `constant`, `edge`, `symmetric` and
`wrap` -- numpy's own code, so an oracle that shares nothing with the library.  index_map is
the definition's index formula written out, which tests/test_pad_model.py holds np.pad to."""
import numpy as np

NONE, COLOR, EDGE, MIRROR, WRAP = 0, 1, 2, 3, 4
NP_MODE = {COLOR: "constant", EDGE: "edge", MIRROR: "symmetric", WRAP: "wrap"}
# ik_gravity
CENTER, N, S, E, W, NE, NW, SE, SW = range(9)
LEFT, RIGHT, TOP, BOTTOM = (W, NW, SW), (E, NE, SE), (N, NE, NW), (S, SE, SW)


def place(w, h, width, height, gravity):
    """(cw, ch, x0, y0): the canvas of a w x h image and where the image lies in it"""
    cw, ch = max(w, width), max(h, height)
    x0 = 0 if gravity in LEFT else cw - w if gravity in RIGHT else (cw - w) // 2
    y0 = 0 if gravity in TOP else ch - h if gravity in BOTTOM else (ch - h) // 2
    return cw, ch, x0, y0


def frame_pixel(C, depth, color, alpha):
    """the C samples of the frame pixel of colour mode"""
    s = 1 if depth == 1 else 257
    r, g, b = ((color >> 16) & 255) * s, ((color >> 8) & 255) * s, (color & 255) * s
    px = [r, g, b] if C >= 3 else [(2126 * r + 7152 * g + 722 * b) // 10000]
    if C in (2, 4):
        px.append(alpha * s)
    return px


def pad(img, mode, gravity=CENTER, width=0, height=0, color=0, alpha=0):
    """img (H, W, C), uint8 or uint16, on its canvas"""
    h, w, C = img.shape
    cw, ch, x0, y0 = place(w, h, width, height, gravity)
    widths = ((y0, ch - h - y0), (x0, cw - w - x0))
    if mode != COLOR:
        return np.pad(img, widths + ((0, 0),), mode=NP_MODE[mode])
    px = frame_pixel(C, img.dtype.itemsize, color, alpha)
    return np.stack([np.pad(img[..., c], widths, mode="constant", constant_values=px[c]) for c in range(C)], axis=-1)


def index_map(mode, i, n):
    """the source index of signed index i on an axis of n samples (edge, wrap, mirror)"""
    if mode == EDGE:
        return min(max(i, 0), n - 1)
    if mode == WRAP:
        return i % n
    j = i % (2 * n)
    return j if j < n else 2 * n - 1 - j
