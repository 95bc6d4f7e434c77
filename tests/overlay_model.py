"""The watermark overlay restated in numpy (rules 1-7): all integers, uint64
throughout, so the restatement is exact.  Images are (H, W, C) arrays of uint8 or uint16."""
import numpy as np

CENTER, N, S, E, W, NE, NW, SE, SW = range(9)
GRAVITIES = (CENTER, N, S, E, W, NE, NW, SE, SW)
MAX_OFFSET = 1 << 24


def place(Wb, Hb, wo, ho, gravity, dx=0, dy=0, tile=False):
    """(x, y, w, h, x0, y0): the window in the base (all 0 when empty) and the overlay's origin"""
    sx, sy = Wb - wo, Hb - ho
    x0 = (0 if gravity in (W, NW, SW) else sx if gravity in (E, NE, SE) else sx // 2) + dx  # // floors
    y0 = (0 if gravity in (N, NE, NW) else sy if gravity in (S, SE, SW) else sy // 2) + dy
    if tile:
        x, y, x1, y1 = 0, 0, Wb, Hb
    else:
        x, y, x1, y1 = max(x0, 0), max(y0, 0), min(x0 + wo, Wb), min(y0 + ho, Hb)
    if x1 <= x or y1 <= y:
        return 0, 0, 0, 0, x0, y0
    return x, y, x1 - x, y1 - y, x0, y0


def to_depth(v, src_depth, dst_depth):
    """rule 1: samples (uint64) of src_depth bytes at dst_depth bytes"""
    if src_depth == dst_depth:
        return v
    return v * 257 if dst_depth == 2 else (v + 128) // 257


def overlay_samples(O, C, depth):
    """rules 1 and 2: the overlay as a base of C channels and `depth` bytes sees it:
    f (ho, wo, 1 or 3) and fa (ho, wo), uint64"""
    M = 256 ** depth - 1
    s = to_depth(O.astype(np.uint64), O.dtype.itemsize, depth)
    co = O.shape[2]
    fa = s[..., co - 1] if co in (2, 4) else np.full(O.shape[:2], M, np.uint64)
    if C >= 3:
        f = s[..., :3] if co >= 3 else np.repeat(s[..., :1], 3, axis=2)
    elif co >= 3:
        f = ((2126 * s[..., 0] + 7152 * s[..., 1] + 722 * s[..., 2]) // 10000)[..., None]
    else:
        f = s[..., :1]
    return f, fa


def effective_alpha(fa, opacity, depth):
    """rule 3"""
    M = 256 ** depth - 1
    opM = opacity if depth == 1 else opacity * 257
    return (np.asarray(fa, np.uint64) * np.uint64(opM) + np.uint64(M // 2)) // np.uint64(M)


def blend_opaque(c, f, a, depth):
    """rule 4 on uint64 arrays"""
    M = np.uint64(256 ** depth - 1)
    return (f * a + c * (M - a) + M // np.uint64(2)) // M


def blend_alpha(c, ca, f, a, depth):
    """rule 5 on uint64 arrays: (colour, alpha); c and f (..., k), ca and a (...)"""
    M = np.uint64(256 ** depth - 1)
    t = ca * (M - a)
    D = a * M + t
    out_a = (D + M // np.uint64(2)) // M
    Dz = np.where(D == 0, np.uint64(1), D)[..., None]
    Nn = f * (a * M)[..., None] + c * t[..., None]
    out_c = (Nn + Dz // np.uint64(2)) // Dz
    keep = (D == 0)
    return np.where(keep[..., None], c, out_c), np.where(keep, ca, out_a)


def overlay(B, O, gravity=CENTER, dx=0, dy=0, opacity=255, tile=False):
    """B under O: a new array of B's shape and dtype"""
    Hb, Wb, C = B.shape
    ho, wo = O.shape[:2]
    depth = B.dtype.itemsize
    x, y, w, h, x0, y0 = place(Wb, Hb, wo, ho, gravity, dx, dy, tile)
    out = B.copy()
    if not w:
        return out
    f, fa = overlay_samples(O, C, depth)
    ys = (np.arange(y, y + h) - y0) % ho  # Euclidean: numpy's % takes the divisor's sign
    xs = (np.arange(x, x + w) - x0) % wo
    f, fa = f[ys][:, xs], fa[ys][:, xs]
    a = effective_alpha(fa, opacity, depth)
    win = B[y:y + h, x:x + w].astype(np.uint64)
    if C in (1, 3):
        res = blend_opaque(win, f, a[..., None], depth)
    else:
        oc, oa = blend_alpha(win[..., :C - 1], win[..., C - 1], f, a, depth)
        res = np.concatenate([oc, oa[..., None]], axis=2)
    out[y:y + h, x:x + w] = res.astype(B.dtype)
    return out
