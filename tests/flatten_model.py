"""The background flatten restated in numpy (u64), for the tests: the project's own
definition.  With M the sample maximum, c a sample, a its pixel's alpha
and b the background channel (b8 * 257 at 16 bits),

    out = (c * a + b * (M - a) + M // 2) // M

and the channel rule: Rgba -> Rgb; LumaA -> Luma for a gray colour, Rgb (luma replicated)
for any other; Luma and Rgb as they are."""
import numpy as np

EDGE16 = (0, 1, 127, 128, 254, 255, 256, 257, 32767, 32768, 65279, 65534, 65535)


def blend(c, a, b, M):
    c, a, b = (np.asarray(v, dtype=np.uint64) for v in (c, a, b))
    M = np.uint64(M)
    return (c * a + b * (M - a) + M // np.uint64(2)) // M


def background_channels(rgb: int, depth: int):
    """(R, G, B) of 0xRRGGBB at the image's depth (bytes per sample)."""
    b8 = ((rgb >> 16) & 255, (rgb >> 8) & 255, rgb & 255)
    return b8 if depth == 1 else tuple(v * 257 for v in b8)


def out_channels(c: int, rgb: int) -> int:
    if c == 4:
        return 3
    if c == 2:
        r, g, b = background_channels(rgb, 1)
        return 1 if r == g == b else 3
    return c


def flatten(img: np.ndarray, rgb: int, oc: int = None) -> np.ndarray:
    """img (H, W, C) uint8 or uint16 onto 0xRRGGBB: (H, W, out_channels) of the same dtype.
    oc forces the output channels of a LumaA image (3 is allowed with a gray colour)."""
    assert img.ndim == 3 and img.dtype in (np.uint8, np.uint16)
    C = img.shape[2]
    if C not in (2, 4):
        return img.copy()
    depth = img.dtype.itemsize
    M = 255 if depth == 1 else 65535
    bg = background_channels(rgb, depth)
    oc = oc or out_channels(C, rgb)
    a = img[..., C - 1]
    out = np.empty(img.shape[:2] + (oc,), img.dtype)
    for k in range(oc):
        out[..., k] = blend(img[..., k if C == 4 else 0], a, bg[k], M)
    return out
