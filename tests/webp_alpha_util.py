"""Lossy WebP files with an alpha plane, and libwebp's answer for them -- TEST
INFRASTRUCTURE ONLY (shared by tests/test_webp_alpha_host.py and
tests/test_gpu_webp_alpha.py; the checker of the GPU path's alpha half, never the product).

decode_rgba(): WebPDecodeRGBA of the system libwebp, the pixels the GPU path must equal.
pillow_files(): files of Pillow's encoder that between them carry a raw and a lossless
plane, pre-processing 0 and 1 and the filters libwebp's encoder picks.
hand_built(): a VP8X container put together here -- the "VP8 " chunk of webp_tool.encode
and a raw ALPH chunk whose plane is forward-filtered here with a chosen filter, so all
four filters occur at every size whatever an encoder would choose.
broken_files(): the files the GPU path must leave to libwebp."""
from __future__ import annotations

import ctypes
import io

import numpy as np
from PIL import Image

import ikutil
import webp_tool as wt

SIZES = [(1, 1), (1, 9), (9, 1), (65, 64), (64, 65), (130, 67)]


def decode_rgba(data: bytes) -> np.ndarray:
    L = wt.lib()
    L.WebPDecodeRGBA.restype = ctypes.c_void_p
    L.WebPDecodeRGBA.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_int),
                                 ctypes.POINTER(ctypes.c_int)]
    w, h = ctypes.c_int(), ctypes.c_int()
    p = L.WebPDecodeRGBA(data, len(data), ctypes.byref(w), ctypes.byref(h))
    if not p:
        raise ValueError("WebPDecodeRGBA failed")
    a = np.frombuffer(ctypes.string_at(p, w.value * h.value * 4), np.uint8).reshape(h.value, w.value, 4).copy()
    L.WebPFree(p)
    return a


# ---- the RIFF container ----
def chunks(data: bytes) -> list[tuple[bytes, bytes]]:
    assert data[:4] == b"RIFF" and data[8:12] == b"WEBP"
    out, p = [], 12
    while p + 8 <= len(data):
        n = int.from_bytes(data[p + 4:p + 8], "little")
        out.append((data[p:p + 4], data[p + 8:p + 8 + n]))
        p += 8 + n + (n & 1)
    return out


def riff(parts: list[tuple[bytes, bytes]]) -> bytes:
    body = b"WEBP"
    for cc, payload in parts:
        body += cc + len(payload).to_bytes(4, "little") + payload + (b"\x00" if len(payload) & 1 else b"")
    return b"RIFF" + len(body).to_bytes(4, "little") + body


def vp8x(w: int, h: int, flags: int) -> tuple[bytes, bytes]:
    return b"VP8X", bytes([flags, 0, 0, 0]) + (w - 1).to_bytes(3, "little") + (h - 1).to_bytes(3, "little")


# ---- libwebp's alpha filters (dsp/filters.c) ----
def predict(plane: np.ndarray, filt: int) -> np.ndarray:
    """The prediction of every pixel from the un-filtered plane."""
    a = plane.astype(np.int32)
    h, w = a.shape
    left = np.zeros_like(a)
    left[:, 1:] = a[:, :-1]
    above = np.zeros_like(a)
    above[1:] = a[:-1]
    corner = np.zeros_like(a)
    corner[1:, 1:] = a[:-1, :-1]
    pred = {0: np.zeros_like(a), 1: left, 2: above, 3: np.clip(left + above - corner, 0, 255)}[filt].copy()
    if filt:
        pred[0, :] = left[0, :]    # row 0 from the left ((0, 0) from 0)
        pred[1:, 0] = above[1:, 0]  # column 0 from above
    return pred


def forward_filter(plane: np.ndarray, filt: int) -> np.ndarray:
    return ((plane.astype(np.int32) - predict(plane, filt)) & 255).astype(np.uint8)


def unfilter(filtered: np.ndarray, filt: int) -> np.ndarray:
    """The decoder's side, pixel by pixel in raster order (the gradient's clip is serial)."""
    h, w = filtered.shape
    if filt == 0:
        return filtered.copy()
    f = filtered.astype(np.int32).tolist()
    out = [[0] * w for _ in range(h)]
    for y in range(h):
        row, up = out[y], out[y - 1] if y else None
        for x in range(w):
            if y == 0:
                p = row[x - 1] if x else 0
            elif x == 0:
                p = up[0]
            elif filt == 1:
                p = row[x - 1]
            elif filt == 2:
                p = up[x]
            else:
                p = min(255, max(0, row[x - 1] + up[x] - up[x - 1]))
            row[x] = (f[y][x] + p) & 255
    return np.array(out, dtype=np.uint8).reshape(h, w)


# ---- the files ----
def alpha_of(kind: str, w: int, h: int, seed: int) -> np.ndarray:
    yy, xx = np.mgrid[0:h, 0:w]
    if kind == "noise":
        return ikutil.synth(w, h, 4, seed=seed, alpha="random")[..., 3].copy()
    if kind == "smooth":
        return ((xx * 3 + yy * 2 + seed) % 256).astype(np.uint8)
    if kind == "levels":
        return (((xx // 7 + yy // 5) % 4) * 85).astype(np.uint8)
    raise ValueError(kind)


def _pillow(rgba: np.ndarray, **kw) -> bytes:
    b = io.BytesIO()
    Image.fromarray(rgba, "RGBA").save(b, format="WEBP", **kw)
    return b.getvalue()


PILLOW_KINDS = [("noise", dict(quality=80)), ("smooth", dict(quality=80)), ("levels", dict(quality=75)),
                ("smooth", dict(quality=80, alpha_quality=50)), ("smooth", dict(quality=60, method=6))]


def pillow_files(sizes=((130, 67), (64, 65))) -> list[tuple[str, bytes]]:
    out = []
    for w, h in sizes:
        for k, (kind, kw) in enumerate(PILLOW_KINDS):
            px = ikutil.synth(w, h, 4, seed=3 + k, pattern="S")
            px[..., 3] = alpha_of(kind, w, h, seed=5 + k)
            out.append((f"{kind} {w}x{h} {kw}", _pillow(px, **kw)))
    return out


def alph_header(data: bytes) -> dict:
    """What a file's ALPH header byte says."""
    (payload,) = [p for cc, p in chunks(data) if cc == b"ALPH"]
    b = payload[0]
    return dict(compression=b & 3, filter=(b >> 2) & 3, pre=(b >> 4) & 3, reserved=b >> 6)


def hand_built(w: int, h: int, filt: int, kind: str = "noise", seed: int = 0, header_extra: int = 0,
               drop_bytes: int = 0) -> bytes:
    """VP8X + a raw ALPH chunk (filter filt; header_extra ors into the header byte;
    drop_bytes cuts the plane short) + the "VP8 " chunk of webp_tool.encode."""
    rgb = ikutil.synth(w, h, 3, seed=seed + 11 * w + h, pattern="S")
    (vp8,) = [c for c in chunks(wt.encode(rgb, 75)) if c[0] == b"VP8 "]
    plane = forward_filter(alpha_of(kind, w, h, seed + w + 3 * h + filt), filt).tobytes()
    if drop_bytes:
        plane = plane[:-drop_bytes]
    return riff([vp8x(w, h, 0x10), (b"ALPH", bytes([filt << 2 | header_extra]) + plane), vp8])


def broken_files() -> list[tuple[str, bytes]]:
    """Files the GPU path leaves to libwebp (ik_webp_alpha_plane: IK_ERR_UNSUPPORTED)."""
    w, h = 40, 30
    rgb = ikutil.synth(w, h, 3, seed=2, pattern="S")
    rgba = ikutil.synth(w, h, 4, seed=2, pattern="S")
    rgba[..., 3] = alpha_of("smooth", w, h, 1)
    opaque = wt.encode(rgb, 80)
    lossy_alpha = _pillow(rgba, quality=80)
    assert alph_header(lossy_alpha)["compression"] == 1
    parts = chunks(lossy_alpha)
    cut = [(cc, p[:max(2, len(p) // 2)] if cc == b"ALPH" else p) for cc, p in parts]
    return [
        ("opaque", opaque),
        ("lossless", _pillow(rgba, lossless=True, exact=True)),
        ("flag without chunk", riff([vp8x(w, h, 0x10)] + [c for c in chunks(opaque) if c[0] == b"VP8 "])),
        ("short raw plane", hand_built(w, h, 1, drop_bytes=5)),
        ("reserved bits 2", hand_built(w, h, 1, header_extra=2 << 6)),
        ("truncated lossless payload", riff(cut)),
    ]
