"""Windowed resampling (fit=cover / fit=exact) for the tests: the windowed twins of
resize_model.ResizeModel over lib/libik_resizemodel.so, the reference of a fit target
(the oracle's resize_dimensions plus image 0.25.8's resize_to_fill crop rule, written
out here), the oracle's pixels of a window, and the geometry matrix the CPU model walk
and the GPU parity test share.  TEST INFRASTRUCTURE ONLY."""
from __future__ import annotations

import ctypes
from types import SimpleNamespace

import numpy as np

from resize_model import (_PLAN, _STATS, _TABLES, FUSED, NAIVE, PERIODIC, ResizeModel)  # noqa: F401

CONTAIN, COVER, EXACT = 0, 1, 2               # ik_fit
NEAREST, TRIANGLE, CATMULLROM, GAUSSIAN, LANCZOS3 = range(5)
U32 = 0xFFFFFFFF


class WindowModel(ResizeModel):
    """plan / tables / run of a window win = (iw, ih, x0, y0, nw, nh)."""

    def __init__(self):
        super().__init__()
        L, i = self.lib, ctypes.c_int
        L.ikm_resize_plan_window.argtypes = [i] * 11 + [ctypes.POINTER(ctypes.c_int32), i]
        L.ikm_resize_table_window.restype = ctypes.c_longlong
        L.ikm_resize_table_window.argtypes = [i] * 12 + [ctypes.c_void_p, ctypes.c_longlong]
        L.ikm_resize_run_window.argtypes = [ctypes.c_void_p, ctypes.c_longlong, ctypes.c_longlong] + [i] * 12 + [
            ctypes.c_void_p, ctypes.c_longlong, ctypes.c_longlong, i, i, ctypes.POINTER(ctypes.c_longlong)]

    def plan_window(self, W, H, C, win, f, n=1):
        out = (ctypes.c_int32 * len(_PLAN))()
        assert self.lib.ikm_resize_plan_window(W, H, C, *win, int(f), n, out, len(_PLAN)) == len(_PLAN)
        p = SimpleNamespace(**dict(zip(_PLAN, out)))
        p.geom = (W, H, C) + tuple(win) + (int(f), n)
        p.family = NAIVE if not p.slots else PERIODIC if p.per_A else FUSED
        return p

    def raw_tables_window(self, W, H, C, win, f, n=1):
        """The fourteen tables as flat arrays, in ikm_resize_table's order."""
        out = []
        for k, (name, dt) in enumerate(_TABLES):
            size = self.lib.ikm_resize_table_window(W, H, C, *win, int(f), n, k, None, 0)
            assert size >= 0
            a = np.zeros(size // np.dtype(dt).itemsize, dt)
            if size:
                assert self.lib.ikm_resize_table_window(W, H, C, *win, int(f), n, k, a.ctypes.data, size) == size
            out.append(a)
        return out

    def raw_tables(self, W, H, C, nw, nh, f, n=1):
        out = []
        for k, (name, dt) in enumerate(_TABLES):
            size = self.lib.ikm_resize_table(W, H, C, nw, nh, int(f), n, k, None, 0)
            a = np.zeros(size // np.dtype(dt).itemsize, dt)
            if size:
                assert self.lib.ikm_resize_table(W, H, C, nw, nh, int(f), n, k, a.ctypes.data, size) == size
            out.append(a)
        return out

    def tables_window(self, W, H, C, win, f, n=1):
        t = self.plan_window(W, H, C, win, f, n)
        for (name, _), a in zip(_TABLES, self.raw_tables_window(W, H, C, win, f, n)):
            setattr(t, name, a)
        nw, nh = win[4], win[5]
        t.wx = t.wx.reshape(nw, t.Tx)
        t.wy = t.wy.reshape(nh, t.Ty)
        t.strips = t.strips.reshape(-1, 3)
        t.bands = t.bands.reshape(-1, 2)
        t.per_bands = t.per_bands.reshape(-1, 2)
        t.hdr = t.hdr.reshape(-1, 4)
        return t

    def run_window(self, src, win, f, n=1, fma=False, family=-1):
        """src (H, W, C) -> the window's (nh, nw, C) pixels and the run's statistics.  The
        destination is prefilled with a sentinel per byte position, so an unwritten byte
        shows (`unwritten_out`)."""
        src = np.ascontiguousarray(src)
        H, W, C = src.shape
        nw, nh = win[4], win[5]
        a = np.full((nh, nw, C), 0x5A, np.uint8)
        b = np.full((nh, nw, C), 0xA5, np.uint8)
        st = (ctypes.c_longlong * len(_STATS))()
        for out in (a, b):
            rc = self.lib.ikm_resize_run_window(src.ctypes.data, W * C, H * W * C, W, H, C, *win, int(f), n, 1,
                                                out.ctypes.data, nw * C, nh * nw * C, int(bool(fma)), family, st)
            assert rc == 0, "ikm_resize_run_window refused the arguments"
        s = SimpleNamespace(**dict(zip(_STATS, st)))
        s.unwritten_out = int((a != b).sum())   # a byte nobody wrote keeps its two different sentinels
        return a, s


def fit_reference(orc, W, H, w, h, fit):
    """(iw, ih, x0, y0, nw, nh) as the issue restates image 0.25.8, from the oracle's
    iko_resize_image_dims / iko_resize_dimensions and the crop rule; None where the
    library must report an overflow (a virtual side above u32)."""
    if fit == CONTAIN or (fit == COVER and (w is None or h is None)):
        nw, nh = orc.resize_image_dims(W, H, w, h)
        return (nw, nh, 0, 0, nw, nh)
    f32 = np.float32
    tw = w if w is not None else int(min(max(np.round(f32(W) * (f32(h) / f32(H))), 0), U32))
    th = h if h is not None else int(min(max(np.round(f32(H) * (f32(w) / f32(W))), 0), U32))
    tw, th = max(tw, 1), max(th, 1)
    if fit == EXACT:
        return (tw, th, 0, 0, tw, th)
    ratio = max(tw / W, th / H)                 # f64, as resize_dimensions
    if max(np.round(W * ratio), np.round(H * ratio)) > U32:
        return None
    iw, ih = ctypes.c_uint32(), ctypes.c_uint32()
    orc.lib.iko_resize_dimensions(ctypes.c_uint32(W), ctypes.c_uint32(H), ctypes.c_uint32(tw), ctypes.c_uint32(th), 1,
                                  ctypes.byref(iw), ctypes.byref(ih))
    iw, ih = iw.value, ih.value
    if tw * ih > iw * th:                       # Python integers: no overflow (u64 in the crate)
        x0, y0 = 0, (ih - th) // 2
    else:
        x0, y0 = (iw - tw) // 2, 0
    return (iw, ih, x0, y0, min(tw, iw - x0), min(th, ih - y0))


def oracle_window(orc, src, win, f):
    """The oracle's resize to iw x ih, cropped: what a window must equal."""
    iw, ih, x0, y0, nw, nh = win
    return orc.resize(src, iw, ih, int(f))[y0:y0 + nh, x0:x0 + nw]


def case(name, W, H, C, tw, th, f, family, n=1):
    return SimpleNamespace(name=name, W=W, H=H, C=C, tw=tw, th=th, f=f, family=family, n=n)


def _matrix():
    out = []
    for f in range(5):
        for C in (1, 2, 3, 4):
            # 200 x 60 -> 50 x 40: virtual 133 x 40, columns 41..90; 64 x 200 -> 40 x 50: virtual
            # 40 x 125, rows 37..86.  (Rows of W * C bytes are multiples of 8 in every case, so
            # a device source can be allocated with nothing after its last row.)
            out.append(case(f"col-f{f}-c{C}", 200, 60, C, 50, 40, f, FUSED))
            out.append(case(f"row-f{f}-c{C}", 64, 200, C, 40, 50, f, FUSED))
    return out


# every filter x channel count, a column crop and a row crop each
MATRIX = _matrix()
# the named cases of the issue.  family: what ik_resize_plan_info_window must report.
NAMED = [
    # RGBA 1400 x 50 -> 300 x 24: virtual 672 x 24, columns 186..485; the window's first
    # source byte (382 * 4) is no multiple of 128 and its 2.5 KB of source columns cross
    # a strip.  1400 x 48: the same on the periodic kernel (virtual 700 x 24, R = 2)
    case("rgba-mid-strip", 1400, 50, 4, 300, 24, LANCZOS3, FUSED),
    case("rgba-mid-strip-periodic", 1400, 48, 4, 300, 24, LANCZOS3, PERIODIC),
    # RGB: the strip's first pixel sits 43 / 39 / 39 pixels into the strip's LDS row (no
    # multiple of 8), with the strip's first byte 2 / 1 / 0 bytes into a pixel
    case("rgb-odd-origin-phi2", 1104, 41, 3, 200, 20, LANCZOS3, FUSED),
    case("rgb-odd-origin-phi1", 1304, 41, 3, 260, 20, LANCZOS3, FUSED),
    case("rgb-odd-origin-periodic", 1000, 48, 3, 200, 24, LANCZOS3, PERIODIC),
    # 96 x 256 -> 48 x 64: virtual 48 x 128, R = 2, rows 32..95
    case("periodic-row", 96, 256, 4, 48, 64, TRIANGLE, PERIODIC),
    # 96 x 256 -> 48 x 62: rows 33..94
    case("periodic-row-odd-y0", 96, 256, 3, 48, 62, TRIANGLE, PERIODIC),
    # 2 x 400 -> 100 x 100: virtual 100 x 20000, rows 9950..10049
    case("naive-upscale", 2, 400, 4, 100, 100, LANCZOS3, NAIVE),
    # 8 x 1600 -> 100 x 100: virtual 100 x 20000 again, RGB
    case("naive-upscale-c3", 8, 1600, 3, 100, 100, TRIANGLE, NAIVE),
    # 400 x 2 -> 100 x 100: virtual 20000 x 100, columns 9950..10049 read three source pixels:
    # the two-pass kernels' column range
    case("naive-col-crop", 400, 2, 4, 100, 100, LANCZOS3, NAIVE),
]
CASES = MATRIX + NAMED
