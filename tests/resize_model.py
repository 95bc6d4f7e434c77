"""ctypes view of lib/libik_resizemodel.so (csrc/ik_resize_model.cpp): the resampler's
host plan as numpy tables, and its CPU walk of them.  TEST INFRASTRUCTURE ONLY."""
from __future__ import annotations

import ctypes
import os
from types import SimpleNamespace

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODEL_SO = os.path.join(ROOT, "rust-image-transform_amd", "lib", "libik_resizemodel.so")

NAIVE, FUSED, PERIODIC = 0, 1, 2          # kernel family, as ik_resize_plan_info's last value
FAMILY_NAMES = ["k_vert_naive", "k_resize_fused", "k_resize_periodic"]
STRIP_BYTES, ROW_WORDS, MAX_STRIP_COLS, MAX_STRIP_WEIGHTS = 2048, 2304, 512, 4096
INFO = ["slots", "rows", "flush", "wl", "NS", "NB", "per_A", "per_R", "NBp", "Tx", "Ty", "max_strip_cols"]
_PLAN = INFO + ["per_base", "band_h", "max_strip_weights", "lds_words", "nsteps", "per_steps", "lds_pad"]
_TABLES = [("lx", np.int32), ("cx", np.int32), ("wx", np.float32), ("ly", np.int32), ("cy", np.int32),
           ("wy", np.float32), ("strips", np.int32), ("bands", np.int32), ("hdr", np.int32), ("smask", np.uint64),
           ("sw", np.float32), ("band_step", np.int32), ("per_w", np.float32), ("per_bands", np.int32)]
_STATS = ["family", "max_word", "lds_words", "unwritten", "outside", "table_oob", "max_put_word"]


def lds_idx(i):
    return i + ((i >> 5) << 2)


class ResizeModel:
    def __init__(self):
        if not os.path.exists(MODEL_SO):
            raise RuntimeError(f"{MODEL_SO} not found: build it with `make -C rust-image-transform_amd`")
        L = self.lib = ctypes.CDLL(MODEL_SO)
        i = ctypes.c_int
        L.ikm_resize_plan.argtypes = [i] * 7 + [ctypes.POINTER(ctypes.c_int32), i]
        L.ikm_resize_table.restype = ctypes.c_longlong
        L.ikm_resize_table.argtypes = [i] * 8 + [ctypes.c_void_p, ctypes.c_longlong]
        L.ikm_resize_run.argtypes = [ctypes.c_void_p, ctypes.c_longlong, ctypes.c_longlong] + [i] * 8 + [
            ctypes.c_void_p, ctypes.c_longlong, ctypes.c_longlong, i, i, ctypes.POINTER(ctypes.c_longlong)]

    def plan(self, W, H, C, nw, nh, f, n=1):
        """The plan's summary: INFO (ik_resize_plan_info's first twelve values) and more."""
        out = (ctypes.c_int32 * len(_PLAN))()
        assert self.lib.ikm_resize_plan(W, H, C, nw, nh, int(f), n, out, len(_PLAN)) == len(_PLAN)
        p = SimpleNamespace(**dict(zip(_PLAN, out)))
        p.geom = (W, H, C, nw, nh, int(f), n)
        p.family = NAIVE if not p.slots else PERIODIC if p.per_A else FUSED  # exact mode, rows that fit 2^31
        return p

    def tables(self, W, H, C, nw, nh, f, n=1):
        t = self.plan(W, H, C, nw, nh, f, n)
        for k, (name, dt) in enumerate(_TABLES):
            size = self.lib.ikm_resize_table(W, H, C, nw, nh, int(f), n, k, None, 0)
            assert size >= 0
            a = np.zeros(size // np.dtype(dt).itemsize, dt)
            if size:
                assert self.lib.ikm_resize_table(W, H, C, nw, nh, int(f), n, k, a.ctypes.data, size) == size
            setattr(t, name, a)
        t.wx = t.wx.reshape(nw, t.Tx)
        t.wy = t.wy.reshape(nh, t.Ty)
        t.strips = t.strips.reshape(-1, 3)
        t.bands = t.bands.reshape(-1, 2)
        t.per_bands = t.per_bands.reshape(-1, 2)
        t.hdr = t.hdr.reshape(-1, 4)
        if t.slots:
            t.sw = t.sw.reshape(-1, t.rows, t.slots)
        if t.per_A:
            t.per_w = t.per_w.reshape(-1, t.per_A, t.per_R)
        return t

    def run(self, src, nw, nh, f, n=1, fma=False, family=-1, pitch=None, fill=0):
        """src: (H, W, C) or (nimg, H, W, C) -> same leading shape of (nh, nw, C), and the
        run's statistics.  n: the launch size the plan is made for.  pitch: source row
        pitch (rows padded with `fill`)."""
        src = np.ascontiguousarray(src)
        single = src.ndim == 3
        if single:
            src = src[None]
        nimg, H, W, C = src.shape
        pitch = pitch or W * C
        buf = np.full((nimg, H, pitch), fill, np.uint8)
        buf[:, :, :W * C] = src.reshape(nimg, H, W * C)
        out = np.zeros((nimg, nh, nw, C), np.uint8)
        st = (ctypes.c_longlong * len(_STATS))()
        rc = self.lib.ikm_resize_run(buf.ctypes.data, pitch, H * pitch, W, H, C, nw, nh, int(f), n, nimg,
                                     out.ctypes.data, nw * C, nh * nw * C, int(bool(fma)), family, st)
        assert rc == 0, "ikm_resize_run refused the arguments"
        return (out[0] if single else out), SimpleNamespace(**dict(zip(_STATS, st)))
