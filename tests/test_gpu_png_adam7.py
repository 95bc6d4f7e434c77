"""GPU: Adam7-interlaced PNG streams decode on the GPU path (inflate, the pass images
resolved and unfiltered side by side, k_png_adam7 into the image's rows, png's EXPAND),
not on the host decoder.  Every stream is written by png_adam7_util (IHDR byte 12 is
asserted to be 1: Pillow's writer ignores interlace=1), and the expected pixels are
the source array, Pillow's (libpng's) decode of the same bytes and this library's host
decoder on the same bytes (ik_set_png_gpu_min above the file's size).  Every GPU
decode asserts with ik_png_counters that the GPU count rose and the host count did not."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import ikutil
import png_adam7_util as A7
from imagekit import (DeviceBytes, ImageFormat, TransformError, decode_image, decode_image_batch, transform_batch,
                      transform_batch_submit_device)

pytestmark = pytest.mark.gpu

GEOMETRY = [(1, 1), (2, 2), (3, 3), (4, 4), (5, 1), (1, 5), (5, 5), (8, 8), (9, 9), (7, 5), (33, 17), (129, 33),
            (67, 131)]
HOST_ONLY = 1 << 40


@pytest.fixture
def gpu_png(ik):
    assert ik.ik_set_png_gpu_min(0) == 0  # every PNG through the GPU path
    yield ik
    ik.ik_set_png_gpu_min(256 << 10)


def counters(ik):
    c = (ctypes.c_ulonglong * 2)()
    assert ik.ik_png_counters(c) == 0
    return c[0], c[1]


def samples(w, h, ctype, depth, seed=0):
    r = ikutil.splitmix64(0xADA70000 + seed, w * h * A7.SPP[ctype]).reshape(h, w, A7.SPP[ctype])
    return (r & np.uint64((1 << depth) - 1)).astype(np.uint16)


def palette(depth):
    n = 1 << depth
    return (ikutil.splitmix64(0x9A1, n * 3) & np.uint64(255)).astype(np.uint8).reshape(n, 3)


def on_host(ik, png):
    """The host decoder's answer for the same bytes."""
    ik.ik_set_png_gpu_min(HOST_ONLY)
    try:
        g0, h0 = counters(ik)
        d, _ = decode_image(png)
        assert counters(ik) == (g0, h0 + 1)
        return d.to_array()
    finally:
        ik.ik_set_png_gpu_min(0)


def on_gpu(ik, png):
    g0, h0 = counters(ik)
    d, fmt = decode_image(png)
    g1, h1 = counters(ik)
    assert (g1 - g0, h1 - h0) == (1, 0), "the interlaced stream must decode on the GPU path"
    assert fmt is None
    return d.to_array()


def check(ik, s, ctype, depth, **kw):
    png = A7.make_png(s, ctype, depth, **kw)
    want = A7.expanded(s, ctype, depth, kw.get("plte"), kw.get("trns"))
    got = on_gpu(ik, png)
    assert got.dtype == want.dtype and got.shape == want.shape
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(got, on_host(ik, png))
    pil = A7.pillow_pixels(png)
    if pil is not None:  # Pillow keeps no tRNS key alpha and reduces 16-bit colour to the high bytes
        w2 = want[..., : pil.shape[-1]]
        np.testing.assert_array_equal(pil, w2 >> 8 if (w2.dtype != pil.dtype and pil.dtype == np.uint8) else w2)


@pytest.mark.parametrize("wh", GEOMETRY, ids=lambda g: f"{g[0]}x{g[1]}")
@pytest.mark.parametrize("ctype,depth", [(6, 8), (2, 8), (0, 1)], ids=["rgba8", "rgb8", "gray1"])
def test_geometry(gpu_png, ctype, depth, wh):
    check(gpu_png, samples(wh[0], wh[1], ctype, depth, seed=wh[0] * 131 + wh[1]), ctype, depth)


def _trns_for(ctype, depth, s):
    if ctype == 3:
        return bytes((ikutil.splitmix64(0x7A5, max(1, (1 << depth) - 1)) & np.uint64(255)).astype(np.uint8))
    key = [int(v) for v in s[3, 5]]
    return b"".join(int(v).to_bytes(2, "big") for v in key)


COLOUR = ([(c, 8, False) for c in (0, 4, 2, 6)] + [(c, 16, False) for c in (0, 4, 2, 6)] +
          [(0, d, t) for d in (1, 2, 4) for t in (False, True)] +
          [(3, d, t) for d in (1, 2, 4, 8) for t in (False, True)] + [(2, 8, True), (2, 16, True)])


@pytest.mark.parametrize("wh", [(33, 17), (129, 33)], ids=lambda g: f"{g[0]}x{g[1]}")
@pytest.mark.parametrize("ctype,depth,trns", COLOUR, ids=lambda v: str(int(v)))
def test_colour_types(gpu_png, ctype, depth, trns, wh):
    s = samples(wh[0], wh[1], ctype, depth, seed=ctype * 16 + depth)
    kw = {}
    if ctype == 3:
        kw["plte"] = palette(depth)
    if trns:
        kw["trns"] = _trns_for(ctype, depth, s)
        if ctype != 3:
            s[9, :] = s[3, 5]  # a row of the transparent colour
    check(gpu_png, s, ctype, depth, **kw)


def _restarted(first):
    """The y % 5 cycle, shifted so that the first row of every pass takes `first`."""
    return lambda q, y: (y + first) % 5


FILTERS = [0, 1, 2, 3, 4, _restarted(2), _restarted(3), _restarted(4)]


@pytest.mark.parametrize("filt", FILTERS, ids=["none", "sub", "up", "avg", "paeth", "first-up", "first-avg", "first-paeth"])
@pytest.mark.parametrize("ctype,depth", [(6, 8), (2, 8), (0, 4)], ids=["rgba8", "rgb8", "gray4"])
def test_filters(gpu_png, ctype, depth, filt):
    """Up / Average / Paeth on a pass's first row: wrong if it reads the previous pass's last row."""
    check(gpu_png, samples(33, 17, ctype, depth, seed=77), ctype, depth, filt=filt)


@pytest.fixture(scope="module")
def big():
    """512 x 384 noise, RGBA8 and RGB8: IDATs many times the 16 KiB search chunk, so
    several decoder lanes and window markers, and passes that begin and end inside lanes."""
    out = {}
    for c, ctype in ((4, 6), (3, 2)):
        src = ikutil.synth(512, 384, c, seed=5 + c, pattern="N", alpha="random")
        for idat in (None, 8192):
            png = A7.make_png(src, ctype, 8, level=6, idat=idat)
            assert len(A7.idat_bytes(png)) > 8 * 16384
            out[c, idat] = (src, png)
    return out


@pytest.mark.parametrize("idat", [None, 8192], ids=["one-idat", "8k-idats"])
@pytest.mark.parametrize("c", [4, 3], ids=["rgba8", "rgb8"])
def test_lanes_and_windows(gpu_png, big, c, idat):
    src, png = big[c, idat]
    got = on_gpu(gpu_png, png)
    np.testing.assert_array_equal(got, src)
    np.testing.assert_array_equal(got, on_host(gpu_png, png))
    np.testing.assert_array_equal(A7.pillow_pixels(png), src)


_LANE_CHILD = r"""
import ctypes, sys
import numpy as np
sys.path[:0] = [%(pkg)r, %(tests)r]
import ikutil, png_adam7_util as A7
from imagekit import _lib, decode_image
lib = _lib.load()
assert lib.ik_init(0) == 0
assert lib.ik_set_png_gpu_min(0) == 0
src = ikutil.synth(512, 384, 4, seed=9, pattern="N", alpha="random")
png = A7.make_png(src, 6, 8)
assert len(A7.idat_bytes(png)) > 8 * 16384
c0 = (ctypes.c_ulonglong * 2)(); lib.ik_png_counters(c0)
d, _ = decode_image(png)
c1 = (ctypes.c_ulonglong * 2)(); lib.ik_png_counters(c1)
assert (c1[0] - c0[0], c1[1] - c0[1]) == (1, 0), (list(c0), list(c1))
assert np.array_equal(d.to_array(), src)
print("lane-ok")
"""


def test_lane_decoder_in_a_child_process(ik):
    """IK_PNG_DECODE=lane (the one-thread-per-lane decoder shares resolve): read once per
    process, so a fresh child."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = _LANE_CHILD % {"pkg": os.path.join(root, "rust-image-transform_amd"), "tests": os.path.join(root, "tests")}
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, IK_PNG_DECODE="lane"), capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0 and "lane-ok" in r.stdout, r.stdout + r.stderr


def test_batch_of_twelve(gpu_png):
    """Interlaced and plain streams of every bytes-per-pixel class in one batch: each
    image equals its single decode; twelve on the GPU, none on the host."""
    spec = [(6, 8, 1, (129, 33)), (6, 8, 0, (67, 131)), (2, 8, 1, (67, 131)), (2, 8, 0, (33, 17)),
            (0, 8, 1, (129, 33)), (4, 8, 1, (33, 17)), (4, 8, 0, (40, 30)), (2, 16, 1, (33, 17)),
            (6, 16, 1, (67, 131)), (6, 16, 0, (9, 9)), (0, 1, 1, (129, 33)), (4, 16, 1, (5, 5))]
    assert {max(1, A7.SPP[c] * d // 8) for c, d, _, _ in spec} == {1, 2, 3, 4, 6, 8}
    pngs = [A7.make_png(samples(w, h, c, d, seed=i), c, d, interlace=il) for i, (c, d, il, (w, h)) in enumerate(spec)]
    single = [on_gpu(gpu_png, p) if p[28] == 1 else decode_image(p)[0].to_array() for p in pngs]
    g0, h0 = counters(gpu_png)
    got = decode_image_batch(pngs)
    g1, h1 = counters(gpu_png)
    assert (g1 - g0, h1 - h0) == (12, 0)
    for i, (c, d, _il, (w, h)) in enumerate(spec):
        np.testing.assert_array_equal(got[i][0].to_array(), single[i])
        np.testing.assert_array_equal(single[i], A7.expanded(samples(w, h, c, d, seed=i), c, d))


def test_device_inputs(gpu_png):
    """Interlaced files already in device memory take the same path, with no copy back."""
    rgb = ikutil.synth(640, 480, 3, seed=21, pattern="S")
    idx = samples(640, 480, 3, 8, seed=22)
    pal = palette(8)
    datas = [A7.make_png(rgb, 2, 8), A7.make_png(idx, 3, 8, plte=pal, trns=_trns_for(3, 8, idx))]
    n = len(datas)
    want = transform_batch(datas, [(320, None)] * n, [ImageFormat.webp] * n, [80] * n)
    dev = [DeviceBytes(d) for d in datas]
    g0, h0 = counters(gpu_png)
    got = transform_batch_submit_device(dev, [(320, None)] * n, [ImageFormat.webp] * n, [80] * n).wait()
    g1, h1 = counters(gpu_png)
    assert (g1 - g0, h1 - h0) == (n, 0)
    assert got == want


def _bad_filter(rows, s_shape, bits):
    geo = A7.passes(s_shape[1], s_shape[0], bits)[0]
    first = sum(g[5] for g in geo[:2])  # the first row of pass 3
    rows = list(rows)
    rows[first] = bytes([7]) + rows[first][1:]
    return rows


ERRORS = {
    "filter-7-in-pass-3": dict(raw_edit=lambda rows: _bad_filter(rows, (17, 33), 32)),
    "one-row-short": dict(raw_edit=lambda rows: rows[:-1]),
    "interlace-2": dict(interlace=2),
}


@pytest.mark.parametrize("name", list(ERRORS))
def test_errors_are_the_host_decoders(gpu_png, name):
    png = A7.make_png(samples(33, 17, 6, 8, seed=3), 6, 8, **ERRORS[name])
    gpu_png.ik_set_png_gpu_min(HOST_ONLY)
    try:
        with pytest.raises(TransformError) as host:
            decode_image(png)
    finally:
        gpu_png.ik_set_png_gpu_min(0)
    with pytest.raises(TransformError) as gpu:
        decode_image(png)
    assert str(gpu.value) == str(host.value) and str(host.value)
