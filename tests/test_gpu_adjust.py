"""GPU: the colour adjustment.  Everything is compared with zero tolerance: k_adjust against
tests/adjust_model.py for every format and every (matrix, table) variant at the sizes where
its edge handling changes; every 8-bit triple; every 16-bit sample; the raw call on a caller's
area on the wide and the byte paths with poison around every row; the defaults; and
transform() against the by-hand chain."""
import ctypes
import io

import numpy as np
import pytest
from PIL import Image

import adjust_model as am
import ikutil
from imagekit import (Adjust, DynamicImage, ImageFormat, Overlay, _lib, decode_image, encode_image, resize_image)
from imagekit.transform import transform

pytestmark = pytest.mark.gpu
POISON = 0xA5
IK_ERR_INVALID = 2
J, WP = ImageFormat.jpeg, ImageFormat.webp
FORMATS = [(C, d) for d in (1, 2) for C in (1, 2, 3, 4)]
# the four (MATRIX, TABLE) variants; on a gray base the matrix is not applied
VARIANTS = {
    "none": dict(),
    "matrix": dict(saturation=60, hue=75),
    "table": dict(brightness=10, contrast=20, gamma=2.2),
    "both": dict(saturation=-40, hue=-120, brightness=-15, contrast=35, gamma=0.45, invert=1),
}
# the most rows of workgroups in a launch (kAdjustRowCap) times the most rows one takes at once
ROWS_BEFORE_STRIDE = 256 * 4


def counters(ik):
    c = (ctypes.c_ulonglong * 2)()
    assert ik.ik_adjust_counters(c) == 0
    return np.array([c[0], c[1]], dtype=np.int64)


def noise(H, W, C, depth, seed):
    """random samples plus the corners 0 and M"""
    M = 256 ** depth - 1
    r = np.random.default_rng(seed).integers(0, M + 1, (H, W, C))
    flat = r.reshape(-1)
    flat[::7] = 0
    flat[3::11] = M
    return r.astype(np.uint8 if depth == 1 else np.uint16)


def adjust_of(kw):
    """the model's keyword arguments as an Adjust (invert is a bool there)"""
    return Adjust(**dict(kw, invert=bool(kw.get("invert", 0))))


def want_of(img, kw):
    q, t, flags = am.cached_plan(img.dtype.itemsize, **kw)
    return am.apply_plan(img, q, t, flags)


def launches(C, kw):
    """the launches one adjusted image costs: none where the plan leaves these channels alone"""
    tone = any(kw.get(k) for k in ("brightness", "contrast", "gamma", "invert"))
    colour = any(kw.get(k) for k in ("saturation", "hue"))
    return 1 if tone or (colour and C >= 3) else 0


@pytest.mark.parametrize("C,depth", FORMATS, ids=lambda v: str(v))
def test_kernel_equals_model(ik, C, depth):
    S = ik.ik_adjust_span()
    shapes = [(H, W) for W in (1, 2, 3, 5, S - 1, S, S + 1) for H in (1, 3)] + [(ROWS_BEFORE_STRIDE + 5, 5)]
    for name, kw in VARIANTS.items():
        a = adjust_of(kw)
        for H, W in shapes:
            img = noise(H, W, C, depth, seed=H * 31 + W + C * 7 + depth)
            d = DynamicImage.from_array(img[..., 0] if C == 1 else img)
            c0 = counters(ik)
            got = d.adjust(a)
            n = launches(C, kw)
            assert np.array_equal(counters(ik) - c0, (n, n)), (name, H, W)
            assert got.dimensions() == (W, H) and got.depth == depth and got.channels == C
            want = want_of(img, kw)
            g = got.to_array().reshape(img.shape)
            assert np.array_equal(g, want), (name, H, W, np.argwhere(g != want)[:4].tolist())
            if C in (2, 4):
                assert np.array_equal(g[..., -1], img[..., -1])               # alpha as the input's
            assert np.array_equal(d.to_array().reshape(img.shape), img)       # the source is not changed


@pytest.fixture(scope="module")
def all_triples():
    """a 4096 x 4096 RGB8 image that holds each of the 2^24 colours once"""
    v = np.arange(1 << 24, dtype=np.uint32).reshape(4096, 4096)
    return np.stack([v & 255, (v >> 8) & 255, v >> 16], axis=2).astype(np.uint8)


@pytest.mark.parametrize("kw", [dict(grayscale=True), dict(saturation=60, hue=75, brightness=10, contrast=20, gamma=2.2)],
                         ids=["grayscale", "all"])
def test_every_8bit_triple(ik, all_triples, kw):
    a = Adjust(**kw)
    d = DynamicImage.from_array(all_triples)
    c0 = counters(ik)
    got = d.adjust(a).to_array()
    assert np.array_equal(counters(ik) - c0, (1, 1))
    mk = dict(brightness=a.brightness, contrast=a.contrast, saturation=a.saturation, hue=a.hue, gamma=a.gamma)
    q, t, flags = am.plan(1, **mk)
    for k in range(0, 4096, 512):  # the model strip by strip
        want = am.apply_plan(all_triples[k:k + 512], q, t, flags)
        assert np.array_equal(got[k:k + 512], want), k


def test_every_16bit_sample(ik):
    ramp = np.arange(65536, dtype=np.uint16).reshape(256, 256)
    kw = dict(brightness=-7, contrast=30, gamma=2.2)
    c0 = counters(ik)
    got = DynamicImage.from_array(ramp).adjust(**kw).to_array().reshape(256, 256)
    assert np.array_equal(counters(ik) - c0, (1, 1))
    t = am.cached_plan(2, **kw)[1]
    assert np.array_equal(got, t[ramp])
    assert not np.array_equal(got, ramp)


def run_raw(ik, imgs, kw, pitch, gap, off, expect=0):
    """imgs (n, H, W, C) through ik_adjust_batch_device on a torch buffer, in place.  Returns the
    n images after checking that no byte outside the W * C * depth bytes of each row changed
    (pitch padding, before, after and between the images)."""
    import torch
    n, H, W, C = imgs.shape
    depth = imgs.dtype.itemsize
    row = W * C * depth
    stride = pitch * H + gap
    buf = np.full(off + n * stride + 64, POISON, np.uint8)
    for i in range(n):
        buf[off + i * stride:off + i * stride + pitch * H].reshape(H, pitch)[:, :row] = \
            np.ascontiguousarray(imgs[i]).view(np.uint8).reshape(H, row)
    dev = torch.from_numpy(buf).cuda()
    torch.cuda.synchronize()
    assert dev.data_ptr() % 4 == 0
    a = adjust_of(kw)._struct()
    rc = ik.ik_adjust_batch_device(dev.data_ptr() + off, W, H, C, depth, pitch, stride, n, ctypes.byref(a), None)
    assert rc == expect, _lib.last_error()
    assert ik.ik_dev_synchronize() == 0
    got = dev.cpu().numpy()
    if expect:
        assert np.array_equal(got, buf), "a refused call wrote"
        return None
    out = np.zeros((n, H, row), np.uint8)
    keep = np.ones(got.size, bool)
    for i in range(n):
        lo = off + i * stride
        out[i] = got[lo:lo + pitch * H].reshape(H, pitch)[:, :row]
        keep[lo:lo + pitch * H].reshape(H, pitch)[:, :row] = False
    assert (got[keep] == POISON).all(), "a store outside the W * C * depth bytes of a row"
    return out.view(imgs.dtype).reshape(n, H, W, C)


@pytest.mark.parametrize("C,depth", FORMATS, ids=lambda v: str(v))
def test_raw_call_on_a_callers_area(ik, C, depth):
    S = ik.ik_adjust_span()
    W, H = S + 7, 5
    imgs = np.stack([noise(H, W, C, depth, seed=50 + i) for i in range(3)])
    row = W * C * depth
    al = (row + 3) // 4 * 4
    kw = VARIANTS["both"]
    want = np.stack([want_of(im, kw) for im in imgs])
    c0 = counters(ik)
    layouts = [dict(pitch=al + 12, gap=100, off=0), dict(pitch=al + 8, gap=40, off=4)]      # the wide path
    layouts += [dict(pitch=al + 8, gap=40, off=o) for o in (1, 2, 3)]                      # bytes: the base
    layouts += [dict(pitch=al + 5, gap=0, off=0), dict(pitch=al + 4, gap=33, off=0)]       # bytes: pitch, stride
    for lay in layouts:
        got = run_raw(ik, imgs, kw, **lay)
        assert np.array_equal(got, want), (lay, np.argwhere(got != want)[:4].tolist())
    assert np.array_equal(counters(ik) - c0, (len(layouts), 3 * len(layouts)))
    # one image on the byte path with the table alone, and the matrix alone where there is colour
    for name in ("table", "matrix"):
        got = run_raw(ik, imgs[:1], VARIANTS[name], pitch=row + 1, gap=0, off=1)
        assert np.array_equal(got[0], want_of(imgs[0], VARIANTS[name])), name


def test_raw_call_refusals(ik):
    imgs = noise(4, 6, 3, 1, seed=1)[None]
    c0 = counters(ik)
    import torch
    dev = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    ok = Adjust(invert=True)._struct()
    names = ["dev", "W", "H", "C", "depth", "pitch", "stride", "n", "adj", "stream"]
    good = [dev.data_ptr(), 6, 4, 3, 1, 20, 80, 2, ctypes.byref(ok), None]
    for k, v in (("dev", None), ("adj", None), ("W", 0), ("H", 0), ("n", 0), ("C", 0), ("C", 5), ("depth", 3),
                 ("pitch", 17), ("stride", 79), ("n", 65536), ("W", (1 << 24) + 1)):
        a = list(good)
        a[names.index(k)] = v
        assert ik.ik_adjust_batch_device(*a) == IK_ERR_INVALID, (k, v)
        assert _lib.last_error()
    bad = _lib.Adjust(0, 0, 0, 0, 11.0, 0)
    a = list(good)
    a[8] = ctypes.byref(bad)
    assert ik.ik_adjust_batch_device(*a) == IK_ERR_INVALID and "gamma" in _lib.last_error()
    none = _lib.Adjust()
    a[8] = ctypes.byref(none)
    assert ik.ik_adjust_batch_device(*a) == 0  # no adjustment: nothing launched
    assert ik.ik_dev_synchronize() == 0
    assert np.array_equal(counters(ik), c0), "a refused or empty call counted a launch"
    assert not dev.cpu().numpy().any()
    del imgs


# ---- transforms ---------------------------------------------------------------------------
def png_of(img):
    b = io.BytesIO()
    mode = {1: "L", 2: "LA", 3: "RGB", 4: "RGBA"}[1 if img.ndim == 2 else img.shape[2]]
    Image.fromarray(img, mode).save(b, format="PNG")
    return b.getvalue()


@pytest.fixture(scope="module")
def files():
    rgba = ikutil.synth(96, 64, 4, seed=21, pattern="S", alpha="random")
    rgb = ikutil.synth(96, 64, 3, seed=23, pattern="S")
    jb = io.BytesIO()
    Image.fromarray(rgb, "RGB").save(jb, format="JPEG", quality=90)
    return {"rgba": png_of(rgba), "rgb": png_of(rgb), "jpeg": jb.getvalue()}


def test_defaults_launch_nothing(ik, files):
    img = noise(9, 13, 4, 1, seed=5)
    d = DynamicImage.from_array(img)
    c0 = counters(ik)
    cp = d.adjust(Adjust())
    assert cp._h.value != d._h.value
    assert np.array_equal(cp.to_array(), img)
    # a gray image under a matrix alone: a copy too
    g = DynamicImage.from_array(img[..., :2].copy())
    assert np.array_equal(g.adjust(grayscale=True).to_array(), img[..., :2])
    for fmt, q in ((J, 85), (WP, 80)):
        for data in files.values():
            assert transform(data, 48, 32, fmt, q, adjust=Adjust()) == transform(data, 48, 32, fmt, q)
            assert transform(data, None, None, fmt, q, adjust=Adjust(gamma=0)) == transform(data, None, None, fmt, q)
    assert np.array_equal(counters(ik), c0)


def chain(data, w, h, a, fmt, q, sharpen=None, o=None):
    img, _ = decode_image(data)
    rs = resize_image(img, w, h).adjust(a)
    if sharpen:
        rs = rs.unsharpen(sharpen)
    if o is not None:
        rs = rs.overlay(o)
    return encode_image(rs, fmt, q)


@pytest.mark.parametrize("fmt,q", [(J, 85), (WP, 80)], ids=["jpeg85", "webp80"])
def test_transform_equals_the_chain(ik, files, fmt, q):
    mark = DynamicImage.from_array(noise(10, 24, 4, 1, seed=31))
    o = Overlay(mark, "se", -2, -2, 200)
    for data in (files["rgba"], files["rgb"], files["jpeg"]):
        for a in (Adjust(grayscale=True), adjust_of(VARIANTS["both"]), Adjust(gamma=2.2)):
            c0 = counters(ik)
            got = transform(data, 48, 32, fmt, q, adjust=a, sharpen=1.5, overlay=o)
            assert np.array_equal(counters(ik) - c0, (1, 1))
            assert got == chain(data, 48, 32, a, fmt, q, 1.5, o)
            assert got != transform(data, 48, 32, fmt, q, sharpen=1.5, overlay=o)
            # w and h both None: the decoded image itself is adjusted, in place, and it is the call's own
            assert transform(data, None, None, fmt, q, adjust=a, sharpen=1.5, overlay=o) == chain(
                data, None, None, a, fmt, q, 1.5, o)
            # the adjustment alone
            assert transform(data, 48, 32, fmt, q, adjust=a) == chain(data, 48, 32, a, fmt, q)
            assert transform(data, None, None, fmt, q, adjust=a) == chain(data, None, None, a, fmt, q)
