"""GPU: fit=cover / fit=exact.  A cover output is the oracle's resize to the virtual size
iw x ih (image 0.25.8 imageops::resize restated) sliced [y0:y0+nh, x0:x0+nw]: bit for bit
in the default mode, within 1 LSB in the FMA mode.  ik_resize_plan_info_window says which
kernel family every launch takes.  Then the destination padding, the plan cache across
exact and cover plans of one output size, CONTAIN against the calls without a fit, and a
48-request batch with the fits mixed against the oracle's files."""
import ctypes
import io

import numpy as np
import pytest

import ikutil
import oracle_np
from resize_model import FUSED, NAIVE, PERIODIC
from resize_window_model import CASES, CONTAIN, COVER, EXACT, LANCZOS3, TRIANGLE, fit_reference, oracle_window

pytestmark = pytest.mark.gpu
IK_RESIZE_EXACT, IK_RESIZE_FMA = 0, 1
POISON = 0xA5
AUTO, MIXED_HOST = 3, 0


def family_of(ik, W, H, C, win, f, n):
    out = (ctypes.c_int32 * 13)()
    assert ik.ik_resize_plan_info_window(W, H, C, *win, int(f), n, out, 13) == 13
    return out[12]


def device_window(ik, imgs, win, f, dst_pitch=None, dst_gap=0):
    """imgs (n, H, W, C) through ik_resize_window_batch_device.  The source allocation ends
    with its last row (rows W * C apart, a multiple of 8 in every case; images back to back).
    The destination is prefilled with POISON, rows dst_pitch apart, images dst_pitch * nh +
    dst_gap apart.
    Returns the (n, nh, nw, C) pixels after checking that no byte outside them changed."""
    n, H, W, C = imgs.shape
    nw, nh = win[4], win[5]
    pitch = W * C
    assert pitch % 8 == 0
    dst_pitch = dst_pitch or nw * C
    stride, dstride = pitch * H, dst_pitch * nh + dst_gap
    src = np.ascontiguousarray(imgs).reshape(-1)
    dst = np.full(n * dstride, POISON, np.uint8)
    d_src, d_dst = ctypes.c_void_p(), ctypes.c_void_p()
    assert ik.ik_dev_alloc(src.nbytes, ctypes.byref(d_src)) == 0
    assert ik.ik_dev_alloc(dst.nbytes, ctypes.byref(d_dst)) == 0
    try:
        assert ik.ik_memcpy_h2d(d_src, src.ctypes.data, src.nbytes) == 0
        assert ik.ik_memcpy_h2d(d_dst, dst.ctypes.data, dst.nbytes) == 0
        assert ik.ik_resize_window_batch_device(d_src, W, H, C, pitch, stride, n, *win, int(f), d_dst, dst_pitch,
                                                dstride, None) == 0
        assert ik.ik_dev_synchronize() == 0
        assert ik.ik_memcpy_d2h(dst.ctypes.data, d_dst, dst.nbytes) == 0
    finally:
        ik.ik_dev_free(d_src)
        ik.ik_dev_free(d_dst)
    out = np.zeros((n, nh, nw, C), np.uint8)
    keep = np.ones(dst.size, bool)
    for i in range(n):
        rows = dst[i * dstride:i * dstride + dst_pitch * nh].reshape(nh, dst_pitch)
        out[i] = rows[:, :nw * C].reshape(nh, nw, C)
        keep[i * dstride:i * dstride + dst_pitch * nh].reshape(nh, dst_pitch)[:, :nw * C] = False
    assert (dst[keep] == POISON).all(), "a store outside the window's nw x nh pixels"
    return out


def noise(n, W, H, C, seed):
    return np.stack([ikutil.synth(W, H, C, seed=seed + i, pattern="N", alpha="random") for i in range(n)])


@pytest.fixture()
def fma_mode(ik):
    mode = ik.ik_get_resize_mode()
    assert ik.ik_set_resize_mode(IK_RESIZE_FMA) == 0
    yield
    assert ik.ik_set_resize_mode(mode) == 0


# ---- 6. pixel parity against the oracle crop --------------------------------------------
@pytest.mark.parametrize("c", CASES, ids=lambda c: c.name)
def test_cover_equals_the_oracle_crop(ik, oracle, c):
    assert ik.ik_get_resize_mode() == IK_RESIZE_EXACT
    win = fit_reference(oracle, c.W, c.H, c.tw, c.th, COVER)
    assert family_of(ik, c.W, c.H, c.C, win, c.f, 1) == c.family
    imgs = noise(1, c.W, c.H, c.C, seed=c.W + c.C)
    got = device_window(ik, imgs, win, c.f)
    np.testing.assert_array_equal(got[0], oracle_window(oracle, imgs[0], win, c.f))


@pytest.mark.parametrize("c", CASES, ids=lambda c: c.name)
def test_cover_fma_within_one_lsb(ik, oracle, fma_mode, c):
    win = fit_reference(oracle, c.W, c.H, c.tw, c.th, COVER)
    # the FMA mode has no periodic kernel: those plans take the fused one
    assert family_of(ik, c.W, c.H, c.C, win, c.f, 1) == (NAIVE if c.family == NAIVE else FUSED)
    imgs = noise(1, c.W, c.H, c.C, seed=c.W + c.C)
    got = device_window(ik, imgs, win, c.f)
    want = oracle_window(oracle, imgs[0], win, c.f)
    assert np.abs(got[0].astype(int) - want.astype(int)).max() <= 1


def test_tall_virtual_image(ik, oracle):
    """1 x 4000 -> cover 4000 x 8: eight rows of a virtual 4000 x 16,000,000 image."""
    from imagekit import DynamicImage, FitMode, resize_image
    src = (np.arange(4000, dtype=np.uint32) * 7 % 256).astype(np.uint8).reshape(4000, 1, 1)
    out = resize_image(DynamicImage.from_array(src), 4000, 8, ikutil.TRIANGLE, fit=FitMode.cover).to_array()
    assert out.shape == (8, 4000, 1)
    # the oracle cannot resize to 16,000,000 rows; the eight rows' own weights can be applied
    F = np.float32
    ratio = F(4000) / F(16000000)
    for r in range(8):
        c = (F(7999996 + r) + F(0.5)) * ratio
        left = min(max(int(np.floor(c - F(1))), 0), 3999)
        right = min(max(int(np.ceil(c + F(1))), left + 1), 4000)
        c = c - F(0.5)
        w = [max(F(1) - abs(F(i) - c), F(0)) for i in range(left, right)]
        s = F(0)
        for x in w:
            s = F(s + x)
        t = F(0)
        for k, x in enumerate(w):
            t = F(t + F(F(src[left + k, 0, 0]) * F(x / s)))
        # the horizontal pass of a one-pixel row has one tap of weight 1
        assert (out[r] == int(np.floor(np.clip(t, 0, 255) + F(0.5)))).all()


@pytest.mark.parametrize("C", [3, 2], ids=["Rgb16", "La16"])
@pytest.mark.parametrize("g", [(200, 60, 50, 40), (60, 200, 40, 50)], ids=["col", "row"])
@pytest.mark.parametrize("f", [TRIANGLE, LANCZOS3])
def test_cover_16_bit(ik, oracle, C, g, f):
    """16-bit images resize through the two-pass pair only: its column range and row origin."""
    from imagekit import DynamicImage, FitMode, resize_image
    W, H, tw, th = g
    iw, ih, x0, y0, nw, nh = win = fit_reference(oracle, W, H, tw, th, COVER)
    with np.errstate(over="ignore"):
        src = (ikutil.splitmix64(900 + C, W * H * C) & np.uint64(0xFFFF)).astype(np.uint16).reshape(H, W, C)
    out = resize_image(DynamicImage.from_array(src), tw, th, f, fit=FitMode.cover)
    assert out.depth == 2 and out.dimensions() == (nw, nh)
    want = oracle_np.resize(src, iw, ih, f)[y0:y0 + nh, x0:x0 + nw]
    np.testing.assert_array_equal(out.to_array(), want)


# ---- 7. poisoned padding ----------------------------------------------------------------
PADDING = [c for c in CASES if c.name in ("col-f4-c4", "row-f1-c3", "rgba-mid-strip", "rgb-odd-origin-phi2",
                                          "periodic-row-odd-y0", "rgb-odd-origin-periodic", "naive-upscale-c3",
                                          "naive-col-crop", "col-f0-c1", "row-f4-c2")]


@pytest.mark.parametrize("c", PADDING, ids=lambda c: c.name)
def test_poisoned_padding(ik, oracle, c):
    """n = 3 images into a pitch-padded destination with a gap between the images: the bytes
    outside nw x nh keep the sentinel (device_window checks it), the pixels are the oracle's."""
    win = fit_reference(oracle, c.W, c.H, c.tw, c.th, COVER)
    assert family_of(ik, c.W, c.H, c.C, win, c.f, 3) == c.family
    imgs = noise(3, c.W, c.H, c.C, seed=31 + c.C)
    got = device_window(ik, imgs, win, c.f, dst_pitch=(win[4] * c.C + 255) // 256 * 256 + 256, dst_gap=1024)
    for i in range(3):
        np.testing.assert_array_equal(got[i], oracle_window(oracle, imgs[i], win, c.f))


def test_window_outside_the_virtual_image_is_refused(ik):
    from imagekit import DynamicImage, _lib
    img = DynamicImage.from_array(np.zeros((8, 8, 3), np.uint8))
    out = ctypes.c_void_p()
    for win in ((4, 4, 1, 0, 4, 4), (4, 4, 0, 2, 4, 3), (4, 4, 0, 0, 0, 4), (4, 4, 4, 0, 1, 1)):
        assert ik.ik_resize_window(img._h, *win, LANCZOS3, ctypes.byref(out)) == 2, win
        assert not out.value and _lib.last_error()


# ---- 8. plan cache ----------------------------------------------------------------------
@pytest.mark.parametrize("g,order", [((208, 60, 3, 50, 40), (EXACT, COVER, EXACT)),
                                     ((60, 208, 4, 40, 50), (COVER, EXACT, COVER))], ids=["exact-first", "cover-first"])
def test_exact_and_cover_plans_of_one_output_size(ik, oracle, g, order):
    from imagekit import DynamicImage, resize_image
    W, H, C, tw, th = g
    src = noise(1, W, H, C, seed=W)[0]
    img = DynamicImage.from_array(src)
    for fit in order:
        win = fit_reference(oracle, W, H, tw, th, fit)
        assert win[4:] == (tw, th)
        got = resize_image(img, tw, th, TRIANGLE, fit=fit).to_array()
        np.testing.assert_array_equal(got, oracle_window(oracle, src, win, TRIANGLE))


# ---- 9. behaviour unchanged -------------------------------------------------------------
def _png(px):
    from PIL import Image
    b = io.BytesIO()
    Image.fromarray(px, {3: "RGB", 4: "RGBA"}[px.shape[2]]).save(b, format="PNG")
    return b.getvalue()


def _jpeg(px):
    from PIL import Image
    b = io.BytesIO()
    Image.fromarray(px, "RGB").save(b, format="JPEG", quality=90, subsampling=2)
    return b.getvalue()


@pytest.fixture(scope="module")
def sources():
    a = ikutil.synth(640, 360, 4, seed=41, pattern="S")
    b = ikutil.synth(360, 480, 3, seed=42, pattern="S")
    return [(a, _png(a)), (b, _jpeg(b))]


def test_contain_is_the_call_without_a_fit(ik, sources):
    from imagekit import DynamicImage, FitMode, ImageFormat, resize_image, transform_batch
    from imagekit.transform import transform
    img = DynamicImage.from_array(sources[0][0])
    for w, h in ((100, 100), (100, None), (None, 77), (640, 360), (0, 5)):
        out = ctypes.c_void_p()
        assert ik.ik_resize(img._h, -1 if w is None else w, -1 if h is None else h, LANCZOS3, ctypes.byref(out)) == 0
        plain = DynamicImage(out.value)
        np.testing.assert_array_equal(resize_image(img, w, h, fit=FitMode.contain).to_array(), plain.to_array())
    assert resize_image(img, None, None, fit=FitMode.cover) is img
    datas = [s[1] for s in sources] * 4
    sizes = [(100, 100), (100, None), (None, 77), (90, 120)] * 2
    fmts = [ImageFormat.webp, ImageFormat.jpeg] * 4
    qs = [80, 85] * 4
    plain = transform_batch(datas, sizes, fmts, qs)
    assert transform_batch(datas, sizes, fmts, qs, fits=[FitMode.contain] * 8) == plain
    for k in (0, 1):
        assert transform(datas[k], *sizes[k], fmts[k], qs[k], fit=FitMode.contain) == plain[k]
        assert transform(datas[k], *sizes[k], fmts[k], qs[k]) == plain[k]


# ---- 10. end to end ---------------------------------------------------------------------
def test_batch_with_mixed_fits_equals_the_oracle(ik, oracle, sources):
    """48 requests over a PNG and a baseline JPEG source, the fits mixed per request, JPEG
    and WebP outputs; 32 of them are one cover geometry coded as WebP q80, which the default
    IK_WEBP_AUTO encoder hands to the exact GPU coder in one call."""
    from imagekit import FilterType, FitMode, ImageFormat, transform_batch
    from imagekit.transform import transform
    WEBP, JPEG = ImageFormat.webp, ImageFormat.jpeg
    reqs = [(0, 128, 128, FitMode.cover, WEBP, 80)] * 32
    reqs += [(0, 128, 128, FitMode.exact, WEBP, 80), (0, 128, 128, FitMode.exact, WEBP, 80),      # the same output size
             (0, 128, 128, FitMode.contain, WEBP, 80), (0, 128, 128, FitMode.contain, JPEG, 85),
             (1, 100, 100, FitMode.cover, JPEG, 85), (1, 100, 100, FitMode.cover, JPEG, 85),      # a row crop, grouped
             (1, 100, 100, FitMode.exact, JPEG, 85), (1, 100, 100, FitMode.exact, JPEG, 85),
             (1, 100, 100, FitMode.contain, WEBP, 70), (1, 61, 200, FitMode.cover, WEBP, 70),
             (0, 200, 61, FitMode.cover, JPEG, 60), (0, 77, None, FitMode.cover, WEBP, 80),       # one side None
             (1, 360, 480, FitMode.cover, JPEG, 85), (1, 180, 480, FitMode.cover, WEBP, 80),      # no resampling
             (0, 640, 90, FitMode.exact, JPEG, 85), (1, None, 33, FitMode.exact, WEBP, 80)]
    assert len(reqs) == 48
    px = [sources[0][0], oracle.jpeg_decode(sources[1][1], mode=1)]
    datas = [sources[r[0]][1] for r in reqs]
    c = (ctypes.c_ulonglong * 4)()
    encoder = ik.ik_get_webp_encoder()
    try:
        assert ik.ik_set_webp_encoder(AUTO) == 0 and ik.ik_set_webp_mixed(MIXED_HOST) == 0
        assert ik.ik_webp_enc_counters(c) == 0
        exact0 = c[0]
        got = transform_batch(datas, [(r[1], r[2]) for r in reqs], [r[4] for r in reqs], [r[5] for r in reqs],
                              FilterType.Lanczos3, fits=[r[3] for r in reqs])
        assert ik.ik_webp_enc_counters(c) == 0
        assert c[0] - exact0 == 32, "the cover group of 32 goes to the uniform exact call"
        memo = {}
        for k, (s, w, h, fit, fmt, q) in enumerate(reqs):
            if (s, w, h, fit, fmt, q) not in memo:
                H, W = px[s].shape[:2]
                win = fit_reference(oracle, W, H, w, h, int(fit))
                rgb = oracle.to_rgb8(np.ascontiguousarray(oracle_window(oracle, px[s], win, LANCZOS3)))
                want = oracle.webp_encode_rgb(rgb, float(q)) if fmt is WEBP else oracle.jpeg_encode_rgb(rgb, q)
                memo[(s, w, h, fit, fmt, q)] = (want, transform(datas[k], w, h, fmt, q, fit=fit))
            want, single = memo[(s, w, h, fit, fmt, q)]
            assert got[k] == single, f"request {k} {reqs[k][1:]}: the batch differs from ik_transform_fit"
            assert got[k] == want, f"request {k} {reqs[k][1:]}: the file differs from the oracle's"
    finally:
        ik.ik_set_webp_mixed(-1)
        ik.ik_set_webp_encoder(encoder)
