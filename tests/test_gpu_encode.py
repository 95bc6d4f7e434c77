"""GPU parity for encode_image's device front ends (reference src/transform.rs:113-150).

WebP: the device YUV420 planes must equal libwebp 1.2.2's own import (and the
oracle restatement); the WebP bytes must equal WebPEncodeRGB(to_rgb8(img), q)
byte for byte -- i.e. webp 0.3.1 Encoder::from_rgb(..).encode(q) on the same
libwebp.  JPEG: device coefficients (test_jpeg_coeffs_match_oracle) and bytes must
equal the image 0.25.8 JpegEncoder restatement byte for byte, and every byte test
says which coder wrote its scan -- k_jpeg_huff_enc, or the host coder for a stream
past the GPU coder's buffer (ik_jpeg_enc_counters) -- and that it is the one the
plain Python coder (tests/oracle_jpeg_huff.py) predicts.  AVIF: rav1e (the reference's AV1 encoder)
is absent, the build codes AV1 with libavif/aom: parity unpinned, checked as a
decoded-PSNR bound (Pillow/dav1d), dimensions, alpha handling and q-monotone size.
The AVIF front end itself (k_avif_yuv444: the Y, U, V, A planes and the transparent
flag) is compared with the oracle value for value in tests/test_gpu_avif_front.py."""
import ctypes
import io

import numpy as np
import pytest

import ikutil
import oracle_jpeg_huff as jh
from imagekit import DynamicImage, ImageFormat, encode_image, transform_batch

pytestmark = pytest.mark.gpu

SIZES = [(1, 1), (2, 3), (7, 5), (64, 48), (65, 49), (100, 100), (320, 240), (511, 257), (512, 512)]


def _dev_yuv(ik, img: np.ndarray):
    h, w, c = img.shape
    d = DynamicImage.from_array(img)
    uw, uh = (w + 1) // 2, (h + 1) // 2
    n = w * h + 2 * uw * uh
    dy = ctypes.c_void_p()
    assert ik.ik_dev_alloc(n, ctypes.byref(dy)) == 0
    try:
        # the image handle's device pointer/pitch are private: go through a fresh upload
        from imagekit import _lib
        pitch = ((w * c + 255) // 256) * 256
        ds = ctypes.c_void_p()
        assert ik.ik_dev_alloc(pitch * h + 16, ctypes.byref(ds)) == 0
        buf = np.zeros((h, pitch), np.uint8)
        buf[:, :w * c] = img.reshape(h, w * c)
        assert ik.ik_memcpy_h2d(ds, buf.ctypes.data, buf.nbytes) == 0
        assert ik.ik_webp_yuv420_device(ds, w, h, c, pitch, dy, None) == 0, _lib.last_error()
        assert ik.ik_dev_synchronize() == 0
        out = np.zeros(n, np.uint8)
        assert ik.ik_memcpy_d2h(out.ctypes.data, dy, n) == 0
        ik.ik_dev_free(ds)
    finally:
        ik.ik_dev_free(dy)
    del d
    return out[:w * h].reshape(h, w), out[w * h:w * h + uw * uh].reshape(uh, uw), \
        out[w * h + uw * uh:].reshape(uh, uw)


@pytest.mark.parametrize("wh", SIZES)
@pytest.mark.parametrize("c", [1, 3, 4])
def test_webp_yuv420_planes(ik, oracle, wh, c):
    w, h = wh
    img = ikutil.synth(w, h, c, seed=w + h, pattern="N")
    rgb = oracle.to_rgb8(img)
    gy, gu, gv = _dev_yuv(ik, img)
    ly, lu, lv = oracle.libwebp_import_yuv(rgb)
    np.testing.assert_array_equal(gy, ly)
    np.testing.assert_array_equal(gu, lu)
    np.testing.assert_array_equal(gv, lv)


@pytest.mark.parametrize("wh", [(1, 1), (7, 5), (64, 48), (320, 240), (512, 512)])
@pytest.mark.parametrize("q", [1, 10, 75, 80, 100])
def test_webp_bytes_match_libwebp(ik, oracle, wh, q):
    w, h = wh
    img = ikutil.synth(w, h, 4, seed=q, pattern="S")
    got = encode_image(DynamicImage.from_array(img), ImageFormat.webp, q)
    assert got == oracle.webp_encode_rgb(oracle.to_rgb8(img), float(q))


def _dev_jpeg_coeffs(ik, img: np.ndarray, q: int) -> np.ndarray:
    from imagekit import _lib
    h, w, c = img.shape
    nm = ((w + 7) // 8) * ((h + 7) // 8)
    pitch = ((w * c + 255) // 256) * 256
    buf = np.zeros((h, pitch), np.uint8)
    buf[:, :w * c] = img.reshape(h, w * c)
    out = np.full((nm, 3, 64), 0x7ABC, np.int16)
    ds, dc = ctypes.c_void_p(), ctypes.c_void_p()
    assert ik.ik_dev_alloc(buf.nbytes + 16, ctypes.byref(ds)) == 0
    assert ik.ik_dev_alloc(out.nbytes, ctypes.byref(dc)) == 0
    try:
        assert ik.ik_memcpy_h2d(ds, buf.ctypes.data, buf.nbytes) == 0
        assert ik.ik_memcpy_h2d(dc, out.ctypes.data, out.nbytes) == 0
        assert ik.ik_jpeg_coeffs_device(ds, w, h, c, pitch, q, dc, None) == 0, _lib.last_error()
        assert ik.ik_memcpy_d2h(out.ctypes.data, dc, out.nbytes) == 0
    finally:
        ik.ik_dev_free(ds)
        ik.ik_dev_free(dc)
    return out


def _coeff_patterns(w, h, c):
    """(name, (h, w, c) image): pattern S and N, the two flat extremes, saturated
    primaries and secondaries pixel by pixel, and a one-pixel black/white checker (the
    largest coefficients a block can hold; with the primaries, the `as u8` limits
    of the colour conversion).  Alpha, where there is one, is noise: to_rgb8 drops it."""
    yy, xx = np.mgrid[0:h, 0:w]
    colours = np.array([[255, 0, 0], [0, 255, 0], [0, 0, 255], [255, 255, 0], [0, 255, 255], [255, 0, 255]], np.uint8)
    prim = colours[(xx + 2 * yy) % 6]
    check = np.repeat((((xx + yy) & 1) * 255).astype(np.uint8)[..., None], 3, -1)
    alpha = ikutil.synth(w, h, 1, seed=w * h, pattern="N")

    def with_channels(rgb):
        if c == 3:
            return np.ascontiguousarray(rgb)
        if c == 1:
            return np.ascontiguousarray(rgb[..., :1])
        return np.ascontiguousarray(np.concatenate([rgb[..., :1] if c == 2 else rgb, alpha], -1))

    return [("S", ikutil.synth(w, h, c, seed=w + c, pattern="S")),
            ("N", ikutil.synth(w, h, c, seed=w + c, pattern="N", alpha="random")),
            ("all-0", np.zeros((h, w, c), np.uint8)),
            ("all-255", np.full((h, w, c), 255, np.uint8)),
            ("primaries", with_channels(prim)),
            ("checker", with_channels(check))]


# edge replication on both axes; 1, 2, 7, 8, 9, 13 and 169 MCUs against the
# coefficient kernel's 8-MCU workgroups
COEFF_SIZES = [(1, 1), (7, 5), (8, 8), (9, 9), (17, 7), (64, 8), (65, 49), (100, 100)]


@pytest.mark.parametrize("c", [1, 2, 3, 4])
@pytest.mark.parametrize("wh", COEFF_SIZES)
def test_jpeg_coeffs_match_oracle(ik, oracle, wh, c):
    """k_jpeg_coeffs (to_rgb8, YCbCr with `as u8`, edge replication, FDCT, quantise)
    against the oracle, coefficient for coefficient."""
    w, h = wh
    for name, img in _coeff_patterns(w, h, c):
        rgb = oracle.to_rgb8(img)
        for q in (1, 50, 100):
            np.testing.assert_array_equal(_dev_jpeg_coeffs(ik, img, q), oracle.jpeg_coeffs(rgb, q),
                                          err_msg=f"pattern {name}, q{q}: [mcu][component][natural index]")


def _enc_counts(ik):
    c = (ctypes.c_ulonglong * 2)()
    assert ik.ik_jpeg_enc_counters(c) == 0
    return np.array([c[0], c[1]], np.int64)  # [k_jpeg_huff_enc, host coder]


def _host_coded(ik, oracle, rgb, q):
    """Which coder the image must take: the GPU coder gives up exactly when twice
    the reference coder's unstuffed bytes exceed its buffer."""
    h, w, _ = rgb.shape
    return 2 * jh.code(oracle.jpeg_coeffs(rgb, q)).nbytes > ik.ik_jpeg_enc_capacity(w, h)


def _moved(host):
    return [0, 1] if host else [1, 0]


@pytest.mark.parametrize("wh", SIZES)
@pytest.mark.parametrize("q", [1, 10, 50, 85, 100])
def test_jpeg_bytes_match_oracle(ik, oracle, wh, q):
    w, h = wh
    img = ikutil.synth(w, h, 3, seed=q + w, pattern="S")
    c0 = _enc_counts(ik)
    got = encode_image(DynamicImage.from_array(img), ImageFormat.jpeg, q)
    moved = _enc_counts(ik) - c0
    assert got == oracle.jpeg_encode_rgb(img, q)
    assert moved.tolist() == _moved(_host_coded(ik, oracle, img, q))


@pytest.mark.parametrize("c", [1, 2, 4])
def test_jpeg_to_rgb8_channels(ik, oracle, c):
    img = ikutil.synth(37, 23, c, seed=c, pattern="N")
    c0 = _enc_counts(ik)
    got = encode_image(DynamicImage.from_array(img), ImageFormat.jpeg, 85)
    moved = _enc_counts(ik) - c0
    assert got == oracle.jpeg_encode_rgb(oracle.to_rgb8(img), 85)
    assert moved.tolist() == _moved(_host_coded(ik, oracle, oracle.to_rgb8(img), 85))


@pytest.mark.parametrize("pattern,q,host", [("N", 100, True), ("S", 50, False)])
def test_jpeg_coder_taken(ik, oracle, pattern, q, host):
    """64x48 noise at q100 does not fit the GPU coder's buffer and is coded on the
    host from the device coefficients; the smooth image is coded by k_jpeg_huff_enc.
    Both must match the oracle."""
    img = ikutil.synth(64, 48, 3, seed=3, pattern=pattern)
    assert _host_coded(ik, oracle, img, q) == host
    c0 = _enc_counts(ik)
    got = encode_image(DynamicImage.from_array(img), ImageFormat.jpeg, q)
    moved = _enc_counts(ik) - c0
    assert got == oracle.jpeg_encode_rgb(img, q)
    assert moved.tolist() == _moved(host)


def test_jpeg_group_with_one_host_coded_image(ik, oracle):
    """jpeg_front_group: four same-size PNG sources in one request, resized and coded
    at q100 in one coefficient and one Huffman launch.  The noise image does not fit
    the GPU coder's buffer and sits between GPU-coded neighbours."""
    from PIL import Image
    srcs = [ikutil.synth(128, 96, 3, seed=30 + k, pattern="N" if k == 1 else "S") for k in range(4)]
    blobs = []
    for s in srcs:
        buf = io.BytesIO()
        Image.fromarray(s).save(buf, format="PNG")
        blobs.append(buf.getvalue())
    rgbs = [oracle.to_rgb8(oracle.resize(s, 64, 48, ikutil.LANCZOS3)) for s in srcs]
    host = [_host_coded(ik, oracle, r, 100) for r in rgbs]
    assert host == [False, True, False, False]
    c0 = _enc_counts(ik)
    got = transform_batch(blobs, [(64, None)] * 4, [ImageFormat.jpeg] * 4, [100] * 4)
    moved = _enc_counts(ik) - c0
    bt = (ctypes.c_double * 13)()
    assert ik.ik_batch_last_timing(bt, 13) == 0
    for g, r in zip(got, rgbs):
        assert g == oracle.jpeg_encode_rgb(r, 100)
    assert moved.tolist() == [3, 1]
    assert bt[9] == 4  # all four went through the batched encoder's launch


def test_quality_clamp(ik, oracle):
    img = ikutil.synth(40, 30, 3, seed=1)
    d = DynamicImage.from_array(img)
    assert encode_image(d, ImageFormat.jpeg, 0) == oracle.jpeg_encode_rgb(img, 1)
    assert encode_image(d, ImageFormat.jpeg, 101) == oracle.jpeg_encode_rgb(img, 100)
    assert encode_image(d, ImageFormat.webp, 0) == oracle.webp_encode_rgb(img, 1.0)


# ---- AVIF (image AvifEncoder -> ravif/rav1e in the reference; libavif/aom here) ----
def _psnr(a, b):
    mse = np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2)
    return 99.0 if mse == 0 else 10 * np.log10(255.0 ** 2 / mse)


@pytest.mark.parametrize("wh", [(1, 1), (17, 9), (320, 240), (512, 512)])
def test_avif_encode_decodes_close_to_source(ik, wh):
    from PIL import Image
    w, h = wh
    src = ikutil.synth(w, h, 4, seed=w + h, pattern="S")
    b = encode_image(DynamicImage.from_array(src), ImageFormat.avif, 80)
    assert b[4:12] == b"ftypavif"
    im = Image.open(io.BytesIO(b))
    assert im.size == (w, h) and im.mode == "RGB"  # opaque source: no alpha plane
    if w * h >= 64:
        assert _psnr(np.asarray(im), src[..., :3]) > 30.0


def test_avif_alpha_and_gray(ik):
    from PIL import Image
    src = ikutil.synth(96, 64, 4, seed=3, pattern="S").copy()
    src[..., 3] = np.linspace(0, 255, 96, dtype=np.uint8)[None, :]
    im = Image.open(io.BytesIO(encode_image(DynamicImage.from_array(src), ImageFormat.avif, 90)))
    assert im.mode == "RGBA"
    a = np.asarray(im)
    assert np.abs(a[..., 3].astype(int) - src[..., 3]).max() <= 8
    g = ikutil.synth(40, 30, 1, seed=4, pattern="S")
    im = Image.open(io.BytesIO(encode_image(DynamicImage.from_array(g), ImageFormat.avif, 90)))
    rgb = np.asarray(im.convert("RGB")).astype(int)
    assert np.abs(rgb - g.repeat(3, axis=2)).mean() < 3.0


def test_avif_quality_orders_size(ik):
    img = DynamicImage.from_array(ikutil.synth(256, 256, 3, seed=9, pattern="N"))
    assert len(encode_image(img, ImageFormat.avif, 10)) < len(encode_image(img, ImageFormat.avif, 95))
