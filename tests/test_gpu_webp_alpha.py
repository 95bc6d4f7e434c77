"""GPU: lossy WebP files with an alpha plane on the device path (IK_WEBP_ALPHA_DECODE=gpu:
ik_vp8d_host.cpp reads the ALPH chunk's filtered plane, k_vp8d_alpha undoes libwebp's
prediction filter in place, the RGBA instantiation of k_vp8d_rgb writes the pixels).

Bar: all four channels identical to libwebp's WebPDecodeRGBA (tests/webp_alpha_util.py),
and ik_webp_counters moving by (1, 0) per file -- with IK_WEBP_DECODE=gpu a file the GPU
path leaves to libwebp is an error, so a pass proves the device decoded it.  The sizes
cover row 0 and column 0 alone, the band seam at row 64 and the skew's tail at 63, 64
and 65 columns, each with all four filters.  With the switch unset nothing changes: an
alpha file under IK_WEBP_DECODE=gpu is still an error."""
import ctypes

import numpy as np
import pytest

import ikutil
import webp_alpha_util as au
import webp_tool as wt
from imagekit import (FilterType, ImageFormat, TransformError, decode_image, decode_image_batch, transform_batch)
from imagekit.transform import transform

pytestmark = pytest.mark.gpu


def counters(lib):
    c = (ctypes.c_ulonglong * 2)()
    assert lib.ik_webp_counters(c) == 0
    return np.array([c[0], c[1]], dtype=np.int64)


def timing(lib):
    t = (ctypes.c_double * 13)()
    assert lib.ik_webp_last_timing(t, 13) == 0
    return list(t)


def same(got, want, what):
    assert got.shape == want.shape, what
    if not np.array_equal(got, want):
        bad = np.argwhere(np.any(got != want, axis=-1))
        y, x = bad[0]
        raise AssertionError(f"{what}: {len(bad)} pixels differ, first at ({x}, {y}): {got[y, x]} vs {want[y, x]}")


@pytest.fixture
def alpha_gpu(monkeypatch):
    monkeypatch.setenv("IK_WEBP_ALPHA_DECODE", "gpu")
    monkeypatch.setenv("IK_WEBP_DECODE", "gpu")


def check(lib, data: bytes, what: str):
    c0 = counters(lib)
    img, fmt = decode_image(data)
    assert list(counters(lib) - c0) == [1, 0], what
    assert fmt is ImageFormat.webp and img.channels == 4, what
    same(img.to_array(), au.decode_rgba(data), what)


PILLOW = au.pillow_files()


@pytest.mark.parametrize("k", range(len(PILLOW)), ids=[n for n, _ in PILLOW])
def test_pillow_files(ik, alpha_gpu, k):
    name, data = PILLOW[k]
    check(ik, data, name)


@pytest.mark.parametrize("filt", [0, 1, 2, 3])
@pytest.mark.parametrize("wh", au.SIZES, ids=[f"{w}x{h}" for w, h in au.SIZES])
def test_hand_built_filters(ik, alpha_gpu, wh, filt):
    w, h = wh
    for kind in ("noise", "smooth"):
        check(ik, au.hand_built(w, h, filt, kind), f"{w}x{h} filter {filt} {kind}")


def test_noise_alpha_333x222(ik, alpha_gpu):
    (item,) = au.pillow_files(sizes=[(333, 222)])[:1]
    assert au.alph_header(item[1])["compression"] == 0  # noise: a raw plane
    check(ik, item[1], "333x222 noise")
    for filt in (1, 2, 3):  # and every filter over several bands and chunks
        check(ik, au.hand_built(333, 222, filt), f"333x222 filter {filt}")


def test_broken_alpha_files(ik, monkeypatch):
    monkeypatch.setenv("IK_WEBP_ALPHA_DECODE", "gpu")
    for name, data in au.broken_files()[2:]:  # flag without chunk, short plane, reserved bits, truncated payload
        monkeypatch.setenv("IK_WEBP_DECODE", "gpu")
        with pytest.raises(TransformError):
            decode_image(data)
        monkeypatch.setenv("IK_WEBP_DECODE", "auto")
        try:
            want = au.decode_rgba(data)
        except ValueError:
            with pytest.raises(TransformError):
                decode_image(data)
            continue
        img, _ = decode_image(data)
        got = img.to_array()
        same(got, want if got.shape[-1] == 4 else wt.decode_rgb(data), name)


def test_switch_unset_changes_nothing(ik, monkeypatch):
    monkeypatch.delenv("IK_WEBP_ALPHA_DECODE", raising=False)
    data = au.hand_built(65, 64, 3)
    monkeypatch.setenv("IK_WEBP_DECODE", "gpu")
    with pytest.raises(TransformError):
        decode_image(data)
    with pytest.raises(TransformError):
        decode_image_batch([data])
    monkeypatch.setenv("IK_WEBP_ALPHA_DECODE", "host")
    with pytest.raises(TransformError):
        decode_image(data)
    monkeypatch.setenv("IK_WEBP_DECODE", "auto")
    c0 = counters(ik)
    img, _ = decode_image(data)
    assert list(counters(ik) - c0) == [0, 1]
    same(img.to_array(), au.decode_rgba(data), "host")


@pytest.fixture(scope="module")
def mixed():
    """(kind, bytes, libwebp's pixels): two opaque files, three alpha files (filters 1, 2, 3,
    different sizes), one lossless file, and an alpha file above the auto threshold."""
    rgba = ikutil.synth(40, 30, 4, seed=2, alpha="random")
    import io

    from PIL import Image
    b = io.BytesIO()
    Image.fromarray(rgba).save(b, format="WEBP", lossless=True, exact=True)
    files = [
        ("opaque", wt.encode(ikutil.synth(200, 150, 3, seed=6, pattern="N"), 60)),
        ("alpha", au.hand_built(130, 67, 1)),
        ("alpha", au.hand_built(64, 65, 2, "smooth")),
        ("lossless", b.getvalue()),
        ("opaque", wt.encode(ikutil.synth(97, 61, 3, seed=7, pattern="S"), 90)),
        ("alpha", au.hand_built(65, 64, 3)),
        ("alpha", au.hand_built(2048, 1536, 3, "smooth")),
    ]
    return [(k, d, wt.decode_rgb(d) if k == "opaque" else au.decode_rgba(d)) for k, d in files]


def test_mixed_batch(ik, monkeypatch, mixed):
    monkeypatch.setenv("IK_WEBP_ALPHA_DECODE", "gpu")
    monkeypatch.setenv("IK_WEBP_DECODE", "auto")
    assert 2048 * 1536 >= ik.ik_webp_gpu_min_batch_pixels()
    datas = [d for _, d, _ in mixed]
    for cap in (None, "60000"):
        if cap:
            monkeypatch.setenv("IK_VP8D_BATCH_BYTES", cap)
        c0 = counters(ik)
        res = decode_image_batch(datas)
        assert list(counters(ik) - c0) == [6, 1], cap  # all but the lossless file on the GPU
        t = timing(ik)
        assert (t[5], t[6], t[12]) == (6, 1, 4), cap
        assert t[9] == 1 if cap is None else t[9] >= 3, cap
        for (kind, _, want), (img, fmt) in zip(mixed, res):
            assert fmt is ImageFormat.webp
            same(img.to_array(), want, f"{kind} {want.shape} cap {cap}")


def test_transform_bytes_do_not_depend_on_the_switch(ik, monkeypatch):
    datas = [PILLOW[1][1], au.hand_built(130, 67, 3, "smooth"), PILLOW[0][1]]
    n = len(datas)
    out = {}
    for where in ("host", "gpu"):
        monkeypatch.setenv("IK_WEBP_ALPHA_DECODE", where)
        monkeypatch.setenv("IK_WEBP_DECODE", "gpu" if where == "gpu" else "auto")
        c0 = counters(ik)
        one = [[transform(d, 48, None, fmt, 80, FilterType.Triangle) for d in datas]
               for fmt in (ImageFormat.jpeg, ImageFormat.webp)]
        batch = [transform_batch(datas, [(48, None)] * n, [fmt] * n, [80] * n, FilterType.Triangle)
                 for fmt in (ImageFormat.jpeg, ImageFormat.webp)]
        assert list(counters(ik) - c0) == ([4 * n, 0] if where == "gpu" else [0, 4 * n]), where
        out[where] = (one, batch)
    for k in range(2):
        for i in range(n):
            assert out["gpu"][0][k][i] == out["host"][0][k][i], (k, i)
            assert bytes(out["gpu"][1][k][i]) == bytes(out["host"][1][k][i]), (k, i)
            assert bytes(out["gpu"][1][k][i]) == out["gpu"][0][k][i], (k, i)
