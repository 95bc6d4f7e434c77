"""GPU: ik_transform_batch's post stage follows its plan (csrc/ik_post_plan.h,
tests/test_post_plan.py) under the default IK_WEBP_AUTO encoder: 32 same-geometry WebP
requests go through the uniform exact call, 31 to libwebp on the host, and a geometry's
JPEG pair through the GPU JPEG coder beside its WebP pair.  Which coder ran is read from
the library's counters; every file is byte-identical to the oracle's transform.  One tiny
PNG serves every request -- the image size does not enter the routing."""
import ctypes
import io

import pytest

import ikutil

pytestmark = pytest.mark.gpu

AUTO, MIXED_HOST = 3, 0
W, H, NW, NH = 64, 48, 40, 30


@pytest.fixture(scope="module")
def source():
    from PIL import Image
    src = ikutil.synth(W, H, 3, seed=5, pattern="S")
    b = io.BytesIO()
    Image.fromarray(src, "RGB").save(b, format="PNG")
    return src, b.getvalue()


def webp_counters(ik):
    c = (ctypes.c_ulonglong * 4)()  # uniform exact, mixed exact, libwebp on the host, mixed calls
    assert ik.ik_webp_enc_counters(c) == 0
    return list(c)


def jpeg_counters(ik):
    c = (ctypes.c_ulonglong * 2)()  # GPU-coded, host-coded
    assert ik.ik_jpeg_enc_counters(c) == 0
    return list(c)


def run_auto(ik, png, fmts, qs):
    """transform_batch of len(fmts) requests for png at NW x NH under AUTO with the mixed
    call off; the files and what the WebP and JPEG coder counters gained."""
    from imagekit import FilterType, transform_batch
    n = len(fmts)
    encoder = ik.ik_get_webp_encoder()
    try:
        assert ik.ik_set_webp_encoder(AUTO) == 0
        assert ik.ik_set_webp_mixed(MIXED_HOST) == 0
        w0, j0 = webp_counters(ik), jpeg_counters(ik)
        out = transform_batch([png] * n, [(NW, NH)] * n, fmts, qs, FilterType.Lanczos3)
        w1, j1 = webp_counters(ik), jpeg_counters(ik)
    finally:
        ik.ik_set_webp_mixed(-1)  # back to the environment's
        ik.ik_set_webp_encoder(encoder)
    return out, [b - a for a, b in zip(w0, w1)], [b - a for a, b in zip(j0, j1)]


def test_32_same_geometry_requests_take_the_uniform_exact_call(ik, oracle, source):
    from imagekit import ImageFormat
    src, png = source
    want, dims = oracle.transform(src, NW, NH, ikutil.LANCZOS3, ImageFormat.webp.value, 80)
    assert dims == (NW, NH)
    out, dw, _ = run_auto(ik, png, [ImageFormat.webp] * 32, [80] * 32)
    assert dw == [32, 0, 0, 0], "all 32 by the uniform exact call, none on the host"
    assert out == [want] * 32


def test_31_same_geometry_requests_go_to_the_host_coder(ik, oracle, source):
    from imagekit import ImageFormat
    src, png = source
    want, _ = oracle.transform(src, NW, NH, ikutil.LANCZOS3, ImageFormat.webp.value, 80)
    out, dw, _ = run_auto(ik, png, [ImageFormat.webp] * 31, [80] * 31)
    assert dw == [0, 0, 31, 0], "all 31 by libwebp on the host, none by the uniform call"
    assert out == [want] * 31


def test_a_jpeg_pair_and_a_webp_pair_of_one_geometry(ik, oracle, source):
    from imagekit import ImageFormat
    src, png = source
    fmts = [ImageFormat.jpeg, ImageFormat.webp, ImageFormat.jpeg, ImageFormat.webp]
    qs = [85, 80, 85, 80]
    want = [oracle.transform(src, NW, NH, ikutil.LANCZOS3, f.value, q)[0] for f, q in zip(fmts, qs)]
    out, dw, dj = run_auto(ik, png, fmts, qs)
    assert dj == [2, 0], "the JPEG pair coded on the GPU"
    assert dw == [0, 0, 2, 0], "the WebP pair by libwebp on the host"
    assert out == want
