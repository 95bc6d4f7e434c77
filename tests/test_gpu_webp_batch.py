"""GPU: a batch's lossy WebP inputs decoded together (decode_webp_batch, ik_vp8d_host.cpp:
the host workers parse partition 0 and the tokens of every file in parallel, then one
staged area, one k_vp8d_recon launch handing out (image, MB row) tickets over all the
frames, one k_vp8d_rgb launch over the plan's row tiles).

Bar: the pixels of libwebp's WebPDecodeRGB (tests/webp_tool.py), as for the one-request
decoder (tests/test_gpu_webp_decode.py), and per item the status decode_image gives on
the same bytes.  Every case asserts through ik_webp_counters how many streams the GPU
reconstructed: the number of plain lossy files it sent, no fewer.  IK_VP8D_GRID=3 makes
three waves wrap through every ticket of the batch (and across image boundaries);
IK_VP8D_BATCH_BYTES forces the split into sub-launches."""
import ctypes
import io

import numpy as np
import pytest
from PIL import Image

import ikutil
import webp_tool as wt
from imagekit import (DeviceBytes, DynamicImage, FilterType, ImageFormat, TransformError, _lib, decode_image,
                      decode_image_batch, transform_batch, transform_batch_submit_device)
from imagekit.transform import transform

pytestmark = pytest.mark.gpu

LEFT = "leaves this file to libwebp"


def counters(lib):
    c = (ctypes.c_ulonglong * 2)()
    assert lib.ik_webp_counters(c) == 0
    return np.array([c[0], c[1]], dtype=np.int64)


def timing(lib):
    t = (ctypes.c_double * 10)()
    assert lib.ik_webp_last_timing(t, 10) == 0
    return list(t)


def decode_batch_status(lib, datas):
    """ik_decode_batch with its per-item results: (pixels or None, format, status) per
    item, the call's status and its error message."""
    n = len(datas)
    bufs = [bytes(d) for d in datas]
    ptrs = (ctypes.c_void_p * n)(*[ctypes.cast(ctypes.c_char_p(b), ctypes.c_void_p) for b in bufs])
    lens = (ctypes.c_size_t * n)(*[len(b) for b in bufs])
    outs = (ctypes.c_void_p * n)()
    fmts = (ctypes.c_int * n)()
    status = (ctypes.c_int * n)()
    rc = lib.ik_decode_batch(ptrs, lens, n, outs, fmts, status)
    msg = _lib.last_error() if rc else ""
    items = []
    for i in range(n):
        px = DynamicImage(outs[i]).to_array() if outs[i] else None
        items.append((px, fmts[i], status[i]))
    return items, rc, msg


def decode_one_status(lib, data):
    out = ctypes.c_void_p()
    fmt = ctypes.c_int(-1)
    st = lib.ik_decode(data, len(data), ctypes.byref(out), ctypes.byref(fmt))
    msg = _lib.last_error() if st else ""
    if out.value:
        DynamicImage(out.value)  # (freed with the wrapper)
    return st, msg


def same(got, want, what):
    assert got.shape == want.shape, what
    if not np.array_equal(got, want):
        bad = np.argwhere(np.any(got != want, axis=-1))
        y, x = bad[0]
        raise AssertionError(f"{what}: {len(bad)} pixels differ, first at ({x}, {y}): {got[y, x]} vs {want[y, x]}")


def gpu_batch(lib, datas, what):
    """decode_image_batch of plain lossy files: all of them on the GPU, libwebp's pixels."""
    c0 = counters(lib)
    res = decode_image_batch(datas)
    assert list(counters(lib) - c0) == [len(datas), 0], what
    t = timing(lib)
    assert (t[5], t[6]) == (len(datas), 0)
    out = []
    for i, (img, fmt) in enumerate(res):
        assert fmt is ImageFormat.webp
        out.append(img.to_array())
    return out, t


# ---- the geometry batch: one MB, 2x2 MBs (the min(mb_x + 2, mb_w) wait at mb_w = 2), one
# MB column (every row waits for need = 1), one MB row (no wait at all), ragged sizes,
# a tall narrow frame, smooth and noisy VGA frames over the quality range ----
GEOMETRY = [(1, 1, "S", 80), (16, 16, "S", 80), (17, 17, "N", 80), (15, 200, "S", 80), (200, 15, "N", 80),
            (33, 49, "N", 80), (64, 2049, "S", 80), (640, 480, "S", 80), (640, 480, "N", 30), (640, 480, "N", 80),
            (640, 480, "N", 100)]


@pytest.fixture(scope="module")
def geometry():
    datas = [wt.encode(ikutil.synth(w, h, 3, seed=31 * w + h + q, pattern=p), q) for w, h, p, q in GEOMETRY]
    return datas, [wt.decode_rgb(d) for d in datas]


def test_geometry_batch(ik, monkeypatch, geometry):
    monkeypatch.setenv("IK_WEBP_DECODE", "gpu")
    datas, want = geometry
    got, t = gpu_batch(ik, datas, "geometry")
    for g, w, spec in zip(got, want, GEOMETRY):
        same(g, w, str(spec))
    assert t[9] == 1 and t[7] == sum((h + 15) // 16 for _, h, _, _ in GEOMETRY)


def test_geometry_batch_three_waves(ik, monkeypatch, geometry):
    monkeypatch.setenv("IK_WEBP_DECODE", "gpu")
    monkeypatch.setenv("IK_VP8D_GRID", "3")
    datas, want = geometry
    got, t = gpu_batch(ik, datas, "grid 3")
    for g, w, spec in zip(got, want, GEOMETRY):
        same(g, w, f"grid 3 {spec}")
    assert t[8] == 3 and t[9] == 1


def test_geometry_batch_sub_launches(ik, monkeypatch, geometry):
    monkeypatch.setenv("IK_WEBP_DECODE", "gpu")
    monkeypatch.setenv("IK_VP8D_BATCH_BYTES", "600000")  # (a VGA frame's planes alone are 460 KB)
    datas, want = geometry
    got, t = gpu_batch(ik, datas, "sub-launches")
    for g, w, spec in zip(got, want, GEOMETRY):
        same(g, w, f"split {spec}")
    assert t[9] >= 3
    monkeypatch.setenv("IK_VP8D_GRID", "3")
    got, t = gpu_batch(ik, datas, "sub-launches, grid 3")
    for g, w, spec in zip(got, want, GEOMETRY):
        same(g, w, f"split, grid 3 {spec}")
    assert t[9] >= 3 and t[8] == 3


CONFIGS = [
    dict(segments=1, sns_strength=0),
    dict(segments=2),
    dict(segments=4, sns_strength=100),
    dict(filter_strength=0),
    dict(filter_type=0, filter_strength=60),
    dict(filter_type=0, filter_strength=100, filter_sharpness=5),
    dict(filter_strength=100, filter_sharpness=7),
    dict(filter_strength=40, filter_sharpness=2),
    dict(method=0, partitions=1),
    dict(method=0, partitions=2),
    dict(method=1, partitions=3, filter_type=0, filter_strength=50),
    dict(method=2, partitions=3, segments=4),
    dict(method=6),
    dict(method=3, autofilter=1),
]


def test_bitstream_features_in_one_batch(ik, monkeypatch):
    # segments, the three filter types, sharpness, 1..8 token partitions, methods 0..6
    monkeypatch.setenv("IK_WEBP_DECODE", "gpu")
    monkeypatch.setenv("IK_VP8D_GRID", "3")
    datas = [wt.encode(ikutil.synth(301 - 16 * (k % 3), 257, 3, seed=13 + k, pattern="SN"[k & 1]), 75, **c)
             for k, c in enumerate(CONFIGS)]
    got, _ = gpu_batch(ik, datas, "configurations")
    for g, d, c in zip(got, datas, CONFIGS):
        same(g, wt.decode_rgb(d), str(c))


def test_many_small_frames(ik, monkeypatch):
    # 40 frames of two MB rows each: more images than a small grid has waves
    monkeypatch.setenv("IK_WEBP_DECODE", "gpu")
    datas = [wt.encode(ikutil.synth(48, 32, 3, seed=100 + s, pattern="SN"[s & 1]), 80) for s in range(40)]
    want = [wt.decode_rgb(d) for d in datas]
    for grid in (None, "3"):
        if grid:
            monkeypatch.setenv("IK_VP8D_GRID", grid)
        got, t = gpu_batch(ik, datas, f"40 small, grid {grid}")
        for s in range(40):
            same(got[s], want[s], f"seed {s}, grid {grid}")
        assert t[7] == 80 and (grid is None or t[8] == 3)


def _truncate_tokens(data: bytes, keep: float) -> bytes:
    # cut the token partition short and rewrite the chunk and RIFF sizes, so that
    # the container is consistent and only the token data runs out
    f = bytearray(data[20:])
    part0 = (f[0] | f[1] << 8 | f[2] << 16) >> 5
    start = 10 + part0
    cut = start + max(1, int((len(f) - start) * keep))
    f = bytes(f[:cut])
    if len(f) & 1:
        f += b"\x00"
    body = b"WEBP" + b"VP8 " + len(f).to_bytes(4, "little") + f
    return b"RIFF" + len(body).to_bytes(4, "little") + body


def _save(px, fmt, **kw):
    b = io.BytesIO()
    Image.fromarray(px).save(b, format=fmt, **kw)
    return b.getvalue()


@pytest.fixture(scope="module")
def mixed():
    """(name, bytes) of one batch: plain lossy files (the first above the auto threshold
    alone), the WebP kinds the GPU path leaves to libwebp, two broken files, a JPEG, a PNG."""
    rgba = ikutil.synth(40, 30, 4, seed=2, alpha="random")
    rgb = ikutil.synth(120, 90, 3, seed=4, pattern="S")
    return [
        ("lossy", wt.encode(ikutil.synth(2048, 1536, 3, seed=5, pattern="S"), 80)),
        ("alpha", _save(rgba, "WEBP", quality=80)),
        ("lossy", wt.encode(ikutil.synth(200, 150, 3, seed=6, pattern="N"), 60)),
        ("lossless", _save(rgba, "WEBP", lossless=True, exact=True)),
        ("truncated", _truncate_tokens(wt.encode(ikutil.synth(200, 150, 3, seed=8, pattern="N"), 90), 0.5)),
        ("stub", b"RIFF\x04\x00\x00\x00WEBP"),
        ("jpeg", _save(rgb, "JPEG", quality=90)),
        ("png", _save(rgb, "PNG")),
        ("lossy", wt.encode(ikutil.synth(97, 61, 3, seed=7, pattern="S"), 90)),
    ]


def test_mixed_verdicts_auto(ik, monkeypatch, mixed):
    monkeypatch.setenv("IK_WEBP_DECODE", "auto")
    assert 2048 * 1536 >= ik.ik_webp_gpu_min_batch_pixels()
    datas = [d for _, d in mixed]
    c0 = counters(ik)
    items, rc, msg = decode_batch_status(ik, datas)
    dc = counters(ik) - c0
    assert list(dc) == [3, 4], "the lossy files on the GPU; alpha, lossless, truncated and stub handed to libwebp"
    t = timing(ik)
    assert (t[5], t[6]) == (3, 4)
    assert rc != 0 and msg.startswith("input 4:")
    for (name, d), (px, fmt, st) in zip(mixed, items):
        one_st, _ = decode_one_status(ik, d)
        assert st == one_st, name  # decode_image's status on the same bytes
        if name in ("truncated", "stub"):
            assert st != 0 and px is None
            with pytest.raises(TransformError):
                decode_image(d)
        elif name in ("alpha", "lossless"):
            assert st == 0 and px.shape == (30, 40, 4) and fmt == ImageFormat.webp.value
        elif name == "lossy":
            assert st == 0 and fmt == ImageFormat.webp.value
            same(px, wt.decode_rgb(d), name)
        else:
            assert st == 0 and px.shape == (90, 120, 3)
            assert fmt == (ImageFormat.jpeg.value if name == "jpeg" else -1)


def test_mixed_verdicts_gpu_only(ik, monkeypatch, mixed):
    monkeypatch.setenv("IK_WEBP_DECODE", "gpu")
    datas = [d for _, d in mixed]
    c0 = counters(ik)
    items, rc, msg = decode_batch_status(ik, datas)
    assert list(counters(ik) - c0) == [3, 0]
    assert rc != 0 and msg.startswith("input 1:") and LEFT in msg
    for (name, d), (px, fmt, st) in zip(mixed, items):
        one_st, one_msg = decode_one_status(ik, d)
        assert st == one_st, name
        if name in ("alpha", "lossless", "truncated", "stub"):
            assert st != 0 and px is None and LEFT in one_msg
        elif name == "lossy":
            assert st == 0
            same(px, wt.decode_rgb(d), name)
        else:
            assert st == 0 and px.shape == (90, 120, 3)
    # each handed-back file alone: the batch's message is the one-request path's
    for k in (1, 3, 4, 5):
        _, rc, msg = decode_batch_status(ik, [datas[k]])
        assert rc != 0 and LEFT in msg, mixed[k][0]


def test_auto_policy(ik, monkeypatch):
    # under the threshold: libwebp, as for ik_decode; the same frames repeated past it:
    # the GPU; the pixels are WebPDecodeRGB's either way
    monkeypatch.delenv("IK_WEBP_DECODE", raising=False)
    thr = ik.ik_webp_gpu_min_batch_pixels()
    assert thr > 0
    datas = [wt.encode(ikutil.synth(640, 480, 3, seed=40 + s, pattern="SN"[s & 1]), 80) for s in range(3)]
    want = [wt.decode_rgb(d) for d in datas]
    assert 3 * 640 * 480 < thr, "the policy test's small batch must lie under the threshold"
    c0 = counters(ik)
    small = decode_image_batch(datas)
    assert list(counters(ik) - c0) == [0, 3]
    reps = -(-thr // (3 * 640 * 480))
    c0 = counters(ik)
    big = decode_image_batch(datas * reps)
    assert list(counters(ik) - c0) == [3 * reps, 0]
    for i in range(3):
        same(small[i][0].to_array(), want[i], f"host {i}")
    for i in range(3 * reps):
        same(big[i][0].to_array(), want[i % 3], f"gpu {i}")


def test_transform_batch(ik, monkeypatch):
    monkeypatch.setenv("IK_WEBP_DECODE", "gpu")
    geo = [(640, 480), (333, 222), (100, 700), (1023, 769)]
    datas = [wt.encode(ikutil.synth(*geo[s % 4], 3, seed=60 + s, pattern="S"), 80) for s in range(8)]
    c0 = counters(ik)
    got = transform_batch(datas, [(160, None)] * 8, [ImageFormat.jpeg] * 8, [85] * 8, FilterType.Triangle)
    assert list(counters(ik) - c0) == [8, 0]
    for i, d in enumerate(datas):
        assert got[i] == transform(d, 160, None, ImageFormat.jpeg, 85, FilterType.Triangle), i


def test_transform_batch_submit_device(ik, monkeypatch):
    monkeypatch.setenv("IK_WEBP_DECODE", "gpu")
    webps = [wt.encode(ikutil.synth(320 + 16 * s, 240, 3, seed=70 + s, pattern="S"), 80) for s in range(2)]
    pngs = [_save(ikutil.synth(300, 200 + 8 * s, 4, seed=80 + s, pattern="S"), "PNG") for s in range(2)]
    datas = [webps[0], pngs[0], pngs[1], webps[1]]
    c0 = counters(ik)
    got = transform_batch_submit_device([DeviceBytes(d) for d in datas], [(128, None)] * 4, [ImageFormat.jpeg] * 4,
                                        [85] * 4, FilterType.Triangle).wait()
    assert list(counters(ik) - c0) == [2, 0]
    for i, d in enumerate(datas):
        assert got[i] == transform(d, 128, None, ImageFormat.jpeg, 85, FilterType.Triangle), i


def test_batch_of_one(ik, monkeypatch):
    d = wt.encode(ikutil.synth(333, 222, 3, seed=90, pattern="N"), 70)
    for mode, want_counts in (("gpu", [1, 0]), ("auto", [0, 1]), ("host", [0, 1])):
        monkeypatch.setenv("IK_WEBP_DECODE", mode)
        c0 = counters(ik)
        (img, fmt), = decode_image_batch([d])
        assert list(counters(ik) - c0) == want_counts, mode
        one, one_fmt = decode_image(d)
        assert list(counters(ik) - c0) == [2 * v for v in want_counts], mode  # (the one-request path counts too)
        assert fmt is one_fmt is ImageFormat.webp
        same(img.to_array(), one.to_array(), mode)
        same(img.to_array(), wt.decode_rgb(d), mode)
