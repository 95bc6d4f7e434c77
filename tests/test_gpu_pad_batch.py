"""GPU: pads through the batch paths.  Every file of every `_opts` form is compared, byte for
byte, with the composition by handles: decode -> resize -> adjust -> blur -> ik_image_pad ->
ik_image_overlay -> ik_encode; the pad, blur and overlay launch counters with the launches that
follow from who shares what; a resize group's members with different canvases, and with pads
that differ only in colour, through its coder groups; a request that is not resized; 16-bit
sources; and a batch whose pads are all IK_PAD_NONE against the 80-byte layout."""
import ctypes
import io
import struct
import zlib

import numpy as np
import pytest
from PIL import Image

import ikutil
from imagekit import (Adjust, DeviceBytes, DynamicImage, ImageFormat, Overlay, Pad, _lib, decode_image, encode_image,
                      resize_image, transform_batch, transform_batch_submit, transform_batch_submit_device)
from imagekit.transform import _inputs, _request_opts, transform

pytestmark = pytest.mark.gpu
J, WP = ImageFormat.jpeg, ImageFormat.webp


def png_of(img):
    b = io.BytesIO()
    Image.fromarray(img, {3: "RGB", 4: "RGBA"}[img.shape[2]]).save(b, format="PNG")
    return b.getvalue()


def jpeg_of(img):
    b = io.BytesIO()
    Image.fromarray(img, "RGB").save(b, format="JPEG", quality=90)
    return b.getvalue()


@pytest.fixture(scope="module")
def sources(ik):
    return dict(p1=png_of(ikutil.synth(96, 64, 4, seed=71, pattern="S", alpha="random")),
                p2=png_of(ikutil.synth(96, 64, 4, seed=72, pattern="S", alpha="random")),
                j1=jpeg_of(ikutil.synth(96, 64, 3, seed=73, pattern="S")),
                j2=jpeg_of(ikutil.synth(96, 64, 3, seed=74, pattern="S")))


@pytest.fixture(scope="module")
def requests_(ik, sources):
    """(data, (w, h), pad, adjust, blur, overlay, fmt, quality) per request.  Contain fits
    96 x 64 into the 48 x 48 box as 48 x 32; Pad() with its zero sizes pads that to the box."""
    s = sources
    mark = DynamicImage.from_array(np.random.default_rng(75).integers(0, 256, (10, 24, 4)).astype(np.uint8))
    white, mirror, top = Pad(color="ffffff"), Pad("mirror"), Pad("edge", "n")
    return [
        (s["p1"], (48, 48), white, None, None, None, J, 85),             # 0, 1: RGBA, one pad
        (s["p2"], (48, 48), Pad(color=0xFFFFFF), None, None, None, J, 85),  #    (an equal Pad: the same 24 bytes)
        (s["p1"], (48, 48), mirror, None, None, None, WP, 80),           # 2, 3: the same canvas, another mode
        (s["p2"], (48, 48), mirror, None, None, None, WP, 80),
        # 4: with 0 and 1, after an adjustment and a blur and before a mark against the canvas's corner
        (s["p1"], (48, 48), white, Adjust(saturation=40), 1.0, Overlay(mark, "se", -2, -2, 200), J, 85),
        (s["j1"], (48, 48), top, None, None, None, WP, 80),              # 5, 6: RGB from JPEG, the image at the top
        (s["j2"], (48, 48), top, None, None, None, WP, 80),
        (s["j1"], (None, None), Pad("wrap", "sw", 120, 80), None, None, None, J, 85),  # 7: not resized: an explicit canvas
        (s["p1"], (48, 48), None, None, None, None, J, 85),              # 8: no pad: 48 x 32
        # 9, 10: only w is given, so the box's missing side is computed as the resize computes it (32): the
        # zero width is 48, and neither it nor a zero height would add anything; the explicit height does
        (s["j1"], (48, None), Pad("edge", "s", 0, 40), None, None, None, J, 85),
        (s["j2"], (48, None), Pad("edge", "s", 0, 40), None, None, None, J, 85),
        # 11: the same box with both sizes zero: the canvas is the image, no pass
        (s["j1"], (48, None), Pad("mirror"), None, None, None, WP, 80),
    ]


# Who shares a launch (csrc/ik_post_stage.cpp; a set of one takes the per-image call, which
# launches and counts as a set of one would):
#   resize   RGBA 96x64 -> 48x32 on a 48x48 canvas at (0, 8): {0, 1, 2, 3, 4}; 8 has the window but
#            not the canvas, so it is alone; RGB 96x64 -> 48x32 at (0, 0) of 48x48: {5, 6}; 7 is
#            not resized; RGB 96x64 -> 48x32 at (0, 8) of 48x40: {9, 10}; 11's canvas is its 48x32
#            image, the only one of that key
#   pad      white {0, 1, 4}, mirror {2, 3}, top {5, 6}, bottom {9, 10}, and 7 image by image: 5
#            launches, 10 images; 11 launches nothing
#   adjust   {4}; blur {4}; mark {4}: one launch, one image each
PAD, ADJUST, BLUR, OVERLAY = (5, 10), (1, 1), (1, 1), (1, 1)
SIZES = [(48, 48)] * 7 + [(120, 80), (48, 32), (48, 40), (48, 40), (48, 32)]


def counters(ik):
    out = []
    for fn in (ik.ik_pad_counters, ik.ik_adjust_counters, ik.ik_blur_counters, ik.ik_overlay_counters,
               ik.ik_flatten_counters):
        c = (ctypes.c_ulonglong * 2)()
        assert fn(c) == 0
        out.append((int(c[0]), int(c[1])))
    return np.array(out, dtype=np.int64)


def chain(data, w, h, pad, adjust, blur, overlay, fmt, q):
    """the request composed by handles; a zero pad size is the side of the box, and where the box
    has no such side, the resized image's own (ik_image_pad's zero), which is what the missing
    side of the target comes to"""
    img, _ = decode_image(data)
    rs = resize_image(img, w, h)
    if adjust is not None:
        rs = rs.adjust(adjust)
    if blur:
        rs = rs.blur(blur)
    if pad is not None:
        s = pad._struct()
        rs = rs.pad(Pad(pad.mode, pad.gravity, s.width or (w or 0), s.height or (h or 0), s.color, s.alpha))
    if overlay is not None:
        rs = rs.overlay(overlay)
    return encode_image(rs, fmt, q)


@pytest.fixture(scope="module")
def want(ik, requests_):
    return [chain(data, w, h, *rest) for data, (w, h), *rest in requests_]


def batch_args(reqs):
    args = ([r[0] for r in reqs], [r[1] for r in reqs], [r[6] for r in reqs], [r[7] for r in reqs])
    kw = dict(pads=[r[2] for r in reqs], adjusts=[r[3] for r in reqs], blurs=[r[4] for r in reqs],
              overlays=[r[5] for r in reqs])
    return args, kw


def test_the_chain_gives_canvases(ik, requests_, want):
    for out, size in zip(want, SIZES):
        assert decode_image(out)[0].dimensions() == size
    assert len(set(want)) == len(want)


def test_transform_alone(ik, requests_, want):
    c0 = counters(ik)
    for (data, (w, h), pad, adjust, blur, overlay, fmt, q), w_ in zip(requests_, want):
        assert transform(data, w, h, fmt, q, pad=pad, adjust=adjust, blur=blur, overlay=overlay) == w_
    # every request that pads costs a launch of its own here
    assert np.array_equal(counters(ik) - c0, ((10, 10), ADJUST, BLUR, OVERLAY, (0, 0)))


def test_transform_batch(ik, requests_, want):
    args, kw = batch_args(requests_)
    c0 = counters(ik)
    outs = transform_batch(*args, **kw)
    delta = counters(ik) - c0
    print("pad, adjust, blur, overlay, flatten (launches, images):", delta.tolist())
    assert outs == want, [i for i in range(len(want)) if outs[i] != want[i]]
    assert np.array_equal(delta, (PAD, ADJUST, BLUR, OVERLAY, (0, 0))), delta.tolist()
    for out, size in zip(outs, SIZES):
        assert decode_image(out)[0].dimensions() == size


def test_transform_batch_submit(ik, requests_, want):
    args, kw = batch_args(requests_)
    c0 = counters(ik)
    assert transform_batch_submit(*args, **kw).wait() == want
    assert np.array_equal(counters(ik) - c0, (PAD, ADJUST, BLUR, OVERLAY, (0, 0)))


def test_transform_batch_submit_device(ik, requests_, want):
    args, kw = batch_args(requests_)
    assert ik.ik_set_png_gpu_min(0) == 0
    try:
        dev = [DeviceBytes(d) for d in args[0]]
        c0 = counters(ik)
        assert transform_batch_submit_device(dev, *args[1:], **kw).wait() == want
        assert np.array_equal(counters(ik) - c0, (PAD, ADJUST, BLUR, OVERLAY, (0, 0)))
    finally:
        ik.ik_set_png_gpu_min(256 << 10)


def raw_batch(ik, datas, sizes, fmts, qs, ra, size):
    n = len(datas)
    keep, ptrs, lens = _inputs(datas)
    ws = (ctypes.c_int64 * n)(*[-1 if s[0] is None else s[0] for s in sizes])
    hs = (ctypes.c_int64 * n)(*[-1 if s[1] is None else s[1] for s in sizes])
    fs = (ctypes.c_int * n)(*[int(f.value) for f in fmts])
    qa = (ctypes.c_int * n)(*qs)
    outs, olens, status = (ctypes.c_void_p * n)(), (ctypes.c_size_t * n)(), (ctypes.c_int * n)()
    rc = ik.ik_transform_batch_opts(ptrs, lens, n, ws, hs, ra, size, fs, qa, 4, 0, outs, olens, status)
    res = []
    for i in range(n):
        res.append(ctypes.string_at(outs[i], olens[i]) if outs[i] else None)
        if outs[i]:
            ik.ik_buf_free(outs[i])
    return rc, res, list(status)


def test_one_quality_different_canvases_and_colours(ik, sources):
    """Six JPEG requests of one source geometry, one window and one quality.  Before the pad they
    were one resize group and one coder group; now {0, 1} (64 x 48), {2, 3} (48 x 64) and {4, 5}
    (48 x 48) are three, each with a JPEG coder group whose images agree.  4 and 5 differ only
    in colour: one resize group, one coder group, two pad launches.  Pads: {0, 1}, {2, 3}, {4},
    {5}: 4 launches, 6 images."""
    j1, j2 = sources["j1"], sources["j2"]
    wide, tall = Pad(width=64, height=48, color="ffffff"), Pad(width=48, height=64, color="ffffff")
    reqs = [(j1, (48, 48), wide), (j2, (48, 48), wide), (j1, (48, 48), tall), (j2, (48, 48), tall),
            (j1, (48, 48), Pad(color="ff0000")), (j2, (48, 48), Pad(color="0000ff"))]
    datas, sizes, pads = [r[0] for r in reqs], [r[1] for r in reqs], [r[2] for r in reqs]
    expect = [chain(d, w, h, p, None, None, None, J, 85) for d, (w, h), p in reqs]
    c0 = counters(ik)
    ra = _request_opts(6, pads=pads)
    assert ctypes.sizeof(ra._type_) == 104
    rc, outs, status = raw_batch(ik, datas, sizes, [J] * 6, [85] * 6, ra, 104)
    assert rc == 0 and status == [0] * 6, (_lib.last_error(), status)
    assert np.array_equal((counters(ik) - c0)[0], (4, 6))
    assert outs == expect, [i for i in range(6) if outs[i] != expect[i]]
    assert [decode_image(o)[0].dimensions() for o in outs] == [(64, 48)] * 2 + [(48, 64)] * 2 + [(48, 48)] * 2
    assert outs[4] != outs[5]
    # the same through WebP coder groups
    expect = [chain(d, w, h, p, None, None, None, WP, 80) for d, (w, h), p in reqs]
    rc, outs, status = raw_batch(ik, datas, sizes, [WP] * 6, [80] * 6, ra, 104)
    assert rc == 0 and status == [0] * 6 and outs == expect


def png16_of(px):
    """a 16-bit RGB PNG by hand: Pillow cannot write one"""
    h, w, _ = px.shape
    raw = b"".join(b"\0" + px[y].astype(">u2").tobytes() for y in range(h))

    def chunk(t, d):
        return struct.pack(">I", len(d)) + t + d + struct.pack(">I", zlib.crc32(t + d))
    return (b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 16, 2, 0, 0, 0))
            + chunk(b"IDAT", zlib.compress(raw)) + chunk(b"IEND", b""))


def test_sixteen_bit_sources(ik):
    """16-bit images are never grouped: each is padded on the image-by-image tail"""
    datas = []
    for seed in (81, 82):
        px = np.random.default_rng(seed).integers(0, 65536, (40, 60, 3)).astype(np.uint16)
        datas.append(png16_of(px))
        img = decode_image(datas[-1])[0]
        assert img.depth == 2 and np.array_equal(img.to_array(), px)
    pad = Pad("mirror", "e")
    expect = [chain(d, 30, 30, pad, None, None, None, J, 85) for d in datas]
    c0 = counters(ik)
    assert transform_batch(datas, [(30, 30)] * 2, [J] * 2, [85] * 2, pads=pad) == expect
    assert np.array_equal((counters(ik) - c0)[0], (2, 2))
    assert decode_image(expect[0])[0].dimensions() == (30, 30)


def test_pads_all_none_are_the_80_byte_layout(ik, requests_, want):
    """the mixed batch with every pad IK_PAD_NONE, at 104 bytes: the files and every post counter
    of the same batch at 80 bytes"""
    args, kw = batch_args(requests_)
    datas, sizes, fmts, qs = args
    kw = dict(kw, pads=None)
    ra4 = _request_opts(len(datas), **kw)
    assert ctypes.sizeof(ra4._type_) == 80
    c0 = counters(ik)
    rc4, outs4, status4 = raw_batch(ik, datas, sizes, fmts, qs, ra4, 80)
    d4 = counters(ik) - c0
    ra5 = (_lib.RequestOpts5 * len(datas))()
    for a, b in zip(ra5, ra4):
        ctypes.memmove(ctypes.byref(a), ctypes.byref(b), 80)
    c0 = counters(ik)
    rc5, outs5, status5 = raw_batch(ik, datas, sizes, fmts, qs, ra5, 104)
    d5 = counters(ik) - c0
    assert rc4 == 0 and rc5 == 0 and status4 == status5 == [0] * len(datas)
    assert outs5 == outs4 and outs4[8] == want[8] and outs4[0] != want[0]
    assert np.array_equal(d4, d5) and np.array_equal(d5, ((0, 0), ADJUST, BLUR, OVERLAY, (0, 0))), (d4.tolist(), d5.tolist())
