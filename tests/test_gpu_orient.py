"""GPU: EXIF orientation.  The orient kernels are exact permutations, so everything here
is compared with zero tolerance: ik_orient_batch_device against numpy (the header's
table) for every orientation, pixel size and tile edge, on both the dword and the byte
path, with poisoned padding; its refusals; ik_image_orient against Pillow's
Image.transpose; ik_decode_oriented against ImageOps.exif_transpose; ik_transform_oriented
against the by-hand chain; and a mixed batch against each request alone."""
import ctypes
import io

import numpy as np
import pytest
from PIL import Image, ImageOps

import exif_util as xu
import ikutil
from imagekit import (DynamicImage, FitMode, ImageFormat, Orientation, _lib, decode_image, encode_image,
                      resize_image, transform_batch)
from imagekit.transform import _inputs, transform

pytestmark = pytest.mark.gpu
POISON = 0xA5
IK_ERR_INVALID = 2
AREA = 1 << 20  # bytes of each of the two device areas the kernel tests share


@pytest.fixture(scope="module")
def areas(ik):
    d_src, d_dst = ctypes.c_void_p(), ctypes.c_void_p()
    assert ik.ik_dev_alloc(AREA, ctypes.byref(d_src)) == 0
    assert ik.ik_dev_alloc(AREA, ctypes.byref(d_dst)) == 0
    yield d_src.value, d_dst.value
    ik.ik_dev_free(d_src)
    ik.ik_dev_free(d_dst)


def ramp(n, H, W, px):
    """Bytes that differ between neighbours in every direction and inside a pixel: a
    multiplicative hash of the flat byte index (256 values cannot be unique over a tile,
    but no two bytes a wrong permutation could exchange within a few pixels agree)."""
    i = np.arange(n * H * W * px, dtype=np.uint64)
    with np.errstate(over="ignore"):
        v = (i * np.uint64(0x9E3779B97F4A7C15)) >> np.uint64(56)
    return v.astype(np.uint8).reshape(n, H, W, px)


def run_orient(ik, areas, imgs, C, depth, o, src_pitch=None, dst_pitch=None, src_gap=0, dst_gap=0, src_off=0,
               dst_off=0, expect=0):
    """imgs (n, H, W, px) uint8 through ik_orient_batch_device.  Returns the (n, oh, ow, px)
    bytes after checking that no byte of the destination area outside them changed."""
    d_src, d_dst = areas
    n, H, W, px = imgs.shape
    assert px == C * depth
    ow, oh = (H, W) if o >= 5 else (W, H)
    src_pitch = src_pitch or W * px
    dst_pitch = dst_pitch or ow * px
    sstride, dstride = src_pitch * H + src_gap, dst_pitch * oh + dst_gap
    src = np.full(src_off + n * sstride, 0x3C, np.uint8)
    for i in range(n):
        src[src_off + i * sstride:src_off + i * sstride + src_pitch * H].reshape(H, src_pitch)[:, :W * px] = \
            imgs[i].reshape(H, W * px)
    dst = np.full(dst_off + n * dstride + 64, POISON, np.uint8)
    assert src.nbytes <= AREA and dst.nbytes <= AREA
    assert ik.ik_memcpy_h2d(d_src, src.ctypes.data, src.nbytes) == 0
    assert ik.ik_memcpy_h2d(d_dst, dst.ctypes.data, dst.nbytes) == 0
    rc = ik.ik_orient_batch_device(d_src + src_off, W, H, C, depth, src_pitch, sstride, n, o, d_dst + dst_off,
                                   dst_pitch, dstride, None)
    assert rc == expect, _lib.last_error()
    assert ik.ik_dev_synchronize() == 0
    assert ik.ik_memcpy_d2h(dst.ctypes.data, d_dst, dst.nbytes) == 0
    if expect:
        assert (dst == POISON).all(), "a refused call wrote to the destination"
        return None
    out = np.zeros((n, oh, ow, px), np.uint8)
    keep = np.ones(dst.size, bool)
    for i in range(n):
        lo = dst_off + i * dstride
        out[i] = dst[lo:lo + dst_pitch * oh].reshape(oh, dst_pitch)[:, :ow * px].reshape(oh, ow, px)
        keep[lo:lo + dst_pitch * oh].reshape(oh, dst_pitch)[:, :ow * px] = False
    assert (dst[keep] == POISON).all(), "a store outside the out_w x out_h pixels"
    return out


def sizes(ik):
    T, S = ik.ik_orient_tile(), ik.ik_orient_strip()
    assert T >= 2 and S >= 2
    # (W, H): the issue's six around the tile edge, and the row kernel's strip edge
    return [(1, 1), (1, T + 1), (T + 1, 1), (T - 1, T + 1), (T, T), (2 * T + 3, T + 2), (S + 1, 2), (2 * S - 1, 5)]


PIXELS = [(c, d) for d in (1, 2) for c in (1, 2, 3, 4)]


@pytest.mark.parametrize("C,depth", PIXELS, ids=lambda v: str(v))
def test_kernel_equals_numpy(ik, areas, C, depth):
    """Every orientation and size, rows packed (for odd sizes: the byte path), rows padded to
    a multiple of 4 (the dword path) and rows padded to an odd pitch from an odd base."""
    px = C * depth
    for W, H in sizes(ik):
        img = ramp(1, H, W, px)
        for o in range(1, 9):
            want = xu.orient_np(img[0], o)
            ow = H if o >= 5 else W
            for sp, dp, so, do in ((None, None, 0, 0),
                                   ((W * px + 3) // 4 * 4 + 4, (ow * px + 3) // 4 * 4 + 8, 0, 0),
                                   (W * px + 5 - (W * px) % 2, ow * px + 3 - (ow * px) % 2, 1, 3)):
                got = run_orient(ik, areas, img, C, depth, o, sp, dp, 0, 0, so, do)
                assert np.array_equal(got[0], want), (W, H, o, sp, dp)


@pytest.mark.parametrize("C,depth", [(3, 1), (4, 1), (3, 2), (1, 1)], ids=lambda v: str(v))
def test_batch_of_three_with_gaps(ik, areas, C, depth):
    T = ik.ik_orient_tile()
    px = C * depth
    W, H = T + 5, T - 3
    imgs = ramp(3, H, W, px)
    for o in range(1, 9):
        ow = H if o >= 5 else W
        for sp, dp, sg, dg in (((W * px + 3) // 4 * 4 + 12, (ow * px + 3) // 4 * 4 + 4, 40, 100),
                               (W * px + 7, ow * px + 1, 33, 77)):
            got = run_orient(ik, areas, imgs, C, depth, o, sp, dp, sg, dg)
            for i in range(3):
                assert np.array_equal(got[i], xu.orient_np(imgs[i], o)), (o, i, sp, dp)


def test_refusals_leave_the_destination_alone(ik, areas):
    d_src, d_dst = areas
    bad = IK_ERR_INVALID
    # orientation outside 1..8 (transposed sizes are moot: nothing may be written at all)
    for o in (0, 9, -1, 100):
        dst = np.full(4096, POISON, np.uint8)
        assert ik.ik_memcpy_h2d(d_dst, dst.ctypes.data, dst.nbytes) == 0
        assert ik.ik_orient_batch_device(d_src, 10, 6, 3, 1, 30, 180, 2, o, d_dst, 30, 180, None) == bad
        assert ik.ik_dev_synchronize() == 0
        assert ik.ik_memcpy_d2h(dst.ctypes.data, d_dst, dst.nbytes) == 0
        assert (dst == POISON).all()

    def refused(*args):
        dst = np.full(8192, POISON, np.uint8)
        assert ik.ik_memcpy_h2d(d_dst, dst.ctypes.data, dst.nbytes) == 0
        assert ik.ik_orient_batch_device(*args) == bad, args
        assert ik.ik_dev_synchronize() == 0
        assert ik.ik_memcpy_d2h(dst.ctypes.data, d_dst, dst.nbytes) == 0
        assert (dst == POISON).all(), args

    for o in (1, 2, 6):
        ow, oh = (6, 10) if o >= 5 else (10, 6)
        ok = [d_src, 10, 6, 3, 1, 32, 32 * 6, 2, o, d_dst, ow * 3 + 2, (ow * 3 + 2) * oh, None]
        assert ik.ik_orient_batch_device(*ok) == 0
        assert ik.ik_dev_synchronize() == 0

        def but(**kw):
            names = ["src", "W", "H", "C", "depth", "sp", "ss", "n", "o", "dst", "dp", "ds", "stream"]
            a = list(ok)
            for k, v in kw.items():
                a[names.index(k)] = v
            return a

        refused(*but(src=None))
        refused(*but(dst=None))
        refused(*but(W=0))
        refused(*but(H=0))
        refused(*but(n=0))
        refused(*but(C=0))
        refused(*but(C=5))
        refused(*but(depth=0))
        refused(*but(depth=3))
        refused(*but(sp=29))              # below W * 3
        refused(*but(dp=ow * 3 - 1))
        refused(*but(depth=2, sp=59))     # below W * 6
        refused(*but(ss=32 * 6 - 1))      # n > 1: below rows * pitch
        refused(*but(ds=(ow * 3 + 2) * oh - 1))
        refused(*but(n=65536, ss=32 * 6, ds=(ow * 3 + 2) * oh))
    # one image: the strides are not looked at
    assert ik.ik_orient_batch_device(d_src, 10, 6, 3, 1, 32, 0, 1, 6, d_dst, 20, 0, None) == 0
    assert ik.ik_dev_synchronize() == 0


# ---- image handles ------------------------------------------------------------------------
def test_image_orient_equals_pillow_transpose(ik):
    rgb = ikutil.synth(37, 21, 3, seed=5, pattern="N")
    img = DynamicImage.from_array(rgb)
    pil = Image.fromarray(rgb, "RGB")
    for o, op in xu.PIL_OP.items():
        got = img.apply_orientation(o)
        assert got.dimensions() == ((21, 37) if o >= 5 else (37, 21)) and got.depth == 1
        np.testing.assert_array_equal(got.to_array(), np.asarray(pil.transpose(op)))
    np.testing.assert_array_equal(img.apply_orientation(1).to_array(), rgb)
    np.testing.assert_array_equal(img.apply_orientation(Orientation.rotate90).to_array(), np.rot90(rgb, -1))

    wide = (ramp(1, 70, 9, 8)[0].view(np.uint16)).reshape(70, 9, 4)
    img16 = DynamicImage.from_array(wide)
    for o, op in xu.PIL_OP.items():
        got = img16.apply_orientation(o)
        assert got.depth == 2 and got.color() == "Rgba16"
        want = np.stack([np.asarray(Image.fromarray(np.ascontiguousarray(wide[:, :, k])).transpose(op))
                         for k in range(4)], -1)
        np.testing.assert_array_equal(got.to_array(), want)
    out = ctypes.c_void_p()
    for o in (0, 9, -1):
        assert ik.ik_image_orient(img._h, o, ctypes.byref(out)) == IK_ERR_INVALID
    assert ik.ik_image_orient(None, 3, ctypes.byref(out)) == IK_ERR_INVALID


@pytest.fixture(scope="module")
def photo():
    return Image.fromarray(ikutil.synth(41, 23, 3, seed=9, pattern="S"), "RGB")


@pytest.mark.parametrize("fmt", ["PNG", "WEBP"])
def test_decode_auto_equals_exif_transpose(ik, photo, fmt):
    for o in range(1, 9):
        data = xu.pillow_file(fmt, o, photo)
        got, _ = decode_image(data, orient=Orientation.auto)
        want = np.asarray(ImageOps.exif_transpose(Image.open(io.BytesIO(data))).convert("RGB"))
        np.testing.assert_array_equal(got.to_array(), want)
        stored, _ = decode_image(data, orient=Orientation.stored)
        plain, _ = decode_image(data)
        np.testing.assert_array_equal(stored.to_array(), plain.to_array())
        np.testing.assert_array_equal(plain.to_array(), np.asarray(photo))


def test_decode_auto_jpeg_and_forced_values(ik, photo):
    for o in range(1, 9):
        data = xu.pillow_file("JPEG", o, photo)
        plain, f = decode_image(data)
        got, f2 = decode_image(data, orient=Orientation.auto)
        assert f is ImageFormat.jpeg and f2 is ImageFormat.jpeg
        np.testing.assert_array_equal(got.to_array(), xu.orient_np(plain.to_array(), o))
        # a forced value wins over the file's
        forced, _ = decode_image(data, orient=8)
        np.testing.assert_array_equal(forced.to_array(), xu.orient_np(plain.to_array(), 8))
    out, fmt = ctypes.c_void_p(), ctypes.c_int()
    data = xu.pillow_file("PNG", 6, photo)
    for bad in (-2, 9, 100):
        assert ik.ik_decode_oriented(data, len(data), bad, ctypes.byref(out), ctypes.byref(fmt)) == IK_ERR_INVALID


# ---- transforms ---------------------------------------------------------------------------
@pytest.mark.parametrize("out_fmt", [ImageFormat.jpeg, ImageFormat.webp])
def test_transform_oriented_equals_the_chain(ik, photo, out_fmt):
    for src_fmt, o in (("PNG", 6), ("JPEG", 5), ("WEBP", 3), ("PNG", 1), ("JPEG", None)):
        data = xu.pillow_file(src_fmt, o, photo)
        got = transform(data, 16, 12, out_fmt, 80, fit=FitMode.cover, orient=Orientation.auto)
        img, _ = decode_image(data)
        if o not in (None, 1):
            img = img.apply_orientation(o)
        want = encode_image(resize_image(img, 16, 12, fit=FitMode.cover), out_fmt, 80)
        assert got == want, (src_fmt, o)
        if o in (None, 1):  # no pass: the _fit call's bytes
            assert got == transform(data, 16, 12, out_fmt, 80, fit=FitMode.cover)
    # stored is the call without the argument, whatever the file says
    data = xu.pillow_file("PNG", 6, photo)
    assert transform(data, 16, 12, out_fmt, 80, orient=Orientation.stored) == transform(data, 16, 12, out_fmt, 80)
    buf, n = _lib.u8p(), ctypes.c_size_t()
    assert ik.ik_transform_oriented(data, len(data), 16, 12, 0, 9, int(out_fmt.value), 80, 4, ctypes.byref(buf),
                                    ctypes.byref(n)) == IK_ERR_INVALID


def test_batch_mixed_orientations(ik, photo):
    A = xu.pillow_file("PNG", 6, photo)
    B = xu.pillow_file("JPEG", 3, photo)
    Cw = xu.pillow_file("WEBP", 8, photo)
    D = xu.pillow_file("PNG", None, photo)
    AUTO, STORED = Orientation.auto, Orientation.stored
    J, Wf = ImageFormat.jpeg, ImageFormat.webp
    cover, contain, exact = FitMode.cover, FitMode.contain, FitMode.exact
    reqs = [  # data, (w, h), fit, orient, fmt
        (A, (16, 16), cover, AUTO, J), (A, (16, 16), cover, AUTO, J), (A, (16, 16), cover, AUTO, J),
        (D, (20, None), contain, 8, Wf), (D, (20, None), contain, 8, Wf), (D, (20, None), contain, 8, Wf),
        (B, (10, 10), exact, AUTO, J),
        (B, (12, 12), contain, STORED, Wf),
        (Cw, (9, 14), cover, AUTO, J),
        (A, (30, 30), contain, 3, Wf),
        (D, (11, 7), exact, STORED, J),
        (Cw, (8, 8), exact, 6, Wf),
    ]
    datas = [r[0] for r in reqs]
    szs = [r[1] for r in reqs]
    fits = [r[2] for r in reqs]
    orients = [r[3] for r in reqs]
    fmts = [r[4] for r in reqs]
    qs = [80] * len(reqs)
    got = transform_batch(datas, szs, fmts, qs, fits=fits, orient=orients)
    for i, r in enumerate(reqs):
        alone = transform(r[0], r[1][0], r[1][1], r[4], 80, fit=r[2], orient=r[3])
        assert got[i] == alone, i
    # the turned requests differ from their stored-order selves (the test would pass on a no-op otherwise)
    assert got[0] != transform(A, 16, 16, J, 80, fit=cover)
    # orient = NULL, and all STORED, are the _fit call
    n = len(reqs)
    keep, ptrs, lens = _inputs(datas)
    ws = (ctypes.c_int64 * n)(*[s[0] for s in szs])
    hs = (ctypes.c_int64 * n)(*[-1 if s[1] is None else s[1] for s in szs])
    fa = (ctypes.c_int * n)(*[int(f) for f in fits])
    fs = (ctypes.c_int * n)(*[int(f.value) for f in fmts])
    qa = (ctypes.c_int * n)(*qs)
    want = transform_batch(datas, szs, fmts, qs, fits=fits)
    for oa in (None, (ctypes.c_int * n)(*[0] * n)):
        outs, olens, status = (ctypes.c_void_p * n)(), (ctypes.c_size_t * n)(), (ctypes.c_int * n)()
        assert ik.ik_transform_batch_oriented(ptrs, lens, n, ws, hs, fa, oa, fs, qa, 4, 0, outs, olens, status) == 0
        for i in range(n):
            assert ctypes.string_at(outs[i], olens[i]) == want[i], i
            ik.ik_buf_free(outs[i])
    bad = (ctypes.c_int * n)(*([0] * (n - 1) + [9]))
    outs, olens, status = (ctypes.c_void_p * n)(), (ctypes.c_size_t * n)(), (ctypes.c_int * n)()
    assert ik.ik_transform_batch_oriented(ptrs, lens, n, ws, hs, fa, bad, fs, qa, 4, 0, outs, olens,
                                          status) == IK_ERR_INVALID
