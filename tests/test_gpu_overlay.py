"""GPU: the watermark overlay.  Everything is compared with zero tolerance: k_overlay against
tests/overlay_model.py for every base and overlay format, the window's ragged edges on the
wide and the byte path with a canary around every row, tiling, every 8-bit (f, a, c) triple,
a batch with gaps; ik_image_overlay; ik_transform_opts against the by-hand chain; a mixed
batch against each request alone, with the launch counters; the device-resident submit;
and the 56-byte layout at its defaults against the 24-byte one."""
import ctypes
import io

import numpy as np
import pytest
from PIL import Image

import ikutil
import overlay_model as om
from imagekit import (DeviceBytes, DynamicImage, FitMode, Gravity, ImageFormat, Overlay, TransformError, _lib,
                      decode_image, encode_image, resize_image, transform_batch, transform_batch_submit,
                      transform_batch_submit_device)
from imagekit.transform import _inputs, transform

pytestmark = pytest.mark.gpu
CANARY = 0xA5
IK_ERR_INVALID = 2
BASE_AREA, OV_AREA = 17 << 20, 5 << 20
J, WP = ImageFormat.jpeg, ImageFormat.webp
FORMATS = [(C, d) for d in (1, 2) for C in (1, 2, 3, 4)]


@pytest.fixture(scope="module")
def areas(ik):
    d_base, d_ov = ctypes.c_void_p(), ctypes.c_void_p()
    assert ik.ik_dev_alloc(BASE_AREA, ctypes.byref(d_base)) == 0
    assert ik.ik_dev_alloc(OV_AREA, ctypes.byref(d_ov)) == 0
    yield d_base.value, d_ov.value
    ik.ik_dev_free(d_base)
    ik.ik_dev_free(d_ov)


def counters(ik):
    c = (ctypes.c_ulonglong * 2)()
    assert ik.ik_overlay_counters(c) == 0
    return np.array([c[0], c[1]], dtype=np.int64)


def noise(H, W, C, depth, seed):
    """random samples; where there is an alpha channel, plenty of alpha 0 and alpha M"""
    r = np.random.default_rng(seed).integers(0, 256 ** depth, (H, W, C))
    if C in (2, 4):
        r[..., C - 1][r[..., C - 1] % 5 == 0] = 0
        r[..., C - 1][r[..., C - 1] % 5 == 1] = 256 ** depth - 1
    return r.astype(np.uint8 if depth == 1 else np.uint16)


def row_bytes(img):
    return np.ascontiguousarray(img).view(np.uint8).reshape(img.shape[0], -1)


def run_overlay(ik, areas, bases, O, g=om.CENTER, dx=0, dy=0, op=255, tile=False, pitch=None, gap=0, off=0,
                ov_pitch=None, ov_off=0, expect=0):
    """bases (n, H, W, C) under O through ik_overlay_batch_device, in place.  Returns the n
    images after checking that no byte of the base area outside the W * C * depth bytes of
    each row changed (pitch padding, before, after and between the images) and that the
    overlay's area did not change at all."""
    d_base, d_ov = areas
    n, H, W, C = bases.shape
    depth = bases.dtype.itemsize
    row = W * C * depth
    pitch = pitch or row
    stride = pitch * H + gap
    buf = np.full(off + n * stride + 64, CANARY, np.uint8)
    for i in range(n):
        buf[off + i * stride:off + i * stride + pitch * H].reshape(H, pitch)[:, :row] = row_bytes(bases[i])
    ho, wo, co = O.shape
    orow = wo * co * O.dtype.itemsize
    ov_pitch = ov_pitch or orow
    ob = np.full(ov_off + ov_pitch * ho + 64, 0x5A, np.uint8)
    ob[ov_off:ov_off + ov_pitch * ho].reshape(ho, ov_pitch)[:, :orow] = row_bytes(O)
    assert buf.nbytes <= BASE_AREA and ob.nbytes <= OV_AREA
    assert ik.ik_memcpy_h2d(d_base, buf.ctypes.data, buf.nbytes) == 0
    assert ik.ik_memcpy_h2d(d_ov, ob.ctypes.data, ob.nbytes) == 0
    rc = ik.ik_overlay_batch_device(d_base + off, W, H, C, depth, pitch, stride, n, d_ov + ov_off, wo, ho, co,
                                    O.dtype.itemsize, ov_pitch, g, dx, dy, op, int(tile), None)
    assert rc == expect, _lib.last_error()
    assert ik.ik_dev_synchronize() == 0
    got, ob2 = np.empty_like(buf), np.empty_like(ob)
    assert ik.ik_memcpy_d2h(got.ctypes.data, d_base, got.nbytes) == 0
    assert ik.ik_memcpy_d2h(ob2.ctypes.data, d_ov, ob2.nbytes) == 0
    assert np.array_equal(ob2, ob), "the overlay was written"
    if expect:
        assert np.array_equal(got, buf), "a refused call wrote to the base"
        return None
    out = np.zeros((n, H, row), np.uint8)
    keep = np.ones(got.size, bool)
    for i in range(n):
        lo = off + i * stride
        out[i] = got[lo:lo + pitch * H].reshape(H, pitch)[:, :row]
        keep[lo:lo + pitch * H].reshape(H, pitch)[:, :row] = False
    assert (got[keep] == CANARY).all(), "a store outside the W * C * depth bytes of a row"
    return out.view(bases.dtype).reshape(n, H, W, C)


def check(ik, areas, B, O, g=om.CENTER, dx=0, dy=0, op=255, tile=False, **kw):
    got = run_overlay(ik, areas, B[None], O, g, dx, dy, op, tile, **kw)[0]
    want = om.overlay(B, O, g, dx, dy, op, tile)
    assert np.array_equal(got, want), (B.shape, B.dtype, O.shape, O.dtype, g, dx, dy, op, tile, kw,
                                       np.argwhere(got != want)[:4].tolist())


@pytest.mark.parametrize("C,depth", FORMATS, ids=lambda v: str(v))
def test_kernel_equals_model(ik, areas, C, depth):
    """every overlay format under this base format: 8 x 8 = 64 cases over the parametrisation"""
    S = ik.ik_overlay_span()
    B = noise(9, S + 3, C, depth, seed=100 + C * 2 + depth)
    for co, od in FORMATS:
        O = noise(3, 5, co, od, seed=co * 2 + od)
        for op in (1, 128, 255):
            check(ik, areas, B, O, om.NW, -2, 1, op, tile=True)
        check(ik, areas, B, O, om.SE, -1, -2, 255)
        check(ik, areas, B, O, om.CENTER, 0, 0, 128, pitch=(B.shape[1] * C * depth + 3) // 4 * 4 + 4)


@pytest.mark.parametrize("C,depth", [(3, 1), (1, 1), (4, 1), (3, 2), (2, 2)], ids=lambda v: str(v))
def test_window_edges_on_both_paths(ik, areas, C, depth):
    S = ik.ik_overlay_span()
    W, H = 2 * S + 40, 5
    B = noise(H, W, C, depth, seed=7)
    row = W * C * depth
    layouts = [dict(pitch=(row + 3) // 4 * 4 + 8, off=4),                       # the wide path, poisoned padding
               dict(pitch=row + 3 - row % 2, off=1, ov_pitch=None, ov_off=1)]   # bytes: base + 1, an odd pitch
    for ww in (1, 3, S - 1, S, S + 1):
        O = noise(3, ww, 4, 1, seed=ww)
        for x0 in range(8):
            for lay in layouts if x0 in (0, 1, 3) else layouts[:1]:
                check(ik, areas, B, O, om.NW, x0, 1, 200, **lay)
        # a window that ends at the base's last column
        for lay in layouts:
            check(ik, areas, B, O, om.NE, 0, 2, 255, **lay)
            check(ik, areas, B, O, om.SE, 0, 0, 77, **lay)


@pytest.mark.parametrize("C,depth", [(3, 1), (1, 1), (4, 2)], ids=lambda v: str(v))
def test_clipped_larger_and_empty(ik, areas, C, depth):
    B = noise(11, 37, C, depth, seed=3)
    O = noise(6, 9, 4, 1, seed=4)
    for g, dx, dy in ((om.NW, -4, 0), (om.NE, 5, 0), (om.N, 0, -3), (om.S, 0, 4), (om.CENTER, -20, 2), (om.SE, 8, 5)):
        assert 0 < om.place(37, 11, 9, 6, g, dx, dy)[2] * om.place(37, 11, 9, 6, g, dx, dy)[3] < 54
        check(ik, areas, B, O, g, dx, dy, 255, pitch=37 * C * depth + 3)
    big = noise(29, 80, 2, 2, seed=5)  # larger than the base on both axes
    for g in om.GRAVITIES:
        check(ik, areas, B, big, g, 0, 0, 180)
    check(ik, areas, B, noise(29, 5, 3, 1, seed=6), om.CENTER, 0, 0, 255)  # taller only
    check(ik, areas, B, noise(2, 80, 3, 1, seed=6), om.CENTER, 0, 0, 255)  # wider only
    c0 = counters(ik)
    for g, dx, dy in ((om.NW, -9, 0), (om.NW, 37, 0), (om.NW, 0, -6), (om.NW, 0, 11), (om.SE, 1 << 24, 0)):
        assert om.place(37, 11, 9, 6, g, dx, dy)[:4] == (0, 0, 0, 0)
        check(ik, areas, B, O, g, dx, dy, 255)
    assert np.array_equal(counters(ik), c0), "an empty window launched"
    check(ik, areas, B, O, om.NW, 0, 0, 255)
    assert np.array_equal(counters(ik) - c0, (1, 1))


def test_tile(ik, areas):
    for C, depth in FORMATS:
        B = noise(21, 67, C, depth, seed=C + depth)
        for co, od in ((4, 1), (2, 2), (3, 1)):
            check(ik, areas, B, noise(3, 5, co, od, seed=9), om.NW, -2, 1, 255, tile=True)
            check(ik, areas, B, noise(3, 5, co, od, seed=9), om.NW, -2, 1, 99, tile=True, pitch=67 * C * depth + 5, off=3)
    check(ik, areas, noise(21, 67, 3, 1, seed=1), noise(40, 100, 4, 1, seed=2), om.CENTER, 3, -50, 255, tile=True)


def test_every_8bit_triple_on_an_opaque_base(ik, areas):
    """(f, a, c) for all 2^24 triples at opacity 255 in one launch: a 4096 x 4096 Luma8 base
    whose 256 x 256 blocks each hold one c, under a tiled 256 x 256 LumaA overlay that holds
    f in x and a in y."""
    y, x = np.mgrid[0:4096, 0:4096]
    B = ((x // 256) * 16 + y // 256).astype(np.uint8)[..., None]
    oy, ox = np.mgrid[0:256, 0:256]
    O = np.stack([ox, oy], axis=2).astype(np.uint8)
    got = run_overlay(ik, areas, B[None], O, om.NW, 0, 0, 255, True)[0]
    seen = np.zeros(256, bool)
    for k in range(16):  # the model strip by strip (a strip starts at a multiple of the overlay's height)
        want = om.overlay(B[256 * k:256 * (k + 1)], O, om.NW, 0, 0, 255, True)
        assert np.array_equal(got[256 * k:256 * (k + 1)], want), k
        seen[np.unique(B[256 * k:256 * (k + 1)])] = True
    assert seen.all()


def test_a_million_quadruples_on_an_rgba_base(ik, areas):
    """2^20 random (f, a, c, ca) per channel plus the corners, RGBA8 under RGBA8"""
    B = noise(1024, 1024, 4, 1, seed=11)
    O = noise(1024, 1024, 4, 1, seed=12)
    k = 0
    for f in (0, 255):
        for a in (0, 1, 254, 255):
            for c in (0, 255):
                for ca in (0, 1, 254, 255):
                    O[0, k], B[0, k] = (f, f, 255 - f, a), (c, 255 - c, c, ca)
                    k += 1
    for op in (255, 254, 1):
        check(ik, areas, B, O, om.NW, 0, 0, op)


@pytest.mark.parametrize("C,depth", [(3, 1), (4, 1), (1, 2), (4, 2)], ids=lambda v: str(v))
def test_batch_of_three_with_gaps(ik, areas, C, depth):
    S = ik.ik_overlay_span()
    W, H = S + 7, 6
    bases = np.stack([noise(H, W, C, depth, seed=70 + i) for i in range(3)])
    O = noise(4, 33, 4, 1, seed=8)
    row = W * C * depth
    c0 = counters(ik)
    for pitch, gap, tile in (((row + 3) // 4 * 4 + 12, 100, False), (row + 7 - row % 2, 33, False),
                             ((row + 3) // 4 * 4, 40, True)):
        got = run_overlay(ik, areas, bases, O, om.SE, -3, -1, 200, tile, pitch=pitch, gap=gap)
        for i in range(3):
            assert np.array_equal(got[i], om.overlay(bases[i], O, om.SE, -3, -1, 200, tile)), (i, pitch, gap, tile)
    assert np.array_equal(counters(ik) - c0, (3, 9))


def test_refusals_leave_everything_alone(ik, areas):
    d_base, d_ov = areas
    B, O = noise(6, 10, 3, 1, seed=1)[None], noise(3, 4, 4, 1, seed=2)
    c0 = counters(ik)
    for kw in (dict(g=9), dict(g=-1), dict(op=0), dict(op=256), dict(tile=2), dict(dx=(1 << 24) + 1),
               dict(dy=-(1 << 24) - 1)):
        run_overlay(ik, areas, B, O, expect=IK_ERR_INVALID, **kw)
    ok = [d_base, 10, 6, 3, 1, 32, 192, 2, d_ov, 4, 3, 4, 1, 16, 0, 0, 0, 255, 0, None]
    names = ["base", "W", "H", "C", "depth", "pitch", "stride", "n", "ov", "wo", "ho", "co", "od", "op", "g", "dx", "dy",
             "opacity", "tile", "stream"]
    for k, v in (("base", None), ("ov", None), ("W", 0), ("H", 0), ("n", 0), ("C", 0), ("C", 5), ("depth", 3), ("wo", 0),
                 ("ho", 0), ("co", 0), ("co", 5), ("od", 0), ("od", 3), ("stride", 191), ("pitch", 29), ("op", 15), ("n", 65536), ("ov", d_base + 64)):
        a = list(ok)
        a[names.index(k)] = v
        assert ik.ik_overlay_batch_device(*a) == IK_ERR_INVALID, (k, v)
        assert _lib.last_error()
    assert np.array_equal(counters(ik), c0), "a refused call counted a launch"


# ---- image handles ------------------------------------------------------------------------
def test_image_overlay_equals_model(ik):
    for C, depth in FORMATS:
        img = noise(37, 53, C, depth, seed=C * 10 + depth)
        d = DynamicImage.from_array(img[..., 0] if C == 1 else img)
        for co, od in ((4, 1), (1, 1), (3, 2), (2, 2)):
            mk = noise(7, 12, co, od, seed=co)
            mark = DynamicImage.from_array(mk[..., 0] if co == 1 else mk)
            for g, dx, dy, op, tile in ((Gravity.center, 0, 0, 255, False), (Gravity.se, -2, -3, 128, False),
                                        ("nw", -5, 2, 200, True)):
                c0 = counters(ik)
                got = d.overlay(mark, g, dx, dy, op, tile)
                assert np.array_equal(counters(ik) - c0, (1, 1))
                assert got.dimensions() == (53, 37) and got.depth == depth and got.channels == C
                want = om.overlay(img, mk, int(Overlay(mark, g).gravity), dx, dy, op, tile)
                np.testing.assert_array_equal(got.to_array().reshape(want.shape), want)
            np.testing.assert_array_equal(d.to_array().reshape(img.shape), img)  # img is not changed
            np.testing.assert_array_equal(mark.to_array().reshape(mk.shape), mk)
        c0 = counters(ik)
        far = d.overlay(mark, Gravity.nw, 100, 0)  # an empty window: an equal copy, no launch
        assert far._h.value != d._h.value
        np.testing.assert_array_equal(far.to_array(), d.to_array())
        assert np.array_equal(counters(ik), c0)
    out = ctypes.c_void_p()
    for bad in ((9, 0, 0, 255, 0), (0, 1 << 25, 0, 255, 0), (0, 0, 0, 0, 0), (0, 0, 0, 256, 0), (0, 0, 0, 255, 2)):
        assert ik.ik_image_overlay(d._h, mark._h, *bad, ctypes.byref(out)) == IK_ERR_INVALID
    assert ik.ik_image_overlay(d._h, None, 0, 0, 0, 255, 0, ctypes.byref(out)) == IK_ERR_INVALID


# ---- transforms ---------------------------------------------------------------------------
def png_of(img):
    b = io.BytesIO()
    mode = {1: "L", 2: "LA", 3: "RGB", 4: "RGBA"}[1 if img.ndim == 2 else img.shape[2]]
    Image.fromarray(img, mode).save(b, format="PNG")
    return b.getvalue()


@pytest.fixture(scope="module")
def files():
    rgba = ikutil.synth(96, 64, 4, seed=21, pattern="S", alpha="random")
    rgb = [ikutil.synth(96, 64, 3, seed=23 + i, pattern="S") for i in range(4)]
    other = ikutil.synth(72, 48, 3, seed=29, pattern="S")
    jb = io.BytesIO()
    Image.fromarray(rgb[0], "RGB").save(jb, format="JPEG", quality=90)
    return {"rgba": png_of(rgba), "rgb": [png_of(r) for r in rgb], "other": png_of(other), "jpeg": jb.getvalue()}


@pytest.fixture(scope="module")
def marks(ik):
    a = DynamicImage.from_array(noise(10, 24, 4, 1, seed=31))
    b = DynamicImage.from_array(noise(6, 6, 2, 1, seed=32))
    return a, b


def chain(data, w, h, o, fmt, q, sharpen=None):
    img, _ = decode_image(data)
    rs = resize_image(img, w, h)
    if sharpen:
        rs = rs.unsharpen(sharpen)
    return encode_image(rs.overlay(o), fmt, q)


@pytest.mark.parametrize("fmt,q", [(J, 85), (WP, 80)], ids=["jpeg85", "webp80"])
def test_transform_opts_equals_the_chain(ik, files, marks, fmt, q):
    for data in (files["rgba"], files["rgb"][0], files["jpeg"]):
        for o in (Overlay(marks[0], "se", -2, -2, 200), Overlay(marks[1], tile=True, opacity=90), Overlay(marks[0])):
            c0 = counters(ik)
            got = transform(data, 48, 32, fmt, q, overlay=o)
            assert np.array_equal(counters(ik) - c0, (1, 1))
            assert got == chain(data, 48, 32, o, fmt, q)
            assert got != transform(data, 48, 32, fmt, q)
            # w and h both None: the decoded image itself is composited, in place, and it is the call's own
            assert transform(data, None, None, fmt, q, overlay=o) == chain(data, None, None, o, fmt, q)
            # with sharpen set: the mark goes on after the filter and is not sharpened
            assert transform(data, 48, 32, fmt, q, sharpen=1.5, overlay=o) == chain(data, 48, 32, o, fmt, q, 1.5)
    assert transform(files["rgb"][0], 48, 32, fmt, q, overlay=marks[0]) == chain(files["rgb"][0], 48, 32, Overlay(marks[0]), fmt, q)


def mixed_requests(files, marks):
    """(data, (w, h), overlay, fmt, quality): four same-geometry requests that share one
    overlay, one of that geometry with another gravity, two with none, one of another geometry"""
    A, Bm = marks
    share = Overlay(A, "se", -2, -2, 200)
    r = files["rgb"]
    return [(r[0], (48, 32), share, J, 85), (r[1], (48, 32), share, J, 85), (r[2], (48, 32), None, J, 85),
            (r[3], (48, 32), Overlay(A, "se", -2, -2, 200), WP, 80),  # an equal Overlay of the same handle: shares
            (r[0], (48, 32), Overlay(A, "nw", -2, -2, 200), J, 85), (r[1], (48, 32), None, WP, 80),
            (files["other"], (36, 24), Overlay(Bm, tile=True), J, 85), (r[2], (48, 32), share, WP, 80)]


def test_mixed_batch_equals_each_request_alone(ik, files, marks):
    reqs = mixed_requests(files, marks)
    alone = [transform(r[0], r[1][0], r[1][1], r[3], r[4], overlay=r[2]) for r in reqs]
    args = ([r[0] for r in reqs], [r[1] for r in reqs], [r[3] for r in reqs], [r[4] for r in reqs])
    kw = dict(overlays=[r[2] for r in reqs])
    for run in (lambda: transform_batch(*args, **kw), lambda: transform_batch_submit(*args, **kw).wait()):
        c0 = counters(ik)
        got = run()
        # one launch for the four that share, one for the other gravity, one for the other geometry
        assert np.array_equal(counters(ik) - c0, (3, 6))
        for i in range(len(reqs)):
            assert got[i] == alone[i], i
    assert alone[0] != alone[4]
    # one overlay for all
    got = transform_batch(*args, overlays=reqs[0][2])
    assert got[0] == alone[0] and got[2] == transform(reqs[2][0], 48, 32, J, 85, overlay=reqs[0][2]) and got[2] != alone[2]


def test_device_resident_submit(ik, files, marks):
    reqs = mixed_requests(files, marks)
    args = ([r[1] for r in reqs], [r[3] for r in reqs], [r[4] for r in reqs])
    kw = dict(overlays=[r[2] for r in reqs])
    datas = [r[0] for r in reqs]
    assert ik.ik_set_png_gpu_min(0) == 0
    try:
        want = transform_batch_submit(datas, *args, **kw).wait()
        dev = [DeviceBytes(d) for d in datas]
        c0 = counters(ik)
        got = transform_batch_submit_device(dev, *args, **kw).wait()
        assert np.array_equal(counters(ik) - c0, (3, 6))
        assert got == want
        plain = transform_batch_submit_device(dev, *args).wait()
        assert [g == p for g, p in zip(got, plain)] == [r[2] is None for r in reqs]
    finally:
        ik.ik_set_png_gpu_min(256 << 10)


def _raw_batch(ik, fn, datas, sizes, fmts, qs, opts, opt_size, ticketed=False):
    n = len(datas)
    keep, ptrs, lens = _inputs(datas)
    ws = (ctypes.c_int64 * n)(*[s[0] for s in sizes])
    hs = (ctypes.c_int64 * n)(*[s[1] for s in sizes])
    fs = (ctypes.c_int * n)(*[int(f.value) for f in fmts])
    qa = (ctypes.c_int * n)(*qs)
    outs, olens, status = (ctypes.c_void_p * n)(), (ctypes.c_size_t * n)(), (ctypes.c_int * n)()
    ticket = ctypes.c_uint64()
    tail = [fs, qa, 4, 0, outs, olens, status] + ([ctypes.byref(ticket)] if ticketed else [])
    rc = fn(ptrs, lens, n, ws, hs, opts, opt_size, *tail)
    if rc == 0 and ticketed:
        rc = ik.ik_transform_batch_wait(ticket.value)
    res = []
    for i in range(n):
        res.append(ctypes.string_at(outs[i], olens[i]) if outs[i] else None)
        if outs[i]:
            ik.ik_buf_free(outs[i])
    if rc:
        raise TransformError(_lib.last_error())
    return res


def test_nothing_moved_at_the_defaults(ik, files):
    """overlay NULL in the 56-byte layout: the bytes of the 24-byte layout, and no overlay launch"""
    datas = [files["rgba"], files["rgb"][0], files["rgb"][1], files["jpeg"]]
    sizes, fmts, qs = [(32, 20), (20, 14), (48, 32), (30, 30)], [J, WP, WP, J], [85, 80, 80, 90]
    n = 4
    o2, o3 = (_lib.RequestOpts2 * n)(), (_lib.RequestOpts3 * n)()
    for i in range(n):
        o2[i].background = o3[i].background = -1
    o2[1].fit = o3[1].fit = int(FitMode.cover)
    o2[2].sharpen_sigma = o3[2].sharpen_sigma = 1.0
    c0 = counters(ik)
    for fn, ticketed in ((ik.ik_transform_batch_opts, False), (ik.ik_transform_batch_submit_opts, True)):
        a = _raw_batch(ik, fn, datas, sizes, fmts, qs, o2, 24, ticketed)
        b = _raw_batch(ik, fn, datas, sizes, fmts, qs, o3, 56, ticketed)
        assert a == b and all(a)
    buf, ln = _lib.u8p(), ctypes.c_size_t()
    single = []
    for o, size in ((o2[2], 24), (o3[2], 56)):
        assert ik.ik_transform_opts(datas[2], len(datas[2]), 48, 32, int(WP.value), 80, 4, ctypes.byref(o), size,
                                    ctypes.byref(buf), ctypes.byref(ln)) == 0, _lib.last_error()
        single.append(ctypes.string_at(buf, ln.value))
        ik.ik_buf_free(buf)
    assert single[0] == single[1] == a[2]
    assert np.array_equal(counters(ik), c0)
