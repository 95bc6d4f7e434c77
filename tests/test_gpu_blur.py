"""GPU: blur and unsharpen.  Every comparison is bit-exact: k_blur against tests/blur_model.py
through ik_blur_batch_device for C = 1..4, both depths and both operations, at the tile's
edges, on the wide and the byte path, with a canary around every written row and poisoned
pitch gaps in the source; its refusals; ik_image_blur / ik_image_unsharpen; ik_transform_opts
against the by-hand chain; a mixed batch against each request alone, with the launch
counters; the device-resident form; and the 24-byte options layout at its defaults against
the 12-byte one and the entry points without options."""
import ctypes
import io

import numpy as np
import pytest
from PIL import Image

import blur_model as bm
import ikutil
from imagekit import (DeviceBytes, DynamicImage, ImageFormat, TransformError, _lib, decode_image, encode_image,
                      resize_image, transform_batch, transform_batch_submit, transform_batch_submit_device)
from imagekit.transform import _inputs, transform

pytestmark = pytest.mark.gpu
CANARY = 0xA5
POISON = 0xE7  # the source's pitch gaps and everything around its rows
IK_ERR_INVALID = 2
AREA = 1 << 20  # bytes of each of the two device areas the kernel tests share
J, WP = ImageFormat.jpeg, ImageFormat.webp
SIGMAS = (0.0625, 0.5, 1, 2.5)


@pytest.fixture(scope="module")
def areas(ik):
    d_src, d_dst = ctypes.c_void_p(), ctypes.c_void_p()
    assert ik.ik_dev_alloc(AREA, ctypes.byref(d_src)) == 0
    assert ik.ik_dev_alloc(AREA, ctypes.byref(d_dst)) == 0
    yield d_src.value, d_dst.value
    ik.ik_dev_free(d_src)
    ik.ik_dev_free(d_dst)


@pytest.fixture(scope="module")
def tile(ik):
    t = (ctypes.c_int * 2)()
    assert ik.ik_blur_tile(t) == 0
    assert t[0] >= 8 and t[1] >= 2
    return t[0], t[1]


def counters(ik):
    c = (ctypes.c_ulonglong * 2)()
    assert ik.ik_blur_counters(c) == 0
    return np.array([c[0], c[1]], dtype=np.int64)


def as_bytes(imgs):
    n, H = imgs.shape[:2]
    return np.ascontiguousarray(imgs).view(np.uint8).reshape(n, H, -1)


def run_blur(ik, areas, imgs, sigma, sharpen=0, threshold=0, src_pitch=None, dst_pitch=None, src_gap=0, dst_gap=0,
             src_off=0, dst_off=0):
    """imgs (n, H, W, C) through ik_blur_batch_device.  Returns the same shape and dtype after
    checking that no byte of the destination area outside the W * C * depth bytes of each row
    changed.  The source's gaps hold POISON: a kernel that read one would change the result."""
    d_src, d_dst = areas
    n, H, W, C = imgs.shape
    depth = imgs.dtype.itemsize
    row = W * C * depth
    src_pitch = src_pitch or row
    dst_pitch = dst_pitch or row
    sstride, dstride = src_pitch * H + src_gap, dst_pitch * H + dst_gap
    src = np.full(src_off + n * sstride + 64, POISON, np.uint8)
    sb = as_bytes(imgs)
    for i in range(n):
        src[src_off + i * sstride:src_off + i * sstride + src_pitch * H].reshape(H, src_pitch)[:, :row] = sb[i]
    dst = np.full(dst_off + n * dstride + 64, CANARY, np.uint8)
    assert src.nbytes <= AREA and dst.nbytes <= AREA
    assert ik.ik_memcpy_h2d(d_src, src.ctypes.data, src.nbytes) == 0
    assert ik.ik_memcpy_h2d(d_dst, dst.ctypes.data, dst.nbytes) == 0
    rc = ik.ik_blur_batch_device(d_src + src_off, W, H, C, depth, src_pitch, sstride, n, sigma, sharpen, threshold,
                                 d_dst + dst_off, dst_pitch, dstride, None)
    assert rc == 0, _lib.last_error()
    assert ik.ik_dev_synchronize() == 0
    assert ik.ik_memcpy_d2h(dst.ctypes.data, d_dst, dst.nbytes) == 0
    out = np.zeros((n, H, row), np.uint8)
    keep = np.ones(dst.size, bool)
    for i in range(n):
        lo = dst_off + i * dstride
        out[i] = dst[lo:lo + dst_pitch * H].reshape(H, dst_pitch)[:, :row]
        keep[lo:lo + dst_pitch * H].reshape(H, dst_pitch)[:, :row] = False
    assert (dst[keep] == CANARY).all(), "a store outside the W * C * depth bytes of a row"
    return out.view(imgs.dtype).reshape(n, H, W, C)


def contents(H, W, C, depth, seed):
    """two images: random content, and a checkerboard of 0 and M (it drives the unsharpen
    clamp at both ends), the channels' phases shifted against each other"""
    M = 256 ** depth - 1
    dt = np.uint8 if depth == 1 else np.uint16
    rnd = np.random.default_rng(seed).integers(0, M + 1, (H, W, C)).astype(dt)
    yy, xx, cc = np.mgrid[0:H, 0:W, 0:C]
    cb = (((yy + xx + cc) & 1) * M).astype(dt)
    return np.stack([rnd, cb])


def paths(row):
    """(src pitch, dst pitch, src offset, dst offset): the wide path on both sides, the byte
    path on both (base + 1, odd pitches), and the two mixtures"""
    up = (row + 3) // 4 * 4
    odd = row + 5 - row % 2
    return ((up + 4, up + 8, 0, 4), (odd, odd + 2, 1, 3), (up, odd, 4, 1), (odd, up + 4, 3, 0))


def check(ik, areas, imgs, sigma, thresholds, which):
    """blur and unsharpen of imgs against the model, on the paths named by `which`"""
    M = 256 ** imgs.dtype.itemsize - 1
    B = np.stack([bm.blur(im, sigma) for im in imgs])  # computed once, shared by every comparison below
    row = imgs.shape[2] * imgs.shape[3] * imgs.dtype.itemsize
    for p in which:
        sp, dp, so, do = paths(row)[p]
        got = run_blur(ik, areas, imgs, sigma, 0, 0, sp, dp, 0, 0, so, do)
        assert np.array_equal(got, B), ("blur", imgs.shape, sigma, p)
        for t in thresholds:
            t = M if t == "M" else t
            got = run_blur(ik, areas, imgs, sigma, 1, t, sp, dp, 0, 0, so, do)
            want = np.stack([bm.unsharpen_rule(im, b, t, M) for im, b in zip(imgs, B)])
            assert np.array_equal(got, want), ("unsharpen", imgs.shape, sigma, t, p)
            if t >= M:
                assert np.array_equal(got, imgs)  # a threshold at M never triggers


@pytest.mark.parametrize("depth", [1, 2])
@pytest.mark.parametrize("C", [1, 2, 3, 4])
def test_kernel_equals_model_at_the_tile_edges(ik, areas, tile, C, depth):
    TW, TH = tile
    sizes = [(1, 1), (1, TH + 3), (TW + 5, 1)]
    sizes += [(W, H) for W in (TW - 1, TW, TW + 1) for H in (TH - 1, TH, TH + 1)]
    sizes += [(2 * TW + 3, 2 * TH + 1)]
    k = 0
    c0 = counters(ik)
    for W, H in sizes:
        imgs = contents(H, W, C, depth, seed=W * 131 + H * 7 + C)
        for sigma in SIGMAS:
            # every size on the wide and on the byte path; the mixtures and the thresholds in turn
            check(ik, areas, imgs, sigma, [(0, 1, "M")[k % 3]], (0, 1, 2 + k % 2))
            k += 1
    # all three thresholds, all four paths, where the tile is crossed in both directions
    check(ik, areas, contents(TH + 1, TW + 1, C, depth, seed=5), 1, (0, 1, "M"), (0, 1, 2, 3))
    # a blur and an unsharpen launch of two images per (size, sigma, path); the last check 4 x 4
    launches = len(sizes) * len(SIGMAS) * 3 * 2 + 16
    assert len(sizes) == 13 and np.array_equal(counters(ik) - c0, (launches, 2 * launches))


@pytest.mark.parametrize("depth", [1, 2])
@pytest.mark.parametrize("C", [1, 2, 3, 4])
def test_the_widest_halo(ik, areas, tile, C, depth):
    """sigma 32: 129 taps, 64 columns of halo on each side; on a TW + 1 x 5 image the window is
    clamped on both sides in x and covers the whole axis in y, on 3 x 3 it does both ways"""
    TW, TH = tile
    for W, H in ((TW + 1, 5), (3, 3)):
        check(ik, areas, contents(H, W, C, depth, seed=W + C), 32, (0, "M"), (0, 1))
    # and with room for the whole window: interior outputs beside clamped ones, both axes
    imgs = contents(2 * TH + 3, 2 * TW + 70, C, depth, seed=9)[:1]
    check(ik, areas, imgs, 32, (1,), (0, 1) if C == 4 else (0,))


@pytest.mark.parametrize("C,depth", [(1, 1), (3, 1), (4, 1), (2, 2), (3, 2), (4, 2)])
def test_batch_of_three_with_gaps(ik, areas, tile, C, depth):
    TW, TH = tile
    W, H = TW + 7, TH + 2
    two = contents(H, W, C, depth, seed=77)
    imgs = np.concatenate([two, contents(H, W, C, depth, seed=78)[:1]])
    M = 256 ** depth - 1
    row = W * C * depth
    B = np.stack([bm.blur(im, 1.5) for im in imgs])
    for sp, dp, sg, dg in (((row + 3) // 4 * 4 + 12, (row + 3) // 4 * 4 + 4, 40, 100),
                           (row + 7 - row % 2, row + 3 - row % 2, 33, 77)):
        got = run_blur(ik, areas, imgs, 1.5, 0, 0, sp, dp, sg, dg)
        assert np.array_equal(got, B), (sp, dp)
        got = run_blur(ik, areas, imgs, 1.5, 1, 3, sp, dp, sg, dg)
        assert np.array_equal(got, np.stack([bm.unsharpen_rule(im, b, 3, M) for im, b in zip(imgs, B)])), (sp, dp)


def test_refusals_leave_the_destination_alone(ik, areas):
    d_src, d_dst = areas
    before = counters(ik)

    def refused(*args):
        dst = np.full(8192, CANARY, np.uint8)
        assert ik.ik_memcpy_h2d(d_dst, dst.ctypes.data, dst.nbytes) == 0
        assert ik.ik_blur_batch_device(*args) == IK_ERR_INVALID, args
        assert _lib.last_error()
        assert ik.ik_dev_synchronize() == 0
        assert ik.ik_memcpy_d2h(dst.ctypes.data, d_dst, dst.nbytes) == 0
        assert (dst == CANARY).all(), args

    names = ["src", "W", "H", "C", "depth", "sp", "ss", "n", "sigma", "sharpen", "thr", "dst", "dp", "ds", "stream"]
    for C, sharpen in ((1, 0), (3, 1), (4, 0)):
        ok = [d_src, 10, 6, C, 1, 10 * C + 4, (10 * C + 4) * 6, 2, 1.0, sharpen, 2, d_dst, 10 * C + 2, (10 * C + 2) * 6, None]
        assert ik.ik_blur_batch_device(*ok) == 0
        assert ik.ik_dev_synchronize() == 0
        before += (1, 2)

        def but(**kw):
            a = list(ok)
            for k, v in kw.items():
                a[names.index(k)] = v
            return a

        refused(*but(src=None))
        refused(*but(dst=None))
        refused(*but(W=0))
        refused(*but(H=0))
        refused(*but(n=0))
        for c in (0, 5):
            refused(*but(C=c))
        refused(*but(depth=0))
        refused(*but(depth=3))
        for s in (0.0, 0.06, 32.5, -1.0, float("nan"), float("inf")):
            refused(*but(sigma=s))
        for s in (-1, 2):
            refused(*but(sharpen=s))
        for t in (-1, 65536):
            refused(*but(thr=t))
        refused(*but(sp=10 * C - 1))
        refused(*but(dp=10 * C - 1))
        refused(*but(depth=2, sp=20 * C - 1, ss=20 * C * 6, dp=20 * C, ds=20 * C * 6))
        refused(*but(ss=(10 * C + 4) * 6 - 1))  # n > 1: below rows * pitch
        refused(*but(ds=(10 * C + 2) * 6 - 1))
        refused(*but(n=65536))
        # source and destination must not overlap: the same bytes, and one row into the other
        refused(*but(dst=d_src, dp=10 * C + 4, ds=(10 * C + 4) * 6))
        refused(*but(src=d_dst + (10 * C + 2) * 11))
        refused(*but(src=d_dst + 8, dst=d_dst))
    # one image: the strides are not looked at
    assert ik.ik_blur_batch_device(d_src, 10, 6, 4, 1, 40, 0, 1, 1.0, 0, 0, d_dst, 40, 0, None) == 0
    assert ik.ik_dev_synchronize() == 0
    before += (1, 1)
    assert np.array_equal(counters(ik), before), "a refused call counted a launch"


# ---- image handles ------------------------------------------------------------------------
def test_image_calls_equal_the_model(ik):
    out = ctypes.c_void_p()
    for C, depth in ((1, 1), (2, 1), (3, 1), (4, 1), (1, 2), (3, 2), (4, 2)):
        img = contents(37, 83, C, depth, seed=C * 10 + depth)[0]
        arr = img[..., 0] if C == 1 else img
        d = DynamicImage.from_array(arr)
        M = 256 ** depth - 1
        for sigma in (0.8, 3.0):
            B = bm.blur(arr, sigma)
            c0 = counters(ik)
            got = d.blur(sigma)
            assert np.array_equal(counters(ik) - c0, (1, 1))
            assert got.dimensions() == (83, 37) and got.depth == depth and got.channels == C
            np.testing.assert_array_equal(got.to_array().reshape(arr.shape), B)
            for t in (0, 5):
                np.testing.assert_array_equal(d.unsharpen(sigma, t).to_array().reshape(arr.shape),
                                              bm.unsharpen_rule(arr, B, t, M))
        np.testing.assert_array_equal(d.to_array().reshape(arr.shape), arr)  # the source image is unchanged
        np.testing.assert_array_equal(d.blur(0.25).to_array().reshape(arr.shape), arr)  # one tap: an equal copy
        for bad in (0.0, 0.01, 33.0, float("nan")):
            assert ik.ik_image_blur(d._h, bad, ctypes.byref(out)) == IK_ERR_INVALID
            assert ik.ik_image_unsharpen(d._h, bad, 0, ctypes.byref(out)) == IK_ERR_INVALID
        for bad in (-1, 65536):
            assert ik.ik_image_unsharpen(d._h, 1.0, bad, ctypes.byref(out)) == IK_ERR_INVALID
        with pytest.raises(ValueError):
            d.blur(0)
        with pytest.raises(ValueError):
            d.unsharpen(1.0, -1)


# ---- transforms ---------------------------------------------------------------------------
def png_of(img):
    b = io.BytesIO()
    mode = {1: "L", 2: "LA", 3: "RGB", 4: "RGBA"}[1 if img.ndim == 2 else img.shape[2]]
    Image.fromarray(img, mode).save(b, format="PNG")
    return b.getvalue()


@pytest.fixture(scope="module")
def files():
    rgb = [ikutil.synth(96, 64, 3, seed=40 + k, pattern="S") for k in range(3)]
    rgba = ikutil.synth(80, 56, 4, seed=44, pattern="S", alpha="random")
    jb = io.BytesIO()
    Image.fromarray(rgb[0], "RGB").save(jb, format="JPEG", quality=90)
    return {"rgb": [png_of(r) for r in rgb], "rgba": png_of(rgba), "jpeg": jb.getvalue()}


@pytest.mark.parametrize("fmt,q", [(J, 85), (WP, 80)], ids=["jpeg85", "webp80"])
def test_single_request_equals_the_chain(ik, files, fmt, q):
    for data in (files["rgb"][0], files["jpeg"], files["rgba"]):
        img, _ = decode_image(data)
        rs = resize_image(img, 40, 24)
        c0 = counters(ik)
        got = transform(data, 40, 24, fmt, q, sharpen=(1.0, 2))
        assert np.array_equal(counters(ik) - c0, (1, 1))
        assert got == encode_image(rs.unsharpen(1.0, 2), fmt, q)
        blurred = transform(data, 40, 24, fmt, q, blur=4)
        assert blurred == encode_image(rs.blur(4), fmt, q)
        plain = transform(data, 40, 24, fmt, q)
        assert got != plain and blurred != plain and got != blurred
        c0 = counters(ik)
        assert transform(data, 40, 24, fmt, q, blur=None, sharpen=None) == plain
        assert np.array_equal(counters(ik), c0)
    # w and h both None: the filter sees the decoded image
    data = files["rgb"][1]
    img, _ = decode_image(data)
    assert transform(data, None, None, fmt, q, sharpen=(1.0, 2)) == encode_image(img.unsharpen(1.0, 2), fmt, q)
    assert transform(data, None, None, fmt, q, blur=4) == encode_image(img.blur(4), fmt, q)
    with pytest.raises(ValueError):
        transform(data, 40, 24, fmt, q, blur=1, sharpen=1)
    with pytest.raises(ValueError):
        transform(data, 40, 24, fmt, q, blur=64)


def mixed_requests(files):
    a, b, c = files["rgb"]
    A, Bg = (48, 32), (30, 20)  # the two output geometries (96 x 64 sources, contain)
    s12, s10 = (1.0, 2), (1.0, 0)
    return [  # data, (w, h), blur, sharpen, fmt, quality
        (a, A, None, s12, J, 85), (b, A, None, s12, J, 85), (c, A, None, s12, WP, 80),  # one set of three
        (a, A, None, s10, J, 85),                                                       # a lone setting
        (b, A, 4, None, WP, 80), (c, A, 4, None, WP, 80),                               # a set of two
        (a, A, None, None, J, 85), (b, A, None, None, WP, 80),                          # no filter
        (a, Bg, None, s12, J, 85), (c, Bg, None, s12, J, 85),                           # a set of two
        (b, Bg, 0.5, None, WP, 80),                                                     # lone
        (c, Bg, None, None, J, 70),                                                     # no filter
    ]


def test_mixed_batch_equals_each_request_alone(ik, files):
    reqs = mixed_requests(files)
    assert len(reqs) == 12
    c0 = counters(ik)
    alone = [transform(r[0], r[1][0], r[1][1], r[4], r[5], blur=r[2], sharpen=r[3]) for r in reqs]
    assert np.array_equal(counters(ik) - c0, (9, 9))
    kw = dict(blurs=[r[2] for r in reqs], sharpens=[r[3] for r in reqs])
    args = ([r[0] for r in reqs], [r[1] for r in reqs], [r[4] for r in reqs], [r[5] for r in reqs])
    # five (resize group, setting) sets: 3 + 1 + 2 images of geometry A, 2 + 1 of B; the three
    # requests without a filter take no launch
    for run in (lambda: transform_batch(*args, **kw), lambda: transform_batch_submit(*args, **kw).wait()):
        c0 = counters(ik)
        got = run()
        assert np.array_equal(counters(ik) - c0, (5, 9))
        for i in range(12):
            assert got[i] == alone[i], i
    # the filter settings matter
    assert alone[0] != alone[3] and alone[0] != alone[6] and alone[4] != alone[7]
    # requests without a filter alone: no launch, the batch without the arguments
    sub = [6, 7, 11]
    c0 = counters(ik)
    got = transform_batch(*[[a[i] for i in sub] for a in args], blurs=[None] * 3, sharpens=[None] * 3)
    assert np.array_equal(counters(ik), c0)
    assert got == [alone[i] for i in sub] == transform_batch(*[[a[i] for i in sub] for a in args])
    # requests that share no resize group (one of each geometry) are filtered image by image
    sub = [0, 8]
    c0 = counters(ik)
    got = transform_batch(*[[a[i] for i in sub] for a in args], **{k: [v[i] for i in sub] for k, v in kw.items()})
    assert np.array_equal(counters(ik) - c0, (2, 2))
    assert got == [alone[i] for i in sub]
    with pytest.raises(ValueError):
        transform_batch(*args, blurs=[1.0] * 12, sharpens=[1.0] * 12)
    with pytest.raises(TransformError, match="request 1"):  # IK_ERR_INVALID from the library itself
        bad = (_lib.RequestOpts2 * 2)(_lib.RequestOpts2(0, 0, -1, 0, 0, 0), _lib.RequestOpts2(0, 0, -1, 1.0, 1.0, 0))
        _raw_batch(ik, ik.ik_transform_batch_opts, args[0][:2], args[1][:2], args[2][:2], args[3][:2], bad, 24)


def test_device_resident_batch(ik, files):
    reqs = mixed_requests(files)
    kw = dict(blurs=[r[2] for r in reqs], sharpens=[r[3] for r in reqs])
    args = ([r[1] for r in reqs], [r[4] for r in reqs], [r[5] for r in reqs])
    datas = [r[0] for r in reqs]
    assert ik.ik_set_png_gpu_min(0) == 0
    try:
        want = transform_batch_submit(datas, *args, **kw).wait()
        dev = [DeviceBytes(d) for d in datas]
        c0 = counters(ik)
        got = transform_batch_submit_device(dev, *args, **kw).wait()
        assert np.array_equal(counters(ik) - c0, (5, 9))
        assert got == want
        plain = transform_batch_submit_device(dev, *args).wait()
        assert [g == p for g, p in zip(got, plain)] == [r[2] is None and r[3] is None for r in reqs]
    finally:
        ik.ik_set_png_gpu_min(256 << 10)


def _raw_batch(ik, fn, datas, sizes, fmts, qs, *mid, ticketed=False):
    """fn(bytes, lens, n, w, h, *mid, fmt, quality, filter, threads, outs, out_lens, status[, ticket])"""
    n = len(datas)
    if isinstance(datas[0], DeviceBytes):
        ptrs = (ctypes.c_void_p * n)(*[d.ptr for d in datas])
        lens = (ctypes.c_size_t * n)(*[len(d) for d in datas])
    else:
        keep, ptrs, lens = _inputs(datas)
    ws = (ctypes.c_int64 * n)(*[s[0] for s in sizes])
    hs = (ctypes.c_int64 * n)(*[-1 if s[1] is None else s[1] for s in sizes])
    fs = (ctypes.c_int * n)(*[int(f.value) for f in fmts])
    qa = (ctypes.c_int * n)(*qs)
    outs, olens, status = (ctypes.c_void_p * n)(), (ctypes.c_size_t * n)(), (ctypes.c_int * n)()
    ticket = ctypes.c_uint64()
    tail = [fs, qa, 4, 0, outs, olens, status] + ([ctypes.byref(ticket)] if ticketed else [])
    rc = fn(ptrs, lens, n, ws, hs, *mid, *tail)
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
    """Every entry of the 24-byte layout at its defaults: the bytes of the 12-byte layout and of
    the entry points without options, and no blur launch."""
    datas = [files["rgba"], files["rgb"][0], files["rgb"][1], files["jpeg"]]
    sizes, fmts, qs = [(32, 20), (20, None), (48, 32), (30, 30)], [J, WP, WP, J], [85, 80, 80, 90]
    n = 4
    c0 = counters(ik)
    d12 = (_lib.RequestOpts * n)(*[_lib.RequestOpts(0, 0, -1) for _ in range(n)])
    d24 = (_lib.RequestOpts2 * n)(*[_lib.RequestOpts2(0, 0, -1, 0.0, 0.0, 0) for _ in range(n)])
    for i in range(n):
        w, h = sizes[i][0], -1 if sizes[i][1] is None else sizes[i][1]
        res = []
        for o in (None, _lib.RequestOpts(0, 0, -1), _lib.RequestOpts2(0, 0, -1, 0.0, 0.0, 0)):
            buf, ln = _lib.u8p(), ctypes.c_size_t()
            assert ik.ik_transform_opts(datas[i], len(datas[i]), w, h, int(fmts[i].value), qs[i], 4,
                                        ctypes.byref(o) if o is not None else None, 24 if o is None else ctypes.sizeof(o),
                                        ctypes.byref(buf), ctypes.byref(ln)) == 0, _lib.last_error()
            res.append(ctypes.string_at(buf, ln.value))
            ik.ik_buf_free(buf)
        assert res[0] == res[1] == res[2] == transform(datas[i], sizes[i][0], sizes[i][1], fmts[i], qs[i])
    want = _raw_batch(ik, ik.ik_transform_batch, datas, sizes, fmts, qs)
    for o, size in ((None, 12), (None, 24), (d12, 12), (d24, 24)):
        assert _raw_batch(ik, ik.ik_transform_batch_opts, datas, sizes, fmts, qs, o, size) == want
        assert _raw_batch(ik, ik.ik_transform_batch_submit_opts, datas, sizes, fmts, qs, o, size, ticketed=True) == want
    dev = [DeviceBytes(d) for d in datas]
    want_dev = _raw_batch(ik, ik.ik_transform_batch_submit_device, dev, sizes, fmts, qs, ticketed=True)
    assert want_dev == want
    for o, size in ((d12, 12), (d24, 24)):
        assert _raw_batch(ik, ik.ik_transform_batch_submit_device_opts, dev, sizes, fmts, qs, o, size,
                          ticketed=True) == want_dev
    assert np.array_equal(counters(ik), c0), "a call at its defaults launched a blur"
    # a threshold alone (both sigmas 0) asks for nothing
    t24 = (_lib.RequestOpts2 * n)(*[_lib.RequestOpts2(0, 0, -1, 0.0, 0.0, 9) for _ in range(n)])
    assert _raw_batch(ik, ik.ik_transform_batch_opts, datas, sizes, fmts, qs, t24, 24) == want
    assert np.array_equal(counters(ik), c0)
    assert transform_batch(datas, sizes, fmts, qs) == want
