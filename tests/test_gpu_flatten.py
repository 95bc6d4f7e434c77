"""GPU: the background flatten.  Everything is compared with zero tolerance (the one Pillow
bound says so itself): k_flatten against tests/flatten_model.py for the six variants, every
(sample, alpha) pair and the row edges, on the wide and the byte path, with a canary around
every written row; its refusals; ik_image_flatten; the bleed that flatten-then-resize
removes; ik_transform_opts against the by-hand chain; a mixed batch against each request
alone, with the launch counters; the device-resident form; and the *_opts calls at their
defaults against the entry points without options."""
import ctypes
import io

import numpy as np
import pytest
from PIL import Image

import flatten_model as fm
import ikutil
from imagekit import (DeviceBytes, DynamicImage, FilterType, FitMode, ImageFormat, Orientation, TransformError, _lib,
                      decode_image, encode_image, resize_image, transform_batch, transform_batch_submit,
                      transform_batch_submit_device)
from imagekit.transform import _inputs, transform

pytestmark = pytest.mark.gpu
CANARY = 0xA5
IK_ERR_INVALID = 2
AREA = 1 << 20  # bytes of each of the two device areas the kernel tests share
OPT_SIZE = ctypes.sizeof(_lib.RequestOpts)
VARIANTS = [(4, 3, 1), (2, 1, 1), (2, 3, 1), (4, 3, 2), (2, 1, 2), (2, 3, 2)]  # (C, out channels, depth)
J, WP, AV = ImageFormat.jpeg, ImageFormat.webp, ImageFormat.avif


@pytest.fixture(scope="module")
def areas(ik):
    d_src, d_dst = ctypes.c_void_p(), ctypes.c_void_p()
    assert ik.ik_dev_alloc(AREA, ctypes.byref(d_src)) == 0
    assert ik.ik_dev_alloc(AREA, ctypes.byref(d_dst)) == 0
    yield d_src.value, d_dst.value
    ik.ik_dev_free(d_src)
    ik.ik_dev_free(d_dst)


def counters(ik):
    c = (ctypes.c_ulonglong * 2)()
    assert ik.ik_flatten_counters(c) == 0
    return np.array([c[0], c[1]], dtype=np.int64)


def as_bytes(imgs):
    """(n, H, W, C) uint8 / uint16 as (n, H, W * C * depth) bytes, native-endian as the device holds them"""
    n, H = imgs.shape[:2]
    return np.ascontiguousarray(imgs).view(np.uint8).reshape(n, H, -1)


def run_flatten(ik, areas, imgs, rgb, oc, src_pitch=None, dst_pitch=None, src_gap=0, dst_gap=0, src_off=0, dst_off=0,
                expect=0):
    """imgs (n, H, W, C) through ik_flatten_batch_device.  Returns (n, H, W, oc) of imgs'
    dtype after checking that no byte of the destination area outside the W * oc * depth
    bytes of each row changed: pitch gaps, before the first row, after the last, between images."""
    d_src, d_dst = areas
    n, H, W, C = imgs.shape
    depth = imgs.dtype.itemsize
    srow, drow = W * C * depth, W * oc * depth
    src_pitch = src_pitch or srow
    dst_pitch = dst_pitch or drow
    sstride, dstride = src_pitch * H + src_gap, dst_pitch * H + dst_gap
    src = np.full(src_off + n * sstride, 0x3C, np.uint8)
    sb = as_bytes(imgs)
    for i in range(n):
        src[src_off + i * sstride:src_off + i * sstride + src_pitch * H].reshape(H, src_pitch)[:, :srow] = sb[i]
    dst = np.full(dst_off + n * dstride + 64, CANARY, np.uint8)
    assert src.nbytes <= AREA and dst.nbytes <= AREA
    assert ik.ik_memcpy_h2d(d_src, src.ctypes.data, src.nbytes) == 0
    assert ik.ik_memcpy_h2d(d_dst, dst.ctypes.data, dst.nbytes) == 0
    rc = ik.ik_flatten_batch_device(d_src + src_off, W, H, C, depth, src_pitch, sstride, n, rgb, oc, d_dst + dst_off,
                                    dst_pitch, dstride, None)
    assert rc == expect, _lib.last_error()
    assert ik.ik_dev_synchronize() == 0
    assert ik.ik_memcpy_d2h(dst.ctypes.data, d_dst, dst.nbytes) == 0
    if expect:
        assert (dst == CANARY).all(), "a refused call wrote to the destination"
        return None
    out = np.zeros((n, H, drow), np.uint8)
    keep = np.ones(dst.size, bool)
    for i in range(n):
        lo = dst_off + i * dstride
        out[i] = dst[lo:lo + dst_pitch * H].reshape(H, dst_pitch)[:, :drow]
        keep[lo:lo + dst_pitch * H].reshape(H, dst_pitch)[:, :drow] = False
    assert (dst[keep] == CANARY).all(), "a store outside the W * out_channels * depth bytes of a row"
    return out.view(imgs.dtype).reshape(n, H, W, oc)


def grid_source(C, depth):
    """256 x 256: pixel (x, y) carries sample V[x] and alpha V[y]; the other colour channels
    are fixed permutations of x.  V is the identity at 8 bits; at 16 bits the edge set plus
    seeded random values."""
    if depth == 1:
        V = np.arange(256, dtype=np.uint8)
    else:
        rnd = np.random.default_rng(0xF1A7 + C).integers(0, 65536, 256 - len(fm.EDGE16))
        V = np.concatenate([np.array(fm.EDGE16), rnd]).astype(np.uint16)
    x = np.arange(256)
    img = np.empty((256, 256, C), V.dtype)
    img[..., 0] = V[x][None, :]
    if C == 4:
        img[..., 1] = V[(x * 7 + 13) % 256][None, :]
        img[..., 2] = V[255 - x][None, :]
    img[..., C - 1] = V[x][:, None]
    return img


@pytest.mark.parametrize("C,oc,depth", VARIANTS, ids=lambda v: str(v))
def test_kernel_equals_model(ik, areas, C, oc, depth):
    img = grid_source(C, depth)
    ran = 0
    for rgb in (0x000000, 0xFFFFFF, 0x7F80FE, 0x010101):
        if oc == 1 and fm.out_channels(2, rgb) != 1:
            continue  # (a refusal: test_refusals)
        got = run_flatten(ik, areas, img[None], rgb, oc)
        np.testing.assert_array_equal(got[0], fm.flatten(img, rgb, oc), err_msg="%06x" % rgb)
        ran += 1
    assert ran == (3 if oc == 1 else 4)


def noise(n, H, W, C, depth, seed):
    r = np.random.default_rng(seed).integers(0, 256 ** depth, (n, H, W, C))
    r[..., C - 1][r[..., C - 1] % 5 == 0] = 0            # plenty of alpha 0 and alpha M among the random ones
    r[..., C - 1][r[..., C - 1] % 5 == 1] = 256 ** depth - 1
    return r.astype(np.uint8 if depth == 1 else np.uint16)


@pytest.mark.parametrize("C,oc,depth", VARIANTS, ids=lambda v: str(v))
def test_row_edges_on_both_paths(ik, areas, C, oc, depth):
    S, cap = ik.ik_flatten_span(), ik.ik_flatten_row_cap()
    assert S >= 8 and cap >= 1
    rgb = 0x808080 if oc == 1 else 0x7F80FE
    cases = [(W, H) for W in (1, 2, 3, 4, 5, S - 1, S, S + 1, 2 * S + 3) for H in (1, 2, 5)] + [(3, cap + 2)]
    for W, H in cases:
        img = noise(1, H, W, C, depth, seed=W * 31 + H)
        want = fm.flatten(img[0], rgb, oc)
        srow, drow = W * C * depth, W * oc * depth
        for sp, dp, so, do in (((srow + 3) // 4 * 4 + 4, (drow + 3) // 4 * 4 + 8, 0, 4),    # the wide path, both sides
                               (srow + 5 - srow % 2, drow + 3 - drow % 2, 1, 3),          # bytes: base + 1, odd pitches
                               ((srow + 3) // 4 * 4, drow + 3 - drow % 2, 0, 1),          # wide loads, byte stores
                               (srow + 5 - srow % 2, (drow + 3) // 4 * 4 + 4, 3, 0)):     # byte loads, wide stores
            got = run_flatten(ik, areas, img, rgb, oc, sp, dp, 0, 0, so, do)
            assert np.array_equal(got[0], want), (W, H, sp, dp, so, do)


@pytest.mark.parametrize("C,oc,depth", [(4, 3, 1), (2, 3, 1), (2, 1, 2), (4, 3, 2)], ids=lambda v: str(v))
def test_batch_of_three_with_gaps(ik, areas, C, oc, depth):
    S = ik.ik_flatten_span()
    W, H = S + 7, 6
    rgb = 0x101010 if oc == 1 else 0xFE017F
    imgs = noise(3, H, W, C, depth, seed=77)
    srow, drow = W * C * depth, W * oc * depth
    for sp, dp, sg, dg in (((srow + 3) // 4 * 4 + 12, (drow + 3) // 4 * 4 + 4, 40, 100),
                           (srow + 7 - srow % 2, drow + 1 - drow % 2 + 2, 33, 77)):
        got = run_flatten(ik, areas, imgs, rgb, oc, sp, dp, sg, dg)
        for i in range(3):
            assert np.array_equal(got[i], fm.flatten(imgs[i], rgb, oc)), (i, sp, dp)


def test_refusals_leave_the_destination_alone(ik, areas):
    d_src, d_dst = areas
    before = counters(ik)

    def refused(*args):
        dst = np.full(8192, CANARY, np.uint8)
        assert ik.ik_memcpy_h2d(d_dst, dst.ctypes.data, dst.nbytes) == 0
        assert ik.ik_flatten_batch_device(*args) == IK_ERR_INVALID, args
        assert _lib.last_error()
        assert ik.ik_dev_synchronize() == 0
        assert ik.ik_memcpy_d2h(dst.ctypes.data, d_dst, dst.nbytes) == 0
        assert (dst == CANARY).all(), args

    names = ["src", "W", "H", "C", "depth", "sp", "ss", "n", "rgb", "oc", "dst", "dp", "ds", "stream"]
    for C, oc, rgb in ((4, 3, 0x7F80FE), (2, 1, 0x404040), (2, 3, 0x7F80FE), (2, 3, 0x404040)):
        ok = [d_src, 10, 6, C, 1, 10 * C + 4, (10 * C + 4) * 6, 2, rgb, oc, d_dst, 10 * oc + 2, (10 * oc + 2) * 6, None]
        assert ik.ik_flatten_batch_device(*ok) == 0
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
        for c in (0, 1, 3, 5):
            refused(*but(C=c))
        refused(*but(depth=0))
        refused(*but(depth=3))
        for o in (0, 2, 4):
            refused(*but(oc=o))
        if C == 4:
            refused(*but(oc=1))
        refused(*but(rgb=-1))
        refused(*but(rgb=0x1000000))
        refused(*but(sp=10 * C - 1))
        refused(*but(dp=10 * oc - 1))
        refused(*but(depth=2, sp=20 * C - 1, ss=20 * C * 6, dp=20 * oc, ds=20 * oc * 6))
        refused(*but(ss=(10 * C + 4) * 6 - 1))  # n > 1: below rows * pitch
        refused(*but(ds=(10 * oc + 2) * 6 - 1))
        refused(*but(n=65536))
    refused(d_src, 10, 6, 2, 1, 24, 144, 2, 0x7F80FE, 1, d_dst, 12, 72, None)  # Luma wants a gray colour
    refused(d_src, 10, 6, 2, 1, 24, 144, 2, 0x808081, 1, d_dst, 12, 72, None)
    # one image: the strides are not looked at
    assert ik.ik_flatten_batch_device(d_src, 10, 6, 4, 1, 40, 0, 1, 0x123456, 3, d_dst, 30, 0, None) == 0
    assert ik.ik_dev_synchronize() == 0
    before += (1, 1)
    assert np.array_equal(counters(ik), before), "a refused call counted a launch"


# ---- image handles ------------------------------------------------------------------------
def test_image_flatten_equals_model(ik):
    for C, depth in ((4, 1), (2, 1), (4, 2), (2, 2)):
        img = noise(1, 37, 53, C, depth, seed=C * 10 + depth)[0]
        d = DynamicImage.from_array(img)
        for bg in (0xFFFFFF, 0x000000, 0x7F80FE, 0x333333):
            c0 = counters(ik)
            got = d.flatten(bg)
            assert np.array_equal(counters(ik) - c0, (1, 1))
            want = fm.flatten(img, bg)
            assert got.dimensions() == (53, 37) and got.depth == depth
            assert got.channels == fm.out_channels(C, bg)
            np.testing.assert_array_equal(got.to_array(), want)
        np.testing.assert_array_equal(d.flatten((0x7F, 0x80, 0xFE)).to_array(), d.flatten("#7f80fe").to_array())
        c0 = counters(ik)
        np.testing.assert_array_equal(d.flatten(None).to_array(), img)  # IK_BG_NONE: an equal copy
        assert np.array_equal(counters(ik), c0)
    for C, depth in ((3, 1), (1, 1), (3, 2), (1, 2)):
        img = noise(1, 20, 31, C, depth, seed=5)[0]
        d = DynamicImage.from_array(img[..., 0] if C == 1 else img)
        c0 = counters(ik)
        for bg in (0x123456, None):
            got = d.flatten(bg)
            assert got._h.value != d._h.value
            np.testing.assert_array_equal(got.to_array(), d.to_array())
        assert np.array_equal(counters(ik), c0), "an image without alpha was flattened"
    out = ctypes.c_void_p()
    d = DynamicImage.from_array(noise(1, 4, 4, 4, 1, seed=1)[0])
    for bad in (-2, 0x1000000, -100):
        assert ik.ik_image_flatten(d._h, bad, ctypes.byref(out)) == IK_ERR_INVALID
    assert ik.ik_image_flatten(None, 0, ctypes.byref(out)) == IK_ERR_INVALID
    with pytest.raises(ValueError):
        d.flatten("white")


def test_image_flatten_within_one_of_pillow(ik):
    """A sanity bound, tolerance +-1 stated as such: Pillow's alpha_composite blends in two
    rounded steps, so it bounds the definition and is not the definition."""
    img = noise(1, 64, 64, 4, 1, seed=9)[0]
    for bg in (0xFFFFFF, 0x000000, 0x7F80FE):
        back = Image.new("RGBA", (64, 64), fm.background_channels(bg, 1) + (255,))
        pil = np.asarray(Image.alpha_composite(back, Image.fromarray(img, "RGBA")))
        assert (pil[..., 3] == 255).all()
        got = DynamicImage.from_array(img).flatten(bg).to_array()
        assert np.abs(got.astype(int) - pil[..., :3].astype(int)).max() <= 1


@pytest.mark.parametrize("f", [FilterType.Lanczos3, FilterType.Triangle], ids=lambda f: f.name)
def test_the_bleed_is_gone(ik, oracle, f):
    """Left half opaque blue, right half red under alpha 0, onto white, 64 x 64 -> 16 x 16.
    Flatten-then-resize is the oracle's resize of the model-flattened pixels, bit for bit, and
    no pixel left of the boundary column (8) has red above blue; nor has any other: what
    red there is came from the white, which gives green the same, so red == green throughout.
    Without a background the hidden red is visible: red above blue from the boundary column
    on, and left of it red above green (the opaque blue has neither): the bleed that
    test_gpu_alpha.py documents.  (Left of the boundary the bled red stays below the blue,
    17 of 238 for Lanczos3 and 32 of 223 for Triangle in column 7: red above blue is only
    reached from column 8 on.)"""
    src = np.zeros((64, 64, 4), np.uint8)
    src[:, :32] = (0, 0, 255, 255)
    src[:, 32:] = (255, 0, 0, 0)
    d = DynamicImage.from_array(src)
    got = d.flatten(0xFFFFFF).resize_exact(16, 16, f).to_array()
    np.testing.assert_array_equal(got, oracle.resize(fm.flatten(src, 0xFFFFFF), 16, 16, int(f)))
    r, g, b = (got[..., k].astype(int) for k in range(3))
    assert not (r[:, :8] > b[:, :8]).any()
    assert not (r > b).any() and (r == g).all()
    raw = d.resize_exact(16, 16, f).to_array()
    np.testing.assert_array_equal(raw, oracle.resize(src, 16, 16, int(f)))
    rr, rg, rb = (raw[..., k].astype(int) for k in range(3))
    assert (rr > rb).any() and (rr[:, 8:] > rb[:, 8:]).all()
    assert (rr[:, :8] > rg[:, :8]).any() and (rg == 0).all()


# ---- transforms ---------------------------------------------------------------------------
def png_of(img):
    b = io.BytesIO()
    mode = {1: "L", 2: "LA", 3: "RGB", 4: "RGBA"}[1 if img.ndim == 2 else img.shape[2]]
    Image.fromarray(img, mode).save(b, format="PNG")
    return b.getvalue()


@pytest.fixture(scope="module")
def files():
    rgba = ikutil.synth(96, 64, 4, seed=21, pattern="S", alpha="random")
    la = ikutil.synth(80, 56, 2, seed=22, pattern="S", alpha="edge")
    rgb = ikutil.synth(72, 48, 3, seed=23, pattern="S")
    assert rgba[..., 3].min() < 255 and la[..., 1].min() < 255
    jb = io.BytesIO()
    Image.fromarray(rgb, "RGB").save(jb, format="JPEG", quality=90)
    return {"rgba": png_of(rgba), "la": png_of(la), "rgb": png_of(rgb), "jpeg": jb.getvalue()}


def opts_of(fit=0, orient=0, bg=None):
    return _lib.RequestOpts(int(fit), int(orient), -1 if bg is None else bg)


def call_opts(ik, data, w, h, fmt, q, filt, opts, opt_size=OPT_SIZE):
    buf, n = _lib.u8p(), ctypes.c_size_t()
    rc = ik.ik_transform_opts(data, len(data), w, h, int(fmt.value), q, filt, ctypes.byref(opts) if opts else None,
                              opt_size, ctypes.byref(buf), ctypes.byref(n))
    assert rc == 0, _lib.last_error()
    try:
        return ctypes.string_at(buf, n.value)
    finally:
        ik.ik_buf_free(buf)


@pytest.mark.parametrize("fmt,q", [(J, 85), (WP, 80)], ids=["jpeg85", "webp80"])
def test_transform_opts_equals_the_chain(ik, files, fmt, q):
    for name, bg in (("rgba", 0x7F80FE), ("la", 0x7F80FE), ("la", 0xFFFFFF), ("rgba", 0x000000)):
        data = files[name]
        c0 = counters(ik)
        got = call_opts(ik, data, 40, 24, fmt, q, 4, opts_of(FitMode.cover, 6, bg))
        assert np.array_equal(counters(ik) - c0, (1, 1))
        img, _ = decode_image(data)
        flat = img.apply_orientation(6).flatten(bg)
        assert flat.channels == fm.out_channels(4 if name == "rgba" else 2, bg)
        want = encode_image(resize_image(flat, 40, 24, fit=FitMode.cover), fmt, q)
        assert got == want, (name, bg)
        assert got == transform(data, 40, 24, fmt, q, fit=FitMode.cover, orient=6, background=bg)
        none = call_opts(ik, data, 40, 24, fmt, q, 4, opts_of(FitMode.cover, 6, None))
        assert none == transform(data, 40, 24, fmt, q, fit=FitMode.cover, orient=6)
        assert got != none, "the background changed nothing"


def test_avif_with_a_background_has_no_alpha_plane(ik, files):
    for name in ("rgba", "la"):
        with_bg = Image.open(io.BytesIO(transform(files[name], 32, 32, AV, 80, background=0xFFFFFF)))
        assert "A" not in with_bg.getbands() and with_bg.size[0] <= 32
        without = Image.open(io.BytesIO(transform(files[name], 32, 32, AV, 80)))
        assert "A" in without.getbands()


def mixed_requests(files):
    cover, contain, exact = FitMode.cover, FitMode.contain, FitMode.exact
    white, black, colour = 0xFFFFFF, 0x000000, 0x7F80FE
    A, L, R, Jf = files["rgba"], files["la"], files["rgb"], files["jpeg"]
    return [  # data, (w, h), fit, orient, background, fmt, quality
        (A, (32, 32), cover, 0, white, J, 85), (A, (32, 32), cover, 0, white, J, 85),      # four of one
        (A, (40, None), contain, 0, white, WP, 80), (A, (17, 9), exact, 0, white, J, 70),   # (geometry, background)
        (A, (32, 32), cover, 6, black, WP, 80),
        (L, (30, 30), contain, 3, colour, J, 85),
        (L, (24, 24), cover, 0, white, WP, 80),
        (A, (32, 32), cover, 0, None, J, 85),
        (R, (20, 20), cover, 5, white, J, 85),
        (Jf, (25, None), contain, 0, black, WP, 80),
        (Jf, (16, 16), exact, 8, None, J, 85),
        (R, (33, 21), exact, 0, colour, WP, 80),
    ]


def test_mixed_batch_equals_each_request_alone(ik, files):
    reqs = mixed_requests(files)
    assert len(reqs) == 12
    alone = [call_opts(ik, r[0], r[1][0], -1 if r[1][1] is None else r[1][1], r[5], r[6], 4, opts_of(r[2], r[3], r[4]))
             for r in reqs]
    kw = dict(fits=[r[2] for r in reqs], orient=[r[3] for r in reqs], backgrounds=[r[4] for r in reqs])
    args = ([r[0] for r in reqs], [r[1] for r in reqs], [r[5] for r in reqs], [r[6] for r in reqs])
    # the four of one (geometry, background) share a launch; the black RGBA and the two LA
    # requests take one each; the requests without alpha or without a background take none
    for run in (lambda: transform_batch(*args, **kw), lambda: transform_batch_submit(*args, **kw).wait()):
        c0 = counters(ik)
        got = run()
        assert np.array_equal(counters(ik) - c0, (4, 7))
        for i in range(12):
            assert got[i] == alone[i], i
    # the group of four beside requests that are not flattened: one launch in all
    sub = [0, 1, 2, 3, 7, 8, 9, 10, 11]
    c0 = counters(ik)
    got = transform_batch(*[[a[i] for i in sub] for a in args], **{k: [v[i] for i in sub] for k, v in kw.items()})
    assert np.array_equal(counters(ik) - c0, (1, 4))
    assert got == [alone[i] for i in sub]
    # requests without alpha or without a background alone: no launch
    sub = [7, 8, 9, 10, 11]
    c0 = counters(ik)
    got = transform_batch(*[[a[i] for i in sub] for a in args], **{k: [v[i] for i in sub] for k, v in kw.items()})
    assert np.array_equal(counters(ik), c0)
    assert got == [alone[i] for i in sub]
    # the background matters where there is alpha, and only there
    assert alone[0] != alone[7]
    assert alone[8] == transform(reqs[8][0], 20, 20, J, 85, fit=FitMode.cover, orient=5)
    with pytest.raises(ValueError):
        transform_batch(*args, fits=kw["fits"], orient=kw["orient"], backgrounds=["nope"] * 12)
    with pytest.raises(TransformError):  # IK_ERR_INVALID from the library: a bad fit inside the options
        bad = (_lib.RequestOpts * 1)(_lib.RequestOpts(7, 0, 0xFFFFFF))
        _raw_batch(ik, ik.ik_transform_batch_opts, [files["rgba"]], [(8, 8)], [J], [80], bad, OPT_SIZE)


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


def png_counts(ik):
    c = (ctypes.c_ulonglong * 2)()
    assert ik.ik_png_counters(c) == 0
    return c[0], c[1]


def test_device_resident_batch(ik, files):
    pngs = [png_of(ikutil.synth(128, 96, 4, seed=30 + k, pattern="N", alpha="random")) for k in range(4)]
    kw = dict(fits=[FitMode.cover] * 4, backgrounds=[0xFFFFFF] * 4)
    args = ([(48, 48)] * 4, [WP] * 4, [80] * 4)
    assert ik.ik_set_png_gpu_min(0) == 0
    try:
        want = transform_batch_submit(pngs, *args, **kw).wait()
        dev = [DeviceBytes(p) for p in pngs]
        g0, h0 = png_counts(ik)
        c0 = counters(ik)
        got = transform_batch_submit_device(dev, *args, **kw).wait()
        g1, h1 = png_counts(ik)
        assert (g1 - g0, h1 - h0) == (4, 0), "the device-resident PNG streams must decode on the GPU"
        assert np.array_equal(counters(ik) - c0, (1, 4))
        assert got == want
        assert got != transform_batch_submit_device(dev, *args, fits=kw["fits"]).wait()
        # an explicit orientation works; IK_ORIENT_AUTO is refused before anything is queued
        turned = transform_batch_submit_device(dev, *args, orient=[6] * 4, **kw).wait()
        assert turned == transform_batch_submit(pngs, *args, orient=[6] * 4, **kw).wait() and turned != got
        with pytest.raises(TransformError, match="IK_ORIENT_AUTO"):
            transform_batch_submit_device(dev, *args, orient=[0, 0, Orientation.auto, 0], **kw)
    finally:
        ik.ik_set_png_gpu_min(256 << 10)


def test_nothing_moved_at_the_defaults(ik, files):
    """opts NULL, or every entry at its defaults: the bytes of the entry points without options,
    and no flatten launch."""
    datas = [files["rgba"], files["la"], files["rgb"], files["jpeg"]]
    sizes, fmts, qs = [(32, 20), (20, None), (16, 16), (30, 30)], [J, WP, WP, J], [85, 80, 75, 90]
    n = 4
    c0 = counters(ik)
    defaults = (_lib.RequestOpts * n)(*[opts_of() for _ in range(n)])
    for i in range(n):
        w, h = sizes[i][0], -1 if sizes[i][1] is None else sizes[i][1]
        buf, ln = _lib.u8p(), ctypes.c_size_t()
        assert ik.ik_transform_fit(datas[i], len(datas[i]), w, h, 0, int(fmts[i].value), qs[i], 4, ctypes.byref(buf),
                                   ctypes.byref(ln)) == 0
        want = ctypes.string_at(buf, ln.value)
        ik.ik_buf_free(buf)
        assert call_opts(ik, datas[i], w, h, fmts[i], qs[i], 4, None) == want
        assert call_opts(ik, datas[i], w, h, fmts[i], qs[i], 4, opts_of()) == want
    contain = (ctypes.c_int * n)(*[0] * n)
    want = _raw_batch(ik, ik.ik_transform_batch_fit, datas, sizes, fmts, qs, contain)
    for o in (None, defaults):
        assert _raw_batch(ik, ik.ik_transform_batch_opts, datas, sizes, fmts, qs, o, OPT_SIZE) == want
        assert _raw_batch(ik, ik.ik_transform_batch_submit_opts, datas, sizes, fmts, qs, o, OPT_SIZE, ticketed=True) == want
    dev = [DeviceBytes(d) for d in datas]
    want_dev = _raw_batch(ik, ik.ik_transform_batch_submit_device, dev, sizes, fmts, qs, ticketed=True)
    assert want_dev == want
    for o in (None, defaults):
        assert _raw_batch(ik, ik.ik_transform_batch_submit_device_opts, dev, sizes, fmts, qs, o, OPT_SIZE,
                          ticketed=True) == want_dev
    assert np.array_equal(counters(ik), c0), "a call at its defaults launched a flatten"
    # the Python mirror without the new arguments makes the calls it made before
    assert transform_batch(datas, sizes, fmts, qs) == want
