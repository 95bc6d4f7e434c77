"""CPU: ik_blur_axis_plan against tests/blur_model.py bit for bit (the weights come from the
same glibc expf, never from the code under test); the model's own properties; the Python
argument forms; and the refusals the library makes before any device work (no GPU here)."""
import ctypes

import numpy as np
import pytest

import blur_model as bm
from imagekit import _lib
from imagekit.transform import _filter_args, _request_opts, _sharpen, _sigma

IK_ERR_INVALID = 2
F = np.float32


def lib_axis(lib, L, sigma):
    taps = ctypes.c_uint32()
    assert lib.ik_blur_axis_plan(L, sigma, None, None, None, 0, ctypes.byref(taps)) == 0, _lib.last_error()
    T = taps.value
    cap = T + 3  # rows wider than T: the padding is zero too
    left, count = (ctypes.c_int32 * L)(), (ctypes.c_int32 * L)()
    w = (ctypes.c_float * (L * cap))()
    assert lib.ik_blur_axis_plan(L, sigma, left, count, w, cap, ctypes.byref(taps)) == 0, _lib.last_error()
    assert taps.value == T
    return np.array(left), np.array(count), np.array(w, dtype=F).reshape(L, cap), T


@pytest.mark.parametrize("sigma", [0.0625, 0.25, 0.5, 1, 2.5, 32])
def test_axis_plan_equals_the_model_bitwise(sigma):
    lib = _lib.load()
    for L in (1, 2, 3, 7, 64, 300):
        left, count, w, T = lib_axis(lib, L, sigma)
        ml, mc, mw = bm.axis_weights(L, sigma)
        assert T == mw.shape[1] == mc.max()
        assert np.array_equal(left, ml) and np.array_equal(count, mc), (L, sigma)
        assert np.array_equal(w[:, :T].view(np.uint32), mw.view(np.uint32)), (L, sigma)
        assert (w[:, T:] == 0).all()
        for o in range(L):
            assert (w[o, count[o]:] == 0).all() and (w[o, :count[o]] > 0).all()
        assert (left >= 0).all() and (left + count <= L).all() and (count >= 1).all()
        if sigma <= 0.25:  # one tap of weight 1.0: the identity
            assert T == 1 and np.array_equal(left, np.arange(L)) and (w[:, 0] == 1.0).all()
    # an axis shorter than the window: both clamps act, every output reads the whole axis
    left, count, w, T = lib_axis(lib, 3, 32)
    assert T == 3 and (left == 0).all() and (count == 3).all()
    # the widest window of all
    left, count, w, T = lib_axis(lib, 300, 32)
    assert T == 129 and left[150] == 150 - 64 and count[150] == 129
    # a buffer too narrow is refused, with the taps reported
    taps = ctypes.c_uint32()
    buf = (ctypes.c_int32 * 7)()
    assert lib.ik_blur_axis_plan(7, 1.0, buf, buf, (ctypes.c_float * 28)(), 4, ctypes.byref(taps)) == IK_ERR_INVALID
    assert taps.value == 5
    for bad in (0.0, 0.06, 32.5, -1.0, float("nan"), float("inf")):
        assert lib.ik_blur_axis_plan(7, bad, None, None, None, 0, ctypes.byref(taps)) == IK_ERR_INVALID, bad
    assert lib.ik_blur_axis_plan(0, 1.0, None, None, None, 0, ctypes.byref(taps)) == IK_ERR_INVALID


def test_model_self_checks():
    rng = np.random.default_rng(0xB1)
    for dtype, M in ((np.uint8, 255), (np.uint16, 65535)):
        for sigma in (0.0625, 0.25):  # the identity
            img = rng.integers(0, M + 1, (9, 11, 3)).astype(dtype)
            assert np.array_equal(bm.blur(img, sigma), img)
            assert np.array_equal(bm.unsharpen(img, sigma, 0), img)
        for v in (0, 1, M // 2, M - 1, M):
            # normalised weights sum to 1 within a few ulp, far from a half: a constant stays
            img = np.full((7, 20, 2), v, dtype)
            for sigma in (0.5, 1, 2.5, 32):
                assert np.array_equal(bm.blur(img, sigma), img), (v, sigma)
        # the unsharpen rule at |d| == threshold (untouched) and threshold + 1, and its clamps
        S = np.array([100, 100, 100, 100, 0, M, 5, M - 5], dtype)
        B = np.array([90, 89, 110, 111, 50, M - 50, 40, M - 40], dtype)
        got = bm.unsharpen_rule(S, B, 10, M)
        assert got.tolist() == [100, 111, 100, 89, 0, M, 0, M]
        assert bm.unsharpen_rule(S, B, M, M).tolist() == S.tolist()  # a threshold at M never triggers
        assert bm.unsharpen_rule(S, B, 0, M).tolist() == [110, 111, 90, 89, 0, M, 0, M]
        # a checkerboard of 0 and M drives both clamps through the whole chain
        yy, xx = np.mgrid[0:12, 0:13]
        cb = (((yy + xx) & 1) * M).astype(dtype)
        sharp = bm.unsharpen(cb, 1.0, 0)
        assert np.array_equal(sharp, cb)  # 0 - d clamps to 0, M + d to M
        b = bm.blur(cb, 1.0)
        assert 0 < b.min() and b.max() < M
    # channels are independent: a 2-channel image equals its channels filtered alone
    img = rng.integers(0, 256, (10, 9, 2)).astype(np.uint8)
    both = bm.blur(img, 1.5)
    for c in range(2):
        assert np.array_equal(both[..., c], bm.blur(img[..., c], 1.5))


def test_python_argument_forms():
    assert ctypes.sizeof(_lib.RequestOpts2) == 24 and ctypes.sizeof(_lib.RequestOpts) == 12
    assert [f[0] for f in _lib.RequestOpts2._fields_] == ["fit", "orient", "background", "blur_sigma", "sharpen_sigma",
                                                          "sharpen_threshold"]
    assert _sigma(None) == 0.0 and _sigma(0) == 0.0 and _sigma(1) == 1.0 and _sigma(np.float32(0.0625)) == 0.0625
    assert _sigma(32) == 32.0 and _sigma(2.5) == 2.5
    for bad in (-1, 0.06, 32.0001, float("nan"), float("inf"), -float("inf"), True, "1", (1,), b"1", object()):
        with pytest.raises(ValueError):
            _sigma(bad)
    assert _sharpen(None) == (0.0, 0) and _sharpen(1.5) == (1.5, 0) and _sharpen((1, 2)) == (1.0, 2)
    assert _sharpen([2.5, 65535]) == (2.5, 65535) and _sharpen((1.0, np.int64(7))) == (1.0, 7)
    for bad in ((1, -1), (1, 65536), (1, 2.0), (1, True), (1,), (1, 2, 3), (40, 0), "1", (None, "x")):
        with pytest.raises(ValueError):
            _sharpen(bad)
    assert _filter_args(None, None) == (0.0, 0.0, 0) and _filter_args(4, None) == (4.0, 0.0, 0)
    assert _filter_args(None, (1.0, 2)) == (0.0, 1.0, 2)
    with pytest.raises(ValueError, match="together"):
        _filter_args(1.0, 1.0)
    ra = _request_opts(3, fits=[0, 1, 2], backgrounds=[None, "ffffff", 5], blurs=[None, 4, None],
                       sharpens=[(1.0, 2), None, None])
    assert ra._type_ is _lib.RequestOpts2
    assert [(r.fit, r.orient, r.background, r.blur_sigma, r.sharpen_sigma, r.sharpen_threshold) for r in ra] == [
        (0, 0, -1, 0.0, 1.0, 2), (1, 0, 0xFFFFFF, 4.0, 0.0, 0), (2, 0, 5, 0.0, 0.0, 0)]
    assert _request_opts(2, sharpens=[1, None])._type_ is _lib.RequestOpts2
    assert _request_opts(2, backgrounds=[None, 1])._type_ is _lib.RequestOpts  # without the new arguments: as before
    for kw in (dict(blurs=[1.0, -1]), dict(sharpens=[(1.0, -1), None]), dict(blurs=[1, None], sharpens=[1, None]),
               dict(blurs=["x", None])):
        with pytest.raises(ValueError):
            _request_opts(2, **kw)


def _batch_args(n, opts, opt_size, with_ticket):
    keep = [b"\x89PNG\r\n\x1a\n" + b"\0" * 32] * n
    ptrs = (ctypes.c_void_p * n)(*[ctypes.cast(ctypes.c_char_p(d), ctypes.c_void_p).value for d in keep])
    lens = (ctypes.c_size_t * n)(*[len(d) for d in keep])
    ws, hs = (ctypes.c_int64 * n)(*[8] * n), (ctypes.c_int64 * n)(*[8] * n)
    fs, qs = (ctypes.c_int * n)(*[1] * n), (ctypes.c_int * n)(*[80] * n)
    outs, olens, status = (ctypes.c_void_p * n)(), (ctypes.c_size_t * n)(), (ctypes.c_int * n)()
    ticket = ctypes.c_uint64()
    args = [ptrs, lens, n, ws, hs, opts, opt_size, fs, qs, 4, 0, outs, olens, status]
    return (args + [ctypes.byref(ticket)] if with_ticket else args), keep


BAD_FILTERS = [  # (blur sigma, sharpen sigma, threshold), a word of the message
    ((0.06, 0, 0), "blur sigma"), ((32.5, 0, 0), "blur sigma"), ((-1.0, 0, 0), "blur sigma"),
    ((float("nan"), 0, 0), "blur sigma"), ((float("inf"), 0, 0), "blur sigma"),
    ((0, 0.01, 0), "sharpen sigma"), ((0, 33.0, 0), "sharpen sigma"), ((0, -0.5, 0), "sharpen sigma"),
    ((0, float("nan"), 0), "sharpen sigma"),
    ((0, 1.0, -1), "threshold"), ((0, 1.0, 65536), "threshold"), ((0, 0, -1), "threshold"),
    ((1.0, 1.0, 0), "blur and sharpen together"),
]


def test_refusals_before_any_device_work():
    lib = _lib.load()  # loads without a GPU; none of these calls reaches one
    png = b"\x89PNG\r\n\x1a\n" + b"\0" * 32
    buf, n = _lib.u8p(), ctypes.c_size_t()

    def single(opts, opt_size):
        return lib.ik_transform_opts(png, len(png), 8, 8, 1, 80, 4, ctypes.byref(opts), opt_size, ctypes.byref(buf),
                                     ctypes.byref(n))

    # both declared sizes pass the size check (the orientation is refused after it); no other does
    assert single(_lib.RequestOpts(0, 99, -1), 12) == IK_ERR_INVALID and "unknown orientation" in _lib.last_error()
    assert single(_lib.RequestOpts2(0, 99, -1, 0, 0, 0), 24) == IK_ERR_INVALID and "unknown orientation" in _lib.last_error()
    for bad_size in (0, 8, 13, 16, 20, 28):
        assert single(_lib.RequestOpts2(0, 0, -1, 0, 0, 0), bad_size) == IK_ERR_INVALID
        assert "unknown options size" in _lib.last_error()
    for (b, s, t), word in BAD_FILTERS:
        assert single(_lib.RequestOpts2(0, 0, -1, b, s, t), 24) == IK_ERR_INVALID, (b, s, t)
        assert word in _lib.last_error(), _lib.last_error()

    entries = [(lib.ik_transform_batch_opts, False), (lib.ik_transform_batch_submit_opts, True),
               (lib.ik_transform_batch_submit_device_opts, True)]
    for fn, with_ticket in entries:
        for size, T in ((12, _lib.RequestOpts), (24, _lib.RequestOpts2)):
            # past the size check: request 1's fit is what is refused
            opts = (T * 2)()
            opts[0].background = opts[1].background = -1
            opts[1].fit = 7
            args, keep = _batch_args(2, opts, size, with_ticket)
            assert fn(*args) == IK_ERR_INVALID
            assert "request 1" in _lib.last_error() and "unknown fit" in _lib.last_error()
        for bad_size in (0, 8, 13, 16, 20, 28):
            args, keep = _batch_args(2, (_lib.RequestOpts2 * 2)(), bad_size, with_ticket)
            assert fn(*args) == IK_ERR_INVALID
            assert "unknown options size" in _lib.last_error()
        for (b, s, t), word in BAD_FILTERS:
            opts = (_lib.RequestOpts2 * 2)(_lib.RequestOpts2(0, 0, -1, 0, 1.0, 3), _lib.RequestOpts2(0, 0, -1, b, s, t))
            args, keep = _batch_args(2, opts, 24, with_ticket)
            assert fn(*args) == IK_ERR_INVALID, (b, s, t)
            assert "request 1" in _lib.last_error() and word in _lib.last_error(), _lib.last_error()
    out = ctypes.c_void_p()
    assert lib.ik_image_blur(None, 1.0, ctypes.byref(out)) == IK_ERR_INVALID
    assert lib.ik_image_unsharpen(None, 1.0, 0, ctypes.byref(out)) == IK_ERR_INVALID
    tile = (ctypes.c_int * 2)()
    assert lib.ik_blur_tile(tile) == 0 and tile[0] >= 8 and tile[1] >= 2
    c = (ctypes.c_ulonglong * 2)()
    assert lib.ik_blur_counters(c) == 0
