"""CPU: the background flatten's arithmetic (tests/flatten_model.py) is the nearest integer
of the exact quotient, exhaustively at 8 bits and on the edge set and a million random
triples at 16; the channel rule; the Python argument forms; and the refusals the library
makes before any device work (no GPU here)."""
import ctypes
import itertools

import numpy as np
import pytest

import flatten_model as fm
from imagekit import _lib
from imagekit.transform import BG_NONE, _background, _request_opts

IK_ERR_INVALID = 2


def nearest(c, a, b, M):
    """floor(x + 0.5) of the float64 quotient.  The quotient's distance from a half-integer
    is at least 1 / (2 M) (7.6e-6 at 16 bits) and its float64 error below 1e-10."""
    c, a, b = (np.asarray(v, dtype=np.float64) for v in (c, a, b))
    return np.floor((c * a + b * (M - a)) / M + 0.5).astype(np.uint64)


def test_every_8_bit_triple_is_the_nearest_integer():
    c, a = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    for b in range(256):
        got = fm.blend(c, a, b, 255)
        assert np.array_equal(got, nearest(c, a, b, 255)), b
        assert np.array_equal(got[:, 0], np.full(256, b)) and np.array_equal(got[:, 255], np.arange(256))


def test_16_bit_edges_and_a_million_random_triples():
    e = np.array(list(itertools.product(fm.EDGE16, repeat=3)), dtype=np.uint64)
    assert len(e) == 13 ** 3
    assert np.array_equal(fm.blend(e[:, 0], e[:, 1], e[:, 2], 65535), nearest(e[:, 0], e[:, 1], e[:, 2], 65535))
    r = np.random.default_rng(0xF1A7).integers(0, 65536, size=(1_000_000, 3), dtype=np.uint64)
    got = fm.blend(r[:, 0], r[:, 1], r[:, 2], 65535)
    assert np.array_equal(got, nearest(r[:, 0], r[:, 1], r[:, 2], 65535))
    assert got.max() <= 65535
    # the largest numerator fits in u32, as the kernel computes it
    assert 65535 * 65535 + 32767 < 1 << 32
    assert fm.blend(5, 0, 777, 65535) == 777 and fm.blend(5, 65535, 777, 65535) == 5


def test_channel_rule():
    assert fm.out_channels(4, 0x123456) == 3 and fm.out_channels(4, 0x808080) == 3
    assert fm.out_channels(2, 0x808080) == 1 and fm.out_channels(2, 0) == 1 and fm.out_channels(2, 0xFFFFFF) == 1
    assert fm.out_channels(2, 0x808081) == 3 and fm.out_channels(2, 0x7F80FE) == 3
    assert fm.out_channels(1, 0x123456) == 1 and fm.out_channels(3, 0x123456) == 3
    assert fm.background_channels(0x7F80FE, 1) == (0x7F, 0x80, 0xFE)
    assert fm.background_channels(0x7F80FE, 2) == (0x7F7F, 0x8080, 0xFEFE)
    la = np.array([[[10, 0], [10, 255], [200, 128]]], np.uint8)
    np.testing.assert_array_equal(fm.flatten(la, 0x404040)[0, :, 0], [0x40, 10, (200 * 128 + 0x40 * 127 + 127) // 255])
    rgb = fm.flatten(la, 0xFF0000)
    assert rgb.shape == (1, 3, 3)
    np.testing.assert_array_equal(rgb[0, 0], [255, 0, 0])
    np.testing.assert_array_equal(rgb[0, 1], [10, 10, 10])  # luma replicated, as to_rgb8 replicates it
    rgba16 = np.array([[[65535, 0, 1, 0], [1, 2, 3, 65535]]], np.uint16)
    np.testing.assert_array_equal(fm.flatten(rgba16, 0x0180FF), [[[257, 0x8080, 65535], [1, 2, 3]]])
    opaque = np.arange(12, dtype=np.uint8).reshape(2, 2, 3)
    np.testing.assert_array_equal(fm.flatten(opaque, 0xABCDEF), opaque)


def test_python_argument_forms():
    assert _background(None) == BG_NONE == -1
    assert _background(0) == 0 and _background(0xFFFFFF) == 0xFFFFFF and _background(np.int64(0x7F80FE)) == 0x7F80FE
    assert _background((0x7F, 0x80, 0xFE)) == 0x7F80FE and _background([1, 2, 3]) == 0x010203
    assert _background("7f80fe") == 0x7F80FE and _background("#7F80Fe") == 0x7F80FE and _background("000000") == 0
    for bad in (-1, -2, 0x1000000, 1.5, True, "", "fff", "#fff", "7f80fg", "0x7f80f", "##7f80fe", " 7f80fe", "+7f80f",
                (1, 2), (1, 2, 3, 4), (1, 2, 256), (-1, 0, 0), (1.0, 2, 3), (True, 0, 0), b"7f80fe", object()):
        with pytest.raises(ValueError):
            _background(bad)
    ra = _request_opts(3, fits=[0, 1, 2], backgrounds=[None, "ffffff", 5])
    assert [(r.fit, r.orient, r.background) for r in ra] == [(0, 0, -1), (1, 0, 0xFFFFFF), (2, 0, 5)]
    assert ctypes.sizeof(_lib.RequestOpts) == 12
    with pytest.raises(ValueError):
        _request_opts(1, backgrounds=["white"])


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


def test_refusals_before_any_device_work():
    lib = _lib.load()  # loads without a GPU; none of these calls reaches one
    size = ctypes.sizeof(_lib.RequestOpts)
    png = b"\x89PNG\r\n\x1a\n" + b"\0" * 32
    buf, n = _lib.u8p(), ctypes.c_size_t()

    def single(opts, opt_size):
        return lib.ik_transform_opts(png, len(png), 8, 8, 1, 80, 4, ctypes.byref(opts), opt_size, ctypes.byref(buf),
                                     ctypes.byref(n))

    for bad_size in (0, size - 4, size + 4, 8, 16):
        assert single(_lib.RequestOpts(0, 0, 0xFFFFFF), bad_size) == IK_ERR_INVALID
        assert "unknown options size" in _lib.last_error()
        assert lib.ik_transform_opts(png, len(png), 8, 8, 1, 80, 4, None, bad_size, ctypes.byref(buf),
                                     ctypes.byref(n)) == IK_ERR_INVALID
        assert "unknown options size" in _lib.last_error()
    for bad_bg in (0x1000000, -2):
        assert single(_lib.RequestOpts(0, 0, bad_bg), size) == IK_ERR_INVALID
        assert "background" in _lib.last_error()

    entries = [(lib.ik_transform_batch_opts, False), (lib.ik_transform_batch_submit_opts, True),
               (lib.ik_transform_batch_submit_device_opts, True)]
    for fn, with_ticket in entries:
        good = (_lib.RequestOpts * 2)(_lib.RequestOpts(0, 0, -1), _lib.RequestOpts(1, 6, 0x102030))
        args, keep = _batch_args(2, good, size + 1, with_ticket)
        assert fn(*args) == IK_ERR_INVALID
        assert "unknown options size" in _lib.last_error()
        for bad_bg in (0x1000000, -2):
            opts = (_lib.RequestOpts * 2)(_lib.RequestOpts(0, 0, -1), _lib.RequestOpts(0, 0, bad_bg))
            args, keep = _batch_args(2, opts, size, with_ticket)
            assert fn(*args) == IK_ERR_INVALID
            assert "request 1" in _lib.last_error() and "background" in _lib.last_error()
    # IK_ORIENT_AUTO (-1) cannot be resolved for device-resident inputs: refused before anything is queued
    auto = (_lib.RequestOpts * 2)(_lib.RequestOpts(0, 6, 0xFFFFFF), _lib.RequestOpts(0, -1, 0xFFFFFF))
    args, keep = _batch_args(2, auto, size, True)
    assert lib.ik_transform_batch_submit_device_opts(*args) == IK_ERR_INVALID
    assert "IK_ORIENT_AUTO" in _lib.last_error()
