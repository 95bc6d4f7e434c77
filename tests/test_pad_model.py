"""CPU: the pad's host half.  ik_pad_place against tests/pad_model.py; the model's np.pad modes
against the definition's index formula; the fifth options layout's size;
the bindings; and every refusal of a pad field, which the library makes before any device
work, so that it can be seen here, without a device."""
import ctypes

import numpy as np
import pytest

import pad_model as pm
from imagekit import Pad, PadMode, _lib
from imagekit.transform import _pads, _request_opts

IK_ERR_INVALID = 2


def lib_place(w, h, width, height, gravity):
    out = (ctypes.c_int32 * 4)()
    assert _lib.load().ik_pad_place(w, h, width, height, gravity, out) == 0, _lib.last_error()
    return tuple(out)


def test_place_equals_the_model():
    for gravity in range(9):
        # odd and even margins on each axis, a canvas narrower than the image, size 0
        for (w, h) in ((5, 3), (6, 4), (1, 1)):
            for width in (0, 1, w - 1, w, w + 1, w + 2, w + 7, 1 << 24):
                for height in (0, h - 1, h, h + 1, h + 4, h + 9):
                    assert lib_place(w, h, width, height, gravity) == pm.place(w, h, width, height, gravity)
    assert lib_place(5, 3, 12, 0, pm.E) == (12, 3, 7, 0) and lib_place(5, 3, 12, 8, pm.CENTER) == (12, 8, 3, 2)
    assert lib_place(0, 0, 4, 4, pm.SE) == (4, 4, 4, 4)
    lib = _lib.load()
    out = (ctypes.c_int32 * 4)()
    for bad in ((5, 3, 8, 8, 9), (5, 3, 8, 8, -1), (5, 3, (1 << 24) + 1, 8, 0), (5, 3, 8, (1 << 24) + 1, 0),
                ((1 << 24) + 1, 3, 8, 8, 0)):
        assert lib.ik_pad_place(*bad, out) == IK_ERR_INVALID, bad
    assert lib.ik_pad_place(5, 3, 8, 8, 0, None) == IK_ERR_INVALID


@pytest.mark.parametrize("mode", [pm.EDGE, pm.MIRROR, pm.WRAP])
def test_np_pad_is_the_index_formula(mode):
    """margins of several folds on both sides, and a one-sample axis"""
    for (h, w) in ((3, 5), (1, 1), (2, 7)):
        img = np.arange(h * w * 2, dtype=np.uint16).reshape(h, w, 2)
        for gravity, width, height in ((pm.CENTER, 4 * w + 3, 3 * h + 2), (pm.SE, w + 1, h + 9), (pm.NW, 3 * w, h)):
            got = pm.pad(img, mode, gravity, width, height)
            cw, ch, x0, y0 = pm.place(w, h, width, height, gravity)
            ys = [pm.index_map(mode, y - y0, h) for y in range(ch)]
            xs = [pm.index_map(mode, x - x0, w) for x in range(cw)]
            assert np.array_equal(got, img[np.ix_(ys, xs)])


def test_colour_mode_of_the_model():
    img = np.full((2, 2, 4), 9, np.uint16)
    out = pm.pad(img, pm.COLOR, pm.NW, 3, 3, 0x102030, 128)
    assert out[2, 2].tolist() == [0x10 * 257, 0x20 * 257, 0x30 * 257, 128 * 257] and (out[:2, :2] == 9).all()
    assert pm.frame_pixel(1, 1, 0xFF8000, 7) == [(2126 * 255 + 7152 * 128) // 10000]
    assert pm.frame_pixel(2, 2, 0xFF8000, 7) == [(2126 * 65535 + 7152 * 128 * 257) // 10000, 7 * 257]
    assert pm.frame_pixel(3, 1, 0xFF8000, 7) == [255, 128, 0]


def test_sizes_and_bindings():
    lib = _lib.load()
    assert ctypes.sizeof(_lib.Pad) == 24
    assert ctypes.sizeof(_lib.RequestOpts5) == 104
    assert _lib.RequestOpts5.pad.offset == 80 and _lib.RequestOpts5.adjust.offset == 56
    assert [f[0] for f in _lib.Pad._fields_] == ["mode", "gravity", "width", "height", "color", "alpha"]
    names = {n for n, _, _ in _lib.SIGNATURES}
    for fn in ("ik_pad_place", "ik_image_pad", "ik_pad_batch_device", "ik_pad_span", "ik_pad_row_cap", "ik_pad_counters"):
        assert fn in names and hasattr(lib, fn)
    assert lib.ik_pad_span() >= 16 and lib.ik_pad_span() % 16 == 0 and lib.ik_pad_row_cap() >= 1
    c = (ctypes.c_ulonglong * 2)()
    assert lib.ik_pad_counters(c) == 0 and lib.ik_pad_counters(None) == IK_ERR_INVALID
    out = ctypes.c_void_p()
    assert lib.ik_image_pad(None, None, ctypes.byref(out)) == IK_ERR_INVALID


def test_python_arguments():
    p = Pad("mirror", "se", 10, 20, "ff8000", 7)
    s = p._struct()
    assert (s.mode, s.gravity, s.width, s.height, s.color, s.alpha) == (3, 7, 10, 20, 0xFF8000, 7)
    d = Pad()._struct()
    assert (d.mode, d.gravity, d.width, d.height, d.color, d.alpha) == (1, 0, 0, 0, 0, 255)
    assert Pad(PadMode.wrap, 4).mode == PadMode.wrap and Pad(color=(1, 2, 3)).color == 0x010203
    for kw in (dict(mode="none"), dict(mode=0), dict(mode=5), dict(gravity="up"), dict(gravity=9), dict(width=-1),
               dict(height=(1 << 24) + 1), dict(width=1.5), dict(width=True), dict(alpha=256), dict(alpha=-1),
               dict(color=1 << 24), dict(color=None)):
        with pytest.raises(ValueError):
            Pad(**kw)
    assert _pads(None, 3) is None and _pads([None, None], 2) is None
    assert _pads(p, 3) == [p, p, p] and _pads([p], 2) == [p, p] and _pads([None, p], 2) == [None, p]
    with pytest.raises(Exception):
        _pads([p, p], 3)


def test_request_opts_picks_104_only_for_a_pad():
    from imagekit import Adjust
    assert ctypes.sizeof(_request_opts(2)._type_) == 12
    assert ctypes.sizeof(_request_opts(2, blurs=[1, None], pads=None)._type_) == 24
    assert ctypes.sizeof(_request_opts(2, adjusts=[None, Adjust(invert=True)], pads=[None, None])._type_) == 80
    ra = _request_opts(3, blurs=[None, 2.0, None], pads=[Pad(color="ffffff"), None, Pad("wrap", "n", 64, 0)])
    assert ra._type_ is _lib.RequestOpts5 and ctypes.sizeof(ra._type_) == 104
    assert [(r.pad.mode, r.pad.gravity, r.pad.width, r.pad.color, r.pad.alpha) for r in ra] == [
        (1, 0, 0, 0xFFFFFF, 255), (0, 0, 0, 0, 0), (4, 1, 64, 0, 255)]
    assert ra[1].blur_sigma == 2.0 and ra[0].background == -1 and ra[0].overlay is None


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


BAD_PADS = [  # (mode, gravity, width, height, color, alpha), a word of the message
    ((5, 0, 0, 0, 0, 0), "mode"), ((-1, 0, 0, 0, 0, 0), "mode"),
    ((1, 9, 0, 0, 0, 0), "gravity"), ((2, -1, 0, 0, 0, 0), "gravity"),
    ((1, 0, -1, 0, 0, 0), "size"), ((1, 0, (1 << 24) + 1, 0, 0, 0), "size"),
    ((3, 0, 0, -1, 0, 0), "size"), ((4, 0, 0, (1 << 24) + 1, 0, 0), "size"),
    ((1, 0, 0, 0, -1, 0), "colour"), ((1, 0, 0, 0, 1 << 24, 0), "colour"),
    ((1, 0, 0, 0, 0, -1), "alpha"), ((1, 0, 0, 0, 0, 256), "alpha"),
    ((0, 1, 0, 0, 0, 0), "without a mode"), ((0, 0, 8, 0, 0, 0), "without a mode"), ((0, 0, 0, 8, 0, 0), "without a mode"),
    ((0, 0, 0, 0, 1, 0), "without a mode"), ((0, 0, 0, 0, 0, 255), "without a mode"),
]
# neighbours of 104, and every size the earlier layouts' tests pin as unknown
BAD_SIZES = (100, 103, 105, 108, 112, 0, 8, 13, 16, 20, 28, 32, 48, 52, 55, 57, 60, 64, 68, 76, 79, 81, 84, 96)


def opts5(pad=(0, 0, 0, 0, 0, 0), fit=0, orient=0):
    return _lib.RequestOpts5(fit, orient, -1, 0, 0, 0, None, 0, 0, 0, 0, 0, 0, _lib.Adjust(), _lib.Pad(*pad))


def opts4(fit=0, orient=0):
    return _lib.RequestOpts4(fit, orient, -1, 0, 0, 0, None, 0, 0, 0, 0, 0, 0, _lib.Adjust())


def test_refusals_before_any_device_work():
    lib = _lib.load()  # loads without a GPU; none of these calls reaches one
    png = b"\x89PNG\r\n\x1a\n" + b"\0" * 32
    buf, n = _lib.u8p(), ctypes.c_size_t()

    def single(opts, opt_size):
        return lib.ik_transform_opts(png, len(png), 8, 8, 1, 80, 4, ctypes.byref(opts), opt_size, ctypes.byref(buf),
                                     ctypes.byref(n))

    # a pad with mode 0 and every field 0 at size 104 gets as far as the 80-byte layout does: past
    # the size check and the pad check to the orientation, which is refused last.  So does a good pad
    assert single(opts4(orient=99), 80) == IK_ERR_INVALID and "unknown orientation" in _lib.last_error()
    assert single(opts5(orient=99), 104) == IK_ERR_INVALID and "unknown orientation" in _lib.last_error()
    assert single(opts5((3, 7, 64, 0, 0xFFFFFF, 255), orient=99), 104) == IK_ERR_INVALID
    assert "unknown orientation" in _lib.last_error()
    for bad_size in BAD_SIZES:
        assert single(opts5(), bad_size) == IK_ERR_INVALID and "unknown options size" in _lib.last_error(), bad_size
    for pad, word in BAD_PADS:
        assert single(opts5(pad), 104) == IK_ERR_INVALID, pad
        assert "pad" in _lib.last_error() and word in _lib.last_error(), _lib.last_error()
    entries = [(lib.ik_transform_batch_opts, False), (lib.ik_transform_batch_submit_opts, True),
               (lib.ik_transform_batch_submit_device_opts, True)]
    for fn, with_ticket in entries:
        for opts, size in (((_lib.RequestOpts5 * 2)(opts5(), opts5(fit=7)), 104),
                           ((_lib.RequestOpts4 * 2)(opts4(), opts4(fit=7)), 80)):  # past the checks: request 1's fit
            args, keep = _batch_args(2, opts, size, with_ticket)
            assert fn(*args) == IK_ERR_INVALID
            assert "request 1" in _lib.last_error() and "unknown fit" in _lib.last_error()
        for bad_size in BAD_SIZES:
            args, keep = _batch_args(2, (_lib.RequestOpts5 * 2)(), bad_size, with_ticket)
            assert fn(*args) == IK_ERR_INVALID and "unknown options size" in _lib.last_error(), bad_size
        for pad, word in BAD_PADS:
            opts = (_lib.RequestOpts5 * 2)(opts5((1, 0, 0, 0, 0, 0)), opts5(pad))
            args, keep = _batch_args(2, opts, 104, with_ticket)
            assert fn(*args) == IK_ERR_INVALID, pad
            assert "request 1" in _lib.last_error() and word in _lib.last_error(), _lib.last_error()
