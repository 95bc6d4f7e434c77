"""CPU: the watermark overlay's host half.  ik_overlay_place against tests/overlay_model.py
case by case; the model's own properties (the definition of DESIGN section 4); the third
options layout's size; the bindings; and every refusal of an overlay field, which the
library makes before any device work, so that it can be seen here, without a device."""
import ctypes
from fractions import Fraction

import numpy as np
import pytest

import overlay_model as om
from imagekit import DynamicImage, Gravity, Overlay, _lib
from imagekit.transform import _overlays, _request_opts

IK_ERR_INVALID = 2


def lib_place(lib, W, H, wo, ho, g, dx, dy, tile):
    out = (ctypes.c_int32 * 6)()
    assert lib.ik_overlay_place(W, H, wo, ho, g, dx, dy, int(tile), out) == 0, _lib.last_error()
    return tuple(out)


PLACE_CASES = (
    # (W, H, wo, ho, dx, dy, tile)
    [(40, 30, 7, 5, 0, 0, False), (41, 31, 8, 4, 0, 0, False)]             # odd and even W - wo, H - ho
    + [(40, 30, 8, 5, 0, 0, False), (41, 30, 8, 5, 3, -2, False)]
    + [(10, 30, 17, 5, 0, 0, False), (40, 6, 7, 13, 0, 0, False)]          # wider, taller than the base
    + [(10, 6, 17, 13, 0, 0, False), (10, 6, 18, 12, 1, 1, False)]         # both; odd and even negative W - wo
    + [(40, 30, 9, 7, -36, 0, False), (40, 30, 9, 7, 36, 0, False)]        # clipped left, right (from some gravities)
    + [(40, 30, 9, 7, 0, -27, False), (40, 30, 9, 7, 0, 27, False)]        # top, bottom
    + [(40, 30, 9, 7, -49, 0, False), (40, 30, 9, 7, 49, 0, False)]        # emptied on each side
    + [(40, 30, 9, 7, 0, -37, False), (40, 30, 9, 7, 0, 37, False)]
    + [(40, 30, 9, 7, 1 << 24, -(1 << 24), False)]
    + [(67, 21, 5, 3, -2, 1, True), (67, 21, 5, 3, -33, -50, True), (4, 4, 9, 9, -5, -5, True)]  # tile, negative origin
)


def test_place_equals_the_model():
    lib = _lib.load()
    seen_empty = seen_clip = 0
    for W, H, wo, ho, dx, dy, tile in PLACE_CASES:
        for g in om.GRAVITIES:
            want = om.place(W, H, wo, ho, g, dx, dy, tile)
            assert lib_place(lib, W, H, wo, ho, g, dx, dy, tile) == want, (W, H, wo, ho, g, dx, dy, tile)
            seen_empty += want[2] == 0
            seen_clip += 0 < want[2] < min(wo, W) or 0 < want[3] < min(ho, H)
    assert seen_empty and seen_clip
    # the nine origins by hand, W - wo = 33 (odd), H - ho = 26 (even)
    want = {om.CENTER: (16, 13), om.N: (16, 0), om.S: (16, 26), om.E: (33, 13), om.W: (0, 13), om.NE: (33, 0),
            om.NW: (0, 0), om.SE: (33, 26), om.SW: (0, 26)}
    for g, (x0, y0) in want.items():
        assert lib_place(lib, 40, 31, 7, 5, g, 0, 0, False) == (x0, y0, 7, 5, x0, y0)
        assert int(Gravity(g)) == g
    # a wider overlay gets a negative origin, floored towards minus infinity: (10 - 17) / 2 -> -4
    assert lib_place(lib, 10, 30, 17, 5, om.CENTER, 0, 0, False) == (0, 12, 10, 5, -4, 12)
    assert lib_place(lib, 10, 30, 17, 5, om.CENTER, 0, 0, True) == (0, 0, 10, 30, -4, 12)
    assert lib_place(lib, 0, 5, 3, 3, om.CENTER, 0, 0, True)[:4] == (0, 0, 0, 0)
    out = (ctypes.c_int32 * 6)()
    for bad in ((40, 30, 0, 5, 0, 0, 0, 0), (40, 30, 5, 0, 0, 0, 0, 0), (40, 30, 5, 5, 9, 0, 0, 0),
                (40, 30, 5, 5, -1, 0, 0, 0), (40, 30, 5, 5, 0, (1 << 24) + 1, 0, 0), (40, 30, 5, 5, 0, 0, -(1 << 24) - 1, 0),
                (40, 30, 5, 5, 0, 0, 0, 2), ((1 << 24) + 1, 30, 5, 5, 0, 0, 0, 0), (40, 30, 5, (1 << 24) + 1, 0, 0, 0, 0)):
        assert lib.ik_overlay_place(*bad, out) == IK_ERR_INVALID, bad
    assert lib.ik_overlay_place(40, 30, 5, 5, 0, 0, 0, 0, None) == IK_ERR_INVALID


@pytest.mark.parametrize("depth", [1, 2])
def test_model_properties(depth):
    M = 256 ** depth - 1
    dt = np.uint8 if depth == 1 else np.uint16
    if depth == 1:
        v = np.arange(256, dtype=np.uint64)
    else:
        v = np.unique(np.concatenate([[0, 1, 2, 127, 128, 255, 256, 257, 32767, 32768, 65534, 65535],
                                      np.random.default_rng(5).integers(0, 65536, 84)])).astype(np.uint64)
    f, a, c = np.meshgrid(v, v, v, indexing="ij")
    # a = 0 leaves the base; a = M on an opaque base gives f
    zero, full = np.zeros_like(v), np.full_like(v, M)
    assert np.array_equal(om.blend_opaque(c[:, 0], f[:, 0], np.uint64(0), depth), c[:, 0])
    assert np.array_equal(om.blend_opaque(c[:, 0], f[:, 0], np.uint64(M), depth), f[:, 0])
    for ca in (zero[0], v[len(v) // 2], full[0]):
        oc, oa = om.blend_alpha(c[:, 0, :, None], np.full(c[:, 0].shape, ca), f[:, 0, :, None], np.zeros_like(c[:, 0]), depth)
        assert np.array_equal(oc[..., 0], c[:, 0]) and (oa == ca).all()
    oc, oa = om.blend_alpha(c[:, 0, :, None], np.full(c[:, 0].shape, np.uint64(M)), f[:, 0, :, None],
                            np.full(c[:, 0].shape, np.uint64(M)), depth)
    assert np.array_equal(oc[..., 0], f[:, 0]) and (oa == M).all()
    # rule 5 with ca = M is rule 4, over the whole grid
    oc, oa = om.blend_alpha(c[..., None], np.full(c.shape, np.uint64(M)), f[..., None], a, depth)
    assert np.array_equal(oc[..., 0], om.blend_opaque(c, f, a, depth)) and (oa == M).all()
    # rule 4 is the integer nearest to the exact quotient (M is odd: no ties), on a sample
    r4 = om.blend_opaque(c, f, a, depth)
    pick = np.random.default_rng(9).integers(0, len(v), (4000, 3))
    for i, j, k in pick:
        fi, ai, ci = int(v[i]), int(v[j]), int(v[k])
        exact = Fraction(fi * ai + ci * (M - ai), M)
        got = int(r4[i, j, k])
        assert abs(exact - got) < Fraction(1, 2), (fi, ai, ci, got)
    # rule 5's outputs stay samples, and the alpha never falls below either side's
    ca = c
    oc, oa = om.blend_alpha(np.full(c.shape + (1,), np.uint64(M)), ca, f[..., None], a, depth)
    assert oc.max() <= M and oa.max() <= M and (oa >= np.maximum(a, ca)).all()
    # rules 1-3
    assert om.effective_alpha(M, 255, depth) == M and om.effective_alpha(0, 255, depth) == 0
    assert om.effective_alpha(M, 1, depth) == (1 if depth == 1 else 257)
    assert om.to_depth(np.uint64(255), 1, 2) == 65535 and om.to_depth(np.uint64(65535), 2, 1) == 255
    assert om.to_depth(np.uint64(128), 2, 1) == 0 and om.to_depth(np.uint64(129), 2, 1) == 1
    white = np.full((1, 1, 3), M, dt)
    fl, fa = om.overlay_samples(white, 1, depth)
    assert fl[0, 0, 0] == M and fa[0, 0] == M  # the luma weights sum to 10000
    fl, _ = om.overlay_samples(np.array([[[M, 0, 0]]], dt), 2, depth)
    assert fl[0, 0, 0] == 2126 * M // 10000


def test_model_overlay_places_and_tiles():
    B = np.random.default_rng(1).integers(0, 256, (21, 67, 3)).astype(np.uint8)
    O = np.random.default_rng(2).integers(0, 256, (3, 5, 3)).astype(np.uint8)
    got = om.overlay(B, O, om.SE)
    assert np.array_equal(got[18:, 62:], O) and np.array_equal(got[:18], B[:18]) and np.array_equal(got[:, :62], B[:, :62])
    t = om.overlay(B, O, om.NW, -2, 1, tile=True)
    for y in range(21):
        for x in range(67):
            assert np.array_equal(t[y, x], O[(y - 1) % 3, (x + 2) % 5])
    assert np.array_equal(om.overlay(B, O, om.E, 5, 0), B)  # an empty window
    # a 16-bit RGBA overlay on an 8-bit gray base: depth, luma, alpha, opacity in that order
    O16 = np.array([[[65535, 0, 0, 32768]]], np.uint16)
    g = om.overlay(np.full((1, 1, 1), 10, np.uint8), O16, om.CENTER, opacity=128)
    a = (128 * 128 + 127) // 255
    assert g[0, 0, 0] == ((2126 * 255 // 10000) * a + 10 * (255 - a) + 127) // 255


def test_layout_and_bindings():
    lib = _lib.load()
    assert ctypes.sizeof(_lib.RequestOpts3) == 56
    assert _lib.RequestOpts3.overlay.offset == 24 and _lib.RequestOpts3.reserved.offset == 52
    names = {n for n, _, _ in _lib.SIGNATURES}
    for fn in ("ik_overlay_place", "ik_image_overlay", "ik_overlay_batch_device", "ik_overlay_span",
               "ik_overlay_counters"):
        assert fn in names and hasattr(lib, fn)
    assert lib.ik_overlay_span() >= 16
    c = (ctypes.c_ulonglong * 2)()
    assert lib.ik_overlay_counters(c) == 0 and lib.ik_overlay_counters(None) == IK_ERR_INVALID
    out = ctypes.c_void_p()
    assert lib.ik_image_overlay(None, None, 0, 0, 0, 255, 0, ctypes.byref(out)) == IK_ERR_INVALID


def test_python_arguments():
    mark = DynamicImage(0)  # a null handle: nothing here reaches the library
    o = Overlay(mark, "se", -3, 4, 200, True)
    assert (o.gravity, o.dx, o.dy, o.opacity, o.tile) == (Gravity.se, -3, 4, 200, True)
    assert Overlay(mark, 6).gravity is Gravity.nw and Overlay(mark).opacity == 255
    for kw in (dict(gravity="up"), dict(gravity=9), dict(dx=1.5), dict(dy=(1 << 24) + 1), dict(opacity=0),
               dict(opacity=256), dict(opacity=True), dict(tile=1)):
        with pytest.raises(ValueError):
            Overlay(mark, **kw)
    with pytest.raises(ValueError):
        Overlay("logo.png")
    assert _overlays(None, 3) is None and _overlays([None, None], 2) is None
    assert _overlays(o, 3) == [o, o, o] and _overlays([o], 2) == [o, o]
    assert _overlays(mark, 2)[1].image is mark
    with pytest.raises(Exception):
        _overlays([o, o], 3)
    ra = _request_opts(3, blurs=[None, 2.0, None], overlays=[o, None, mark])
    assert ra._type_ is _lib.RequestOpts3
    assert [(r.overlay, r.overlay_gravity, r.overlay_dx, r.overlay_dy, r.overlay_opacity, r.overlay_tile, r.reserved)
            for r in ra] == [(None, 7, -3, 4, 200, 1, 0), (None, 0, 0, 0, 0, 0, 0), (None, 0, 0, 0, 255, 0, 0)]
    assert ra[1].blur_sigma == 2.0 and ra[0].background == -1
    # without an overlay: the layouts of before
    assert _request_opts(2, blurs=[1, None])._type_ is _lib.RequestOpts2
    assert _request_opts(2, backgrounds=[None, 1], overlays=[None, None])._type_ is _lib.RequestOpts


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


HANDLE = 0x1000  # never dereferenced: every case below is refused before the overlay is looked at
BAD_OVERLAYS = [  # (overlay, gravity, dx, dy, opacity, tile, reserved), a word of the message
    ((HANDLE, 9, 0, 0, 255, 0, 0), "gravity"), ((HANDLE, -1, 0, 0, 255, 0, 0), "gravity"),
    ((HANDLE, 0, 0, 0, 256, 0, 0), "opacity"), ((HANDLE, 0, 0, 0, -1, 0, 0), "opacity"),
    ((HANDLE, 0, 0, 0, 255, 2, 0), "tile"), ((HANDLE, 0, 0, 0, 255, -1, 0), "tile"),
    ((HANDLE, 0, 0, 0, 255, 0, 1), "reserved"), ((None, 0, 0, 0, 0, 0, 7), "reserved"),
    ((HANDLE, 0, (1 << 24) + 1, 0, 255, 0, 0), "offset"), ((HANDLE, 0, 0, -(1 << 24) - 1, 255, 0, 0), "offset"),
    ((None, 3, 0, 0, 0, 0, 0), "without an overlay"), ((None, 0, 1, 0, 0, 0, 0), "without an overlay"),
    ((None, 0, 0, -1, 0, 0, 0), "without an overlay"), ((None, 0, 0, 0, 255, 0, 0), "without an overlay"),
    ((None, 0, 0, 0, 0, 1, 0), "without an overlay"),
]


def opts3(ov=(None, 0, 0, 0, 0, 0, 0), fit=0, orient=0):
    return _lib.RequestOpts3(fit, orient, -1, 0, 0, 0, *ov)


def test_refusals_before_any_device_work():
    lib = _lib.load()  # loads without a GPU; none of these calls reaches one
    png = b"\x89PNG\r\n\x1a\n" + b"\0" * 32
    buf, n = _lib.u8p(), ctypes.c_size_t()

    def single(opts, opt_size):
        return lib.ik_transform_opts(png, len(png), 8, 8, 1, 80, 4, ctypes.byref(opts), opt_size, ctypes.byref(buf),
                                     ctypes.byref(n))

    # the third size passes the size check (the orientation is refused after it); its neighbours do not
    assert single(opts3(orient=99), 56) == IK_ERR_INVALID and "unknown orientation" in _lib.last_error()
    for bad_size in (32, 48, 52, 55, 57, 60, 64):
        assert single(opts3(), bad_size) == IK_ERR_INVALID and "unknown options size" in _lib.last_error()
    for ov, word in BAD_OVERLAYS:
        assert single(opts3(ov), 56) == IK_ERR_INVALID, ov
        assert word in _lib.last_error(), _lib.last_error()
    entries = [(lib.ik_transform_batch_opts, False), (lib.ik_transform_batch_submit_opts, True),
               (lib.ik_transform_batch_submit_device_opts, True)]
    for fn, with_ticket in entries:
        opts = (_lib.RequestOpts3 * 2)(opts3(), opts3(fit=7))  # past the size check: request 1's fit
        args, keep = _batch_args(2, opts, 56, with_ticket)
        assert fn(*args) == IK_ERR_INVALID
        assert "request 1" in _lib.last_error() and "unknown fit" in _lib.last_error()
        for bad_size in (48, 57, 64):
            args, keep = _batch_args(2, (_lib.RequestOpts3 * 2)(), bad_size, with_ticket)
            assert fn(*args) == IK_ERR_INVALID and "unknown options size" in _lib.last_error()
        for ov, word in BAD_OVERLAYS:
            opts = (_lib.RequestOpts3 * 2)(opts3(), opts3(ov))
            args, keep = _batch_args(2, opts, 56, with_ticket)
            assert fn(*args) == IK_ERR_INVALID, ov
            assert "request 1" in _lib.last_error() and word in _lib.last_error(), _lib.last_error()
