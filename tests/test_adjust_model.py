"""CPU: the colour adjustment's host half.  ik_adjust_plan against tests/adjust_model.py bit
for bit; the model's own properties (the definition of DESIGN section 4); its distance to the
real-number definition; the fourth options layout's size; the bindings; and every refusal of
an adjustment field, which the library makes before any device work, so that it can be seen
here, without a device."""
import ctypes
import itertools

import numpy as np
import pytest

import adjust_model as am
from imagekit import Adjust, _lib
from imagekit.transform import _adjusts, _request_opts

IK_ERR_INVALID = 2
GAMMAS = (0.0, 0.1, 0.45, 1.0, 2.2, 10.0)


def lib_plan(depth, brightness=0, contrast=0, saturation=0, hue=0, gamma=0.0, invert=0, want_table=True):
    lib = _lib.load()
    a = _lib.Adjust(brightness, contrast, saturation, hue, gamma, invert)
    t = (ctypes.c_uint16 * (256 if depth == 1 else 65536))()
    q = (ctypes.c_int32 * 9)()
    f = ctypes.c_int(-1)
    assert lib.ik_adjust_plan(ctypes.byref(a), depth, t if want_table else None, q, ctypes.byref(f)) == 0, _lib.last_error()
    return np.array(q, np.int64).reshape(3, 3), np.frombuffer(t, np.uint16).copy(), f.value


@pytest.mark.parametrize("saturation", [-100, -50, 0, 37, 100])
def test_plan_matrix_equals_the_model(saturation):
    for hue in (-360, -90, 0, 15, 75, 180, 360):
        q, _, f = lib_plan(1, saturation=saturation, hue=hue)
        mq, _, mf = am.plan(1, saturation=saturation, hue=hue)
        assert np.array_equal(q, mq), (saturation, hue, q, mq)
        assert f == mf


@pytest.mark.parametrize("depth", [1, 2])
def test_plan_table_equals_the_model(depth):
    # the 16-bit grid is thinner in (brightness, contrast): a table there is 65536 pow calls
    bc = list(itertools.product((-100, -40, 0, 25, 100), (-100, -35, 0, 60, 100))) if depth == 1 else [
        (0, 0), (25, -35), (-40, 60), (100, 100)]
    for (b, c), g, inv in itertools.product(bc, GAMMAS, (0, 1)):
        _, t, f = lib_plan(depth, brightness=b, contrast=c, gamma=g, invert=inv)
        _, mt, mf = am.plan(depth, brightness=b, contrast=c, gamma=g, invert=inv)
        assert np.array_equal(t, mt), (depth, b, c, g, inv)
        assert f == mf, (depth, b, c, g, inv)
        # the flags alone, without a table to fill
        assert lib_plan(depth, brightness=b, contrast=c, gamma=g, invert=inv, want_table=False)[2] == f


def test_matrix_properties():
    assert np.array_equal(am.matrix(-100, 0), np.array([[13933, 46871, 4732]] * 3))
    gray = np.array([0, 1, 127, 128, 254, 255, 65535], np.int64)
    for s, h in itertools.product(range(-100, 101, 10), range(-360, 361, 15)):
        q = am.matrix(s, h)
        assert np.all(q.sum(axis=1) == 65536)
        assert np.abs(q).sum(axis=1).max() * 255 + 32768 < 2 ** 31
        # gray triples are fixed points
        assert np.array_equal((q.sum(axis=1)[None, :] * gray[:, None] + 32768) >> 16, np.stack([gray] * 3, 1))
    assert np.array_equal(am.matrix(0, 0), 65536 * np.eye(3, dtype=np.int64))
    assert np.array_equal(am.matrix(0, 360), 65536 * np.eye(3, dtype=np.int64))


@pytest.mark.parametrize("depth", [1, 2])
def test_table_properties(depth):
    M = 255 if depth == 1 else 65535
    ident = np.arange(M + 1, dtype=np.uint16)
    assert am.plan(depth)[2] == 0
    assert np.array_equal(am.table(depth), ident)
    assert np.array_equal(am.table(depth, gamma=1.0), am.table(depth, gamma=0.0))
    assert np.array_equal(am.table(depth, invert=1), M - ident)
    for b, c, g in ((0, 0, 2.2), (30, -20, 0.45), (-60, 80, 0.0), (100, 100, 10.0), (-100, 0, 0.1)):
        t = am.table(depth, b, c, g, 0).astype(np.int64)
        assert np.all(np.diff(t) >= 0)
        t = am.table(depth, b, c, g, 1).astype(np.int64)
        assert np.all(np.diff(t) <= 0)
    if depth == 1:
        assert np.all(am.table(1, contrast=-100) == 128)


@pytest.mark.parametrize("depth,bound", [(1, 1), (2, 3)])
def test_distance_to_the_real_definition(depth, bound):
    """The Q16 result against floor(px . m + 0.5) clamped, in float64.  The bound follows from
    the quantisation: a row's coefficient error is at most 2^-15 in all (2^-17 for each of the
    two rounded entries, their sum for the diagonal), times M, plus the two roundings."""
    M = 255 if depth == 1 else 65535
    rng = np.random.default_rng(7)
    px = rng.integers(0, M + 1, size=(4096, 3), dtype=np.int64)
    corners = np.array(list(itertools.product((0, 1, M // 2, M - 1, M), repeat=3)), np.int64)
    px = np.concatenate([px, corners])
    worst = 0
    for s, h in itertools.product((-100, -50, 0, 37, 100), (-360, -90, 0, 15, 75, 180, 360)):
        m = np.array(am.real_matrix(s, h), np.float64)
        exact = np.clip(np.floor(px.astype(np.float64) @ m.T + 0.5), 0, M).astype(np.int64)
        q = am.matrix(s, h)
        got = np.clip((px @ q.T + 32768) >> 16, 0, M)
        worst = max(worst, int(np.abs(got - exact).max()))
    print("largest distance at depth", depth, ":", worst)
    assert worst <= bound


def test_model_apply_keeps_alpha_and_gray():
    rng = np.random.default_rng(3)
    for dt, C in itertools.product((np.uint8, np.uint16), (1, 2, 3, 4)):
        px = rng.integers(0, np.iinfo(dt).max + 1, size=(5, 7, C)).astype(dt)
        out = am.apply(px, saturation=-100, brightness=10, gamma=2.2)
        assert out.dtype == dt and out.shape == px.shape
        if C in (2, 4):
            assert np.array_equal(out[..., -1], px[..., -1])
        if C <= 2:  # the matrix is not applied
            assert np.array_equal(out[..., 0], am.table(px.dtype.itemsize, brightness=10, gamma=2.2)[px[..., 0]])
        else:       # grayscale: three equal samples
            assert np.array_equal(out[..., 0], out[..., 1]) and np.array_equal(out[..., 1], out[..., 2])
    assert np.array_equal(am.apply(px), px)


def test_layout_and_bindings():
    lib = _lib.load()
    assert ctypes.sizeof(_lib.Adjust) == 24
    assert ctypes.sizeof(_lib.RequestOpts4) == 80
    assert _lib.RequestOpts4.adjust.offset == 56 and _lib.RequestOpts4.overlay.offset == 24
    names = {n for n, _, _ in _lib.SIGNATURES}
    for fn in ("ik_adjust_plan", "ik_image_adjust", "ik_adjust_batch_device", "ik_adjust_span", "ik_adjust_counters"):
        assert fn in names and hasattr(lib, fn)
    assert lib.ik_adjust_span() >= 16
    c = (ctypes.c_ulonglong * 2)()
    assert lib.ik_adjust_counters(c) == 0 and lib.ik_adjust_counters(None) == IK_ERR_INVALID
    out = ctypes.c_void_p()
    assert lib.ik_image_adjust(None, None, ctypes.byref(out)) == IK_ERR_INVALID
    a = _lib.Adjust()
    assert lib.ik_adjust_plan(ctypes.byref(a), 3, None, None, None) == IK_ERR_INVALID
    assert lib.ik_adjust_plan(None, 1, None, None, None) == IK_ERR_INVALID
    assert lib.ik_adjust_plan(ctypes.byref(a), 1, None, None, None) == 0


def test_python_arguments():
    a = Adjust(brightness=10, contrast=-20, saturation=30, hue=-45, gamma=2.2, invert=True)
    s = a._struct()
    assert (s.brightness, s.contrast, s.saturation, s.hue, s.invert) == (10, -20, 30, -45, 1)
    assert s.gamma == np.float32(2.2)
    assert Adjust(grayscale=True).saturation == -100 and Adjust().is_none() and not Adjust(invert=True).is_none()
    for kw in (dict(brightness=101), dict(contrast=-101), dict(saturation=1.5), dict(hue=361), dict(gamma=0.05),
               dict(gamma=10.5), dict(gamma=-1), dict(gamma=float("nan")), dict(gamma=float("inf")), dict(invert=2),
               dict(brightness=True), dict(grayscale=True, saturation=5), dict(grayscale=1)):
        with pytest.raises(ValueError):
            Adjust(**kw)
    assert _adjusts(None, 3) is None and _adjusts([None, Adjust()], 2) is None
    assert _adjusts(a, 3) == [a, a, a] and _adjusts([a], 2) == [a, a]
    with pytest.raises(Exception):
        _adjusts([a, a], 3)


def test_request_opts_picks_the_layouts():
    a = Adjust(grayscale=True)
    # as before
    assert ctypes.sizeof(_request_opts(2)._type_) == 12
    assert ctypes.sizeof(_request_opts(2, backgrounds=[None, 1])._type_) == 12
    assert ctypes.sizeof(_request_opts(2, blurs=[1, None])._type_) == 24
    assert ctypes.sizeof(_request_opts(2, sharpens=[None, (1.0, 3)])._type_) == 24
    assert ctypes.sizeof(_request_opts(2, blurs=[1, None], adjusts=None)._type_) == 24
    assert ctypes.sizeof(_request_opts(2, backgrounds=[None, 1], adjusts=[None, Adjust()])._type_) == 12
    # with an adjustment
    ra = _request_opts(3, blurs=[None, 2.0, None], adjusts=[a, None, Adjust(hue=15, gamma=0.45)])
    assert ra._type_ is _lib.RequestOpts4 and ctypes.sizeof(ra._type_) == 80
    assert [(r.adjust.saturation, r.adjust.hue, r.adjust.gamma) for r in ra] == [
        (-100, 0, 0.0), (0, 0, 0.0), (0, 15, float(np.float32(0.45)))]
    assert ra[1].blur_sigma == 2.0 and ra[0].background == -1 and ra[0].overlay is None


def test_request_opts_keeps_56_for_an_overlay():
    from imagekit import DynamicImage
    mark = DynamicImage(0)  # a null handle: nothing here reaches the library
    assert ctypes.sizeof(_request_opts(2, overlays=[mark, None])._type_) == 56
    assert ctypes.sizeof(_request_opts(2, overlays=[mark, None], adjusts=[None, Adjust(invert=True)])._type_) == 80


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


BAD_ADJUSTS = [  # (brightness, contrast, saturation, hue, gamma, invert), a word of the message
    ((101, 0, 0, 0, 0.0, 0), "brightness"), ((0, -101, 0, 0, 0.0, 0), "contrast"),
    ((0, 0, 101, 0, 0.0, 0), "saturation"), ((0, 0, 0, 361, 0.0, 0), "hue"),
    ((0, 0, 0, 0, 0.05, 0), "gamma"), ((0, 0, 0, 0, 10.5, 0), "gamma"), ((0, 0, 0, 0, -1.0, 0), "gamma"),
    ((0, 0, 0, 0, float("nan"), 0), "gamma"), ((0, 0, 0, 0, float("inf"), 0), "gamma"),
    ((0, 0, 0, 0, 0.0, 2), "invert"),
]
BAD_SIZES = (68, 76, 79, 81, 84, 96)


def opts4(adj=(0, 0, 0, 0, 0.0, 0), fit=0, orient=0):
    return _lib.RequestOpts4(fit, orient, -1, 0, 0, 0, None, 0, 0, 0, 0, 0, 0, _lib.Adjust(*adj))


def test_refusals_before_any_device_work():
    lib = _lib.load()  # loads without a GPU; none of these calls reaches one
    png = b"\x89PNG\r\n\x1a\n" + b"\0" * 32
    buf, n = _lib.u8p(), ctypes.c_size_t()

    def single(opts, opt_size):
        return lib.ik_transform_opts(png, len(png), 8, 8, 1, 80, 4, ctypes.byref(opts), opt_size, ctypes.byref(buf),
                                     ctypes.byref(n))

    # the fourth size passes the size check (the orientation is refused after it); its neighbours do not
    assert single(opts4(orient=99), 80) == IK_ERR_INVALID and "unknown orientation" in _lib.last_error()
    for bad_size in BAD_SIZES:
        assert single(opts4(), bad_size) == IK_ERR_INVALID and "unknown options size" in _lib.last_error()
    for adj, word in BAD_ADJUSTS:
        assert single(opts4(adj), 80) == IK_ERR_INVALID, adj
        assert word in _lib.last_error(), _lib.last_error()
    entries = [(lib.ik_transform_batch_opts, False), (lib.ik_transform_batch_submit_opts, True),
               (lib.ik_transform_batch_submit_device_opts, True)]
    for fn, with_ticket in entries:
        opts = (_lib.RequestOpts4 * 2)(opts4(), opts4(fit=7))  # past the size check: request 1's fit
        args, keep = _batch_args(2, opts, 80, with_ticket)
        assert fn(*args) == IK_ERR_INVALID
        assert "request 1" in _lib.last_error() and "unknown fit" in _lib.last_error()
        for bad_size in BAD_SIZES:
            args, keep = _batch_args(2, (_lib.RequestOpts4 * 2)(), bad_size, with_ticket)
            assert fn(*args) == IK_ERR_INVALID and "unknown options size" in _lib.last_error()
        for adj, word in BAD_ADJUSTS:
            opts = (_lib.RequestOpts4 * 2)(opts4(), opts4(adj))
            args, keep = _batch_args(2, opts, 80, with_ticket)
            assert fn(*args) == IK_ERR_INVALID, adj
            assert "request 1" in _lib.last_error() and word in _lib.last_error(), _lib.last_error()
    # the plan call itself refuses the same fields
    for adj, word in BAD_ADJUSTS:
        a = _lib.Adjust(*adj)
        assert lib.ik_adjust_plan(ctypes.byref(a), 1, None, None, None) == IK_ERR_INVALID
        assert word in _lib.last_error()
