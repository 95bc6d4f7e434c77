"""CPU: fit=cover / fit=exact without a device -- ik_fit_target against the oracle's
resize_dimensions and the crop rule, the windowed resize plan's tables against the whole
virtual plan's rows, the CPU model's walk of them against the oracle's crop, and
ik_post_plan_fit's grouping by the whole window."""
import ctypes

import numpy as np
import pytest

import ikutil
from imagekit import _lib
from resize_model import FUSED, NAIVE, PERIODIC
from resize_window_model import (CASES, CONTAIN, COVER, EXACT, LANCZOS3, NAMED, TRIANGLE, U32, WindowModel,
                                 fit_reference, oracle_window)
from test_resize_plan import SWEEP, _channels, _gid

STRIP_BYTES = 2048


@pytest.fixture(scope="module")
def model():
    return WindowModel()


@pytest.fixture(scope="module")
def orc():
    return ikutil.Oracle()


def fit_target(W, H, w, h, fit):
    out = (ctypes.c_uint32 * 6)()
    rc = _lib.load().ik_fit_target(W, H, -1 if w is None else w, -1 if h is None else h, fit, out)
    return rc, tuple(out)


# ---- 1. ik_fit_target -------------------------------------------------------------------
FIT_SWEEP = [
    # (W, H, w, h): column crops, row crops, odd (iw - nw) and (ih - nh), one-pixel sides
    (4096, 2304, 512, 512), (2304, 4096, 512, 512), (200, 60, 50, 40), (60, 200, 40, 50), (640, 480, 100, 100),
    (480, 640, 100, 100), (641, 479, 100, 99), (479, 641, 99, 100), (1001, 333, 77, 50), (333, 1001, 50, 77),
    (100, 50, 50, 50), (50, 100, 50, 50), (7, 5, 3, 3), (5, 7, 3, 3), (1, 1, 1, 1), (1, 1, 9, 4), (9, 4, 1, 1),
    (1, 4000, 4000, 8), (4000, 1, 8, 4000), (3, 2, 1, 1000), (640, 480, 640, 480), (640, 480, 0, 0), (640, 480, 0, 7),
    (640, 480, 7, 0), (17, 13, 17, 1), (17, 13, 1, 13), (1000, 1000, 333, 334), (1000, 1000, 334, 333),
    (65535, 3, 2, 65535), (123, 457, 1000, 1000),
    # one side None: nothing to crop
    (640, 480, 100, None), (640, 480, None, 100), (479, 641, 99, None), (1, 4000, None, 8), (4000, 1, 8, None),
]


@pytest.mark.parametrize("g", FIT_SWEEP, ids=lambda g: "x".join(str(v) for v in g))
def test_fit_target_sweep(orc, g):
    W, H, w, h = g
    for fit in (CONTAIN, COVER, EXACT):
        want = fit_reference(orc, W, H, w, h, fit)
        rc, got = fit_target(W, H, w, h, fit)
        assert rc == 0 and got == want, (fit, got, want)
        iw, ih, x0, y0, nw, nh = got
        assert nw >= 1 and nh >= 1 and x0 + nw <= iw and y0 + nh <= ih
    if w is not None and h is not None:
        iw, ih, x0, y0, nw, nh = fit_target(W, H, w, h, COVER)[1]
        tw, th = max(w, 1), max(h, 1)
        assert (nw, nh) == (tw, th)               # the virtual image covers the target
        assert x0 == 0 or y0 == 0                 # cropped along one axis only
        assert (x0, y0) == ((iw - tw) // 2, (ih - th) // 2)
    # CONTAIN is resize_image's size
    assert fit_target(W, H, w, h, CONTAIN)[1][4:] == orc.resize_image_dims(W, H, w, h)


def test_fit_target_crop_directions_and_odd_margins():
    assert fit_target(4096, 2304, 512, 512, COVER) == (0, (910, 512, 199, 0, 512, 512))   # columns, (910 - 512) / 2
    assert fit_target(2304, 4096, 512, 512, COVER) == (0, (512, 910, 0, 199, 512, 512))   # rows
    assert fit_target(641, 479, 100, 99, COVER) == (0, (132, 99, 16, 0, 100, 99))         # odd iw - nw = 32 -> 16
    assert fit_target(200, 60, 50, 40, COVER) == (0, (133, 40, 41, 0, 50, 40))            # odd margin 83 -> 41
    assert fit_target(1, 4000, 4000, 8, COVER) == (0, (4000, 16000000, 0, 7999996, 4000, 8))
    assert fit_target(640, 480, 0, 0, COVER) == (0, (1, 1, 0, 0, 1, 1))                   # Some(0) -> 1
    assert fit_target(640, 480, 100, 100, EXACT) == (0, (100, 100, 0, 0, 100, 100))
    assert fit_target(640, 480, 100, 100, CONTAIN) == (0, (100, 75, 0, 0, 100, 75))


def test_fit_target_errors():
    lib = _lib.load()
    out = (ctypes.c_uint32 * 6)()
    # the virtual side above u32: 3 x 2 covering 1 x U32 is 6442450942 x U32
    assert fit_reference(ikutil.Oracle(), 3, 2, 1, U32, COVER) is None
    assert lib.ik_fit_target(3, 2, 1, U32, COVER, out) == 2 and "overflow" in _lib.last_error()
    assert lib.ik_fit_target(3, 2, 1, U32, EXACT, out) == 0 and tuple(out)[4:] == (1, U32)
    assert lib.ik_fit_target(3, 2, U32 + 1, 1, COVER, out) == 2 and "u32" in _lib.last_error()
    assert lib.ik_fit_target(3, 2, 1, 1, 3, out) == 2       # no such fit
    assert lib.ik_fit_target(3, 2, -1, -1, COVER, out) == 2  # both None: the caller returns the input
    assert lib.ik_fit_target(3, 2, 1, 1, COVER, None) == 2


# ---- 2. windowed tables -----------------------------------------------------------------
@pytest.mark.parametrize("g", SWEEP, ids=_gid)
def test_full_window_tables_are_todays(model, g):
    """A full window reproduces the whole resize's tables and summary byte for byte."""
    (W, H), (nw, nh) = g
    for C in _channels(W):
        for f in (TRIANGLE, LANCZOS3):
            for n in (1, 64):
                a = model.plan(W, H, C, nw, nh, f, n)
                b = model.plan_window(W, H, C, (nw, nh, 0, 0, nw, nh), f, n)
                a.geom = b.geom = None
                assert a == b
                for x, y in zip(model.raw_tables(W, H, C, nw, nh, f, n),
                                model.raw_tables_window(W, H, C, (nw, nh, 0, 0, nw, nh), f, n)):
                    assert x.dtype == y.dtype and x.tobytes() == y.tobytes()


def check_window_tables(model, W, H, C, win, f, n=1):
    iw, ih, x0, y0, nw, nh = win
    t = model.tables_window(W, H, C, win, f, n)
    v = model.tables(W, H, C, iw, ih, f, 1)     # the whole virtual plan
    # the window's rows of the virtual tables (the tap stride may be narrower: the rest is zero)
    for (l, c, w, T), (vl, vc, vw, o0, cnt) in (((t.lx, t.cx, t.wx, t.Tx), (v.lx, v.cx, v.wx, x0, nw)),
                                                 ((t.ly, t.cy, t.wy, t.Ty), (v.ly, v.cy, v.wy, y0, nh))):
        assert len(l) == len(c) == cnt and w.shape == (cnt, T)
        np.testing.assert_array_equal(l, vl[o0:o0 + cnt])
        np.testing.assert_array_equal(c, vc[o0:o0 + cnt])
        assert T <= vw.shape[1] and T % 4 == 0 and T >= c.max()
        assert w.tobytes() == np.ascontiguousarray(vw[o0:o0 + cnt, :T]).tobytes()
        assert not vw[o0:o0 + cnt, T:].any()
    if t.slots:
        lo, hi = (int(t.lx[0]) * C) & ~127, int(t.lx[-1] + t.cx[-1]) * C
        assert t.strips[0, 0] == 0 and t.strips[-1, 1] == nw
        for ox0, ox1, sb in t.strips:
            need = int((t.lx[ox0:ox1] + t.cx[ox0:ox1]).max()) * C
            assert lo <= sb and sb % 128 == 0 and sb <= int(t.lx[ox0]) * C   # starts inside the window's bytes
            assert need - sb <= STRIP_BYTES and need <= hi                   # and what it needs ends inside them
        r0, r1 = int(t.ly[0]), int(t.ly[-1] + t.cy[-1])
        assert t.bands[0, 0] == 0 and t.bands[-1, 1] == nh
        for start, count, emit, _ in t.hdr:
            assert r0 <= start and start + count <= r1
        for (oy0, oy1) in t.bands:
            assert r0 <= t.ly[oy0] and t.ly[oy1 - 1] + t.cy[oy1 - 1] <= r1
        if t.per_A:
            assert H % ih == 0 and t.per_R == H // ih                       # the virtual ratio, not H / nh
            A, R = t.per_A, t.per_R
            pw = t.per_w.reshape(-1, A, R)
            for s in range(pw.shape[0]):                                    # a weighted row is a row of the window
                for e in range(A):
                    for j in range(R):
                        if pw[s, e, j] != 0:
                            assert r0 <= R * s + t.per_base + j < r1
            for y in range(nh):                                             # every output's taps are in the sweep
                for k in range(t.cy[y]):
                    s, j = divmod(int(t.ly[y]) + k - t.per_base, R)
                    assert 0 <= s - y < A and pw[s, s - y, j] == t.wy[y, k]
    return t


@pytest.mark.parametrize("c", CASES, ids=lambda c: c.name)
def test_cover_window_tables(model, orc, c):
    win = fit_reference(orc, c.W, c.H, c.tw, c.th, COVER)
    t = check_window_tables(model, c.W, c.H, c.C, win, c.f, c.n)
    assert t.family == c.family
    # what the named cases are for
    if c.name.startswith("rgba-mid-strip"):
        assert (int(t.lx[0]) * 4) % 128 != 0 and t.NS >= 2
    if c.name.startswith("rgb-odd-origin"):
        ox0, _, sb = t.strips[0]
        assert (int(t.lx[ox0]) - sb // 3) % 8 != 0
        assert sb % 3 == {"phi2": 2, "phi1": 1, "periodic": 0}[c.name.rsplit("-", 1)[1]]
    if c.name == "periodic-row":
        assert win[3] == 32 and t.per_R == 2
    if c.name == "periodic-row-odd-y0":
        assert win[3] % 2 == 1


def test_window_tables_headline(model, orc):
    """4096 x 2304 -> cover 512 x 512: the strips span the window's source columns only."""
    win = fit_reference(orc, 4096, 2304, 512, 512, COVER)
    assert win == (910, 512, 199, 0, 512, 512)
    for f in (TRIANGLE, LANCZOS3):
        t = check_window_tables(model, 4096, 2304, 4, win, f, 64)
        whole = model.plan(4096, 2304, 4, 910, 512, f, 64)
        assert t.family == whole.family == FUSED
        assert t.NS * 910 <= whole.NS * 512 + 910   # strips in proportion to the kept columns, plus a halo strip


# ---- 3. table size ----------------------------------------------------------------------
def test_table_size_follows_the_window(model, orc):
    """1 x 4000 -> cover 4000 x 8: the virtual height is 16,000,000 and the plan has eight
    rows, which are sample.rs's weights of rows 7999996..8000003 (restated for those rows)."""
    win = fit_reference(orc, 1, 4000, 4000, 8, COVER)
    assert win == (4000, 16000000, 0, 7999996, 4000, 8)
    t = model.tables_window(1, 4000, 1, win, TRIANGLE)
    assert len(t.ly) == len(t.cy) == 8 and t.wy.shape[0] == 8 and len(t.lx) == 4000
    F = np.float32
    ratio = F(4000) / F(16000000)
    for r in range(8):
        c = (F(7999996 + r) + F(0.5)) * ratio          # upscale: sratio = 1, support = 1
        left = min(max(int(np.floor(c - F(1))), 0), 3999)
        right = min(max(int(np.ceil(c + F(1))), left + 1), 4000)
        c = c - F(0.5)
        w = [max(F(1) - abs(F(i) - c), F(0)) for i in range(left, right)]
        s = F(0)
        for x in w:
            s = F(s + x)
        assert (t.ly[r], t.cy[r]) == (left, right - left)
        np.testing.assert_array_equal(t.wy[r, :right - left], np.array([F(x / s) for x in w], F))
    out, st = model.run_window(np.arange(4000, dtype=np.uint8).reshape(4000, 1, 1), win, TRIANGLE)
    assert (st.unwritten, st.outside, st.table_oob, st.unwritten_out) == (0, 0, 0, 0) and out.shape == (8, 4000, 1)
    assert (out == out[:, :1]).all() and 2000 % 256 - 1 <= out[0, 0, 0] <= 2000 % 256


# ---- 4. the CPU model's walk ------------------------------------------------------------
@pytest.mark.parametrize("c", CASES, ids=lambda c: c.name)
def test_model_walk_equals_the_oracle_crop(model, orc, c):
    win = fit_reference(orc, c.W, c.H, c.tw, c.th, COVER)
    src = ikutil.synth(c.W, c.H, c.C, seed=c.W + c.C, pattern="N", alpha="random")
    want = oracle_window(orc, src, win, c.f)
    families = [-1] + ([FUSED] if c.family == PERIODIC else [])   # the fused kernel also walks periodic plans
    for fam in families:
        got, st = model.run_window(src, win, c.f, n=c.n, family=fam)
        assert st.family == (c.family if fam < 0 else fam)
        assert (st.unwritten, st.outside, st.table_oob, st.unwritten_out) == (0, 0, 0, 0)
        np.testing.assert_array_equal(got, want)
    if c.family != NAIVE:                                          # FMA mode: the fused kernel, within 1 LSB
        got, st = model.run_window(src, win, c.f, n=c.n, fma=True, family=FUSED)
        assert (st.unwritten, st.outside, st.table_oob, st.unwritten_out) == (0, 0, 0, 0)
        assert np.abs(got.astype(int) - want.astype(int)).max() <= 1


# ---- 5. ik_post_plan_fit ----------------------------------------------------------------
JPEG, WEBP = 0, 1
AUTO, MIX_HOST = 3, 0


def post_plan(reqs, fits=None, enc=AUTO, mix=MIX_HOST):
    """reqs: (W, H, w, h, fmt) -> per-request (size, resize group, coder group, route, window)."""
    lib, m = _lib.load(), len(reqs)

    def arr(ct, vals):
        return (ct * m)(*vals)

    nw, nh = (ctypes.c_uint32 * m)(), (ctypes.c_uint32 * m)()
    rg, cg, route = (ctypes.c_int * m)(), (ctypes.c_int * m)(), (ctypes.c_int * m)()
    info, win = (ctypes.c_uint32 * 4)(), (ctypes.c_uint32 * (6 * m))()
    head = [m, arr(ctypes.c_int, [1] * m), arr(ctypes.c_uint32, [r[0] for r in reqs]),
            arr(ctypes.c_uint32, [r[1] for r in reqs]), arr(ctypes.c_uint32, [3] * m),
            arr(ctypes.c_uint64, [(r[0] * 3 + 255) & ~255 for r in reqs]), arr(ctypes.c_int, [0] * m),
            arr(ctypes.c_uint32, [1] * m), arr(ctypes.c_int64, [-1 if r[2] is None else r[2] for r in reqs]),
            arr(ctypes.c_int64, [-1 if r[3] is None else r[3] for r in reqs])]
    tail = [arr(ctypes.c_int, [r[4] for r in reqs]), arr(ctypes.c_int, [80] * m), enc, mix, nw, nh, rg, cg, route, info]
    if fits == "plain":
        assert lib.ik_post_plan(*head, *tail) == 0
        return list(zip(zip(nw, nh), rg, cg, route)), tuple(info)
    fa = None if fits is None else arr(ctypes.c_int, fits)
    assert lib.ik_post_plan_fit(*head, fa, *tail, win) == 0
    wins = [tuple(win[6 * k:6 * k + 6]) for k in range(m)]
    return list(zip(zip(nw, nh), rg, cg, route)), tuple(info), wins


def test_post_plan_fit_groups_by_the_whole_window(orc):
    # the same (W, H, nw, nh) four ways: exact, cover, and two cover windows that differ only in
    # where they sit cannot exist for one (W, H), so a second source size supplies the third group
    reqs = [(400, 300, 100, 100, WEBP)] * 6
    fits = [EXACT, COVER, EXACT, COVER, CONTAIN, CONTAIN]
    plan, info, wins = post_plan(reqs, fits)
    for k, f in enumerate(fits):
        assert wins[k] == fit_reference(orc, 400, 300, 100, 100, f)
        assert plan[k][0] == wins[k][4:]
    rg = [p[1] for p in plan]
    assert rg[0] == rg[2] and rg[1] == rg[3] and rg[4] == rg[5] and len({rg[0], rg[1], rg[4]}) == 3 and min(rg) >= 0
    assert plan[0][0] == plan[1][0] == (100, 100) and plan[4][0] == (100, 75)
    assert info[2] == 3
    # coder groups stay inside their resize group
    assert len({p[2] for p in plan}) == 3


def test_post_plan_fit_cover_crop_without_resampling_joins_no_group():
    # 100 x 50 -> cover 50 x 50: the virtual image is the image, only the crop is left
    plan, info, wins = post_plan([(100, 50, 50, 50, JPEG)] * 3, [COVER] * 3)
    assert wins[0] == (100, 50, 25, 0, 50, 50) and [p[1] for p in plan] == [-1] * 3 and info[2] == 0


def test_post_plan_fit_all_contain_is_post_plan():
    reqs = [(640, 480, 100, None, WEBP), (640, 480, 100, 100, WEBP), (640, 480, 100, 75, JPEG), (640, 480, None, None, JPEG),
            (320, 200, 100, 100, WEBP), (320, 200, 100, 100, WEBP), (640, 480, U32 + 1, 1, WEBP)] * 6
    plain = post_plan(reqs, "plain")
    for fits in (None, [CONTAIN] * len(reqs)):
        got = post_plan(reqs, fits)
        assert got[:2] == plain
        for (size, *_), w in zip(got[0], got[2]):
            assert w == ((size[0], size[1], 0, 0) + size if size != (0, 0) else (0,) * 6)
    # and a bad fit is refused
    lib = _lib.load()
    one = lambda ct, v: (ct * 1)(v)  # noqa: E731
    out = [(ctypes.c_uint32 * 1)(), (ctypes.c_uint32 * 1)(), (ctypes.c_int * 1)(), (ctypes.c_int * 1)(),
           (ctypes.c_int * 1)(), (ctypes.c_uint32 * 4)()]
    assert lib.ik_post_plan_fit(1, one(ctypes.c_int, 1), one(ctypes.c_uint32, 8), one(ctypes.c_uint32, 8),
                                one(ctypes.c_uint32, 3), one(ctypes.c_uint64, 256), one(ctypes.c_int, 0),
                                one(ctypes.c_uint32, 1), one(ctypes.c_int64, 4), one(ctypes.c_int64, 4),
                                one(ctypes.c_int, 7), one(ctypes.c_int, WEBP), one(ctypes.c_int, 80), AUTO, MIX_HOST,
                                *out, None) == 2


# ---- the plan's summary through the C ABI -------------------------------------------------
@pytest.mark.parametrize("c", NAMED, ids=lambda c: c.name)
def test_plan_info_window_matches_the_model(model, orc, c):
    win = fit_reference(orc, c.W, c.H, c.tw, c.th, COVER)
    out = (ctypes.c_int32 * 13)()
    assert _lib.load().ik_resize_plan_info_window(c.W, c.H, c.C, *win, int(c.f), c.n, out, 13) == 13
    p = model.plan_window(c.W, c.H, c.C, win, c.f, c.n)
    assert list(out)[:12] == [p.slots, p.rows, p.flush, p.wl, p.NS, p.NB, p.per_A, p.per_R, p.NBp, p.Tx, p.Ty,
                              p.max_strip_cols]
    assert out[12] == c.family
    # a window outside the virtual image is refused
    assert _lib.load().ik_resize_plan_info_window(c.W, c.H, c.C, win[0], win[1], win[2] + 1, win[3],
                                                  win[0] - win[2], win[5], int(c.f), 1, out, 13) < 0
