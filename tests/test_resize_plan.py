"""CPU: the resampler's host plan (csrc/ik_resize_plan.h) and its CPU model
(csrc/ik_resize_model.cpp, lib/libik_resizemodel.so).

1. Table invariants over a sweep of geometries and all five filters: what the
   kernels assume of their step tables, strips, periodic tables and LDS layout.
2. ikm_resize_run -- a plain walk of those tables in the kernels' order -- equals
   the oracle (image 0.25.8 imageops::resize restated) bit for bit.
3. VARIANTS: for every launchable variant of the resize kernels, a geometry that
   takes it; the search that found them; what the search could not reach.

A variant is what launch_resize's dispatch distinguishes:
  ("fused", A, R, WL)     k_resize_fused<A, R, 3, WL, .>  A = slots, R = rows
  ("periodic", A, R, WL)  k_resize_periodic<A, R, 3, WL>  A = per_A, R = per_R
  ("naive",)              k_vert_naive + k_horz_naive
"""
import numpy as np
import pytest

import ikutil
from resize_model import (FUSED, MAX_STRIP_COLS, MAX_STRIP_WEIGHTS, NAIVE, PERIODIC, ROW_WORDS, STRIP_BYTES,
                          ResizeModel, lds_idx)

NEAREST, TRIANGLE, CATMULLROM, GAUSSIAN, LANCZOS3 = range(5)
FILTERS = range(5)


@pytest.fixture(scope="module")
def model():
    return ResizeModel()


@pytest.fixture(scope="module")
def orc():
    return ikutil.Oracle()


# ---- the sweep -------------------------------------------------------------------
# every geometry of tests/test_gpu_resize.py ...
GPU_SMALL = [((64, 48), (17, 13)), ((97, 61), (32, 20)), ((256, 256), (32, 32)), ((33, 1), (7, 1)),
             ((2, 2), (200, 200)), ((40, 30), (40, 7)), ((50, 50), (51, 49)), ((1, 1), (3, 5)),
             ((300, 7), (5, 300)), ((129, 257), (64, 128))]
GPU_MEDIUM = [((800, 600), (400, 300)), ((1920, 1080), (640, 360)), ((1000, 1000), (100, 100)),
              ((2000, 2000), (431, 431)), ((640, 480), (320, 240)), ((1024, 768), (1023, 767)),
              ((333, 222), (1000, 666)), ((123, 45), (1230, 450)), ((800, 600), (1, 1)), ((5000, 8), (3, 2)),
              ((1000, 700), (125, 88)), ((1000, 704), (125, 88)), ((800, 600), (400, 300)), ((800, 600), (800, 10000))]
GPU_PERIODIC = [((2048, 1024), (256, 128)), ((1024, 1024), (256, 256)), ((640, 480), (160, 120)),
                ((96, 64), (48, 32)), ((512, 4096), (64, 512)), ((3000, 2000), (375, 250)),
                ((37, 64), (37, 8)), ((4096, 256), (512, 32)), ((300, 900), (7, 450)), ((64, 2048), (64, 256)),
                ((8, 8), (4, 4)), ((3, 16), (3, 2)), ((5, 12), (5, 3)), ((10, 6), (5, 3)), ((7, 64), (9, 16))]
HEADLINE = ((4096, 4096), (512, 512))


def _bounded():
    """... plus a bounded space of small ones: W, H <= 256 from a fixed stream, and rows
    of up to ~6200 bytes at C = 1 (wide windows, few columns per strip: where a padded
    tap reaches furthest past its strip)."""
    r = ikutil.splitmix64(0x5EED, 4 * 72).reshape(-1, 4)
    out = [((int(a % 256) + 1, int(b % 256) + 1), (int(c % 256) + 1, int(d % 256) + 1)) for a, b, c, d in r]
    out += [((256, 256), (256, 255)), ((255, 3), (256, 256)), ((256, 1), (1, 1)), ((1, 256), (1, 255)),
            ((6200, 8), (775, 8)), ((6199, 5), (2000, 3)), ((1751, 8), (5, 8)), ((1693, 8), (7, 8)),
            ((1664, 9), (4, 3)), ((1635, 8), (9, 8)), ((2048, 8), (8, 8)), ((2049, 9), (2048, 8)),
            ((1550, 16), (3100, 8)), ((1550, 40), (513, 35)), ((6200, 3), (6200, 2))]
    return out


SWEEP = GPU_SMALL + GPU_MEDIUM + GPU_PERIODIC + _bounded()
WIDE_C1_ONLY = 1551  # W above this: C = 1 alone keeps W * C within ~6200 bytes


def _gid(g):
    return f"{g[0][0]}x{g[0][1]}-{g[1][0]}x{g[1][1]}"


def _channels(W):
    return (1, 2, 3, 4) if W <= WIDE_C1_ONLY or W in (1920, 2000, 2048, 3000, 4096, 5000) else (1,)


# ---- 1. table invariants -----------------------------------------------------------
def check_fused_tables(t):
    """Per band: every output row emitted once and in order; every tap of every row once,
    with its own weight, in increasing source order; an even number of steps; at most
    `rows` rows per step; mask bits only for rows the step brings in and slots below
    `slots` that stand for rows of the band.  Returns the most steps any row took."""
    W, H, C, nw, nh, f, n = t.geom
    A, R = t.slots, t.rows
    assert A in (2, 4, 8, 16) and R in (4, 8) and R * A <= 64
    assert t.flush == 3
    assert len(t.band_step) == t.NB + 1 and t.band_step[0] == 0 and t.band_step[-1] == len(t.smask) == len(t.hdr)
    assert t.bands[0, 0] == 0 and t.bands[-1, 1] == nh and (t.bands[1:, 0] == t.bands[:-1, 1]).all()
    assert (t.bands[:, 1] > t.bands[:, 0]).all()
    most = 0
    for b, (oy0, oy1) in enumerate(t.bands):
        kb, ke = t.band_step[b], t.band_step[b + 1]
        assert (ke - kb) % 2 == 0 and ke > kb
        taps = {}
        nxt, steps_of_row = oy0, 0
        for k in range(kb, ke):
            start, cnt, emit, zero = (int(v) for v in t.hdr[k])
            m = int(t.smask[k])
            assert zero == 0 and 0 <= cnt <= R and emit in (0, 1)
            assert 0 <= start and start + cnt <= H   # rows with taps need no clamp (cnt = 0 may start at H: ld clamps)
            assert m >> (R * A) == 0
            w = t.sw[k]
            for j in range(R):
                for d in range(A):
                    if (m >> (j * A + d)) & 1:
                        assert j < cnt and nxt + d < oy1, "mask bit for a row the step does not bring in, or past the band"
                        taps.setdefault(nxt + d, []).append((start + j, w[j, d]))
                    else:
                        assert w[j, d].view(np.uint32) == 0, "weight without its mask bit"
            steps_of_row += 1
            if emit:
                assert nxt < oy1, "more emits than rows"
                got = taps.pop(nxt, [])
                l, c = int(t.ly[nxt]), int(t.cy[nxt])
                assert [s for s, _ in got] == list(range(l, l + c)), f"row {nxt}: taps out of order or not once each"
                np.testing.assert_array_equal(np.array([v for _, v in got], np.float32).view(np.uint32),
                                              t.wy[nxt, :c].view(np.uint32))
                most = max(most, steps_of_row)
                nxt, steps_of_row = nxt + 1, 0
            elif k == ke - 1:
                assert cnt == 0 and m == 0   # the padding step of an odd band
        assert nxt == oy1 and not taps
    return most


def check_periodic_tables(t):
    W, H, C, nw, nh, f, n = t.geom
    A, R, base = t.per_A, t.per_R, t.per_base
    G = 2 * A if A % 2 else A
    assert R * nh == H
    pb = t.per_bands
    assert pb[0, 0] == 0 and pb[-1, 1] == nh and (pb[1:, 0] == pb[:-1, 1]).all() and (pb[:, 1] > pb[:, 0]).all()
    h = pb[:, 1] - pb[:, 0]
    assert ((h[:-1] + A - 1) % G == 0).all(), "a band but the last sweeps a whole number of groups"
    # every step the kernel runs has its weights: t1 of the last band
    t1 = pb[:, 0] + ((h + A - 1 + G - 1) // G) * G
    assert t1.max() <= t.per_steps == t.per_w.shape[0]
    want = np.zeros_like(t.per_w)
    seen = np.zeros(t.per_w.shape, bool)
    for y in range(nh):
        for k in range(int(t.cy[y])):
            s = int(t.ly[y]) + k - base
            step, j = s // R, s % R
            e = step - y
            assert 0 <= e < A, "a real tap outside the A steps of its output row"
            assert not seen[step, e, j]
            seen[step, e, j] = True
            want[step, e, j] = t.wy[y, k]
    np.testing.assert_array_equal(t.per_w.view(np.uint32), want.view(np.uint32))


def check_strips_and_lds(t):
    W, H, C, nw, nh, f, n = t.geom
    s = t.strips
    assert s[0, 0] == 0 and s[-1, 1] == nw and (s[1:, 0] == s[:-1, 1]).all() and (s[:, 1] > s[:, 0]).all()
    cols = s[:, 1] - s[:, 0]
    assert cols.max() <= MAX_STRIP_COLS and t.max_strip_cols == (cols.max() + 3) // 4 * 4
    if t.wl:
        assert (cols * t.Tx).max() <= MAX_STRIP_WEIGHTS
    assert t.Tx % 4 == 0 and t.Tx >= t.cx.max() and t.Ty >= t.cy.max()
    F = t.flush
    sw_at = F * ROW_WORDS
    assert t.lds_words == sw_at + (t.max_strip_weights if t.wl else 0) + t.max_strip_cols + t.lds_pad
    assert t.lds_words * 4 <= 64 * 1024
    k = np.arange(t.Tx)
    phis = set()
    for ox0, ox1, sb in s:
        lx, cx = t.lx[ox0:ox1].astype(np.int64), t.cx[ox0:ox1]
        assert sb == (int(lx[0]) * C) & ~127 and sb % 128 == 0
        assert (lx * C >= sb).all() and ((lx + cx) * C - sb).max() <= STRIP_BYTES
        # every word the horizontal pass addresses -- all Tx taps, the zero-weight ones
        # too, from any of the F rows -- lies inside the launch's LDS
        if C == 3:
            phis.add(sb % 3)
            px = (lx - sb // 3)[:, None] + k[None]
            assert (px >= 0).all()
            word = 3 * px + (px >> 3) + 2
            # the taps with a weight read what row_put wrote: byte b of the strip at x = b + phi, word x + x // 24
            b = (lx[:, None] + k[None]) * 3 - sb
            x = b + sb % 3
            real = k[None] < cx[:, None]
            assert ((x + x // 24) == 3 * px + (px >> 3))[real].all()
        else:
            idx = (lx * C - sb)[:, None] + k[None] * C
            word = lds_idx(idx) + C - 1
        assert (F - 1) * ROW_WORDS + int(word.max()) < t.lds_words, "a padded tap reads past the launch's LDS"
    return phis


def check_plan(model, g, C, f, n=1):
    (W, H), (nw, nh) = g
    t = model.tables(W, H, C, nw, nh, f, n)
    np.testing.assert_array_equal(t.lx + t.cx <= W, True)
    np.testing.assert_array_equal(t.ly + t.cy <= H, True)
    if not t.slots:
        return t
    check_strips_and_lds(t)
    t.most_steps = check_fused_tables(t)
    if t.per_A:
        check_periodic_tables(t)
    return t


@pytest.mark.parametrize("g", SWEEP, ids=_gid)
def test_table_invariants(model, g):
    for f in FILTERS:
        for C in _channels(g[0][0]):
            check_plan(model, g, C, f, n=1 if (C + f) % 2 else 3)


@pytest.mark.parametrize("C", [3, 4])
@pytest.mark.parametrize("f", [TRIANGLE, LANCZOS3])
@pytest.mark.parametrize("n", [1, 64])
def test_table_invariants_headline(model, C, f, n):
    t = check_plan(model, HEADLINE, C, f, n)
    assert t.family == PERIODIC and t.lds_pad == 0


# ---- 2. the model equals the oracle -----------------------------------------------
def assert_model_exact(model, orc, W, H, C, nw, nh, f, n=1, family=-1, seed=0):
    src = ikutil.synth(W, H, C, seed=seed + W * 7 + H + C, pattern="N", alpha="random")
    # the smallest legal pitch, the padding 0xFF: the last lane's bytes past the row
    got, st = model.run(src, nw, nh, f, n=n, family=family, pitch=(W * C + 7) & ~7, fill=255)
    assert st.unwritten == 0 and st.outside == 0 and st.table_oob == 0, vars(st)
    assert st.max_word < st.lds_words and st.max_put_word < ROW_WORDS
    np.testing.assert_array_equal(got, orc.resize(src, nw, nh, f))
    return st


@pytest.mark.parametrize("g", SWEEP, ids=_gid)
def test_model_equals_oracle(model, orc, g):
    (W, H), (nw, nh) = g
    for f in FILTERS:
        for C in _channels(W):
            assert_model_exact(model, orc, W, H, C, nw, nh, f)


@pytest.mark.parametrize("C", [3, 4])
@pytest.mark.parametrize("f", [TRIANGLE, LANCZOS3])
def test_model_equals_oracle_headline(model, orc, C, f):
    (W, H), (nw, nh) = HEADLINE
    st = assert_model_exact(model, orc, W, H, C, nw, nh, f, n=64)
    assert st.family == PERIODIC


def test_model_fused_walk_of_periodic_geometries(model, orc):
    """The FMA mode and IK_RESIZE_PERIODIC=0 run periodic geometries on k_resize_fused:
    that plan's tables, walked exactly, are the oracle's too."""
    for (W, H), (nw, nh) in GPU_PERIODIC[2:4] + GPU_PERIODIC[6:7] + GPU_PERIODIC[10:]:
        for f in FILTERS:
            assert_model_exact(model, orc, W, H, 3 + f % 2, nw, nh, f, family=FUSED)


def test_model_naive_walk(model, orc):
    for f in FILTERS:
        assert_model_exact(model, orc, 97, 61, 3, 32, 20, f, family=NAIVE)


# ---- 3. the variant table ------------------------------------------------------------
FUSED_AR = [(2, 4), (2, 8), (4, 4), (4, 8), (8, 4), (8, 8), (16, 4)]
PERIODIC_AR = [(2, 2), (2, 4), (2, 8), (4, 2), (4, 4), (4, 8), (6, 2), (6, 4), (6, 8)]
ALL_VARIANTS = ([("fused", a, r, wl) for a, r in FUSED_AR for wl in (1, 0)] +
                [("periodic", a, r, wl) for a, r in PERIODIC_AR for wl in (1, 0)] + [("naive",)])
MAX_ROW_BYTES, MAX_H = 6200, 512  # the search space: W * C, nw * C <= 6200 and H, nh <= 512

# Compiled but never launched (kept, and without a test): the plan's flush depth is
# the constant 3, so no k_resize_fused<A, R, 2, ..> or <A, R, 4, ..> has a caller; and
# every compiled (A, R) has R * A <= 64, so the fused kernel's `else wt = w[...]`
# branch (a step's weights read one by one instead of up front) is dead.
NEVER_LAUNCHED = ["k_resize_fused<A, R, F=2, WL, FMA>: 7 (A, R) x 2 x 2 instances, flush is always 3",
                  "k_resize_fused<A, R, F=4, WL, FMA>: 7 (A, R) x 2 x 2 instances, flush is always 3",
                  "k_resize_fused: the R * A > 64 weight-load branch (no compiled instance has R * A > 64)"]


def variant_of(p):
    """The variant a plan summary launches in the exact mode (p.family: NAIVE / FUSED /
    PERIODIC; the other fields by ik_resize_plan_info's names)."""
    if p.family == NAIVE:
        return ("naive",)
    if p.family == PERIODIC:
        return ("periodic", p.per_A, p.per_R, int(p.wl))
    assert p.family == FUSED
    return ("fused", p.slots, p.rows, int(p.wl))


def is_multi(t, ns=None):
    """t: ResizeModel.tables.  At least two strips and two bands, the last band short and
    not a multiple of the flush depth 3."""
    if t.family == NAIVE or (ns or t.NS) < 2:
        return False
    b = t.per_bands if t.family == PERIODIC else t.bands
    h = b[:, 1] - b[:, 0]
    return len(h) >= 2 and h[-1] < h[0] and h[-1] % 3 != 0


def search_variants(model, heights, widths, filters=FILTERS, channels=(1, 2, 3, 4)):
    """Bounded search with the host plan alone.  The vertical geometry (H, nh, filter)
    decides the family and (A, R) and the bands; the horizontal one (W, nw, C, filter)
    decides WL and the strips: so the two are searched apart, joined, and every join is
    confirmed on its own plan.  heights: (H, nh) pairs; widths: (W, nw) pairs.  Returns
    {(variant, kind): (W, H, C, nw, nh, filter)}: kind "small" the smallest geometry
    (W * C * H, then the tuple) of the variant, kinds "multi3" and "multi4" the smallest
    is_multi ones at C = 3 and C = 4 ("multi": at another C)."""
    found = {}
    for f in filters:
        vert = {}   # (family, A, R, two bands) -> [(H, nh)]
        for H, nh in heights:
            p = model.plan(8, H, 1, 8, nh, f)
            two = max(p.NB, p.NBp) >= 2 and is_multi(model.tables(8, H, 1, 8, nh, f), ns=2)
            for multi in {False, two}:
                vert.setdefault((variant_of(p)[:3], multi), []).append((H, nh))
        horz = {}   # (C, WL or "naive", two strips) -> (W, nw)
        for C in channels:
            for W, nw in widths:
                if W * C > MAX_ROW_BYTES or nw * C > MAX_ROW_BYTES:
                    continue
                p = model.plan(W, 8, C, nw, 8, f)
                wl = int(p.wl) if p.slots else "naive"
                horz.setdefault((C, wl, False), (W, nw))
                if p.NS >= 2 and W * C > STRIP_BYTES:  # a seam inside the source rows, not only more than 512 columns
                    horz.setdefault((C, wl, True), (W, nw))
        for (key, multi), hs in vert.items():
            for (C, wl, two), (W, nw) in horz.items():
                if two != multi:
                    continue
                for H, nh in hs[:2]:
                    p = model.plan(W, H, C, nw, nh, f)
                    if multi and not is_multi(model.tables(W, H, C, nw, nh, f)):
                        continue
                    g = (W, H, C, nw, nh, int(f))
                    k = (variant_of(p), (f"multi{C}" if C in (3, 4) else "multi") if multi else "small")
                    if k not in found or (g[0] * g[2] * g[1], g) < (found[k][0] * found[k][2] * found[k][1], found[k]):
                        found[k] = g
    return found


def search_space():
    """The bounded space the table below was found in: every (H, nh) with H, nh <= 512,
    smallest first, and rows of up to 6200 bytes on a grid of widths."""
    heights = sorted(((H, nh) for H in range(1, MAX_H + 1) for nh in range(1, MAX_H + 1)),
                     key=lambda v: (max(v), v))
    ws = sorted(set(list(range(1, 17)) + list(range(32, MAX_ROW_BYTES + 1, 192)) + [MAX_ROW_BYTES]))
    widths = sorted(((W, nw) for W in ws for nw in ws), key=lambda v: (max(v), v))
    return heights, widths


# (variant, geometry (W, H, C, nw, nh, filter), kind): found by
# search_variants(model, *search_space()).
VARIANTS = [
    (('fused', 2, 4, 1), (1, 1, 1, 1, 1, 0), 'small'),
    (('fused', 2, 4, 1), (800, 9, 3, 6, 17, 0), 'multi3'),
    (('fused', 2, 4, 1), (608, 9, 4, 5, 17, 0), 'multi4'),
    (('fused', 2, 4, 0), (608, 1, 1, 224, 1, 3), 'small'),
    (('fused', 2, 8, 1), (1, 16, 1, 1, 3, 1), 'small'),
    (('fused', 2, 8, 1), (800, 102, 3, 2, 17, 1), 'multi3'),
    (('fused', 2, 8, 1), (608, 102, 4, 2, 17, 1), 'multi4'),
    (('fused', 2, 8, 0), (1568, 16, 1, 416, 3, 1), 'small'),
    (('fused', 2, 8, 0), (2912, 102, 1, 800, 17, 1), 'multi'),
    (('fused', 4, 4, 1), (1, 1, 1, 1, 3, 0), 'small'),
    (('fused', 4, 4, 1), (800, 5, 3, 6, 17, 0), 'multi3'),
    (('fused', 4, 4, 1), (608, 5, 4, 5, 17, 0), 'multi4'),
    (('fused', 4, 4, 0), (608, 1, 1, 224, 3, 3), 'small'),
    (('fused', 4, 4, 0), (2912, 13, 1, 800, 17, 1), 'multi'),
    (('fused', 4, 8, 1), (1, 14, 1, 1, 3, 1), 'small'),
    (('fused', 4, 8, 1), (800, 70, 3, 2, 17, 1), 'multi3'),
    (('fused', 4, 8, 1), (608, 70, 4, 2, 17, 1), 'multi4'),
    (('fused', 4, 8, 0), (800, 19, 1, 416, 4, 2), 'small'),
    (('fused', 4, 8, 0), (2912, 70, 1, 800, 17, 1), 'multi'),
    (('fused', 8, 4, 1), (1, 1, 1, 1, 5, 0), 'small'),
    (('fused', 8, 4, 1), (800, 3, 3, 6, 17, 0), 'multi3'),
    (('fused', 8, 4, 1), (608, 3, 4, 5, 17, 0), 'multi4'),
    (('fused', 8, 4, 0), (608, 1, 1, 224, 5, 3), 'small'),
    (('fused', 8, 4, 0), (992, 15, 3, 800, 17, 3), 'multi3'),
    (('fused', 8, 4, 0), (992, 15, 4, 800, 17, 3), 'multi4'),
    (('fused', 8, 8, 1), (1, 23, 1, 1, 5, 2), 'small'),
    (('fused', 8, 8, 1), (800, 70, 3, 5, 17, 2), 'multi3'),
    (('fused', 8, 8, 1), (608, 70, 4, 6, 17, 2), 'multi4'),
    (('fused', 8, 8, 0), (608, 24, 1, 224, 5, 3), 'small'),
    (('fused', 8, 8, 0), (992, 134, 3, 800, 33, 3), 'multi3'),
    (('fused', 8, 8, 0), (992, 134, 4, 800, 33, 3), 'multi4'),
    (('fused', 16, 4, 1), (1, 1, 1, 1, 9, 0), 'small'),
    (('fused', 16, 4, 1), (800, 2, 3, 6, 17, 0), 'multi3'),
    (('fused', 16, 4, 1), (608, 2, 4, 5, 17, 0), 'multi4'),
    (('fused', 16, 4, 0), (608, 1, 1, 224, 9, 3), 'small'),
    (('fused', 16, 4, 0), (992, 8, 3, 800, 17, 3), 'multi3'),
    (('fused', 16, 4, 0), (992, 8, 4, 800, 17, 3), 'multi4'),
    (('periodic', 2, 2, 1), (1, 4, 1, 1, 2, 1), 'small'),
    (('periodic', 2, 2, 1), (800, 68, 3, 2, 34, 1), 'multi3'),
    (('periodic', 2, 2, 1), (608, 68, 4, 2, 34, 1), 'multi4'),
    (('periodic', 2, 2, 0), (1568, 4, 1, 416, 2, 1), 'small'),
    (('periodic', 2, 2, 0), (2912, 68, 1, 800, 34, 1), 'multi'),
    (('periodic', 2, 4, 1), (1, 8, 1, 1, 2, 1), 'small'),
    (('periodic', 2, 4, 1), (800, 136, 3, 2, 34, 1), 'multi3'),
    (('periodic', 2, 4, 1), (608, 136, 4, 2, 34, 1), 'multi4'),
    (('periodic', 2, 4, 0), (1568, 8, 1, 416, 2, 1), 'small'),
    (('periodic', 2, 4, 0), (2912, 136, 1, 800, 34, 1), 'multi'),
    (('periodic', 2, 8, 1), (1, 16, 1, 1, 2, 1), 'small'),
    (('periodic', 2, 8, 1), (800, 272, 3, 2, 34, 1), 'multi3'),
    (('periodic', 2, 8, 1), (608, 272, 4, 2, 34, 1), 'multi4'),
    (('periodic', 2, 8, 0), (1568, 16, 1, 416, 2, 1), 'small'),
    (('periodic', 2, 8, 0), (2912, 272, 1, 800, 34, 1), 'multi'),
    (('periodic', 4, 2, 1), (1, 6, 1, 1, 3, 2), 'small'),
    (('periodic', 4, 2, 1), (800, 68, 3, 5, 34, 2), 'multi3'),
    (('periodic', 4, 2, 1), (608, 68, 4, 6, 34, 2), 'multi4'),
    (('periodic', 4, 2, 0), (800, 6, 1, 416, 3, 2), 'small'),
    (('periodic', 4, 2, 0), (2144, 68, 1, 5, 34, 2), 'multi'),
    (('periodic', 4, 4, 1), (1, 12, 1, 1, 3, 2), 'small'),
    (('periodic', 4, 4, 1), (800, 136, 3, 5, 34, 2), 'multi3'),
    (('periodic', 4, 4, 1), (608, 136, 4, 6, 34, 2), 'multi4'),
    (('periodic', 4, 4, 0), (800, 12, 1, 416, 3, 2), 'small'),
    (('periodic', 4, 4, 0), (2144, 136, 1, 5, 34, 2), 'multi'),
    (('periodic', 4, 8, 1), (1, 24, 1, 1, 3, 2), 'small'),
    (('periodic', 4, 8, 1), (800, 272, 3, 5, 34, 2), 'multi3'),
    (('periodic', 4, 8, 1), (608, 272, 4, 6, 34, 2), 'multi4'),
    (('periodic', 4, 8, 0), (800, 24, 1, 416, 3, 2), 'small'),
    (('periodic', 4, 8, 0), (2144, 272, 1, 5, 34, 2), 'multi'),
    (('periodic', 6, 2, 1), (1, 8, 1, 1, 4, 3), 'small'),
    (('periodic', 6, 2, 1), (800, 76, 3, 8, 38, 3), 'multi3'),
    (('periodic', 6, 2, 1), (608, 76, 4, 8, 38, 3), 'multi4'),
    (('periodic', 6, 2, 0), (608, 8, 1, 224, 4, 3), 'small'),
    (('periodic', 6, 2, 0), (992, 76, 3, 800, 38, 3), 'multi3'),
    (('periodic', 6, 2, 0), (992, 76, 4, 800, 38, 3), 'multi4'),
    (('periodic', 6, 4, 1), (1, 16, 1, 1, 4, 3), 'small'),
    (('periodic', 6, 4, 1), (800, 152, 3, 8, 38, 3), 'multi3'),
    (('periodic', 6, 4, 1), (608, 152, 4, 8, 38, 3), 'multi4'),
    (('periodic', 6, 4, 0), (608, 16, 1, 224, 4, 3), 'small'),
    (('periodic', 6, 4, 0), (992, 152, 3, 800, 38, 3), 'multi3'),
    (('periodic', 6, 4, 0), (992, 152, 4, 800, 38, 3), 'multi4'),
    (('periodic', 6, 8, 1), (1, 32, 1, 1, 4, 3), 'small'),
    (('periodic', 6, 8, 1), (800, 304, 3, 8, 38, 3), 'multi3'),
    (('periodic', 6, 8, 1), (608, 304, 4, 8, 38, 3), 'multi4'),
    (('periodic', 6, 8, 0), (608, 32, 1, 224, 4, 3), 'small'),
    (('periodic', 6, 8, 0), (992, 304, 3, 800, 38, 3), 'multi3'),
    (('periodic', 6, 8, 0), (992, 304, 4, 800, 38, 3), 'multi4'),
    (('naive',), (1, 1, 1, 1, 17, 0), 'small'),
]
# Variants no geometry of the search space reaches: none.
# Without a "multi" geometry.  The search is a heuristic over its space (widths on a grid,
# the first horizontal hit per (C, WL), two heights per vertical key), so its silence
# proves nothing; the argument does.  naive has no strips or bands.  fused (2, 4, WL=0)
# with more than two output rows needs at most two rows open at once and at most four new
# source rows per output row: that is Nearest, whose Tx is 4, so its weights always fit
# LDS (WL = 1), or a Triangle at an integer ratio, which is periodic, not fused.
NO_MULTI = [('fused', 2, 4, 0), ('naive',)]
UNREACHABLE = []


def test_variants_table(model):
    """Each entry's plan is the variant it names; every launchable variant has one."""
    phis, most_steps = set(), 0
    for variant, (W, H, C, nw, nh, f), kind in VARIANTS:
        assert W * C <= MAX_ROW_BYTES and nw * C <= MAX_ROW_BYTES and H <= MAX_H and nh <= MAX_H
        t = check_plan(model, ((W, H), (nw, nh)), C, f)
        assert variant_of(t) == variant, (variant, kind)
        if kind != "small":
            assert is_multi(t) and W * C > STRIP_BYTES
            if C == 3:
                phis |= {int(sb) % 3 for sb in t.strips[:, 2]}
        if t.family != NAIVE:
            most_steps = max(most_steps, t.most_steps)
    named = {v for v, _, _ in VARIANTS}
    assert named | set(UNREACHABLE) == set(ALL_VARIANTS) and not named & set(UNREACHABLE)
    assert {v for v, _, k in VARIANTS if k != "small"} | set(NO_MULTI) == named
    assert phis == {0, 1, 2}, "the RGB strips of the table start at every phase of a pixel"
    assert most_steps > 1, "the chunked path: a row whose first window is longer than `rows`"
    assert any(v[0] == "fused" and v[1] == 16 for v in named)


def test_search_finds_the_table_rows(model):
    """The search itself, on a corner of its space: what it returns there is in the table
    or no smaller than the table's entry."""
    heights = [(H, nh) for H in range(1, 17) for nh in range(1, 6)]
    widths = [(W, nw) for W in (1, 608, 800) for nw in (1, 224, 416)]
    found = search_variants(model, heights, widths, channels=(1,))
    small = {v: g for v, g, k in VARIANTS if k == "small"}
    assert found
    for (v, kind), g in found.items():
        p = model.plan(*g)
        assert variant_of(p) == v
        if kind == "small":
            assert (small[v][0] * small[v][2] * small[v][1], small[v]) <= (g[0] * g[2] * g[1], g)


@pytest.mark.parametrize("entry", VARIANTS, ids=lambda e: "-".join(map(str, e[0])) + "-" + e[2])
def test_model_equals_oracle_on_variants(model, orc, entry):
    variant, (W, H, C, nw, nh, f), kind = entry
    for n in (1, 3):
        st = assert_model_exact(model, orc, W, H, C, nw, nh, f, n=n)
        assert st.family == {"naive": NAIVE, "fused": FUSED, "periodic": PERIODIC}[variant[0]]
    if variant[0] == "periodic":
        assert_model_exact(model, orc, W, H, C, nw, nh, f, family=FUSED)
