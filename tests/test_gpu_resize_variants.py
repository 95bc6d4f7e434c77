"""GPU: the resampler pinned variant by variant (tests/test_resize_plan.py VARIANTS),
with hostile source and destination padding, content aimed at the clamp and at
single weights, and the FMA mode on the fused variants.  Every launch goes through
ik_resize_batch_device; ik_resize_plan_info says which kernel variant it takes, so
no case can drift onto another kernel unnoticed.  Pixels: equal to the oracle
(image 0.25.8 imageops::resize restated), bit for bit."""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest

import ikutil
from resize_model import FUSED, INFO, NAIVE, PERIODIC, ResizeModel
from test_resize_plan import (CATMULLROM, GAUSSIAN, LANCZOS3, NEAREST, TRIANGLE, VARIANTS, variant_of)

pytestmark = pytest.mark.gpu
IK_RESIZE_EXACT, IK_RESIZE_FMA = 0, 1
POISON = 0xA5


def plan_info(ik, W, H, C, nw, nh, f, n):
    out = (ctypes.c_int32 * 13)()
    assert ik.ik_resize_plan_info(W, H, C, nw, nh, int(f), n, out, 13) == 13
    p = SimpleNamespace(**dict(zip(INFO + ["family"], out)))
    p.grid = 0 if p.family == NAIVE else p.NS * (p.NBp if p.family == PERIODIC else p.NB) * n
    return p


def roundup(v, m):
    return (v + m - 1) // m * m


def device_resize(ik, imgs, nw, nh, f, pitch=None, gap=0, dst_pitch=None, dst_gap=0, fill=0):
    """imgs (n, H, W, C) through ik_resize_batch_device.  Source rows `pitch` apart, images
    pitch * H + gap apart, padding and gaps filled with `fill` (a byte, or "noise");
    destination prefilled with POISON, rows dst_pitch apart, images dst_pitch * nh +
    dst_gap apart.  Returns the (n, nh, nw, C) pixels after checking that no byte outside
    them changed."""
    n, H, W, C = imgs.shape
    pitch = pitch or roundup(W * C, 8)
    dst_pitch = dst_pitch or nw * C
    stride, dstride = pitch * H + gap, dst_pitch * nh + dst_gap
    if isinstance(fill, str):
        src = (ikutil.splitmix64(77, n * stride) & np.uint64(255)).astype(np.uint8)
    else:
        src = np.full(n * stride, fill, np.uint8)
    for i in range(n):
        rows = src[i * stride:i * stride + pitch * H].reshape(H, pitch)
        rows[:, :W * C] = imgs[i].reshape(H, W * C)
    dst = np.full(n * dstride, POISON, np.uint8)
    d_src, d_dst = ctypes.c_void_p(), ctypes.c_void_p()
    assert ik.ik_dev_alloc(src.nbytes, ctypes.byref(d_src)) == 0
    assert ik.ik_dev_alloc(dst.nbytes, ctypes.byref(d_dst)) == 0
    try:
        assert ik.ik_memcpy_h2d(d_src, src.ctypes.data, src.nbytes) == 0
        assert ik.ik_memcpy_h2d(d_dst, dst.ctypes.data, dst.nbytes) == 0
        assert ik.ik_resize_batch_device(d_src, W, H, C, pitch, stride, n, nw, nh, int(f), d_dst, dst_pitch, dstride,
                                         None) == 0
        assert ik.ik_dev_synchronize() == 0
        assert ik.ik_memcpy_d2h(dst.ctypes.data, d_dst, dst.nbytes) == 0
    finally:
        ik.ik_dev_free(d_src)
        ik.ik_dev_free(d_dst)
    out = np.zeros((n, nh, nw, C), np.uint8)
    keep = np.ones(dst.size, bool)
    for i in range(n):
        rows = dst[i * dstride:i * dstride + dst_pitch * nh].reshape(nh, dst_pitch)
        out[i] = rows[:, :nw * C].reshape(nh, nw, C)
        k = keep[i * dstride:i * dstride + dst_pitch * nh].reshape(nh, dst_pitch)
        k[:, :nw * C] = False
    assert (dst[keep] == POISON).all(), "a store outside the output rows"
    return out


def noise(n, W, H, C, seed):
    return np.stack([ikutil.synth(W, H, C, seed=seed + i, pattern="N", alpha="random") for i in range(n)])


def check_exact(ik, oracle, imgs, nw, nh, f, **kw):
    got = device_resize(ik, imgs, nw, nh, f, **kw)
    for i in range(len(imgs)):
        np.testing.assert_array_equal(got[i], oracle.resize(imgs[i], nw, nh, int(f)))


def _vid(e):
    v, g, kind = e
    return "-".join(str(x) for x in v) + f"-{kind}-" + "x".join(str(x) for x in g)


# ---- every variant -------------------------------------------------------------------
@pytest.mark.parametrize("entry", VARIANTS, ids=_vid)
def test_variant_exact(ik, oracle, entry):
    """The named geometry at its own C (the exact variant asserted), and at C = 4 and 3,
    n = 1 and n = 3.  C moves only the strips and WL, so the other C keep the family, A
    and R -- unless one output column's window (up to 2048 bytes at the named C) no
    longer fits a strip at a larger C: the plan then has no slots and the launch is the
    two-pass fallback, which is asserted and compared like the rest.  That happens to 18
    (entry, C) pairs, all "multi" entries with two to eight output columns: the multi3
    entries of fused (2,8,1) (4,8,1) (8,8,1) and of periodic (2,*,1) (4,*,1) (6,*,1) at
    C = 4, and the C = 1 multi entries of periodic (4,*,0) at C = 3 and 4."""
    variant, (W, H, C0, nw, nh, f), kind = entry
    for C in dict.fromkeys((C0, 4, 3)):
        for n in (1, 3):
            p = plan_info(ik, W, H, C, nw, nh, f, n)
            if C == C0:
                assert variant_of(p) == variant
            elif p.slots == 0:
                assert C > C0 and variant_of(p) == ("naive",)
            else:
                assert variant_of(p)[:3] == variant[:3]
            check_exact(ik, oracle, noise(n, W, H, C, seed=W + H + C), nw, nh, f, fill=0xFF)


# Geometries whose padded zero-weight taps read furthest: an edge column with a short
# window under a long Tx (the plan's lds_pad > 0: without it, and without the kernels
# zeroing it, those taps leave the launch's LDS), and strips narrower than the widest
# (the unused tails of the LDS weights and offsets, which the kernels zero).
LDS_EDGE = [((1751, 8, 1, 5, 8, GAUSSIAN), ("fused", 8, 4, 0), True),
            ((1693, 8, 1, 7, 8, LANCZOS3), ("fused", 8, 4, 0), True),
            ((1664, 9, 1, 4, 3, CATMULLROM), ("fused", 4, 4, 0), True),
            ((1100, 45, 4, 1000, 40, LANCZOS3), ("fused", 8, 4, 1), False),
            ((2000, 20, 3, 130, 9, LANCZOS3), ("fused", 8, 4, 1), False),
            ((700, 20, 4, 90, 10, LANCZOS3), ("periodic", 6, 2, 1), False)]


@pytest.mark.parametrize("g,variant,padded", LDS_EDGE, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_lds_pad_and_short_strips(ik, oracle, g, variant, padded):
    W, H, C, nw, nh, f = g
    n = 2
    assert variant_of(plan_info(ik, W, H, C, nw, nh, f, n)) == variant
    t = ResizeModel().tables(W, H, C, nw, nh, f, n)
    cols = t.strips[:, 1] - t.strips[:, 0]
    if padded:
        assert t.lds_pad > 0
    else:
        assert t.wl and t.lds_pad == 0 and cols[-1] + 4 <= cols.max()   # a short last strip, weights in LDS
    # twice: the second launch meets whatever the first left in LDS
    for seed in (1, 2):
        check_exact(ik, oracle, noise(n, W, H, C, seed=seed), nw, nh, f, fill=0xFF)


GRIDS = (1, 2, 7, 8, 9, 17)


@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("periodic", [False, True])
def test_grid_sizes(ik, oracle, grid, periodic):
    """The XCD-aware tile order L = x * per + min(x, rem) + h / 8 with per = 0 (grids below
    8), rem = 0 and rem != 0: NS * NB * n workgroups for each of GRIDS, on both kernels."""
    for nh in range(1, 640):
        for n in (1, 3):
            g = (40, 2 * nh + (0 if periodic else 1), 4, 20, nh, TRIANGLE)
            p = plan_info(ik, *g, n)
            if p.grid == grid and p.family == (PERIODIC if periodic else FUSED):
                W, H, C, nw, nh, f = g
                check_exact(ik, oracle, noise(n, W, H, C, seed=grid), nw, nh, f)
                return
    pytest.fail(f"no geometry with {grid} workgroups")


# ---- hostile padding -------------------------------------------------------------------
def _by_family(C):
    """One single-strip and one multi-strip geometry per kernel family for this C, and the
    variant each takes (rows of 6200 bytes keep WL = 1 at every C but 1)."""
    single = {FUSED: ((97, 61, C, 32, 20, LANCZOS3), ("fused", 8, 4, 1)),
              PERIODIC: ((96, 64, C, 48, 32, LANCZOS3), ("periodic", 6, 2, 1)),
              NAIVE: ((3, 40, C, 3, 700, NEAREST), ("naive",))}
    multi = {FUSED: ((6200 // C, 45, C, 401, 23, CATMULLROM), ("fused", 8, 4, 0 if C == 1 else 1)),
             PERIODIC: ((6200 // C, 80, C, 300, 40, TRIANGLE), ("periodic", 2, 2, 1)),
             NAIVE: ((6200 // C, 12, C, 310, 400, NEAREST), ("naive",))}
    return single, multi


@pytest.mark.parametrize("C", [1, 2, 3, 4])
@pytest.mark.parametrize("family", [FUSED, PERIODIC, NAIVE], ids=["fused", "periodic", "naive"])
@pytest.mark.parametrize("strips", ["single", "multi"])
def test_hostile_padding(ik, oracle, C, family, strips):
    (W, H, C, nw, nh, f), variant = _by_family(C)[strips == "multi"][family]
    n = 2
    p = plan_info(ik, W, H, C, nw, nh, f, n)
    assert p.family == family and variant_of(p) == variant
    if family != NAIVE:
        assert (p.NS >= 2) == (strips == "multi")
    imgs = noise(n, W, H, C, seed=5 * C + family)
    tight = roundup(W * C, 8)
    odd_dst = nw * C + 4                              # not a multiple of 4 for C = 1 and C = 3
    if C in (1, 3):
        odd_dst = nw * C + (1 if (nw * C + 1) % 4 else 2)
    assert C not in (1, 3) or odd_dst % 4
    # the smallest legal pitch, images exactly pitch * H apart, destination rows exactly nw * C
    check_exact(ik, oracle, imgs, nw, nh, f, pitch=tight, gap=0, dst_pitch=nw * C, dst_gap=0, fill=0xFF)
    check_exact(ik, oracle, imgs, nw, nh, f, pitch=tight, gap=0, dst_pitch=odd_dst, dst_gap=4, fill="noise")
    # slack in the rows and between the images
    check_exact(ik, oracle, imgs, nw, nh, f, pitch=tight + 40, gap=24, dst_pitch=odd_dst, dst_gap=8, fill=0xFF)
    check_exact(ik, oracle, imgs, nw, nh, f, pitch=tight + 40, gap=24, dst_pitch=nw * C + 64, dst_gap=0, fill="noise")


# ---- content -------------------------------------------------------------------
# (W, H, vertical ratio) -> (1000, 40): a slight horizontal downscale, where Lanczos3 and
# CatmullRom overshoot on fine patterns; several strips at C = 3 and 4, two bands
# the two-pass fallback: the same rows upscaled 12 -> 200, where more than 16 output rows are open at once
CONTENT_GEOMS = {FUSED: (1100, 45, 1), PERIODIC: (1100, 80, 2), NAIVE: (1100, 12, 1)}
CONTENT_OUT = {FUSED: (1000, 40), PERIODIC: (1000, 40), NAIVE: (1000, 200)}
CONTENT_VARIANTS = {(FUSED, LANCZOS3): ("fused", 8, 4, 1), (FUSED, CATMULLROM): ("fused", 8, 4, 1),
                    (FUSED, TRIANGLE): ("fused", 4, 4, 1), (PERIODIC, LANCZOS3): ("periodic", 6, 2, 1),
                    (PERIODIC, CATMULLROM): ("periodic", 4, 2, 1), (PERIODIC, TRIANGLE): ("periodic", 2, 2, 1),
                    (NAIVE, LANCZOS3): ("naive",), (NAIVE, CATMULLROM): ("naive",), (NAIVE, TRIANGLE): ("naive",)}


def contents(W, H, C, vr, seam_x, seam_y):
    """vr: the vertical ratio.  Checker cells and stripes are 2 px wide and 2 * vr rows
    tall: at one pixel the Lanczos3 output of these geometries stays within 34..221 (the
    pattern sits at the filter's cut-off); at two it rings past both ends of the clamp."""
    yy, xx = np.mgrid[0:H, 0:W]
    yc, xx = yy // (2 * vr), xx // 2

    def rep(a):
        return np.repeat(a[..., None], C, -1).astype(np.uint8)
    out = {"black": np.zeros((H, W, C), np.uint8), "white": np.full((H, W, C), 255, np.uint8),
           "checker": rep(((xx + yc) & 1) * 255), "stripes-x": rep((xx & 1) * 255), "stripes-y": rep((yc & 1) * 255),
           "per-channel": np.broadcast_to(np.array([10, 80, 160, 250], np.uint8)[:C], (H, W, C)).copy(),
           "noise": ikutil.synth(W, H, C, seed=9, pattern="N", alpha="random")}
    spots = {"interior": (W // 3 + 1, H // 3 + 1), "strip-seam": (seam_x, H // 2), "band-seam": (W // 2, seam_y)}
    for name, (x, y) in spots.items():
        a = np.zeros((H, W, C), np.uint8)
        a[y, x] = 255
        out["impulse-" + name] = a
        out["hole-" + name] = 255 - a
    return out


@pytest.mark.parametrize("C", [4, 3])
@pytest.mark.parametrize("family", [FUSED, PERIODIC, NAIVE], ids=["fused", "periodic", "naive"])
@pytest.mark.parametrize("f", [LANCZOS3, CATMULLROM, TRIANGLE])
def test_content(ik, oracle, C, family, f):
    (W, H, vr), (nw, nh) = CONTENT_GEOMS[family], CONTENT_OUT[family]
    t = ResizeModel().tables(W, H, C, nw, nh, f, 3)
    p = plan_info(ik, W, H, C, nw, nh, f, 3)
    assert p.family == family and variant_of(p) == CONTENT_VARIANTS[family, f]
    if family == NAIVE:
        seam_x, seam_y = 256, H - 1          # no strips or bands: a 256-lane block edge, the last row
    else:
        assert p.NS >= 2
        bands = t.per_bands if family == PERIODIC else t.bands
        assert len(bands) >= 2
        seam_x = int(t.lx[t.strips[1, 0]]) + 1   # a source column that the first two strips both read
        seam_y = int(t.ly[bands[1, 0]]) + 1      # a source row that the first two bands both read
    cs = contents(W, H, C, vr, seam_x, seam_y)
    for m in ("checker", "stripes-x", "stripes-y"):
        # precondition, on the oracle alone: Lanczos3 overshoots to both sides of the clamp
        o = oracle.resize(cs[m], nw, nh, LANCZOS3)
        assert o.min() == 0 and o.max() == 255, m
    names = list(cs)
    for k in range(0, len(names), 3):
        group = names[k:k + 3]
        while len(group) < 3:
            group.append(names[0])
        got = device_resize(ik, np.stack([cs[m] for m in group]), nw, nh, f, fill=0xFF)
        for i, m in enumerate(group):
            np.testing.assert_array_equal(got[i], oracle.resize(cs[m], nw, nh, f), err_msg=m)


@pytest.mark.parametrize("C", [4, 3])
@pytest.mark.parametrize("ratio", [2, 4])
def test_triangle_integer_ratio_half_way(ik, oracle, C, ratio):
    """Triangle at exactly 2:1 and 4:1: the sums are multiples of 1/8, so half-way cases
    of the final round are common."""
    nw, nh = 150, 33
    imgs = noise(2, nw * ratio, nh * ratio, C, seed=ratio)
    assert plan_info(ik, nw * ratio, nh * ratio, C, nw, nh, TRIANGLE, 2).family == PERIODIC
    check_exact(ik, oracle, imgs, nw, nh, TRIANGLE, fill=0xFF)


# ---- FMA mode -------------------------------------------------------------------
@pytest.fixture
def fma(ik):
    assert ik.ik_get_resize_mode() == IK_RESIZE_EXACT
    assert ik.ik_set_resize_mode(IK_RESIZE_FMA) == 0
    yield
    assert ik.ik_set_resize_mode(IK_RESIZE_EXACT) == 0


@pytest.mark.parametrize("entry", [e for e in VARIANTS if e[0][0] != "naive"], ids=_vid)
def test_variant_fma_within_one_lsb(ik, oracle, fma, entry):
    """Under FMA every fused-plan geometry, the periodic ones too, runs k_resize_fused:
    within 1 LSB of the oracle; Nearest (weights 0 and 1) exact."""
    variant, (W, H, C, nw, nh, f), kind = entry
    p = plan_info(ik, W, H, C, nw, nh, f, 2)
    assert p.family == FUSED
    imgs = noise(2, W, H, C, seed=W + nh)
    got = device_resize(ik, imgs, nw, nh, f, fill=0xFF).astype(np.int32)
    want = np.stack([oracle.resize(im, nw, nh, f) for im in imgs]).astype(np.int32)
    assert np.abs(got - want).max() <= (0 if f == NEAREST else 1)
