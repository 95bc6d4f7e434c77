"""GPU: the PNG unfilter kernels (ik_png.hip: k_png_unfilter, k_png_unfilter_su;
ik_unfilter.h's device branch) pinned on their predictor inputs and hand-off edges.

Every image is written by png_filter_util.py (held by test_png_filter_util.py) and
must decode bit-exactly to its source array, on the GPU path (on_gpu: no stream
may fall back to the host decoder).
  a. predictor inputs, variant by variant (diagonal kernel, word-at-a-time at 4 and
     8 bytes per pixel, byte-wise at 1, 2, 3, 6): every feasible Paeth (b - c, a - c)
     with c at both ends of its range, every (a, b) under Average, every (raw, a)
     under Sub and (raw, b) under Up -- in every byte lane of the pixel;
  b. the diagonal kernel's geometry: row chunks around the hand-off group (8) and
     the 63-step wave skew, heights around one band, two bands, one workgroup and
     two (K 1 -> 2), the last band's publish condition, rowbytes % 16 in {0, 1, 15};
  c. the band loop's second trip (images taller than 32 workgroups x 16 bands x 64);
  d. the scan path: empty row slices, segments starting on, before and after the
     slice boundaries, row chunks at the thread, wave and workgroup edges, LA16
     beside RGBA8, and bytes that carry through add_bytes and the wave / LDS prefix."""
import numpy as np
import pytest

import png_filter_util as pf
from imagekit import decode_image, decode_image_batch
from test_gpu_png import gpu_png, on_gpu  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

BYTEWISE = (1, 2, 3, 6)
RGBA8, LA16 = (8, 6), (16, 4)


def bpp_of(kind):
    return pf.CHANNELS[kind[1]] * kind[0] // 8


def png_of(rows, kind, fts, **kw):
    bpp = bpp_of(kind)
    h, w = rows.shape[0], rows.shape[1] // bpp
    return pf.write_png(rows, w, h, kind[0], kind[1], fts, **kw)


def check_batch(cases):
    """cases: (rows, (depth, colour type), filter types); one decode_image_batch call."""
    datas = [png_of(rows, kind, fts, idat_size=65536) for rows, kind, fts in cases]
    out = decode_image_batch(datas) if len(datas) > 1 else [decode_image(datas[0])]
    assert len(out) == len(cases)
    for n, ((d, fmt), (rows, kind, fts)) in enumerate(zip(out, cases)):
        h, w = rows.shape[0], rows.shape[1] // bpp_of(kind)
        want = pf.from_rows(rows, w, h, kind[0], kind[1])
        got = d.to_array()
        assert fmt is None and got.dtype == want.dtype
        np.testing.assert_array_equal(got.reshape(want.shape), want, err_msg=f"image {n}: {w}x{h} {kind}")


def probe_phases(bpp):
    return (1, 0) if bpp in BYTEWISE else (1,)


# ---- a. predictor inputs ----------------------------------------------------------------
@pytest.mark.parametrize("bpp", [4, 8, 1, 2, 3, 6])
def test_paeth_inputs(on_gpu, bpp):
    rows, fts = pf.probe_image(bpp, 4, pf.paeth_triples(zero_c=bpp in BYTEWISE), phases=probe_phases(bpp))
    check_batch([(rows, pf.KIND[bpp], fts)])


@pytest.mark.parametrize("bpp", [4, 8, 1, 2, 3, 6])
def test_average_inputs(on_gpu, bpp):
    u, v = pf.pair_triples()
    rows, fts = pf.probe_image(bpp, 3, np.stack([u, v, u ^ v], 1), phases=probe_phases(bpp))
    check_batch([(rows, pf.KIND[bpp], fts)])


@pytest.mark.parametrize("bpp", [4, 8, 1, 2, 3, 6])
def test_sub_up_inputs(on_gpu, bpp):
    """(The even rows cycle through all types, so the 4-byte images hold Paeth rows
    and take the diagonal kernel, not the scan path.)"""
    u, v = pf.pair_triples()
    cases = []
    for ft in (1, 2):
        rows, fts = pf.probe_image(bpp, ft, np.stack([v, v, u], 1), raw=u, phases=probe_phases(bpp))
        assert (fts >= 3).any()
        cases.append((rows, pf.KIND[bpp], fts))
    check_batch(cases)


# ---- b. diagonal-kernel geometry -------------------------------------------------------
L8_WIDTHS = [1, 15, 16, 17, 112, 113, 127, 128, 129, 1008, 1009, 1024, 1025, 1136, 1151, 1152, 1153]
HEIGHTS = [1, 63, 64, 65, 127, 128, 129, 1023, 1024, 1025, 1088, 1089]


def l8_geometry():
    """Each width with a one-band, a two-band and a two-workgroup (K = 2) height;
    each height with 1, 9 and 65 row chunks."""
    wh = []
    for i, w in enumerate(L8_WIDTHS):
        wh += [(w, (1, 63, 64)[i % 3]), (w, (65, 127, 128)[i % 3]), (w, (1025, 1088, 1089)[i % 3])]
    for i, h in enumerate(HEIGHTS):
        wh += [((1, 15, 16)[i % 3], h), (129, h), (1025, h)]
    return list(dict.fromkeys(wh))


def noise_case(k, w, h, kind, need_paeth=False):
    rng = np.random.default_rng(1000 + k)
    rows = rng.integers(0, 256, (h, w * bpp_of(kind)), dtype=np.uint8)
    fts = rng.integers(0, 5, h).astype(np.uint8)
    fts[0] = k % 5
    if need_paeth and not (fts >= 3).any():
        fts[-1] = 4
    return rows, kind, fts


def test_l8_geometry_cases_meet_the_plan():
    """(No GPU work: the case list itself, against the kernel's constants.)"""
    wh = l8_geometry()
    nch = lambda w: (w + 15) // 16
    for w in L8_WIDTHS:
        hs = [h for ww, h in wh if ww == w]
        assert any(h <= 64 for h in hs) and any(64 < h <= 128 for h in hs) and any(h > 1024 for h in hs)
    for h in HEIGHTS:
        assert {1, 9, 65} <= {nch(w) for w, hh in wh if hh == h}
    assert {nch(w) for w in L8_WIDTHS} >= {1, 7, 8, 9, 63, 64, 65, 71, 72, 73}
    assert {w % 16 for w in L8_WIDTHS} >= {0, 1, 15}


@pytest.mark.parametrize("part", range(4))
def test_geometry_l8(on_gpu, part):
    """Batches that interleave the cases, so k_png_unfilter's tickets mix images of
    one and of several workgroups."""
    wh = l8_geometry()
    check_batch([noise_case(k, w, h, (8, 0)) for k, (w, h) in enumerate(wh) if k % 4 == part])


@pytest.mark.parametrize("kinds", [((8, 4), (16, 0)), ((8, 2),), (RGBA8, LA16), ((16, 2),), ((16, 6),)],
                         ids=["bpp2", "bpp3", "bpp4", "bpp6", "bpp8"])
def test_geometry_other_pixel_sizes(on_gpu, kinds):
    """Row bytes around 1, 8 / 9, 64 / 65 and 72 / 73 chunks for the other pixel sizes
    (the 4-byte images with an Average or Paeth row: the diagonal kernel)."""
    bpp = bpp_of(kinds[0])
    heights = [(1, 1025), (64, 1089), (65, 1024), (128, 1088), (63, 1023), (129, 127)]
    cases = []
    for i, rb in enumerate([1, 17, 113, 128, 129, 1009, 1024, 1025, 1153]):
        w = -(-rb // bpp)
        for h in heights[i % len(heights)]:
            k = len(cases)
            cases.append(noise_case(bpp * 100 + k, w, h, kinds[k % len(kinds)], need_paeth=bpp == 4))
    check_batch(cases)


# ---- c. the capped-K band loop ---------------------------------------------------------
def test_band_loop_second_trip(on_gpu):
    """Taller than 32 x 16 x 64 = 32,768 rows (+ 1,024): a wave takes a second band
    (band += 16 K, K capped at 32), and band 512 waits on band 511."""
    cases = []
    for k, (w, h, kind) in enumerate([(17, 33857, (8, 0)), (5, 33920, RGBA8)]):
        rng = np.random.default_rng(7 + k)
        rows = rng.integers(0, 256, (h, w * bpp_of(kind)), dtype=np.uint8)
        fts = ((np.arange(h) + k) % 5).astype(np.uint8)
        fts[h // 2:] = rng.integers(0, 5, h - h // 2)
        assert set(fts.tolist()) == {0, 1, 2, 3, 4}
        cases.append((rows, kind, fts))
    check_batch(cases)


# ---- d. the scan path ------------------------------------------------------------------
CARRY_BYTES = np.array([0x00, 0x01, 0x7F, 0x80, 0xFE, 0xFF], np.uint8)
SCAN_WIDTHS = [1, 3, 4, 5, 15, 16, 17, 1001, 1023, 1024, 1025, 4095, 8191]  # in 4-byte pixels
SCAN_HEIGHTS = [1, 2, 15, 16, 17, 31]


def carry_rows(rng, h, w, filtered, fts):
    """Rows of the carry bytes, with all-0xFF rows among them -- as the pixels, or
    (filtered) as the stream's filtered bytes, which the kernel's sums start from."""
    x = CARRY_BYTES[rng.integers(0, len(CARRY_BYTES), (h, w * 4))]
    x[rng.random(h) < 0.25] = 0xFF
    return pf.unfilter_rows_scan(x, 4, fts) if filtered else x


def scan_types(rng, h, k):
    fts = rng.choice(np.array([0, 1, 2, 2], np.uint8), h)
    fts[0] = k % 3
    return fts


@pytest.mark.parametrize("kind", [RGBA8, LA16], ids=["rgba8", "la16"])
def test_scan_path_sizes(on_gpu, kind):
    """Every height (below kSuRanges = 16 some workgroups' row slices are empty) with
    every width: 4, 256, 1,024 and 2,048 chunks a row and one more or less."""
    rng = np.random.default_rng(kind[0])
    cases = []
    for h in SCAN_HEIGHTS:
        for w in SCAN_WIDTHS:
            k = len(cases)
            fts = scan_types(rng, h, k)
            cases.append((carry_rows(rng, h, w, k % 2 == 1, fts), kind, fts))
    check_batch(cases)


def boundary_types(h, delta):
    """Up rows, with a None or Sub row at H jr / 16 + delta for every workgroup jr."""
    fts = np.full(h, 2, np.uint8)
    for jr in range(16):
        y = h * jr // 16 + delta
        if 0 <= y < h:
            fts[y] = jr % 2
    return fts


@pytest.mark.parametrize("kind", [RGBA8, LA16], ids=["rgba8", "la16"])
def test_scan_path_segments_at_slice_boundaries(on_gpu, kind):
    rng = np.random.default_rng(100 + kind[0])
    cases = []
    for h in (160, 161, 1000):
        for delta in (-1, 0, 1):
            w = (300, 1025, 77)[(delta + 1)]
            fts = boundary_types(h, delta)
            cases.append((carry_rows(rng, h, w, h != 161, fts), kind, fts))
    h, w = 161, 1001
    for fts in (np.full(h, 2, np.uint8), np.full(h, 1, np.uint8), (1 + np.arange(h) % 2).astype(np.uint8),
                (2 - np.arange(h) % 2).astype(np.uint8)):  # Up from row 0, all Sub, Sub / Up, Up / Sub
        cases.append((carry_rows(rng, h, w, len(cases) % 2 == 0, fts), kind, fts))
    # the same pixels with a final Paeth row: the diagonal kernel, the same result
    rows, _, fts = cases[1]
    twin = fts.copy()
    twin[-1] = 4
    cases.append((rows, kind, twin))
    check_batch(cases)
