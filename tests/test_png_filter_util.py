"""CPU: the PNG writer and probe images of png_filter_util.py, which the GPU
unfilter tests (test_gpu_png_unfilter.py) rest on.  The filters round-trip through
the byte-wise reference, Pillow (libpng) decodes every kind of file to the source
pixels, and what a probe image puts under the predictor is computed here from the
image itself with the reference predictor -- conditions the inputs meet exactly:
every feasible Paeth (d1, d2) in every byte lane of a pixel, every Paeth outcome
class and both +-255 extremes at every byte offset of a 16-byte chunk for the
byte-wise variants, every (a, b) under Average in every byte lane."""
import io

import numpy as np
import pytest
from PIL import Image

import png_filter_util as pf

BPPS = [1, 2, 3, 4, 6, 8]
BYTEWISE = [1, 2, 3, 6]


def noise_rows(h, rowbytes, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, rowbytes), dtype=np.uint8)


@pytest.mark.parametrize("bpp", BPPS)
@pytest.mark.parametrize("ft", [0, 1, 2, 3, 4, "mixed"])
def test_unfilter_inverts_filter(bpp, ft):
    h, w = 11, 23
    x = noise_rows(h, w * bpp, bpp * 10 + (9 if ft == "mixed" else ft))
    x[3] = 255
    x[4] = 0
    fts = np.random.default_rng(bpp).integers(0, 5, h) if ft == "mixed" else ft
    f = pf.filter_rows(x, bpp, fts)
    assert f.dtype == np.uint8 and f.shape == x.shape
    np.testing.assert_array_equal(pf.unfilter_rows(f, bpp, fts), x)
    if ft == 0:
        np.testing.assert_array_equal(f, x)


@pytest.mark.parametrize("bpp", [2, 4])
def test_scan_unfilter_equals_the_reference(bpp):
    """unfilter_rows_scan (types 0 / 1 / 2 from chosen filtered bytes) against the byte loop."""
    rng = np.random.default_rng(bpp)
    f = np.array([0x00, 0x01, 0x7F, 0x80, 0xFE, 0xFF], np.uint8)[rng.integers(0, 6, (19, 31 * bpp))]
    f[5] = 0xFF
    fts = rng.integers(0, 3, 19)
    x = pf.unfilter_rows_scan(f, bpp, fts)
    np.testing.assert_array_equal(x, pf.unfilter_rows(f, bpp, fts))
    np.testing.assert_array_equal(pf.filter_rows(x, bpp, fts), f)


def test_filter_rows_known_bytes():
    """A hand-worked 2 x 2 RGB image, one row of each of Sub and Paeth."""
    x = np.array([[10, 20, 30, 250, 5, 40], [12, 18, 33, 1, 200, 90]], np.uint8)
    f = pf.filter_rows(x, 3, [1, 4])
    np.testing.assert_array_equal(f[0], [10, 20, 30, 240, 241, 10])
    # row 1: first pixel predicts from b (a = c = 0); second: p = a + b - c per byte
    #   byte 3: a 12 b 250 c 10 -> p 252: pa 240 pb 2 pc 242 -> b;  1 - 250 = 7 (mod 256)
    #   byte 4: a 18 b 5 c 20 -> p 3: pa 15 pb 2 pc 17 -> b;  200 - 5 = 195
    #   byte 5: a 33 b 40 c 30 -> p 43: pa 10 pb 3 pc 13 -> b;  90 - 40 = 50
    np.testing.assert_array_equal(f[1], [2, 254, 3, 7, 195, 50])


def pil_pixels(data):
    im = Image.open(io.BytesIO(data))
    a = np.asarray(im)
    return im, a


@pytest.mark.parametrize("bpp", [1, 2, 3, 4])
def test_pillow_decodes_8bit_files(bpp):
    w, h = 37, 29
    x = noise_rows(h, w * bpp, 40 + bpp)
    fts = np.arange(h) % 5
    data = pf.write_png(x, w, h, 8, pf.CTYPE[bpp], fts, idat_size=777)
    im, a = pil_pixels(data)
    assert im.mode == {1: "L", 2: "LA", 3: "RGB", 4: "RGBA"}[bpp] and im.size == (w, h)
    np.testing.assert_array_equal(a.reshape(h, w * bpp), x)
    np.testing.assert_array_equal(pf.to_rows(pf.from_rows(x, w, h, 8, pf.CTYPE[bpp])), x)


def test_pillow_decodes_16bit_gray_file():
    """Pillow keeps 16 bits only for gray ("I;16"); the colour kinds share the writer's
    code (bpp = samples * 2) and are held by the filter round trip."""
    w, h = 41, 17
    px = np.random.default_rng(3).integers(0, 65536, (h, w, 1)).astype(np.uint16)
    rows = pf.to_rows(px)
    assert rows.shape == (h, 2 * w) and rows[0, 0] == px[0, 0, 0] >> 8
    data = pf.write_png(rows, w, h, 16, 0, np.arange(h) % 5)
    im, a = pil_pixels(data)
    np.testing.assert_array_equal(a.astype(np.uint16), px[..., 0])
    np.testing.assert_array_equal(pf.from_rows(rows, w, h, 16, 0), px)


@pytest.mark.parametrize("ctype", [4, 2, 6])
def test_pillow_reads_16bit_colour_files_high_bytes(ctype):
    """Pillow reduces 16-bit LA / RGB / RGBA to 8 bits (libpng strips the low byte):
    the high bytes it returns are the source's."""
    c = pf.CHANNELS[ctype]
    w, h = 19, 13
    px = np.random.default_rng(ctype).integers(0, 65536, (h, w, c)).astype(np.uint16)
    data = pf.write_png(pf.to_rows(px), w, h, 16, ctype, np.arange(h) % 5)
    im, a = pil_pixels(data)
    assert im.size == (w, h)
    if c == 2 and im.mode == "RGBA":  # (gray + alpha at 16 bits opens as RGBA: R = G = B = gray)
        a = a[..., [0, 3]]
    if a.dtype == np.uint8 and a.shape == (h, w, c):
        np.testing.assert_array_equal(a, (px >> 8).astype(np.uint8))
    else:  # a Pillow that keeps the 16 bits
        np.testing.assert_array_equal(np.asarray(a, np.uint16).reshape(h, w, c), px)


# ---- the triple sets ------------------------------------------------------------------
def test_paeth_pair_set_is_the_feasible_hexagon():
    d1, d2 = pf.paeth_pairs()
    assert len(d1) == 3 * 255 * 255 + 3 * 255 + 1
    t = pf.paeth_triples().astype(int)
    assert len(t) == 2 * len(d1)
    got = set(zip((t[:, 1] - t[:, 2]).tolist(), (t[:, 0] - t[:, 2]).tolist()))
    want = {(p, q) for p in range(-255, 256) for q in range(-255, 256) if max(0, p, q) - min(0, p, q) <= 255}
    assert got == want


def probe_file(bpp, ft, triples, raw=None, **kw):
    rows, fts = pf.probe_image(bpp, ft, triples, raw=raw, **kw)
    depth, ctype = pf.KIND[bpp]
    h, w = rows.shape[0], rows.shape[1] // bpp
    return rows, fts, pf.write_png(rows, w, h, depth, ctype, fts)


def inputs_of_rows(rows, fts, bpp, ft):
    """a, b, c and the byte's position in the row, of every byte of the rows of type
    ft -- from the image, as the unfilter will see them."""
    a, b, c = pf.neighbours(rows, bpp)
    r = fts == ft
    pos = np.broadcast_to(np.arange(rows.shape[1]), rows.shape)[r]
    return a[r].astype(np.int32), b[r].astype(np.int32), c[r].astype(np.int32), pos


def probe_phases(bpp):
    return (1, 0) if bpp in BYTEWISE else (1,)


@pytest.fixture(scope="module")
def feasible_codes():
    d1, d2 = pf.paeth_pairs()
    return np.unique((d1 + 255) * 511 + (d2 + 255))


@pytest.mark.parametrize("bpp", BPPS)
def test_paeth_probe_covers_every_pair_in_every_byte_lane(bpp, feasible_codes):
    rows, fts, data = probe_file(bpp, 4, pf.paeth_triples(zero_c=bpp in BYTEWISE), phases=probe_phases(bpp))
    assert set(fts[0::2].tolist()) == {0, 1, 2, 3, 4} and (fts[1::2] == 4).all()
    a, b, c, pos = inputs_of_rows(rows, fts, bpp, 4)
    code = (b - c + 255) * 511 + (a - c + 255)
    for j in range(bpp):  # the byte of the pixel: the byte lane inside unfilter_word
        lane = pos % bpp == j
        got = np.unique(code[lane])
        assert np.isin(feasible_codes, got).all(), f"byte {j}: {len(feasible_codes) - np.isin(feasible_codes, got).sum()} pairs missing"
        # each pair with c at its lowest and at its highest feasible value
        d1, d2 = (b - c)[lane], (a - c)[lane]
        lo = -np.minimum(0, np.minimum(d1, d2))
        hi = 255 - np.maximum(0, np.maximum(d1, d2))
        assert np.isin(feasible_codes, np.unique(code[lane][c[lane] == lo])).all()
        assert np.isin(feasible_codes, np.unique(code[lane][c[lane] == hi])).all()
    if bpp <= 4:  # (Pillow reduces the 16-bit colour kinds to 8 bits)
        _, px = pil_pixels(data)
        np.testing.assert_array_equal(px.reshape(rows.shape), rows)


@pytest.mark.parametrize("bpp", BYTEWISE)
def test_paeth_probe_covers_every_outcome_at_every_chunk_offset(bpp):
    """The byte-wise unfilter_chunk is 16 unrolled byte steps: each step (byte offset
    in the row mod 16) meets the seven Paeth outcome classes -- a, b, c winning
    strictly, the ties a=b, a=c, b=c, and d1 = d2 = 0 -- and d1, d2 at +-255."""
    rows, fts = pf.probe_image(bpp, 4, pf.paeth_triples(zero_c=True), phases=probe_phases(bpp))
    a, b, c, pos = inputs_of_rows(rows, fts, bpp, 4)
    d1, d2 = b - c, a - c
    pa, pb, pc = np.abs(d1), np.abs(d2), np.abs(d1 + d2)
    m = np.minimum(pa, np.minimum(pb, pc))
    cls = (pa == m) * 1 + (pb == m) * 2 + (pc == m) * 4  # which of a, b, c are nearest: 1..7
    for off in range(16):
        at = pos % 16 == off
        assert set(np.unique(cls[at]).tolist()) == {1, 2, 3, 4, 5, 6, 7}, f"offset {off}"
        # in the tie classes the candidates differ, so a wrong pick shows (a = b in class 3 always)
        assert (a[at & (cls == 5)] != c[at & (cls == 5)]).any() and (b[at & (cls == 6)] != c[at & (cls == 6)]).any()
        for d in (d1, d2):
            assert d[at].min() == -255 and d[at].max() == 255, f"offset {off}"
    # the first BPP bytes of a chunk take a and c from the chunk before: probes there too
    assert all(((pos % 16 < bpp) & (pos >= 16) & (cls == k)).any() for k in range(1, 8))


@pytest.mark.parametrize("bpp", BPPS)
def test_average_probe_covers_every_pair_in_every_byte_lane(bpp):
    u, v = pf.pair_triples()
    rows, fts, data = probe_file(bpp, 3, np.stack([u, v, u ^ v], 1), phases=probe_phases(bpp))
    a, b, _, pos = inputs_of_rows(rows, fts, bpp, 3)
    for j in range(bpp):
        lane = pos % bpp == j
        assert len(np.unique(a[lane] * 256 + b[lane])) == 65536, f"byte {j}"
    if bpp <= 4:
        _, px = pil_pixels(data)
        np.testing.assert_array_equal(px.reshape(rows.shape), rows)


@pytest.mark.parametrize("bpp", BPPS)
@pytest.mark.parametrize("ft", [1, 2])
def test_sub_up_probes_cover_every_raw_and_neighbour(bpp, ft):
    u, v = pf.pair_triples()
    rows, fts = pf.probe_image(bpp, ft, np.stack([v, v, u], 1), raw=u, phases=probe_phases(bpp))
    filt = pf.filter_rows(rows, bpp, fts)
    a, b, _, pos = inputs_of_rows(rows, fts, bpp, ft)
    raw = filt[fts == ft].astype(np.int32)
    nb = a if ft == 1 else b
    for j in range(bpp):
        lane = pos % bpp == j
        assert len(np.unique(raw[lane] * 256 + nb[lane])) == 65536, f"byte {j}"
    # even rows bring a Paeth row into the image: bpp 4 takes the diagonal kernel
    assert (fts == 4).any()


def test_probe_rows_survive_the_reference_unfilter():
    """A small probe image through the byte-wise reference (the big ones go through Pillow)."""
    t = pf.paeth_triples()[::97]
    for bpp in (3, 8):
        rows, fts = pf.probe_image(bpp, 4, t, width=65, phases=(1, 0))
        np.testing.assert_array_equal(pf.unfilter_rows(pf.filter_rows(rows, bpp, fts), bpp, fts), rows)
