"""PNG row filters in plain numpy, a PNG writer for 8- and 16-bit L / LA / RGB /
RGBA with chosen row filters, and the probe images that put chosen predictor
inputs (a = left, b = up, c = up-left) under every byte of a pixel.

filter_rows is the PNG definition vectorised over the image (filtering reads only
the unfiltered image, so a, b, c are shifted copies); unfilter_rows is its inverse
as a byte loop straight from the specification -- the reference of the tests.
Rows are (H, rowbytes) uint8 arrays as they lie in the stream (16-bit samples big
endian), `bpp` the bytes per pixel (1, 2, 3, 4, 6, 8)."""
import struct
import zlib

import numpy as np

CHANNELS = {0: 1, 4: 2, 2: 3, 6: 4}  # PNG colour type -> samples per pixel
CTYPE = {1: 0, 2: 4, 3: 2, 4: 6}
# the image kind behind each bytes-per-pixel class of the unfilter: (depth, colour type)
KIND = {1: (8, 0), 2: (8, 4), 3: (8, 2), 4: (8, 6), 6: (16, 2), 8: (16, 6)}


def paeth(a, b, c):
    """The Paeth predictor of int arrays a, b, c (0..255), as the specification words it."""
    p = a + b - c
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
    return np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))


def neighbours(raw_rows, bpp):
    """a, b, c of every byte of the unfiltered image (int16; zeros outside it)."""
    x = np.asarray(raw_rows, np.uint8).astype(np.int16)
    a = np.zeros_like(x)
    a[:, bpp:] = x[:, :-bpp]
    b = np.zeros_like(x)
    b[1:] = x[:-1]
    c = np.zeros_like(x)
    c[1:, bpp:] = x[:-1, :-bpp]
    return a, b, c


def row_types(ft, h):
    return np.full(h, ft, np.uint8) if np.isscalar(ft) else np.asarray(ft, np.uint8).reshape(h)


def filter_rows(raw_rows, bpp, ft):
    """Filtered bytes (H, rowbytes) of the unfiltered rows; ft: one type or one per row."""
    x = np.asarray(raw_rows, np.uint8).astype(np.int16)
    ft = row_types(ft, x.shape[0])
    assert ft.max(initial=0) <= 4
    a, b, c = neighbours(raw_rows, bpp)
    out = x.copy()
    for t in range(1, 5):
        r = ft == t
        if not r.any():
            continue
        pred = a[r] if t == 1 else b[r] if t == 2 else (a[r] + b[r]) >> 1 if t == 3 else paeth(a[r], b[r], c[r])
        out[r] = x[r] - pred
    return (out & 255).astype(np.uint8)


def unfilter_rows(filt_rows, bpp, ft):
    """The inverse of filter_rows, byte by byte (slow: small images only)."""
    f = np.asarray(filt_rows, np.uint8)
    h, rb = f.shape
    ft = row_types(ft, h)
    out = np.zeros((h, rb), np.uint8)
    prev = [0] * rb
    for y in range(h):
        src, cur, t = f[y].tolist(), [0] * rb, int(ft[y])
        for i in range(rb):
            a = cur[i - bpp] if i >= bpp else 0
            b = prev[i]
            c = prev[i - bpp] if i >= bpp else 0
            if t == 0:
                pred = 0
            elif t == 1:
                pred = a
            elif t == 2:
                pred = b
            elif t == 3:
                pred = (a + b) // 2
            else:
                p = a + b - c
                pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
                pred = a if pa <= pb and pa <= pc else b if pb <= pc else c
            cur[i] = (src[i] + pred) & 255
        out[y] = cur
        prev = cur
    return out


def unfilter_rows_scan(filt_rows, bpp, ft):
    """unfilter_rows for rows of types 0 / 1 / 2 only, a row at a time (Sub is a sum
    along the row per byte of the pixel): builds images from chosen filtered bytes."""
    f = np.asarray(filt_rows, np.uint8)
    h, rb = f.shape
    assert rb % bpp == 0
    ft = row_types(ft, h)
    assert ft.max(initial=0) <= 2
    out = np.zeros((h, rb), np.uint8)
    prev = np.zeros(rb, np.uint8)
    for y in range(h):
        if ft[y] == 1:
            out[y] = (np.cumsum(f[y].reshape(-1, bpp).astype(np.uint32), 0) & 255).reshape(rb)
        else:
            out[y] = f[y] + prev if ft[y] == 2 else f[y]  # (uint8: mod 256)
        prev = out[y]
    return out


def to_rows(img):
    """(H, W, C) uint8 / uint16 pixels -> the stream's rows (16-bit big endian)."""
    h = img.shape[0]
    if img.dtype == np.uint16:
        return img.astype(">u2").view(np.uint8).reshape(h, -1)
    return np.ascontiguousarray(img, np.uint8).reshape(h, -1)


def from_rows(raw_rows, w, h, depth, ctype):
    """The stream's rows -> (H, W, C) pixels, uint16 at depth 16."""
    r = np.ascontiguousarray(raw_rows, np.uint8)
    if depth == 16:
        return r.view(">u2").astype(np.uint16).reshape(h, w, CHANNELS[ctype])
    return r.reshape(h, w, CHANNELS[ctype])


def _chunk(t, d):
    return struct.pack(">I", len(d)) + t + d + struct.pack(">I", zlib.crc32(t + d) & 0xFFFFFFFF)


def write_png(raw_rows, w, h, depth, ctype, ft, level=1, idat_size=None):
    """A PNG file of the unfiltered rows with row filter(s) `ft`."""
    bpp = CHANNELS[ctype] * depth // 8
    raw_rows = np.asarray(raw_rows, np.uint8)
    assert depth in (8, 16) and raw_rows.shape == (h, w * bpp)
    body = np.empty((h, 1 + w * bpp), np.uint8)
    body[:, 0] = row_types(ft, h)
    body[:, 1:] = filter_rows(raw_rows, bpp, ft)
    z = zlib.compress(body.tobytes(), level)
    out = b"\x89PNG\r\n\x1a\n" + _chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, depth, ctype, 0, 0, 0))
    step = idat_size or len(z)
    for i in range(0, len(z), step):
        out += _chunk(b"IDAT", z[i:i + step])
    return out + _chunk(b"IEND", b"")


# ---- triple sets -------------------------------------------------------------------
def paeth_pairs():
    """Every feasible (d1 = b - c, d2 = a - c): max(0, d1, d2) - min(0, d1, d2) <= 255."""
    d1, d2 = np.meshgrid(np.arange(-255, 256), np.arange(-255, 256), indexing="ij")
    d1, d2 = d1.ravel(), d2.ravel()
    ok = np.maximum(0, np.maximum(d1, d2)) - np.minimum(0, np.minimum(d1, d2)) <= 255
    return d1[ok], d2[ok]


def paeth_triples(zero_c=False):
    """(a, b, c) for every feasible (d1, d2), c at its lowest and its highest feasible
    value; zero_c adds d1 = d2 = 0 at every c (that class is one pair, too few to
    reach every byte offset of a chunk)."""
    d1, d2 = paeth_pairs()
    lo = -np.minimum(0, np.minimum(d1, d2))
    hi = 255 - np.maximum(0, np.maximum(d1, d2))
    c = np.concatenate([lo, hi])
    d1, d2 = np.tile(d1, 2), np.tile(d2, 2)
    t = np.stack([c + d2, c + d1, c], 1)
    if zero_c:
        t = np.concatenate([t, np.repeat(np.arange(256), 3).reshape(256, 3)])
    assert t.min() >= 0 and t.max() <= 255
    return t.astype(np.uint8)


def pair_triples():
    """All 65,536 (u, v): Average's (a, b) = (u, v); Sub's and Up's (raw, a) / (raw, b)
    with raw = u (probe_image's `raw`) and a = b = v."""
    u, v = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    return u.ravel().astype(np.uint8), v.ravel().astype(np.uint8)


def _hash(n, salt):
    i = np.arange(n, dtype=np.uint64) + np.uint64(salt)
    return ((i * np.uint64(2654435761)) >> np.uint64(13)).astype(np.uint8)


def probe_image(bpp, ft, triples, raw=None, width=2049, phases=(1,), seed=1):
    """Unfiltered rows (H, width * bpp) and their filter types.

    Rows come in pairs (2k, 2k+1); in the odd row of a pair of phase 1 every odd
    pixel x is a probe, and for each byte of the pixel independently a = row 2k+1
    pixel x-1, b = row 2k pixel x, c = row 2k pixel x-1 are free (the even columns
    belong to one probe only).  Phase 0 moves the probes to the even pixels from 2
    on (1- and 2-byte pixels reach only half of a chunk's byte offsets otherwise);
    pair k has phase phases[k % len].  The triples go to the probes in a seeded
    random order, byte j of the pixels taking the list rotated by j * 7919, so the
    bytes of one pixel hold different triples.  A probe's own value is a hash of
    its index -- or, where `raw` is given, what makes its filtered byte raw[i].
    Odd rows carry filter `ft`, even rows cycle through 0..4."""
    triples = np.asarray(triples, np.uint8)
    n = len(triples)
    order = np.random.default_rng(seed).permutation(n)
    per = (width - 1) // 2
    pairs = -(-n // per)
    slots = pairs * per
    img = _hash(2 * pairs * width * bpp, 77).reshape(2 * pairs, width, bpp)
    k = np.arange(slots) // per
    x = 2 * (np.arange(slots) % per) + 2 - np.asarray(phases)[k % len(phases)]
    for j in range(bpp):
        idx = order[(np.arange(slots) + j * 7919) % n]
        a, b, c = (triples[idx, q] for q in range(3))
        img[2 * k + 1, x - 1, j] = a
        img[2 * k, x, j] = b
        img[2 * k, x - 1, j] = c
        if raw is not None:
            ai, bi, ci = a.astype(np.int16), b.astype(np.int16), c.astype(np.int16)
            pred = 0 if ft == 0 else ai if ft == 1 else bi if ft == 2 else (ai + bi) >> 1 if ft == 3 else paeth(ai, bi, ci)
            img[2 * k + 1, x, j] = (np.asarray(raw, np.uint8)[idx].astype(np.int16) + pred) & 255
    fts = np.empty(2 * pairs, np.uint8)
    fts[0::2] = np.arange(pairs) % 5
    fts[1::2] = ft
    return img.reshape(2 * pairs, width * bpp), fts
