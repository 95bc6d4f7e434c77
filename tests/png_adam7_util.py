"""A PNG writer for the Adam7 tests: any colour type and bit depth, interlaced or
not, a chosen filter type per row of each pass, IDAT splitting, and hooks to damage
the inflated bytes.  Also the PNG spec's pass geometry restated, and the pixels
png's EXPAND gives for a source array (what decode_image returns)."""
import struct
import zlib

import numpy as np

SPP = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}
X0, Y0 = (0, 4, 0, 2, 0, 1, 0), (0, 0, 4, 0, 2, 0, 1)
DX, DY = (8, 8, 4, 4, 2, 2, 1), (8, 8, 8, 4, 4, 2, 2)


def passes(w, h, bits_pp):
    """PNG spec section 8.2: (x0, y0, dx, dy, pw, ph, rowbytes, raw offset) of every
    non-empty pass, and the inflated length."""
    out, off = [], 0
    for p in range(7):
        pw, ph = len(range(X0[p], w, DX[p])), len(range(Y0[p], h, DY[p]))
        if pw and ph:
            rb = (pw * bits_pp + 7) // 8
            out.append((X0[p], Y0[p], DX[p], DY[p], pw, ph, rb, off))
            off += (rb + 1) * ph
    return out, off


def chunk(t, d):
    return struct.pack(">I", len(d)) + t + d + struct.pack(">I", zlib.crc32(t + d) & 0xFFFFFFFF)


def pack_rows(s, depth):
    """(h, w, spp) samples -> (h, rowbytes) bytes: big-endian 16-bit samples, fields
    below 8 bits MSB first with zero padding bits."""
    h, w, spp = s.shape
    if depth == 16:
        return s.astype(">u2").view(np.uint8).reshape(h, w * spp * 2)
    if depth == 8:
        return s.astype(np.uint8).reshape(h, w * spp)
    f = 8 // depth
    v = np.zeros((h, (w + f - 1) // f * f), np.uint8)
    v[:, :w] = s[..., 0]
    v = v.reshape(h, -1, f)
    return sum(v[:, :, k] << (8 - depth - k * depth) for k in range(f)).astype(np.uint8)


def filter_rows(rows, bpp, ft_of):
    """rows (h, rowbytes) -> filter byte + filtered row, each; ft_of(y) = filter type."""
    out, prev = [], np.zeros(rows.shape[1], np.int32)
    for y in range(rows.shape[0]):
        cur, ft = rows[y].astype(np.int32), ft_of(y)
        a = np.concatenate([np.zeros(bpp, np.int32), cur[:-bpp]])[: len(cur)]
        c = np.concatenate([np.zeros(bpp, np.int32), prev[:-bpp]])[: len(cur)]
        if ft == 0:
            f = cur
        elif ft == 1:
            f = cur - a
        elif ft == 2:
            f = cur - prev
        elif ft == 3:
            f = cur - ((a + prev) >> 1)
        else:
            p = a + prev - c
            pa, pb, pc = np.abs(p - a), np.abs(p - prev), np.abs(p - c)
            f = cur - np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, prev, c))
        out.append(bytes([ft]) + (f & 255).astype(np.uint8).tobytes())
        prev = cur
    return out


def raw_stream(s, depth, interlace=True, filt=None):
    """The inflated bytes of an image of (h, w, spp) samples.  filt: None = the
    y % 5 cycle restarted in every pass, an int = that type on every row, or a
    callable (pass index among the non-empty ones, row of the pass) -> type."""
    h, w, spp = s.shape
    bpp = max(1, spp * depth // 8)
    geo = passes(w, h, spp * depth)[0] if interlace else [(0, 0, 1, 1, w, h, 0, 0)]
    rows = []
    for q, (x0, y0, dx, dy, _pw, _ph, _rb, _off) in enumerate(geo):
        if callable(filt):
            ft_of = lambda y, q=q: filt(q, y)  # noqa: E731
        else:
            ft_of = (lambda y: y % 5) if filt is None else (lambda y: filt)
        rows += filter_rows(pack_rows(s[y0::dy, x0::dx], depth), bpp, ft_of)
    return rows


def make_png(s, ctype, depth=8, interlace=1, filt=None, plte=None, trns=None, level=6, idat=None, raw_edit=None):
    """The PNG file.  s: (h, w, spp) integer samples; interlace: IHDR's method byte (1:
    Adam7 rows; 0 or 2: plain rows under that byte); idat: split the zlib stream into
    IDAT chunks of that many bytes; raw_edit: list of filtered rows -> the list to
    compress (to damage a stream)."""
    s = np.asarray(s)
    h, w, spp = s.shape
    assert spp == SPP[ctype]
    rows = raw_stream(s, depth, interlace == 1, filt)
    if raw_edit is not None:
        rows = raw_edit(rows)
    raw = b"".join(rows)
    if interlace == 1 and raw_edit is None:
        assert len(raw) == passes(w, h, spp * depth)[1]
    z = zlib.compress(raw, level)
    out = b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, depth, ctype, 0, 0, interlace))
    if plte is not None:
        out += chunk(b"PLTE", bytes(np.asarray(plte, np.uint8).reshape(-1)))
    if trns is not None:
        out += chunk(b"tRNS", bytes(trns))
    step = idat or len(z)
    for o in range(0, len(z), step):
        out += chunk(b"IDAT", z[o:o + step])
    out += chunk(b"IEND", b"")
    assert out[28] == interlace  # IHDR byte 12: the interlace method really is in the file
    return out


def idat_bytes(png):
    """The concatenated IDAT payloads of a file."""
    pos, z = 8, b""
    while pos < len(png):
        n, t = struct.unpack(">I", png[pos:pos + 4])[0], png[pos + 4:pos + 8]
        if t == b"IDAT":
            z += png[pos + 8:pos + 8 + n]
        pos += 12 + n
    return z


def expanded(s, ctype, depth, plte=None, trns=None):
    """What decode_image gives for the samples: png's EXPAND (palette -> RGB(A), gray
    below 8 bits scaled, a tRNS key as alpha), 16-bit samples kept as uint16."""
    s = np.asarray(s)
    dt, top = (np.uint16, 65535) if depth == 16 else (np.uint8, 255)
    if ctype == 3:
        pal = np.zeros((256, 4), np.uint8)
        pal[:, 3] = 255
        p = np.asarray(plte, np.uint8).reshape(-1, 3)
        pal[: len(p), :3] = p
        if trns is not None:
            pal[: len(trns), 3] = np.frombuffer(bytes(trns), np.uint8)
        return pal[s[..., 0]][..., : 4 if trns is not None else 3]
    px = s.astype(np.uint32)
    if ctype == 0 and depth < 8:
        px = px * (255 // ((1 << depth) - 1))
    if trns is None:
        return px.astype(dt)
    key = np.array(struct.unpack(">" + "H" * SPP[ctype], bytes(trns)), np.uint32)
    a = np.where((s.astype(np.uint32) == key).all(-1), 0, top)
    return np.concatenate([px, a[..., None]], -1).astype(dt)


def pillow_pixels(png):
    """Pillow's (libpng's) decode of the file, brought to decode_image's layout where
    Pillow keeps one: None for what Pillow reduces (16-bit colour) or widens."""
    import io

    from PIL import Image
    im = Image.open(io.BytesIO(png))
    im.load()
    tr = im.info.get("transparency")
    if im.mode == "P":
        return np.asarray(im.convert("RGBA" if tr is not None else "RGB"))
    if im.mode == "1":
        a = np.asarray(im.convert("L"))
    elif im.mode in ("L", "LA", "RGB", "RGBA"):
        a = np.asarray(im)
        if png[25] == 4 and im.mode == "RGBA":  # (Pillow opens 16-bit gray + alpha as RGBA)
            a = a[..., [0, 3]]
    elif im.mode in ("I;16", "I;16B", "I"):
        a = np.asarray(im).astype(np.uint16)
    else:
        return None
    if a.ndim == 2:
        a = a[..., None]
    return a
