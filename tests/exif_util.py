"""EXIF test inputs built by hand: TIFF payloads with a chosen IFD0, and the three
containers (JPEG APP1, PNG eXIf, WebP EXIF) wrapped around them chunk by chunk, so the
tests can place the metadata where Pillow never does.  Also the numpy form of the eight
orientations (include/imagekit_hip.h) and the Pillow-written files the tests share."""
import io
import struct
import zlib

import numpy as np
from PIL import Image

ORIENTATION, SHORT, LONG = 0x0112, 3, 4
PREFIX = b"Exif\0\0"
# Image.transpose op of each EXIF value (what ImageOps.exif_transpose applies)
PIL_OP = {2: Image.Transpose.FLIP_LEFT_RIGHT, 3: Image.Transpose.ROTATE_180, 4: Image.Transpose.FLIP_TOP_BOTTOM,
          5: Image.Transpose.TRANSPOSE, 6: Image.Transpose.ROTATE_270, 7: Image.Transpose.TRANSVERSE,
          8: Image.Transpose.ROTATE_90}


def orient_np(a, o):
    """out[y][x] of the header's table for an (H, W, ...) array."""
    if o == 1:
        return a.copy()
    if o == 2:
        return a[:, ::-1].copy()
    if o == 3:
        return a[::-1, ::-1].copy()
    if o == 4:
        return a[::-1].copy()
    t = np.swapaxes(a, 0, 1)  # t[y][x] = S[x][y]
    if o == 5:
        return t.copy()
    if o == 6:  # S[H-1-x][y]: 90 degrees clockwise
        return np.rot90(a, -1).copy()
    if o == 7:  # S[H-1-x][W-1-y]
        return t[::-1, ::-1].copy()
    if o == 8:  # S[x][W-1-y]: 90 degrees counter-clockwise
        return np.rot90(a, 1).copy()
    raise ValueError(o)


def entry(tag, typ, count, value, le):
    """One 12-byte IFD entry whose value fits the value field (SHORTs left-justified)."""
    e = "<" if le else ">"
    if typ == SHORT and count <= 2:
        vals = list(value) if isinstance(value, (list, tuple)) else [value]
        field = struct.pack(e + "H" * len(vals), *vals).ljust(4, b"\0")
    else:
        field = struct.pack(e + "I", value if not isinstance(value, (list, tuple)) else value[0])
    return struct.pack(e + "HHI", tag, typ, count) + field


def tiff(entries, le=True, prefix=False, ifd_offset=8, count=None):
    """A TIFF payload: header, IFD0 at ifd_offset with `entries` (12-byte blobs) and a zero
    next-IFD link.  count overrides the entry count written (to point past the payload);
    an ifd_offset past the payload is written as is, with the IFD left at 8."""
    e = "<" if le else ">"
    head = (b"II" if le else b"MM") + struct.pack(e + "HI", 42, ifd_offset)
    at = ifd_offset if 8 <= ifd_offset <= 64 else 8
    body = b"\0" * (at - 8) + struct.pack(e + "H", len(entries) if count is None else count) + b"".join(entries)
    body += struct.pack(e + "I", 0)
    return (PREFIX if prefix else b"") + head + body


def other(le, k=0):
    """IFD0 entries that are not the orientation: XResolution-like LONGs and a SHORT."""
    return [entry(0x0100, LONG, 1, 640, le), entry(0x0128, SHORT, 1, 2, le), entry(0x0131 + k, LONG, 1, 77, le)]


def _base_image():
    return Image.fromarray((np.arange(7 * 5 * 3, dtype=np.uint8) * 2).reshape(5, 7, 3), "RGB")


def jpeg_wrap(payload, after_app0=True):
    """A baseline JPEG with one APP1 holding `payload` (prefixed as JPEG requires), before
    or after the APP0 Pillow writes."""
    buf = io.BytesIO()
    _base_image().save(buf, format="JPEG")
    b = buf.getvalue()
    assert b[2:4] == b"\xff\xe0"
    app0_end = 4 + struct.unpack(">H", b[4:6])[0]
    p = payload if payload.startswith(PREFIX) else PREFIX + payload
    app1 = b"\xff\xe1" + struct.pack(">H", len(p) + 2) + p
    at = app0_end if after_app0 else 2
    return b[:at] + app1 + b[at:]


def _png_chunk(typ, data):
    return struct.pack(">I", len(data)) + typ + data + struct.pack(">I", zlib.crc32(typ + data))


def png_wrap(payload, after_idat=False):
    buf = io.BytesIO()
    _base_image().save(buf, format="PNG")
    b = buf.getvalue()
    pos, chunks = 8, []
    while pos < len(b):
        n = struct.unpack(">I", b[pos:pos + 4])[0]
        chunks.append((b[pos + 4:pos + 8], b[pos:pos + 12 + n]))
        pos += 12 + n
    out = b[:8]
    for typ, raw in chunks:
        if typ == (b"IEND" if after_idat else b"IDAT") and payload is not None:
            out += _png_chunk(b"eXIf", payload)
            payload = None
        out += raw
    return out


def webp_wrap(payload):
    """A VP8X RIFF: VP8X, the lossless image chunk, an odd-sized unknown chunk (padded),
    then EXIF."""
    buf = io.BytesIO()
    _base_image().save(buf, format="WEBP", lossless=True)
    b = buf.getvalue()
    assert b[12:16] == b"VP8L"
    image = b[12:]
    if len(image) & 1:
        image += b"\0"

    def chunk(typ, data):
        return typ + struct.pack("<I", len(data)) + data + (b"\0" if len(data) & 1 else b"")

    vp8x = chunk(b"VP8X", bytes([0x08, 0, 0, 0]) + (6).to_bytes(3, "little") + (4).to_bytes(3, "little"))
    body = b"WEBP" + vp8x + image + chunk(b"JUNK", b"abc") + chunk(b"EXIF", payload)
    return b"RIFF" + struct.pack("<I", len(body)) + body


WRAPPERS = {
    "jpeg-app1-after-app0": lambda p: jpeg_wrap(p, True),
    "jpeg-app1-before-app0": lambda p: jpeg_wrap(p, False),
    "png-exif-before-idat": lambda p: png_wrap(p, False),
    "png-exif-after-idat": lambda p: png_wrap(p, True),
    "webp-exif-after-odd-chunk": webp_wrap,
}


def pillow_file(fmt, o, img=None):
    """A Pillow-written file (JPEG, PNG or lossless WEBP) of img (default: 7 x 5 RGB)
    carrying EXIF orientation o; o None writes no EXIF."""
    img = img or _base_image()
    kw = {"lossless": True} if fmt == "WEBP" else {}
    if o is not None:
        ex = Image.Exif()
        ex[ORIENTATION] = o
        kw["exif"] = ex.tobytes()
    buf = io.BytesIO()
    img.save(buf, format=fmt, **kw)
    return buf.getvalue()
