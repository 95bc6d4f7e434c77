"""GPU: the upload's gather + CRC pass (ik_png.hip k_png_gather, k_png_crc_check) at its edges.

k_png_gather handles a piece (<= kPngGatherPiece = 65,536 bytes of one IDAT payload) in
the 16-byte granules of its source, a wave loading a 1 KiB span ("tile") at a time, and
realigns them to the destination's granules; the piece's CRC is joined from per-thread
sums.  What can go wrong is at edges: the source and destination misalignments (each
0..15, independent), pieces shorter than a granule, a word, a tile, a row of the
workgroup (8 KiB) or one byte either side of those, the last piece of a chunk, chunks of
several pieces, zero-length chunks, neighbours sharing a destination granule, and loads
next to the end of a device allocation.

The files are built here: 256 x 384 RGBA noise, filter 0, zlib level 0 -- stored blocks,
so a flipped payload byte still inflates and only the CRC can tell -- cut into IDAT
chunks of chosen lengths after a private ancillary chunk of 0..15 bytes that moves the
first payload byte over every source alignment (both input kinds put the file's first
byte on a 16-byte boundary).  Bars: pixels equal to Pillow's and the source, decoded by
the GPU path (ik_png_counters moves by (1, 0) per file: a wrong piece CRC would send a
good file to the host decoder); a corrupt chunk (zlib.crc32 of the chunk differs from
the stored CRC) gives png's CRC error for that file only."""
import ctypes
import io
import struct
import zlib

import numpy as np
import pytest
from PIL import Image

from imagekit import DeviceBytes, ImageFormat, TransformError, _lib, decode_image, transform_batch, \
    transform_batch_submit_device
from imagekit.transform import DynamicImage

pytestmark = pytest.mark.gpu

PIECE = 65536  # ik_png_gather.h kPngGatherPiece
TILE = 1024    # one wave's load instruction: 64 lanes x 16 bytes
LENGTHS = [1, 2, 3, 4, 5, 15, 16, 17, 63, 64, 65, 255, 256, 257, TILE - 1, TILE, TILE + 1, PIECE - 1, PIECE, PIECE + 1]
W, H = 256, 384


def _chunk(t, d):
    return struct.pack(">I", len(d)) + t + d + struct.pack(">I", zlib.crc32(t + d) & 0xFFFFFFFF)


@pytest.fixture(scope="module")
def src():
    """(pixels, zlib stream): 256 x 384 RGBA noise in stored blocks (393,000 bytes and more)"""
    img = np.random.default_rng(7).integers(0, 256, (H, W, 4), dtype=np.uint8)
    raw = b"".join(b"\0" + img[y].tobytes() for y in range(H))
    co = zlib.compressobj(0)
    z = co.compress(raw) + co.flush()
    assert len(z) > sum(LENGTHS) + 2 * PIECE
    return img, z


def _file(z, lengths, pad, iend=True):
    """the stream in IDAT chunks of `lengths` (the rest in one more), after a private
    ancillary chunk of `pad` bytes; returns (file, [(payload offset, length)])"""
    out = b"\x89PNG\r\n\x1a\n" + _chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, 8, 6, 0, 0, 0))
    out += _chunk(b"gaPd", bytes(range(pad)))
    at, pos = [], 0
    for n in list(lengths) + [len(z)]:
        n = min(n, len(z) - pos)
        at.append((len(out) + 8, n))
        out += _chunk(b"IDAT", z[pos:pos + n])
        pos += n
        if pos == len(z):
            break
    return out + (_chunk(b"IEND", b"") if iend else b""), at


def _counters(ik):
    n = (ctypes.c_ulonglong * 2)()
    assert ik.ik_png_counters(n) == 0
    return n[0], n[1]


@pytest.fixture(scope="module")
def gpu_png(ik):
    assert ik.ik_set_png_gpu_min(0) == 0  # every PNG through the GPU path
    yield ik
    ik.ik_set_png_gpu_min(256 << 10)


def _decode_batch(ik, files):
    """ik_decode_batch: (rc, last error, [status], [pixels or None], counters' move)"""
    n = len(files)
    ptrs = (ctypes.c_void_p * n)(*[ctypes.cast(ctypes.c_char_p(x), ctypes.c_void_p) for x in files])
    lens = (ctypes.c_size_t * n)(*[len(x) for x in files])
    outs, fmts, status = (ctypes.c_void_p * n)(), (ctypes.c_int * n)(), (ctypes.c_int * n)()
    g0, h0 = _counters(ik)
    rc = ik.ik_decode_batch(ptrs, lens, n, outs, fmts, status)
    err = _lib.last_error() if rc else ""
    g1, h1 = _counters(ik)
    px = [DynamicImage(outs[i]).to_array().reshape(H, W, 4) if outs[i] else None for i in range(n)]
    return rc, err, [status[i] for i in range(n)], px, (g1 - g0, h1 - h0)


def _device_equals_host(files):
    """the same files as DeviceBytes (each its own allocation of exactly len bytes) and as
    host bytes give the same WebP bytes or fail alike, item by item"""
    n = len(files)
    args = ([(W, H)] * n, [ImageFormat.webp] * n, [80] * n)
    want = []
    for f in files:
        try:
            want.append(transform_batch([f], args[0][:1], args[1][:1], args[2][:1], filter=1)[0])
        except TransformError:
            want.append(None)
    p = transform_batch_submit_device([DeviceBytes(f) for f in files], *args, filter=1)
    try:
        got = p.wait()
    except TransformError:
        got = None
    st = [p._status[i] for i in range(n)]
    assert [s != 0 for s in st] == [w is None for w in want]
    if got is None:  # (a failing item: read the others in a batch without it)
        ok = [i for i in range(n) if want[i] is not None]
        if ok:
            again = transform_batch_submit_device([DeviceBytes(files[i]) for i in ok], [(W, H)] * len(ok),
                                                  [ImageFormat.webp] * len(ok), [80] * len(ok), filter=1).wait()
            assert again == [want[i] for i in ok]
    else:
        assert got == want
    return want


def _sweep_files(z):
    # file a: source misalignment (53 + a) & 15 at the first payload byte; the lengths
    # rotated so each meets several source and destination misalignments over the files
    return [_file(z, LENGTHS[a % len(LENGTHS):] + LENGTHS[:a % len(LENGTHS)], a)[0] for a in range(16)]


def test_alignment_sweep_host_inputs(gpu_png, src):
    img, z = src
    files = _sweep_files(z)
    assert sorted((f.index(b"IDAT") + 4) & 15 for f in files) == list(range(16))
    for f in files[:2]:
        np.testing.assert_array_equal(np.asarray(Image.open(io.BytesIO(f))), img)
    rc, err, st, px, moved = _decode_batch(gpu_png, files)
    assert rc == 0 and st == [0] * 16, err
    assert moved == (16, 0), "a good file went to the host decoder (a piece CRC is wrong?)"
    for p in px:
        np.testing.assert_array_equal(p, img)


def test_alignment_sweep_device_inputs(gpu_png, src):
    _, z = src
    g0, h0 = _counters(gpu_png)
    want = _device_equals_host(_sweep_files(z))
    g1, h1 = _counters(gpu_png)
    assert None not in want
    assert (g1 - g0, h1 - h0) == (32, 0)  # 16 host-input calls and the device batch, all on the GPU


@pytest.mark.parametrize("name", ["one_byte_chunks", "zero_length_idat", "three_pieces_and_a_bit"])
def test_degenerate_splits(gpu_png, src, name):
    img, z = src
    if name == "one_byte_chunks":
        # a stream of its own, short enough for some hundred 1-byte chunks throughout
        small = np.ascontiguousarray(img[:8, :16])
        zz = zlib.compress(b"".join(b"\0" + small[y].tobytes() for y in range(8)), 0)
        assert 300 < len(zz) < 800
        f = (b"\x89PNG\r\n\x1a\n" + _chunk(b"IHDR", struct.pack(">IIBBBBB", 16, 8, 8, 6, 0, 0, 0)) +
             b"".join(_chunk(b"IDAT", zz[i:i + 1]) for i in range(len(zz))) + _chunk(b"IEND", b""))
        g0, h0 = _counters(gpu_png)
        got, _ = decode_image(f)
        g1, h1 = _counters(gpu_png)
        assert (g1 - g0, h1 - h0) == (1, 0)
        np.testing.assert_array_equal(got.to_array().reshape(small.shape), np.asarray(Image.open(io.BytesIO(f))))
        np.testing.assert_array_equal(got.to_array().reshape(small.shape), small)
        return
    lengths = [777, 0, 5, 0, 0, 4099] if name == "zero_length_idat" else [3, 3 * PIECE + 11]
    f, at = _file(z, lengths, 3)
    assert [n for _, n in at][:len(lengths)] == lengths
    np.testing.assert_array_equal(np.asarray(Image.open(io.BytesIO(f))), img)
    rc, err, st, px, moved = _decode_batch(gpu_png, [f])
    assert rc == 0 and moved == (1, 0), err
    np.testing.assert_array_equal(px[0], img)
    _device_equals_host([f])


def _flip(f, at, bit=0x10):
    b = bytearray(f)
    b[at] ^= bit
    return bytes(b)


def test_crc_detection(gpu_png, src):
    """One file per flipped bit, all in one batch with the intact file first and last: for
    each chunk-length class the payload's first and last byte, the bytes either side of a
    tile boundary and of a piece boundary where the chunk has them, and a bit of the stored
    CRC.  Expected from the file itself: zlib.crc32 over the chunk no longer equals the
    stored CRC, for which png (and the parent build) reports a CRC error for that file."""
    img, z = src
    f, at = _file(z, LENGTHS, 5)
    bad = []
    for off, n in at:
        where = {0, n - 1} | {p for p in (TILE - 1, TILE, PIECE - 1, PIECE, 2 * PIECE - 1, 2 * PIECE) if p < n}
        # (pieces are counted from the chunk's first byte; the kernel counts a piece's spans
        # back from its last granule: the bytes either side of that granule's first byte and
        # of the span boundary 1 KiB before it as well)
        g = n - 1 - ((off + n - 1) & 15)
        where |= {p for p in (g - 1, g, g - TILE + 15, g - TILE + 16) if 0 <= p < n}
        for p in sorted(where):
            bad.append(_flip(f, off + p))
        bad.append(_flip(f, off + n + 2, 0x01))  # the stored CRC
    for b in bad:  # the expectation, from zlib
        k = 8
        mism = 0
        while k + 12 <= len(b):
            ln = struct.unpack(">I", b[k:k + 4])[0]
            mism += (zlib.crc32(b[k + 4:k + 8 + ln]) & 0xFFFFFFFF) != struct.unpack(">I", b[k + 8 + ln:k + 12 + ln])[0]
            k += 12 + ln
        assert mism == 1
    rc, err, st, px, moved = _decode_batch(gpu_png, [f] + bad + [f])
    assert rc != 0 and "crc" in err.lower()
    assert st[0] == 0 and st[-1] == 0, "the unmodified file must pass"
    np.testing.assert_array_equal(px[0], img)
    np.testing.assert_array_equal(px[-1], img)
    missed = [i for i, s in enumerate(st[1:-1]) if s == 0]
    assert not missed, f"corrupt files accepted: {missed}"
    assert moved == (2, len(bad))
    # one of them alone: png's error through decode_image
    with pytest.raises(TransformError) as ei:
        decode_image(bad[len(bad) // 2])
    assert "crc" in str(ei.value).lower() or "Png" in str(ei.value)


def test_batch_isolation(gpu_png, src):
    """A corrupt file between good ones: its pieces follow the first file's last piece and
    precede the third file's first in the plan, and the streams are neighbours in the
    stream area.  Only its own result is an error."""
    img, z = src
    a, _ = _file(z, [17, 1025], 1)
    b, at = _file(z, [5, PIECE + 1], 9)
    c, _ = _file(z, [1, 1, 1], 14)
    off, n = at[-1]
    files = [a, _flip(b, off + n - 1), c, _flip(b, at[0][0]), a]
    rc, err, st, px, moved = _decode_batch(gpu_png, files)
    assert rc != 0 and "crc" in err.lower()
    assert [s != 0 for s in st] == [False, True, False, True, False]
    assert moved == (3, 2)
    for i in (0, 2, 4):
        np.testing.assert_array_equal(px[i], img)
    want = _device_equals_host(files)
    assert [w is None for w in want] == [False, True, False, True, False]


def test_device_input_ends_with_its_allocation(gpu_png, src):
    """DeviceBytes allocates exactly len bytes.  With IEND the last payload byte is 17 bytes
    before the allocation's end; without it (the file cut after the last IDAT's CRC) it is
    5 bytes before, inside the last 16 -- whatever the host-input path makes of that file,
    the device-input path makes the same.  The last chunk's length moves the payload's end
    over the granule's sixteen positions."""
    _, z = src
    files = []
    for k in range(16):
        files.append(_file(z, [len(z) - 40 - k], k)[0])
        files.append(_file(z, [len(z) - 40 - k], k, iend=False)[0])
    assert len({(len(f) - 5) & 15 for f in files[1::2]}) > 8
    want = _device_equals_host(files)
    assert None not in want[0::2]
