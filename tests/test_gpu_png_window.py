"""GPU: the wave decoder's stream window (wave::kWindowBits, ik_png_wave.h) at its edges.

k_png_wave stages a block's body in LDS window by window; the window's size is set
by the LDS budget of a CU shared with the WebP coder.  These streams
are made so that, at the window size the header states, block bodies

  a  fit one window with a few bytes to spare,
  b  end within the last 32 bits of a window / just past a window's edge (the final
     sub-lane's warm-up and EXIT, a block end right after an edge),
  c  span three or more windows (noise at Z_HUFFMAN_ONLY and at level 1, stored blocks),
  d  are much smaller than a window (Z_FULL_FLUSH every 300 bytes),
  e  use the fixed codes and cross a window edge.

The block extents are not guessed: `deflate_blocks` walks each stream (a plain
DEFLATE symbol walk) and every case asserts its property on the extents it finds.
Bar: the pixels equal Pillow's decode (libpng + zlib) and the source, and every
stream is decoded by the GPU path (ik_png_counters).  One batch of 8 such streams
goes through ik_transform_batch with the exact GPU WebP coder, two batches in
flight, so decoder and coder run side by side: bytes == libwebp's."""
import ctypes
import io
import os
import re
import struct
import zlib

import numpy as np
import pytest
from PIL import Image

import ikutil
from deflate_writer import deflate_blocks  # the block walk (RFC 1951), grown into a token walker there
from imagekit import ImageFormat, decode_image, transform_batch, transform_batch_submit

pytestmark = pytest.mark.gpu

_HDR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "rust-image-transform_amd", "csrc",
                    "ik_png_wave.h")


def window_bits():
    """wave::kWindowBits as the header states it (the tests follow the window's size)"""
    m = re.search(r"#define\s+IK_WAVE_WINDOW_BYTES\s+(\d+)", open(_HDR).read())
    assert m, "ik_png_wave.h no longer defines IK_WAVE_WINDOW_BYTES"
    return 8 * int(m.group(1))


W = window_bits()

# ---- the streams ----
def _chunk(t, d):
    return struct.pack(">I", len(d)) + t + d + struct.pack(">I", zlib.crc32(t + d) & 0xFFFFFFFF)


def _raw(img):  # filter type 0 on every row: the stream's bytes are the image's
    h, w, c = img.shape
    return b"".join(b"\0" + img[y].tobytes() for y in range(h))


def _png(img, z):
    h, w, c = img.shape
    ihdr = struct.pack(">IIBBBBB", w, h, 8, {3: 2, 4: 6}[c], 0, 0, 0)
    return b"\x89PNG\r\n\x1a\n" + _chunk(b"IHDR", ihdr) + _chunk(b"IDAT", z) + _chunk(b"IEND", b"")


def _noise(w, h, c, seed, levels):
    return np.random.default_rng(seed).integers(0, levels, size=(h, w, c), dtype=np.uint8)


def _co(level=6, strategy=zlib.Z_DEFAULT_STRATEGY):
    # memLevel 9: a block holds up to 32 K symbols (8: 16 K), so zlib's symbol buffer
    # does not end the block before the test does
    return zlib.compressobj(level, zlib.DEFLATED, 15, 9, strategy)


def _first_block_of(raw, lo, hi):
    """A Z_HUFFMAN_ONLY stream of raw whose first block's body holds lo..hi bits (the
    block is ended by a Z_FULL_FLUSH after as many bytes as that takes)."""
    def make(n):
        co = _co(6, zlib.Z_HUFFMAN_ONLY)
        z = co.compress(raw[:n]) + co.flush(zlib.Z_FULL_FLUSH) + co.compress(raw[n:]) + co.flush()
        b = deflate_blocks(z, 1)[0]
        return z, b[3] - b[2]

    n = (lo + hi) // 2 // 6
    for _ in range(60):
        z, got = make(n)
        if lo <= got <= hi:
            return z
        step = int(((lo + hi) / 2 - got) * n / got)
        n += step if step else (1 if got < lo else -1)
        assert 0 < n < len(raw), "the image is too small for this block"
    raise AssertionError(f"no first block of {lo}..{hi} bits found")


def _body_bits(b):
    return b[3] - b[2]


def _case(name, c):
    """(image, zlib stream, check(blocks)): the stream of case `name` with c channels"""
    seed = sum(map(ord, name)) * 8 + c
    if name in ("fits", "ends_at_edge", "ends_past_edge"):
        img = _noise(96 if c == 4 else 128, 96, c, seed, 64)  # 64 levels: ~6 bits per byte, a dynamic code
        lo, hi = {"fits": (W - 128, W - 33), "ends_at_edge": (W - 31, W), "ends_past_edge": (W + 1, W + 256)}[name]
        z = _first_block_of(_raw(img), lo, hi)

        def check(bl):
            assert bl[0][0] == 2 and lo <= _body_bits(bl[0]) <= hi, bl[0]
        return img, z, check
    if name in ("three_windows_huffman", "three_windows_level1"):
        # 512x384 RGB is the largest shape; the RGBA frame is the smallest that holds the block
        # (192 levels: ~7.6 bits per byte, so zlib codes the block and does not store it)
        img = _noise(*((512, 384) if c == 3 else (160, 120)), c, seed, 192)
        co = _co(6, zlib.Z_HUFFMAN_ONLY) if name.endswith("huffman") else _co(1)
        z = co.compress(_raw(img)) + co.flush()

        def check(bl):
            assert bl[0][0] == 2 and _body_bits(bl[0]) > 2 * W, (bl[0], W)
        return img, z, check
    if name == "stored":
        img = _noise(160, 120, c, seed, 256)
        z = zlib.compress(_raw(img), 0)

        def check(bl):
            assert all(b[0] == 0 for b in bl) and _body_bits(bl[0]) > 2 * W, bl[0]
        return img, z, check
    if name == "tiny_blocks":
        img = ikutil.synth(96, 96, c, seed=seed, pattern="S")
        raw, co, z = _raw(img), _co(6), b""
        for i in range(0, len(raw), 300):
            z += co.compress(raw[i:i + 300]) + co.flush(zlib.Z_FULL_FLUSH)
        z += co.flush()

        def check(bl):
            coded = [b for b in bl if b[0] != 0]
            assert len(coded) >= 90 and max(map(_body_bits, coded)) < W // 16, len(coded)
        return img, z, check
    if name == "fixed_codes":
        img = ikutil.synth(256, 192, c, seed=seed, pattern="S")
        co = _co(6, zlib.Z_FIXED)
        z = co.compress(_raw(img)) + co.flush()

        def check(bl):
            assert all(b[0] == 1 for b in bl) and max(map(_body_bits, bl)) > W, [b[0] for b in bl]
        return img, z, check
    raise KeyError(name)


CASES = ["fits", "ends_at_edge", "ends_past_edge", "three_windows_huffman", "three_windows_level1", "stored",
         "tiny_blocks", "fixed_codes"]
# the extents that decide a case lie in its first block, except where every block counts
_WHOLE = {"stored", "tiny_blocks", "fixed_codes"}
_made = {}


def case(name, c):
    """(image, PNG file), made once; the case's property is asserted on the walked extents"""
    if (name, c) not in _made:
        img, z, check = _case(name, c)
        check(deflate_blocks(z, None if name in _WHOLE else 1))
        _made[name, c] = (img, _png(img, z))
    return _made[name, c]


def _counters(ik):
    n = (ctypes.c_ulonglong * 2)()
    assert ik.ik_png_counters(n) == 0
    return n[0], n[1]


@pytest.fixture(scope="module")
def gpu_png(ik):
    assert ik.ik_set_png_gpu_min(0) == 0  # every PNG through the GPU path
    yield ik
    ik.ik_set_png_gpu_min(256 << 10)


@pytest.mark.parametrize("c", [4, 3])
@pytest.mark.parametrize("name", CASES)
def test_window_case(gpu_png, name, c):
    img, data = case(name, c)
    pil = np.asarray(Image.open(io.BytesIO(data)))
    np.testing.assert_array_equal(pil, img)
    g0, h0 = _counters(gpu_png)
    got, fmt = decode_image(data)
    g1, h1 = _counters(gpu_png)
    assert fmt is None
    np.testing.assert_array_equal(got.to_array(), pil)
    assert (g1 - g0, h1 - h0) == (1, 0), "the stream must be decoded by the GPU path"


def test_window_streams_beside_the_exact_coder(gpu_png, oracle):
    """8 of the streams per batch, WebP out of the exact GPU coder (AUTO keeps batches
    under 32 frames on libwebp: encoder 2), two batches in flight: the second batch's
    k_png_wave runs beside the first's k_vp8x_run."""
    picks = [(n, 4 if i % 2 == 0 else 3) for i, n in enumerate(CASES)]
    made = [case(n, c) for n, c in picks]
    datas = [d for _, d in made]
    n = len(datas)
    sizes, fmts, qs = [(64, 64)] * n, [ImageFormat.webp.value] * n, [80] * n
    prev = gpu_png.ik_get_webp_encoder()
    try:
        assert gpu_png.ik_set_webp_encoder(0) == 0
        ref = transform_batch(datas, sizes, fmts, qs, filter=ikutil.TRIANGLE)
        assert gpu_png.ik_set_webp_encoder(2) == 0
        g0, h0 = _counters(gpu_png)
        pa = transform_batch_submit(datas, sizes, fmts, qs, filter=ikutil.TRIANGLE, threads=8)
        pb = transform_batch_submit(datas[::-1], sizes, fmts, qs, filter=ikutil.TRIANGLE, threads=8)
        ga, gb = pa.wait(), pb.wait()
        g1, h1 = _counters(gpu_png)
    finally:
        gpu_png.ik_set_webp_encoder(prev)
    assert (g1 - g0, h1 - h0) == (2 * n, 0), "every stream must be decoded by the GPU path"
    for i, (img, _) in enumerate(made):
        want, _ = oracle.transform(img, 64, 64, ikutil.TRIANGLE, ImageFormat.webp.value, 80)
        assert ref[i] == want, f"{picks[i]}: libwebp path differs from the oracle's transform"
        assert ga[i] == ref[i], f"{picks[i]}: exact coder's bytes differ from libwebp's"
        assert gb[n - 1 - i] == ref[i], f"{picks[i]} (second batch): exact coder's bytes differ from libwebp's"
