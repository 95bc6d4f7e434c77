"""GPU: the PNG kernel stage's second decode round, and one thread decoding on two
devices in turn.

A second round needs a lane that overflows its first token region.  Bytes of two
values compressed with Z_HUFFMAN_ONLY give a stream of literals alone at 1-2 bits each
(a block's code has three symbols: 0, 255, end of block), so one token per inflated
byte and more than half a token per compressed bit, against a first region of 3/8
(wave decoder) or 1/4 (lane decoder) token per bit: every lane overflows and decodes
again in the region sized by the exact bound.  The capacities are restated from
ik_png_wave.h region_capacity / ik_inflate.h tok_capacity and the inequality is
asserted for every lane length before any decode."""
import ctypes
import io
import os
import struct
import subprocess
import sys
import zlib

import numpy as np
import pytest
from PIL import Image

import ikutil
import png_adam7_util as A7
from imagekit import _lib, decode_image, decode_image_batch

pytestmark = pytest.mark.gpu

WINDOW_BITS, SUB = 8 * 10496, 64          # ik_png_wave.h kWindowBits, kSub
CHUNK_BITS = {"wave": 8 * 65536, "lane": 8 * 16384}  # ik_png.h kPngWaveChunkBytes, kPngChunkBytes


def region_capacity(bits):
    """ik_png_wave.h region_capacity(bits, false): a wave lane's first token region."""
    slack = (bits // WINDOW_BITS + 2) * (48 * SUB) + 64
    return (bits // 8 * 3 + slack + 7) & ~7


def tok_capacity(bits):
    """ik_inflate.h tok_capacity(bits, false): the lane decoder's."""
    return (bits // 4 + 2 * 128 + 64 + 7) & ~7


CAPACITY = {"wave": region_capacity, "lane": tok_capacity}


def two_valued_png(w, h, seed):
    """Gray8, every byte 0 or 255, filter type 0 on every row, Huffman-only DEFLATE."""
    px = ((ikutil.splitmix64(0x2B17 + seed, w * h) >> np.uint64(17)) & np.uint64(1)).astype(np.uint8) * 255
    px = px.reshape(h, w)
    raw = b"".join(b"\0" + px[y].tobytes() for y in range(h))
    co = zlib.compressobj(6, zlib.DEFLATED, 15, 8, zlib.Z_HUFFMAN_ONLY)
    z = co.compress(raw) + co.flush()
    png = (b"\x89PNG\r\n\x1a\n" + A7.chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 0, 0, 0, 0)) + A7.chunk(b"IDAT", z) +
           A7.chunk(b"IEND", b""))
    return px[..., None], png, len(raw), len(z)


def noise_rgba_png():
    """The batch's other stream, 640 x 480 RGBA8 noise.  The token area holds half again
    what the first round's regions take (png_plan_work), and the two-valued stream's
    second regions (a token per bit) come out of that half: 1.2 MB of incompressible
    stream beside it leaves room for them with either decoder, where a stream that
    compresses well would send the two-valued one to the host decoder ("token area
    full") and the second round would go untested."""
    rgba = ikutil.synth(640, 480, 4, seed=31, pattern="N", alpha="random")
    b = io.BytesIO()
    Image.fromarray(rgba, "RGBA").save(b, format="PNG")
    assert len(A7.idat_bytes(b.getvalue())) > 1200000
    return rgba, b.getvalue()


def assert_every_lane_overflows(raw_len, zlen, decoder):
    """One token per inflated byte; a literal costs at most 2 bits, so a lane of b bits
    holds at least b / 2 tokens less its blocks' headers (a three-symbol code's header is
    under 200 bits, a block holds 16,383 literals: under 1 % of a block).  A lane runs
    from a block start near a search chunk's start to the next chunk's: about a chunk,
    and the last one whatever is left; and the whole stream as a single lane."""
    nbits = 8 * zlen
    assert nbits <= 2 * raw_len, "the literals must cost 2 bits at most"
    cap, cbits = CAPACITY[decoder], CHUNK_BITS[decoder]
    assert raw_len > cap(nbits), (raw_len, cap(nbits))
    nchunks = (nbits - 16 + cbits - 1) // cbits
    for b in [cbits] * (nchunks - 1) + [nbits - 16 - (nchunks - 1) * cbits]:
        least = b // 2 - b // 100 - 200
        assert least > cap(b), (decoder, b, least, cap(b))
    return nchunks


@pytest.fixture(scope="module")
def streams():
    big = two_valued_png(1024, 768, 1)
    small = two_valued_png(256, 256, 2)
    return {"big": big, "small": small, "rgba": noise_rgba_png()}


def test_the_streams_force_a_second_round(streams):
    _, _, raw_len, zlen = streams["big"]
    assert raw_len == 787200
    assert assert_every_lane_overflows(raw_len, zlen, "wave") == 3  # three 64 KiB search chunks
    assert assert_every_lane_overflows(raw_len, zlen, "lane") >= 3
    _, _, raw_len, zlen = streams["small"]
    assert raw_len == 65792
    assert assert_every_lane_overflows(raw_len, zlen, "wave") == 1
    assert_every_lane_overflows(raw_len, zlen, "lane")


@pytest.fixture
def gpu_png(ik):
    assert ik.ik_set_png_gpu_min(0) == 0  # every PNG through the GPU path
    yield ik
    ik.ik_set_png_gpu_min(256 << 10)


def counters(ik):
    c = (ctypes.c_ulonglong * 2)()
    assert ik.ik_png_counters(c) == 0
    return c[0], c[1]


def decode_rounds(ik):
    t = (ctypes.c_double * 17)()
    assert ik.ik_png_last_timing(t, 17) == 0
    return t[7]


@pytest.mark.parametrize("which", ["big", "small"])
def test_second_decode_round(gpu_png, streams, which):
    src, png, raw_len, zlen = streams[which]
    assert_every_lane_overflows(raw_len, zlen, "wave")
    rgba, rgba_png = streams["rgba"]
    g0, h0 = counters(gpu_png)
    got = decode_image_batch([png, rgba_png])
    g1, h1 = counters(gpu_png)
    np.testing.assert_array_equal(got[0][0].to_array(), src)
    np.testing.assert_array_equal(got[1][0].to_array(), rgba)
    assert (g1 - g0, h1 - h0) == (2, 0), "both streams must decode on the GPU path"
    assert decode_rounds(gpu_png) >= 2


_LANE_CHILD = r"""
import ctypes, sys
import numpy as np
sys.path[:0] = [%(pkg)r, %(tests)r]
import test_gpu_png_rounds as R
from imagekit import _lib, decode_image_batch
lib = _lib.load()
assert lib.ik_init(0) == 0
assert lib.ik_set_png_gpu_min(0) == 0
src, png, raw_len, zlen = R.two_valued_png(1024, 768, 1)
R.assert_every_lane_overflows(raw_len, zlen, "lane")
rgba, rgba_png = R.noise_rgba_png()
g0 = R.counters(lib)
got = decode_image_batch([png, rgba_png])
g1 = R.counters(lib)
assert (g1[0] - g0[0], g1[1] - g0[1]) == (2, 0), (g0, g1)
assert np.array_equal(got[0][0].to_array(), src)
assert np.array_equal(got[1][0].to_array(), rgba)
assert R.decode_rounds(lib) >= 2, R.decode_rounds(lib)
print("lane-ok")
"""


def test_second_round_of_the_lane_decoder_in_a_child_process(ik):
    """IK_PNG_DECODE=lane is read once per process, so a fresh child."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = _LANE_CHILD % {"pkg": os.path.join(root, "rust-image-transform_amd"), "tests": os.path.join(root, "tests")}
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, IK_PNG_DECODE="lane"), capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0 and "lane-ok" in r.stdout, r.stdout + r.stderr


def test_two_devices_from_one_thread(gpu_png):
    """The unfilter's fork / join events belong to the device they record on: a thread
    that decoded on device 0 decodes on device 1 and on device 0 again.  Paeth rows send
    the diagonal unfilter kernel to the side stream."""
    if gpu_png.ik_device_count() < 2:
        pytest.skip("one GPU on this machine")
    src = ikutil.synth(640, 480, 4, seed=33, pattern="N", alpha="random")
    png = A7.make_png(src, 6, 8, interlace=0, filt=4)
    try:
        for device in (0, 1, 0):
            assert gpu_png.ik_init(device) == 0, _lib.last_error()
            g0, h0 = counters(gpu_png)
            d, _ = decode_image(png)
            g1, h1 = counters(gpu_png)
            np.testing.assert_array_equal(d.to_array(), src)
            assert (g1 - g0, h1 - h0) == (1, 0), f"device {device}: the stream must decode on the GPU path"
    finally:
        assert gpu_png.ik_init(0) == 0
