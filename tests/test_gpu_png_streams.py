"""GPU: PNG inflate (k_png_find, k_png_wave, k_png_expand8, k_png_resolve; k_png_decode
under IK_PNG_DECODE=lane) on DEFLATE streams zlib cannot write.

Every other PNG test feeds the decoder zlib's streams.  deflate_streams.py holds the
ones a non-zlib writer sends: match distances 32507..32768 (also as a block's, lane's
and expand unit's first token: window marker index 0), steps of exactly 48 bits back
to back (the cursor's refill at its limit), blocks of slow-path codes, a two-literal
table entry beside slow codes, a distance code of one code and of none, HCLEN 5 / 19,
HLIT 286, HDIST 30, lengths sent without repeat codes, length 258 as 284 + 31, stored
blocks of 0 and 65535 bytes after each end-bit phase, every block type in one lane,
600 empty blocks in a row.  Each case's property is asserted on the walked stream
(test_deflate_writer.py, CPU), and the CPU model runs them in test_png_streams_model.py.

Bar: pixels equal to Pillow's (libpng + zlib) and the source, decoded by the GPU path
(ik_png_counters moves by (1, 0): a valid stream on the host decoder is a bug).  The
streams zlib rejects raise TransformError, and in a batch fail their own slot only."""
import ctypes
import io
import os
import subprocess
import sys

import numpy as np
import pytest
from PIL import Image

import deflate_streams as ds
from imagekit import TransformError, _lib, decode_image, decode_image_batch
from imagekit.transform import DynamicImage

pytestmark = pytest.mark.gpu

EXPECTED_FALLBACK = ds.EXPECTED_FALLBACK  # (the one set, deflate_streams.py; asserted exactly below)


def _counters(ik):
    n = (ctypes.c_ulonglong * 2)()
    assert ik.ik_png_counters(n) == 0
    return n[0], n[1]


@pytest.fixture(scope="module")
def gpu_png(ik):
    assert ik.ik_set_png_gpu_min(0) == 0  # every PNG through the GPU path
    yield ik
    ik.ik_set_png_gpu_min(256 << 10)


@pytest.fixture(scope="module")
def pillow():
    """Pillow's pixels of every valid case's file (made once)"""
    return {n: np.asarray(Image.open(io.BytesIO(ds.valid(n).png))).reshape(ds.valid(n).img.shape) for n in ds.VALID}


def _pixels(d, like):
    return d.to_array().reshape(like.shape)


@pytest.mark.parametrize("name", ds.VALID)
def test_valid_stream(gpu_png, pillow, name):
    c = ds.valid(name)
    np.testing.assert_array_equal(pillow[name], c.img)
    g0, h0 = _counters(gpu_png)
    got, fmt = decode_image(c.png)
    g1, h1 = _counters(gpu_png)
    assert fmt is None
    np.testing.assert_array_equal(_pixels(got, c.img), pillow[name])
    assert ((g1 - g0, h1 - h0) == (0, 1)) == (name in EXPECTED_FALLBACK), "the stream must be decoded by the GPU path"
    assert (g1 - g0) + (h1 - h0) == 1


def _batch(gpu_png, pillow, names):
    """the named cases in one decode_image_batch: every image equals its single decode and
    Pillow's; returns how the counters moved"""
    single = {n: _pixels(decode_image(ds.valid(n).png)[0], ds.valid(n).img) for n in names}
    g0, h0 = _counters(gpu_png)
    got = decode_image_batch([ds.valid(n).png for n in names])
    g1, h1 = _counters(gpu_png)
    for n, (d, _) in zip(names, got):
        np.testing.assert_array_equal(_pixels(d, ds.valid(n).img), single[n])
        np.testing.assert_array_equal(single[n], pillow[n])
    return g1 - g0, h1 - h0


def test_valid_streams_in_one_batch(gpu_png, pillow):
    """Every case that decodes on the GPU alone does so in a batch: exactly (n, 0)."""
    names = [n for n in ds.VALID if n not in EXPECTED_FALLBACK]
    assert _batch(gpu_png, pillow, names) == (len(names), 0)


def test_all_valid_streams_in_one_batch(gpu_png, pillow):
    """All cases together, the expected fallback among them: exactly (n, 0).  A batch's
    streams share one token area, sized for their first-round lanes plus half; the half
    belonging to far_across_lanes' 1.5 Mbit alone (about 290,000 tokens) is several times
    what empty_blocks' eight or so split lanes take (about 10,000 tokens each), and no
    other case splits -- so here it decodes on the GPU, and no neighbour is starved."""
    assert EXPECTED_FALLBACK == {"empty_blocks"}
    assert _batch(gpu_png, pillow, list(ds.VALID)) == (len(ds.VALID), 0)


def test_split_idat(gpu_png, pillow):
    """the far-distance streams in IDAT chunks of 4093 bytes (the gather joins them)"""
    import deflate_writer as dw
    for n in ("dist_top", "far_across_lanes"):
        c = ds.valid(n)
        g0, h0 = _counters(gpu_png)
        got, _ = decode_image(dw.png(c.img, c.z, idat=4093))
        g1, h1 = _counters(gpu_png)
        np.testing.assert_array_equal(_pixels(got, c.img), pillow[n])
        assert (g1 - g0, h1 - h0) == (1, 0)


_LANE_CHILD = r"""
import ctypes, io, sys
import numpy as np
from PIL import Image
sys.path[:0] = [%(pkg)r, %(tests)r]
import ikutil
ikutil.use_pillow_codecs()
import deflate_streams as ds
from imagekit import _lib, decode_image
lib = _lib.load()
assert lib.ik_init(0) == 0
assert lib.ik_set_png_gpu_min(0) == 0
def counters():
    c = (ctypes.c_ulonglong * 2)(); lib.ik_png_counters(c); return c[0], c[1]
host = []
for n in ds.VALID:
    c = ds.valid(n)
    g0, h0 = counters()
    d, _ = decode_image(c.png)
    g1, h1 = counters()
    assert (g1 - g0) + (h1 - h0) == 1, (n, g0, h0, g1, h1)
    if h1 - h0:
        host.append(n)
    pil = np.asarray(Image.open(io.BytesIO(c.png))).reshape(c.img.shape)
    assert np.array_equal(d.to_array().reshape(c.img.shape), pil) and np.array_equal(pil, c.img), n
print("lane-host=" + ",".join(sorted(host)) + ";")
print("lane-ok")
"""


def test_overrun_below_the_gpu_threshold(ik, gpu_png):
    """A known divergence, recorded: a file below ik_set_png_gpu_min goes to the host decoder,
    which tries libdeflate first, and libdeflate clips a code-length repeat that overruns
    HLIT + HDIST where zlib (and the GPU path, test_invalid_stream) calls it an error.  Either
    answer is pinned: png's error, or the pixels of the stream with that run clipped."""
    b = ds.invalid("lengths_overrun")
    ik.ik_set_png_gpu_min(1 << 40)
    try:
        g0, h0 = _counters(ik)
        try:
            got, _ = decode_image(b.png)
        except TransformError:
            got = None
        g1, h1 = _counters(ik)
    finally:
        ik.ik_set_png_gpu_min(0)
    assert (g1 - g0, h1 - h0) == (0, 1)
    if got is not None:
        np.testing.assert_array_equal(_pixels(got, b.img), b.img)


def test_lane_decoder_in_a_child_process(ik):
    """IK_PNG_DECODE=lane (the one-thread-per-lane decoder; expand and resolve are shared):
    read once per process, so every valid case in one fresh child."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = _LANE_CHILD % {"pkg": os.path.join(root, "rust-image-transform_amd"), "tests": os.path.join(root, "tests")}
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, IK_PNG_DECODE="lane"), capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0 and "lane-ok" in r.stdout, r.stdout + r.stderr
    want = "lane-host=" + ",".join(sorted(ds.EXPECTED_FALLBACK)) + ";"
    assert want in r.stdout, r.stdout


@pytest.mark.parametrize("name", ds.INVALID)
def test_invalid_stream(gpu_png, pillow, name):
    b = ds.invalid(name)
    with pytest.raises(TransformError):
        decode_image(b.png)
    # in a batch it fails its own slot only
    left, right = ds.valid("no_dist"), ds.valid("mixed_types")
    batch = [left.png, b.png, right.png]
    n = len(batch)
    ptrs = (ctypes.c_void_p * n)(*[ctypes.cast(ctypes.c_char_p(x), ctypes.c_void_p) for x in batch])
    lens = (ctypes.c_size_t * n)(*[len(x) for x in batch])
    outs, fmts, status = (ctypes.c_void_p * n)(), (ctypes.c_int * n)(), (ctypes.c_int * n)()
    rc = gpu_png.ik_decode_batch(ptrs, lens, n, outs, fmts, status)
    assert rc != 0 and _lib.last_error()
    assert [status[i] != 0 for i in range(n)] == [False, True, False]
    assert not outs[1]
    np.testing.assert_array_equal(_pixels(DynamicImage(outs[0]), left.img), pillow["no_dist"])
    np.testing.assert_array_equal(_pixels(DynamicImage(outs[2]), right.img), pillow["mixed_types"])
