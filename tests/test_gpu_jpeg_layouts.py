"""GPU: decode_image on JPEG layouts Pillow's writer cannot produce.

Every other JPEG the suite decodes comes out of PIL.Image.save: 4:4:4 / 4:2:2 /
4:2:0, one interleaved scan, Annex K (or, progressive, libjpeg's optimised)
Huffman tables, 8-bit quantisation tables, JFIF.  The files here come from
tests/jpeg_writer.py (tests/test_jpeg_writer.py makes them trustworthy on a CPU:
Pillow opens each, the libjpeg-mode oracle equals Pillow on each):

- samplings 4:4:0 (the h1v2 branches of ik_jpeg.hip upsampled() and
  upsampled_zune()), 4:1:1 and 3x1 (replication; a 4x1 luma grid), 4:1:0 (ten
  blocks per MCU, jsync::kMaxBPM), 2x2/2x1/1x1 (chroma planes of different size:
  color_fast_ok false), luma below the maximum factors, gray declared 2x2;
- Huffman tables built from the file's statistics or skewed to 15/16-bit codes,
  with tables of their own for Cb and Cr; Pillow's optimize=True files;
- baseline files of several scans (the host entropy decoder, by design: scan()
  sends an image with a second scan there);
- progressive by spectral selection and with DC successive approximation, with
  restart intervals (k_jpeg_prog) and without (host);
- fill bytes, stray segments, several tables per segment, bytes after EOI, RSTn
  wrapping; Adobe transform 0 and 1; SOF1; 16-bit quantisation entries above 255.

Bar, per file: the libjpeg-turbo mode equals Pillow bit for bit, the default
zune-jpeg mode equals the oracle's restatement bit for bit, and ik_jpeg_counters
shows the entropy decoding ran where the design says (the self-synchronising GPU
decoder for one interleaved scan of 4 KiB and up, k_jpeg_prog for progressive
scans with restart intervals, the host otherwise)."""
import ctypes
import io

import numpy as np
import pytest
from PIL import Image

import ikutil
import jpeg_writer as jw
from imagekit import ImageFormat, decode_image, decode_image_batch

pytestmark = pytest.mark.gpu

LIBJPEG, ZUNE = 0, 1
MOVED = {"gpu": (1, 0), "host": (0, 1)}


def _counts(ik):
    c = (ctypes.c_ulonglong * 2)()
    assert ik.ik_jpeg_counters(c) == 0
    return c[0], c[1]


def _pillow(data):
    im = Image.open(io.BytesIO(data))
    return np.asarray(im if im.mode in ("RGB", "L") else im.convert("RGB"))


def _check(ik, oracle, data, where):
    """Both reconstructions of one file, and where its entropy decoding was counted."""
    assert ik.ik_get_jpeg_reconstruction() == ZUNE  # the default
    c0 = _counts(ik)
    img, fmt = decode_image(data)
    c1 = _counts(ik)
    assert fmt is ImageFormat.jpeg
    want = oracle.jpeg_decode(data, ZUNE)
    np.testing.assert_array_equal(img.to_array(), want)
    assert (c1[0] - c0[0], c1[1] - c0[1]) == MOVED[where]
    assert ik.ik_set_jpeg_reconstruction(LIBJPEG) == 0
    try:
        lj, _ = decode_image(data)
        c2 = _counts(ik)
    finally:
        assert ik.ik_set_jpeg_reconstruction(ZUNE) == 0
    np.testing.assert_array_equal(lj.to_array(), _pillow(data).reshape(want.shape))
    assert (c2[0] - c1[0], c2[1] - c1[1]) == MOVED[where]


@pytest.mark.parametrize("name", [c.name for c in jw.CASES])
def test_layout_equals_pillow_and_the_zune_restatement(ik, oracle, name):
    c, f = jw.BY_NAME[name], jw.build(name)
    if c.where == "gpu" and c.kw.get("sof", jw.SOF0) != jw.SOF2:
        assert len(f.scan_bytes) == 1 and len(f.scan_bytes[0]) >= 4096  # the self-synchronising decoder's
    _check(ik, oracle, f.data, c.where)


@pytest.mark.parametrize("sub", [0, 1, 2])
def test_pillow_optimised_baseline_tables(ik, oracle, sub):
    """Baseline with libjpeg's optimised Huffman tables (optimize=True): the only
    tables other than Annex K's that Pillow writes into a baseline file."""
    buf = io.BytesIO()
    Image.fromarray(ikutil.synth(203, 149, 3, seed=70 + sub, pattern="N")).save(buf, format="JPEG", quality=95,
                                                                              subsampling=sub, optimize=True)
    data = buf.getvalue()
    assert b"\xff\xc0" in data and len(data) >= 8192
    _check(ik, oracle, data, "gpu")


BATCH = ["440_big", "410_big_dri5", "411_tiny", "221_big", "low_big_dri5", "gray22_big", "311_big", "440_long_dri5",
         "420_scan_per_comp", "440_prog_dcapprox_dri3", "pq1_big", "adobe0_420_big", "410_1x1", "fill_big"]


def test_mixed_layouts_in_one_batch(ik, oracle):
    """Several layouts in one decode_image_batch call (the self-synchronising
    decoder takes its share of them in one launch): each image equals its own
    single-image answer, in both reconstructions."""
    blobs = [jw.build(n).data for n in BATCH]
    assert ik.ik_get_jpeg_reconstruction() == ZUNE
    out = decode_image_batch(blobs)
    for (img, fmt), b, n in zip(out, blobs, BATCH):
        assert fmt is ImageFormat.jpeg
        np.testing.assert_array_equal(img.to_array(), decode_image(b)[0].to_array(), err_msg=n)
        np.testing.assert_array_equal(img.to_array(), oracle.jpeg_decode(b, ZUNE), err_msg=n)
    assert ik.ik_set_jpeg_reconstruction(LIBJPEG) == 0
    try:
        out = decode_image_batch(blobs)
    finally:
        assert ik.ik_set_jpeg_reconstruction(ZUNE) == 0
    for (img, _), b, n in zip(out, blobs, BATCH):
        a = img.to_array()
        np.testing.assert_array_equal(a, _pillow(b).reshape(a.shape), err_msg=n)
