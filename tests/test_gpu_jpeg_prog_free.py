"""GPU: progressive JPEG without restart markers, entropy-decoded on the GPU behind
ik_set_jpeg_prog_free / IK_JPEG_PROG_FREE (off by default).

decode_image on such a file (reference src/transform.rs:31 -> zune-jpeg 0.4.21)
decodes every scan serially; with the switch at gpu the DC-first and AC-first
scans go through the self-synchronising decoder's launches, DC refinement is a
bit per block (k_jprog_dc_refine) and AC refinement one serial chain per
component (k_jprog_ac_chain).

Bar: with the switch at gpu every eligible file -- SOF2, no restart interval at
any scan, 4 KiB of entropy-coded bytes over its scans -- is counted GPU-decoded by
ik_jpeg_counters and equals Pillow bit for bit in libjpeg mode and the zune
restatement (oracle/jpeg_dec.c) in the default mode; smaller files, and every
file with the switch at host, are counted host-decoded; damaged files end as they
do with the switch at host, and leave the library usable."""
import ctypes
import io

import numpy as np
import pytest
from PIL import Image

import ikutil
import jpeg_prog_util as pu
from imagekit import ImageFormat, TransformError, decode_image, decode_image_batch

pytestmark = pytest.mark.gpu

LIBJPEG, ZUNE = 0, 1
HOST, GPU = 0, 1
MOVED = {"gpu": (1, 0), "host": (0, 1)}


def _counts(ik):
    c = (ctypes.c_ulonglong * 2)()
    assert ik.ik_jpeg_counters(c) == 0
    return c[0], c[1]


def _pillow(data):
    im = Image.open(io.BytesIO(data))
    return np.asarray(im if im.mode in ("RGB", "L") else im.convert("RGB"))


class _switch:
    """The switch at `where` for a block, back at the environment's value after it."""

    def __init__(self, ik, where):
        self.ik, self.where = ik, where

    def __enter__(self):
        assert self.ik.ik_set_jpeg_prog_free(self.where) == 0
        assert self.ik.ik_get_jpeg_prog_free() == self.where

    def __exit__(self, *exc):
        assert self.ik.ik_set_jpeg_prog_free(-1) == 0


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


def test_the_default_is_the_host(ik):
    assert ik.ik_set_jpeg_prog_free(-1) == 0
    assert ik.ik_get_jpeg_prog_free() == HOST


def test_setter_and_environment(ik, monkeypatch):
    try:
        assert ik.ik_set_jpeg_prog_free(GPU) == 0 and ik.ik_get_jpeg_prog_free() == GPU
        assert ik.ik_set_jpeg_prog_free(HOST) == 0 and ik.ik_get_jpeg_prog_free() == HOST
        assert ik.ik_set_jpeg_prog_free(-1) == 0
        monkeypatch.setenv("IK_JPEG_PROG_FREE", "gpu")
        assert ik.ik_get_jpeg_prog_free() == GPU
        monkeypatch.setenv("IK_JPEG_PROG_FREE", "host")
        assert ik.ik_get_jpeg_prog_free() == HOST
        assert ik.ik_set_jpeg_prog_free(2) == ik.ik_set_jpeg_device(2) != 0  # the other setters' status
    finally:
        ik.ik_set_jpeg_prog_free(-1)


SINGLE = {
    "noise_444": pu.noise_444,
    "s_420": pu.s_420,
    "s_422": pu.s_422,
    "noise_420_big": pu.noise_420_big,
    "gray": pu.gray,
    "flat_gray_noise_rows": pu.flat_gray_noise_rows,
    "optimised_420": pu.optimised_420,
}
for _s in pu.WRITER_SAMPLINGS:
    for _k in pu.WRITER_SCRIPTS:
        SINGLE[f"{_s}_{_k}"] = (lambda s, k: lambda: pu.writer(s, k).data)(_s, _k)


@pytest.mark.parametrize("name", list(SINGLE))
def test_eligible_file_is_gpu_decoded_and_exact(ik, oracle, name):
    data = SINGLE[name]()
    assert b"\xff\xc2" in data and b"\xff\xdd" not in data
    assert sum(e - s for s, e in pu.scan_spans(data)) >= 4096
    with _switch(ik, GPU):
        _check(ik, oracle, data, "gpu")


def test_below_the_threshold_stays_on_the_host(ik, oracle):
    data = pu.tiny()
    assert sum(e - s for s, e in pu.scan_spans(data)) < 4096
    with _switch(ik, GPU):
        _check(ik, oracle, data, "host")


def test_flat_image_is_below_the_threshold(ik, oracle):
    """A flat 512 x 512 gray image codes to 1.5 KiB over its six scans: exact, and
    by the 4 KiB rule the host's (SINGLE's flat_gray_noise_rows is the eligible
    file whose AC-first scans are long end-of-block runs)."""
    data = pu.flat_gray()
    assert sum(e - s for s, e in pu.scan_spans(data)) < 4096
    with _switch(ik, GPU):
        _check(ik, oracle, data, "host")


def test_overlapping_first_scans_stay_on_the_host(ik, oracle):
    """The GPU path runs an image's Ah = 0 scans together; a file that codes a band
    twice depends on their order, so the host decoder, which keeps it, takes it."""
    data = pu.overlapping_first_scans().data
    assert sum(e - s for s, e in pu.scan_spans(data)) >= 4096
    with _switch(ik, GPU):
        _check(ik, oracle, data, "host")


def test_switch_at_host_keeps_the_host(ik, oracle):
    with _switch(ik, HOST):
        _check(ik, oracle, pu.s_420(), "host")


def test_mixed_batch(ik, oracle):
    """Baseline, progressive with restart rows (k_jpeg_prog), three restart-free
    progressive files of different sampling, a PNG and a file below the threshold,
    in one call: each equals its own single-request answer."""
    b = io.BytesIO()
    Image.fromarray(ikutil.synth(320, 240, 3, seed=3, pattern="N")).save(b, format="JPEG", quality=90)
    baseline = b.getvalue()
    assert b"\xff\xc0" in baseline and len(baseline) >= 8192
    p = io.BytesIO()
    Image.fromarray(ikutil.synth(64, 48, 3, seed=4)).save(p, format="PNG")
    blobs = [baseline, pu.with_restart_rows(), pu.noise_444(), pu.s_420(), pu.writer("411", "dc_approx").data,
             p.getvalue(), pu.tiny()]
    with _switch(ik, GPU):
        singles = [decode_image(x)[0].to_array() for x in blobs]
        c0 = _counts(ik)
        out = decode_image_batch(blobs)
        c1 = _counts(ik)
    assert (c1[0] - c0[0], c1[1] - c0[1]) == (5, 1)  # the PNG is no JPEG stream; the 17 x 9 file is the host's
    for (img, _), want, x in zip(out, singles, blobs):
        np.testing.assert_array_equal(img.to_array(), want)
        if x[:2] == b"\xff\xd8":
            np.testing.assert_array_equal(img.to_array(), oracle.jpeg_decode(x, ZUNE))


def _outcome(data):
    try:
        return "pixels", decode_image(data)[0].to_array()
    except TransformError as e:
        return "error", str(e)


def _damaged():
    good = pu.s_420()
    spans = pu.scan_spans(good)
    out = {}
    for tag, (s, _) in (("middle_scan", spans[len(spans) // 2]), ("last_scan", spans[-1])):
        b = bytearray(good)
        for j in range(s + 40, s + 48):  # the recipe of test_jpeg_progressive_restarts_corrupt_interval_...
            if b[j] != 0xFF and b[j - 1] != 0xFF:
                b[j] ^= 0x5A
        out[tag] = bytes(b)
    out["cut_in_half"] = good[:len(good) // 2]
    return out


@pytest.mark.parametrize("tag", ["middle_scan", "last_scan", "cut_in_half"])
def test_damaged_file_ends_as_on_the_host(ik, oracle, tag):
    data = _damaged()[tag]
    with _switch(ik, HOST):
        kind_h, val_h = _outcome(data)
    with _switch(ik, GPU):
        kind_g, val_g = _outcome(data)
        assert kind_g == kind_h
        if kind_h == "pixels":
            np.testing.assert_array_equal(val_g, val_h)
        else:
            assert val_g == val_h
        # and the library is usable: a good file right after
        _check(ik, oracle, pu.noise_444(), "gpu")
