"""CPU: the host half of the GPU path for lossy WebP files with an alpha plane
(ik_webp_alpha_plane, ik_vp8d_host.cpp): the container rules, the ALPH header, and the
filtered plane -- raw bytes, or a lossless stream read through libwebp as the green
channel of the VP8L file it would be.

Bar: the plane it returns, un-filtered here in numpy with libwebp's prediction rules
(tests/webp_alpha_util.py), equals the alpha channel of libwebp's WebPDecodeRGBA of the
whole file, for Pillow-made files (raw and lossless planes, pre-processing 0 and 1, the
encoder's filters) and for hand-built files with each of the four filters at sizes
that are one row, one column, and 63 / 64 / 65 wide or tall.  Files the GPU path leaves
to libwebp return IK_ERR_UNSUPPORTED."""
import ctypes

import numpy as np
import pytest

import webp_alpha_util as au
from imagekit import _lib

IK_OK, IK_ERR_UNSUPPORTED = 0, 4


def alpha_plane(data: bytes):
    """(status, filtered plane, filter, compression) of ik_webp_alpha_plane."""
    lib = _lib.load()
    cap = 1 << 16
    buf = np.zeros(cap, np.uint8)
    w, h = ctypes.c_uint32(), ctypes.c_uint32()
    filt, comp = ctypes.c_int(-1), ctypes.c_int(-1)
    st = lib.ik_webp_alpha_plane(data, len(data), buf.ctypes.data, cap, ctypes.byref(w), ctypes.byref(h),
                                 ctypes.byref(filt), ctypes.byref(comp))
    if st:
        return st, None, None, None
    return st, buf[:w.value * h.value].reshape(h.value, w.value).copy(), filt.value, comp.value


def check(name: str, data: bytes):
    st, plane, filt, comp = alpha_plane(data)
    assert st == IK_OK, f"{name}: {_lib.last_error()}"
    want = au.decode_rgba(data)[..., 3]
    assert plane.shape == want.shape, name
    hdr = au.alph_header(data)
    assert (filt, comp) == (hdr["filter"], hdr["compression"]), name
    np.testing.assert_array_equal(au.unfilter(plane, filt), want, err_msg=name)
    return hdr


@pytest.fixture(scope="module")
def pillow_files():
    return au.pillow_files()


def test_pillow_files(pillow_files):
    seen = [check(name, data) for name, data in pillow_files]
    # what the files cover between them: both compressions, both pre-processing values, a filter
    assert {h["compression"] for h in seen} == {0, 1}
    assert {h["pre"] for h in seen} == {0, 1}
    assert any(h["filter"] for h in seen)


@pytest.mark.parametrize("filt", [0, 1, 2, 3])
@pytest.mark.parametrize("wh", au.SIZES, ids=[f"{w}x{h}" for w, h in au.SIZES])
def test_hand_built_raw_planes(wh, filt):
    w, h = wh
    for kind in ("noise", "smooth"):
        data = au.hand_built(w, h, filt, kind)
        hdr = check(f"{w}x{h} filter {filt} {kind}", data)
        assert hdr == dict(compression=0, filter=filt, pre=0, reserved=0)


def test_the_forward_filters_here_are_libwebps():
    # the hand-built planes are only a check if this file's forward filter is the inverse of
    # libwebp's un-filter: WebPDecodeRGBA gives the plane that went in
    for filt in (1, 2, 3):
        data = au.hand_built(130, 67, filt, "noise")
        np.testing.assert_array_equal(au.decode_rgba(data)[..., 3], au.alpha_of("noise", 130, 67, 130 + 3 * 67 + filt))


def test_files_left_to_libwebp():
    names = []
    for name, data in au.broken_files():
        st, _, _, _ = alpha_plane(data)
        assert st == IK_ERR_UNSUPPORTED, name
        names.append(name)
    assert names == ["opaque", "lossless", "flag without chunk", "short raw plane", "reserved bits 2",
                     "truncated lossless payload"]


def test_container_rules():
    w, h = 9, 9
    good = au.hand_built(w, h, 3)
    parts = au.chunks(good)
    assert alpha_plane(good)[0] == IK_OK
    alph = [c for c in parts if c[0] == b"ALPH"][0]
    vp8 = [c for c in parts if c[0] == b"VP8 "][0]
    cases = {
        "two ALPH chunks": [au.vp8x(w, h, 0x10), alph, alph, vp8],
        "chunk without the flag": [au.vp8x(w, h, 0), alph, vp8],
        "animation flag": [au.vp8x(w, h, 0x12), alph, vp8],
        "canvas is not the frame": [au.vp8x(w + 1, h, 0x10), alph, vp8],
        "compression 2": [au.vp8x(w, h, 0x10), (b"ALPH", bytes([2]) + alph[1][1:]), vp8],
        "pre-processing 2": [au.vp8x(w, h, 0x10), (b"ALPH", bytes([2 << 4]) + alph[1][1:]), vp8],
        "ALPH after the frame": [au.vp8x(w, h, 0x10), vp8, alph],
    }
    for name, p in cases.items():
        assert alpha_plane(au.riff(p))[0] == IK_ERR_UNSUPPORTED, name


def test_switch_default_and_setter(monkeypatch):
    lib = _lib.load()
    monkeypatch.delenv("IK_WEBP_ALPHA_DECODE", raising=False)
    assert lib.ik_get_webp_alpha_decode() == 0  # off by default
    monkeypatch.setenv("IK_WEBP_ALPHA_DECODE", "gpu")
    assert lib.ik_get_webp_alpha_decode() == 1  # read per call
    monkeypatch.setenv("IK_WEBP_ALPHA_DECODE", "host")
    assert lib.ik_get_webp_alpha_decode() == 0
    try:
        assert lib.ik_set_webp_alpha_decode(1) == 0 and lib.ik_get_webp_alpha_decode() == 1
        assert lib.ik_set_webp_alpha_decode(7) != 0 and lib.ik_get_webp_alpha_decode() == 1
    finally:
        assert lib.ik_set_webp_alpha_decode(-1) == 0
    assert lib.ik_get_webp_alpha_decode() == 0
