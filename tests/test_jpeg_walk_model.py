"""CPU: the JPEG marker walk behind in-place decoding of device-resident bodies
(csrc/ik_jpeg_walk.h), through its host entry ik_jpeg_walk_host -- the same code
k_jpeg_walk runs with one wave per file.

For every case of jpeg_writer.CASES, Pillow files and a few files built for the walk:
the skeleton, offsets, verdict and reason equal a second statement of the rules
(jpeg_device_util.ref_walk); the skeleton followed by the file's bytes from the
entropy offset decodes (oracle/jpeg_dec.c) to the pixels of the whole file, i.e. it
carries the same frame, tables and restart interval; the entropy offset is where the
writer put the first scan's bytes."""
import numpy as np
import pytest

import jpeg_device_util as ju
import jpeg_writer as jw
from imagekit import _lib


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def check_against_rules(lib, data):
    skel, info = ju.walk(lib, data)
    verdict, reason, rskel, ent, eoi, sof = ju.ref_walk(data)
    assert (info.verdict, info.reason) == (verdict, reason)
    assert skel == rskel
    assert (info.entropy_offset, info.eoi_offset, info.sof_marker) == (ent, eoi, sof)
    return skel, info


def same_pixels(oracle, skel, info, data):
    """the skeleton + the file from the entropy offset on == the file, decoded on the CPU"""
    np.testing.assert_array_equal(oracle.jpeg_decode(skel + data[info.entropy_offset:]), oracle.jpeg_decode(data))


IN_PLACE_CASES = [c.name for c in jw.CASES if c.where == "gpu" and "prog" not in c.name]


@pytest.mark.parametrize("name", [c.name for c in jw.CASES])
def test_writer_cases(lib, oracle, name):
    f = jw.build(name)
    case = jw.BY_NAME[name]
    skel, info = check_against_rules(lib, f.data)
    # the first scan's bytes start at the entropy offset
    sb = f.scan_bytes[0]
    assert f.data[info.entropy_offset:info.entropy_offset + len(sb)] == sb
    single = len(case.kw.get("scans") or (0,)) == 1
    if single:
        # (also under trailer_*, bytes after EOI; fill bytes before EOI count to the scan, as on the host)
        assert info.eoi_offset == info.entropy_offset + len(sb) + case.kw.get("fill", 0)
    same_pixels(oracle, skel, info, f.data)
    progressive = case.kw.get("sof") == jw.SOF2
    if progressive:
        assert (info.verdict, info.reason) == (ju.COPY_BACK, ju.R_NOT_BASELINE)
    elif not single:
        assert (info.verdict, info.reason) == (ju.COPY_BACK, ju.R_COMPONENTS)
    elif len(sb) < 4096:
        assert (info.verdict, info.reason) == (ju.COPY_BACK, ju.R_SMALL)
    else:
        assert (info.verdict, info.reason) == (ju.IN_PLACE, ju.R_NONE)


def test_every_gpu_baseline_case_is_in_place(lib):
    """every single-scan baseline case of 4 KiB or more: sof1, pq1, fill, stray, merged,
    adobe*, the _dri5 variants, gray"""
    names = set(IN_PLACE_CASES)
    for must in ("sof1_big", "pq1_big", "fill_big", "stray_big", "merged_big", "adobe0_big", "adobe0_420_big",
                 "adobe1_big", "trailer_big", "440_big_dri5", "gray22_big", "gray22_big_dri5", "420_optimal",
                 "440_long_dri5", "410_big"):
        assert must in names
    for name in IN_PLACE_CASES:
        _, info = ju.walk(lib, jw.build(name).data)
        assert (info.verdict, info.reason) == (ju.IN_PLACE, ju.R_NONE), name


@pytest.mark.parametrize("kind", ["420_opt", "444", "gray", "420_dri"])
def test_pillow_baseline(lib, oracle, kind):
    data = ju.pillow(kind)
    skel, info = check_against_rules(lib, data)
    assert (info.verdict, info.reason, info.sof_marker) == (ju.IN_PLACE, ju.R_NONE, 0xC0)
    assert info.eoi_offset == len(data) - 2
    same_pixels(oracle, skel, info, data)


def test_pillow_progressive(lib, oracle):
    data = ju.pillow("progressive")
    skel, info = check_against_rules(lib, data)
    assert (info.verdict, info.reason, info.sof_marker) == (ju.COPY_BACK, ju.R_NOT_BASELINE, 0xC2)
    same_pixels(oracle, skel, info, data)


def test_sos_with_fewer_components(lib):
    _, info = check_against_rules(lib, ju.special("sos_subset").data)
    assert (info.verdict, info.reason) == (ju.COPY_BACK, ju.R_COMPONENTS)


def test_last_eoi(lib, oracle):
    # garbage after EOI
    f = jw.build("trailer_big")
    _, info = check_against_rules(lib, f.data)
    assert info.eoi_offset == len(f.data) - len(jw.GARBAGE) - 2 and f.data[info.eoi_offset:][:2] == b"\xff\xd9"
    # FF D9 inside an APPn payload before SOS is not the scan's end
    f = ju.special("eoi_in_appn")
    assert f.data.index(b"\xff\xd9") < f.data.index(f.scan_bytes[0])
    skel, info = check_against_rules(lib, f.data)
    assert info.verdict == ju.IN_PLACE and info.eoi_offset == len(f.data) - 2
    assert b"\xff\xd9" not in skel
    same_pixels(oracle, skel, info, f.data)
    # ... nor is one that lies before the scan in a file too short for the search window to clear it
    tiny = jw.encode(jw.ycbcr(ju._noise(17, 17)), jw.S420, extra=((0xE3, b"x\xff\xd9y"),), trailer=b"")
    cut = tiny.data[:-2]  # and no EOI after the scan
    _, info = check_against_rules(lib, cut)
    assert info.eoi_offset == len(cut)
    # no EOI at all: the file's end
    data = ju.no_eoi()
    _, info = check_against_rules(lib, data)
    assert info.verdict == ju.IN_PLACE and info.eoi_offset == len(data)
    # an EOI further than 4 KiB from the end is not looked for (as the host parser's search)
    data = jw.build("420_optimal").data + bytes(5000)
    _, info = check_against_rules(lib, data)
    assert info.eoi_offset == len(data)


def test_malformed(lib):
    for data, reason in ((ju.length_overrun(), ju.R_LENGTH), (ju.cut_in_header(), ju.R_LENGTH),
                         (ju.no_soi(), ju.R_NO_SOI), (b"", ju.R_NO_SOI), (b"\xff", ju.R_NO_SOI)):
        _, info = check_against_rules(lib, data)
        assert (info.verdict, info.reason) == (ju.MALFORMED, reason)
    # cut right after a marker, inside the length field
    f = jw.build("420_optimal").data
    k = f.index(b"\xff\xc4")
    for cut in (k + 2, k + 3):
        _, info = check_against_rules(lib, f[:cut])
        assert (info.verdict, info.reason) == (ju.MALFORMED, ju.R_LENGTH)
    # a cut in mid-scan is no matter of the walk's: the decoder finds it
    _, info = check_against_rules(lib, ju.cut_mid_scan())
    assert info.verdict == ju.IN_PLACE
    # only SOI, or EOI before any scan: no SOS
    for data in (b"\xff\xd8", b"\xff\xd8\xff\xd9", f[:k]):
        _, info = check_against_rules(lib, data)
        assert (info.verdict, info.reason) == (ju.COPY_BACK, ju.R_NO_SOS)


@pytest.mark.parametrize("first", [False, True])
def test_big_appn_payloads_are_stepped_over(lib, oracle, first):
    data = ju.big_appn_first() if first else ju.special("big_appn").data
    assert len(data) > 2 * len(ju.PAYLOAD)
    if first:
        assert data.index(b"Exif") < data.index(b"\xff\xdb")
    skel, info = check_against_rules(lib, data)
    assert (info.verdict, info.reason) == (ju.IN_PLACE, ju.R_NONE)
    assert len(skel) < 1024 and ju.PAYLOAD[:16] not in skel and b"Exif" not in skel and b"ICC_PROFILE" not in skel
    same_pixels(oracle, skel, info, data)


def test_skeleton_too_large(lib):
    """tables sent until the slot overflows: a copy-back, not an error"""
    f = jw.build("420_optimal").data
    k = f.index(b"\xff\xdb")
    ln = int.from_bytes(f[k + 2:k + 4], "big") + 2
    data = f[:k] + f[k:k + ln] * 70 + f[k:]
    skel, info = check_against_rules(lib, data)
    assert (info.verdict, info.reason) == (ju.COPY_BACK, ju.R_LARGE) and len(skel) <= ju.SLOT
    # an APP0 with a thumbnail-sized payload likewise
    data = f[:2] + b"\xff\xe0" + (5002).to_bytes(2, "big") + bytes(5000) + f[2:]
    _, info = check_against_rules(lib, data)
    assert (info.verdict, info.reason) == (ju.COPY_BACK, ju.R_LARGE)


def test_fill_bytes_and_garbage(lib):
    f = jw.build("fill_big")
    assert b"\xff\xff\xff\xff\xdb" in f.data
    skel, info = check_against_rules(lib, f.data)
    assert info.verdict == ju.IN_PLACE and b"\xff\xff" not in skel[:4]
    g = jw.build("420_optimal").data
    k = g.index(b"\xff\xc4")
    _, info = check_against_rules(lib, g[:k] + b"\x00\x01" + g[k:])
    assert (info.verdict, info.reason) == (ju.COPY_BACK, ju.R_GARBAGE)


def test_bad_arguments(lib):
    import ctypes
    info = ju.WalkInfo()
    skel = (ctypes.c_uint8 * 16)()
    assert lib.ik_jpeg_walk_host(b"\xff\xd8", 2, skel, 16, ctypes.byref(info)) != 0
    assert "4096" in _lib.last_error()
