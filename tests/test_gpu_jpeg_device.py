"""GPU: baseline JPEG bodies of a device-resident batch decoded where they lie
(ik_transform_batch_submit_device: k_jpeg_walk brings back each file's skeleton and
two offsets, the host parser reads the skeleton, the self-synchronising decoder reads
the scan from the caller's memory).

Every check submits the same files twice -- as DeviceBytes through
transform_batch_submit_device and as host bytes through transform_batch_submit -- with
the same requests (each file to (64, None) JPEG q85 and to (None, None) WebP q80) and
asserts byte-identical outputs and equal per-request status, under both
reconstruction modes.  ik_jpeg_device_counters says which way each file went:
[0] taken in place, [1] copied back before parsing, [2] taken in place and copied
back later for the host decoder.

Two things to know about the files: jpeg_writer.CASES has no `420_tiny` (`440_tiny` and
the 4:2:0 `fill_small` are the tiny files here), and `440_y_then_chroma_big` /
`420_scan_per_comp_dri5` name fewer components in their first SOS than the frame has,
which the walk sees in the SOS header and answers with a copy-back before parsing ([1]);
the late fallback ([2]) is shown by the FF C4 file and by a file whose full scan is sent
twice (every component in the first SOS, a second SOS behind it)."""
import ctypes
import io

import numpy as np
import pytest
from PIL import Image

import ikutil
import jpeg_device_util as ju
import jpeg_writer as jw
from imagekit import DeviceBytes, ImageFormat, _lib, transform_batch_submit, transform_batch_submit_device

pytestmark = pytest.mark.gpu

ZUNE, LIBJPEG = 1, 0
HOSTILE = (b"\xff\xda\x00\x0c\x03\x01\x00\x02\x11\x03\x11\x00\x3f\x00", b"\xff\xd9", b"\xff\x00\xff\x00")


@pytest.fixture(params=[ZUNE, LIBJPEG], ids=["zune", "libjpeg"])
def recon(ik, request):
    prev = ik.ik_get_jpeg_reconstruction()
    assert ik.ik_set_jpeg_reconstruction(request.param) == 0
    yield request.param
    ik.ik_set_jpeg_reconstruction(prev)


def dev_counters(lib):
    c = (ctypes.c_ulonglong * 3)()
    assert lib.ik_jpeg_device_counters(c) == 0
    return np.array(list(c), dtype=np.int64)


def jpeg_counters(lib):
    c = (ctypes.c_ulonglong * 2)()
    assert lib.ik_jpeg_counters(c) == 0
    return np.array(list(c), dtype=np.int64)


def requests(n):
    """each of n files twice: (64, None) JPEG q85 and (None, None) WebP q80"""
    idx = [i for i in range(n) for _ in range(2)]
    sizes = [(64, None), (None, None)] * n
    fmts = [ImageFormat.jpeg, ImageFormat.webp] * n
    qs = [85, 80] * n
    return idx, sizes, fmts, qs


def finish(lib, p):
    """wait for a PendingBatch: (bytes or None per request, status per request, message)"""
    rc = lib.ik_transform_batch_wait(p._ticket)
    p._done = True
    msg = _lib.last_error() if rc else ""
    outs = []
    for i in range(p._n):
        o = p._outs[i]
        outs.append(ctypes.string_at(o, p._olens[i]) if o else None)
        if o:
            lib.ik_buf_free(o)
    return outs, list(p._status), msg


def submit_host(datas):
    idx, sizes, fmts, qs = requests(len(datas))
    return transform_batch_submit([datas[i] for i in idx], sizes, fmts, qs)


def submit_dev(devs):
    idx, sizes, fmts, qs = requests(len(devs))
    return transform_batch_submit_device([devs[i] for i in idx], sizes, fmts, qs)


def both(lib, datas, devs=None):
    """(device run, host run, device-counter delta, jpeg-counter delta of the device run)"""
    want = finish(lib, submit_host(datas))
    devs = devs if devs is not None else [DeviceBytes(d) for d in datas]
    d0, j0 = dev_counters(lib), jpeg_counters(lib)
    got = finish(lib, submit_dev(devs))
    return got, want, dev_counters(lib) - d0, jpeg_counters(lib) - j0


def assert_same(got, want):
    assert got[1] == want[1]  # per-request status
    assert got[0] == want[0]  # bytes (None where a request failed)
    assert got[2] == want[2]  # the first failure's message


def in_place_files():
    return ([jw.build(n).data for n in ("420_optimal", "440_long_dri5", "410_big", "fill_big", "stray_big",
                                        "trailer_big", "gray22_big_dri5")]
            + [ju.pillow(k) for k in ("420_opt", "444", "gray", "420_dri")]
            + [ju.special("big_appn").data, ju.big_appn_first(), ju.special("eoi_in_appn").data])


def test_in_place(ik, recon):
    datas = in_place_files()
    n = 2 * len(datas)
    got, want, dd, dj = both(ik, datas)
    assert all(s == 0 for s in want[1]) and all(o for o in want[0])
    assert_same(got, want)
    assert list(dd) == [n, 0, 0]
    assert list(dj) == [n, 0]


def test_copy_back(ik, recon):
    # (no `420_tiny` among the cases: 440_tiny and the small 4:2:0 fill_small)
    datas = [jw.build("440_tiny").data, jw.build("fill_small").data, ju.pillow("progressive"),
             jw.build("440_prog_spectral_dri3").data, ju.special("sos_subset").data]
    got, want, dd, _ = both(ik, datas)
    assert_same(got, want)
    assert list(dd) == [0, 2 * len(datas), 0]


def test_late_fallback(ik, recon):
    multi = [jw.build("440_y_then_chroma_big").data, jw.build("420_scan_per_comp_dri5").data]
    late = [ju.stray_marker(), ju.scan_twice()]
    good = [jw.build("420_optimal").data]
    got, want, dd, dj = both(ik, multi + late + good)
    assert_same(got, want)
    # the multi-scan files' first SOS names one component of three: copied back at submit;
    # the FF C4 file and the twice-scanned one pass the walk and come back alone, later
    assert list(dd) == [2 * (len(late) + len(good)), 2 * len(multi), 2 * len(late)]
    assert dj[0] == 2 * len(good)


class View(DeviceBytes):
    """len bytes at an offset of a DeviceBytes allocation (which it keeps alive)"""
    __slots__ = ("base",)

    def __init__(self, base, off, n):
        self.base, self.ptr, self.len = base, base.ptr + off, n

    def __del__(self):
        pass


def lone_ff_end():
    """cut right after an FF of the scan: the byte that follows decides nothing"""
    f = jw.build("420_optimal")
    ent = f.data.index(f.scan_bytes[0])
    k = f.data.index(b"\xff\x00", ent + len(f.scan_bytes[0]) // 2)
    return f.data[:k + 1]


def test_no_slack(ik, recon):
    """all the files back to back in one allocation at odd offsets, each followed at once by
    bytes of another kind of meaning: nothing at or past a file's end is read"""
    datas = in_place_files() + [ju.stray_marker(), ju.scan_twice(), ju.no_eoi(), ju.cut_mid_scan(), lone_ff_end(),
                                jw.build("440_tiny").data]
    blob, offs = bytearray(b"\xff\xd9\xff\xda"), []
    for k, d in enumerate(datas):
        blob += b"\xff" * (1 + k % 3)  # 1, 2, 3 past the previous end
        offs.append(len(blob))
        blob += d + HOSTILE[k % 3]
    blob += bytes(8192)  # no file near the allocation's end
    base = DeviceBytes(bytes(blob))
    assert len({o % 4 for o in offs}) == 4  # every alignment of a 32-bit word
    devs = [View(base, o, len(d)) for o, d in zip(offs, datas)]
    got, want, dd, _ = both(ik, datas, devs)
    assert_same(got, want)
    assert dd[0] >= 2 * len(in_place_files())


def test_malformed(ik, recon):
    bad = [ju.cut_mid_scan(), ju.length_overrun()]
    good = [jw.build("420_optimal").data, ju.pillow("420_dri")]
    for datas in ([bad[0]], [bad[1]], bad, [good[0], bad[0], good[1], bad[1]]):
        got, want, _, _ = both(ik, datas)
        assert_same(got, want)
        for k, d in enumerate(datas):
            # (whether a scan cut short is an error is the host decoder's to say: assert_same above)
            if any(d is g for g in good):
                assert got[1][2 * k:2 * k + 2] == [0, 0] and all(got[0][2 * k:2 * k + 2])
            elif d is bad[1]:
                assert all(got[1][2 * k:2 * k + 2]) and not any(got[0][2 * k:2 * k + 2])
    only_good, want_good, _, _ = both(ik, good)
    assert got[0][0:2] == only_good[0][0:2] and got[0][4:6] == only_good[0][2:4]


def test_mixed_batch(ik, recon):
    buf = io.BytesIO()
    Image.fromarray(ikutil.synth(320, 280, 4, seed=3, pattern="N"), "RGBA").save(buf, "PNG")  # 358 KB raw: the GPU path
    png = buf.getvalue()
    buf = io.BytesIO()
    Image.fromarray(ikutil.synth(203, 141, 3, seed=4, pattern="S")).save(buf, "WEBP", quality=80)
    webp = buf.getvalue()
    datas = [png, webp, jw.build("420_optimal").data, ju.pillow("444"), webp, png, jw.build("440_tiny").data]
    got, want, dd, _ = both(ik, datas)
    assert all(s == 0 for s in want[1])
    assert_same(got, want)
    assert list(dd) == [4, 2, 0]


def test_two_batches_in_flight(ik, recon):
    a = in_place_files()[:6]
    b = in_place_files()[6:] + [ju.stray_marker(), jw.build("440_tiny").data]
    want_a, want_b = finish(ik, submit_host(a)), finish(ik, submit_host(b))
    da, db = [DeviceBytes(d) for d in a], [DeviceBytes(d) for d in b]
    pa = submit_dev(da)
    pb = submit_dev(db)
    got_a = finish(ik, pa)
    got_b = finish(ik, pb)
    assert_same(got_a, want_a)
    assert_same(got_b, want_b)


def test_switch(ik, recon, monkeypatch):
    datas = in_place_files()[:4] + [jw.build("440_tiny").data]
    n = 2 * len(datas)
    try:
        assert ik.ik_set_jpeg_device(0) == 0 and ik.ik_get_jpeg_device() == 0
        got, want, dd, _ = both(ik, datas)
        assert_same(got, want)
        assert list(dd) == [0, n, 0]
        assert ik.ik_set_jpeg_device(-1) == 0
        monkeypatch.setenv("IK_JPEG_DEVICE", "copy")  # read per batch
        assert ik.ik_get_jpeg_device() == 0
        got2, _, dd, _ = both(ik, datas)
        assert list(dd) == [0, n, 0] and got2 == got
        monkeypatch.setenv("IK_JPEG_DEVICE", "inplace")
        assert ik.ik_get_jpeg_device() == 1
        got3, _, dd, _ = both(ik, datas)
        assert list(dd) == [n - 2, 2, 0] and got3 == got
        assert ik.ik_set_jpeg_device(2) != 0
    finally:
        ik.ik_set_jpeg_device(-1)
