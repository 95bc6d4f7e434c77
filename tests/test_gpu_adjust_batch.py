"""GPU: colour adjustments through one batch.  Ten small requests chosen so that the adjust
step of the post stage sees a group of several, a lone member, a member it must leave alone,
one that also carries a blur and a watermark, one that is not resized and one that fails in
the decoder.  Every output is compared with the same request through transform() alone, byte
for byte, and the adjust, blur and overlay launch counters with the launches that follow from
who shares what."""
import ctypes
import io

import numpy as np
import pytest
from PIL import Image

import ikutil
from imagekit import (Adjust, DeviceBytes, DynamicImage, ImageFormat, Overlay, TransformError, _lib, transform_batch,
                      transform_batch_submit, transform_batch_submit_device)
from imagekit.transform import _inputs, _request_opts, transform

pytestmark = pytest.mark.gpu
J, WP = ImageFormat.jpeg, ImageFormat.webp
FAILED = 9  # the truncated file's place in the batch


def png_of(img):
    b = io.BytesIO()
    Image.fromarray(img, {3: "RGB", 4: "RGBA"}[img.shape[2]]).save(b, format="PNG")
    return b.getvalue()


@pytest.fixture(scope="module")
def requests_(ik):
    """(data, (w, h), adjust, blur, overlay, fmt, quality) per request"""
    r1 = png_of(ikutil.synth(96, 64, 3, seed=61, pattern="S"))
    r2 = png_of(ikutil.synth(96, 64, 3, seed=62, pattern="S"))
    rgba = png_of(ikutil.synth(96, 64, 4, seed=63, pattern="S", alpha="random"))
    other = png_of(ikutil.synth(72, 48, 3, seed=64, pattern="S"))
    mark = DynamicImage.from_array(np.random.default_rng(65).integers(0, 256, (10, 24, 4)).astype(np.uint8))
    gray = Adjust(grayscale=True)
    warm = Adjust(saturation=40, hue=15, brightness=5, contrast=10, gamma=1.8)
    return [
        (r1, (48, 32), gray, None, None, J, 85),                    # 0, 1: a pair that shares geometry and adjustment
        (r2, (48, 32), Adjust(saturation=-100), None, None, J, 85),  #       (an equal Adjust: the same 24 bytes)
        (r1, (48, 32), warm, None, None, J, 85),                    # 2: the same resize group, another adjustment
        (r2, (48, 32), None, None, None, J, 85),                    # 3: the same group, none
        (r1, (48, 32), gray, 1.0, Overlay(mark, "se", -2, -2, 200), WP, 80),  # 4: with the pair; then a blur and a mark
        (r2, (None, None), warm, None, None, WP, 80),               # 5: not resized: adjusted on the decoded image
        (rgba, (48, 32), Adjust(invert=True), None, None, WP, 80),  # 6: RGBA: a group of its own geometry, alone
        (other, (36, 24), gray, None, None, J, 85),                 # 7: alone at every stage
        (r1, (48, 32), Adjust(), None, None, WP, 80),               # 8: an Adjust that changes nothing
        (r1[:len(r1) // 2], (48, 32), gray, None, None, J, 85),     # 9: truncated: its own decode status
    ]


# Who shares a launch (csrc/ik_post_stage.cpp; a set of one takes the per-image call, which
# launches and counts as a set of one would):
#   resize   96x64 RGB -> 48x32 {0, 1, 2, 3, 4, 8}; 5 is not resized; 6 and 7 are the only ones of
#            their geometry: none of the three is in a group
#   adjust   inside the group grayscale {0, 1, 4} and warm {2}; image by image 5, 6 and 7:
#            5 launches, 7 images
#   filter   blur 1.0 {4}: 1 launch, 1 image
#   mark     {4}: 1 launch, 1 image
# The truncated file fails in the decoder and reaches none of them.
ADJUST, BLUR, OVERLAY = (5, 7), (1, 1), (1, 1)


def counters(ik):
    out = []
    for fn in (ik.ik_adjust_counters, ik.ik_blur_counters, ik.ik_overlay_counters):
        c = (ctypes.c_ulonglong * 2)()
        assert fn(c) == 0
        out.append((int(c[0]), int(c[1])))
    return np.array(out, dtype=np.int64)


@pytest.fixture(scope="module")
def alone(ik, requests_):
    """each request through transform() by itself, computed once (None: the truncated file)"""
    out = []
    for i, (data, (w, h), a, blur, ov, fmt, q) in enumerate(requests_):
        if i == FAILED:
            with pytest.raises(TransformError):
                transform(data, w, h, fmt, q, adjust=a, blur=blur, overlay=ov)
            out.append(None)
        else:
            out.append(transform(data, w, h, fmt, q, adjust=a, blur=blur, overlay=ov))
    return out


def batch_args(reqs):
    args = ([r[1] for r in reqs], [r[5] for r in reqs], [r[6] for r in reqs])
    kw = dict(adjusts=[r[2] for r in reqs], blurs=[r[3] for r in reqs], overlays=[r[4] for r in reqs])
    return args, kw


def wait_all(ik, pb):
    """PendingBatch.wait() raises for the first failed request and drops the others' bytes; the
    same wait, keeping every output and status"""
    rc = ik.ik_transform_batch_wait(pb._ticket)
    pb._done = True
    outs = []
    for i in range(pb._n):
        outs.append(ctypes.string_at(pb._outs[i], pb._olens[i]) if pb._outs[i] else None)
        if pb._outs[i]:
            ik.ik_buf_free(pb._outs[i])
    return rc, outs, list(pb._status)


def check(ik, alone, run, expect=(ADJUST, BLUR, OVERLAY)):
    c0 = counters(ik)
    rc, outs, status = run()
    delta = counters(ik) - c0
    print("adjust, blur, overlay (launches, images):", delta.tolist())
    assert rc != 0 and "item %d" % FAILED in _lib.last_error()
    assert np.array_equal(delta, expect), delta.tolist()
    assert [s != 0 for s in status] == [i == FAILED for i in range(len(status))], status
    assert outs[FAILED] is None
    for i, want in enumerate(alone):
        assert outs[i] == want, i


def raw_batch(ik, reqs, kw):
    """ik_transform_batch_opts with the options array the Python call builds, every output and
    status kept"""
    (sizes, fmts, qs), _ = batch_args(reqs)
    datas = [r[0] for r in reqs]
    n = len(reqs)
    keep, ptrs, lens = _inputs(datas)
    ws = (ctypes.c_int64 * n)(*[-1 if s[0] is None else s[0] for s in sizes])
    hs = (ctypes.c_int64 * n)(*[-1 if s[1] is None else s[1] for s in sizes])
    fs = (ctypes.c_int * n)(*[int(f.value) for f in fmts])
    qa = (ctypes.c_int * n)(*qs)
    ra = _request_opts(n, blurs=kw["blurs"], overlays=kw["overlays"], adjusts=kw["adjusts"])
    size = ctypes.sizeof(ra._type_)
    outs, olens, status = (ctypes.c_void_p * n)(), (ctypes.c_size_t * n)(), (ctypes.c_int * n)()
    rc = ik.ik_transform_batch_opts(ptrs, lens, n, ws, hs, ra, size, fs, qa, 4, 0, outs, olens, status)
    res = []
    for i in range(n):
        res.append(ctypes.string_at(outs[i], olens[i]) if outs[i] else None)
        if outs[i]:
            ik.ik_buf_free(outs[i])
    return size, rc, res, list(status)


def test_requests_differ_where_their_adjustments_do(alone):
    assert all(alone[i] for i in range(len(alone)) if i != FAILED)
    assert alone[0] != alone[2] and alone[1] != alone[3] and alone[0] != alone[4]
    assert len({alone[0], alone[2], alone[4], alone[8]}) == 4


def test_transform_batch(ik, requests_, alone):
    (sizes, fmts, qs), kw = batch_args(requests_)
    datas = [r[0] for r in requests_]
    c0 = counters(ik)
    with pytest.raises(TransformError, match="item %d" % FAILED):
        transform_batch(datas, sizes, fmts, qs, **kw)
    assert np.array_equal(counters(ik) - c0, (ADJUST, BLUR, OVERLAY))

    def raw():
        size, rc, res, status = raw_batch(ik, requests_, kw)
        assert size == 80
        return rc, res, status

    check(ik, alone, raw)


def test_other_counters_move_as_without_adjustments(ik, requests_, alone):
    """the same batch with no adjustment anywhere: the 56-byte layout, the adjust counters still,
    the blur and overlay counters as above, and the unadjusted requests' bytes as before"""
    (sizes, fmts, qs), kw = batch_args(requests_)
    kw = dict(kw, adjusts=None)
    c0 = counters(ik)
    size, rc, outs, status = raw_batch(ik, requests_, kw)
    assert size == 56 and rc != 0 and "item %d" % FAILED in _lib.last_error()
    assert np.array_equal(counters(ik) - c0, ((0, 0), BLUR, OVERLAY))
    assert outs[3] == alone[3] and outs[8] == alone[8] and outs[0] != alone[0]


def test_transform_batch_submit(ik, requests_, alone):
    (sizes, fmts, qs), kw = batch_args(requests_)
    datas = [r[0] for r in requests_]
    check(ik, alone, lambda: wait_all(ik, transform_batch_submit(datas, sizes, fmts, qs, **kw)))
    c0 = counters(ik)
    with pytest.raises(TransformError, match="item %d" % FAILED):
        transform_batch_submit(datas, sizes, fmts, qs, **kw).wait()
    assert np.array_equal(counters(ik) - c0, (ADJUST, BLUR, OVERLAY))


def test_transform_batch_submit_device(ik, requests_, alone):
    (sizes, fmts, qs), kw = batch_args(requests_)
    assert ik.ik_set_png_gpu_min(0) == 0
    try:
        dev = [DeviceBytes(r[0]) for r in requests_]
        check(ik, alone, lambda: wait_all(ik, transform_batch_submit_device(dev, sizes, fmts, qs, **kw)))
    finally:
        ik.ik_set_png_gpu_min(256 << 10)
