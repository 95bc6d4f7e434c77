"""GPU: every per-request option through one batch.  Each option's own test file checks that
option with at most the earlier ones beside it; here ten requests carry orientation, background,
blur or sharpen and a watermark together, chosen so that every stage of the post stage sees a
group of several, a lone member and a member it must leave alone.  Every output is compared with
the same request through transform() alone, byte for byte, and the flatten, blur and overlay
launch counters with the launches that follow from who shares what."""
import ctypes
import io

import numpy as np
import pytest
from PIL import Image

import ikutil
from imagekit import (DeviceBytes, DynamicImage, ImageFormat, Orientation, Overlay, TransformError, _lib,
                      transform_batch, transform_batch_submit, transform_batch_submit_device)
from imagekit.transform import _inputs, _request_opts, transform

pytestmark = pytest.mark.gpu
J, WP = ImageFormat.jpeg, ImageFormat.webp
WHITE, OTHER = 0xFFFFFF, 0x102030
FAILED = 9  # the truncated file's place in the batch


def png_of(img):
    b = io.BytesIO()
    Image.fromarray(img, {3: "RGB", 4: "RGBA"}[img.shape[2]]).save(b, format="PNG")
    return b.getvalue()


def noise(H, W, C, seed):
    """random samples with plenty of alpha 0 and alpha 255"""
    r = np.random.default_rng(seed).integers(0, 256, (H, W, C))
    r[..., C - 1][r[..., C - 1] % 5 == 0] = 0
    r[..., C - 1][r[..., C - 1] % 5 == 1] = 255
    return r.astype(np.uint8)


@pytest.fixture(scope="module")
def requests_(ik):
    """(data, (w, h), orientation, background, blur, sharpen, overlay, fmt, quality) per request"""
    a1 = png_of(ikutil.synth(96, 64, 4, seed=41, pattern="S", alpha="random"))
    a2 = png_of(ikutil.synth(96, 64, 4, seed=42, pattern="S", alpha="random"))
    rgb = png_of(ikutil.synth(96, 64, 3, seed=43, pattern="S"))
    other = png_of(ikutil.synth(72, 48, 3, seed=44, pattern="S"))
    m0 = DynamicImage.from_array(noise(10, 24, 4, seed=45))
    m1 = DynamicImage.from_array(noise(6, 6, 2, seed=46))
    share = Overlay(m0, "se", -2, -2, 200)
    tiled = Overlay(m1, tile=True, opacity=90)
    st = Orientation.stored
    return [
        (a1, (32, 48), 6, WHITE, None, 1.5, share, J, 85),      # 0, 1: a pair that shares every stage
        (a2, (32, 48), 6, WHITE, None, 1.5, share, J, 85),
        (a1, (48, 32), 3, WHITE, None, 1.5, share, J, 85),      # 2: turned alone, another geometry
        (a2, (32, 48), 6, OTHER, None, 1.5, share, WP, 80),     # 3: flattened alone, then with the pair again
        (a1, (32, 48), 6, WHITE, 1.0, None, None, J, 85),       # 4: with the pair up to the resize; its own filter, no mark
        (rgb, (48, 32), st, WHITE, None, None, None, J, 85),    # 5: no alpha: the background changes nothing
        (rgb, (None, None), st, None, 2.0, None, tiled, WP, 80),  # 6: no resize: filter and mark on the decoded image
        (rgb, (48, 32), st, None, None, None, None, WP, 80),    # 7: every option at its default
        (other, (36, 24), st, None, 1.0, None, tiled, J, 85),   # 8: alone at every stage
        (a1[:len(a1) // 2], (32, 48), 6, WHITE, None, 1.5, share, J, 85),  # 9: truncated: its own decode status
    ]


# Who shares a launch (csrc/ik_post_stage.cpp; a set of one takes the per-image call, which
# launches and counts as a set of one would):
#   orientation  {0, 1, 3, 4} are 96x64 RGBA turned by 6, {2} by 3 (no counter)
#   flatten      64x96 RGBA onto white {0, 1, 4}, onto the other colour {3}, 96x64 RGBA onto white
#                {2}; 5 has a background and no alpha, 6..8 have none: 3 launches, 5 images
#   resize       64x96 RGB -> 32x48 {0, 1, 3, 4}; 96x64 RGB -> 48x32 {2, 5, 7}; 6 is not resized
#                and 8 is the only one of its geometry: neither is in a group
#   filter       inside the first group sharpen 1.5 {0, 1, 3} and blur 1.0 {4}; inside the second
#                {2}; image by image 6 and 8: 5 launches, 7 images
#   watermark    inside the first group the shared mark {0, 1, 3}; inside the second {2}; image by
#                image 6 and 8: 4 launches, 6 images
# The truncated file fails in the decoder and reaches none of them.
FLATTEN, BLUR, OVERLAY = (3, 5), (5, 7), (4, 6)


def counters(ik):
    out = []
    for fn in (ik.ik_flatten_counters, ik.ik_blur_counters, ik.ik_overlay_counters):
        c = (ctypes.c_ulonglong * 2)()
        assert fn(c) == 0
        out.append((int(c[0]), int(c[1])))
    return np.array(out, dtype=np.int64)


def alone_(reqs):
    out = []
    for i, (data, (w, h), o, bg, blur, sharpen, ov, fmt, q) in enumerate(reqs):
        if i == FAILED:
            with pytest.raises(TransformError):
                transform(data, w, h, fmt, q, orient=o, background=bg, blur=blur, sharpen=sharpen, overlay=ov)
            out.append(None)
        else:
            out.append(transform(data, w, h, fmt, q, orient=o, background=bg, blur=blur, sharpen=sharpen, overlay=ov))
    return out


@pytest.fixture(scope="module")
def alone(ik, requests_):
    """each request through transform() by itself, computed once (None: the truncated file)"""
    return alone_(requests_)


def batch_args(reqs):
    args = ([r[1] for r in reqs], [r[7] for r in reqs], [r[8] for r in reqs])
    kw = dict(orient=[r[2] for r in reqs], backgrounds=[r[3] for r in reqs], blurs=[r[4] for r in reqs],
              sharpens=[r[5] for r in reqs], overlays=[r[6] for r in reqs])
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


def check(ik, alone, run):
    c0 = counters(ik)
    rc, outs, status = run()
    delta = counters(ik) - c0
    print("flatten, blur, overlay (launches, images):", delta.tolist())
    assert rc != 0 and "item %d" % FAILED in _lib.last_error()
    assert np.array_equal(delta, (FLATTEN, BLUR, OVERLAY)), delta.tolist()
    assert [s != 0 for s in status] == [i == FAILED for i in range(len(status))], status
    assert outs[FAILED] is None
    for i, want in enumerate(alone):
        assert outs[i] == want, i


def test_requests_differ_where_their_options_do(alone):
    assert len(set(a for a in alone if a is not None)) == len(alone) - 1
    assert all(alone[i] for i in range(len(alone)) if i != FAILED)


def test_transform_batch(ik, requests_, alone):
    reqs = requests_
    (sizes, fmts, qs), kw = batch_args(reqs)
    datas = [r[0] for r in reqs]
    # the Python call raises for the failed request; the whole batch has run by then
    c0 = counters(ik)
    with pytest.raises(TransformError, match="item %d" % FAILED):
        transform_batch(datas, sizes, fmts, qs, **kw)
    assert np.array_equal(counters(ik) - c0, (FLATTEN, BLUR, OVERLAY))

    def raw():  # the same C call with the same options array, every output and status kept
        n = len(reqs)
        keep, ptrs, lens = _inputs(datas)
        ws = (ctypes.c_int64 * n)(*[-1 if s[0] is None else s[0] for s in sizes])
        hs = (ctypes.c_int64 * n)(*[-1 if s[1] is None else s[1] for s in sizes])
        fs = (ctypes.c_int * n)(*[int(f.value) for f in fmts])
        qa = (ctypes.c_int * n)(*qs)
        ra = _request_opts(n, None, kw["orient"], kw["backgrounds"], kw["blurs"], kw["sharpens"], kw["overlays"])
        assert ctypes.sizeof(ra._type_) == 56
        outs, olens, status = (ctypes.c_void_p * n)(), (ctypes.c_size_t * n)(), (ctypes.c_int * n)()
        rc = ik.ik_transform_batch_opts(ptrs, lens, n, ws, hs, ra, 56, fs, qa, 4, 0, outs, olens, status)
        res = []
        for i in range(n):
            res.append(ctypes.string_at(outs[i], olens[i]) if outs[i] else None)
            if outs[i]:
                ik.ik_buf_free(outs[i])
        return rc, res, list(status)

    check(ik, alone, raw)


def test_transform_batch_submit(ik, requests_, alone):
    (sizes, fmts, qs), kw = batch_args(requests_)
    datas = [r[0] for r in requests_]
    check(ik, alone, lambda: wait_all(ik, transform_batch_submit(datas, sizes, fmts, qs, **kw)))
    c0 = counters(ik)
    with pytest.raises(TransformError, match="item %d" % FAILED):
        transform_batch_submit(datas, sizes, fmts, qs, **kw).wait()
    assert np.array_equal(counters(ik) - c0, (FLATTEN, BLUR, OVERLAY))


def test_transform_batch_submit_device(ik, requests_, alone):
    (sizes, fmts, qs), kw = batch_args(requests_)
    assert ik.ik_set_png_gpu_min(0) == 0
    try:
        dev = [DeviceBytes(r[0]) for r in requests_]
        check(ik, alone, lambda: wait_all(ik, transform_batch_submit_device(dev, sizes, fmts, qs, **kw)))
        c0 = counters(ik)
        with pytest.raises(TransformError, match="item %d" % FAILED):
            transform_batch_submit_device(dev, sizes, fmts, qs, **kw).wait()
        assert np.array_equal(counters(ik) - c0, (FLATTEN, BLUR, OVERLAY))
    finally:
        ik.ik_set_png_gpu_min(256 << 10)
