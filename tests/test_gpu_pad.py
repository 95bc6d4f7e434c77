"""GPU: the pad kernel.  Everything is compared with zero tolerance against tests/pad_model.py
(np.pad): every format and mode with many folds, a ragged row end and several workgroups per
row; the sizes around a workgroup's span; every byte offset of the interior against the dword
grid; one-sided pads; the grid stride; the frame pixel; a source with a wide pitch and
poisoned padding; a caller's canvas area with poison around every row; and the pad that
changes nothing."""
import ctypes

import numpy as np
import pytest

import pad_model as pm
from imagekit import DynamicImage, Pad, _lib

pytestmark = pytest.mark.gpu
POISON = 0xA5
IK_ERR_INVALID = 2
FORMATS = [(C, d) for d in (1, 2) for C in (1, 2, 3, 4)]
MODES = {pm.COLOR: "color", pm.EDGE: "edge", pm.MIRROR: "mirror", pm.WRAP: "wrap"}
GRAVITY = {pm.CENTER: "center", pm.N: "n", pm.S: "s", pm.E: "e", pm.W: "w", pm.NE: "ne", pm.NW: "nw", pm.SE: "se",
           pm.SW: "sw"}


def counters(ik):
    c = (ctypes.c_ulonglong * 2)()
    assert ik.ik_pad_counters(c) == 0
    return np.array([c[0], c[1]], dtype=np.int64)


def noise(H, W, C, depth, seed):
    """random samples, every one of them different from its neighbours with near certainty"""
    M = 256 ** depth - 1
    return np.random.default_rng(seed).integers(0, M + 1, (H, W, C)).astype(np.uint8 if depth == 1 else np.uint16)


def device_pad(img, mode, gravity=pm.CENTER, width=0, height=0, color=0, alpha=0):
    C = img.shape[2]
    d = DynamicImage.from_array(img[..., 0] if C == 1 else img)
    out = d.pad(Pad(MODES[mode], GRAVITY[gravity], width, height, color, alpha))
    cw, ch, _, _ = pm.place(img.shape[1], img.shape[0], width, height, gravity)
    assert out.dimensions() == (cw, ch) and out.depth == img.dtype.itemsize
    assert np.array_equal(d.to_array().reshape(img.shape), img)  # the source is not changed
    return out.to_array().reshape(ch, cw, C)


def check(img, mode, **kw):
    got, want = device_pad(img, mode, **kw), pm.pad(img, mode, **kw)
    assert np.array_equal(got, want), (MODES[mode], kw, np.argwhere(got != want)[:4].tolist())


@pytest.mark.parametrize("C,depth", FORMATS, ids=lambda v: str(v))
def test_kernel_equals_model(ik, C, depth):
    """5 x 3 in (2S + 7) x 11: hundreds of folds of mirror and wrap, three workgroups per row,
    a ragged row end"""
    S = ik.ik_pad_span()
    img = noise(3, 5, C, depth, seed=10 * C + depth)
    c0 = counters(ik)
    for mode in MODES:
        check(img, mode, width=2 * S + 7, height=11, color=0x3366CC, alpha=77)
    assert np.array_equal(counters(ik) - c0, (4, 4))


@pytest.mark.parametrize("mode", [pm.EDGE, pm.MIRROR, pm.WRAP])
def test_one_pixel_image(ik, mode):
    for C, depth in ((1, 1), (3, 1), (4, 2)):
        check(noise(1, 1, C, depth, seed=3), mode, width=9, height=7)


@pytest.mark.parametrize("dw", [-1, 0, 1])
def test_widths_around_the_span(ik, dw):
    """a 3-pixel frame around an image one short of, at and one past a workgroup's span"""
    W = ik.ik_pad_span() + dw
    for (C, depth), mode in (((3, 1), pm.MIRROR), ((3, 1), pm.COLOR), ((4, 2), pm.WRAP), ((1, 1), pm.EDGE)):
        check(noise(4, W, C, depth, seed=20 + dw), mode, width=W + 6, height=10, color=0x804020, alpha=9)


@pytest.mark.parametrize("gravity", [pm.W, pm.E])
def test_interior_byte_offsets(ik, gravity):
    """RGB8 with k = 0..6 frame columns on one side: the interior starts 0, 3, ..., 18 bytes
    from the row start (gravity E), or ends that far from the row end (gravity W)"""
    img = noise(3, 37, 3, 1, seed=41)
    for k in range(7):
        for mode in MODES:
            check(img, mode, gravity=gravity, width=37 + k, color=0x0A141E)


@pytest.mark.parametrize("gravity", [pm.N, pm.S, pm.E, pm.W])
def test_one_sided_pads(ik, gravity):
    img = noise(6, 21, 4, 1, seed=43)
    vertical = gravity in (pm.N, pm.S)
    for mode in MODES:
        check(img, mode, gravity=gravity, width=0 if vertical else 21 + 9, height=6 + 5 if vertical else 0,
              color=0x112233, alpha=200)


def test_rows_beyond_the_row_cap(ik):
    """a 2-pixel-wide image of R + 3 rows: the last rows are reached by the grid stride"""
    R = ik.ik_pad_row_cap()
    for (C, depth), mode in (((1, 1), pm.MIRROR), ((3, 1), pm.COLOR), ((2, 2), pm.WRAP)):
        img = noise(R + 3, 2, C, depth, seed=47)
        check(img, mode, width=7, color=0xC0FFEE, alpha=1)
        check(img, mode, gravity=pm.S, width=5, height=R + 6, color=0xC0FFEE, alpha=1)


@pytest.mark.parametrize("C,depth", [(1, 1), (2, 1), (1, 2), (2, 2)], ids=lambda v: str(v))
def test_gray_image_under_a_colour(ik, C, depth):
    img = noise(4, 6, C, depth, seed=51)
    got = device_pad(img, pm.COLOR, width=12, height=8, color=0xFF8000, alpha=255)
    s = 1 if depth == 1 else 257
    luma = (2126 * 255 * s + 7152 * 128 * s) // 10000
    assert got[0, 0, 0] == luma and luma not in (255 * s, 128 * s, 0)
    assert np.array_equal(got, pm.pad(img, pm.COLOR, width=12, height=8, color=0xFF8000, alpha=255))


@pytest.mark.parametrize("alpha", [0, 128, 255])
def test_frame_alpha(ik, alpha):
    for C, depth in ((2, 1), (4, 1), (2, 2), (4, 2)):
        img = noise(5, 7, C, depth, seed=53)
        got = device_pad(img, pm.COLOR, gravity=pm.NW, width=19, height=9, color=0x204060, alpha=alpha)
        assert got[8, 18, C - 1] == alpha * (1 if depth == 1 else 257)
        assert np.array_equal(got, pm.pad(img, pm.COLOR, gravity=pm.NW, width=19, height=9, color=0x204060, alpha=alpha))


def wrapped(ik, torch, img, pitch, off, poison):
    """img in a device buffer with `pitch` bytes per row from byte `off`, everything else
    `poison`, as an image handle over it"""
    H, W, C = img.shape
    row = W * C
    buf = np.full(off + pitch * H + 64, poison, np.uint8)
    buf[off:off + pitch * H].reshape(H, pitch)[:, :row] = img.reshape(H, row)
    dev = torch.from_numpy(buf).cuda()
    torch.cuda.synchronize()
    h = ctypes.c_void_p()
    assert ik.ik_image_wrap_device(dev.data_ptr() + off, W, H, C, pitch, ctypes.byref(h)) == 0, _lib.last_error()
    return dev, DynamicImage(h.value)


@pytest.mark.parametrize("off", [0, 1, 2, 3])
def test_wide_pitch_with_poisoned_padding(ik, off):
    """the source's pitch padding reaches no output: two poisons, one result, the model's.  The
    base is `off` bytes from a dword, so the interior's loads are misaligned however it lies"""
    import torch
    img = noise(5, 45, 3, 1, seed=59)
    for mode in MODES:
        outs = []
        for poison in (0xA5, 0x5A):
            dev, d = wrapped(ik, torch, img, pitch=45 * 3 + 29, off=off, poison=poison)
            outs.append(d.pad(Pad(MODES[mode], "center", 45 + 11, 5 + 4, 0x010203)).to_array())
            del d, dev
        want = pm.pad(img, mode, width=45 + 11, height=5 + 4, color=0x010203)
        assert np.array_equal(outs[0], want) and np.array_equal(outs[1], want), MODES[mode]


@pytest.mark.parametrize("C,depth", [(3, 1), (1, 1), (4, 2)], ids=lambda v: str(v))
def test_raw_call_writes_the_canvas_rows_only(ik, C, depth):
    """ik_pad_batch_device over two images in a caller's areas: the canvases equal the model and
    no byte of the canvas's pitch padding, or between and around the canvases, is written"""
    import torch
    n, H, W, cw, ch = 2, 5, 19, 19 + 10, 5 + 3
    imgs = np.stack([noise(H, W, C, depth, seed=61 + i) for i in range(n)])
    srow, drow = W * C * depth, cw * C * depth
    sp, dp = srow + 7, (drow + 3) // 4 * 4 + 12
    ss, dstride = sp * H + 5, dp * ch + 40
    src = np.full(n * ss + 64, POISON, np.uint8)
    for i in range(n):
        src[i * ss:i * ss + sp * H].reshape(H, sp)[:, :srow] = np.ascontiguousarray(imgs[i]).view(np.uint8).reshape(H, srow)
    dsrc = torch.from_numpy(src).cuda()
    for mode in MODES:
        ddst = torch.full((8 + n * dstride + 64,), POISON, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        p = Pad(MODES[mode], "se", 0, 0, 0x778899, 33)._struct()
        c0 = counters(ik)
        rc = ik.ik_pad_batch_device(dsrc.data_ptr(), W, H, C, depth, sp, ss, n, ctypes.byref(p), cw, ch,
                                    ddst.data_ptr() + 8, dp, dstride, None)
        assert rc == 0, _lib.last_error()
        assert ik.ik_dev_synchronize() == 0
        assert np.array_equal(counters(ik) - c0, (1, n))
        got = ddst.cpu().numpy()
        keep = np.ones(got.size, bool)
        for i in range(n):
            lo = 8 + i * dstride
            out = got[lo:lo + dp * ch].reshape(ch, dp)[:, :drow].copy().view(imgs.dtype).reshape(ch, cw, C)
            keep[lo:lo + dp * ch].reshape(ch, dp)[:, :drow] = False
            want = pm.pad(imgs[i], mode, gravity=pm.SE, width=cw, height=ch, color=0x778899, alpha=33)
            assert np.array_equal(out, want), (MODES[mode], i)
        assert (got[keep] == POISON).all(), "a store outside the cw * C * depth bytes of a canvas row"


def test_raw_call_refusals(ik):
    import torch
    src = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    dst = torch.zeros(8192, dtype=torch.uint8, device="cuda")
    ok = Pad("edge")._struct()
    names = ["src", "W", "H", "C", "depth", "sp", "ss", "n", "pad", "cw", "ch", "dst", "dp", "ds", "stream"]
    good = [src.data_ptr(), 6, 4, 3, 1, 20, 80, 2, ctypes.byref(ok), 9, 6, dst.data_ptr(), 28, 168, None]
    c0 = counters(ik)
    for k, v in (("src", None), ("dst", None), ("pad", None), ("W", 0), ("H", 0), ("n", 0), ("C", 0), ("C", 5),
                 ("depth", 3), ("sp", 17), ("dp", 24), ("ss", 79), ("ds", 164), ("n", 65536), ("cw", 5), ("ch", 3),
                 ("cw", (1 << 24) + 1), ("dp", 30), ("ds", 170), ("dst", dst.data_ptr() + 2), ("dst", src.data_ptr() + 8)):
        a = list(good)
        a[names.index(k)] = v
        assert ik.ik_pad_batch_device(*a) == IK_ERR_INVALID, (k, v)
        assert _lib.last_error()
    none = _lib.Pad()
    a = list(good)
    a[8] = ctypes.byref(none)
    assert ik.ik_pad_batch_device(*a) == IK_ERR_INVALID and "mode" in _lib.last_error()
    assert ik.ik_dev_synchronize() == 0
    assert np.array_equal(counters(ik), c0), "a refused call counted a launch"
    assert not dst.cpu().numpy().any()
    # the handle call refuses IK_PAD_NONE and an empty image under a larger canvas
    d = DynamicImage.from_array(noise(3, 4, 3, 1, seed=1))
    out = ctypes.c_void_p()
    assert ik.ik_image_pad(d._h, ctypes.byref(none), ctypes.byref(out)) == IK_ERR_INVALID and "mode" in _lib.last_error()


def test_canvas_equal_to_the_image_launches_nothing(ik):
    img = noise(9, 13, 4, 1, seed=5)
    d = DynamicImage.from_array(img)
    c0 = counters(ik)
    for p in (Pad(), Pad("mirror", "se", 13, 9), Pad("wrap", "n", 5, 4), Pad("edge", width=13)):
        cp = d.pad(p)
        assert cp._h.value != d._h.value and cp.dimensions() == (13, 9)
        assert np.array_equal(cp.to_array(), img)
    assert np.array_equal(counters(ik), c0)
