"""GPU parity for k_avif_yuv444, the AVIF branch's device front end (reference
src/transform.rs:138-146 -> image AvifEncoder -> to_rgba8 -> ravif RGB->YCbCr).

Everything goes through ik_avif_yuv444_device, which returns what the kernel wrote: the
Y, U, V, A planes and the per-image transparent flag that decides whether the AVIF file
carries an alpha plane.  They are compared value for value with the oracle's restatement of
ravif 0.11.20 (oracle/avif_yuv.c, checked on its own in tests/test_oracle_avif.py): on every
colour, at the widths where a row ends inside, on and just past a wave and a workgroup, for
C = 1..4, with padded rows, in a batch with gaps between the images and between their
planes, and with one translucent pixel at each place where a flag could get lost.  The
plane buffer and the flags are filled with a canary before each call, so a write past an
image's planes or a flag that was never zeroed shows."""
import ctypes

import numpy as np
import pytest

import ikutil

pytestmark = pytest.mark.gpu

IK_ERR_INVALID = 2
CANARY = 0xC5
FLAG_CANARY = 0x5A5A5A5A
PAD = 0x3C  # row padding and inter-image gaps of the source: a non-zero, non-255 byte


class _Dev:
    """Device buffers of one call, freed on exit."""

    def __init__(self, ik):
        self.ik, self.ptrs = ik, []

    def alloc(self, host: np.ndarray) -> ctypes.c_void_p:
        p = ctypes.c_void_p()
        assert self.ik.ik_dev_alloc(host.nbytes, ctypes.byref(p)) == 0
        self.ptrs.append(p)
        assert self.ik.ik_memcpy_h2d(p, host.ctypes.data, host.nbytes) == 0
        return p

    def fetch(self, p, host: np.ndarray) -> np.ndarray:
        assert self.ik.ik_memcpy_d2h(host.ctypes.data, p, host.nbytes) == 0
        return host

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for p in self.ptrs:
            self.ik.ik_dev_free(p)


def _source(imgs, pitch, img_stride):
    """n same-shape (h, w, C) images, rows `pitch` apart, images `img_stride` apart, every
    byte that is no pixel set to PAD."""
    h, w, c = imgs[0].shape
    buf = np.full(len(imgs) * img_stride + 16, PAD, np.uint8)
    for i, img in enumerate(imgs):
        rows = buf[i * img_stride:i * img_stride + h * pitch].reshape(h, pitch)
        rows[:, :w * c] = img.reshape(h, w * c)
    return buf


def _front(ik, imgs, pitch=None, img_stride=None, plane_stride=None):
    """Run the kernel on a batch; returns ([(Y, U, V, A)] per image, flags, the bytes of the
    plane buffer outside the images' planes, the int after the last flag)."""
    from imagekit import _lib
    n = len(imgs)
    h, w, c = imgs[0].shape
    npix = w * h
    pitch = pitch or ((w * c + 255) // 256) * 256
    img_stride = img_stride or h * pitch
    plane_stride = plane_stride or 4 * npix
    tail = 64
    planes = np.full(n * plane_stride + tail, CANARY, np.uint8)
    flags = np.full(n + 1, FLAG_CANARY, np.uint32)
    with _Dev(ik) as dev:
        ds = dev.alloc(_source(imgs, pitch, img_stride))
        dp, df = dev.alloc(planes), dev.alloc(flags)
        rc = ik.ik_avif_yuv444_device(ds, w, h, c, pitch, img_stride, n, dp, plane_stride, df, None)
        assert rc == 0, _lib.last_error()
        assert ik.ik_dev_synchronize() == 0
        dev.fetch(dp, planes)
        dev.fetch(df, flags)
    out, outside = [], np.ones(planes.size, bool)
    for i in range(n):
        o = i * plane_stride
        out.append(tuple(planes[o + k * npix:o + (k + 1) * npix].reshape(h, w) for k in range(4)))
        outside[o:o + 4 * npix] = False
    return out, flags[:n].astype(np.int64).tolist(), planes[outside], int(flags[n])


def _assert_planes(got, want, img, what=""):
    """Planes equal the oracle's; a failure names the plane and the first differing pixels
    with their source values."""
    msgs = []
    for name, g, w in zip("YUVA", got, want):
        bad = np.argwhere(g != w)
        if len(bad):
            first = ["(x %d, y %d) source %s: got %d, oracle %d" % (x, y, img[y, x].tolist(), g[y, x], w[y, x])
                     for y, x in bad[:8]]
            msgs.append("plane %s differs from the oracle at %d of %d pixels; first: %s"
                        % (name, len(bad), g.size, "; ".join(first)))
    assert not msgs, (what + ": " if what else "") + "\n".join(msgs)


def _check(ik, oracle, imgs, want_flags=None, **kw):
    got, flags, outside, guard = _front(ik, imgs, **kw)
    for i, img in enumerate(imgs):
        want = oracle.avif_yuv444(img)
        _assert_planes(got[i], want[:4], img, "image %d of %d" % (i, len(imgs)))
        assert flags[i] == want[4], "flags %s, image %d: oracle %d" % (flags, i, want[4])
    if want_flags is not None:
        assert flags == want_flags
    assert (outside == CANARY).all(), "bytes outside the images' planes were written"
    assert guard == FLAG_CANARY, "the int after the last flag was written"


def test_every_colour(ik, oracle):
    """One 4096 x 4096 RGB image holding each of the 2^24 colours once (pixel index =
    r<<16 | g<<8 | b): Y, U and V equal the oracle on all of them, A is 255, the flag 0."""
    idx = np.arange(1 << 24, dtype=np.uint32)
    img = np.stack([idx >> 16, (idx >> 8) & 255, idx & 255], -1).astype(np.uint8).reshape(4096, 4096, 3)
    del idx
    got, flags, outside, guard = _front(ik, [img])
    want = oracle.avif_yuv444(img)
    _assert_planes(got[0], want[:4], img)
    assert (got[0][3] == 255).all()
    assert flags == [0] and want[4] == 0
    assert (outside == CANARY).all() and guard == FLAG_CANARY


@pytest.mark.parametrize("c", [1, 2, 3, 4])
@pytest.mark.parametrize("h", [1, 3])
@pytest.mark.parametrize("w", [1, 63, 64, 65, 255, 256, 257, 300])
def test_shapes(ik, oracle, w, h, c):
    """Rows that end inside, on and one past a wave (64) and a workgroup (256), every channel
    count, noise with random alpha, rows padded to 256 bytes with non-zero padding."""
    _check(ik, oracle, [ikutil.synth(w, h, c, seed=w * 8 + h + c, pattern="N", alpha="random")])


FLAG_XS = [0, 63, 64, 255, 256, -1]


@pytest.mark.parametrize("c", [2, 4])
@pytest.mark.parametrize("w", [65, 257, 300])
def test_flag_one_translucent_pixel(ik, oracle, w, c):
    """An opaque image with a single translucent pixel: in lane 0 and lane 63 of a wave, in
    the first lane of the next wave, on both sides of a workgroup edge and in the last
    pixel of a row (the last, partial workgroup), on the first and the last row, with
    alpha 254 and 0.  The flag is 1 every time, and 0 for the opaque image itself."""
    h = 3
    img = ikutil.synth(w, h, c, seed=w + c, pattern="N")
    assert (img[..., -1] == 255).all()
    _check(ik, oracle, [img], want_flags=[0])
    for y in (0, h - 1):
        for x in sorted({x % w for x in FLAG_XS if x < w}):
            for alpha in (254, 0):
                one = img.copy()
                one[y, x, -1] = alpha
                try:
                    _check(ik, oracle, [one], want_flags=[1])
                except AssertionError as e:
                    raise AssertionError("alpha %d at (x %d, y %d) of %d x %d, C %d: %s" % (alpha, x, y, w, h, c, e))


@pytest.mark.parametrize("c", [1, 3])
@pytest.mark.parametrize("w", [65, 257, 300])
def test_flag_stays_clear_without_alpha_channel(ik, oracle, w, c):
    """C = 1 and C = 3 have no alpha: the flag is 0 whatever the bytes are (noise, all 0,
    all 254), and A is 255."""
    h = 3
    for img in (ikutil.synth(w, h, c, seed=w, pattern="N"), np.zeros((h, w, c), np.uint8),
                np.full((h, w, c), 254, np.uint8)):
        _check(ik, oracle, [img], want_flags=[0])


@pytest.mark.parametrize("which", [1, 0, 2])
def test_batch_flags_and_strides(ik, oracle, which):
    """Three 70 x 5 RGBA images in one launch, the source images further apart than their
    rows need, the plane sets 96 bytes apart: planes per image equal the oracle, only the
    image with the translucent pixel raises its flag, the gaps keep the canary."""
    w, h, c, n = 70, 5, 4, 3
    imgs = [ikutil.synth(w, h, c, seed=40 + i, pattern="N") for i in range(n)]
    imgs[which][h - 1, w - 1, 3] = 254
    pitch = ((w * c + 255) // 256) * 256
    want = [0] * n
    want[which] = 1
    _check(ik, oracle, imgs, want_flags=want, pitch=pitch, img_stride=h * pitch + 512,
           plane_stride=4 * w * h + 96)


def test_bad_arguments_write_nothing(ik):
    w, h, c, n = 20, 4, 4, 2
    pitch, npix = 256, w * h
    img_stride, plane_stride = h * pitch, 4 * npix
    imgs = [ikutil.synth(w, h, c, seed=i, pattern="N", alpha="random") for i in range(n)]
    planes = np.full(n * plane_stride + 64, CANARY, np.uint8)
    flags = np.full(n + 1, FLAG_CANARY, np.uint32)
    with _Dev(ik) as dev:
        ds = dev.alloc(_source(imgs, pitch, img_stride))
        dp, df = dev.alloc(planes), dev.alloc(flags)
        good = dict(src=ds, w=w, h=h, c=c, pitch=pitch, img_stride=img_stride, n=n, planes=dp,
                    plane_stride=plane_stride, flags=df)
        bad = [dict(src=None), dict(planes=None), dict(flags=None), dict(w=0), dict(h=0), dict(c=0), dict(c=5),
               dict(n=0), dict(plane_stride=4 * npix - 1), dict(plane_stride=0), dict(pitch=w * c - 1),
               dict(img_stride=h * pitch - 1)]
        for change in bad:
            a = dict(good, **change)
            rc = ik.ik_avif_yuv444_device(a["src"], a["w"], a["h"], a["c"], a["pitch"], a["img_stride"], a["n"],
                                          a["planes"], a["plane_stride"], a["flags"], None)
            assert rc == IK_ERR_INVALID, "%s: returned %d" % (change, rc)
        assert ik.ik_dev_synchronize() == 0
        assert (dev.fetch(dp, planes) == CANARY).all()
        assert (dev.fetch(df, flags) == FLAG_CANARY).all()
        # the same buffers, good arguments: the call does write them
        a = good
        assert ik.ik_avif_yuv444_device(a["src"], a["w"], a["h"], a["c"], a["pitch"], a["img_stride"], a["n"],
                                        a["planes"], a["plane_stride"], a["flags"], None) == 0
        assert ik.ik_dev_synchronize() == 0
        assert dev.fetch(df, flags).tolist() == [1, 1, FLAG_CANARY]
        assert (dev.fetch(dp, planes)[:n * plane_stride] != CANARY).any()
