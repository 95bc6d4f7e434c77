"""GPU: the exact WebP coder's mixed call (ik_webp_encode_exact_items: images of different
sizes and qualities in one analysis, one set-up and one k_vp8x_run_mixed launch) and the
batch path behind ik_set_webp_mixed(IK_WEBP_MIXED_GPU).

Bar, as for the uniform call (tests/test_gpu_vp8x.py): every file is byte-identical to
WebPEncodeRGB(to_rgb8(img), q) -- the reference codes WebP with libwebp (reference
src/transform.rs:129-137).  All frames are tiny; the geometries are the plan test's."""
import ctypes
import io

import numpy as np
import pytest

import ikutil
import vp8_content
import vp8_parse
from imagekit import _lib
from test_gpu_vp8x import encode_exact, first_diff
from test_vp8x_mixed_plan import GEOMETRIES

pytestmark = pytest.mark.gpu

IK_ERR_INVALID = 2
MIXED_HOST, MIXED_GPU = 0, 1


def _planes_bytes(w, h):
    return w * h + 2 * ((w + 1) // 2) * ((h + 1) // 2)


def _device_planes(ik, imgs, gaps=None):
    """Every image through ik_webp_yuv420_device into one device buffer, each at a
    256-byte aligned offset of its own, gaps[i] more bytes (a multiple of 256) left free
    after image i; returns (buffer, addresses)."""
    offs, total = [], 0
    for i, img in enumerate(imgs):
        h, w, _ = img.shape
        offs.append(total)
        total += (_planes_bytes(w, h) + 255) // 256 * 256 + (gaps[i] if gaps and i < len(gaps) else 0)
    dy = ctypes.c_void_p()
    assert ik.ik_dev_alloc(total, ctypes.byref(dy)) == 0
    for img, off in zip(imgs, offs):
        h, w, c = img.shape
        pitch = ((w * c + 255) // 256) * 256
        ds = ctypes.c_void_p()
        assert ik.ik_dev_alloc(pitch * h + 16, ctypes.byref(ds)) == 0
        buf = np.zeros((h, pitch), np.uint8)
        buf[:, :w * c] = img.reshape(h, w * c)
        assert ik.ik_memcpy_h2d(ds, buf.ctypes.data, buf.nbytes) == 0
        assert ik.ik_webp_yuv420_device(ds, w, h, c, pitch, ctypes.c_void_p(dy.value + off), None) == 0, \
            _lib.last_error()
        assert ik.ik_dev_synchronize() == 0
        ik.ik_dev_free(ds)
    return dy, [dy.value + o for o in offs]


def encode_items(ik, imgs, qs, gaps=None):
    """The files of ik_webp_encode_exact_items for imgs[i] at quality qs[i]."""
    n = len(imgs)
    dy, addr = _device_planes(ik, imgs, gaps)
    items = (_lib.WebpExactItem * n)()
    for i, img in enumerate(imgs):
        items[i] = _lib.WebpExactItem(addr[i], img.shape[1], img.shape[0], int(qs[i]))
    outs = (_lib.u8p * n)()
    lens = (ctypes.c_size_t * n)()
    try:
        assert ik.ik_webp_encode_exact_items(items, n, ctypes.cast(outs, ctypes.c_void_p),
                                             ctypes.cast(lens, ctypes.c_void_p)) == 0, _lib.last_error()
    finally:
        ik.ik_dev_free(dy)
    files = []
    for i in range(n):
        files.append(ctypes.string_at(outs[i], lens[i]))
        ik.ik_buf_free(outs[i])
    return files


def counters(ik):
    c = (ctypes.c_ulonglong * 4)()
    assert ik.ik_webp_enc_counters(c) == 0
    return list(c)


def check(got, want, what):
    if got != want:
        pytest.fail(f"{what}: differs at byte {first_diff(got, want)} ({len(got)} vs {len(want)} bytes): "
                    f"{vp8_parse.diagnose(got, want)}")


# twelve images, eight widths in macroblocks: the plan test's nine geometries and three
# sizes that are no multiple of 16 (edge replication by the image's own w, h); the
# qualities put both sides of the chroma error-diffusion switch (98 / 99) and the flat
# frames' qualities (10, 25) into one launch
SIZES = GEOMETRIES + [(7, 5), (17, 31), (100, 70)]
QUALS = [80, 1, 10, 25, 50, 98, 99, 100, 80, 99, 98, 25]
PATS = ["S", "N", "flat_in_noise", "diag45", "S", "N", "diag45", "flat_in_noise", "S", "N", "flat_in_noise", "diag45"]


def _image(k):
    w, h = SIZES[k]
    return vp8_content.geometry_image(PATS[k], w, h)


@pytest.fixture(scope="module")
def mixed_set(oracle):
    """The images, their qualities and libwebp's files (computed once, never changed)."""
    imgs = [_image(k) for k in range(len(SIZES))]
    want = [oracle.webp_encode_rgb(oracle.to_rgb8(img), float(q)) for img, q in zip(imgs, QUALS)]
    return imgs, QUALS, want


def test_one_mixed_call(ik, mixed_set):
    imgs, qs, want = mixed_set
    c0 = counters(ik)
    got = encode_items(ik, imgs, qs)
    c1 = counters(ik)
    for k, (g, w) in enumerate(zip(got, want)):
        check(g, w, f"image {k}: {SIZES[k][0]}x{SIZES[k][1]} {PATS[k]} q{qs[k]}")
    assert (c1[0] - c0[0], c1[1] - c0[1], c1[3] - c0[3]) == (0, len(imgs), 1)


@pytest.mark.parametrize("order", ["reversed", "shuffled"])
def test_order_independence(ik, mixed_set, order):
    imgs, qs, want = mixed_set
    n = len(imgs)
    perm = list(range(n))[::-1] if order == "reversed" else [int(v) for v in np.random.RandomState(5).permutation(n)]
    got = encode_items(ik, [imgs[p] for p in perm], [qs[p] for p in perm])
    for j, p in enumerate(perm):
        check(got[j], want[p], f"position {j} = image {p}")


def test_delegation_to_the_uniform_call(ik, oracle):
    imgs = [ikutil.synth(100, 70, 3, seed=40 + s, pattern="SN"[s & 1]) for s in range(5)]
    uniform = encode_exact(ik, imgs, 80)
    c0 = counters(ik)
    got = encode_items(ik, imgs, [80] * 5)
    c1 = counters(ik)
    assert got == uniform
    assert (c1[0] - c0[0], c1[1] - c0[1], c1[3] - c0[3]) == (5, 0, 0), "one geometry and quality: the uniform call"
    qs = [80, 80, 50, 80, 80]
    got = encode_items(ik, imgs, qs)
    c2 = counters(ik)
    assert (c2[0] - c1[0], c2[1] - c1[1], c2[3] - c1[3]) == (0, 5, 1), "one quality differs: the mixed call"
    for k, (img, q) in enumerate(zip(imgs, qs)):
        check(got[k], oracle.webp_encode_rgb(img, float(q)), f"image {k} q{q}")


def test_gathered_planes(ik, oracle):
    # one geometry and quality, planes 1024, 1280, 1024 and 1792 bytes apart: the mixed
    # call gathers them a common stride apart and hands them to the uniform call
    imgs = [ikutil.synth(33, 20, 3, seed=60 + s, pattern="SN"[s & 1]) for s in range(5)]
    c0 = counters(ik)
    got = encode_items(ik, imgs, [80] * 5, gaps=[0, 256, 0, 768])
    c1 = counters(ik)
    for k, img in enumerate(imgs):
        check(got[k], oracle.webp_encode_rgb(img, 80.0), f"gathered image {k}")
    assert (c1[0] - c0[0], c1[1] - c0[1], c1[3] - c0[3]) == (5, 0, 0), "the uniform call, no mixed call"


def test_calls_share_one_work_area(ik, oracle):
    # the uniform call, the mixed call and ik_vp8_analyze_device in turn on one thread: one
    # scratch slot, one pair of pinned slots, one schedule cache and one host driver
    from test_gpu_vp8_analysis import analyze, check as check_analysis
    uni = [ikutil.synth(33, 20, 3, seed=70 + s, pattern="SNS"[s]) for s in range(3)]
    uwant = [oracle.webp_encode_rgb(img, 80.0) for img in uni]
    # 176x160: 110 MBs, over 96, so two epochs (bounds 0, 96, 110)
    mixed = [uni[0], ikutil.synth(20, 33, 3, seed=73, pattern="N"), ikutil.synth(176, 160, 3, seed=74, pattern="S")]
    mq = [80, 99, 25]

    def uniform_call(what):
        got = encode_exact(ik, uni, 80)
        for k, (g, w) in enumerate(zip(got, uwant)):
            check(g, w, f"{what}, image {k}")
        return got

    first = uniform_call("first uniform call")
    c0 = counters(ik)
    for k, g in enumerate(encode_items(ik, mixed, mq)):
        check(g, oracle.webp_encode_rgb(mixed[k], float(mq[k])), f"mixed call, image {k}")
    c1 = counters(ik)
    assert (c1[1] - c0[1], c1[3] - c0[3]) == (3, 1), "three sizes: one mixed call"
    second = uniform_call("uniform call after the mixed one (cached schedule)")
    for k, a in enumerate(analyze(ik, uni, 80.0)):
        check_analysis(a, vp8_parse.parse(uwant[k]), f"analysis between the calls, image {k}")
    third = uniform_call("uniform call after the analysis")
    assert first == second == third


def test_work_area_growth(ik, oracle, mixed_set):
    # one thread's calls: small, the twelve images (the work area and pinned buffers grow), small again
    imgs, qs, want = mixed_set
    small = [ikutil.synth(33, 20, 3, seed=3, pattern="S"), ikutil.synth(20, 33, 3, seed=4, pattern="N")]
    sq = [80, 99]
    swant = [oracle.webp_encode_rgb(i, float(q)) for i, q in zip(small, sq)]
    for k, (g, w) in enumerate(zip(encode_items(ik, small, sq), swant)):
        check(g, w, f"first small call, image {k}")
    for k, (g, w) in enumerate(zip(encode_items(ik, imgs, qs), want)):
        check(g, w, f"large call, image {k}")
    for k, (g, w) in enumerate(zip(encode_items(ik, small, sq), swant)):
        check(g, w, f"second small call, image {k}")


def test_one_item(ik, oracle):
    img = ikutil.synth(17, 31, 4, seed=9, pattern="N")
    c0 = counters(ik)
    got = encode_items(ik, [img], [50])[0]
    c1 = counters(ik)
    check(got, oracle.webp_encode_rgb(oracle.to_rgb8(img), 50.0), "n = 1")
    assert (c1[0] - c0[0], c1[1] - c0[1]) == (1, 0)  # one geometry: the uniform call


@pytest.mark.parametrize("bad", ["w0", "w16384", "null"])
def test_a_bad_item_is_refused(ik, bad):
    imgs = [ikutil.synth(16, 16, 3, seed=1), ikutil.synth(32, 16, 3, seed=2)]
    dy, addr = _device_planes(ik, imgs)
    items = (_lib.WebpExactItem * 2)()
    items[0] = _lib.WebpExactItem(addr[0], 16, 16, 80)
    items[1] = {"w0": _lib.WebpExactItem(addr[1], 0, 16, 80), "w16384": _lib.WebpExactItem(addr[1], 16384, 16, 80),
                "null": _lib.WebpExactItem(None, 32, 16, 80)}[bad]
    outs = (ctypes.c_void_p * 2)(0x1234, 0x5678)
    lens = (ctypes.c_size_t * 2)(7, 9)
    c0 = counters(ik)
    try:
        rc = ik.ik_webp_encode_exact_items(items, 2, ctypes.cast(outs, ctypes.c_void_p), ctypes.cast(lens, ctypes.c_void_p))
    finally:
        ik.ik_dev_free(dy)
    assert rc == IK_ERR_INVALID
    assert list(outs) == [0x1234, 0x5678] and list(lens) == [7, 9], "outs untouched"
    assert counters(ik) == c0, "nothing was coded"


def test_the_batch_path(ik, oracle):
    # 24 WebP requests at q80 from three small PNGs, each to its own size: no same-geometry
    # group the uniform call takes, so with the switch at gpu all of them form one mixed
    # call.  The encoder is set to EXACT, under which the batch path's minimum is met by
    # two requests (AUTO's is 32, like the uniform groups').
    from PIL import Image
    from imagekit import FilterType, ImageFormat, transform_batch
    srcs = [ikutil.synth(320, 240, 4, seed=0, pattern="S"), ikutil.synth(320, 240, 3, seed=1, pattern="N"),
            ikutil.synth(240, 320, 4, seed=2, pattern="S")]
    pngs = []
    for s in srcs:
        b = io.BytesIO()
        Image.fromarray(s, "RGBA" if s.shape[2] == 4 else "RGB").save(b, format="PNG")
        pngs.append(b.getvalue())
    rng = np.random.RandomState(24)
    n = 24
    sizes = [(int(rng.randint(17, 200)), int(rng.randint(17, 200))) for _ in range(n)]
    datas = [pngs[k % 3] for k in range(n)]
    fmts = [ImageFormat.webp] * n
    qs = [80] * n
    want = [oracle.transform(srcs[k % 3], sizes[k][0], sizes[k][1], ikutil.TRIANGLE, ImageFormat.webp.value, 80)[0]
            for k in range(n)]
    # requests of one source geometry and one output size form a group the uniform call
    # takes (under EXACT from two on); every other request goes mixed
    groups = {}
    for k in range(n):
        sh = srcs[k % 3].shape
        key = (sh, oracle.resize_image_dims(sh[1], sh[0], *sizes[k]))
        groups[key] = groups.get(key, 0) + 1
    n_mixed = sum(c for c in groups.values() if c == 1)
    assert n_mixed >= 16, "the draw leaves most requests alone in their geometry"
    encoder = ik.ik_get_webp_encoder()
    try:
        assert ik.ik_set_webp_encoder(2) == 0
        assert ik.ik_set_webp_mixed(MIXED_GPU) == 0
        assert ik.ik_get_webp_mixed() == MIXED_GPU
        c0 = counters(ik)
        gpu = transform_batch(datas, sizes, fmts, qs, FilterType.Triangle)
        c1 = counters(ik)
        assert ik.ik_set_webp_mixed(MIXED_HOST) == 0
        host = transform_batch(datas, sizes, fmts, qs, FilterType.Triangle)
        c2 = counters(ik)
    finally:
        ik.ik_set_webp_mixed(-1)
        ik.ik_set_webp_encoder(encoder)
    assert (c1[1] - c0[1], c1[3] - c0[3]) == (n_mixed, 1), "switch at gpu: the lone requests in one mixed call"
    assert c1[0] - c0[0] == n - n_mixed and c1[2] == c0[2], "the groups through the uniform call, none on the host"
    assert c2[1] == c1[1] and c2[3] == c1[3], "switch at host: no mixed call"
    assert gpu == host
    for k in range(n):
        check(gpu[k], want[k], f"request {k}: {sizes[k]} of source {k % 3}")
