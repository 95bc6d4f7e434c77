"""CPU: the ticket table of the exact WebP coder's mixed call (ik_webp_exact_plan, no GPU).

One launch codes images of different sizes; its tickets are the images' own orders --
epochs at libwebp's probability refreshes, macroblocks by diagonal mb_x + 2 mb_y, then
the epoch's statistics fold -- merged step by step (a step: one diagonal that holds
macroblocks, or one fold).  The kernel takes tickets in order and a task polls for its
dependencies, so the table is right when every dependency of a ticket holds a smaller
ticket and each image keeps the order it has alone."""
import ctypes

import pytest

from imagekit import _lib
from vp8_content import epoch_bounds, mb_dims

FOLD = 1 << 63

# (w, h) in pixels: 1x1, 4x1, 1x4, 2x3 MBs; 12x8 = 96 MBs, one epoch; 97x1, a last epoch
# of one MB; 97x2, three epochs; 97x8; 20x15
GEOMETRIES = [(16, 16), (64, 16), (16, 64), (32, 33), (192, 128), (1552, 16), (1552, 32), (1552, 128), (320, 240)]
MBS = [(1, 1), (4, 1), (1, 4), (2, 3), (12, 8), (97, 1), (97, 2), (97, 8), (20, 15)]

BATCHES = ([[g] for g in GEOMETRIES] + [GEOMETRIES, GEOMETRIES[::-1], [GEOMETRIES[8]] * 5])
IDS = [f"{g[0][0]}x{g[0][1]}" for g in BATCHES[:9]] + ["all", "reversed", "five"]


def plan(sizes):
    lib = _lib.load()
    n = len(sizes)
    w = (ctypes.c_uint32 * n)(*[s[0] for s in sizes])
    h = (ctypes.c_uint32 * n)(*[s[1] for s in sizes])
    grid = ctypes.c_uint32(0)
    count = lib.ik_webp_exact_plan(w, h, n, None, 0, ctypes.byref(grid))
    assert count > 0, _lib.last_error()
    tasks = (ctypes.c_uint64 * count)()
    assert lib.ik_webp_exact_plan(w, h, n, tasks, count, None) == count
    return list(tasks), grid.value


def fields(t):
    return bool(t & FOLD), (t >> 48) & 0xff, (t >> 32) & 0xffff, t & 0xffffffff


def steps_of(w, h):
    """The step sizes of one geometry, restated: per epoch its non-empty diagonals, then 1
    for the fold."""
    mb_w, _ = mb_dims(w, h)
    b = epoch_bounds(w, h)
    out = []
    for e in range(len(b) - 1):
        diag = {}
        for k in range(b[e], b[e + 1]):
            d = k % mb_w + 2 * (k // mb_w)
            diag[d] = diag.get(d, 0) + 1
        out += [diag[d] for d in sorted(diag)] + [1]
    return out


def test_geometries_are_the_named_ones():
    assert [mb_dims(*g) for g in GEOMETRIES] == MBS
    assert len(epoch_bounds(192, 128)) == 2
    assert epoch_bounds(1552, 16)[-2:] == [96, 97]
    assert len(epoch_bounds(1552, 32)) == 4


@pytest.mark.parametrize("sizes", BATCHES, ids=IDS)
def test_every_task_once_and_after_its_dependencies(sizes):
    tasks, _ = plan(sizes)
    at_mb, at_fold = {}, {}
    for t, task in enumerate(tasks):
        fold, e, img, mb = fields(task)
        key = (img, e) if fold else (img, mb)
        book = at_fold if fold else at_mb
        assert key not in book, f"ticket {t}: {key} twice"
        book[key] = t
        assert img < len(sizes)
        if fold:
            assert mb == 0
    for img, (w, h) in enumerate(sizes):
        mb_w, mb_h = mb_dims(w, h)
        b = epoch_bounds(w, h)
        assert sorted(m for (i, m) in at_mb if i == img) == list(range(mb_w * mb_h))
        assert sorted(e for (i, e) in at_fold if i == img) == list(range(len(b) - 1))
        for e in range(len(b) - 1):
            f = at_fold[(img, e)]
            for k in range(b[e], b[e + 1]):
                assert fields(tasks[at_mb[(img, k)]])[1] == e, "the MB's ticket names its epoch"
                assert at_mb[(img, k)] < f, f"image {img}: fold {e} before its MB {k}"
            if e + 2 < len(b):
                assert all(f < at_mb[(img, k)] for k in range(b[e + 1], b[e + 2])), \
                    f"image {img}: an MB of epoch {e + 1} before fold {e}"
        for k in range(mb_w * mb_h):
            mx, my = k % mb_w, k // mb_w
            if mx:
                assert at_mb[(img, k - 1)] < at_mb[(img, k)], f"image {img} MB {k}: left neighbour later"
            if my:  # the top-right neighbour, or the top one in the last column
                nb = k - mb_w + (1 if mx < mb_w - 1 else 0)
                assert at_mb[(img, nb)] < at_mb[(img, k)], f"image {img} MB {k}: top(-right) neighbour later"


@pytest.mark.parametrize("sizes", BATCHES[9:], ids=IDS[9:])
def test_each_image_keeps_its_single_image_order(sizes):
    tasks, _ = plan(sizes)
    for img, size in enumerate(sizes):
        alone, _ = plan([size])
        mine = [t & ~(0xffff << 32) for t in tasks if fields(t)[2] == img]
        assert mine == alone, f"image {img} ({size[0]}x{size[1]})"


@pytest.mark.parametrize("sizes", BATCHES, ids=IDS)
def test_grid_is_the_widest_merged_step(sizes):
    tasks, grid = plan(sizes)
    per_image = [steps_of(w, h) for w, h in sizes]
    assert sum(map(sum, per_image)) == len(tasks)
    widest = max(sum(s[k] for s in per_image if k < len(s)) for k in range(max(map(len, per_image))))
    assert grid == min(widest, 2048, len(tasks))
    # and the table is those steps in order: step k of every image that still has one, by image
    at = 0
    for k in range(max(map(len, per_image))):
        for img, s in enumerate(per_image):
            if k < len(s):
                assert all(fields(t)[2] == img for t in tasks[at:at + s[k]]), f"step {k}, image {img}"
                at += s[k]


def test_epoch_field_fits_eight_bits_at_the_largest_frame():
    # 16383 x 16383: 1024 x 1024 MBs, M = nmb / 8, epochs at M, 2M+1, ...: the count of
    # bounds below nmb plus one -- by arithmetic, without building the table
    mb = (16383 + 15) // 16
    nmb = mb * mb
    m = max(nmb >> 3, 96)
    epochs = len(range(m, nmb, m + 1)) + 1
    assert epochs == 8 and epochs - 1 < 256
    # the most epochs any frame has: nmb / (M + 1) + 1 with M >= nmb / 8 - 1 is at most 9
    for n in (1, 96, 97, 98, 193, 194, 775, 776, 777, 8 * 97 + 8, 10 ** 4, nmb):
        mm = max(n >> 3, 96)
        assert len(range(mm, n, mm + 1)) + 1 <= 9


def test_bad_arguments_are_refused():
    lib = _lib.load()
    one = (ctypes.c_uint32 * 1)(16)
    big = (ctypes.c_uint32 * 1)(16384)
    zero = (ctypes.c_uint32 * 1)(0)
    assert lib.ik_webp_exact_plan(one, big, 1, None, 0, None) == -1
    assert lib.ik_webp_exact_plan(zero, one, 1, None, 0, None) == -1
    assert lib.ik_webp_exact_plan(one, one, 0, None, 0, None) == -1
    assert lib.ik_webp_exact_plan(one, one, 1, None, 0, None) == 2  # one MB and its fold
