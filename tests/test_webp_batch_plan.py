"""CPU: ik_webp_batch_plan, the launch plan decode_webp_batch (ik_vp8d_host.cpp) lays a
batch of lossy WebP frames out by: which request is placed k-th (largest first), the
MB-row ticket each placed frame starts at, and where a byte cap cuts the batch into
sub-launches.  Host only -- no GPU needed."""
import ctypes

import numpy as np
import pytest

from imagekit import _lib


def plan(mb_w, mb_h, nbytes, cap):
    lib = _lib.load()
    n = len(mb_w)
    mw = (ctypes.c_uint32 * max(n, 1))(*mb_w)
    mh = (ctypes.c_uint32 * max(n, 1))(*mb_h)
    by = (ctypes.c_uint64 * max(n, 1))(*nbytes)
    order = (ctypes.c_uint32 * (n + 1))(*([0xFFFFFFFF] * (n + 1)))
    row_start = (ctypes.c_uint32 * (n + 1))(*([0xFFFFFFFF] * (n + 1)))
    lo = (ctypes.c_uint32 * (n + 1))(*([0xFFFFFFFF] * (n + 1)))
    launches = lib.ik_webp_batch_plan(mw, mh, by, n, cap, order, row_start, lo)
    return launches, list(order)[:n], list(row_start), list(lo)[:launches + 1]


def check(mb_w, mb_h, nbytes, cap):
    """The properties every plan has; returns (launches, order, row_start, launch_lo)."""
    n = len(mb_w)
    launches, order, row_start, lo = plan(mb_w, mb_h, nbytes, cap)
    assert sorted(order) == list(range(n))
    assert lo[0] == 0 and lo[-1] == n and all(a < b for a, b in zip(lo, lo[1:]))
    for a, b in zip(lo, lo[1:]):
        ks = order[a:b]
        rows = [mb_h[i] for i in ks]
        assert rows == sorted(rows, reverse=True)  # non-increasing in MB rows
        for p, q in zip(ks, ks[1:]):  # then in MBs, then by request
            if mb_h[p] == mb_h[q]:
                assert (mb_w[p], -p) >= (mb_w[q], -q)
        # the prefix sums of the placed frames' MB rows, from 0 in each sub-launch
        want = np.concatenate([[0], np.cumsum(rows)])
        assert row_start[a:b] == list(want[:-1])
        if b == n:
            assert row_start[n] == want[-1]
        # the cap: a sub-launch holds what fits, or one frame alone
        assert sum(nbytes[i] for i in ks) <= cap or len(ks) == 1
    # sub-launches are cut only where the next frame would not fit
    for a, b, c in zip(lo, lo[1:], lo[2:]):
        assert sum(nbytes[i] for i in order[a:b]) + nbytes[order[b]] > cap
    return launches, order, row_start, lo


def test_everything_in_one_launch():
    mb_w = [40, 4, 120, 64, 1, 40]
    mb_h = [30, 129, 68, 48, 13, 30]
    nbytes = [w * h * 1000 for w, h in zip(mb_w, mb_h)]
    launches, order, row_start, lo = check(mb_w, mb_h, nbytes, 1 << 40)
    assert launches == 1 and lo == [0, 6]
    assert order == [1, 2, 3, 0, 5, 4]  # by MB rows; the equal pair by request
    assert row_start == [0, 129, 197, 245, 275, 305, 318]


def test_equal_rows_go_by_macroblocks():
    launches, order, _, _ = check([10, 30, 20], [8, 8, 8], [1, 1, 1], 100)
    assert launches == 1 and order == [1, 2, 0]


def test_cap_splits_ten_equal_images_4_4_2():
    n = 10
    launches, order, row_start, lo = check([3] * n, [2] * n, [1000] * n, 4000)
    assert launches == 3 and lo == [0, 4, 8, 10]
    assert order == list(range(n))
    assert row_start == [0, 2, 4, 6, 0, 2, 4, 6, 0, 2, 4]


def test_an_image_above_the_cap_is_alone():
    mb_w = [4, 200, 4, 4]
    mb_h = [4, 150, 5, 3]
    nbytes = [100, 10_000, 100, 100]
    launches, order, row_start, lo = check(mb_w, mb_h, nbytes, 1000)
    assert launches == 2 and lo == [0, 1, 4]
    assert order == [1, 2, 0, 3]
    assert row_start == [0, 0, 5, 9, 12]


def test_an_image_above_the_cap_in_the_middle():
    # equal rows, so the big one is placed by its MBs ahead of the small ones; every
    # frame here is above or at the cap with its neighbour: one launch each
    launches, order, row_start, lo = check([1, 9, 1], [2, 2, 2], [600, 5000, 600], 1000)
    assert launches == 3 and order == [1, 0, 2] and lo == [0, 1, 2, 3]
    assert row_start == [0, 0, 0, 2]


def test_one_image():
    launches, order, row_start, lo = check([7], [5], [123], 1 << 30)
    assert (launches, order, row_start, lo) == (1, [0], [0, 5], [0, 1])
    launches, order, row_start, lo = check([7], [5], [123], 1)  # above the cap: still launched
    assert (launches, order, row_start, lo) == (1, [0], [0, 5], [0, 1])


def test_no_images():
    launches, order, row_start, lo = plan([], [], [], 1 << 20)
    assert launches == 0 and order == [] and lo == [0]


@pytest.mark.parametrize("seed", range(8))
def test_random_batches(seed):
    rng = np.random.default_rng(seed)
    n = int(rng.integers(1, 60))
    mb_w = [int(v) for v in rng.integers(1, 260, n)]
    mb_h = [int(v) for v in rng.integers(1, 40, n)]  # few distinct values: ties
    nbytes = [w * h * 640 + 4096 for w, h in zip(mb_w, mb_h)]
    cap = int(rng.choice([max(nbytes) // 2, max(nbytes), 3 * max(nbytes), sum(nbytes)]))
    launches, _, _, lo = check(mb_w, mb_h, nbytes, cap)
    assert launches == len(lo) - 1
