"""CPU: the Adam7 pass table of the GPU PNG decoder (ik_png_adam7_plan, csrc/ik_png_plan.h)
against the PNG spec's pass geometry restated in png_adam7_util.passes: the pass
count, every field of every non-empty pass, and the inflated length -- which is also
the length of what the test writer compresses."""
import ctypes

import numpy as np
import pytest

import png_adam7_util as A7

BITS = (1, 2, 4, 8, 16, 24, 32, 48, 64)
SIZES = [(w, h) for w in range(1, 21) for h in range(1, 21)] + [(4096, 4096), (1, 70000)]


@pytest.fixture(scope="module")
def lib():
    from imagekit import _lib
    return _lib.load()  # loads without a GPU


def plan(lib, w, h, bits):
    out = (ctypes.c_uint64 * 56)()
    tot = ctypes.c_uint64()
    n = lib.ik_png_adam7_plan(w, h, bits, out, ctypes.byref(tot))
    return [tuple(out[8 * q:8 * q + 8]) for q in range(n)], tot.value


@pytest.mark.parametrize("bits", BITS)
def test_plan_equals_the_spec(lib, bits):
    for w, h in SIZES:
        got, tot = plan(lib, w, h, bits)
        want, wtot = A7.passes(w, h, bits)
        assert got == want, (w, h, bits)
        assert tot == wtot, (w, h, bits)
        assert 1 <= len(got) <= 7
        assert sum(p[4] * p[5] for p in got) == w * h  # every pixel in exactly one pass


def test_null_outputs_are_allowed(lib):
    assert lib.ik_png_adam7_plan(9, 9, 8, None, None) == 7
    assert lib.ik_png_adam7_plan(1, 1, 8, None, None) == 1


@pytest.mark.parametrize("ctype,depth", [(0, 1), (0, 2), (0, 4), (0, 8), (0, 16), (3, 1), (3, 8), (4, 8), (4, 16),
                                         (2, 8), (2, 16), (6, 8), (6, 16)])
def test_raw_total_is_the_writers_length(lib, ctype, depth):
    spp = A7.SPP[ctype]
    for w, h in [(1, 1), (2, 2), (3, 3), (5, 1), (1, 5), (7, 5), (9, 9), (33, 17), (129, 33)]:
        s = np.zeros((h, w, spp), np.uint16)
        raw = b"".join(A7.raw_stream(s, depth))
        _, tot = plan(lib, w, h, spp * depth)
        assert len(raw) == tot, (w, h, ctype, depth)
