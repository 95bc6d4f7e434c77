"""CPU: the oracle's restatement of the AVIF front end (oracle/avif_yuv.c: to_rgba8, then
ravif 0.11.20's 8-bit BT.601 full-range YCbCr 4:4:4 in f32), the checker of k_avif_yuv444
(tests/test_gpu_avif_front.py).

No copy of ravif exists here, so the restatement is cross-checked against the same formula
in float64 over every colour: the two may differ only where rounding is a near tie, those
sites are counted, and the count is pinned."""
import numpy as np
import pytest

# float64 sites within TIE_EPS of a half-integer, counted from the float64 formula alone
# (Y, U, V) out of 2^24 colours: the only places where the f32 oracle may differ, by 1
TIE_EPS = 1e-3
TIE_SITES = {"Y": 26871, "U": 32768, "V": 32768}


@pytest.fixture(scope="module")
def all_colours():
    """Every (r, g, b) once, as a 4096 x 4096 RGB image (pixel index = r<<16 | g<<8 | b)."""
    idx = np.arange(1 << 24, dtype=np.uint32)
    img = np.stack([idx >> 16, (idx >> 8) & 255, idx & 255], -1).astype(np.uint8).reshape(4096, 4096, 3)
    img.setflags(write=False)
    return img


@pytest.fixture(scope="module")
def all_colour_planes(oracle, all_colours):
    return {fma: oracle.avif_yuv444(all_colours, chroma_fma=fma) for fma in (True, False)}


def _f64_plane(img, name):
    r, g, b = (img[..., k].astype(np.float64) for k in range(3))
    y = 0.299 * r + 0.587 * g + 0.114 * b
    if name == "Y":
        return y
    if name == "U":
        return (b - y) * 0.5 / 0.886 + 128
    return (r - y) * 0.5 / 0.701 + 128


@pytest.mark.parametrize("k,name", [(0, "Y"), (1, "U"), (2, "V")])
def test_oracle_matches_float64_on_every_colour(all_colours, all_colour_planes, k, name):
    """Both modes of the oracle against float64, round half up and clip.  The f32 error of
    these expressions is below 2e-4 (a handful of roundings of at most 255 * 2^-24 each, times
    a chroma gain below 1), so a value may differ, by 1, only where the float64 value lies
    within 1e-3 of a half-integer; everywhere else it is equal.  The number of such sites is
    pinned so the exempt set cannot grow."""
    x = _f64_plane(all_colours, name)
    ref = np.clip(np.floor(x + 0.5), 0, 255).astype(np.uint8)
    tie = np.abs((x + 0.5) - np.round(x + 0.5)) < TIE_EPS
    del x
    assert int(tie.sum()) == TIE_SITES[name]
    for fma in (True, False):
        d = all_colour_planes[fma][k].astype(np.int16) - ref
        bad = (d != 0) & ~tie
        print(f"{name} chroma_fma={int(fma)}: {int((d != 0).sum())} values differ from float64, all at tie sites")
        assert not bad.any(), f"{name} chroma_fma={int(fma)}: differs from float64 away from a tie at colours " \
                              f"(r<<16|g<<8|b) {np.flatnonzero(bad)[:8].tolist()}"
        assert np.abs(d).max() <= 1


def test_fused_and_unfused_chroma_counts(all_colour_planes):
    """What the fused multiply-add changes, measured with the oracle itself (DESIGN.md quotes
    these): Y has no fused step, so it must not move; U and V move by 1 at a few thousand
    colours and nowhere by more."""
    f, n = all_colour_planes[True], all_colour_planes[False]
    counts = {name: int((f[k] != n[k]).sum()) for k, name in enumerate("YUV")}
    print("colours at which chroma_fma=1 and chroma_fma=0 differ:", counts)
    assert counts["Y"] == 0
    for k in (1, 2):
        assert 0 < counts["YUV"[k]] < 1 << 14
        assert np.abs(f[k].astype(np.int16) - n[k]).max() == 1
    np.testing.assert_array_equal(f[3], 255)
    np.testing.assert_array_equal(n[3], 255)
    assert f[4] == 0 and n[4] == 0


@pytest.mark.parametrize("fma", [True, False])
def test_gray_has_neutral_chroma(oracle, fma):
    """L and LA: r = g = b = l, so Y = l (the three weights sum to 1 within f32) and U = V = 128
    for each of the 256 levels, and alpha passes through."""
    l = np.arange(256, dtype=np.uint8).reshape(1, 256, 1)
    y, u, v, a, t = oracle.avif_yuv444(l, fma)
    np.testing.assert_array_equal(y[0], l[0, :, 0])
    np.testing.assert_array_equal(u, 128)
    np.testing.assert_array_equal(v, 128)
    np.testing.assert_array_equal(a, 255)
    assert t == 0
    alpha = (np.arange(256) * 7 % 256).astype(np.uint8)
    la = np.concatenate([l, alpha.reshape(1, 256, 1)], -1)
    y, u, v, a, t = oracle.avif_yuv444(la, fma)
    np.testing.assert_array_equal(y[0], l[0, :, 0])
    np.testing.assert_array_equal(u, 128)
    np.testing.assert_array_equal(v, 128)
    np.testing.assert_array_equal(a[0], alpha)
    assert t == 1


# colour -> (Y, U, V) by hand from Y = .299r + .587g + .114b, U = (b - Y) / 1.772 + 128,
# V = (r - Y) / 1.402 + 128, rounded; None marks the two exact ties of real arithmetic
# (yellow's U and cyan's V are 128 - 127.5 = 0.5), where f32 may land on either side
HAND = {
    (0, 0, 0): (0, 128, 128),
    (255, 255, 255): (255, 128, 128),
    (255, 0, 0): (76, 85, 255),      # Y 76.245  U 84.972   V 255.5 -> saturates
    (0, 255, 0): (150, 44, 21),      # Y 149.685 U 43.528   V 21.235
    (0, 0, 255): (29, 255, 107),     # Y 29.07   U 255.5 -> saturates, V 107.265
    (255, 255, 0): (226, None, 149),  # Y 225.93  U 0.5      V 148.735
    (0, 255, 255): (179, 171, None),  # Y 178.755 U 171.028  V 0.5
    (255, 0, 255): (105, 212, 235),  # Y 105.315 U 212.472  V 234.765
}


@pytest.mark.parametrize("fma", [True, False])
def test_primaries_and_secondaries_by_hand(oracle, fma):
    img = np.array(list(HAND), np.uint8).reshape(1, -1, 3)
    y, u, v, a, t = oracle.avif_yuv444(img, fma)
    for i, (rgb, want) in enumerate(HAND.items()):
        got = (int(y[0, i]), int(u[0, i]), int(v[0, i]))
        for g, w, plane in zip(got, want, "YUV"):
            if w is None:
                assert g in (0, 1), f"{rgb} {plane}: {g}, an exact tie at 0.5"
            else:
                assert g == w, f"{rgb} {plane}: {g}, by hand {w}"
    np.testing.assert_array_equal(a, 255)
    assert t == 0


@pytest.mark.parametrize("fma", [True, False])
@pytest.mark.parametrize("c", [1, 2, 3, 4])
def test_channel_counts_go_through_to_rgba8(oracle, c, fma):
    """C = 1..4 is to_rgba8 followed by the C = 4 path; the flag follows the alpha plane."""
    import ikutil
    img = ikutil.synth(61, 7, c, seed=10 + c, pattern="N", alpha="random")
    rgba = oracle.to_rgba8(img)
    if c == 1:
        np.testing.assert_array_equal(rgba, np.concatenate([img.repeat(3, 2), np.full_like(img, 255)], -1))
    got, want = oracle.avif_yuv444(img, fma), oracle.avif_yuv444(rgba, fma)
    for g, w in zip(got[:4], want[:4]):
        np.testing.assert_array_equal(g, w)
    np.testing.assert_array_equal(got[3], rgba[..., 3])
    assert got[4] == want[4] == int((rgba[..., 3] != 255).any())
    assert got[4] == (1 if c in (2, 4) else 0)


@pytest.mark.parametrize("c", [2, 4])
def test_flag_is_any_alpha_below_255(oracle, c):
    import ikutil
    img = ikutil.synth(9, 4, c, seed=c, pattern="N")
    assert oracle.avif_yuv444(img)[4] == 0
    for at in ((0, 0), (3, 8)):
        for alpha in (254, 0):
            one = img.copy()
            one[at[0], at[1], -1] = alpha
            assert oracle.avif_yuv444(one)[4] == 1
