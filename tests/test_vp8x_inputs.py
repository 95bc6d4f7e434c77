"""CPU: a census of what libwebp itself decides on the exact coder's chosen inputs
(tests/vp8_content.py), read from its own bytes (oracle.webp_encode_rgb through
tests/vp8_parse.py) -- proof that the content cases of tests/test_gpu_vp8x_content.py
(every pattern x {64x48, 100x70} x q {1, 10, 25, 50, 98, 99, 100}) reach what they are chosen for:
every intra-4, i16 and chroma mode in numbers, frames that end with 1, 2, 3 and 4 segments,
flat macroblocks (256 equal luma samples: IsFlatSource16 and the D/SD doubling chain of
PickBestIntra16) beside intra-4 ones, and levels above 67 (MAX_VARIABLE_LEVEL, where both
rate loops clamp their table index) in every coefficient type at q100.  The geometries are
held to the epoch structure they are named for.  An edit of the patterns that stops
testing one of these fails here, not silently.

The counts below are caps from below, not measurements: what the set gave when it was
chosen is far above each (run with -s to see the figures).

The `level > 2047` clamp (MAX_LEVEL in QuantizeBlock) is not reached, and no 8-bit picture
can reach it: source and prediction are bytes, so a residual is at most 255 in size, a 4x4
block's DC at most 8 * 255 = 2040, the WHT's outputs at most 16 * 2040 / 2 = 16320, and the
smallest i16-DC quantiser step is 8 -- a level of at most 2040; the other three types'
coefficients are at most 2040 too, with steps of at least 4.  libwebp's RGB import narrows it
further (luma 16 ... 235): the largest level seen here is 1752 = 8 * 219, the i16-DC of
`checker16`'s black-beside-white macroblocks at q99 and q100; the census asserts that figure's
bin (68 ... 2046) and that the 2047 bin is empty.  The clamp stays pinned by the CPU model
alone (oracle/vp8_modes.c quantize_block against libwebp's bytes)."""
import numpy as np
import pytest

import ikutil
import oracle_vp8
import vp8_content
import vp8_parse
from test_vp8_analysis import check_against_bitstream
from test_vp8_modes import restated_webp

QUALITIES = vp8_content.CONTENT_QUALITIES
I4_NAMES, I16_NAMES = vp8_parse.I4_NAMES, vp8_parse.I16_NAMES


def flat_macroblocks(y):
    """Per macroblock (mb_h, mb_w): 256 equal luma samples, the frame's edge replicated
    as libwebp's import does."""
    h, w = y.shape
    mb_w, mb_h = vp8_content.mb_dims(w, h)
    yp = np.pad(y, ((0, mb_h * 16 - h), (0, mb_w * 16 - w)), mode="edge")
    mbs = yp.reshape(mb_h, 16, mb_w, 16).transpose(0, 2, 1, 3).reshape(mb_h, mb_w, 256)
    return (mbs == mbs[:, :, :1]).all(-1)


@pytest.fixture(scope="module")
def census():
    orc = ikutil.Oracle()
    c = {"i4": np.zeros(10, np.int64), "i16": np.zeros(4, np.int64), "uv": np.zeros(4, np.int64),
         "segments": np.zeros(5, np.int64), "flat": 0, "flat_beside_i4": 0, "frames": 0,
         "levels": np.zeros((4, 4), np.int64), "levels_q100": np.zeros((4, 4), np.int64), "largest": (0, "")}
    for w, h in vp8_content.CONTENT_SIZES:
        mb_w, mb_h = vp8_content.mb_dims(w, h)
        for name, rgb in vp8_content.patterns(w, h).items():
            yuv = orc.libwebp_import_yuv(rgb)
            flat = flat_macroblocks(yuv[0])
            for q in QUALITIES:
                where = f"{name} {w}x{h} q{q}"
                want = orc.webp_encode_rgb(rgb, float(q))
                r = vp8_parse.parse(want)
                assert (r["width"], r["height"]) == (w, h) and not r["overrun"], where
                i4 = r["is_i4"].astype(bool)
                sub = r["bmodes"].reshape(mb_h, 4, mb_w, 4).transpose(0, 2, 1, 3)
                c["i4"] += np.bincount(sub[i4].reshape(-1), minlength=10)
                c["i16"] += np.bincount(r["ymode"][~i4], minlength=4)
                c["uv"] += np.bincount(r["uvmode"].reshape(-1), minlength=4)
                # the number of segments the frame ends with is not in the bytes as such
                # (the filter levels there are raised after coding): the restated analysis
                # gives it, held to the bytes' segment header, map and quantisers here
                a = oracle_vp8.analyze(*yuv, quality=float(q))
                check_against_bitstream(a, r, where)
                c["segments"][a["num_segments"]] += 1
                c["flat"] += int(flat.sum())
                c["flat_beside_i4"] += int(flat.sum()) if i4.any() else 0
                # the levels come from the restated coder's token walk, on a file equal to libwebp's
                lv = np.zeros((4, 4), np.uint32)
                assert restated_webp(orc, *yuv, float(q), levels=lv) == want, where
                for key in ("levels", "levels_q100") if q == 100 else ("levels",):
                    c[key][:, :3] += lv[:, :3]
                    c[key][:, 3] = np.maximum(c[key][:, 3], lv[:, 3])
                if lv[:, 3].max() > c["largest"][0]:
                    c["largest"] = (int(lv[:, 3].max()), where)
                c["frames"] += 1
    print(f"\ncensus over {c['frames']} frames (patterns x {vp8_content.CONTENT_SIZES} x q {QUALITIES}):")
    print("  intra-4 sub-blocks:", dict(zip(I4_NAMES, c["i4"].tolist())))
    print("  i16 macroblocks:   ", dict(zip(I16_NAMES, c["i16"].tolist())))
    print("  chroma modes:      ", dict(zip(I16_NAMES, c["uv"].tolist())))
    print("  frames ending with 1/2/3/4 segments:", c["segments"][1:].tolist())
    print(f"  flat macroblocks: {c['flat']}, of them {c['flat_beside_i4']} in frames that also hold intra-4")
    for key in ("levels", "levels_q100"):
        print(f"  {key} per type (i16-AC, i16-DC, chroma, i4) as [1..67, 68..2046, 2047, largest]:", c[key].tolist())
    print("  largest level:", c["largest"])
    return c


def test_every_mode_is_chosen(census):
    for name, n in zip(I4_NAMES, census["i4"]):
        assert n >= 20, f"intra-4 {name} chosen {n} times"
    for name, n in zip(I16_NAMES, census["i16"]):
        assert n >= 10, f"i16 {name} chosen {n} times"
    for name, n in zip(I16_NAMES, census["uv"]):
        assert n >= 10, f"chroma {name} chosen {n} times"


def test_every_segment_count_occurs(census):
    assert census["segments"][0] == 0 and (census["segments"][1:] >= 1).all(), census["segments"].tolist()


def test_flat_macroblocks_beside_intra4(census):
    assert census["flat"] >= 100 and census["flat_beside_i4"] >= 1, (census["flat"], census["flat_beside_i4"])


def test_levels_pass_the_variable_level_table(census):
    # every coefficient type codes a level above 67 at q100; none codes 2047 (see the docstring)
    lv = census["levels_q100"]
    for t, name in enumerate(("i16-AC", "i16-DC", "chroma", "i4")):
        assert lv[t, 1] >= 1 and lv[t, 3] > 67, f"{name}: {lv[t].tolist()}"
    assert (census["levels"][:, 2] == 0).all() and census["levels"][:, 3].max() <= 2040, census["levels"].tolist()


# geometry -> (number of epochs, macroblocks in the last one); M = max(mb_count / 8, 96)
EPOCHS = {(16, 64): (1, 4), (64, 16): (1, 4), (32, 33): (1, 6), (192, 128): (1, 96), (1536, 16): (1, 96),
          (16, 1552): (2, 1), (3088, 16): (2, 97), (1552, 32): (3, 1), (1552, 128): (8, 91)}
MB_DIMS = {(16, 64): (1, 4), (64, 16): (4, 1), (32, 33): (2, 3), (192, 128): (12, 8), (1536, 16): (96, 1),
           (16, 1552): (1, 97), (3088, 16): (193, 1), (1552, 32): (97, 2), (1552, 128): (97, 8)}


def test_geometries_sit_on_their_epoch_edges():
    assert sorted(vp8_content.GEOMETRIES) == sorted(EPOCHS)
    for w, h in vp8_content.GEOMETRIES:
        mb_w, mb_h = (w + 15) // 16, (h + 15) // 16
        assert (mb_w, mb_h) == MB_DIMS[(w, h)]
        n = mb_w * mb_h
        # libwebp's loop itself: `if (--cnt < 0) { refresh; cnt = max_count; }` before each MB
        m = cnt = max(n >> 3, 96)
        bounds = [0]
        for k in range(n):
            cnt -= 1
            if cnt < 0:
                bounds.append(k)
                cnt = m
        bounds.append(n)
        assert bounds == vp8_content.epoch_bounds(w, h), (w, h)
        assert (len(bounds) - 1, bounds[-1] - bounds[-2]) == EPOCHS[(w, h)], (w, h, bounds)
        assert bounds[1:-1] == [m * (e + 1) + e for e in range(len(bounds) - 2)], (w, h, bounds)
    assert max(776 >> 3, 96) == 97 and max(775 >> 3, 96) == 96  # 776: the first count with M = 97


def test_diagnose_names_the_difference():
    # the GPU tests' failure message (vp8_parse.diagnose) on libwebp files that are known to differ
    orc = ikutil.Oracle()
    a = vp8_content.pattern("flat_in_noise", 64, 48)
    fa = orc.webp_encode_rgb(a, 80.0)
    assert vp8_parse.diagnose(fa, fa) == "files equal"
    assert "segment header" in vp8_parse.diagnose(orc.webp_encode_rgb(a, 50.0), fa)  # other quantisers
    assert "differs at byte 40 (40 vs" in vp8_parse.diagnose(fa[:40], fa)  # a cut file: no exception
    # a flat frame at q100 (one segment), and the same with macroblock 26 (x 5, y 3) busy: coding is
    # causal, so no macroblock before it may be named
    f = vp8_content.pattern("flat0", 100, 70)
    g = f.copy()
    g[48:64, 80:96] = vp8_content.pattern("checker1", 16, 16)
    d = vp8_parse.diagnose(orc.webp_encode_rgb(g, 100.0), orc.webp_encode_rgb(f, 100.0))
    assert "first at macroblock" in d and int(d.split("first at macroblock ")[1].split()[0]) >= 26, d
