"""GPU: the exact WebP coder (k_vp8_analyze, k_vp8_kmeans, k_vp8x_setup, k_vp8x_run, the
schedule and bitstream of ik_vp8x_host.cpp) on chosen content, strips and epoch edges --
what ikutil.synth's patterns S and N, at the sizes of tests/test_gpu_vp8x.py and
tests/test_gpu_vp8_analysis.py, never ask of it (reference src/transform.rs:129-137 ->
webp 0.3.1 -> libwebp WebPEncodeRGB).

Inputs: tests/vp8_content.py -- flat, striped, diagonal, saturated and one-pixel-checker
frames, flat macroblocks beside noise (IsFlatSource16 and the D/SD doubling of
PickBestIntra16, the three flatness penalties, every intra-4 direction in numbers, levels
above 67), frames one macroblock wide or high, and frames of 96, 97, 193, 194 and 776
macroblocks, which end on the edges of libwebp's probability-refresh epochs.
tests/test_vp8x_inputs.py proves on the CPU that the inputs reach those branches;
tests/test_vp8_modes.py holds the CPU model to libwebp on the same inputs, so a
difference here is the kernels' or the schedule's own.

Bar: the file is byte-identical to WebPEncodeRGB at q 1 ... 100 (98 and 99: the chroma
error-diffusion switch; 10 and 25: where the flat doubling decides the flat frames' bytes), alone and in a mixed batch; the analysis stage alone equals what
libwebp wrote into its segment header and map.  No tolerance anywhere.  A mismatch is
reported as the first macroblock whose decisions differ (vp8_parse.diagnose)."""
import pytest

import ikutil
import vp8_content
import vp8_parse
from test_gpu_vp8_analysis import analyze, check
from test_gpu_vp8x import encode_exact
from vp8_parse import diagnose

pytestmark = pytest.mark.gpu


def _same(got, want, where):
    assert got == want, f"{where}: {diagnose(got, want)}"


@pytest.mark.parametrize("q", vp8_content.CONTENT_QUALITIES)
@pytest.mark.parametrize("wh", vp8_content.CONTENT_SIZES, ids=lambda wh: f"{wh[0]}x{wh[1]}")
@pytest.mark.parametrize("name", vp8_content.PATTERN_NAMES)
def test_content(ik, oracle, name, wh, q):
    img = vp8_content.pattern(name, *wh)
    _same(encode_exact(ik, [img], q)[0], oracle.webp_encode_rgb(img, float(q)), f"{name} {wh[0]}x{wh[1]} q{q}")


@pytest.mark.parametrize("q", [80, 100])
@pytest.mark.parametrize("name", ["S", "N", "flat_in_noise", "diag45"])
@pytest.mark.parametrize("wh", vp8_content.GEOMETRIES, ids=lambda wh: f"{wh[0]}x{wh[1]}")
def test_geometry(ik, oracle, wh, name, q):
    img = vp8_content.geometry_image(name, *wh)
    _same(encode_exact(ik, [img], q)[0], oracle.webp_encode_rgb(img, float(q)), f"{wh[0]}x{wh[1]} {name} q{q}")


# the analysis stage alone: flat frames are the point (a one-bin alpha histogram through
# k_vp8_kmeans and SimplifySegments)
@pytest.mark.parametrize("q", [10.0, 80.0, 95.0])
@pytest.mark.parametrize("wh", vp8_content.CONTENT_SIZES, ids=lambda wh: f"{wh[0]}x{wh[1]}")
@pytest.mark.parametrize("name", vp8_content.PATTERN_NAMES)
def test_analysis_on_content(ik, oracle, name, wh, q):
    img = vp8_content.pattern(name, *wh)
    r = vp8_parse.parse(oracle.webp_encode_rgb(img, q))
    check(analyze(ik, [img], q)[0], r, f"{name} {wh[0]}x{wh[1]} q{q}")


@pytest.mark.parametrize("q", [10.0, 80.0, 95.0])
@pytest.mark.parametrize("name", ["S", "flat_in_noise", "flat255"])
@pytest.mark.parametrize("wh", vp8_content.STRIPS, ids=lambda wh: f"{wh[0]}x{wh[1]}")
def test_analysis_on_strips(ik, oracle, wh, name, q):
    img = vp8_content.geometry_image(name, *wh)
    r = vp8_parse.parse(oracle.webp_encode_rgb(img, q))
    check(analyze(ik, [img], q)[0], r, f"{wh[0]}x{wh[1]} {name} q{q}")


@pytest.mark.parametrize("q", [80, 99])
def test_mixed_batch(ik, oracle, q):
    # six frames of 100x70 whose macroblocks take very different times (all-i16-DC beside
    # all-intra-4): the ticket order crosses images at every diagonal
    w, h = 100, 70
    names = ["flat0", "N", "diag135", "primaries", "flat_in_noise", "S"]
    imgs = [vp8_content.geometry_image(name, w, h) for name in names]
    for name, got, img in zip(names, encode_exact(ik, imgs, q), imgs):
        _same(got, oracle.webp_encode_rgb(img, float(q)), f"batch image {name} q{q}")


def test_schedule_cache(ik, oracle):
    # exact_schedule is cached per thread on (w, h, n): one thread's calls with the same
    # macroblock count (96, then 97) but other diagonals, and a changing batch size
    for w, h, n in [(192, 128, 1), (128, 192, 1), (1536, 16, 1), (192, 128, 2), (192, 128, 1), (16, 1552, 1),
                    (1552, 16, 1)]:
        imgs = [ikutil.synth(w, h, 3, seed=w + 2 * h + i, pattern="S") for i in range(n)]
        for i, (got, img) in enumerate(zip(encode_exact(ik, imgs, 80), imgs)):
            _same(got, oracle.webp_encode_rgb(img, 80.0), f"{w}x{h} n={n} image {i}")
