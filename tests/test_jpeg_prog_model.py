"""CPU: the GPU's entropy decoding of progressive JPEG without restart markers, run
by its CPU model (libik_jpegmodel.so ikm_jprog_decode: the same ik_jpeg_sync.h
code the ik_jsync.hip kernels use).

decode_image on a progressive JPEG (reference src/transform.rs:31 -> zune-jpeg
0.4.21) decodes every scan serially.  Of the four scan kinds three parallelise:
DC-first scans are baseline blocks without an AC part, AC-first scans
synchronise at every end of block (a unit is a block, or an EOBn symbol with all
the blocks its run covers), DC refinement is a bit per block.  The model decodes
a file serially by the host decoder's rules, and again with every Ah = 0 scan
through the lane scheme (warm-up, fix rounds, bases, decode pass) and the Ah > 0
scans by the serial rules.

Bar, per file and lane geometry: the two ways agree, and the lane way's
coefficients equal the serial decode's -- and, for tests/jpeg_writer.py's files,
the coefficients the writer coded.

What this file does not check: both ways decode AC refinement scans with the same
ac_refine_block, and tests/jpeg_writer.py writes none, so on the CPU that function
is compared only with itself.  Its independent check is on the GPU, where
tests/test_gpu_jpeg_prog_free.py compares the pixels of Pillow's files -- AC
refinement in each -- with libjpeg-turbo (Pillow) and the zune restatement."""
import ctypes

import numpy as np
import pytest

import jpeg_prog_util as pu
import jpeg_writer as jw
from test_jpeg_model import model  # noqa: F401  (the model's binding)

LANE_BITS = (64, 128, 1024)
WARM_BITS = (0, 1024)

FILES = {
    "noise_444": pu.noise_444,
    "s_420": pu.s_420,
    "gray": pu.gray,
    "flat_gray": pu.flat_gray,
    "optimised_420": pu.optimised_420,
    "440_prog_spectral_norst": lambda: jw.build("440_prog_spectral_norst").data,
}
for _s in ("411", "221"):
    for _k in ("spectral", "dc_approx"):
        FILES[f"{_s}_{_k}"] = (lambda s, k: lambda: pu.writer(s, k, (75, 53), "S").data)(_s, _k)


def _bind(model):
    f = model.ikm_jprog_decode
    f.restype = ctypes.c_int
    f.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t,
                  ctypes.POINTER(ctypes.c_longlong)]
    return f


def _run(model, data, lane_bits, warm_bits, nblocks=0):
    st = (ctypes.c_longlong * 11)()
    coef = np.zeros((nblocks, 64), np.int16)
    rc = _bind(model)(data, len(data), lane_bits, warm_bits, coef.ctypes.data if nblocks else None, coef.size, st)
    return rc, list(st), coef


def _nblocks(data):
    """Blocks of the coefficient image (every component padded to whole MCUs)."""
    p = data.find(b"\xff\xc2")
    h, w, nc = data[p + 5] << 8 | data[p + 6], data[p + 7] << 8 | data[p + 8], data[p + 9]
    hv = [(data[p + 11 + 3 * i] >> 4, data[p + 11 + 3 * i] & 15) for i in range(nc)]
    hm, vm = max(a for a, _ in hv), max(b for _, b in hv)
    return sum(-(-w // (8 * hm)) * a * -(-h // (8 * vm)) * b for a, b in hv)


@pytest.fixture(scope="module")
def serial(model):
    """Each file's serial decode, computed once."""
    cache = {}

    def get(name):
        if name not in cache:
            data = FILES[name]()
            rc, _, coef = _run(model, data, 0, 0, _nblocks(data))
            assert rc == 0
            cache[name] = coef
        return cache[name]
    return get


@pytest.mark.parametrize("warm_bits", WARM_BITS)
@pytest.mark.parametrize("lane_bits", LANE_BITS)
@pytest.mark.parametrize("name", list(FILES))
def test_lanes_equal_serial(model, serial, name, lane_bits, warm_bits):
    data = FILES[name]()
    want = serial(name)
    rc, st, coef = _run(model, data, lane_bits, warm_bits, len(want))
    assert rc == 0 and st[4] == 1, f"rc {rc}, stats {st}"
    np.testing.assert_array_equal(coef, want)
    assert st[6] >= 2 and st[0] >= st[6]  # at least a lane per first scan


@pytest.mark.parametrize("name", ["440_prog_spectral_norst", "411_dc_approx", "221_spectral"])
def test_serial_equals_the_writers_coefficients(serial, name):
    """The serial way against coefficients no decoder produced.  A one-component
    scan codes only the blocks that hold samples (T.81 A.2.2): the AC coefficients
    of a component's padding blocks are in no scan and stay zero."""
    w, h = 75, 53
    f = jw.build(name) if name.endswith("norst") else pu.writer(*name.split("_", 1), (w, h), "S")
    sampling = jw.S440 if name.startswith("440") else pu.WRITER_SAMPLINGS[name[:3]]
    hm, vm = max(a for a, _ in sampling), max(b for _, b in sampling)
    want, b0 = f.coef.copy(), 0
    for ch, cv in sampling:
        bw, bh = -(-w // (8 * hm)) * ch, -(-h // (8 * vm)) * cv
        sbw, sbh = -(-(-(-w * ch // hm)) // 8), -(-(-(-h * cv // vm)) // 8)
        blocks = want[b0:b0 + bw * bh].reshape(bh, bw, 64)
        blocks[sbh:, :, 1:] = 0
        blocks[:, sbw:, 1:] = 0
        b0 += bw * bh
    np.testing.assert_array_equal(serial(name), want)


def test_many_lanes_in_both_first_scan_kinds(model):
    _, st, _ = _run(model, pu.s_420(), 1024, 1024)
    assert st[7] >= 8 and st[8] >= 8, st


def test_cold_lanes_are_repaired(model):
    rc, st, _ = _run(model, pu.s_420(), 128, 0)
    assert rc == 0 and st[4] == 1 and st[1] > 0 and st[2] > 0, st


def test_flat_image_runs_span_many_lanes_worth_of_blocks(model):
    """512 x 512 flat: 4,096 blocks per AC-first scan in a few EOB runs -- fewer
    lanes than a sixty-fourth of the blocks they cover."""
    rc, st, _ = _run(model, pu.flat_gray(), 64, 0)
    assert rc == 0 and st[4] == 1
    assert st[10] >= 4000 and st[9] < st[10] / 64, st


def test_other_files_are_refused(model):
    import io
    from PIL import Image
    import ikutil
    b = io.BytesIO()
    Image.fromarray(ikutil.synth(320, 240, 3, seed=1)).save(b, format="JPEG", quality=85)
    for data in (b.getvalue(), pu.with_restart_rows(), jw.build("440_prog_spectral_dri3").data):
        assert _run(model, data, 1024, 1024)[0] == -1
