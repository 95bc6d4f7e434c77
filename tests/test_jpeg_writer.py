"""CPU: the JPEG writer of the layout tests (tests/jpeg_writer.py) and its matrix.

The GPU layout tests (tests/test_gpu_jpeg_layouts.py) decode files Pillow cannot
write: samplings 4:4:0, 4:1:1, 4:1:0, 3x1, unequal chroma planes, luma below the
maximum factors; several scans; Huffman tables that are not Annex K's; 16-bit
quantisation tables; marker texture.  Here, without a GPU, every file of that
matrix must open in Pillow (libjpeg-turbo) and decode to the same pixels, bit for
bit, in the oracle's libjpeg mode -- the bar tests/test_oracle_jpeg.py holds for
Pillow-written files -- so that a GPU mismatch is the kernels' and not the
fixture's or the oracle's.  The interleaved files of 4 KiB and up also go through
the host model of the self-synchronising decoder (ik_jpeg_model.cpp), with
tests/test_jpeg_model.py's assertions and one more: its coefficients, block by
block, are the ones the writer coded, which a transposed block grid or an
off-by-one at ten blocks per MCU would break."""
import ctypes
import io

import numpy as np
import pytest
from PIL import Image

import jpeg_writer as jw
import oracle_jpeg_huff as jh
from test_jpeg_model import model  # noqa: F401  (the model's binding)

LIBJPEG, ZUNE = 0, 1
NAMES = [c.name for c in jw.CASES]
# one interleaved baseline scan of 4 KiB and up: what the self-synchronising decoder takes
JSYNC = [c.name for c in jw.CASES if c.where == "gpu" and c.kw.get("sof", jw.SOF0) != jw.SOF2]


def pillow_pixels(data: bytes) -> np.ndarray:
    im = Image.open(io.BytesIO(data))
    return np.asarray(im if im.mode in ("RGB", "L") else im.convert("RGB"))


@pytest.mark.parametrize("name", NAMES)
def test_file_opens_in_pillow_and_the_oracle_equals_it(oracle, name):
    c, f = jw.BY_NAME[name], jw.build(name)
    pil = pillow_pixels(f.data)
    ch = 1 if c.content == "gray" else 3
    assert pil.reshape(c.h, c.w, ch).shape == (c.h, c.w, ch)
    np.testing.assert_array_equal(oracle.jpeg_decode(f.data, LIBJPEG), pil.reshape(c.h, c.w, ch))
    assert oracle.jpeg_decode(f.data, ZUNE).shape == (c.h, c.w, ch)


def test_the_matrix_reaches_what_it_claims():
    """The files are what their names say: where the GPU tests expect the
    self-synchronising decoder the scan has 4 KiB, every layout of the issue is
    there at three sizes, tables and markers are the unusual ones."""
    for name in JSYNC:
        f = jw.build(name)
        assert len(f.scan_bytes) == 1 and len(f.scan_bytes[0]) >= 4096, name
    for c in jw.CASES:
        if c.where == "host" and c.kw.get("sof", jw.SOF0) != jw.SOF2 and "scans" not in c.kw:
            assert len(jw.build(c.name).scan_bytes[0]) < 4096, c.name
    for tag in ("440", "411", "410", "311", "221", "low", "gray22"):
        c, f = jw.BY_NAME[tag + "_tiny"], jw.build(tag + "_tiny")
        assert (c.w, c.h) == (f.mcu[0] + 1, f.mcu[1] + 1)
        # a restart interval of 5 MCUs divides no MCU row and leaves a short last interval
        s = c.kw["sampling"]
        single = len(s) == 1
        mw, mh = (8, 8) if single else f.mcu
        mcux, mcuy = -(-jw.BIG[0] // mw), -(-jw.BIG[1] // mh)
        assert mcux % 5 and (mcux * mcuy) % 5
        assert jw.build(tag + "_big_dri5").data.count(b"\xff\xdd\x00\x04\x00\x05") == 1
    assert sum(h * v for h, v in jw.S410) == 10  # the most blocks per MCU a scan may have
    # 16-bit quantisation entries above 255
    segs, _ = jh.jpeg_segments(jw.build("pq1_small").data)
    dqt = [p for m, p in segs if m == 0xDB]
    assert len(dqt) == 2 and all(p[0] >> 4 == 1 and len(p) == 129 for p in dqt)
    assert max(int.from_bytes(dqt[0][1 + 2 * i:3 + 2 * i], "big") for i in range(64)) > 255
    # several tables per segment
    segs, _ = jh.jpeg_segments(jw.build("merged_small").data)
    assert [m for m, _ in segs].count(0xC4) == 1 and [m for m, _ in segs].count(0xDB) == 1
    # RSTn wraps: more than 8 intervals
    for name in ("rstwrap_small", "rstwrap_big"):
        scan = jw.build(name).scan_bytes[0]
        assert sum(scan.count(bytes([0xFF, 0xD0 + k])) for k in range(8)) > 8
    assert jw.build("fill_small").data[2:7] == b"\xff\xff\xff\xff\xe0"
    assert jw.build("trailer_big").data.endswith(b"\xff\xd9" + jw.GARBAGE)
    assert b"\xff\xc1" in jw.build("sof1_small").data and b"JFIF" not in jw.build("adobe0_small").data


@pytest.mark.parametrize("name", ["420_optimal", "440_long", "440_prog_dcapprox_dri3"])
def test_huffman_tables_are_valid_and_unusual(name):
    segs, _ = jh.jpeg_segments(jw.build(name).data)
    dht = {p[0]: (list(p[1:17]), list(p[17:])) for m, p in segs if m == 0xC4}
    std = {0x00: jh.DC_LUMA, 0x10: jh.AC_LUMA, 0x01: jh.DC_CHROMA, 0x11: jh.AC_CHROMA}
    assert {0x00, 0x01, 0x02, 0x10, 0x11, 0x12} <= set(dht)  # Cb and Cr have tables of their own
    for key, (bits, vals) in dht.items():
        assert std.get(key) != (bits, vals)
        assert len(set(vals)) == len(vals) == sum(bits)
        kraft = sum(n * 2 ** (16 - l) for l, n in enumerate(bits, 1))
        assert kraft < 1 << 16  # a prefix code with a code point to spare: no code is all ones
        if "long" in name:
            assert bits[15] == min(2, len(vals)) and bits[14] == min(2, max(0, len(vals) - 2))


def test_optimal_table_is_a_length_limited_huffman_code():
    # counts 1, 2, 4, ... would give codes of up to 22 bits: K.3 cuts them to 16, rarer symbols no shorter
    bits, vals = jw.optimal_table({s: 1 << s for s in range(22)})
    assert sum(bits) == 22 and sorted(vals) == list(range(22))
    assert sum(n * 2 ** (16 - l) for l, n in enumerate(bits, 1)) < 1 << 16
    codes = jh.huffman_codes(bits, vals)
    assert codes[0][1] == 16 and codes[21][1] == 1
    assert all(codes[a][1] >= codes[b][1] for a, b in zip(range(21), range(1, 22)))
    # two equally likely symbols: codes 0 and 10 (the all-ones code point stays free)
    bits, vals = jw.optimal_table({5: 7, 9: 7})
    assert (bits[:2], sorted(vals)) == ([1, 1], [5, 9])


@pytest.mark.parametrize("geom", [(2048, 512), (1024, 1024), (512, 0)])
@pytest.mark.parametrize("name", JSYNC)
def test_model_decodes_the_layout(model, name, geom):  # noqa: F811
    f = jw.build(name)
    st = (ctypes.c_longlong * 9)()
    out = np.zeros(f.coef.shape, np.int16)
    rc = model.ikm_jsync_decode(f.data, len(f.data), geom[0], geom[1], out.ctypes.data, out.size, st)
    st = list(st)
    assert rc == 0 and st[5] == 1, f"rc {rc}, stats {st}"
    assert st[6] >= 1 and st[0] >= st[6]  # at least a lane per interval
    np.testing.assert_array_equal(out, f.coef)
