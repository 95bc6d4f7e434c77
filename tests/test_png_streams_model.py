"""CPU: the GPU PNG decoder's inflate algorithms (the wave decoder ikm_inflate_wave, the
lane decoder ikm_inflate_chunked; libik_pngmodel.so runs the code the kernels run) on
the DEFLATE streams zlib cannot write (deflate_streams.py: distances up to 32768,
48-bit steps back to back, blocks of slow codes, one distance code or none, the
header's extremes, stored-block edges, 600 empty blocks).

Bar: bytes identical to zlib.decompress for every valid stream at search chunks of
4096, 16384 and 65536 bytes; a non-zero return for every stream zlib rejects."""
import pytest

import deflate_streams as ds
from test_png_model import inflate as inflate_chunked
from test_png_model import model as chunked_model  # noqa: F401 (a fixture)
from test_png_wave_model import inflate as inflate_wave
from test_png_wave_model import model  # noqa: F401 (a fixture)

CHUNKS = [4096, 16384, 65536]


@pytest.mark.parametrize("chunk", CHUNKS)
@pytest.mark.parametrize("name", ds.VALID)
def test_wave_inflate_equals_zlib(model, name, chunk):  # noqa: F811
    c = ds.valid(name)
    rc, out, st = inflate_wave(model, c.z, len(c.raw), chunk)
    assert rc == 0, st
    assert out == c.raw
    if name == "empty_blocks":  # more blocks than a lane's piece table holds: the lane splits
        assert st["lanes"] > 1 and st["rounds"] > 1, st
    if name == "far_across_lanes" and chunk == ds.WAVE_CHUNK:
        assert st["lanes"] >= 2 and st["markers"] > 0, st


@pytest.mark.parametrize("chunk", CHUNKS)
@pytest.mark.parametrize("name", ds.VALID)
def test_chunked_inflate_equals_zlib(chunked_model, name, chunk):
    c = ds.valid(name)
    rc, out, st = inflate_chunked(chunked_model, c.z, len(c.raw), chunk)
    if name in ds.EXPECTED_FALLBACK:
        # (a coded block costs the lane decoder a 136-token table, an empty one 10 bits: its
        # token region overflows; the GPU path then hands the stream to the host decoder)
        assert rc == -2 and st[8] >= 1, st
        return
    assert rc == 0, st
    assert out == c.raw


@pytest.mark.parametrize("name", ds.INVALID)
def test_invalid_stream_is_rejected(model, chunked_model, name):  # noqa: F811
    b = ds.invalid(name)
    n = b.img.size + b.img.shape[0]
    for chunk in CHUNKS:
        rc, _, st = inflate_wave(model, b.z, n, chunk)
        assert rc != 0, ("wave", chunk, st)
        rc, _, st = inflate_chunked(chunked_model, b.z, n, chunk)
        assert rc != 0, ("chunked", chunk, st)
