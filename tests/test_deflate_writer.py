"""CPU: the token-level DEFLATE writer (deflate_writer.py) and the streams it writes
(deflate_streams.py) against the reference readers, before any decoder of ours sees them.

Every valid case: zlib.decompress gives the rows back, Pillow (libpng + zlib) opens
the PNG file to the source pixels, and the case's property holds on the stream as
deflate_writer.walk reads it (ds.valid asserts it while it makes the case; the count it
found is printed).  Every invalid case: zlib.decompress raises zlib.error and Pillow's
load() raises.  The writer's own parts -- canonical codes, the length helpers' Kraft
sums, the forced parse, the walker against zlib's own streams -- have unit tests."""
import io
import zlib

import numpy as np
import pytest
from PIL import Image

import deflate_streams as ds
import deflate_writer as dw


@pytest.mark.parametrize("name", ds.VALID)
def test_valid_stream(name):
    c = ds.valid(name)
    print(f"{name}: {c.found}")
    assert c.z[:2] == b"\x78\x01" and (c.z[0] >> 4) == 7 and not c.z[1] & 0x20
    assert zlib.decompress(c.z) == c.raw
    pil = np.asarray(Image.open(io.BytesIO(c.png)))
    np.testing.assert_array_equal(pil.reshape(c.img.shape), c.img)
    assert c.found  # (the property, counted on the walked stream)
    # the same stream in small IDAT chunks is the same image
    split = dw.png(c.img, c.z, idat=4093)
    assert split.count(b"IDAT") >= len(c.z) // 4093
    np.testing.assert_array_equal(np.asarray(Image.open(io.BytesIO(split))).reshape(c.img.shape), c.img)


@pytest.mark.parametrize("name", ds.INVALID)
def test_invalid_stream(name):
    b = ds.invalid(name)
    with pytest.raises(zlib.error):
        zlib.decompress(b.z)
    with pytest.raises(Exception):
        Image.open(io.BytesIO(b.png)).load()


def test_length_helpers_give_complete_codes():
    rng = np.random.default_rng(3)
    for n, depth in ((286, 15), (286, 10), (286, 9), (30, 15), (30, 5), (19, 7)):
        for used in (2, 3, n // 2, n):
            counts = [0] * n
            for s in rng.choice(n, used, replace=False):
                counts[s] = int(rng.integers(1, 1 << int(rng.integers(1, 16))))
            lens = dw.lengths_from_counts(counts, depth)
            assert dw.kraft(lens) == 1 << 15 and max(lens) <= depth
            assert all((lens[s] > 0) == (counts[s] > 0) for s in range(n))
    counts = [0] * 286
    for s in list(range(40)) + [256, 281, 282, 283, 284]:
        counts[s] = 5 if s > 256 else 100 + s
    lens = dw.lengths_from_counts(counts, 15, deep=4, dummies=range(100, 256))
    assert dw.kraft(lens) == 1 << 15 and all(lens[s] == 15 for s in (281, 282, 283, 284))
    assert all(lens[s] for s in range(40)) and lens[256]
    with pytest.raises(AssertionError):
        dw.check_kraft([2, 2, 2])          # incomplete
    with pytest.raises(AssertionError):
        dw.check_kraft([1, 1, 1])          # oversubscribed
    with pytest.raises(AssertionError):
        dw.check_kraft([0, 0], False)      # only a distance code may be empty
    dw.check_kraft([0, 1])                 # the one permitted incomplete shape
    dw.check_kraft([0], True)


def test_forced_parse_sends_only_true_repeats():
    raw = bytes(range(7)) * 3 + b"abcabcabcabcXabc" + bytes(300)
    for kw in (dict(distances=[7, 3, 1]), dict(min_distance=2), dict(distances=[1], only258=True),
               dict(distances=[3, 7], lengths=(4, 3))):
        toks = dw.tokenize(raw, **kw)
        assert dw.token_bytes(toks) == raw
        m = [t for t in toks if isinstance(t, tuple)]
        assert m
        if "distances" in kw:
            assert {d for _, d in m} <= set(kw["distances"])
        if kw.get("only258"):
            assert {n for n, _ in m} == {258}
        if "min_distance" in kw:
            assert min(d for _, d in m) >= 2
    assert (4, 1) not in dw.tokenize(b"aaab" + b"aaaa", distances=[1], lengths=(3,))


@pytest.mark.parametrize("level,strategy", [(6, zlib.Z_DEFAULT_STRATEGY), (1, zlib.Z_DEFAULT_STRATEGY),
                                            (6, zlib.Z_FIXED), (0, zlib.Z_DEFAULT_STRATEGY), (9, zlib.Z_RLE)])
def test_walker_reads_zlibs_streams(level, strategy):
    """walk() on zlib's own streams: its tokens reproduce the data, the bit costs add up to
    the block's extent, and re-writing the walked blocks gives a stream zlib reads back."""
    rng = np.random.default_rng(level)
    raw = bytes(rng.integers(0, 12, 30000, dtype=np.uint8)) + bytes(range(256)) * 20
    co = zlib.compressobj(level, zlib.DEFLATED, 15, 8, strategy)
    z = co.compress(raw[:20000]) + co.flush(zlib.Z_FULL_FLUSH) + co.compress(raw[20000:]) + co.flush()
    blocks = dw.walk(z)
    out, again = bytearray(), []
    for b in blocks:
        assert b["out"] == len(out)
        if b["type"] == 0:
            data = z[b["body"] >> 3:b["end"] >> 3]
            out += data
            again.append(dw.stored(data, final=bool(b["final"])))
            continue
        toks = [t[1] if t[0] == "lit" else (t[1], t[2]) for t in b["tokens"]]
        assert b["body"] + sum(t[2] if t[0] == "lit" else t[3] for t in b["tokens"]) + b["eob_bits"] == b["end"]
        out += dw.token_bytes(toks, bytes(out))
        again.append(dw.fixed(toks, final=bool(b["final"])) if b["type"] == 1 else
                     dw.dynamic(toks, ll=b["ll"], dl=b["dl"], final=bool(b["final"])))
    assert bytes(out) == raw
    assert zlib.decompress(dw.zlib_stream(again, raw)) == raw
    assert dw.deflate_blocks(z) == [(b["type"], b["hdr"], b["body"], b["end"]) for b in blocks]
