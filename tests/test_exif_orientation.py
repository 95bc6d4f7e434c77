"""ik_exif_orientation (csrc/ik_exif.h; host only, no GPU): the value Pillow wrote into
JPEG APP1, PNG eXIf and WebP EXIF, hand-built TIFF payloads in hand-built containers, and
every prefix of a valid file.  (tests/c/exif_prefixes.cpp walks the same prefixes under
AddressSanitizer and UBSan as a stand-alone program.)"""
import itertools

import pytest

import exif_util as xu
from imagekit import Orientation, exif_orientation

FORMATS = ("JPEG", "PNG", "WEBP")


@pytest.mark.parametrize("fmt", FORMATS)
def test_pillow_written_value(fmt):
    for o in range(1, 9):
        assert exif_orientation(xu.pillow_file(fmt, o)) == o
    assert exif_orientation(xu.pillow_file(fmt, None)) == 1


def test_other_formats_and_junk():
    assert exif_orientation(b"") == 1
    assert exif_orientation(b"GIF89a" + b"\0" * 64) == 1
    assert exif_orientation(b"BM" + xu.tiff([xu.entry(xu.ORIENTATION, xu.SHORT, 1, 6, True)])) == 1
    assert exif_orientation(xu.tiff([xu.entry(xu.ORIENTATION, xu.SHORT, 1, 6, True)])) == 1  # a bare TIFF: not ours
    assert int(Orientation.auto) == -1 and int(Orientation.stored) == 0 and int(Orientation.rotate90) == 6


def payloads():
    """(name, payload, expected)"""
    out = []
    for le, prefix in itertools.product((True, False), (False, True)):
        tag = ("II" if le else "MM") + ("-prefixed" if prefix else "")
        o = xu.entry(xu.ORIENTATION, xu.SHORT, 1, 6, le)
        rest = xu.other(le)
        out.append((tag + "-first", xu.tiff([o] + rest, le, prefix), 6))
        out.append((tag + "-last", xu.tiff(rest + [o], le, prefix), 6))
        out.append((tag + "-absent", xu.tiff(rest, le, prefix), 1))
        out.append((tag + "-ifd-at-20", xu.tiff(rest[:1] + [o], le, prefix, ifd_offset=20), 6))
        for v in range(1, 9):
            out.append((tag + "-value-%d" % v, xu.tiff([xu.entry(xu.ORIENTATION, xu.SHORT, 1, v, le)], le, prefix), v))
        out.append((tag + "-type-long", xu.tiff([xu.entry(xu.ORIENTATION, xu.LONG, 1, 6, le)], le, prefix), 1))
        out.append((tag + "-count-2", xu.tiff([xu.entry(xu.ORIENTATION, xu.SHORT, 2, [6, 6], le)], le, prefix), 1))
        out.append((tag + "-value-0", xu.tiff([xu.entry(xu.ORIENTATION, xu.SHORT, 1, 0, le)], le, prefix), 1))
        out.append((tag + "-value-9", xu.tiff([xu.entry(xu.ORIENTATION, xu.SHORT, 1, 9, le)], le, prefix), 1))
        out.append((tag + "-ifd-offset-past", xu.tiff([o], le, prefix, ifd_offset=4096), 1))
        out.append((tag + "-ifd-offset-huge", xu.tiff([o], le, prefix, ifd_offset=0xFFFFFFF0), 1))
        # the orientation would be entry 2 of a count that runs past the payload
        out.append((tag + "-count-past", xu.tiff(rest[:1] + [o], le, prefix, count=200), 1))
        out.append((tag + "-bad-magic", xu.tiff([o], le, prefix).replace(b"\x2a", b"\x2b", 1), 1))
    return out


PAYLOADS = payloads()


@pytest.mark.parametrize("wrap", sorted(xu.WRAPPERS))
def test_hand_built_payloads_in_hand_built_containers(wrap):
    for name, payload, want in PAYLOADS:
        assert exif_orientation(xu.WRAPPERS[wrap](payload)) == want, (wrap, name)


def test_first_exif_wins_and_scan_ends_the_search():
    six = xu.tiff([xu.entry(xu.ORIENTATION, xu.SHORT, 1, 6, True)])
    j = xu.jpeg_wrap(six)
    # an APP1 that is not EXIF (XMP) before it is stepped over
    xmp = b"\xff\xe1" + (2 + 29 + 3).to_bytes(2, "big") + b"http://ns.adobe.com/xap/1.0/\0abc"
    assert exif_orientation(j[:2] + xmp + j[2:]) == 6
    # an APP1 after the first SOS is not looked at
    plain = xu.pillow_file("JPEG", None)
    sos = plain.index(b"\xff\xda")
    app1 = j[j.index(b"\xff\xe1"):][:4 + 6 + len(six)]
    assert exif_orientation(plain[:sos] + app1 + plain[sos:]) == 6
    eoi = len(plain) - 2
    assert exif_orientation(plain[:eoi] + app1 + plain[eoi:]) == 1
    # PNG: eXIf after IEND is not looked at
    p = xu.pillow_file("PNG", None)
    assert exif_orientation(p + xu._png_chunk(b"eXIf", six)) == 1
    # WebP: a plain VP8L RIFF (no VP8X) carries none
    assert exif_orientation(xu.pillow_file("WEBP", None)) == 1


@pytest.mark.parametrize("wrap", ["jpeg-app1-after-app0", "png-exif-after-idat", "webp-exif-after-odd-chunk"])
def test_every_prefix_is_safe(wrap):
    b = xu.WRAPPERS[wrap](xu.tiff(xu.other(False) + [xu.entry(xu.ORIENTATION, xu.SHORT, 1, 7, False)], le=False))
    assert exif_orientation(b) == 7
    seen = set()
    for k in range(len(b) + 1):
        v = exif_orientation(b[:k])
        assert 1 <= v <= 8
        seen.add(v)
    assert seen == {1, 7}  # nothing but "none yet" and the value
