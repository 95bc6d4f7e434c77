"""A plain reference for the JPEG entropy coder (TEST INFRASTRUCTURE ONLY).

Baseline Huffman coding of quantised coefficients into the stuffed scan bytes
that encode_image's JPEG branch writes between the SOS header and the EOI:
one bit string per image, no parallel structure.  Written from the standard's
Annex K tables (K.3-K.6) and the rules of image 0.25.8's JpegEncoder that
ik_jpeg_enc.hip states:

- 4:4:4 MCUs of Y, Cb, Cr; DC is predicted per component from the previous MCU;
- a zero run of 16 or more before a value is written as ZRL (0xF0) codes;
- EOB (0x00) is written only when zigzag position 63 is zero;
- a 0xFF byte is followed by 0x00;
- the pad is seven one-bits, and the bits left over after the last whole byte
  are dropped.

tests/test_oracle_jpeg.py pins it against the C oracle (oracle/jpeg_enc.c) on a
machine without a GPU."""
from __future__ import annotations

from typing import NamedTuple

import numpy as np

# zigzag position -> natural (row-major) index, Figure A.6
ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5,
                   12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                   35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51,
                   58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63])

# Annex K.3.3: (BITS, HUFFVAL) of the four typical tables
DC_LUMA = ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], list(range(12)))
DC_CHROMA = ([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0], list(range(12)))
AC_LUMA = ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7D], [
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07,
    0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xA1, 0x08, 0x23, 0x42, 0xB1, 0xC1, 0x15, 0x52, 0xD1, 0xF0,
    0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0A, 0x16, 0x17, 0x18, 0x19, 0x1A, 0x25, 0x26, 0x27, 0x28,
    0x29, 0x2A, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3A, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49,
    0x4A, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5A, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69,
    0x6A, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7A, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89,
    0x8A, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9A, 0xA2, 0xA3, 0xA4, 0xA5, 0xA6, 0xA7,
    0xA8, 0xA9, 0xAA, 0xB2, 0xB3, 0xB4, 0xB5, 0xB6, 0xB7, 0xB8, 0xB9, 0xBA, 0xC2, 0xC3, 0xC4, 0xC5,
    0xC6, 0xC7, 0xC8, 0xC9, 0xCA, 0xD2, 0xD3, 0xD4, 0xD5, 0xD6, 0xD7, 0xD8, 0xD9, 0xDA, 0xE1, 0xE2,
    0xE3, 0xE4, 0xE5, 0xE6, 0xE7, 0xE8, 0xE9, 0xEA, 0xF1, 0xF2, 0xF3, 0xF4, 0xF5, 0xF6, 0xF7, 0xF8,
    0xF9, 0xFA])
AC_CHROMA = ([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77], [
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71,
    0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42, 0x91, 0xA1, 0xB1, 0xC1, 0x09, 0x23, 0x33, 0x52, 0xF0,
    0x15, 0x62, 0x72, 0xD1, 0x0A, 0x16, 0x24, 0x34, 0xE1, 0x25, 0xF1, 0x17, 0x18, 0x19, 0x1A, 0x26,
    0x27, 0x28, 0x29, 0x2A, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3A, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48,
    0x49, 0x4A, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5A, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68,
    0x69, 0x6A, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7A, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87,
    0x88, 0x89, 0x8A, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9A, 0xA2, 0xA3, 0xA4, 0xA5,
    0xA6, 0xA7, 0xA8, 0xA9, 0xAA, 0xB2, 0xB3, 0xB4, 0xB5, 0xB6, 0xB7, 0xB8, 0xB9, 0xBA, 0xC2, 0xC3,
    0xC4, 0xC5, 0xC6, 0xC7, 0xC8, 0xC9, 0xCA, 0xD2, 0xD3, 0xD4, 0xD5, 0xD6, 0xD7, 0xD8, 0xD9, 0xDA,
    0xE2, 0xE3, 0xE4, 0xE5, 0xE6, 0xE7, 0xE8, 0xE9, 0xEA, 0xF2, 0xF3, 0xF4, 0xF5, 0xF6, 0xF7, 0xF8,
    0xF9, 0xFA])


def huffman_codes(bits, vals) -> dict:
    """Annex C.2: symbol -> (code, length), codes counted up within a length and
    doubled between lengths."""
    assert sum(bits) == len(vals)
    out, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            out[vals[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return out


_DC = (huffman_codes(*DC_LUMA), huffman_codes(*DC_CHROMA))
_AC = (huffman_codes(*AC_LUMA), huffman_codes(*AC_CHROMA))


def code_of(table: str, component: int, symbol: int):
    """(code, length) of a symbol: table "dc" or "ac", component 0 (Y) or 1, 2 (chroma)."""
    return (_DC if table == "dc" else _AC)[1 if component else 0][symbol]


class Coded(NamedTuple):
    data: bytes       # the stuffed scan bytes (what lies between the SOS header and the EOI)
    total_bits: int   # coded bits before the pad
    nbytes: int       # bytes before stuffing: (total_bits + 7) // 8
    ff: tuple         # offsets of every 0xFF among those nbytes unstuffed bytes


def _amplitude(v: int):
    """F.1.2.1: category (bit count of |v|) and the amplitude bits (v, or v - 1 in
    that many bits for a negative v)."""
    n = abs(v).bit_length()
    return n, (v if v >= 0 else v - 1) & ((1 << n) - 1)


def code(coef) -> Coded:
    """coef: [nmcu][3][64] natural-order quantised coefficients (any integer type)."""
    zz = np.asarray(coef).astype(np.int64).reshape(-1, 3, 64)[:, :, ZIGZAG].tolist()
    parts = []
    pred = [0, 0, 0]
    for mcu in zz:
        for c in range(3):
            blk = mcu[c]
            dc, ac = _DC[1 if c else 0], _AC[1 if c else 0]
            n, amp = _amplitude(blk[0] - pred[c])
            pred[c] = blk[0]
            if n > 11:
                raise ValueError(f"DC difference of category {n}: no baseline code")
            acc, nb = dc[n]
            acc, nb = (acc << n) | amp, nb + n
            run = 0
            for k in range(1, 64):
                v = blk[k]
                if v == 0:
                    run += 1
                    continue
                while run > 15:
                    zc, zl = ac[0xF0]
                    acc, nb = (acc << zl) | zc, nb + zl
                    run -= 16
                n, amp = _amplitude(v)
                if n > 10:
                    raise ValueError(f"AC coefficient of category {n}: no baseline code")
                sc, sl = ac[(run << 4) | n]
                acc, nb = (((acc << sl) | sc) << n) | amp, nb + sl + n
                run = 0
            if blk[63] == 0:
                ec, el = ac[0x00]
                acc, nb = (acc << el) | ec, nb + el
            parts.append(format(acc, "0%db" % nb))
    bits = "".join(parts)
    total_bits = len(bits)
    nbytes = (total_bits + 7) // 8
    bits = (bits + "1111111")[:nbytes * 8]
    raw = int(bits, 2).to_bytes(nbytes, "big") if nbytes else b""
    ff = tuple(int(i) for i in np.flatnonzero(np.frombuffer(raw, np.uint8) == 0xFF))
    return Coded(raw.replace(b"\xff", b"\xff\x00"), total_bits, nbytes, ff)


def jpeg_segments(jpeg: bytes):
    """Walk a baseline file's marker segments: ([(marker, payload)] up to and
    including SOS, the scan bytes between the SOS header and the final EOI)."""
    assert jpeg[:2] == b"\xff\xd8" and jpeg[-2:] == b"\xff\xd9"
    segs, p = [], 2
    while True:
        assert jpeg[p] == 0xFF
        marker = jpeg[p + 1]
        n = int.from_bytes(jpeg[p + 2:p + 4], "big")
        segs.append((marker, jpeg[p + 4:p + 2 + n]))
        p += 2 + n
        if marker == 0xDA:
            return segs, jpeg[p:-2]
