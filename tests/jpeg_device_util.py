"""Files and helpers the JPEG-in-device-memory tests share (TEST INFRASTRUCTURE ONLY):
tests/test_jpeg_walk_model.py (CPU) and tests/test_gpu_jpeg_device.py (GPU).

ref_walk is a second statement of the marker walk (csrc/ik_jpeg_walk.h), written from
the walk's stated rules and the host parser's, so the library's answer is compared
with something that shares no code with it."""
import ctypes
import functools
import io

import numpy as np
from PIL import Image

import ikutil
import jpeg_writer as jw

SLOT = 4096
IN_PLACE, COPY_BACK, MALFORMED = 0, 1, 2
R_NONE, R_NOT_BASELINE, R_SMALL, R_NO_SOS, R_LARGE, R_COMPONENTS, R_GARBAGE, R_LENGTH, R_NO_SOI = range(9)
KEPT = {0xDB, 0xC4, 0xDD, 0xE0, 0xEE, 0xDA}
SOFS = set(range(0xC0, 0xD0)) - {0xC4, 0xC8, 0xCC}


class WalkInfo(ctypes.Structure):
    _fields_ = [("verdict", ctypes.c_int), ("reason", ctypes.c_int), ("sof_marker", ctypes.c_int),
                ("skeleton_len", ctypes.c_uint32), ("entropy_offset", ctypes.c_uint64),
                ("eoi_offset", ctypes.c_uint64)]


def walk(lib, data: bytes):
    """ik_jpeg_walk_host: (skeleton bytes, WalkInfo)."""
    skel = (ctypes.c_uint8 * SLOT)()
    info = WalkInfo()
    buf = bytes(data)
    assert lib.ik_jpeg_walk_host(buf, len(buf), skel, SLOT, ctypes.byref(info)) == 0
    return bytes(skel[:info.skeleton_len]), info


def ref_walk(d: bytes):
    """(verdict, reason, skeleton, entropy offset, eoi offset, sof) by the rules."""
    n = len(d)
    if d[:2] != b"\xff\xd8":
        return MALFORMED, R_NO_SOI, b"", 0, n, 0
    skel, p, why, sof, ncomp, ent = bytearray(b"\xff\xd8"), 2, 0, 0, None, 0
    while True:
        if p < n and d[p] != 0xFF:
            why = why or R_GARBAGE
            break
        while p < n and d[p] == 0xFF:
            p += 1
        if p >= n or d[p] == 0xD9:
            why = why or R_NO_SOS
            break
        m = d[p]
        p += 1
        if m == 0xD8 or 0xD0 <= m <= 0xD7 or m == 0x01:
            continue
        ln = int.from_bytes(d[p:p + 2], "big") if p + 2 <= n else 0
        if ln < 2 or p + ln > n:
            return MALFORMED, R_LENGTH, bytes(skel), 0, n, sof
        if m in SOFS:
            if sof or m not in (0xC0, 0xC1) or ln < 8 or d[p + 2] != 8:
                why = why or R_NOT_BASELINE
            if not sof:
                sof = m
                ncomp = d[p + 7] if ln >= 8 else None
        if m in SOFS or m in KEPT:
            if len(skel) + 2 + ln > SLOT:
                return COPY_BACK, R_LARGE, bytes(skel), 0, n, sof
            skel += b"\xff" + bytes([m]) + d[p:p + ln]
        if m == 0xDA:
            ent = p + ln
            if ncomp is None:
                why = why or R_NOT_BASELINE
            elif ln < 3 or d[p + 2] != ncomp:
                why = why or R_COMPONENTS
            break
        p += ln
    eoi = n
    if ent:
        q = d.rfind(b"\xff\xd9", max(ent, n - 4096))
        if q >= 0:
            eoi = q
        if not why and eoi - ent < 4096:
            why = R_SMALL
    return (COPY_BACK if why else IN_PLACE), why, bytes(skel), ent, eoi, sof


# ---- files ----------------------------------------------------------------------
def _noise(w=203, h=141, seed=5):
    return ikutil.synth(w, h, 3, seed=seed, pattern="N")


@functools.lru_cache(maxsize=None)
def pillow(kind: str) -> bytes:
    """Pillow files: 203x141 noise (far above 4 KiB of scan)."""
    buf = io.BytesIO()
    rgb = Image.fromarray(_noise())
    if kind == "420_opt":
        rgb.save(buf, "JPEG", quality=90, subsampling=2, optimize=True)
    elif kind == "444":
        rgb.save(buf, "JPEG", quality=90, subsampling=0)
    elif kind == "gray":
        rgb.convert("L").save(buf, "JPEG", quality=90)
    elif kind == "420_dri":
        rgb.save(buf, "JPEG", quality=90, subsampling=2, restart_marker_blocks=7)
    elif kind == "progressive":
        rgb.save(buf, "JPEG", quality=90, subsampling=2, progressive=True)
    else:
        raise KeyError(kind)
    return buf.getvalue()


PAYLOAD = bytes((i * 7 + 3) % 251 + 1 for i in range(60000)).replace(b"\xff", b"\x01")


@functools.lru_cache(maxsize=None)
def special(kind: str) -> jw.JpegFile:
    planes = jw.ycbcr(_noise(seed=9))
    if kind == "big_appn":      # 2 x 60 KB of APP1 / APP2 before the scan (written after the tables)
        return jw.encode(planes, jw.S420, extra=((0xE1, b"Exif\0\0" + PAYLOAD), (0xE2, b"ICC_PROFILE\0" + PAYLOAD)))
    if kind == "eoi_in_appn":   # FF D9 inside an APPn payload before SOS
        return jw.encode(planes, jw.S420, extra=((0xE3, b"x\xff\xd9y" * 9),))
    if kind == "sos_subset":    # the first (only) SOS names one component of three
        return jw.encode(planes, jw.S444, scans=(jw.Scan((0,)),))
    raise KeyError(kind)


def big_appn_first() -> bytes:
    """The big-APPn file with the two payloads moved in front of the tables."""
    f = special("big_appn").data
    a = f.index(b"\xff\xe1")
    b = f.index(b"\xff\xda", a + 2 * (len(PAYLOAD) + 12))
    app = f[a:b]
    first = f.index(b"\xff\xdb")
    return f[:first] + app + f[first:a] + f[b:]


def no_eoi() -> bytes:
    f = jw.build("420_optimal").data
    assert f.endswith(b"\xff\xd9")
    return f[:-2]


def stray_marker() -> bytes:
    """A baseline file with one byte in mid-scan overwritten by FF C4."""
    f = jw.build("420_optimal")
    mid = f.data.index(f.scan_bytes[0]) + len(f.scan_bytes[0]) // 2
    return f.data[:mid] + b"\xff\xc4" + f.data[mid + 2:]


def scan_twice() -> bytes:
    """A baseline file whose one full scan is sent twice: every component is in the
    first SOS, so the walk passes it, and the second SOS surfaces as a stray marker."""
    f = jw.build("420_optimal")
    ent = f.data.index(f.scan_bytes[0])
    sos = f.data.rindex(b"\xff\xda", 0, ent)
    end = ent + len(f.scan_bytes[0])
    return f.data[:end] + f.data[sos:end] + f.data[end:]


def cut_mid_scan() -> bytes:
    f = jw.build("420_optimal")
    return f.data[:f.data.index(f.scan_bytes[0]) + len(f.scan_bytes[0]) // 2]


def length_overrun() -> bytes:
    """The DHT segment's length runs past the file's end."""
    f = bytearray(jw.build("420_optimal").data)
    k = f.index(b"\xff\xc4")
    f[k + 2:k + 4] = b"\xff\xf0"
    return bytes(f[:40000])  # (0xfff0 bytes from the DHT on: more than are left)


def cut_in_header() -> bytes:
    f = jw.build("420_optimal").data
    return f[:f.index(b"\xff\xc4") + 12]  # inside the first DHT's code-length counts


def no_soi() -> bytes:
    return b"\x00\x00" + jw.build("420_optimal").data[2:]
