"""A small JPEG writer (TEST INFRASTRUCTURE ONLY), written from ITU-T T.81.

Pillow's writer reaches three samplings, one interleaved scan, Annex K or
libjpeg's optimised tables, 8-bit quantisation tables and a JFIF header.  This
one emits valid streams of everything else the decoder is written for: any
sampling factors and component ids, SOF0 / SOF1 / SOF2, 16-bit quantisation
tables, Huffman tables built from the file's own statistics or deliberately
skewed towards 15- and 16-bit codes, scan scripts (one scan per component,
Y then Cb+Cr, spectral selection, DC successive approximation), restart
intervals of any length, fill bytes, stray segments, bytes after EOI, Adobe
APP14.  It is no good encoder and does not have to be: expected pixels always
come from decoders (Pillow's libjpeg-turbo, oracle/jpeg_dec.c), never from here.

encode() also returns the quantised coefficients in the decoder's block layout
(component after component, rows of MCU-padded blocks, natural order), which
pins the self-synchronising decoder's block-to-component bookkeeping.

CASES at the end is the matrix tests/test_jpeg_writer.py (CPU) and
tests/test_gpu_jpeg_layouts.py (GPU) share."""
from __future__ import annotations

import functools
import math
from typing import NamedTuple

import numpy as np

import ikutil
from oracle_jpeg_huff import AC_CHROMA, AC_LUMA, DC_CHROMA, DC_LUMA, ZIGZAG, huffman_codes

SOF0, SOF1, SOF2 = 0xC0, 0xC1, 0xC2

# the sampling layouts of the issue: (h, v) of Y, Cb, Cr
S444 = ((1, 1), (1, 1), (1, 1))
S420 = ((2, 2), (1, 1), (1, 1))
S422 = ((2, 1), (1, 1), (1, 1))
S440 = ((1, 2), (1, 1), (1, 1))
S411 = ((4, 1), (1, 1), (1, 1))
S410 = ((4, 2), (1, 1), (1, 1))
S311 = ((3, 1), (1, 1), (1, 1))
S221 = ((2, 2), (2, 1), (1, 1))
SLOW = ((1, 1), (2, 2), (2, 2))   # luma below the maximum factors
GRAY22 = ((2, 2),)                # one component whose factors must be ignored


class Scan(NamedTuple):
    comps: tuple      # indices into the frame's components
    Ss: int = 0
    Se: int = 63
    Ah: int = 0
    Al: int = 0


class JpegFile(NamedTuple):
    data: bytes
    coef: np.ndarray  # [block][64] int16, natural order, the decoder's block layout
    scan_bytes: tuple  # entropy-coded bytes of each scan (stuffed, with its RSTn markers)
    mcu: tuple        # MCU width and height in pixels


# ---- scan scripts -------------------------------------------------------------
def script_per_component(n=3):
    return tuple(Scan((i,)) for i in range(n))


def script_y_then_chroma():
    return (Scan((0,)), Scan((1, 2)))


def script_spectral(n=3):
    """Progressive by spectral selection: DC of all components, then two AC bands each."""
    return (Scan(tuple(range(n)), 0, 0),) + tuple(Scan((i,), a, b) for i in range(n) for a, b in ((1, 5), (6, 63)))


def script_dc_approx(n=3):
    """DC successive approximation (Al = 1 and its one-bit refinement), then the AC bands."""
    return ((Scan(tuple(range(n)), 0, 0, 0, 1), Scan(tuple(range(n)), 0, 0, 1, 0))
            + tuple(Scan((i,), 1, 63) for i in range(n)))


# ---- Huffman tables -----------------------------------------------------------
def optimal_table(freq: dict):
    """T.81 K.2 (figures K.1-K.4): (BITS, HUFFVAL) of a code limited to 16 bits for
    the symbols counted in freq, with one code point kept back so that no code is
    all ones."""
    f = [0] * 257
    for s, c in freq.items():
        f[s] = c
    f[256] = 1
    size, others = [0] * 257, [-1] * 257
    while True:
        v1, m = -1, None
        for i in range(257):
            if f[i] and (m is None or f[i] <= m):
                v1, m = i, f[i]
        v2, m = -1, None
        for i in range(257):
            if f[i] and i != v1 and (m is None or f[i] <= m):
                v2, m = i, f[i]
        if v2 < 0:
            break
        f[v1] += f[v2]
        f[v2] = 0
        size[v1] += 1
        while others[v1] >= 0:  # every symbol of both subtrees grows by one bit
            v1 = others[v1]
            size[v1] += 1
        others[v1] = v2  # chain the second subtree behind the first
        size[v2] += 1
        while others[v2] >= 0:
            v2 = others[v2]
            size[v2] += 1
    bits = [0] * 64
    for i in range(257):
        if size[i]:
            assert size[i] < 64
            bits[size[i]] += 1
    for i in range(63, 16, -1):  # figure K.3: Adjust_BITS
        while bits[i] > 0:
            j = i - 2
            while bits[j] == 0:
                j -= 1
            bits[i] -= 2
            bits[i - 1] += 1
            bits[j + 1] += 2
            bits[j] -= 1
    i = 16
    while bits[i] == 0:
        i -= 1
    bits[i] -= 1  # the reserved code point
    vals = sorted((s for s in range(256) if size[s]), key=lambda s: (size[s], s))
    return bits[1:17], vals


def long_table(freq: dict):
    """A valid table that is as bad as can be: the two most frequent symbols get
    16-bit codes, the next two 15-bit codes, every other symbol one common short
    length (Kraft sum below 1, so no code is all ones)."""
    syms = sorted(freq, key=lambda s: (-freq[s], s))
    l16, l15, rest = syms[:2], syms[2:4], sorted(syms[4:])
    bits = [0] * 16
    if rest:
        bits[max(1, math.ceil(math.log2(2 * len(rest)))) - 1] = len(rest)
    bits[14] += len(l15)
    bits[15] += len(l16)
    return bits, rest + l15 + l16


def _std_table(cls, tid):
    return ((DC_LUMA, DC_CHROMA), (AC_LUMA, AC_CHROMA))[cls][1 if tid else 0]


# ---- forward transform --------------------------------------------------------
_C = np.array([[(math.sqrt(0.5) if u == 0 else 1.0) / 2 * math.cos((2 * x + 1) * u * math.pi / 16) for x in range(8)]
               for u in range(8)])


def quant_table(step: int, limit: int) -> np.ndarray:
    """Natural-order table 1 + (u + v) * step, entries capped at limit."""
    u, v = np.mgrid[0:8, 0:8]
    return np.minimum(1 + (u + v) * step, limit).reshape(64).astype(np.int64)


def ycbcr(rgb: np.ndarray) -> np.ndarray:
    """JFIF's RGB -> YCbCr, in float64 (the planes encode() takes)."""
    r, g, b = (rgb[..., k].astype(np.float64) for k in range(3))
    return np.stack([0.299 * r + 0.587 * g + 0.114 * b,
                     128 - 0.168736 * r - 0.331264 * g + 0.5 * b,
                     128 + 0.5 * r - 0.418688 * g - 0.081312 * b], -1)


def _amplitude(v: int):
    n = abs(v).bit_length()
    return n, (v if v >= 0 else v - 1) & ((1 << n) - 1)


def encode(planes, sampling=S420, *, ids=None, sof=SOF0, qstep=2, pq=0, dqt_merged=False, huff="std",
           tables=None, dht_merged=False, scans=None, restart=0, fill=0, extra=(), trailer=b"", jfif=True,
           adobe=None) -> JpegFile:
    """planes: (H, W, ncomp) samples as stored (YCbCr, RGB for Adobe transform 0,
    gray, CMYK), any real type.  sampling: (h, v) per component.  ids: component
    ids (1, 2, 3, ... by default).  qstep: quantisation step growth (quant_table);
    pq 1 writes 16-bit entries (up to 65535), else they are capped at 255.
    huff: "std" | "optimal" | "long"; tables: Huffman table id per component
    (0, 1, 1, 0 by default; DC and AC alike).  scans: a scan script (one
    interleaved scan by default).  restart: DRI interval in MCUs.  fill: 0xFF
    fill bytes before every marker but SOI and RSTn.  extra: (marker, payload)
    segments written between the tables and the first SOS.  trailer: bytes after
    EOI.  adobe: None, or the APP14 transform."""
    planes = np.asarray(planes, np.float64)
    if planes.ndim == 2:
        planes = planes[..., None]
    H, W, nc = planes.shape
    assert nc == len(sampling) and nc in (1, 3, 4)
    hmax, vmax = max(h for h, _ in sampling), max(v for _, v in sampling)
    mcux, mcuy = -(-W // (8 * hmax)), -(-H // (8 * vmax))
    ids = tuple(ids) if ids else tuple(range(1, nc + 1))
    tables = tuple(tables) if tables else (0, 1, 1, 0)[:nc]
    progressive = sof == SOF2
    scans = tuple(scans) if scans else (Scan(tuple(range(nc))),)
    qts = [quant_table(qstep, 65535 if pq else 255), quant_table(2 * qstep, 65535 if pq else 255)]
    tq = (0, 1, 1, 0)[:nc]

    # planes -> quantised coefficients, zigzag order, [by][bx][64] per component
    zz, geom, nat, blk0 = [], [], [], 0
    for i, (h, v) in enumerate(sampling):
        assert hmax % h == 0 and vmax % v == 0, "fractional sampling ratios are not written"
        fx, fy = hmax // h, vmax // v
        dw, dh = -(-W * h // hmax), -(-H * v // vmax)
        p = np.pad(planes[..., i], ((0, dh * fy - H), (0, dw * fx - W)), mode="edge")
        p = p.reshape(dh, fy, dw, fx).mean(axis=(1, 3))
        bw, bh = mcux * h, mcuy * v
        p = np.pad(p, ((0, bh * 8 - dh), (0, bw * 8 - dw)), mode="edge") - 128.0
        blocks = p.reshape(bh, 8, bw, 8).transpose(0, 2, 1, 3)
        f = (_C @ blocks @ _C.T).reshape(bh, bw, 64)
        q = np.clip(np.rint(f / qts[tq[i]]), -1023, 1023).astype(np.int64)
        nat.append(q.reshape(-1, 64))
        zz.append(q[:, :, ZIGZAG].tolist())
        geom.append((h, v, bw, bh, -(-dw // 8), -(-dh // 8)))
        blk0 += bw * bh

    # scans -> tokens (class 0 DC / 1 AC / -1 raw bits, table, symbol, extra bit count, extra bits)
    def tokens(sc: Scan):
        if progressive:
            assert (sc.Ss == 0 and sc.Se == 0) or (sc.Ss > 0 and len(sc.comps) == 1 and sc.Ah == 0)
        else:
            assert (sc.Ss, sc.Se, sc.Ah, sc.Al) == (0, 63, 0, 0)
        if len(sc.comps) == 1:
            c = sc.comps[0]
            units = [[(c, by, bx)] for by in range(geom[c][5]) for bx in range(geom[c][4])]
        else:
            units = [[(c, my * geom[c][1] + y, mx * geom[c][0] + x)
                      for c in sc.comps for y in range(geom[c][1]) for x in range(geom[c][0])]
                     for my in range(mcuy) for mx in range(mcux)]
        intervals, cur, pred = [], [], {}
        for k, unit in enumerate(units):
            if restart and k and k % restart == 0:
                intervals.append(cur)
                cur, pred = [], {}
            for c, by, bx in unit:
                blk, t = zz[c][by][bx], tables[c]
                if sc.Ss == 0:
                    if sc.Ah:
                        cur.append((-1, 0, 0, 1, (blk[0] >> sc.Al) & 1))
                    else:
                        v = blk[0] >> sc.Al
                        n, a = _amplitude(v - pred.get(c, 0))
                        pred[c] = v
                        cur.append((0, t, n, n, a))
                if sc.Se == 0:
                    continue
                run = 0
                for j in range(max(sc.Ss, 1), sc.Se + 1):
                    v = blk[j]
                    v = (abs(v) >> sc.Al) * (1 if v > 0 else -1)
                    if v == 0:
                        run += 1
                        continue
                    while run > 15:
                        cur.append((1, t, 0xF0, 0, 0))
                        run -= 16
                    n, a = _amplitude(v)
                    cur.append((1, t, (run << 4) | n, n, a))
                    run = 0
                if run:
                    cur.append((1, t, 0x00, 0, 0))  # EOB (an EOB run of one block in a progressive scan)
        intervals.append(cur)
        return intervals

    scan_tokens = [tokens(sc) for sc in scans]
    freq = {}
    for ivs in scan_tokens:
        for iv in ivs:
            for cls, t, sym, _, _ in iv:
                if cls >= 0:
                    d = freq.setdefault((cls, t), {})
                    d[sym] = d.get(sym, 0) + 1
    spec = {}
    for key in sorted(freq):
        if huff == "std":
            spec[key] = _std_table(*key)
        else:
            spec[key] = (optimal_table if huff == "optimal" else long_table)(freq[key])
    codes = {key: huffman_codes(*bv) for key, bv in spec.items()}

    def coded(ivs):
        out = bytearray()
        for k, iv in enumerate(ivs):
            if k:
                out += bytes([0xFF, 0xD0 + (k - 1) % 8])
            parts = []
            for cls, t, sym, n, a in iv:
                if cls >= 0:
                    c, l = codes[(cls, t)][sym]
                    parts.append(format(c, "0%db" % l))
                if n:
                    parts.append(format(a, "0%db" % n))
            bits = "".join(parts)
            nbytes = (len(bits) + 7) // 8
            bits = (bits + "1111111")[:nbytes * 8]
            raw = int(bits, 2).to_bytes(nbytes, "big") if nbytes else b""
            out += raw.replace(b"\xff", b"\xff\x00")
        return bytes(out)

    # ---- the file ----
    out = bytearray(b"\xff\xd8")

    def seg(marker, payload=None):
        out.extend(b"\xff" * fill + bytes([0xFF, marker]))
        if payload is not None:
            out.extend((len(payload) + 2).to_bytes(2, "big") + bytes(payload))

    if jfif:
        seg(0xE0, b"JFIF\0\x01\x01\x00\x00\x01\x00\x01\x00\x00")
    if adobe is not None:
        seg(0xEE, b"Adobe\x00\x64\x00\x00\x00\x00" + bytes([adobe]))
    used_q = sorted(set(tq))
    dqt = [bytes([pq << 4 | t]) + b"".join(int(x).to_bytes(2 if pq else 1, "big") for x in qts[t][ZIGZAG])
           for t in used_q]
    for payload in ([b"".join(dqt)] if dqt_merged else dqt):
        seg(0xDB, payload)
    seg(sof, bytes([8]) + H.to_bytes(2, "big") + W.to_bytes(2, "big") + bytes([nc])
        + b"".join(bytes([ids[i], sampling[i][0] << 4 | sampling[i][1], tq[i]]) for i in range(nc)))
    dht = [bytes([cls << 4 | t]) + bytes(bv[0]) + bytes(bv[1]) for (cls, t), bv in spec.items()]
    for payload in ([b"".join(dht)] if dht_merged else dht):
        seg(0xC4, payload)
    if restart:
        seg(0xDD, restart.to_bytes(2, "big"))
    for marker, payload in extra:
        seg(marker, payload)
    scan_bytes = []
    for sc, ivs in zip(scans, scan_tokens):
        seg(0xDA, bytes([len(sc.comps)]) + b"".join(bytes([ids[c], tables[c] << 4 | tables[c]]) for c in sc.comps)
            + bytes([sc.Ss, sc.Se, sc.Ah << 4 | sc.Al]))
        scan_bytes.append(coded(ivs))
        out.extend(scan_bytes[-1])
    seg(0xD9)
    out.extend(trailer)
    return JpegFile(bytes(out), np.concatenate(nat).astype(np.int16), tuple(scan_bytes), (8 * hmax, 8 * vmax))


# ---- the matrix ---------------------------------------------------------------
class Case(NamedTuple):
    name: str
    w: int
    h: int
    pattern: str   # ikutil.synth pattern
    content: str   # "ycc" | "rgb" | "gray" | "cmyk": what the planes hold
    kw: dict       # encode() arguments
    where: str     # entropy decoding the library must count: "gpu" | "host"


BIG = (203, 141)       # off every MCU grid; noise at qstep 2 codes to far more than 4 KiB
GARBAGE = bytes(range(1, 41))
STRAY = ((0xFE, b"a comment between the tables and the scan"), (0xE5, b"APP5\0" + bytes(range(64))))


def _cases():
    out = []

    def add(name, wh, pattern, where, content="ycc", **kw):
        out.append(Case(name, wh[0], wh[1], pattern, content, kw, where))

    layouts = [("440", S440), ("411", S411), ("410", S410), ("311", S311), ("221", S221), ("low", SLOW),
               ("gray22", GRAY22)]
    for tag, s in layouts:
        content = "gray" if len(s) == 1 else "ycc"
        mw, mh = 8 * max(h for h, _ in s), 8 * max(v for _, v in s)
        add(f"{tag}_tiny", (mw + 1, mh + 1), "S", "host", content, sampling=s)
        add(f"{tag}_big", BIG, "N", "gpu", content, sampling=s)
        add(f"{tag}_big_dri5", BIG, "N", "gpu", content, sampling=s, restart=5)
    add("440_1x1", (1, 1), "S", "host", sampling=S440)
    add("410_1x1", (1, 1), "S", "host", sampling=S410)
    # Huffman tables: from the file's own counts, and skewed to 15/16-bit codes; Cb and Cr apart
    for tag, s in (("420", S420), ("440", S440)):
        for huff in ("optimal", "long"):
            for rst in (0, 5):
                add(f"{tag}_{huff}" + ("_dri5" if rst else ""), BIG, "N", "gpu", sampling=s, huff=huff,
                    tables=(0, 1, 2), restart=rst)
    # baseline scan structure: the host entropy decoder by design
    for tag, s in (("420", S420), ("440", S440)):
        for rst in (0, 5):
            add(f"{tag}_scan_per_comp" + ("_dri5" if rst else ""), (75, 53), "S", "host", sampling=s,
                scans=script_per_component(), restart=rst)
    add("420_y_then_chroma", (75, 53), "S", "host", sampling=S420, scans=script_y_then_chroma())
    add("440_y_then_chroma_big", BIG, "N", "host", sampling=S440, scans=script_y_then_chroma(), restart=5)
    # progressive: k_jpeg_prog with restart intervals, the host without
    for tag, s in (("440", S440), ("411", S411), ("221", S221)):
        add(f"{tag}_prog_spectral_dri3", (75, 53), "S", "gpu", sampling=s, sof=SOF2, scans=script_spectral(),
            restart=3)
        add(f"{tag}_prog_dcapprox_dri3", (75, 53), "N", "gpu", sampling=s, sof=SOF2, scans=script_dc_approx(),
            restart=3, huff="optimal", tables=(0, 1, 2))
    add("440_prog_spectral_norst", (75, 53), "S", "host", sampling=S440, sof=SOF2, scans=script_spectral())
    # marker texture, small (12 MCUs) and above 4 KiB
    for tag, wh, pattern, where, rst in (("small", (49, 35), "S", "host", 1), ("big", BIG, "N", "gpu", 7)):
        add(f"fill_{tag}", wh, pattern, where, sampling=S420, fill=3)
        add(f"stray_{tag}", wh, pattern, where, sampling=S420, extra=STRAY)
        add(f"merged_{tag}", wh, pattern, where, sampling=S420, dht_merged=True, dqt_merged=True)
        add(f"trailer_{tag}", wh, pattern, where, sampling=S420, trailer=GARBAGE)
        add(f"rstwrap_{tag}", wh, pattern, where, sampling=S420, restart=rst)
        # colour signalling
        add(f"adobe0_{tag}", wh, pattern, where, "rgb", sampling=S444, jfif=False, adobe=0)
        add(f"adobe0_420_{tag}", wh, pattern, where, "rgb", sampling=S420, jfif=False, adobe=0)
        add(f"adobe1_{tag}", wh, pattern, where, sampling=S420, jfif=False, adobe=1)
        # frame type and table precision
        add(f"sof1_{tag}", wh, pattern, where, sampling=S420, sof=SOF1)
        add(f"pq1_{tag}", wh, pattern, where, sampling=S420, sof=SOF1, pq=1, qstep=40 if tag == "small" else 20)
    # planes of one or two samples per row: libjpeg replicates there where it otherwise interpolates
    for tag, s, wh in (("420_w3", S420, (3, 17)), ("420_w4", S420, (4, 9)), ("422_w4", S422, (4, 9)),
                       ("422_w2", S422, (2, 9)), ("low_w2", SLOW, (2, 5)), ("440_w2", S440, (2, 17))):
        add(tag, wh, "N", "host", sampling=s)
    add("ids_739", (41, 27), "S", "host", sampling=S420, ids=(7, 3, 9))
    add("ids_rgb", (41, 27), "S", "host", "rgb", sampling=S444, ids=(82, 71, 66), jfif=False)
    add("cmyk_adobe0", (41, 27), "S", "host", "cmyk", sampling=S444 + ((1, 1),), jfif=False, adobe=0)
    return out


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


@functools.lru_cache(maxsize=None)
def build(name: str) -> JpegFile:
    c = BY_NAME[name]
    seed = sum(name.encode()) + c.w
    if c.content == "gray":
        planes = ikutil.synth(c.w, c.h, 3, seed=seed, pattern=c.pattern)[..., 1]
    elif c.content == "cmyk":
        planes = ikutil.synth(c.w, c.h, 4, seed=seed, pattern=c.pattern, alpha="random")
    else:
        planes = ikutil.synth(c.w, c.h, 3, seed=seed, pattern=c.pattern)
        if c.content == "ycc":
            planes = ycbcr(planes)
    return encode(planes, **c.kw)
