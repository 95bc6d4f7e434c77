"""A token-level DEFLATE / zlib writer and a token walker (test infrastructure only).

zlib is a conservative writer: it never sends a distance past 32768 - 262, never a
15-bit code back to back with 13 extra bits, never a distance code of one code or
none, never HCLEN 19 without need.  The writer here does not compress: it writes
exactly the blocks, tokens, code lengths and header layout it is told to write
(RFC 1951), so that a test can put the decoder on streams no zlib-made file holds.

  blocks     stored(data) / fixed(tokens) / dynamic(tokens, ll=..., dl=..., ...)
  tokens     an int (a literal byte), (length, distance) (a match), or a raw item:
             ("lsym", s) / ("dsym", s) the code of a symbol, ("bits", value, n)
  lengths    lengths_from_counts (a length-limited Huffman code, optionally with the
             rarest symbols forced to 15 bits), fill_with_dummies (explicit lengths
             completed to a Kraft sum of 1 by unused symbols), SINGLE / NONE distance
             shapes; check_kraft asserts a sum of exactly 1 or the one permitted
             incomplete shape (a single code of length 1; an empty distance code)
  tokenize   a forced parse: a match only where the bytes really repeat at an allowed
             distance (verified byte by byte, overlapping copies included)
  walk       the reader: per block its type, bit extents, code lengths, header layout
             and every token with its bit cost -- the cases assert their properties on
             what walk() finds in the finished stream, never on what the writer was
             asked to do
  zlib_stream / png   the wrappers (CINFO 7, Adler-32; filter type 0 rows, IDAT split)
"""
import heapq
import struct
import zlib

import numpy as np

LBASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEXT = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
DBASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097,
         6145, 8193, 12289, 16385, 24577]
DEXT = [0, 0, 0, 0] + [k for k in range(1, 14) for _ in (0, 1)]
CLORD = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
FIXED_LL = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DL = [5] * 32  # (30 and 31 have codes in the fixed distance code, and no meaning)


def length_symbol(n, alt258=False):
    """(symbol, extra bits, extra value) of match length n; alt258: 258 as 284 + 31"""
    assert 3 <= n <= 258
    if n == 258 and not alt258:
        return 285, 0, 0
    s = max(i for i in range(28) if LBASE[i] <= n)
    assert n - LBASE[s] < (1 << LEXT[s])
    return 257 + s, LEXT[s], n - LBASE[s]


def distance_symbol(d):
    assert 1 <= d <= 32768
    s = max(i for i in range(30) if DBASE[i] <= d)
    return s, DEXT[s], d - DBASE[s]


# ---- code lengths ----
def kraft(lens):
    """the Kraft sum of a code in units of 2^-15"""
    return sum(1 << (15 - n) for n in lens if n)


def check_kraft(lens, is_dist=False):
    """A complete code, or the one incomplete shape DEFLATE readers accept: a single
    code of length 1 (for the distance code also no code at all)."""
    k, used = kraft(lens), [n for n in lens if n]
    assert all(1 <= n <= 15 for n in used)
    assert k == 1 << 15 or used == [1] or (is_dist and not used), ("Kraft sum", k / 32768, used[:8])


def codes(lens):
    """canonical codes, bit-reversed for the LSB-first stream: {symbol: (code, length)}"""
    count = [0] * 16
    for n in lens:
        count[n] += 1
    count[0] = 0
    nxt, code = [0] * 16, 0
    for b in range(1, 16):
        code = (code + count[b - 1]) << 1
        nxt[b] = code
    out = {}
    for s, n in enumerate(lens):
        if n:
            out[s] = (int(format(nxt[n], "0%db" % n)[::-1], 2), n)
            nxt[n] += 1
    return out


def _huffman(freq, limit):
    """{symbol: length <= limit} with a Kraft sum of 1 (two or more symbols)"""
    assert len(freq) >= 2 and len(freq) <= 1 << limit
    heap = [(f, i, (s,)) for i, (s, f) in enumerate(sorted(freq.items()))]
    heapq.heapify(heap)
    depth, tick = dict.fromkeys(freq, 0), len(heap)
    while len(heap) > 1:
        fa, _, sa = heapq.heappop(heap)
        fb, _, sb = heapq.heappop(heap)
        for s in sa + sb:
            depth[s] += 1
        heapq.heappush(heap, (fa + fb, tick, sa + sb))
        tick += 1
    num = [0] * (limit + 1)
    for d in depth.values():
        num[min(d, limit)] += 1
    total = sum(num[n] << (limit - n) for n in range(1, limit + 1))
    while total > 1 << limit:  # (the usual repair: shorten the code space one unit at a time)
        num[limit] -= 1
        for n in range(limit - 1, 0, -1):
            if num[n]:
                num[n] -= 1
                num[n + 1] += 2
                break
        total -= 1
    order = sorted(freq, key=lambda s: (-freq[s], s))
    out, i = {}, 0
    for n in range(1, limit + 1):
        for s in order[i:i + num[n]]:
            out[s] = n
        i += num[n]
    return out


def fill_with_dummies(lens, dummies, is_dist=False):
    """Complete explicit lengths to a Kraft sum of 1: the code space left over goes to
    `dummies` (symbols the block never sends), one per set bit of the remainder."""
    lens, rest = list(lens), (1 << 15) - kraft(lens)
    assert rest >= 0, "oversubscribed"
    dummies = list(dummies)
    for b in range(14, -1, -1):
        if rest >> b & 1:
            s = dummies.pop(0)
            assert lens[s] == 0
            lens[s] = 15 - b
    check_kraft(lens, is_dist)
    return lens


def lengths_from_counts(counts, depth=15, deep=0, dummies=()):
    """Code lengths for the symbols counts sends (counts[s] > 0), none longer than depth.
    depth <= 10 keeps a literal/length code on the decoder's fast table.  deep = k (with
    depth 15): the k rarest symbols get 15 bits exactly -- they hang together under one
    node of the Huffman tree, the rest of that node's code space goes to `dummies`."""
    n = len(counts)
    freq = {s: c for s, c in enumerate(counts) if c}
    lens = [0] * n
    if deep:
        assert depth == 15
        rare = sorted(freq, key=lambda s: (freq[s], -s))[:deep]
        for s in rare:
            del freq[s]
        freq[-1] = 0  # the node that holds them
        if len(freq) < 2:
            freq[-2] = 0
        hl = _huffman(freq, 15 - max(1, (deep - 1).bit_length()))
        for s, v in hl.items():
            if s >= 0:
                lens[s] = v
        for s in rare:
            lens[s] = 15
        assert (1 << (15 - hl[-1])) >= deep
        return fill_with_dummies(lens, dummies)  # (what the node's subtree has left, to symbols never sent)
    if len(freq) < 2:  # (a complete code needs two symbols: the first dummy joins in)
        freq[[s for s in dummies if s not in freq][0]] = 0
    for s, v in _huffman(freq, depth).items():
        lens[s] = v
    check_kraft(lens)
    return lens


def token_counts(tokens, alt258=False):
    """literal/length and distance symbol counts of a token list (with the end-of-block code)"""
    lc, dc = [0] * 286, [0] * 30
    lc[256] = 1
    for t in tokens:
        if isinstance(t, int):
            lc[t] += 1
        elif t[0] == "lsym":
            lc[t[1]] += 1
        elif t[0] == "dsym":
            dc[t[1]] += 1
        elif t[0] != "bits":
            lc[length_symbol(t[0], alt258)[0]] += 1
            dc[distance_symbol(t[1])[0]] += 1
    return lc, dc


# ---- blocks ----
def stored(data, final=False, nlen=None):
    return {"type": 0, "final": final, "data": bytes(data), "nlen": nlen}


def fixed(tokens, final=False, eob=True):
    return {"type": 1, "final": final, "tokens": list(tokens), "eob": eob}


def dynamic(tokens, final=False, ll=None, dl=None, depth=15, deep=0, dist="auto", hclen=None, repeats=True,
            cross=True, hlit=None, hdist=None, alt258=False, ops=None, check=True, eob=True):
    """A dynamic block.  ll / dl: explicit code lengths (else from the tokens' counts by
    lengths_from_counts(depth, deep)); dist: "auto", "single" (one distance code of
    length 1) or "none" (HDIST 1, that length 0).  Header layout: hlit / hdist (at least
    what the lengths need), hclen (at least what the code-length code needs), repeats
    (code-length symbols 16/17/18 used or not), cross (a repeat may run from the
    literal/length lengths into the distance lengths).  alt258: length 258 as 284 + 31.
    ops: the code-length symbols verbatim [(symbol, extra value)] (defect cases);
    check=False skips the Kraft assertions (defect cases)."""
    tokens = list(tokens)
    lc, dc = token_counts(tokens, alt258)
    if not eob:
        lc[256] = 0
    if ll is None:
        unused = [s for s in range(286) if not lc[s]]
        ll = lengths_from_counts(lc, depth, deep, unused)
    if dl is None:
        used = [s for s in range(30) if dc[s]]
        if dist == "none":
            assert not used
            dl = [0]
        elif dist == "single":
            assert len(used) == 1
            dl = [0] * used[0] + [1]
        elif not used:
            dl = [1, 1]  # (what zlib sends for a block without matches)
        else:
            dl = lengths_from_counts(dc, 15, 0, [s for s in range(30) if not dc[s]])
    ll, dl = list(ll), list(dl)
    while len(ll) > 257 and not ll[-1]:
        ll.pop()
    while len(dl) > 1 and not dl[-1]:
        dl.pop()
    ll += [0] * (max(hlit or 257, 257) - len(ll))
    dl += [0] * ((hdist or 1) - len(dl))
    if check:
        check_kraft(ll)
        check_kraft(dl, True)
        assert ll[256]
    return {"type": 2, "final": final, "tokens": tokens, "ll": ll, "dl": dl, "hclen": hclen, "repeats": repeats,
            "cross": cross, "alt258": alt258, "ops": ops, "eob": eob}


def _rle(seq, repeats):
    """code-length symbols [(symbol, extra value)] for the lengths seq"""
    if not repeats:
        return [(n, 0) for n in seq]
    ops, i = [], 0
    while i < len(seq):
        j = i
        while j < len(seq) and seq[j] == seq[i]:
            j += 1
        run, v = j - i, seq[i]
        if v == 0:
            while run >= 11:
                k = min(run, 138)
                ops.append((18, k - 11))
                run -= k
            if run >= 3:
                ops.append((17, run - 3))
                run = 0
        else:
            ops.append((v, 0))
            run -= 1
            while run >= 3:
                k = min(run, 6)
                ops.append((16, k - 3))
                run -= k
        ops += [(v, 0)] * run
        i = j
    return ops


class _Bits:
    def __init__(self):
        self.out, self.acc, self.n = bytearray(), 0, 0

    def put(self, v, n):
        assert 0 <= v < 1 << n
        self.acc |= v << self.n
        self.n += n
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def align(self):
        if self.n:
            self.put(0, 8 - self.n)

    def bit(self):
        return 8 * len(self.out) + self.n


def _put_tokens(w, tokens, lcode, dcode, alt258, eob):
    for t in tokens:
        if isinstance(t, int):
            w.put(*lcode[t])
        elif t[0] == "lsym":
            w.put(*lcode[t[1]])
        elif t[0] == "dsym":
            w.put(*dcode[t[1]])
        elif t[0] == "bits":
            w.put(t[1], t[2])
        else:
            s, n, v = length_symbol(t[0], alt258)
            w.put(*lcode[s])
            w.put(v, n)
            s, n, v = distance_symbol(t[1])
            w.put(*dcode[s])
            w.put(v, n)
    if eob:
        w.put(*lcode[256])


def deflate(blocks, w=None):
    """the raw DEFLATE bytes of the blocks (the last one should be final)"""
    w = w or _Bits()
    for b in blocks:
        w.put(1 if b["final"] else 0, 1)
        w.put(b["type"], 2)
        if b["type"] == 0:
            w.align()
            n = len(b["data"])
            assert n <= 65535
            w.put(n, 16)
            w.put(n ^ 0xFFFF if b["nlen"] is None else b["nlen"], 16)
            w.out += b["data"]
        elif b["type"] == 1:
            _put_tokens(w, b["tokens"], codes(FIXED_LL), codes(FIXED_DL), False, b["eob"])
        elif b["type"] == 2:
            ll, dl = b["ll"], b["dl"]
            if b["ops"] is not None:
                ops = b["ops"]
            elif b["cross"]:
                ops = _rle(ll + dl, b["repeats"])
            else:
                ops = _rle(ll, b["repeats"]) + _rle(dl, b["repeats"])
            cc = [0] * 19
            for s, _ in ops:
                cc[s] += 1
            cl = lengths_from_counts(cc, 7, 0, [s for s in (0, 8, 7, 9) if not cc[s]])
            need = max(i for i in range(19) if cl[CLORD[i]]) + 1
            hclen = b["hclen"] or max(need, 4)
            assert hclen >= need, f"HCLEN {hclen} cannot carry this code-length code (needs {need})"
            w.put(len(ll) - 257, 5)
            w.put(len(dl) - 1, 5)
            w.put(hclen - 4, 4)
            for i in range(hclen):
                w.put(cl[CLORD[i]], 3)
            ccode = codes(cl)
            for s, v in ops:
                w.put(*ccode[s])
                if s >= 16:
                    w.put(v, {16: 2, 17: 3, 18: 7}[s])
            _put_tokens(w, b["tokens"], codes(ll), codes(dl), b["alt258"], b["eob"])
        else:
            pass  # BTYPE 3: the three header bits alone
    w.align()
    return bytes(w.out)


def zlib_stream(blocks, raw):
    """CMF/FLG (CINFO 7: a 32 KiB window, no FDICT) + the blocks + Adler-32 of raw"""
    return b"\x78\x01" + deflate(blocks) + struct.pack(">I", zlib.adler32(raw) & 0xFFFFFFFF)


# ---- the forced parse ----
def tokenize(raw, distances=None, min_distance=None, only258=False, lengths=(258,), start=0, end=None):
    """Tokens of raw[start:end].  A match is sent only where the bytes really repeat
    (raw[i + k] == raw[i + k - d] for every k: the overlapping-copy rule) at a distance
    from `distances`, or at any distance >= min_distance; the k-th match is at most
    lengths[k % len(lengths)] long; only258: matches of length 258 and no others.
    Everything else is a literal.  Among the allowed distances the longest run wins
    (the first listed on a tie)."""
    a = np.frombuffer(bytes(raw), np.uint8)
    n = len(a)
    end = n if end is None else end
    ds = list(distances) if distances is not None else list(range(min_distance, 32769))
    best, bestd = np.zeros(n, np.int32), np.zeros(n, np.int32)
    idx = np.arange(n, dtype=np.int32)
    for d in ds:
        if d >= n:
            continue
        eq = a[d:] == a[:-d]
        if not eq.any():
            continue
        nf = np.where(eq, n, idx[d:])
        run = np.minimum.accumulate(nf[::-1])[::-1] - idx[d:]
        run = np.where(eq, np.minimum(run, end - idx[d:]), 0)
        better = run > best[d:]
        best[d:][better] = run[better]
        bestd[d:][better] = d
    out, i, k = [], start, 0
    while i < end:
        cap = 258 if only258 else lengths[k % len(lengths)]
        m = min(int(best[i]), cap, end - i)
        if m >= 3 and (not only258 or m == 258):
            d = int(bestd[i])
            assert raw[i:i + m] == bytes(raw[i - d + j % d] for j in range(m)) if m > d else raw[i:i + m] == raw[i - d:i - d + m]
            out.append((m, d))
            i += m
            k += 1
        else:
            out.append(raw[i])
            i += 1
    return out


def token_bytes(tokens, history=b""):
    """what the tokens decode to after `history` (the check of a hand-made token list)"""
    out = bytearray(history)
    for t in tokens:
        if isinstance(t, int):
            out.append(t)
        else:
            n, d = t
            assert d <= len(out)
            for _ in range(n):
                out.append(out[-d])
    return bytes(out[len(history):])


# ---- the walker ----
_tables = {}


def _table(lens):
    """entry at the next 15 stream bits (first bit lowest): symbol << 4 | code length"""
    key = tuple(lens)
    if key not in _tables:
        if len(_tables) > 64:
            _tables.clear()
        tab = [0] * 32768
        for s, (r, n) in codes(lens).items():
            tab[r::1 << n] = [(s << 4) | n] * (32768 >> n)
        _tables[key] = tab
    return _tables[key]


def walk(z, max_blocks=None, tokens=True):
    """The blocks of zlib stream z, each a dict: type, final, hdr / body / end (bit
    positions from the stream's first byte: the header's first bit, the body's first bit,
    the bit past the end-of-block code or the stored bytes), out (output bytes before the
    block), n_out, stored: len; dynamic: hlit, hdist, hclen, ll, dl, cl_used (the
    code-length symbols sent), cross (a repeat ran over the literal/distance boundary);
    coded: tokens [(kind, ...)]: ("lit", byte, bits), ("match", length, distance, bits,
    length symbol, length code bits, distance symbol, distance code bits, distance extra
    value), and eob_bits."""
    buf = z + b"\0" * 8

    def bits(pos, n):
        return (int.from_bytes(buf[pos >> 3:(pos >> 3) + 4], "little") >> (pos & 7)) & ((1 << n) - 1)

    pos, out, total = 16, [], 0
    while True:
        b = {"hdr": pos, "final": bits(pos, 1), "type": bits(pos + 1, 2), "out": total}
        bt = b["type"]
        pos += 3
        assert bt != 3
        if bt == 0:
            pos = (pos + 7) & ~7
            n = bits(pos, 16)
            assert n ^ 0xFFFF == bits(pos + 16, 16)
            b["body"] = pos + 32
            b["len"] = b["n_out"] = n
            pos = b["body"] + 8 * n
        else:
            if bt == 1:
                ll, dl = FIXED_LL, FIXED_DL
            else:
                hlit, hdist, hclen = bits(pos, 5) + 257, bits(pos + 5, 5) + 1, bits(pos + 10, 4) + 4
                pos += 14
                cl = [0] * 19
                for i in range(hclen):
                    cl[CLORD[i]] = bits(pos, 3)
                    pos += 3
                ct, lens, used, cross = _table(cl), [], set(), False
                while len(lens) < hlit + hdist:
                    e = ct[bits(pos, 15)]
                    assert e
                    s = e >> 4
                    pos += e & 15
                    used.add(s)
                    before = len(lens)
                    if s < 16:
                        lens.append(s)
                    elif s == 16:
                        lens += [lens[-1]] * (3 + bits(pos, 2))
                        pos += 2
                    elif s == 17:
                        lens += [0] * (3 + bits(pos, 3))
                        pos += 3
                    else:
                        lens += [0] * (11 + bits(pos, 7))
                        pos += 7
                    cross = cross or (s >= 16 and before < hlit < len(lens))
                assert len(lens) == hlit + hdist
                ll, dl = lens[:hlit], lens[hlit:]
                b.update(hlit=hlit, hdist=hdist, hclen=hclen, cl=cl, cl_used=used, cross=cross)
            b.update(ll=list(ll), dl=list(dl))
            lt, dt = _table(ll), _table(dl)
            b["body"] = pos
            toks, n_out = [], 0
            while True:
                e = lt[bits(pos, 15)]
                assert e
                s, ln = e >> 4, e & 15
                p0 = pos
                pos += ln
                if s < 256:
                    n_out += 1
                    if tokens:
                        toks.append(("lit", s, ln))
                    continue
                if s == 256:
                    b["eob_bits"] = ln
                    break
                assert s <= 285
                length = LBASE[s - 257] + bits(pos, LEXT[s - 257])
                pos += LEXT[s - 257]
                e = dt[bits(pos, 15)]
                assert e
                ds, dn = e >> 4, e & 15
                assert ds <= 29
                pos += dn
                dx = bits(pos, DEXT[ds])
                pos += DEXT[ds]
                n_out += length
                if tokens:
                    toks.append(("match", length, DBASE[ds] + dx, pos - p0, s, ln, ds, dn, dx))
            b["tokens"], b["n_out"] = toks, n_out
        b["end"] = pos
        total += b["n_out"]
        out.append(b)
        if b["final"]:
            assert ((pos + 7) >> 3) + 4 == len(z), "the walk must end at the Adler-32"
            break
        if max_blocks and len(out) >= max_blocks:
            break
    return out


def deflate_blocks(z, max_blocks=None):
    """The blocks of zlib stream z: (btype, header bit, first body bit, bit past the
    end-of-block code / the stored bytes); bit positions from the stream's first byte."""
    return [(b["type"], b["hdr"], b["body"], b["end"]) for b in walk(z, max_blocks, tokens=False)]


def matches(blocks):
    return [t for b in blocks if b["type"] for t in b["tokens"] if t[0] == "match"]


# ---- PNG ----
def _chunk(t, d):
    return struct.pack(">I", len(d)) + t + d + struct.pack(">I", zlib.crc32(t + d) & 0xFFFFFFFF)


def raw_rows(img, filters=0):
    """the stream's bytes of image img (h, w, c): filter type 0 rows hold the image's own
    bytes; `filters` (an int or one per row) only sets the type byte -- the bytes given
    are then the filtered ones"""
    h = img.shape[0]
    ft = [filters] * h if isinstance(filters, int) else list(filters)
    return b"".join(bytes([ft[y]]) + img[y].tobytes() for y in range(h))


def rows_image(raw, w, h, c):
    """the image whose filter-type-0 stream is raw (every row's type byte must be 0)"""
    a = np.frombuffer(raw, np.uint8).reshape(h, 1 + w * c)
    assert not a[:, 0].any()
    return a[:, 1:].reshape(h, w, c).copy()


def png(img, z, idat=None):
    """A PNG file of 8-bit image img (h, w, c: gray, gray+alpha, RGB, RGBA) around zlib
    stream z; idat: the stream in IDAT chunks of that many bytes."""
    h, w, c = img.shape
    ihdr = struct.pack(">IIBBBBB", w, h, 8, {1: 0, 2: 4, 3: 2, 4: 6}[c], 0, 0, 0)
    parts = [z] if not idat else [z[i:i + idat] for i in range(0, len(z), idat)]
    return (b"\x89PNG\r\n\x1a\n" + _chunk(b"IHDR", ihdr) + b"".join(_chunk(b"IDAT", p) for p in parts) +
            _chunk(b"IEND", b""))
