"""The DEFLATE streams zlib cannot write, as named cases (deflate_writer.py writes them).

valid(name)   -> Case: image, raw (the filter-type-0 rows), zlib stream z, PNG file, and
                 `found`: the case's property as counted on the walked stream (every
                 case asserts it there, and the tests print it)
invalid(name) -> Bad: a valid case's image with one defect in the stream (PNG CRCs valid)

The content of every case is chosen so that the property holds by construction of the
bytes (rows that repeat at a known distance, planted copies), and then the property is
read back from the finished stream by deflate_writer.walk."""
import collections
import os
import re

import numpy as np

import deflate_writer as dw

_HDR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "rust-image-transform_amd", "csrc")


def _constant(header, pattern):
    """a constant as the header states it (the cases follow the decoder's sizes)"""
    with open(os.path.join(_HDR, header)) as f:
        m = re.search(pattern, f.read())
    assert m, f"{header} no longer states {pattern}"
    return int(m.group(1))


WINDOW_BYTES = _constant("ik_png_wave.h", r"#define\s+IK_WAVE_WINDOW_BYTES\s+(\d+)")
WAVE_CHUNK = _constant("ik_png.h", r"kPngWaveChunkBytes\s*=\s*(\d+)")
K_LB = _constant("ik_png_wave.h", r"constexpr\s+int\s+kLB\s*=\s*(\d+)")  # the fast tables' bits
K_DB = _constant("ik_png_wave.h", r"constexpr\s+int\s+kDB\s*=\s*(\d+)")

Case = collections.namedtuple("Case", "name img raw z png found")
Bad = collections.namedtuple("Bad", "name img z png")

VALID = ["dist_max", "dist_top", "far_across_lanes", "worst_step", "worst_step_lit", "all_slow", "pair_beside_slow",
         "single_dist", "no_dist", "hdr_extremes", "len258_alt", "stored_edges", "mixed_types", "empty_blocks"]
# Valid streams the GPU path hands to the host decoder: a gap, not a pass (DESIGN.md
# section 8).  The one set for both decoders; the tests assert it exactly.
#   empty_blocks  wave decoder (the default): a lane whose piece table is full ends at a
#       block boundary and the chain check starts a new lane there, one per decode round;
#       each new lane takes a token region of its own, and a lone stream's token area
#       (sized for the first round plus half) runs out.  The CPU model, which has no
#       areas, decodes it.  Lane decoder (IK_PNG_DECODE=lane): a coded block costs it a
#       136-token table, an empty one 10 bits -- its token region overflows (the model too).
EXPECTED_FALLBACK = {"empty_blocks"}
INVALID = ["far_at_byte_0", "far_before_start", "single_dist_unused_code", "no_dist_match", "repeat_first",
           "lengths_overrun", "no_end_of_block", "oversubscribed", "incomplete", "length_symbol_286",
           "fixed_distance_30", "stored_nlen", "btype_3"]


def _rng(name):
    return np.random.default_rng(sum(map(ord, name)) * 8)


def _noise_raw(rng, w, h, c, levels=256):
    """filter-type-0 rows of a noise image, as a bytearray (stride 1 + w * c)"""
    img = rng.integers(0, levels, size=(h, w, c), dtype=np.uint8)
    return bytearray(dw.raw_rows(img))


def _plant(raw, stride, dest, n, d):
    """raw[dest : dest + n] becomes a copy from d back (overlap as DEFLATE copies); the
    destination lies inside one row's pixel bytes, so the filter type bytes stay 0"""
    assert dest % stride >= 1 and dest % stride + n <= stride and dest - d >= 0
    for k in range(n):
        raw[dest + k] = raw[dest + k - d]


def _finish(name, raw, w, h, c, blocks, found, idat=None):
    raw = bytes(raw)
    assert len(raw) == h * (1 + w * c)
    img = dw.rows_image(raw, w, h, c)
    z = dw.zlib_stream(blocks, raw)
    return Case(name, img, raw, z, dw.png(img, z, idat), found(dw.walk(z)))


def _final(blocks):
    blocks[-1]["final"] = True
    return blocks


# ---- valid cases ----
def _dist_max(name):
    # gray 255 wide: rows of 256 bytes, 128 rows = 32768 bytes exactly
    rng = _rng(name)
    raw = _noise_raw(rng, 255, 128, 1) * 3
    toks = [int(b) for b in raw[:32768]] + dw.tokenize(raw, distances=[32768], lengths=(258, 3, 4, 100, 258, 5, 31),
                                                        start=32768)

    def found(bl):
        m = [t for t in dw.matches(bl) if t[2] == 32768]
        lens = {t[1] for t in m}
        assert len(m) >= 100 and {3, 258} <= lens and all(t[6] == 29 and t[8] == 8191 for t in m)
        return f"{len(m)} matches at distance 32768, lengths {min(lens)}..{max(lens)} ({len(lens)} distinct)"
    return _finish(name, raw, 255, 384, 1, _final([dw.dynamic(toks)]), found)


_TOP = [32507, 32767, 32768, 24577]


def _dist_top(name):
    rng = _rng(name)
    w, h = 255, 260
    raw = _noise_raw(rng, w, h, 1)
    for r in range(128, h):
        d = _TOP[r % 4]
        n = int(rng.integers(3, 200))
        off = int(rng.integers(1, 256 - n))
        _plant(raw, 256, r * 256 + off, n, d)
    toks = dw.tokenize(raw, distances=_TOP)

    def found(bl):
        cnt = collections.Counter(t[2] for t in dw.matches(bl))
        assert all(cnt[d] >= 20 for d in _TOP), cnt
        ex = {t[8] for t in dw.matches(bl) if t[6] == 29}
        assert {0, 8191} <= ex
        return ", ".join(f"{cnt[d]} at {d}" for d in _TOP) + "; symbol 29 extra bits include 0 and 8191"
    return _finish(name, raw, w, h, 1, _final([dw.dynamic(toks)]), found)


def _far_across_lanes(name):
    rng = _rng(name)
    w, h, c = 256, 192, 4
    stride = 1 + w * c
    raw = _noise_raw(rng, w, h, c)
    per = 12 * stride
    starts = [k * per + 1 for k in range(1, len(raw) // per + 1) if k * per + 1 + 700 < len(raw)]
    for s in starts:
        if s >= 32768:
            _plant(raw, stride, s, 258, 32768)       # a copy from the window's oldest byte, first in its block
            _plant(raw, stride, s + 258, 100, 32767)
            _plant(raw, stride, s + 358, 40, 32507)
    toks = dw.tokenize(raw, min_distance=32507)
    # blocks cut at the planted copies: a block's first token is the copy from 32768 back
    blocks, cur, pos, cuts = [], [], 0, set(starts)
    for t in toks:
        if pos in cuts and cur:
            blocks.append(dw.dynamic(cur))
            cur = []
        cur.append(t)
        pos += 1 if isinstance(t, int) else t[0]
    blocks.append(dw.dynamic(cur))

    def found(bl):
        assert all(b["type"] == 2 and b["n_out"] <= 16384 for b in bl)
        hit = first = 0
        for b in bl:
            o, got, at0 = b["out"], False, False
            for t in b["tokens"]:
                if o - b["out"] >= 258:
                    break
                if t[0] == "match" and t[2] >= 32507:
                    got = True
                    at0 = at0 or (o == b["out"] and t[2] == 32768)
                o += 1 if t[0] == "lit" else t[1]
            hit += got
            first += at0
        assert hit >= 8 and first >= 8
        return (f"{len(bl)} dynamic blocks of <= {max(b['n_out'] for b in bl)} B; {hit} blocks with a match of distance "
                f">= 32507 starting in their first 258 bytes, {first} of them a copy from 32768 as the block's first token")
    case = _finish(name, raw, w, h, c, _final(blocks), found)
    assert len(case.z) > 2 * WAVE_CHUNK
    return case


def _worst_step(name, with_literal):
    rng = _rng(name)
    w, c = 64, 4
    stride = 1 + w * c  # 257: copies from k rows up keep the filter type bytes 0
    raw = _noise_raw(rng, w, 128, c, levels=128)
    toks = [int(b) for b in raw]
    target = stride * 330
    n48 = 0
    while len(raw) < target:
        left = target - len(raw)
        if with_literal and n48 and isinstance(toks[-1], tuple) and left > 600:
            b = 0 if len(raw) % stride == 0 else int(rng.integers(0, 128))
            raw.append(b)
            toks.append(b)
            continue
        # every match 131..257 long (symbols 281..284), the last ones sized to end the last row
        n = int(rng.integers(131, 258)) if left > 600 else 131 if left > 514 else left // 2 if left >= 262 else left
        assert 131 <= n <= 257
        # (every distance is a whole number of rows, so the filter type bytes copy as 0)
        k = int(rng.integers(64, min(127, len(raw) // stride) + 1))
        d = k * stride
        for _ in range(n):
            raw.append(raw[-d])
        toks.append((n, d))
        n48 += 1
    assert dw.token_bytes(toks) == bytes(raw)
    # literals 0..127 at 8 bits (1/2), end-of-block at 2 (1/4), length symbols 281..284 at 15;
    # distance symbols 28 and 29 at 15; the rest of both code spaces to symbols never sent
    ll = [8] * 128 + [0] * 158
    ll[256] = 2
    for s in (281, 282, 283, 284):
        ll[s] = 15
    ll = dw.fill_with_dummies(ll, list(range(128, 256)))
    dl = [0] * 30
    dl[28] = dl[29] = 15
    dl = dw.fill_with_dummies(dl, list(range(28)), True)

    def found(bl):
        assert len(bl) == 1 and bl[0]["type"] == 2
        assert all(bl[0]["ll"][s] == 15 for s in (281, 282, 283, 284)) and bl[0]["dl"][28] == bl[0]["dl"][29] == 15
        t = bl[0]["tokens"]
        best = run = 0
        i = 0
        while i < len(t):
            if t[i][0] == "match" and t[i][3] == 48:
                run += 1
                best = max(best, run)
                i += 2 if with_literal and i + 1 < len(t) and t[i + 1][0] == "lit" else 1
            else:
                run = 0
                i += 1
        assert best >= 200
        syms = collections.Counter(x[6] for x in t if x[0] == "match" and x[3] == 48)
        assert syms[28] >= 20 and syms[29] >= 20
        return (f"{best} consecutive 48-bit matches" + (" with one literal between each two" if with_literal else "") +
                f" (distance symbol 28: {syms[28]}, 29: {syms[29]})")
    return _finish(name, raw, w, len(raw) // stride, c, _final([dw.dynamic(toks, ll=ll, dl=dl)]), found)


def _all_slow(name):
    rng = _rng(name)
    w, c, stride = 64, 4, 257
    # block 1: every literal at 11 bits (1/8 of the code space), the rest to symbols 257 / 258
    # (never sent) and the end-of-block code
    raw = _noise_raw(rng, w, 64, c)
    n1 = 32 * stride
    ll = [11] * 256 + [3, 1, 2]
    b1 = dw.dynamic([int(b) for b in raw[:n1]], ll=ll, dist="none")
    # block 2: copies within a row at distances 17..256, whose symbols 8..15 get 9..15 bits
    for r in range(32, 64):
        off = 80
        while off + 40 < stride:
            n = int(rng.integers(3, 31))
            lo = 17
            hi = min(256, off - 1)
            _plant(raw, stride, r * stride + off, n, int(rng.integers(lo, hi + 1)))
            off += n + int(rng.integers(2, 8))
    toks = dw.tokenize(raw, distances=range(17, 257), lengths=(30,), start=n1)
    dl = list(range(1, 16)) + [15]
    b2 = dw.dynamic(toks, dl=dl, final=True)

    assert K_LB < 11 and K_DB < 9, "the codes of this case (11 and 9..15 bits) are no longer slow ones"

    def found(bl):
        a, b = bl
        slow = sum(1 for t in a["tokens"] if t[2] > K_LB)
        total = len(a["tokens"]) + 1
        assert slow >= 0.9 * total
        m = [t for t in b["tokens"] if t[0] == "match"]
        ds = sum(1 for t in m if t[7] > K_DB)
        assert len(m) >= 100 and ds >= 0.9 * len(m)
        return (f"block 1: {slow} of {total} body symbols with a code longer than {K_LB} bits; block 2: {ds} of {len(m)} "
                f"matches with a distance code longer than {K_DB} bits")
    return _finish(name, raw, w, 64, c, [b1, b2], found)


def _pair_beside_slow(name):
    rng = _rng(name)
    w, h, c = 65, 60, 4
    stride = 1 + w * c  # 261 = 87 triples of (short, short, long); a row's type byte 0 is a short literal
    short = [0, 1, 2]                         # 2, 2 and 3 bits
    pool = list(range(3, 243))                # 11..15 bits
    plen = [11] * 100 + [12] * 60 + [13] * 40 + [14] * 24 + [15] * 16
    raw = bytearray()
    for i in range(stride * h):
        if i % stride == 0:
            raw.append(0)
        elif i % 3 == 2:
            raw.append(pool[int(rng.integers(0, len(pool)))])
        else:
            raw.append(short[int(rng.integers(0, 3))])
    ll = [0] * 286
    ll[0], ll[1], ll[2] = 2, 2, 3
    for s, n in zip(pool, plen):
        ll[s] = n
    ll[256] = 11
    ll = dw.fill_with_dummies(ll, list(range(257, 286)) + list(range(243, 256)))

    def found(bl):
        t = bl[0]["tokens"]
        assert all(x[0] == "lit" for x in t) and len(t) == stride * h
        assert all((11 <= x[2] <= 15) if i % 3 == 2 else (2 <= x[2] <= 3) for i, x in enumerate(t))
        assert bl[0]["eob_bits"] == 11
        deep = collections.Counter(x[2] for i, x in enumerate(t) if i % 3 == 2)
        return (f"{len(t) // 3} times two literals of 2-3 bits, then one of 11..15 bits "
                f"({', '.join(f'{deep[n]} of {n}' for n in sorted(deep))})")
    return _finish(name, raw, w, h, c, _final([dw.dynamic([int(b) for b in raw], ll=ll, dist="none")]), found)


def _single_dist(name, defect=False):
    rng = _rng(name)
    w, h, c, stride = 64, 100, 4, 257
    raw = _noise_raw(rng, w, h, c)
    for r in range(2, h):
        n = int(rng.integers(3, 60))
        off = int(rng.integers(1, stride - n))
        _plant(raw, stride, r * stride + off, n, (257, 300, 384)[r % 3])
    toks = dw.tokenize(raw, distances=[257, 300, 384])
    if defect:  # the other code of the one-bit distance code: a length symbol, then a 1 bit
        k = [i for i, t in enumerate(toks) if isinstance(t, tuple)][20]
        toks = toks[:k] + [("lsym", dw.length_symbol(toks[k][0])[0]), ("bits", 1, 1)]
        return raw, w, h, c, [dw.dynamic(toks, dl=[0] * 16 + [1], final=True)]

    def found(bl):
        dl = bl[0]["dl"]
        m = dw.matches(bl)
        assert [n for n in dl if n] == [1] and len(m) >= 50
        assert bl[0]["end"] - bl[0]["body"] > 8 * WINDOW_BYTES
        return (f"one distance code (symbol {dl.index(1)}, 1 bit) used by {len(m)} matches; body "
                f"{(bl[0]['end'] - bl[0]['body']) // 8} B > the {WINDOW_BYTES} B window")
    return _finish(name, raw, w, h, c, _final([dw.dynamic(toks, dist="single")]), found)


def _no_dist(name, defect=False):
    rng = _rng(name)
    w, h, c = 33, 17, 4
    raw = _noise_raw(rng, w, h, c, levels=40)
    half = len(raw) // 2
    if defect:  # a length symbol where the block has no distance code at all
        lc = dw.token_counts([int(b) for b in raw[half:]])[0]
        lc[257] = 1
        ll = dw.lengths_from_counts(lc)
        return raw, w, h, c, [dw.dynamic([int(b) for b in raw[:half]], dist="none"),
                              dw.dynamic([int(b) for b in raw[half:half + 50]] + [("lsym", 257), ("bits", 0, 8)], ll=ll,
                                         dl=[0], final=True)]
    blocks = [dw.dynamic([int(b) for b in raw[:half]], dist="none"), dw.dynamic([int(b) for b in raw[half:]], dist="none", depth=9)]

    def found(bl):
        assert len(bl) == 2 and all(b["type"] == 2 and b["hdist"] == 1 and b["dl"] == [0] for b in bl)
        assert not dw.matches(bl) and max(bl[1]["ll"]) <= 9
        return f"2 dynamic blocks with HDIST 1 and that length 0, {sum(len(b['tokens']) for b in bl)} literals"
    return _finish(name, raw, w, h, c, _final(blocks), found)


def _hdr_extremes(name):
    rng = _rng(name)
    w, h, c, stride = 64, 48, 4, 257
    raw = _noise_raw(rng, w, h, c, levels=255)
    for r in range(16, h):  # (copies for the blocks with distance codes)
        _plant(raw, stride, r * stride + 9, 40, stride * (1 + r % 8))
        _plant(raw, stride, r * stride + 100, 12, (1, 2, 3, 4, 6, 24, 100, 1000)[r % 8])
    n1, n2 = 16 * stride, 32 * stride
    # A: HCLEN 5 -- the code-length code may then only hold 16, 17, 18, 0 and 8: literals
    #    0..254 and the end-of-block code at 8 bits (255 absent), HLIT 257, HDIST 1 with length 0
    #    (HCLEN 4 leaves 16, 17, 18 and 0: every length 0, no end-of-block code; no valid block has it)
    a = dw.dynamic([int(b) for b in raw[:n1]], ll=[8] * 255 + [0, 8], dist="none", hclen=5)
    # B: HCLEN 19, HLIT 286, HDIST 30, every length sent as itself (no 16 / 17 / 18)
    tb = dw.tokenize(raw, distances=[stride * k for k in range(1, 9)] + [1, 2, 3, 4, 6, 24, 100, 1000], start=n1, end=n2)
    b = dw.dynamic(tb, deep=2, hclen=19, hlit=286, hdist=30, repeats=False)
    # C: a zero run that starts in the literal/length lengths and ends in the distance lengths
    tc = dw.tokenize(raw, distances=[stride * k for k in range(1, 9)], start=n2)
    cb = dw.dynamic(tc, hlit=286, cross=True, final=True)

    def found(bl):
        assert [x["type"] for x in bl] == [2, 2, 2]
        assert (bl[0]["hclen"], bl[0]["hlit"], bl[0]["hdist"]) == (5, 257, 1)
        assert (bl[1]["hclen"], bl[1]["hlit"], bl[1]["hdist"]) == (19, 286, 30) and not bl[1]["cl_used"] & {16, 17, 18}
        assert bl[1]["cl"][15] and max(bl[1]["ll"]) == 15
        assert bl[2]["cross"] and bl[2]["hlit"] == 286 and not bl[0]["cross"] and not bl[1]["cross"]
        assert len(bl[1]["tokens"]) > 100 and len(dw.matches(bl[1:2])) >= 16 and len(dw.matches(bl[2:])) >= 16
        return ("HCLEN 5 / HLIT 257 / HDIST 1 (HCLEN 4 cannot carry an end-of-block code); HCLEN 19 / HLIT 286 / HDIST 30 "
                f"with {bl[1]['hlit'] + bl[1]['hdist']} lengths sent without 16/17/18; a zero run across the "
                "literal/distance boundary")
    return _finish(name, raw, w, h, c, [a, b, cb], found)


def _len258_alt(name):
    rng = _rng(name)
    w, h, c, stride = 64, 120, 4, 257
    base = _noise_raw(rng, w, 2, c)
    raw = bytearray(base * (h // 2))
    for r in range(2, h, 3):
        raw[r * stride + 5] ^= 0x55  # (breaks the run: not every copy is 258 long)
    toks = dw.tokenize(raw, distances=[2 * stride], only258=True)

    def found(bl):
        m = dw.matches(bl)
        assert len(m) >= 20 and all(t[1] == 258 and t[4] == 284 for t in m) and bl[0]["ll"][284]
        assert len(bl[0]["ll"]) < 286 or not bl[0]["ll"][285]
        return f"{len(m)} matches of length 258, every one as symbol 284 with extra bits 31"
    return _finish(name, raw, w, h, c, _final([dw.dynamic(toks, alt258=True)]), found)


def _stored_edges(name):
    rng = _rng(name)
    w, h, c, stride = 64, 300, 4, 257
    raw = _noise_raw(rng, w, h, c)
    blocks, pos = [], 0
    for phase in range(8):
        # a fixed block from a byte boundary ends at bit 3 + 8 a + 9 b + 7: phase (2 + b) % 8,
        # b = its literals of 144 and more (9-bit codes)
        n = 4
        while (2 + sum(1 for v in raw[pos:pos + n] if v >= 144)) % 8 != phase:
            n += 1
        blocks.append(dw.fixed([int(v) for v in raw[pos:pos + n]]))
        pos += n
        blocks.append(dw.stored(raw[pos:pos + 20]))
        pos += 20
    # the same after a dynamic block: its end phase is whatever it is, the set above holds all 8
    blocks.append(dw.dynamic([int(v) for v in raw[pos:pos + 3000]], dist="none"))
    pos += 3000
    blocks += [dw.stored(b""), dw.stored(raw[pos:pos + 65535])]
    pos += 65535
    blocks.append(dw.stored(b""))
    blocks.append(dw.dynamic([int(v) for v in raw[pos:]], dist="none", final=True))

    def found(bl):
        lens = [b["len"] for b in bl if b["type"] == 0]
        assert 0 in lens and 65535 in lens
        ph = {p["end"] % 8 for p, b in zip(bl, bl[1:]) if b["type"] == 0 and p["type"] != 0}
        assert ph == set(range(8)), ph
        return f"stored lengths {sorted(set(lens))}; stored blocks after coded blocks ending at bit phases {sorted(ph)}"
    return _finish(name, raw, w, h, c, blocks, found)


def _mixed_types(name):
    rng = _rng(name)
    w, h, c, stride = 64, 64, 4, 257
    base = _noise_raw(rng, w, 8, c, levels=64)
    raw = bytearray(base * (h // 8))
    for i in rng.integers(8 * stride, len(raw), 300):
        if int(i) % stride:
            raw[int(i)] = int(rng.integers(0, 64))
    ds = [8 * stride, 16 * stride]
    cuts = [0, 4000, 9000, 12000, len(raw)]
    blocks = [dw.fixed(dw.tokenize(raw, distances=ds, start=0, end=4000)),
              dw.dynamic(dw.tokenize(raw, distances=ds, start=4000, end=9000)),
              dw.stored(raw[9000:12000]),
              dw.dynamic(dw.tokenize(raw, distances=ds, start=12000)),
              dw.fixed([], final=True)]

    def found(bl):
        assert [b["type"] for b in bl] == [1, 2, 0, 2, 1] and bl[4]["n_out"] == 0 and bl[4]["final"]
        assert [b["out"] for b in bl] == cuts
        back = []
        for k, b in enumerate(bl):
            if b["type"] == 0 or not b["tokens"]:
                continue
            o, per = b["out"], collections.Counter()
            for t in b["tokens"]:
                if t[0] == "match":
                    src = o - t[2]
                    if src < b["out"]:
                        per[max(j for j in range(k) if bl[j]["out"] <= src)] += 1
                o += 1 if t[0] == "lit" else t[1]
            back.append(per)
        assert back[1][0] >= 5 and back[2][2] >= 5 and back[2][1] >= 1, back
        return (f"fixed, dynamic, stored, dynamic, empty final fixed; block 2: {back[1][0]} matches from block 1; "
                f"block 4: {back[2][2]} from the stored block, {back[2][1]} from block 2")
    return _finish(name, raw, w, h, c, blocks, found)


def _empty_blocks(name):
    rng = _rng(name)
    w, h, c, stride = 48, 32, 4, 193
    raw = _noise_raw(rng, w, 4, c, levels=100) * 8
    half = 16 * stride
    ds = [4 * stride]
    blocks = [dw.dynamic(dw.tokenize(raw, distances=ds, end=half))]
    pick = rng.integers(0, 2, 600)
    blocks += [dw.stored(b"") if p else dw.fixed([]) for p in pick]
    blocks.append(dw.dynamic(dw.tokenize(raw, distances=ds, start=half), final=True))

    def found(bl):
        mid = bl[1:-1]
        assert len(mid) == 600 and all(b["n_out"] == 0 and not b["final"] for b in mid)
        kinds = collections.Counter(b["type"] for b in mid)
        assert kinds[0] >= 200 and kinds[1] >= 200 and bl[0]["n_out"] and bl[-1]["n_out"] and dw.matches(bl[-1:])
        return f"600 empty blocks in a row ({kinds[0]} stored of length 0, {kinds[1]} fixed with the end-of-block code alone)"
    return _finish(name, raw, w, h, c, blocks, found)


_VALID = {"dist_max": _dist_max, "dist_top": _dist_top, "far_across_lanes": _far_across_lanes,
          "worst_step": lambda n: _worst_step(n, False), "worst_step_lit": lambda n: _worst_step(n, True),
          "all_slow": _all_slow, "pair_beside_slow": _pair_beside_slow, "single_dist": _single_dist,
          "no_dist": _no_dist, "hdr_extremes": _hdr_extremes, "len258_alt": _len258_alt,
          "stored_edges": _stored_edges, "mixed_types": _mixed_types, "empty_blocks": _empty_blocks}
_made = {}


def valid(name):
    if name not in _made:
        _made[name] = _VALID[name](name)
    return _made[name]


# ---- invalid cases: one defect each ----
def _small(name, levels=200):
    rng = _rng(name)
    w, h, c = 40, 30, 4
    return _noise_raw(rng, w, h, c, levels), w, h, c


def _bad_header(name, how):
    """A good dynamic block, a dynamic block whose header has the defect, a good final
    block.  Where the defect allows it the middle block is otherwise whole: its body is
    written with the canonical codes a reader that skipped the check would build, and ends
    with the end-of-block code, so such a reader decodes the stream to the right bytes --
    only the check itself makes it fail.  (The middle block lies inside one row's pixel
    bytes, all 3 or more: its code has no lengths for literals 0, 1 and 2.)"""
    raw, w, h, c = _small(name)
    stride = 1 + w * c
    for i in range(len(raw)):
        if i % stride:
            raw[i] += 3
    a = 15 * stride + 1
    b = a + 150
    mid = [int(v) for v in raw[a:b]]
    first = dw.dynamic([int(v) for v in raw[:a]], dist="none")
    last = dw.dynamic([int(v) for v in raw[b:]], dist="none", final=True)
    good = dw.dynamic(mid, dist="none")
    assert good["ll"][:3] == [0, 0, 0]
    ops = dw._rle(good["ll"] + good["dl"], True)
    if how == "repeat_first":
        # 16 with nothing before it, for the three leading zeros (a reader that takes "the
        # previous length" as 0 reads the same lengths)
        assert ops[0] == (17, 0)
        bad = dw.dynamic(mid, ll=good["ll"], dl=[0], ops=[(16, 0)] + ops[1:])
    elif how == "overrun":
        # the last length (the distance code's one zero) as a run of 138 zeros
        assert ops[-1] == (0, 0)
        bad = dw.dynamic(mid, ll=good["ll"], dl=[0], ops=ops[:-1] + [(18, 127)])
    else:
        ll = list(good["ll"])
        body, eob = mid, True
        if how == "no_eob":  # (a block that cannot end: no reader decodes it)
            ll[256] = 0
            k = [s for s in range(3, 256) if not ll[s]][0]
            ll[k] = good["ll"][256]  # (still a complete code)
            eob = False
        elif how == "over":
            k = max(range(257), key=lambda s: ll[s])
            ll[k] -= 1
            # (the codes past the end of the code space cannot be written: symbols left out)
            top = max(ll)
            over = dw.kraft(ll) - (1 << 15) >> (15 - top)  # codes of the longest length past the end
            lost = set([q for q in range(len(ll)) if ll[q] == top][-over:])
            body, eob = [v for v in mid if v not in lost], 256 not in lost
        else:
            k = min((q for q in range(257) if ll[q]), key=lambda q: ll[q])
            ll[k] += 1
        bad = dw.dynamic(body, ll=ll, dl=[0], check=False, eob=eob)
    return raw, w, h, c, [first, bad, last]


def _invalid(name):
    if name == "far_at_byte_0":
        raw, w, h, c = _small(name)
        return raw, w, h, c, [dw.fixed([(3, 1)] + [int(b) for b in raw[3:]], final=True)]
    if name == "far_before_start":
        # 20000 bytes out, then a copy from 32768 back: 12768 bytes before the stream's first
        rng = _rng(name)
        w, h, c = 255, 160, 1
        raw = _noise_raw(rng, w, h, c)
        assert len(raw) > 40000
        toks = [int(b) for b in raw[:20000]] + [(258, 32768)] + [int(b) for b in raw[20258:]]
        return raw, w, h, c, [dw.dynamic(toks, final=True)]
    if name == "single_dist_unused_code":
        return _single_dist(name, defect=True)
    if name == "no_dist_match":
        return _no_dist(name, defect=True)
    if name == "repeat_first":
        return _bad_header(name, "repeat_first")
    if name == "lengths_overrun":
        return _bad_header(name, "overrun")
    if name == "no_end_of_block":
        return _bad_header(name, "no_eob")
    if name == "oversubscribed":
        return _bad_header(name, "over")
    if name == "incomplete":
        return _bad_header(name, "under")
    raw, w, h, c = _small(name)
    half = len(raw) // 2
    head = [int(b) for b in raw[:half]]
    if name == "length_symbol_286":
        return raw, w, h, c, [dw.fixed(head + [("lsym", 286), ("bits", 0, 13)], final=True)]
    if name == "fixed_distance_30":
        return raw, w, h, c, [dw.fixed(head + [("lsym", 257), ("dsym", 30), ("bits", 0, 13)], final=True)]
    if name == "stored_nlen":
        return raw, w, h, c, [dw.fixed(head), dw.stored(raw[half:], final=True, nlen=(len(raw) - half) ^ 0xFFFE)]
    if name == "btype_3":
        return raw, w, h, c, [dw.fixed(head), {"type": 3, "final": True}]
    raise KeyError(name)


def invalid(name):
    if ("bad", name) not in _made:
        raw, w, h, c, blocks = _invalid(name)
        raw = bytes(raw)
        img = dw.rows_image(raw, w, h, c)
        z = dw.zlib_stream(blocks, raw)
        _made["bad", name] = Bad(name, img, z, dw.png(img, z))
    return _made["bad", name]
