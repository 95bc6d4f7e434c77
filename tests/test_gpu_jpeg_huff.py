"""GPU: k_jpeg_huff_enc on chosen coefficients (ik_jpeg_huffman_device), against the
plain Python coder of tests/oracle_jpeg_huff.py (pinned to the C oracle by
tests/test_oracle_jpeg.py).

The kernel's hard cases are set by coefficient values, not pixels, so every field
here is built as coefficients: strips 8 pixels high (nmcu = w / 8), uploaded as
they are.  Every case asserts the length the kernel reports and every byte; a
stream with 2 * nbytes above ik_jpeg_enc_capacity must come back as 0xffffffff
with its output slot untouched.  Where a case claims an edge (a residue, a 0xFF
position, the capacity border) it asserts from the reference's own figures that
the edge was hit.

The kernel gives a thread ceil(blocks / 1024) consecutive blocks, so up to 1024
blocks (341 MCUs) every block is a thread's whole run and every DC difference is
taken across a run boundary."""
import ctypes
import functools

import numpy as np
import pytest

import oracle_jpeg_huff as jh

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5
NO_FIT = 0xFFFFFFFF
THREADS = 1024  # kEncThreads


# ---- fields ([nmcu][3][64] int16, natural order) ----
def zeros(nmcu):
    return np.zeros((nmcu, 3, 64), np.int16)


def put_zz(f, mcu, comp, pos, v):
    f[mcu, comp, jh.ZIGZAG[pos]] = v


def random_field(nmcu, density, seed):
    """density of non-zero coefficients, magnitudes log-uniform in 1..1023"""
    rng = np.random.default_rng(seed)
    mag = np.clip(np.exp(rng.uniform(0.0, np.log(1024.0), (nmcu, 3, 64))).astype(np.int64), 1, 1023)
    sign = rng.integers(0, 2, (nmcu, 3, 64)) * 2 - 1
    return (mag * sign * (rng.random((nmcu, 3, 64)) < density)).astype(np.int16)


def category_value(cat):
    return 0 if cat == 0 else 1 << (cat - 1)


def dense_field(k, nmcu):
    """k MCUs of the dearest blocks baseline can code, then zero MCUs: every AC
    coefficient +-1023 (category 10) and the DC swinging between -1024 and 1023,
    differences of +-2047 (category 11; a swing of +-1024 would make differences
    of 2048, category 12, which the tables cannot code and an FDCT cannot produce:
    the DC of 8-bit samples lies in -1024..1016)."""
    f = zeros(nmcu)
    ac = np.where(np.arange(64) % 2 == 0, 1023, -1023)
    for m in range(k):
        f[m, :, :] = ac
        f[m, :, 0] = -1024 if m % 2 == 0 else 1023
    return f


def stuffing_field(nmcu, cat_a, cat_b):
    """Every block: 1023 at zigzag 16, 32 and 48, i.e. three times the 16-bit code
    1111111111111110 of (run 15, size 10) and ten one-bits of amplitude, runs of 25
    ones.  The last block ends in a 1 at zigzag 63 (no EOB: the stream's last data
    bit is a one); two categories in the first MCU move total_bits."""
    f = zeros(nmcu)
    for pos in (16, 32, 48):
        f[:, :, jh.ZIGZAG[pos]] = 1023
    put_zz(f, nmcu - 1, 2, 63, 1)
    put_zz(f, 0, 0, 1, category_value(cat_a))
    put_zz(f, 0, 1, 1, category_value(cat_b))
    return f


def stuffing_edges(ref):
    """the four things the stuffing case must contain, from the reference's figures"""
    ff = set(ref.ff)
    bp = -(-ref.nbytes // THREADS)
    return {
        "consecutive": sorted(i for i in ff if i + 1 in ff),
        "thread_border": sorted(t for t in range(1, THREADS) if t * bp in ff and t * bp - 1 in ff),
        "last_byte": ref.nbytes - 1 in ff and ref.total_bits % 8 == 1,
        "count": len(ff),
        "bp": bp,
    }


@functools.lru_cache(maxsize=None)
def stuffing_case(nmcu):
    for a in range(11):
        for b in range(11):
            f = stuffing_field(nmcu, a, b)
            ref = jh.code(f)
            e = stuffing_edges(ref)
            if e["bp"] >= 2 and e["consecutive"] and e["thread_border"] and e["last_byte"] and e["count"] >= 64:
                return f, ref, e
    raise AssertionError("no stuffing field has all four edges")


@functools.lru_cache(maxsize=None)
def residue_cases(nmcu=6):
    """One field per value of total_bits & 31: a sparse base, the category of one
    luma coefficient and of one coefficient of the trailing block varied."""
    base = random_field(nmcu, 0.05, seed=77)
    found = {}
    for a in range(11):
        for b in range(11):
            f = base.copy()
            put_zz(f, 2, 0, 1, category_value(a))
            put_zz(f, nmcu - 1, 2, 1, -category_value(b))
            ref = jh.code(f)
            found.setdefault(ref.total_bits & 31, (f, ref))
    return found


# ---- the kernel ----
def run_kernel(ik, fields, stride_pad=0):
    """One launch over same-size fields -> (lengths, output slots, capacity).  The
    slots hold SENTINEL before the call; the padding between images holds values no
    table can code."""
    from imagekit import _lib
    n, nmcu = len(fields), fields[0].shape[0]
    w, h, per = 8 * nmcu, 8, fields[0].size
    stride = per + stride_pad
    host = np.full(n * stride, 0x7ABC, np.int16)
    for i, f in enumerate(fields):
        assert f.shape == (nmcu, 3, 64) and f.dtype == np.int16
        host[i * stride:i * stride + per] = f.reshape(-1)
    cap = ik.ik_jpeg_enc_capacity(w, h)
    out = np.full(n * cap, SENTINEL, np.uint8)
    lens = np.zeros(n, np.uint32)
    d = ctypes.c_void_p()
    assert ik.ik_dev_alloc(host.nbytes, ctypes.byref(d)) == 0
    try:
        assert ik.ik_memcpy_h2d(d, host.ctypes.data, host.nbytes) == 0
        rc = ik.ik_jpeg_huffman_device(d, stride, n, w, h, out.ctypes.data, lens.ctypes.data)
        assert rc == 0, _lib.last_error()
    finally:
        ik.ik_dev_free(d)
    return lens, out.reshape(n, cap), cap


def check(ik, fields, refs=None, stride_pad=0):
    """Every image's length and bytes against the reference; what lies past the
    kernel's last 16-byte store, and the whole slot of a stream that does not fit,
    must still hold the sentinel.  Returns which images were coded."""
    refs = refs or [jh.code(f) for f in fields]
    lens, slots, cap = run_kernel(ik, fields, stride_pad)
    coded = []
    for i, ref in enumerate(refs):
        fits = 2 * ref.nbytes <= cap
        coded.append(fits)
        if not fits:
            assert lens[i] == NO_FIT, f"image {i}: {ref.nbytes} unstuffed bytes do not fit {cap}, got length {lens[i]}"
            assert (slots[i] == SENTINEL).all(), f"image {i}: a stream that does not fit wrote into its slot"
            continue
        assert lens[i] == len(ref.data), f"image {i}: length {lens[i]}, reference {len(ref.data)} ({ref.total_bits} bits)"
        got = slots[i, :lens[i]].tobytes()
        if got != ref.data:
            at = next(k for k in range(len(got)) if got[k] != ref.data[k])
            raise AssertionError(f"image {i}: first difference at byte {at} of {len(got)}: "
                                 f"{got[at:at + 8].hex()} != {ref.data[at:at + 8].hex()}")
        tail = slots[i, (int(lens[i]) + 15) // 16 * 16:]
        assert (tail == SENTINEL).all(), f"image {i}: wrote past its last 16-byte store"
    return coded


# ---- thread partition ----
@pytest.mark.parametrize("kind", ["zero", "sparse"])
@pytest.mark.parametrize("nmcu", [1, 2, 341, 342, 683])
def test_thread_partition(ik, nmcu, kind):
    """3, 6, 1023, 1026 and 2049 blocks: one, two and three blocks per thread, with
    trailing threads that own nothing.  All-zero blocks cost 6 (Y) and 4 (chroma)
    bits, so several threads' runs share each 32-bit word."""
    f = zeros(nmcu) if kind == "zero" else random_field(nmcu, 0.02, seed=nmcu)
    ref = jh.code(f)
    if kind == "zero":
        assert ref.total_bits == nmcu * (6 + 4 + 4)
    assert check(ik, [f], [ref]) == [True]


# ---- zero runs ----
@pytest.mark.parametrize("pos", [1, 15, 16, 17, 32, 33, 48, 49, 62, 63])
def test_single_coefficient_after_a_zero_run(ik, pos):
    """One non-zero AC coefficient per block: runs of exactly 15 (no ZRL) and 16 (one),
    two and three ZRL codes, and position 63, after which no EOB is written."""
    f = zeros(4)
    put_zz(f, 0, 0, pos, 1)
    put_zz(f, 1, 1, pos, -2)
    put_zz(f, 2, 2, pos, 5)
    for c, v in enumerate((-1, 3, -7)):
        put_zz(f, 3, c, pos, v)
    ref = jh.code(f)
    # the field's cost, counted by hand from the rules: an EOB unless pos is 63,
    # (pos - 1) // 16 ZRL codes, the (run, size) code and the amplitude bits
    want = 0
    for m, c, v in ((0, 0, 1), (1, 1, -2), (2, 2, 5), (3, 0, -1), (3, 1, 3), (3, 2, -7)):
        size = abs(v).bit_length()
        want += (jh.code_of("ac", c, 0xF0)[1] * ((pos - 1) // 16) + jh.code_of("ac", c, ((pos - 1) % 16) << 4 | size)[1]
                 + size - (jh.code_of("ac", c, 0)[1] if pos == 63 else 0))
    assert ref.total_bits == want + 4 * (6 + 4 + 4)
    assert check(ik, [f], [ref]) == [True]


# ---- magnitudes ----
AC_VALUES = sorted({s * v for k in range(10) for v in ((1 << (k + 1)) - 1, 1 << k) for s in (1, -1)})
# consecutive MCUs' DCs: differences 0, 0, 1, -1, 1023, -1023, -1, 1024, -1024, -1023, 2047, -2047, 1024
DC_VALUES = [0, 0, 1, 0, 1023, 0, -1, 1023, -1, -1024, 1023, -1024, 0]


@pytest.mark.parametrize("repeat", [1, 9])
def test_magnitudes_at_every_category_border(ik, repeat):
    """AC +-(2^k - 1) and +-2^k for k = 0..9 and +-1023 (categories 1..10, negative
    amplitudes at each power of two), DC differences 0, +-1, +-1023, +-1024 and +-2047
    (category 11).  38 MCUs are 114 blocks, a block per thread: every DC difference
    crosses a run boundary; repeated 9 times (1026 blocks, two per thread) half of
    them lie inside a run."""
    assert {1023, -1023, 512, -512, 511, -511, 1, -1} <= set(AC_VALUES) and len(AC_VALUES) == 38
    d = np.diff(np.array([0] + DC_VALUES))
    assert {0, 1, -1, 1023, -1023, 1024, -1024, 2047, -2047} <= set(d.tolist())
    nmcu = len(AC_VALUES)
    f = zeros(nmcu)
    for m, v in enumerate(AC_VALUES):
        put_zz(f, m, 0, 1 + m % 5, v)
        put_zz(f, m, 1, 2, -v)
        put_zz(f, m, 2, 63, v)
        for c in range(3):
            f[m, c, 0] = DC_VALUES[(m + 4 * c) % len(DC_VALUES)]
    f = np.tile(f, (repeat, 1, 1))
    assert check(ik, [f]) == [True]


# ---- pad and word residues ----
def test_every_residue_of_total_bits(ik):
    """total_bits & 31 takes every value 0..31 (so the seven pad bits start at every
    bit of a word, cross into the next word from 26 on, and are dropped whole when
    total_bits % 8 == 0); the 32 fields go through one launch."""
    cases = residue_cases()
    assert sorted(cases) == list(range(32)), f"residues produced: {sorted(cases)}"
    fields = [cases[r][0] for r in range(32)]
    refs = [cases[r][1] for r in range(32)]
    assert [r.total_bits & 31 for r in refs] == list(range(32))
    assert {r.total_bits % 8 for r in refs} == set(range(8))
    assert all(check(ik, fields, refs))


# ---- stuffing ----
def test_stuffing_at_thread_borders_and_the_last_byte(ik):
    f, ref, e = stuffing_case(48)
    # void unless the reference shows all four: consecutive 0xFF bytes, a 0xFF on both
    # sides of a stuffing thread's first byte (thread t owns bytes [t*bp, (t+1)*bp)),
    # a final 0xFF made of one data bit and the pad, and 64 or more 0xFF in all (the
    # scan of the counts carries across waves)
    assert e["bp"] >= 2 and e["consecutive"] and e["thread_border"] and e["last_byte"] and e["count"] >= 64, e
    assert check(ik, [f], [ref]) == [True]


# ---- capacity border ----
@functools.lru_cache(maxsize=None)
def capacity_border():
    """(k, unstuffed bytes) of the dense strips of k MCUs around 2 * nbytes == capacity;
    the capacity of a strip of k MCUs is ik_jpeg_enc_cap's 3 * w * h + 4096 rounded up to 16"""
    sizes = {}
    for k in range(1, 12):
        sizes[k] = jh.code(dense_field(k, k)).nbytes
        if 2 * sizes[k] > (3 * 8 * k * 8 + 4096 + 15) // 16 * 16:
            return (k - 1, sizes[k - 1]), (k, sizes[k])
    raise AssertionError("dense strips never passed the capacity")


def test_capacity_border(ik):
    (k_fit, b_fit), (k_over, b_over) = capacity_border()
    assert k_fit >= 1 and k_over == k_fit + 1
    for k, nbytes, fits in ((k_fit, b_fit, True), (k_over, b_over, False)):
        cap = ik.ik_jpeg_enc_capacity(8 * k, 8)
        assert (2 * nbytes <= cap) == fits, (k, nbytes, cap)
        assert check(ik, [dense_field(k, k)]) == [fits]


# ---- batch ----
def test_batch_with_an_overflowing_image_between_coded_ones(ik):
    """Five images in one launch, their coefficients a padded stride apart as
    jpeg_front_group lays them out: zero, sparse, one that does not fit, the stuffing
    field, one MCU of data.  The neighbours of the one that does not fit are coded."""
    nmcu = 48
    stuffed, stuffed_ref, _ = stuffing_case(nmcu)
    one = zeros(nmcu)
    one[0] = random_field(1, 1.0, seed=5)[0]
    fields = [zeros(nmcu), random_field(nmcu, 0.03, seed=11), dense_field(16, nmcu), stuffed, one]
    assert check(ik, fields, stride_pad=128) == [True, True, False, True, True]


# ---- seeded sweep ----
SWEEP_DENSITY = [0.01, 0.1, 0.5, 1.0]
SWEEP_NMCU = [5, 9, 64, 171, 400]


@functools.lru_cache(maxsize=None)
def sweep_case(seed):
    f = random_field(SWEEP_NMCU[seed % 5], SWEEP_DENSITY[seed % 4], seed=1000 + seed)
    return f, jh.code(f)


@pytest.mark.parametrize("seed", range(20))
def test_seeded_sweep(ik, seed):
    """Every pairing of four densities and five strip lengths; the dense long ones do
    not fit and are checked as such."""
    f, ref = sweep_case(seed)
    check(ik, [f], [ref])


def test_seeded_sweep_has_both_outcomes(ik):
    fits = [2 * sweep_case(s)[1].nbytes <= ik.ik_jpeg_enc_capacity(8 * sweep_case(s)[0].shape[0], 8) for s in range(20)]
    assert 4 <= sum(fits) <= 16, fits


# ---- arguments ----
def test_misaligned_coefficients_are_refused(ik):
    d = ctypes.c_void_p()
    assert ik.ik_dev_alloc(4 * 192 * 2 + 64, ctypes.byref(d)) == 0
    try:
        cap = ik.ik_jpeg_enc_capacity(8, 8)
        out = np.zeros(2 * cap, np.uint8)
        lens = np.zeros(2, np.uint32)
        # a base that is not 16-byte aligned, a stride that is no multiple of 8: IK_ERR_INVALID, no launch
        assert ik.ik_jpeg_huffman_device(d.value + 2, 192, 1, 8, 8, out.ctypes.data, lens.ctypes.data) == 2
        assert ik.ik_jpeg_huffman_device(d, 192 + 4, 2, 8, 8, out.ctypes.data, lens.ctypes.data) == 2
    finally:
        ik.ik_dev_free(d)
