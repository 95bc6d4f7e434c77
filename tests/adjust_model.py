"""The colour adjustment of DESIGN section 4 restated in numpy and plain Python floats, apart
from the library: cos, sin and pow come from the process's libm through ctypes (the glibc
functions the library's host code calls), never from the library.  plan() is the host half
(the Q16 matrix, the tone table, the flags), apply() the device half (integers only)."""
import ctypes
import ctypes.util
import math

import numpy as np

_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
for _f, _n in (("cos", 1), ("sin", 1), ("pow", 2)):
    getattr(_libm, _f).restype = ctypes.c_double
    getattr(_libm, _f).argtypes = [ctypes.c_double] * _n

L = (0.2126, 0.7152, 0.0722)
S = ((-L[0], -L[1], 1.0 - L[2]), (0.143, 0.140, -0.283), (-(1.0 - L[0]), L[1], L[2]))
PI = 3.141592653589793
FLAG_MATRIX, FLAG_TABLE = 1, 2


def real_matrix(saturation=0, hue=0):
    """m = Hue . Sat in float64, each operation rounded once, in the order of the definition."""
    s = 1.0 + float(saturation) / 100.0
    th = float(hue) * PI / 180.0
    c, sn = _libm.cos(th), _libm.sin(th)
    sat = [[0.0] * 3 for _ in range(3)]
    hu = [[0.0] * 3 for _ in range(3)]
    for i in range(3):
        for j in range(3):
            d = (1.0 if i == j else 0.0) - L[j]
            sat[i][j] = L[j] + s * d
            hu[i][j] = (L[j] + c * d) + sn * S[i][j]
    return [[(hu[i][0] * sat[0][j] + hu[i][1] * sat[1][j]) + hu[i][2] * sat[2][j] for j in range(3)] for i in range(3)]


def matrix(saturation=0, hue=0):
    """The Q16 matrix as a (3, 3) int64 array: off the diagonal floor(m * 65536 + 0.5), on it
    65536 minus the row's other two."""
    m = real_matrix(saturation, hue)
    q = np.zeros((3, 3), np.int64)
    for i in range(3):
        for j in range(3):
            if i != j:
                q[i, j] = math.floor(m[i][j] * 65536.0 + 0.5)
        q[i, i] = 65536 - (int(q[i].sum()) - int(q[i, i]))
    return q


def table(depth, brightness=0, contrast=0, gamma=0.0, invert=0):
    """The tone table T[0..M] as a uint16 array."""
    M = 255 if depth == 1 else 65535
    g = float(np.float32(gamma))  # the field is an f32
    b = float(brightness) / 100.0
    k0 = float(100 + contrast) / 100.0
    k = k0 * k0
    e = 1.0 / g if g != 0.0 else 0.0
    # (float64 arrays: each numpy operation below rounds once, as the scalar one does)
    x = np.arange(M + 1, dtype=np.float64) / float(M)
    x = x + b
    x = (x - 0.5) * k + 0.5
    x = np.clip(x, 0.0, 1.0)
    if g != 0.0:
        x = np.array([_libm.pow(v, e) for v in x.tolist()], np.float64)
    if invert:
        x = 1.0 - x
    return np.floor(x * float(M) + 0.5).astype(np.uint16)


def plan(depth, brightness=0, contrast=0, saturation=0, hue=0, gamma=0.0, invert=0):
    """(matrix, table, flags) of one adjustment at one depth."""
    q = matrix(saturation, hue)
    t = table(depth, brightness, contrast, gamma, invert)
    flags = (FLAG_MATRIX if not np.array_equal(q, 65536 * np.eye(3, dtype=np.int64)) else 0) | (
        FLAG_TABLE if not np.array_equal(t, np.arange(t.size, dtype=np.uint16)) else 0)
    return q, t, flags


def apply_plan(px, q, t, flags):
    """The device half on an (..., C) uint8 or uint16 array: the matrix on three colour samples
    (C >= 3 only), then the table on every colour sample; alpha as it was."""
    M = 255 if px.dtype == np.uint8 else 65535
    C = px.shape[-1]
    cc = 1 if C <= 2 else 3
    out = px.copy()
    col = px[..., :cc].astype(np.int64)
    if (flags & FLAG_MATRIX) and cc == 3:
        acc = np.einsum("ij,...j->...i", q, col) + 32768
        col = np.clip(acc >> 16, 0, M)  # numpy's >> on int64 is arithmetic
    if flags & FLAG_TABLE:
        col = t[col].astype(np.int64)
    out[..., :cc] = col.astype(px.dtype)
    return out


def apply(px, **kw):
    """px under the adjustment kw (plan()'s keyword arguments)."""
    q, t, flags = plan(px.dtype.itemsize, **kw)
    return apply_plan(px, q, t, flags)


_PLANS = {}


def cached_plan(depth, **kw):
    """plan(), computed once per (depth, parameters): the 16-bit tables take 65536 pow calls."""
    key = (depth,) + tuple(sorted(kw.items()))
    if key not in _PLANS:
        _PLANS[key] = plan(depth, **kw)
    return _PLANS[key]
