"""The blur and unsharpen definition restated in numpy, independent of
the library: expf comes from the process's libm through ctypes (the glibc function the
library's host code calls), sqrtf through np.float32 (IEEE-exact).  Every product and sum is
one float32 operation, in ascending tap order."""
import ctypes
import ctypes.util

import numpy as np

F = np.float32
_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.expf.restype = ctypes.c_float
_libm.expf.argtypes = [ctypes.c_float]
PI = F(3.14159265358979323846264338327950288)
MIN_SIGMA, MAX_SIGMA = 0.0625, 32.0


def gaussian(x, sigma):
    x, sigma = F(x), F(sigma)
    cst = F(1.0) / (np.sqrt(F(2.0) * PI) * sigma)
    return cst * F(_libm.expf(-(x * x) / (F(2.0) * (sigma * sigma))))


def axis_weights(L, sigma):
    """(left, count, weights) of an axis of L samples: int arrays of L and an (L, T) float32
    array, zero from count on; T is the taps of the widest output."""
    sigma = F(sigma)
    support = F(2.0) * sigma
    left, count, rows = np.zeros(L, np.int64), np.zeros(L, np.int64), []
    cache = {}  # the weights depend on the offsets only, and these are small exact integers
    for o in range(L):
        c = F(o) + F(0.5)
        l = min(max(int(np.floor(c - support)), 0), L - 1)
        r = min(max(int(np.ceil(c + support)), l + 1), L)
        c = c - F(0.5)
        ws = []
        total = F(0.0)
        for i in range(l, r):
            x = F(i) - c
            key = float(x)
            if key not in cache:
                cache[key] = gaussian(x, sigma)
            ws.append(cache[key])
            total = total + cache[key]
        rows.append([w / total for w in ws])
        left[o], count[o] = l, r - l
    T = int(count.max())
    w = np.zeros((L, T), F)
    for o in range(L):
        w[o, :count[o]] = rows[o]
    return left, count, w


def _pass(a, left, count, w):
    """One pass along axis 0 of the float32 array a: out[o] = sum over ascending k of
    a[left[o] + k] * w[o, k], one float32 multiply and one float32 add per tap.  The taps
    past count[o] are gathered from a clipped index and not added."""
    L = a.shape[0]
    assert a.dtype == F and len(left) == L
    t = np.zeros_like(a)
    shape = (L,) + (1,) * (a.ndim - 1)
    for k in range(w.shape[1]):
        live = (k < count).reshape(shape)
        prod = a[np.minimum(left + k, L - 1)] * w[:, k].reshape(shape)
        t = np.where(live, t + prod, t)
    return t


def blur(img, sigma):
    """img (H, W) or (H, W, C), uint8 or uint16 -> the same shape and dtype"""
    M = 255 if img.dtype == np.uint8 else 65535
    assert img.dtype in (np.uint8, np.uint16)
    H, W = img.shape[:2]
    v = _pass(img.astype(F), *axis_weights(H, sigma))              # vertical, f32, nothing rounded
    h = _pass(np.swapaxes(v, 0, 1).copy(), *axis_weights(W, sigma))  # horizontal over it
    t = np.clip(np.swapaxes(h, 0, 1), F(0), F(M))
    fl = np.floor(t)  # t >= 0: halves away from zero go up; t - floor(t) is exact, t + 0.5 would not be
    return (fl + (t - fl >= F(0.5))).astype(img.dtype)


def unsharpen(img, sigma, threshold):
    M = 255 if img.dtype == np.uint8 else 65535
    return unsharpen_rule(img, blur(img, sigma), threshold, M)


def unsharpen_rule(S, B, threshold, M):
    S64, B64 = S.astype(np.int64), B.astype(np.int64)
    d = S64 - B64
    return np.where(np.abs(d) > threshold, np.clip(S64 + d, 0, M), S64).astype(S.dtype)
