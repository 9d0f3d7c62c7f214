"""Python model of the randomized Hadamard rotation (rofl_rotate; the definition is in include/rofl_zk.h): NumPy float32 and hashlib, the
stage-by-stage network vectorised over the elements.  Every step is one IEEE binary32 operation, so the model, the library's host route
and its kernels are held to the same BYTES, not to a tolerance.  `exact` is the float64 transform of the same signs; check_bounds holds the
model itself to the error bounds the header states."""
import hashlib
import struct

import numpy as np

LABEL = b"rofl-zk/rotate/v1"
LIM = np.float32(2.0 ** 100)
HALF_SQRT2 = np.array([0x3F3504F3], np.uint32).view(np.float32)[0]


def rotated_len(d, k):
    return -(-d >> k) << k


def sign_bits(seed, n):
    """s_e for e < n: bit e & 31 of little-endian u32 word (e >> 5) & 31 of stream block e >> 10"""
    nblk = (n + 1023) >> 10
    stream = b"".join(hashlib.shake_256(LABEL + bytes(seed) + struct.pack("<Q", b)).digest(128) for b in range(nblk))
    words = np.frombuffer(stream, "<u4")
    e = np.arange(n, dtype=np.int64)
    return ((words[e >> 5] >> (e & 31).astype(np.uint32)) & 1).astype(np.uint32)


def scale(k):
    c = np.float32(2.0 ** -(k // 2))
    return c if k % 2 == 0 else np.float32(np.float32(2.0 ** -((k - 1) // 2)) * HALF_SQRT2)      # (a power of two times one float: exact)


def clamp(x):
    x = np.asarray(x, np.float32)
    with np.errstate(invalid="ignore"):
        z = np.where(np.isnan(x) | (x <= -LIM), -LIM, x)
        return np.where(z >= LIM, LIM, z).astype(np.float32)


def flip(z, bits):
    return (z.view(np.uint32) ^ (bits.astype(np.uint32) << np.uint32(31))).view(np.float32)


def butterflies(z, k):
    """k stages over blocks of 2^k elements, h = 1, 2, 4, ...: one float32 addition or subtraction per element and stage"""
    z = z.copy()
    h = 1
    while h < (1 << k):
        v = z.reshape(-1, 2, h)
        a, b = v[:, 0, :].copy(), v[:, 1, :].copy()
        v[:, 0, :] = a + b
        v[:, 1, :] = a - b
        h *= 2
    return z


def rotate(x, seed, k, inverse=False):
    """-> float32[rotated_len(d, k)]; the inverse takes whole blocks"""
    x = np.ascontiguousarray(x, np.float32).reshape(-1)
    dp = rotated_len(x.size, k)
    assert not inverse or dp == x.size
    z = np.zeros(dp, np.float32)
    z[:x.size] = x
    z = clamp(z)
    s = sign_bits(seed, dp)
    if not inverse:
        z = flip(z, s)
    z = butterflies(z, k)
    z = (z * scale(k)).astype(np.float32)
    if inverse:
        z = flip(z, s)
    return z


def exact(x, seed, k, inverse=False):
    """the same transform of the clamped input in float64 with the exact scale 2^(-k/2)"""
    x = np.ascontiguousarray(x, np.float32).reshape(-1)
    dp = rotated_len(x.size, k)
    z = np.zeros(dp, np.float64)
    z[:x.size] = clamp(x).astype(np.float64)
    sg = 1.0 - 2.0 * sign_bits(seed, dp).astype(np.float64)
    if not inverse:
        z = z * sg
    h = 1
    while h < (1 << k):
        v = z.reshape(-1, 2, h)
        a, b = v[:, 0, :].copy(), v[:, 1, :].copy()
        v[:, 0, :] = a + b
        v[:, 1, :] = a - b
        h *= 2
    z = z * 2.0 ** (-k / 2.0)
    return z * sg if inverse else z


def check_bounds(x, seed, k):
    """the model's own claims on a finite input whose butterflies stay normal: forward error <= (k + 2) 2^-24 ||x||, round trip
    <= (2k + 4) 2^-24 ||x||.  -> (forward error, round-trip error) as fractions of their bounds"""
    x = np.ascontiguousarray(x, np.float32).reshape(-1)
    nx = float(np.linalg.norm(clamp(x).astype(np.float64)))
    y = rotate(x, seed, k)
    fe = float(np.linalg.norm(y.astype(np.float64) - exact(x, seed, k)))
    back = rotate(y, seed, k, inverse=True)[:x.size]
    re = float(np.linalg.norm(back.astype(np.float64) - clamp(x).astype(np.float64)))
    fb, rb = (k + 2) * 2.0 ** -24 * nx, (2 * k + 4) * 2.0 ** -24 * nx
    assert fe <= fb and re <= rb, (k, fe, fb, re, rb)
    return (fe / fb if fb else 0.0), (re / rb if rb else 0.0)
