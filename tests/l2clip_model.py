"""Integer / hashlib model of the norm clipping (rofl_clip_l2, include/rofl_zk.h), shared by test_l2_clip_host.py and test_gpu_l2_clip.py.
An f32 enters and leaves as its 32 bits; step counts are Python integers, the stream comes from hashlib.  The scale is found by an integer
square root, not by the library's 32-step search, and the consequences the header states are asserted on the way."""
import hashlib
import math
import struct
from fractions import Fraction

import numpy as np

import noise_model as N
import quant_model as Q
from pq_model import clip

LABEL = b"rofl-zk/clip2/v1"
ONE = 1 << 32      # scale_out of a vector that fits


def block(seed, b):
    """block b of a seed's stream: the first 128 bytes of SHAKE256(label || seed || u64le(b))"""
    seed = bytes(seed)
    assert len(seed) == 32
    return hashlib.shake_256(LABEL + seed + struct.pack("<Q", b)).digest(128)


def words(seed, d):
    """word(0) .. word(d - 1): little-endian word i & 31 of block i >> 5"""
    raw = b"".join(block(seed, b) for b in range((d + 31) >> 5))
    return list(struct.unpack("<%dI" % (len(raw) // 4), raw))[:d]


def steps(v, nb, fb, ff):
    """step 1 -> (bits of c, q): the clip of rofl_clip_f32, then the saturating float-to-fixed rule of |c|"""
    c = clip(v, nb, fb, ff)
    return c, Q.fix_bits(c, fb, ff)


def steps_of(vals, nb, fb, ff):
    """q of every element of a float32 array -> list of int"""
    return [steps(int(b), nb, fb, ff)[1] for b in np.ascontiguousarray(vals, np.float32).view(np.uint32)]


def sum_sq(vals, nb, fb, ff):
    return sum(q * q for q in steps_of(vals, nb, fb, ff))


def ceil_sqrt(d):
    return math.isqrt(d - 1) + 1 if d else 0


def budget(T, d, seeded):
    """Te of step 4; None for the seeded r < 0 (the call returns 11)"""
    if not seeded:
        return T
    r = math.isqrt(T) - ceil_sqrt(d)
    return None if r < 0 else r * r


def scale(S, Te):
    """the largest m below 2^32 with m^2 S <= 2^64 Te"""
    m = min(math.isqrt((Te << 64) // S), ONE - 1)
    assert m * m * S <= Te << 64 and (m == ONE - 1 or (m + 1) ** 2 * S > Te << 64)
    return m


def trunc24(k):
    return k if k < 1 << 24 else k >> (k.bit_length() - 24) << (k.bit_length() - 24)


def round_steps(q, m, w=None):
    """k' of one element from its steps, the scale and its stream word (None: no seeds)"""
    y = q * m
    assert y < 1 << 96
    k = (y >> 32) + (1 if w is not None and w < (y & (ONE - 1)) else 0)
    kk = trunc24(k)
    assert kk <= k <= q, "no magnitude grows: m <= 2^32 - 1"
    return kk


def out_bits(kk, c, ff):
    mag = Fraction(kk, 1 << ff)
    b = Q.round_f32(mag)
    assert Q.value(b) == mag, "the output is an exact f32"
    return b | (c & Q.SIGN) if kk else 0


def clip_l2(vals, T, nb, fb, ff, seed=None, stream=None):
    """rofl_clip_l2 for one vector -> (float32 array, scale_out, k' list or None for a vector that fits).  stream: words to use instead of
    the seed's (a test of the bound under words nobody would draw)"""
    vals = np.ascontiguousarray(vals, np.float32)
    bits = [int(b) for b in vals.view(np.uint32)]
    cq = [steps(b, nb, fb, ff) for b in bits]
    S = sum(q * q for _, q in cq)
    assert S < len(bits) << 128 or not bits
    if S <= T:
        return np.array([N.apply_bits(b, 0, nb, fb, ff) for b in bits], np.uint32).view(np.float32), ONE, None
    seeded = seed is not None or stream is not None
    Te = budget(T, len(bits), seeded)
    assert Te is not None
    m = scale(S, Te)
    ws = (stream if stream is not None else words(seed, len(bits))) if seeded else [None] * len(bits)
    ks = [round_steps(q, m, w) for (_, q), w in zip(cq, ws)]
    assert sum(k * k for k in ks) <= T, "the bound of the definition"
    mx = Q.value(Q.clip_bounds(nb, fb, ff)[1])
    assert all(Fraction(k, 1 << ff) <= mx for k in ks), "inside the clip range"
    return np.array([out_bits(k, c, ff) for k, (c, _) in zip(ks, cq)], np.uint32).view(np.float32), m, ks


def norm_budget(l2_range, fb, ff, reserve_steps=0):
    B = ((1 << l2_range) - 1) & ((1 << fb) - 1)
    r = math.isqrt(B) - reserve_steps
    assert r >= 0
    return r * r


def round_seed(secret, round_no):
    return hashlib.sha3_256(b"rofl-zk/clip2/v1/round" + bytes(secret) + struct.pack("<Q", int(round_no))).digest()
