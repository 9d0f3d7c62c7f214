"""Integer / hashlib model of the probabilistic quantization (rofl_quantize_prob, include/rofl_zk.h), shared by test_prob_quant_host.py and
test_gpu_prob_quant.py.  An f32 enters and leaves as its 32 bits; values are fractions.Fraction (tests/quant_model.py), the stream comes
from hashlib.  The exactness claims of the definition are asserted on the way: the library computes in double, and the model checks that
nothing it computes there is ever rounded."""
import hashlib
import struct
from fractions import Fraction

import numpy as np

import quant_model as Q

LABEL = b"rofl-zk/quant/v1"


def block(seed, b):
    """block b of a seed's stream: the first 128 bytes of SHAKE256(label || seed || u64le(b))"""
    seed = bytes(seed)
    assert len(seed) == 32
    return hashlib.shake_256(LABEL + seed + struct.pack("<Q", b)).digest(128)


def word(seed, e):
    """the u32 word of element index e: little-endian word e & 31 of block e >> 5"""
    return struct.unpack_from("<I", block(seed, e >> 5), 4 * (e & 31))[0]


def words(seed, first, d):
    """words first .. first + d - 1 (one hash per block)"""
    out, cache = [], {}
    for e in range(first, first + d):
        if e >> 5 not in cache:
            cache[e >> 5] = struct.unpack("<32I", block(seed, e >> 5))
        out.append(cache[e >> 5][e & 31])
    return out


def clip(v, nb, fb, ff):
    """bits of what rofl_clip_f32 returns for v: fminf(max, fmaxf(min, v)) -- NaN goes to min; -0.0 stays -0.0"""
    mn, mx = Q.clip_bounds(nb, fb, ff)
    b = Q.bits_of(v)
    if Q.is_nan(b):
        c = mn
    elif Q.is_inf(b):
        c = mn if b & Q.SIGN else b
    else:
        c = mn if Q.value(mn) >= Q.value(b) else b
    if Q.is_inf(c) or Q.value(mx) <= Q.value(c):
        c = mx
    return c


def threshold(v, nb, fb, ff):
    """-> (c bits, f, t) of steps 1 and 2, with the exactness claims asserted"""
    c = clip(v, nb, fb, ff)
    x = abs(Q.value(c)) * (1 << ff)
    f = x.numerator // x.denominator
    r = x - f
    # exact in double: x and f are integers times a power of two with at most 24 significant bits, r is a part of x's bits
    assert x.denominator & (x.denominator - 1) == 0 and x.numerator.bit_length() <= 24 + (x.numerator & -x.numerator).bit_length() - 1
    assert r.numerator.bit_length() <= 24 and f < 1 << 64
    if r > 0:
        assert x < 1 << 23, "a value with a fractional part is below 2^23 grid steps"
        assert (r * (1 << 32)).denominator == 1 or r < Fraction(1, 1 << 8), "r 2^32 is an integer unless the value is far below one step"
    t = (r * (1 << 32)).numerator // (r * (1 << 32)).denominator
    assert 0 <= t < 1 << 32
    return c, f, t


def steps(v, w, nb, fb, ff):
    """k' of step 3: the number of grid steps of the output's magnitude"""
    _, f, t = threshold(v, nb, fb, ff)
    return f + (1 if w < t else 0)


def round_bits(v, w, nb, fb, ff):
    """bits of the output for value v (bits or float) and stream word w"""
    c, f, t = threshold(v, nb, fb, ff)
    k = f + (1 if w < t else 0)
    mag = Fraction(k, 1 << ff)
    out = Q.round_f32(mag)
    assert Q.value(out) == mag, "the output is an exact f32"
    assert mag <= Q.value(Q.clip_bounds(nb, fb, ff)[1]), "rounding up never leaves the clip range"
    if abs(Q.value(c)) * (1 << ff) == f:
        assert out == c & 0x7fffffff, "a value on the grid comes back unchanged"
    return out | (c & Q.SIGN)


def quantize(vals, seed, nb, fb, ff, first=0):
    """rofl_quantize_prob for one vector -> float32 array"""
    vals = np.ascontiguousarray(vals, np.float32)
    bits = vals.view(np.uint32)
    ws = words(seed, first, vals.size)
    return np.array([round_bits(int(b), w, nb, fb, ff) for b, w in zip(bits, ws)], np.uint32).view(np.float32)


_CORPUS = {}


def corpus(fb, ff, nb):
    """-> (value bits, words) of the rounding cases of one format: the float-to-fixed corpus (grid values, ties, the f32 on each side of
    them, zeros, subnormals, infinities, both closed clip bounds and their neighbours on both sides), the NaNs, quarter and three-quarter
    steps -- each with the words t - 1 (rounds up; left out where t = 0), t (rounds down), 0 and 0xffffffff"""
    key = (fb, ff, nb)
    if key not in _CORPUS:
        vals, nans, _ = Q.corpus(fb, ff, nb)
        mx = Q.clip_bounds(nb, fb, ff)[1]
        bits = [int(b) for b in vals.view(np.uint32)] + [int(b) for b in nans.view(np.uint32)] + [mx - 1, (mx - 1) | Q.SIGN]
        for k in (0, 1, 5):
            for h in (Fraction(1, 4), Fraction(3, 4)):
                b = Q.round_f32((k + h) / (1 << ff))
                bits += [b, b | Q.SIGN]
        vb, ws = [], []
        for b in dict.fromkeys(bits):
            t = threshold(b, nb, fb, ff)[2]
            for w in dict.fromkeys(([t - 1] if t else []) + [t, 0, 0xffffffff]):
                vb.append(b)
                ws.append(w)
        _CORPUS[key] = (np.array(vb, np.uint32), np.array(ws, np.uint32))
    return _CORPUS[key]


def corpus_expected(fb, ff, nb):
    vb, ws = corpus(fb, ff, nb)
    return np.array([round_bits(int(b), int(w), nb, fb, ff) for b, w in zip(vb, ws)], np.uint32)


def round_seed(secret, round_no):
    return hashlib.sha3_256(b"rofl-zk/quant/v1/round" + bytes(secret) + struct.pack("<Q", int(round_no))).digest()
