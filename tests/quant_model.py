"""Exact model of the float-to-fixed rule (conversion32.rs:11-18 with the runtime formats of fp.rs) and the edge-case corpus for it.

Python integers and fractions.Fraction only: no float arithmetic decides a result.  An f32 enters as its 32 bits (or as a numpy / Python float,
which is converted to those bits at once); its exact value is a Fraction; every rounding -- to the fixed-point integer, to f32 -- is done here on
integers, to nearest with ties to even.  The model and the oracle (tests/orc.py) are the reference of tests/test_quantize_host.py and
tests/test_gpu_quantize.py; the code under test never is."""
import struct
from fractions import Fraction

import numpy as np

L = 2 ** 252 + 27742317777372353535851937790883648493
VALID_FP = [(fb, ff) for fb in (8, 16, 32, 64) for ff in range(13) if ff < fb]      # valid_fp of the library: 47 formats
RANGES = (8, 16, 32, 64)
INF, FLT_MAX, MIN_NORMAL, MIN_SUBNORMAL, SIGN = 0x7f800000, 0x7f7fffff, 0x00800000, 0x00000001, 0x80000000
NAN_BITS = (0x7fc00000, 0xffc00000, 0x7f800001, 0xffffffff)      # quiet, negative quiet, signalling, all ones


def bits_of(v):
    """the 32 bits of an f32 given as bits (int), numpy.float32 or a Python float that holds an f32 value"""
    if isinstance(v, (int, np.integer)):
        return int(v)
    return struct.unpack("<I", struct.pack("<f", float(v)))[0]


def f32(bits):
    return np.array([bits], np.uint32).view(np.float32)[0]


def is_nan(v):
    b = bits_of(v)
    return (b & 0x7fffffff) > INF


def is_inf(v):
    return (bits_of(v) & 0x7fffffff) == INF


def is_neg(v):
    """v < 0: the sign bit of a non-zero, non-NaN value (-0.0 is not negative)"""
    b = bits_of(v)
    return bool(b & SIGN) and 0 < (b & 0x7fffffff) <= INF


def value(v):
    """the exact value of a finite f32"""
    b = bits_of(v)
    e, m = (b >> 23) & 0xff, b & 0x7fffff
    assert e != 0xff, "not finite"
    mag = Fraction(m, 1 << 149) if e == 0 else Fraction((1 << 23) | m) * Fraction(2) ** (e - 150)
    return -mag if b & SIGN else mag


def round_f32(q):
    """bits of the f32 nearest to the Fraction / int q (ties to even; overflow to infinity, gradual underflow), by integer arithmetic"""
    q = Fraction(q)
    sign = SIGN if q < 0 else 0
    q = abs(q)
    if q == 0:
        return sign
    e = q.numerator.bit_length() - q.denominator.bit_length()      # 2^(e-1) < q < 2^(e+1)
    if Fraction(2) ** e > q:
        e -= 1                                                      # 2^e <= q < 2^(e+1)
    e = max(e, -126)
    n = round(q / Fraction(2) ** (e - 23))                          # Fraction.__round__: ties to even; < 2^23 only in the subnormal range
    bits = ((e + 126) << 23) + n                                    # the hidden bit adds 1 to the exponent field; n == 2^24 carries into it
    return sign | min(bits, INF)


def fix_bits(v, fb, ff):
    """Fix::saturating_from_float(|v|).to_bits(): None for NaN (the reference panics: error 10)"""
    if is_nan(v):
        return None
    top = (1 << fb) - 1
    if is_inf(v):
        return top
    return min(round(abs(value(v)) * (1 << ff)), top)


def scalar(v, fb, ff):
    """f32_to_scalar as an integer below l; None for NaN"""
    k = fix_bits(v, fb, ff)
    if k is None:
        return None
    return (-k) % L if is_neg(v) else k


def shifted(v, nb, fb, ff):
    """what create_rangeproof proves for v: read_from_bytes(f32_to_scalar(v) + 2^(nb-1)) (range_proof_vec/mod.rs:36-43, fp.rs)"""
    return ((scalar(v, fb, ff) + (1 << (nb - 1))) % L) & ((1 << fb) - 1)


def _fix_to_f32(k, ff):
    """Fix::from_bits(k).to_float::<f32>() as the oracle restates it: k rounded to f32, then divided by 2^ff (exact)"""
    return round_f32(value(round_f32(k)) / (1 << ff))


def clip_bounds(nb, fb, ff):
    """get_clip_bounds (conversion32.rs:56-60) -> bits of (min, max)"""
    mx = _fix_to_f32(((1 << (nb - 1)) - 1) & ((1 << fb) - 1), ff)
    return mx | SIGN, mx


def l2_clip_bounds(nb, fb, ff):
    return _fix_to_f32(((1 << nb) - 1) & ((1 << fb) - 1), ff)


def l2_term(v, fb, ff):
    """bits of the element's term of the reference's f32 shadow sum (l2_range_proof_vec/mod.rs:37-50): fl(fl(q q) 2^ff), q = fl(k) / 2^ff"""
    k = fix_bits(v, fb, ff)
    qq = round_f32(value(_fix_to_f32(k, ff)) ** 2)
    return qq if qq == INF else round_f32(value(qq) * (1 << ff))


def status(v, nb, fb, ff):
    """1: outside the closed clip range of nb (min > v || v > max: false for NaN), 2: NaN"""
    if is_nan(v):
        return 2
    if is_inf(v):
        return 1
    return int(abs(value(v)) > value(clip_bounds(nb, fb, ff)[1]))


def scalar_bytes(k):
    return np.frombuffer(int(k).to_bytes(32, "little"), np.uint8)


def _neighbours(b):
    """the two f32 next to the finite f32 with bits b (across zero where b is a zero)"""
    mag, s = b & 0x7fffffff, b & SIGN
    return [s | (mag + 1), (s | (mag - 1)) if mag else (s ^ SIGN) | 1]


_CORPUS = {}


def corpus(fb, ff, nb):
    """-> (values f32[n], nans f32[4], in_range f32[..]).  For k around the rounding,
    clip and saturation thresholds, h in {0, +1/2, -1/2} and both signs: the f32 nearest (k + h) / 2^ff and its two neighbours; the zeros, the
    smallest subnormal and normal, FLT_MAX and the infinities; the closed clip bounds of nb and their outward neighbours.  Distinct bit patterns,
    in a fixed order.  NaNs are apart (they are an error); in_range = the values whose status for nb is 0."""
    key = (fb, ff, nb)
    if key in _CORPUS:
        return _CORPUS[key]
    out = []
    for k in (0, 1, 2, 3, 126, 127, 128, (1 << (nb - 1)) - 1, 1 << (nb - 1), (1 << fb) - 2, (1 << fb) - 1, 1 << fb):
        for h in (Fraction(0), Fraction(1, 2), Fraction(-1, 2)):
            if k + h < 0:
                continue
            c = round_f32((k + h) / (1 << ff))
            for b in [c] + _neighbours(c):
                out += [b & ~SIGN & 0xffffffff, b | SIGN]
    for b in (0, MIN_SUBNORMAL, MIN_NORMAL, FLT_MAX, INF):
        out += [b, b | SIGN]
    mx = clip_bounds(nb, fb, ff)[1]
    out += [mx, mx | SIGN, mx + 1, (mx + 1) | SIGN]
    seen, bits = set(), []
    for b in out:
        if b not in seen and not is_nan(b):
            seen.add(b)
            bits.append(b)
    vals = np.array(bits, np.uint32).view(np.float32)
    inr = np.array([b for b in bits if status(b, nb, fb, ff) == 0], np.uint32).view(np.float32)
    _CORPUS[key] = (vals, np.array(NAN_BITS, np.uint32).view(np.float32), inr)
    return _CORPUS[key]


def scalar_to_f32(s, fb, ff):
    """bits of scalar_to_f32 (conversion32.rs:24-35): a scalar whose top byte is not zero is taken as negative"""
    mask = (1 << fb) - 1
    if s >> 248:
        return _fix_to_f32(((-s) % L) & mask, ff) ^ SIGN
    return _fix_to_f32(s & mask, ff)


L2_FORMATS = ((8, 32, 7), (16, 16, 7), (32, 32, 7))      # (prove_range, fp_bits, fp_frac) of the L2 sum-proof vectors


def l2_vectors(nb, fb, ff):
    """vectors of d in {1, 2, 5, 64} from the corpus for create_rangeproof_l2: mostly values with k <= 3 (zeros, ties, subnormals, small
    negatives: the proof exists), and the closed clip bounds, their outward neighbour and NaN alone and inside longer vectors (the errors)"""
    _, nans, inr = corpus(fb, ff, nb)
    small = [v for v in inr if fix_bits(v, fb, ff) <= 3]
    mx_b = clip_bounds(nb, fb, ff)[1]
    mx, out, nan, tie = f32(mx_b), f32(mx_b + 1), nans[0], f32(round_f32(Fraction(3, 2) / (1 << ff)))

    def cyc(d, o=0, **put):
        v = [small[(o + i) % len(small)] for i in range(d)]
        for i, x in put.items():
            v[int(i[1:])] = x
        return np.array(v, np.float32)
    return [cyc(1), cyc(1, 7), cyc(1, _0=tie), cyc(1, _0=-tie), cyc(1, _0=mx), cyc(1, _0=-mx), cyc(1, _0=out), cyc(1, _0=nan),
            cyc(2, 3), cyc(2, _0=tie, _1=-tie), cyc(2, _0=nan, _1=out),
            cyc(5), cyc(5, 11), cyc(5, 2, _2=nan),
            cyc(64), cyc(64, 5), cyc(64, 9, _63=mx)]
