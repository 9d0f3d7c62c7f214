"""Integer / hashlib model of the distributed noise (rofl_noise_binomial, include/rofl_zk.h), shared by test_binomial_noise_host.py and
test_gpu_binomial_noise.py.  An f32 enters and leaves as its 32 bits; values are fractions.Fraction (tests/quant_model.py), the stream
comes from hashlib.  The exactness claims of steps 2 and 3 of the definition are asserted on the way: the library computes in double, and
the model checks that nothing it computes there is rounded where the definition says it is not."""
import hashlib
import struct
from fractions import Fraction

import numpy as np

import quant_model as Q
from pq_model import clip

LABEL = b"rofl-zk/noise/v1"
K_MIN, K_MAX = 16, 1 << 20


def block(seed, b):
    """block b of a seed's stream: the first 128 bytes of SHAKE256(label || seed || u64le(b))"""
    seed = bytes(seed)
    assert len(seed) == 32
    return hashlib.shake_256(LABEL + seed + struct.pack("<Q", b)).digest(128)


def word_popcounts(seed, w0, n):
    """popcounts of stream words w0 .. w0 + n - 1 (one hash per block) -> int64 array"""
    b0, b1 = w0 >> 5, (w0 + n + 31) >> 5
    raw = np.frombuffer(b"".join(block(seed, b) for b in range(b0, b1)), np.uint8)
    pc = np.unpackbits(raw).reshape(-1, 32).sum(axis=1).astype(np.int64)      # 32 bits = 4 bytes per little-endian word
    return pc[w0 - 32 * b0: w0 - 32 * b0 + n]


def noise(seed, first, d, k):
    """n_e of element indices first .. first + d - 1 -> int64 array: popcount(words e W .. e W + W - 1) - k, W = k / 16"""
    assert k % 16 == 0 and K_MIN <= k <= K_MAX
    W = k // 16
    assert (first + d) * W <= 1 << 63
    n = word_popcounts(seed, first * W, d * W).reshape(d, W).sum(axis=1) - k
    assert (np.abs(n) <= k).all()
    return n


def _round_f64(x):
    """a Fraction rounded to the nearest double, ties to even, as a Fraction (Python's float() of a Fraction is correctly rounded)"""
    return Fraction(float(x))


def apply_bits(v, n, nb, fb, ff):
    """bits of the output of the value rule for value v (bits or float) and noise integer n"""
    c = clip(v, nb, fb, ff)                                   # step 1
    X = Q.value(c) * (1 << ff)                                # step 2: c 2^frac is exact in double (24 significant bits, a shift), and
    assert _round_f64(X) == X                                 # its rounding to an integer is the float-to-fixed rule: ties to even
    fl = X.numerator // X.denominator
    r = X - fl
    q = fl + (1 if r > Fraction(1, 2) or (r == Fraction(1, 2) and fl & 1) else 0)
    if r == 0:
        assert q == X, "the identity for a value on the grid"
    assert _round_f64(Fraction(q)) == q, "q is an exact double"
    y = _round_f64(Fraction(q + int(n)))                      # step 3: ONE double addition
    if abs(q) < 1 << 52:
        assert y == q + int(n), "the addition is exact below 2^52 steps"
    if fb <= 32:
        assert abs(q) < 1 << 52, "every value of the 8-, 16- and 32-bit formats is below 2^52 steps"
    o = Q.round_f32(y / (1 << ff))                            # step 4: y 2^-frac is exact in double; double -> f32 to nearest even
    if y == 0:
        o = 0                                                 # (+0.0: (double)0 is +0.0, and x + (-x) is +0.0)
    out = clip(o, nb, fb, ff)
    steps = Q.value(out) * (1 << ff)
    assert steps.denominator == 1, "the output is an integer multiple of the grid step"
    return out


def add_noise(vals, seed, k, nb, fb, ff, first=0):
    """rofl_noise_binomial for one vector -> float32 array"""
    vals = np.ascontiguousarray(vals, np.float32)
    ns = noise(seed, first, vals.size, k)
    return np.array([apply_bits(int(b), int(n), nb, fb, ff) for b, n in zip(vals.view(np.uint32), ns)], np.uint32).view(np.float32)


def unsaturated_steps(vals, seed, k, fb, ff, first=0):
    """q + n_e of every element, with q the grid steps of a value ALREADY on the grid and no clip anywhere -> list of int"""
    vals = np.ascontiguousarray(vals, np.float32)
    ns = noise(seed, first, vals.size, k)
    out = []
    for b, n in zip(vals.view(np.uint32), ns):
        X = Q.value(int(b)) * (1 << ff)
        assert X.denominator == 1
        out.append(int(X) + int(n))
    return out


def smallest_k(sigma_steps):
    """the smallest valid k with k / 2 >= sigma^2"""
    s2 = Fraction(sigma_steps) ** 2
    k = K_MIN
    while Fraction(k, 2) < s2:
        k += 16
    return k


def round_seed(secret, round_no):
    return hashlib.sha3_256(b"rofl-zk/noise/v1/round" + bytes(secret) + struct.pack("<Q", int(round_no))).digest()
