"""Integer / hashlib model of the discrete Gaussian noise (rofl_noise_dgauss, include/rofl_zk.h), shared by test_dgauss_noise_host.py and
test_gpu_dgauss_noise.py: the sampler of Canonne, Kamath and Steinke (2020) on a per-element stream of SHAKE256 words, in Python integers,
with the bounds the library's 64-bit arithmetic relies on asserted on the way.  The sampler also runs on a caller-supplied word list.
The value rule is the one of the binomial noise (tests/noise_model.py apply_bits)."""
import hashlib
import math
import struct
from fractions import Fraction

import numpy as np

import noise_model as NM

LABEL = b"rofl-zk/dgaus/v1"
S2_MAX = 1 << 24
STREAM_BLOCKS, STREAM_WORDS = 256, 8192
FIRST_MAX = 1 << 55


class Exhausted(Exception):
    """a draw past the last word: the element's noise is 0 (the full stream) / the sampler is not finished (a shorter list)"""


def block(seed, e, j):
    """block j of element index e: the first 128 bytes of SHAKE256(label || seed || u64le(e << 8 | j))"""
    seed = bytes(seed)
    assert len(seed) == 32 and 0 <= j < STREAM_BLOCKS and 0 <= e < FIRST_MAX
    return hashlib.shake_256(LABEL + seed + struct.pack("<Q", (e << 8) | j)).digest(128)


class _Words:
    """used: the words handed out; mark: the word at which the running attempt began (sample() sets it); span: the most blocks any
    attempt reached past the one it began in -- what decides whether a ring of R blocks holds every attempt (span < R); attempts: the
    passes of the rejection loop begun"""
    used = mark = span = attempts = 0

    def _took(self):
        self.span = max(self.span, (self.used >> 5) - (self.mark >> 5))
        self.used += 1


class ListWords(_Words):
    """the stream of a word list: words in order, Exhausted past the end"""
    def __init__(self, words):
        self.words = words

    def next(self):
        if self.used >= len(self.words) or self.used >= STREAM_WORDS:
            raise Exhausted()
        w = int(self.words[self.used])
        self._took()
        return w


class SeedWords(_Words):
    """the stream of element index e of a seed: blocks hashed on demand"""
    def __init__(self, seed, e):
        self.seed, self.e, self.blk, self.cur = seed, e, None, -1

    def next(self):
        if self.used >= STREAM_WORDS:
            raise Exhausted()
        if self.used >> 5 != self.cur:
            self.cur = self.used >> 5
            self.blk = struct.unpack("<32I", block(self.seed, self.e, self.cur))
        w = self.blk[self.used & 31]
        self._took()
        return w


def _below(st, D):
    assert 1 <= D < 1 << 64
    b = (D - 1).bit_length()
    if b == 0:
        return 0
    while True:
        v = st.next()
        if b > 32:
            v |= st.next() << 32
        v &= (1 << b) - 1
        if v < D:
            return v


def _frac(st, n, D):
    assert 0 <= n <= D
    K = 1
    while True:
        assert K <= STREAM_WORDS and D * K < 1 << 63
        if not _below(st, D * K) < n:
            return K & 1
        K += 1


def _expo(st, n, D):
    f = n // D
    for _ in range(f):
        if _frac(st, 1, 1) == 0:
            return 0
    return _frac(st, n - f * D, D)


def sample(st, s2):
    """-> the noise integer; raises Exhausted when the stream ends first.  st.used: the words consumed"""
    assert 1 <= s2 <= S2_MAX
    t = math.isqrt(s2) + 1
    assert 2 * s2 * t * t < 1 << 50
    while True:
        st.mark = st.used
        st.attempts += 1
        U = _below(st, t)
        if _frac(st, U, t) == 0:
            continue
        V = 0
        while V < 64 and _frac(st, 1, 1) == 1:
            V += 1
        if V == 64:
            continue
        X = U + t * V
        assert X <= 64 * t - 1 <= 262207
        B = st.next() & 1
        if B == 1 and X == 0:
            continue
        a = X * t - s2
        assert abs(a) <= 64 * t * t < 1 << 31 and a * a < 1 << 62
        if _expo(st, a * a, 2 * s2 * t * t) == 0:
            continue
        return -X if B else X


def on_words(words, s2):
    """the sampler over a caller's list -> (finished, noise, words used); not finished: it asked for a word past the list (or past word
    8 191), the noise is then 0 and `used` the words it had read"""
    st = ListWords(words)
    try:
        return True, sample(st, s2), st.used
    except Exhausted:
        return False, 0, st.used


def element(seed, e, s2, span=False):
    """-> (noise, words used) of element index e; span=True: -> (noise, words used, the widest attempt's span in blocks)"""
    st = SeedWords(seed, e)
    try:
        n = sample(st, s2)
    except Exhausted:
        n = 0
    return (n, st.used, st.span) if span else (n, st.used)


def noise(seed, first, d, s2):
    assert first + d <= FIRST_MAX
    return np.array([element(seed, first + i, s2)[0] for i in range(d)], np.int64)


def attempts_and_words(seed, first, d, s2):
    """-> (attempts, words) of each element: the passes of the rejection loop it begins and the stream words it consumes -> two int arrays"""
    a, w = np.zeros(d, np.int64), np.zeros(d, np.int64)
    for i in range(d):
        st = SeedWords(seed, first + i)
        try:
            sample(st, s2)
        except Exhausted:
            pass
        a[i], w[i] = st.attempts, st.used
    return a, w


def blocks_used(seed, first, d, s2):
    """XOF blocks each element needs -> int array"""
    return np.array([(element(seed, first + i, s2)[1] + 31) >> 5 for i in range(d)], np.int64)


def uses_two_word_draws(s2):
    """whether step 4's denominator exceeds 32 bits, so that below() takes two words per draw"""
    t = math.isqrt(s2) + 1
    return 2 * s2 * t * t > 1 << 32


def add_noise(vals, seed, s2, nb, fb, ff, first=0, ns=None):
    """rofl_noise_dgauss for one vector -> float32 array (ns: the noise integers, when the caller has them already)"""
    vals = np.ascontiguousarray(vals, np.float32)
    if ns is None:
        ns = noise(seed, first, vals.size, s2)
    return np.array([NM.apply_bits(int(b), int(n), nb, fb, ff) for b, n in zip(vals.view(np.uint32), ns)], np.uint32).view(np.float32)


def pmf(s2, lo, hi):
    """exact probabilities of the discrete Gaussian of variance parameter s2 on lo .. hi (floats from a sum over +-40 sigma)"""
    r = int(40 * math.sqrt(s2)) + 40
    z = sum(math.exp(-x * x / (2.0 * s2)) for x in range(-r, r + 1))
    return {x: math.exp(-x * x / (2.0 * s2)) / z for x in range(lo, hi + 1)}


def smallest_sigma2(sigma_steps):
    """the smallest integer sigma2 >= sigma_steps^2, at least 1"""
    s2 = Fraction(sigma_steps) ** 2
    return max(1, -((-s2.numerator) // s2.denominator))


def chi2(ns, s2):
    """chi-square of noise integers against the exact pmf: values whose expected count is at least 20 are single cells, the rest one
    pooled cell -> (chi2, cells)"""
    N = len(ns)
    r = int(12 * math.sqrt(s2)) + 12
    single = {x: N * q for x, q in pmf(s2, -r, r).items() if N * q >= 20}
    vals, counts = np.unique(np.asarray(ns, np.int64), return_counts=True)
    seen = dict(zip(vals.tolist(), counts.tolist()))
    pool = N - sum(single.values())
    rest = N - sum(seen.get(x, 0) for x in single)
    return sum((seen.get(x, 0) - ex) ** 2 / ex for x, ex in single.items()) + (rest - pool) ** 2 / pool, len(single) + 1


def golden():
    """what tests/golden/dgauss.json holds (python tests/dgauss_model.py rewrites it; about a minute)"""
    seed = bytes(range(32))
    out = {"noise": {}, "words_used": {}, "ring_overruns": {}, "chi2": {}}
    for s2, first, n in ((4096, 0, 32), (1, 0, 32), (1 << 24, 1 << 40, 16), (2, 0, 16), (3, 5, 16), (15, 0, 16), (16, 0, 16), (1 << 16, (1 << 40) + 3, 16), (1 << 24, 0, 16), (50, (1 << 55) - 16, 16)):
        out["noise"]["%d:%d" % (s2, first)] = noise(seed, first, n, s2).tolist()
    for s2, e in ((4096, 7), (4096, 3565), (4096, 9406), (1 << 24, 11567)):
        out["words_used"]["%d:%d" % (s2, e)] = element(seed, e, s2)[1]
    out["ring_overruns"][str(1 << 24)] = [e for e in range(20000) if element(seed, e, 1 << 24, True)[2] >= 2]
    for s2 in (1, 2, 9, 50):
        out["chi2"][str(s2)] = round(chi2(noise(seed, 0, 65536, s2), s2)[0], 4)
    total = sum(noise(hashlib.sha3_256(bytes([k])).digest(), 0, 8192, 9) for k in range(8)).astype(np.float64)
    out["closure_variance"] = round(float(((total - total.mean()) ** 2).mean()), 4)
    return out


if __name__ == "__main__":
    import json
    import os
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dgauss.json")
    json.dump(golden(), open(path, "w"), indent=1, sort_keys=True)
    print(path)
