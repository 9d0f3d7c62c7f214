"""A labelled corpus of 32-byte strings for the Ristretto255 decoders -- the inputs of tests/test_ristretto_corpus_host.py (CPU: pyref, the
oracle and the two host builds of the codec agree on every entry) and tests/test_gpu_decode_sites.py (GPU: every production entry point
that decodes a point reports a refusal the way include/rofl_zk.h documents).

A decoder refuses an encoding for one of five reasons (RFC 9496 4.3.1), the first two read off the bytes, the other three only after the
square-root chain has run: the bytes are not the canonical encoding of a field element (bit 255 set, or s >= p), s is odd, SQRT_RATIO_M1
finds no square, t is negative, y is zero.  classify() walks those steps with big integers (tests/golden/pyref.py) and names the FIRST that
refuses:

    bit255        bit 255 of the string is set (what remains may be a valid encoding)
    noncanon      s >= p
    negative      s is odd
    nonsquare     v u2^2 is a non-zero non-square
    nonsquare_v0  v u2^2 is zero: SQRT_RATIO_M1 is asked for 1 / 0 (s = +-sqrt(-1), where u2 = 1 + s^2 = 0)
    tneg          t = x y is odd
    y0            y = 0 (s = p - 1 alone: u1 = 1 - s^2 = 0)
    valid         none of them

corpus() is a fixed list of (name, bytes32, class): the hand-picked members of every class, the valid edges, and 512 random even canonical
s from a fixed seed, which fall into nonsquare / tneg / valid at about 2 : 1 : 1.  Nothing here needs a GPU or the product library; the
tuples handed out are shared between tests and never changed."""
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import pyref  # noqa: E402

P = pyref.P
N_RANDOM = 512
SEED = 9496
CLASS_FLOOR = 64      # members of each of nonsquare, tneg, valid among the random entries (4 000 draws of pyref split 49 % / 26 % / 25 %)
INVALID_CLASSES = ("bit255", "noncanon", "negative", "nonsquare", "nonsquare_v0", "tneg", "y0")
CLASSES = INVALID_CLASSES + ("valid",)
# where a test puts a bad entry in a vector of 257: the block edges of the 64- and 256-thread kernels and of those with two threads per element
POSITIONS = (0, 63, 64, 127, 128, 255, 256)
D = 257


def enc(s):
    return int(s).to_bytes(32, "little")


def classify(b):
    """the first step of RFC 9496 4.3.1 that refuses the 32 bytes b, or "valid" """
    b = bytes(b)
    assert len(b) == 32
    if b[31] & 0x80:
        return "bit255"
    s = int.from_bytes(b, "little")
    if s >= P:
        return "noncanon"
    if s & 1:
        return "negative"
    ss = s * s % P
    u1, u2 = (1 - ss) % P, (1 + ss) % P
    u2s = u2 * u2 % P
    v = (-(pyref.D * u1 % P * u1) - u2s) % P
    was_square, invsqrt = pyref.sqrt_ratio_m1(1, v * u2s % P)
    if not was_square:
        return "nonsquare_v0" if v * u2s % P == 0 else "nonsquare"
    den_x = invsqrt * u2 % P
    den_y = invsqrt * den_x % P * v % P
    x = pyref.fabs(2 * s * den_x % P)
    y = u1 * den_y % P
    if pyref.is_neg(x * y % P):
        return "tneg"
    if y == 0:
        return "y0"
    return "valid"


def _smallest_valid():
    s = 2
    while classify(enc(s)) != "valid":
        s += 2
    return s


def _even_sqrt_m1():
    r = pyref.SQRT_M1
    assert r * r % P == P - 1
    return r if r % 2 == 0 else P - r


@functools.lru_cache(maxsize=None)
def corpus():
    """((name, bytes32, class), ...), the same on every call"""
    base = [pyref.ristretto_encode(pyref.pt_mul(k, pyref.BASE)) for k in range(1, 17)]
    s1, s2 = (int.from_bytes(b, "little") for b in base[:2])
    out = []

    def add(name, b, want):
        got = classify(b)
        assert got == want, (name, got, want)
        out.append((name, bytes(b), got))
    # p + 1 and p + 17 are even strings, so the parity check lets them through; p + 3 is the one that ONLY the canonical check refuses: a
    # decoder that reduces it computes with s = 3, which gives what s = p - 3 (valid) gives, since everything but |x| reads s^2 -- while
    # p + 1 reduces to s = 1, refused once more at y = 0, and p + 17 to a non-square
    for name, s in (("p", P), ("p+1", P + 1), ("p+2", P + 2), ("p+3", P + 3), ("p+17", P + 17), ("2^255-1", 2 ** 255 - 1)):
        add(name, enc(s), "noncanon")
    assert P + 17 == 2 ** 255 - 2 and (P + 1) % 2 == 0 and (P + 3) % 2 == 0
    add("B|bit255", enc(s1 | 1 << 255), "bit255")
    add("2B|bit255", enc(s2 | 1 << 255), "bit255")
    for name, s in (("1", 1), ("p-2", P - 2), ("p-s(B)", P - s1), ("p-s(2B)", P - s2)):
        add(name, enc(s), "negative")
    add("p-1", enc(P - 1), "y0")
    add("sqrt(-1)", enc(_even_sqrt_m1()), "nonsquare_v0")
    add("0", enc(0), "valid")
    add("p-3", enc(P - 3), "valid")
    add("smallest", enc(_smallest_valid()), "valid")
    for k, b in enumerate(base, start=1):
        add("%dB" % k, b, "valid")
    rng = np.random.default_rng(SEED)
    half = (P + 1) // 2
    for i in range(N_RANDOM):
        s = 2 * (int.from_bytes(rng.integers(0, 256, 32, dtype=np.uint8).tobytes(), "little") % half)      # even, canonical
        b = enc(s)
        c = classify(b)
        assert c in ("nonsquare", "tneg", "valid"), (i, c)      # (the other classes have measure zero among even canonical s)
        out.append(("random%d" % i, b, c))
    for c in ("nonsquare", "tneg", "valid"):
        n = sum(1 for name, _, k in out if k == c and name.startswith("random"))
        assert n >= CLASS_FLOOR, (c, n)
    assert len({b for _, b, _ in out}) == len(out)
    return tuple(out)


def of_class(cls):
    return [e for e in corpus() if e[2] == cls]


@functools.lru_cache(maxsize=None)
def representatives():
    """one entry of each invalid class, in the order of INVALID_CLASSES: each is refused by its own check ALONE (p + 3 is even and reduces
    to a valid s, the bit-255 entry is valid below that bit, p - s(B) is canonical and its negative is valid)"""
    by_name = {e[0]: e for e in corpus()}
    reps = [by_name["B|bit255"], by_name["p+3"], by_name["p-s(B)"], of_class("nonsquare")[0], by_name["sqrt(-1)"], of_class("tneg")[0], by_name["p-1"]]
    assert tuple(e[2] for e in reps) == INVALID_CLASSES
    return tuple(reps)


@functools.lru_cache(maxsize=None)
def valid_edges():
    """the hand-picked valid entries: 0 (the identity), p - 3, the smallest non-zero valid s, B .. 16 B"""
    return tuple(e for e in corpus() if e[2] == "valid" and not e[0].startswith("random"))


@functools.lru_cache(maxsize=None)
def valid_pool():
    """every valid entry but the identity, as a read-only uint8[n, 32]: what honest vectors are filled with"""
    a = as_array([b for n, b, c in corpus() if c == "valid" and n != "0"])
    a.setflags(write=False)
    return a


def as_array(encodings):
    """uint8[n, 32] (a fresh, writable array) of a list of 32-byte strings or corpus entries"""
    bs = [e[1] if isinstance(e, tuple) else bytes(e) for e in encodings]
    return np.frombuffer(b"".join(bs), np.uint8).reshape(-1, 32).copy()


def row(entry):
    return np.frombuffer(entry[1], np.uint8)


def honest_points(n, offset=0):
    """uint8[n, 32] of valid non-identity encodings, cycling through the corpus's from `offset` (fresh, writable)"""
    pool = valid_pool()
    return pool[(np.arange(n) + offset) % len(pool)].copy()


def pyref_add(a, b):
    """encode(decode(a) + decode(b)) by pyref, for two valid encodings"""
    return pyref.ristretto_encode(pyref.pt_add(pyref.ristretto_decode(a), pyref.ristretto_decode(b)))
