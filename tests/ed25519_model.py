"""Ed25519 as RFC 8032 section 5.1 defines it (no context, no prehash), on Python integers with hashlib.sha512: the reference of
tests/test_ed25519_host.py and tests/test_gpu_ed25519.py.  Points are in extended coordinates; nothing here is fast or constant-time."""
import hashlib

P = 2**255 - 19
L = 2**252 + 27742317777372353535851937790883648493
D = -121665 * pow(121666, P - 2, P) % P
SQRT_M1 = pow(2, (P - 1) // 4, P)
IDENTITY = (0, 1, 1, 0)


def add(p, q):
    """p + q in extended coordinates (X, Y, Z, T), x = X / Z, y = Y / Z, x y = T / Z: the unified addition of a = -1, no inversion"""
    (x1, y1, z1, t1), (x2, y2, z2, t2) = p, q
    a, b, c, d = (y1 - x1) * (y2 - x2), (y1 + x1) * (y2 + x2), 2 * D * t1 * t2, 2 * z1 * z2
    e, f, g, h = b - a, d - c, d + c, b + a
    return (e * f % P, g * h % P, f * g % P, e * h % P)


def mul(k, p):
    r = IDENTITY
    while k:
        if k & 1:
            r = add(r, p)
        p = add(p, p)
        k >>= 1
    return r


def affine(p):
    zi = pow(p[2], P - 2, P)
    return (p[0] * zi % P, p[1] * zi % P)


def point(x, y):
    return (x % P, y % P, 1, x * y % P)


def is_identity(p):
    return p[0] % P == 0 and (p[1] - p[2]) % P == 0


def encode(p):
    x, y = affine(p)
    return (y | ((x & 1) << 255)).to_bytes(32, "little")


def decode(b):
    """The point of 32 bytes, or None where RFC 8032 section 5.1.3 refuses them."""
    v = int.from_bytes(b, "little")
    sign, y = v >> 255, v & (2**255 - 1)
    if y >= P:
        return None
    u, w = (y * y - 1) % P, (D * y * y + 1) % P
    x = u * pow(w, 3, P) * pow(u * pow(w, 7, P), (P - 5) // 8, P) % P
    if (w * x * x - u) % P:
        x = x * SQRT_M1 % P
    if (w * x * x - u) % P or (x == 0 and sign):
        return None
    return point(P - x if (x & 1) != sign else x, y)


B = decode((4 * pow(5, P - 2, P) % P).to_bytes(32, "little"))


def expand(seed):
    h = hashlib.sha512(seed).digest()
    a = int.from_bytes(h[:32], "little") & ((1 << 254) - 8) | (1 << 254)
    return a, h[32:]


def public_key(seed):
    return encode(mul(expand(seed)[0], B))


def sign(seed, msg):
    a, prefix = expand(seed)
    pk = encode(mul(a, B))
    r = int.from_bytes(hashlib.sha512(prefix + msg).digest(), "little") % L
    rb = encode(mul(r, B))
    k = int.from_bytes(hashlib.sha512(rb + pk + msg).digest(), "little") % L
    return rb + ((r + k * a) % L).to_bytes(32, "little")


def verify(pk, msg, sig):
    """The verdict byte of rofl_ed25519_verify: 2 malformed (key refused or of small order, S >= l), 0 the equation holds, 1 it does not."""
    a, s = decode(pk), int.from_bytes(sig[32:], "little")
    if a is None or is_identity(mul(8, a)) or s >= L:
        return 2
    k = int.from_bytes(hashlib.sha512(sig[:32] + pk + msg).digest(), "little") % L
    return 0 if encode(add(mul(s, B), mul(k, point(-a[0], a[1])))) == sig[:32] else 1


# ---------------------------------------------------------------- the corpus the host and the device tests share
# message lengths around every SHA-512 block end: 64 prefix bytes (R || A) spill at 48 and 176, 32 (the key's prefix) at 80 and 208
LENS = (0, 1, 46, 47, 48, 63, 64, 65, 78, 79, 80, 95, 96, 97, 174, 175, 176, 206, 207, 208, 300)


def refused_keys():
    """Every class of key that gives verdict 2, as a list of 32-byte strings: y = p, p + 18, 2^255 - 1 (not canonical), a y with no root,
    y = 1 under the sign bit, and the eight points of small order (the four of order 8 from l * Q of a decodable Q)."""
    enc = lambda y, s=0: (y | s << 255).to_bytes(32, "little")      # noqa: E731
    no_root = next(y for y in range(2, 99) if decode(enc(y)) is None)
    x, y = next(affine(t) for t in (mul(L, decode(enc(y))) for y in range(2, 99) if decode(enc(y))) if not is_identity(mul(4, t)))
    assert is_identity(mul(8, point(x, y)))
    eight = [encode(point(sx * x, sy * y)) for sx in (1, -1) for sy in (1, -1)]
    return [enc(P), enc(P + 18), enc(2**255 - 1), enc(no_root), enc(1, 1), enc(1), enc(P - 1), enc(0), enc(0, 1)] + eight


def verdict_cases(pk, msg, sig):
    """[(key, message, signature, verdict)] from ONE valid triple: itself, every class of 1 (a bit flipped in R, in S below l, in the key
    where it still decodes, in the message), every S >= l and every refused key."""
    flip = lambda b, i: b[:i // 8] + bytes([b[i // 8] ^ 1 << i % 8]) + b[i // 8 + 1:]      # noqa: E731
    s0 = int.from_bytes(sig[32:], "little")
    key_bit = next(i for i in range(256) if decode(flip(pk, i)) and not is_identity(mul(8, decode(flip(pk, i)))))
    ones = [(pk, msg, flip(sig, 3), 1), (pk, msg, flip(sig, 256), 1), (flip(pk, key_bit), msg, sig, 1), (pk, flip(msg, 9), sig, 1)]
    twos = [(pk, msg, sig[:32] + s.to_bytes(32, "little"), 2) for s in (L, L + s0, 2**256 - 1)] + [(k, msg, sig, 2) for k in refused_keys()]
    return [(pk, msg, sig, 0)] + ones + twos


def challenge(r32, pk, msg):
    """k of the signature equation: int_le(SHA-512(R || A || M)) mod l on the bytes as they came"""
    return int.from_bytes(hashlib.sha512(r32 + pk + msg).digest(), "little") % L


def small_order_points():
    """T_0 .. T_7 = i T_1 for the point T_1 of order 8 that refused_keys derives: their orders are 1, 8, 4, 8, 2, 8, 4, 8"""
    t1 = decode(refused_keys()[-4])
    ts = [mul(i, t1) for i in range(8)]
    order = lambda t: next(n for n in (1, 2, 4, 8) if is_identity(mul(n, t)))      # noqa: E731
    assert [order(t) for t in ts] == [1, 8, 4, 8, 2, 8, 4, 8] and len({encode(t) for t in ts}) == 8
    return ts


TORSION_R = 0x0123456789abcdef0123456789abcdef0123456789abcdef0123456789abcdef % L      # the nonce of every hand-built signature: fixed, not secret
TORSION_SIZES = {"a": 28, "b": 7, "c": 2, "d": 3, "e": 3, "f": 38}


def torsion_cases(seed):
    """[(key, message, signature, verdict, tag)] where the exact cofactorless rule of verify() differs from its neighbours: a cofactored check,
    (l - k) A for -k A, a decoded R compared as a point, a hidden refusal of a small-order R.  Signatures are built by hand as
    R || le32(r + k a mod l), k = challenge(R, key, M), never through sign(); a tag is its family's letter and the index within it:
      a<i>  the key A + T_i, i = 1 .. 7 (it decodes and is not of small order: never 2), four messages each, k mod 8 = 0, 4, 2 and odd in that
            order: S B - k (A + T_i) = r B - k T_i, so 0 iff the order of T_i divides k
      b<i>  R = enc(r B + T_i) under A, S from that R's k: 1 (8 times the equation holds)
      c0    r = 0, R = enc(identity): 0, the sum P + (-P) encoded;  c1  R = the non-canonical y = p + 1, the same point: 1, the bytes differ
      d<j>  the key A + T_1, r = 0, R = enc(T_j) where -k T_1 = T_j: 0, for the first three j that a message reaches
      e<n>  S = 0, 1, l - 1 under a good R and A: 1
      f<n>  the key y = p + n // 2 with the sign bit n % 2, every y in p .. 2^255 - 1, under a good signature of A: 2
    Every verdict is asserted against verify(); a walk of the message counter that passes 256 tries raises; no case is left out."""
    ts = small_order_points()
    order = (1, 8, 4, 8, 2, 8, 4, 8)
    a, _ = expand(seed)
    pa = mul(a, B)
    pk, r = encode(pa), TORSION_R
    msg = lambda family, n: b"rofl-zk/ed25519/torsion/" + family + b"/%d" % n      # noqa: E731
    sig = lambda r32, s: r32 + (s % L).to_bytes(32, "little")      # noqa: E731
    r_good = encode(mul(r, B))
    cases = []
    for i in range(1, 8):      # (a)
        key, slots = encode(add(pa, ts[i])), {0: None, 4: None, 2: None, 1: None}
        for n in range(256):
            k = challenge(r_good, key, msg(b"a%d" % i, n))
            slot = 1 if k & 1 else k % 8
            if slot in slots and slots[slot] is None:
                slots[slot] = (key, msg(b"a%d" % i, n), sig(r_good, r + k * a), 0 if k % order[i] == 0 else 1, "a%d" % i)
            if all(slots.values()):
                break
        else:
            raise RuntimeError("torsion_cases: 256 messages did not show k mod 8 = 0, 4, 2 and odd under the key A + T_%d" % i)
        cases += slots.values()
    for i in range(1, 8):      # (b)
        rb = encode(add(mul(r, B), ts[i]))
        cases.append((pk, msg(b"b", i), sig(rb, r + challenge(rb, pk, msg(b"b", i)) * a), 1, "b%d" % i))
    for n, (rb, v) in enumerate(((encode(IDENTITY), 0), ((P + 1).to_bytes(32, "little"), 1))):      # (c)
        cases.append((pk, msg(b"c", n), sig(rb, challenge(rb, pk, msg(b"c", n)) * a), v, "c%d" % n))
    key, found = encode(add(pa, ts[1])), {}      # (d)
    for n in range(256):
        for j in range(8):
            k = challenge(encode(ts[j]), key, msg(b"d", n))
            if j not in found and -k % 8 == j:
                found[j] = (key, msg(b"d", n), sig(encode(ts[j]), k * a), 0, "d%d" % j)
        if len(found) >= 3:
            break
    else:
        raise RuntimeError("torsion_cases: 256 messages did not reach three small-order R under the key A + T_1")
    cases += list(found.values())[:3]
    cases += [(pk, msg(b"e", n), sig(r_good, s), 1, "e%d" % n) for n, s in enumerate((0, 1, L - 1))]      # (e)
    good = sig(r_good, r + challenge(r_good, pk, msg(b"f", 0)) * a)      # (f)
    assert verify(pk, msg(b"f", 0), good) == 0
    cases += [((y | s << 255).to_bytes(32, "little"), msg(b"f", 0), good, 2, "f%d" % (2 * (y - P) + s)) for y in range(P, 2**255) for s in (0, 1)]
    for c in cases:
        assert verify(*c[:3]) == c[3], "torsion_cases: the algebra and verify() differ at " + c[4]
    assert {f: sum(c[4][0] == f for c in cases) for f in TORSION_SIZES} == TORSION_SIZES
    return cases
