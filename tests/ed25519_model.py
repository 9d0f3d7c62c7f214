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
