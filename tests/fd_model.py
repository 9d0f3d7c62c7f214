"""Exact model of the kernels' field, point and scalar arithmetic (csrc/fe26.hpp, csrc/quad26.hpp, the sc_* of csrc/fe32.hpp) in plain
Python integers, the corpus that pins the header's limb-bound contract at its extremes, and the checks shared by test_fd_arith_host.py and
test_gpu_fd_arith.py.  No C, no oracle.

Two models of every op of the table in csrc/fd_dbg.hpp (numbering and layout: include/rofl_zk_debug.h):
  * the VALUE model: the value of a limb vector is sum v_i 2^ceil(25.5 i) mod p, and every op is its polynomial (or RFC 9496 4.2 for
    sqrt_ratio) evaluated mod p -- `expect(op, case)`;
  * the LIMB model: the same steps as the header, limb by limb, in unbounded integers, raising BoundError on any u32 / u64 wrap and any
    violated precondition of the header's contract -- `limbs(op, case)`.  It proves that a corpus case lies inside the contract before any
    library code sees it, and it predicts the library's output limbs exactly."""
import random

P = 2 ** 255 - 19
L = 2 ** 252 + 27742317777372353535851937790883648493
R = 2 ** 256
RINV = pow(R, -1, L)
SHIFT = [0, 26, 51, 77, 102, 128, 153, 179, 204, 230]
M = [(1 << 26) - 1 if i % 2 == 0 else (1 << 25) - 1 for i in range(10)]          # FD_M26 / FD_M25
TIGHT = [(1 << 26) + (1 << 19) if i % 2 == 0 else (1 << 25) + (1 << 19) for i in range(10)]      # exclusive
SUB_BIAS = [0x7ffffda] + [0x3fffffe if i % 2 else 0x7fffffe for i in range(1, 10)]                 # 2p in this radix
MUL_F_MAX = (1 << 28) + (1 << 20)          # exclusive bound of fd_mul's first operand (the assertion of the host build)
G19_MAX = (2 ** 32 - 1) // 19              # largest limb g with 19 g < 2^32
G38_MAX = (2 ** 32 - 1) // 38
CARRY_MAX = 2 ** 32 - 2 ** 26              # fd_carry: any limbs below this
SQRTM1 = pow(2, (P - 1) // 4, P)
D = (-121665 * pow(121666, -1, P)) % P
D2 = 2 * D % P
D2_LIMBS = [0x2b2f159, 0x1a6e509, 0x22add7a, 0x0d4141d, 0x0038052, 0x0f3d130, 0x3407977, 0x19ce331, 0x1c56dff, 0x0901b67]

FD_IN, FD_OUT, SC_IN, SC_OUT = 80, 80, 264, 8
(UNPACK, CARRY, PACK, ADD, SUB, NEG, MUL, SQ, MUL_LOOSE, SQ_LOOSE, INVERT, POW22523, SQRT_RATIO, ABS, PRED, MADD, MSUB, GD_ADD, GD_DOUBLE,
 GD_DOUBLE_NOT, TO_NIELS, TO_NIELS_ZINV, GQ_DOUBLE, GQ_ADD) = range(24)
FD_OP_NAMES = ["unpack", "carry", "pack", "add", "sub", "neg", "mul", "sq", "mul_loose", "sq_loose", "invert", "pow22523", "sqrt_ratio", "abs",
               "pred", "madd", "msub", "gd_add", "gd_double", "gd_double_not", "to_niels", "to_niels_zinv", "gq_double", "gq_add"]
FD_THREAD_OPS = list(range(22))
(SC_MONTMUL, SC_TO_MONT, SC_FROM_MONT, SC_MUL_PLAIN, SC_ADD, SC_NEG, SC_SUB, SC_LOAD_REDUCED, SC_FROM_WIDE, SC_FROM_WIDE_MONT, SC_MAC,
 SC_INVERT_MONT) = range(12)
SC_OP_NAMES = ["montmul", "to_mont", "from_mont", "mul_plain", "add", "neg", "sub", "load_reduced", "from_wide", "from_wide_mont", "mac", "invert_mont"]


class BoundError(Exception):
    """a u32 / u64 wrap or a violated precondition of the header's contract"""


def _u32(x, what):
    if not 0 <= x < 2 ** 32:
        raise BoundError("u32 wrap in " + what)
    return x


def _u64(x, what):
    if not 0 <= x < 2 ** 64:
        raise BoundError("u64 wrap in " + what)
    return x


def value(v):
    return sum(x << s for x, s in zip(v, SHIFT)) % P


def is_tight(v):
    return all(0 <= x < t for x, t in zip(v, TIGHT))


def from_int(x):
    """the limbs of 0 <= x < 2^255, each below 2^26 / 2^25 (x >= p gives a non-canonical representation)"""
    assert 0 <= x < 2 ** 255
    return [(x >> SHIFT[i]) & M[i] for i in range(10)]


# ---------------------------------------------------------------- limb model (fe26.hpp step by step)
def l_unpack(w):
    x = sum(int(w[i]) << (32 * i) for i in range(8))
    r = [(x >> SHIFT[i]) & M[i] for i in range(10)]
    r[0] = _u32(r[0] + 19 * (x >> 255), "fd_unpack")
    return r


def l_carry(a):
    if not all(0 <= x < CARRY_MAX for x in a):
        raise BoundError("fd_carry operand >= 2^32 - 2^26")
    r = list(a)
    for i in range(9):
        c = r[i] >> (26 if i % 2 == 0 else 25); r[i] &= M[i]; r[i + 1] = _u32(r[i + 1] + c, "fd_carry")
    c = r[9] >> 25; r[9] &= M[9]; r[0] = _u32(r[0] + 19 * c, "fd_carry")
    c = r[0] >> 26; r[0] &= M[0]; r[1] = _u32(r[1] + c, "fd_carry")
    return r


def l_pack(a):
    """-> the integer of the 8 words (fd_pack); the sum below is what the 64-bit accumulator chain adds up"""
    t = l_carry(a)
    x = sum(v << s for v, s in zip(t, SHIFT))
    if x >> 256:
        raise BoundError("fd_pack value >= 2^256")
    return x


def l_add(a, b):
    return [_u32(x + y, "fd_add") for x, y in zip(a, b)]


def l_sub(a, b):
    if not is_tight(b):
        raise BoundError("fd_sub subtrahend not tight")
    return [_u32(_u32(x + k, "fd_sub") - y, "fd_sub") for x, y, k in zip(a, b, SUB_BIAS)]


def l_neg(a):
    return l_sub([0] * 10, a)


def l_reduce_cols(h):
    h = list(h)

    def carry(i, j):
        sh = 26 if i % 2 == 0 else 25
        c = h[i] >> sh
        h[j] = _u64(h[j] + (c * 19 if i == 9 else c), "fd_reduce_cols")
        h[i] &= (1 << sh) - 1
    for i, j in ((0, 1), (4, 5), (1, 2), (5, 6), (2, 3), (6, 7), (3, 4), (7, 8), (4, 5), (8, 9), (9, 0), (0, 1)):
        carry(i, j)
    return [_u32(x, "fd_reduce_cols result") for x in h]


def l_mul(f, g):
    if not all(0 <= x < MUL_F_MAX for x in f):
        raise BoundError("fd_mul first operand >= 2^28 + 2^20")
    if not all(0 <= 19 * x < 2 ** 32 for x in g):
        raise BoundError("fd_mul second operand: 19 g >= 2^32")
    f2 = [_u32(2 * f[i], "fd_mul 2f") if i % 2 else f[i] for i in range(10)]
    g19 = [19 * x for x in g]
    h = [0] * 10
    for i in range(10):
        fi, fi2 = f[i], f2[i]
        for j in range(10):
            k = i + j
            a = fi2 if (j & 1) else fi           # both indices odd: the doubled limb
            if k >= 10:
                h[k - 10] += a * g19[j]
            else:
                h[k] += a * g[j]
    for x in h:
        _u64(x, "fd_mul column")
    return l_reduce_cols(h)


def l_sq(f):
    if not all(0 <= x * (38 if i % 2 else 19) < 2 ** 32 for i, x in enumerate(f)):
        raise BoundError("fd_sq operand: 19 f (even limb) or 38 f (odd limb) >= 2^32")
    h = [0] * 10
    for i in range(10):
        for j in range(10):
            k = i + j
            t = f[i] * f[j] * (2 if (i & 1) and (j & 1) else 1)
            if k >= 10:
                h[k - 10] += 19 * t
            else:
                h[k] += t
    for x in h:
        _u64(x, "fd_sq column")
    return l_reduce_cols(h)


def l_sqn(a, n):
    for _ in range(n):
        a = l_sq(a)
    return a


def _l_pow_2_250_1(z):
    z2 = l_sq(z)
    z9 = l_mul(l_sqn(z2, 2), z)
    z11 = l_mul(z9, z2)
    z_5_0 = l_mul(l_sq(z11), z9)
    z_10_0 = l_mul(l_sqn(z_5_0, 5), z_5_0)
    z_20_0 = l_mul(l_sqn(z_10_0, 10), z_10_0)
    z_40_0 = l_mul(l_sqn(z_20_0, 20), z_20_0)
    z_50_0 = l_mul(l_sqn(z_40_0, 10), z_10_0)
    z_100_0 = l_mul(l_sqn(z_50_0, 50), z_50_0)
    z_200_0 = l_mul(l_sqn(z_100_0, 100), z_100_0)
    return l_mul(l_sqn(z_200_0, 50), z_50_0), z11


def l_invert(z):
    t, z11 = _l_pow_2_250_1(z)
    return l_mul(l_sqn(t, 5), z11)


def l_pow22523(z):
    t, _ = _l_pow_2_250_1(z)
    return l_mul(l_sqn(t, 2), z)


def l_isneg(a):
    return (l_pack(a) % P) & 1


def l_iszero(a):
    return int(l_pack(a) % P == 0)


def l_eq(a, b):
    return int((l_pack(a) - l_pack(b)) % P == 0)


def l_abs(a):
    t = l_carry(a)
    return l_carry(l_neg(t)) if l_isneg(t) else t


def l_sqrt_ratio(u, v):
    sqrtm1 = from_int(SQRTM1)
    v3 = l_mul(l_sq(v), v)
    v7 = l_mul(l_sq(v3), v)
    r = l_mul(l_mul(u, v3), l_pow22523(l_mul(u, v7)))
    check = l_mul(v, l_sq(r))
    neg_u = l_carry(l_neg(u))
    correct, flipped = l_eq(check, u), l_eq(check, neg_u)
    flipped_i = l_eq(check, l_mul(neg_u, sqrtm1))
    r_prime = l_mul(r, sqrtm1)
    if flipped or flipped_i:
        r = r_prime
    return l_abs(r), int(bool(correct or flipped))


def l_madd(p, q, neg):
    X, Y, Z, T = p
    ypx, ymx, t2d = q
    a_f, b_f = (ypx, ymx) if neg else (ymx, ypx)
    A = l_mul(l_sub(Y, X), a_f)
    B = l_mul(l_add(Y, X), b_f)
    C = l_mul(T, t2d)
    Dd = l_add(Z, Z)
    E, H = l_sub(B, A), l_add(B, A)
    DmC, DpC = l_sub(Dd, C), l_add(Dd, C)
    XF, XG = (DpC, DmC) if neg else (DmC, DpC)
    return [l_mul(XF, E), l_mul(XG, H), l_mul(DmC, DpC), l_mul(E, H)]


def l_gd_add(p, q):
    A = l_mul(l_sub(p[1], p[0]), l_sub(q[1], q[0]))
    B = l_mul(l_add(p[1], p[0]), l_add(q[1], q[0]))
    C = l_mul(l_mul(p[3], q[3]), D2_LIMBS)
    Dd = l_mul(p[2], q[2]); Dd = l_add(Dd, Dd)
    E, H, F, G = l_sub(B, A), l_add(B, A), l_sub(Dd, C), l_add(Dd, C)
    return [l_mul(F, E), l_mul(G, H), l_mul(F, G), l_mul(E, H)]


def l_gd_double(p, with_t=True):
    XX, YY, ZZ = l_sq(p[0]), l_sq(p[1]), l_sq(p[2])
    ZZ2 = l_add(ZZ, ZZ)
    S = l_sq(l_add(p[0], p[1]))
    cY = l_carry(l_add(YY, XX))
    cZ = l_carry(l_sub(YY, XX))
    cX = l_sub(S, cY)
    cT = l_sub(ZZ2, cZ)
    return [l_mul(cT, cX), l_mul(cY, cZ), l_mul(cT, cZ), l_mul(cX, cY) if with_t else list(p[3])]


def l_to_niels(p, zi=None):
    if zi is None:
        zi = l_invert(p[2])
    x, y = l_mul(p[0], zi), l_mul(p[1], zi)
    return [l_pack(l_add(y, x)), l_pack(l_sub(y, x)), l_pack(l_mul(l_mul(x, y), D2_LIMBS))]


def _fds(case, k, n=1):
    r = [[int(x) for x in case[10 * (k + i):10 * (k + i) + 10]] for i in range(n)]
    return r[0] if n == 1 else r


def _words(x):
    return [(x >> (32 * i)) & 0xffffffff for i in range(8)]


def limbs(op, case):
    """the words the library writes for this case (dict word index -> value), by the limb model; BoundError if the case leaves the contract"""
    a, b, c, d = _fds(case, 0, 4)
    if op == UNPACK:
        out = l_unpack(case[:8])
    elif op == CARRY:
        out = l_carry(a)
    elif op == PACK:
        x = l_pack(a); out = _words(x) + _words(x % P)
    elif op == ADD:
        out = l_add(a, b)
    elif op == SUB:
        out = l_sub(a, b)
    elif op == NEG:
        out = l_neg(a)
    elif op == MUL:
        out = l_mul(a, b)
    elif op == SQ:
        out = l_sq(a)
    elif op == MUL_LOOSE:
        out = l_mul(l_sub(a, b), l_add(c, d))
    elif op == SQ_LOOSE:
        out = l_sq(l_add(a, b))
    elif op == INVERT:
        out = l_invert(a)
    elif op == POW22523:
        out = l_pow22523(a)
    elif op == SQRT_RATIO:
        r, f = l_sqrt_ratio(a, b); out = r + [f]
    elif op == ABS:
        out = l_abs(a)
    elif op == PRED:
        out = [l_isneg(a), l_iszero(a), l_eq(a, b)]
    elif op in (MADD, MSUB):
        out = sum(l_madd(_fds(case, 0, 4), _fds(case, 4, 3), op == MSUB), [])
    elif op in (GD_ADD, GQ_ADD):
        out = sum(l_gd_add(_fds(case, 0, 4), _fds(case, 4, 4)), [])
    elif op in (GD_DOUBLE, GQ_DOUBLE):
        out = sum(l_gd_double(_fds(case, 0, 4)), [])
    elif op == GD_DOUBLE_NOT:
        out = sum(l_gd_double(_fds(case, 0, 4), with_t=False), [])
    elif op == TO_NIELS:
        out = sum((_words(x) for x in l_to_niels(_fds(case, 0, 4))), [])
    elif op == TO_NIELS_ZINV:
        out = sum((_words(x) for x in l_to_niels(_fds(case, 0, 4), _fds(case, 4))), [])
    else:
        raise ValueError(op)
    if op in (GQ_ADD, GQ_DOUBLE):
        out = out + out         # the quad's result, then the one-thread result
    return out


# ---------------------------------------------------------------- value model (polynomials mod p)
def _sqrt(x):
    """a square root of the quadratic residue x (p = 5 mod 8)"""
    r = pow(x, (P + 3) // 8, P)
    if r * r % P != x:
        r = r * SQRTM1 % P
    assert r * r % P == x
    return r


def sqrt_ratio(u, v):
    """RFC 9496 4.2: (was_square, the non-negative root of u / v, or of sqrt(-1) u / v when u / v is not a square); (0, 0) for v = 0, u != 0"""
    u %= P; v %= P
    if u == 0:
        return 1, 0
    if v == 0:
        return 0, 0
    q = u * pow(v, -1, P) % P
    sq = pow(q, (P - 1) // 2, P) == 1
    r = _sqrt(q if sq else q * SQRTM1 % P)
    return int(sq), (P - r if r & 1 else r)


def v_madd(p, q, neg):
    X, Y, Z, T = p
    ypx, ymx, t2d = q
    if neg:
        ypx, ymx, t2d = ymx, ypx, -t2d
    A, B, C, Dd = (Y - X) * ymx, (Y + X) * ypx, T * t2d, 2 * Z
    E, H, F, G = B - A, B + A, Dd - C, Dd + C
    return [F * E % P, G * H % P, F * G % P, E * H % P]


def v_gd_add(p, q):
    A, B, C, Dd = (p[1] - p[0]) * (q[1] - q[0]), (p[1] + p[0]) * (q[1] + q[0]), p[3] * q[3] * D2, 2 * p[2] * q[2]
    E, H, F, G = B - A, B + A, Dd - C, Dd + C
    return [F * E % P, G * H % P, F * G % P, E * H % P]


def v_gd_double(p):
    XX, YY, ZZ2, S = p[0] * p[0], p[1] * p[1], 2 * p[2] * p[2], (p[0] + p[1]) ** 2
    cY, cZ = YY + XX, YY - XX
    cX, cT = S - cY, ZZ2 - cZ
    return [cT * cX % P, cY * cZ % P, cT * cZ % P, cX * cY % P]


def v_to_niels(p, zi):
    x, y = p[0] * zi % P, p[1] * zi % P
    return [(y + x) % P, (y - x) % P, x * y * D2 % P]


def expect(op, case):
    """what the output of a case must satisfy, as a list of
         ("fd", k, value, tight): limbs 10k .. 10k+9 have this value mod p (and are tight if the header promises it);
         ("fe", w, value): the 8 words from w are an integer of this value mod p;   ("w", i, x): word i == x;
         ("same", k, j): limbs 10k .. are bit for bit the input's limbs 10j .."""
    va, vb, vc, vd = (value(x) for x in _fds(case, 0, 4))
    p = [value(x) for x in _fds(case, 0, 4)]
    q = [value(x) for x in _fds(case, 4, 4)]
    if op == UNPACK:
        return [("fd", 0, sum(int(case[i]) << (32 * i) for i in range(8)) % P, True)]
    if op == CARRY:
        return [("fd", 0, va, True)]
    if op == PACK:
        return [("fe", 0, va)] + [("w", 8 + i, x) for i, x in enumerate(_words(va))]
    if op == ADD:
        return [("fd", 0, (va + vb) % P, False)]
    if op == SUB:
        return [("fd", 0, (va - vb) % P, False)]
    if op == NEG:
        return [("fd", 0, -va % P, False)]
    if op == MUL:
        return [("fd", 0, va * vb % P, True)]
    if op == SQ:
        return [("fd", 0, va * va % P, True)]
    if op == MUL_LOOSE:
        return [("fd", 0, (va - vb) * (vc + vd) % P, True)]
    if op == SQ_LOOSE:
        return [("fd", 0, (va + vb) ** 2 % P, True)]
    if op == INVERT:
        return [("fd", 0, pow(va, P - 2, P), True)]
    if op == POW22523:
        return [("fd", 0, pow(va, (P - 5) // 8, P), True)]
    if op == SQRT_RATIO:
        sq, r = sqrt_ratio(va, vb)
        return [("fd", 0, r, True), ("w", 10, sq)]
    if op == ABS:
        return [("fd", 0, P - va if va & 1 else va, True)]
    if op == PRED:
        return [("w", 0, va & 1), ("w", 1, int(va == 0)), ("w", 2, int(va == vb))]
    if op in (MADD, MSUB):
        return [("fd", k, x, True) for k, x in enumerate(v_madd(p, q[:3], op == MSUB))]
    if op == GD_ADD:
        return [("fd", k, x, True) for k, x in enumerate(v_gd_add(p, q))]
    if op == GD_DOUBLE:
        return [("fd", k, x, True) for k, x in enumerate(v_gd_double(p))]
    if op == GD_DOUBLE_NOT:
        return [("fd", k, x, True) for k, x in enumerate(v_gd_double(p)[:3])] + [("same", 3, 3)]
    if op == TO_NIELS:
        return [("fe", 8 * k, x) for k, x in enumerate(v_to_niels(p, pow(p[2], P - 2, P)))]
    if op == TO_NIELS_ZINV:
        return [("fe", 8 * k, x) for k, x in enumerate(v_to_niels(p, q[0]))]
    if op in (GQ_ADD, GQ_DOUBLE):
        r = v_gd_add(p, q) if op == GQ_ADD else v_gd_double(p)
        return [("fd", k, x, True) for k, x in enumerate(r + r)]
    raise ValueError(op)


def check_outputs(op, cases, outs, with_limb_model=True):
    """every case of an op against the value model (and tightness), and bit for bit against the limb model"""
    assert len(cases) == len(outs)
    for n, (case, out) in enumerate(zip(cases, outs)):
        tag = "%s case %d" % (FD_OP_NAMES[op], n)
        out = [int(x) for x in out]
        for chk in expect(op, case):
            if chk[0] == "fd":
                v = out[10 * chk[1]:10 * chk[1] + 10]
                assert value(v) == chk[2], tag + ": value of element %d" % chk[1]
                assert not chk[3] or is_tight(v), tag + ": element %d is not tight: %s" % (chk[1], [hex(x) for x in v])
            elif chk[0] == "fe":
                assert sum(out[chk[1] + i] << (32 * i) for i in range(8)) % P == chk[2], tag + ": packed value at word %d" % chk[1]
            elif chk[0] == "w":
                assert out[chk[1]] == chk[2], tag + ": word %d" % chk[1]
            else:
                assert out[10 * chk[1]:10 * chk[1] + 10] == [int(x) for x in case[10 * chk[2]:10 * chk[2] + 10]], tag + ": element %d changed" % chk[1]
        if with_limb_model:
            want = limbs(op, case)
            assert out[:len(want)] == want, tag + ": limbs differ from the limb model"


# ---------------------------------------------------------------- corpus
FIELD_VALUES = [0, 1, 2, P - 1, P - 2, (P - 1) // 2, (P + 1) // 2, SQRTM1, P - SQRTM1, D, D2,
                P, P + 1, P + 18, 2 ** 255 - 1, 2 ** 255 - 20]          # the last five are not canonical


def special_tight():
    """the limb patterns and field values every op sees (all tight)"""
    mx = [t - 1 for t in TIGHT]
    pats = [[0] * 10, mx, list(M), [mx[i] if i % 2 == 0 else 0 for i in range(10)], [mx[i] if i % 2 else 0 for i in range(10)]]
    pats += [[mx[i] if i == k else 0 for i in range(10)] for k in range(10)]          # one hot limb, at its maximum
    pats += [[M[i] + (1 if i == 0 else 0) for i in range(10)]]                         # a carry that ripples through all ten limbs
    return pats + [from_int(x) for x in FIELD_VALUES]


def random_tight(rng):
    kind = rng.randrange(4)
    if kind == 0:
        return [rng.randrange(t) for t in TIGHT]
    if kind == 1:
        return [t - 1 - rng.randrange(4) for t in TIGHT]                               # a hair below the tight bound
    if kind == 2:
        return [rng.choice((0, 1, M[i], TIGHT[i] - 1, rng.randrange(TIGHT[i]))) for i in range(10)]
    return from_int(rng.randrange(2 ** 255))


def _odd_count(n):
    """corpus sizes are no multiple of 4 (a quad) or of the block size, so the tail guards run"""
    return n % 4 != 0 and n % 256 != 0


def _finish(rows, width):
    import numpy as np
    out = np.zeros((len(rows), width), np.uint32)
    for i, r in enumerate(rows):
        flat = [x for e in r for x in e]
        out[i, :len(flat)] = flat
    assert _odd_count(len(rows)), len(rows)
    return out


def _pad_random(rows, rng, k, total):
    while len(rows) < total:
        rows.append([random_tight(rng) for _ in range(k)])
    return rows


def fd_corpus(op):
    """uint32 [n][80]: the cases of one op, deterministic"""
    rng = random.Random(0x26f0 + op)
    sp = special_tight()
    mx = [t - 1 for t in TIGHT]
    zero = [0] * 10
    rows = []
    if op == UNPACK:
        vals = list(FIELD_VALUES) + [x + 2 ** 255 for x in FIELD_VALUES] + [2 ** 256 - 1, 2 ** 255, 2 ** 256 - 2 ** 255 + 18]
        vals += [1 << k for k in range(0, 256, 5)] + [(1 << 256) - 1 - (1 << k) for k in range(0, 256, 7)]
        vals += [rng.randrange(2 ** 256) for _ in range(301 - len(vals) % 4)]
        rows = [[_words(x)] for x in vals]
    elif op in (CARRY, PACK, ABS):
        loose = [[CARRY_MAX - 1] * 10, [CARRY_MAX - 1 if i % 2 == 0 else 0 for i in range(10)], [CARRY_MAX - 1 if i % 2 else 0 for i in range(10)]]
        loose += [[CARRY_MAX - 1 if i == k else 0 for i in range(10)] for k in range(10)]
        loose += [[CARRY_MAX - 1 if i == k else M[i] for i in range(10)] for k in range(10)]
        loose += [l_add(x, y) for x in sp[:6] for y in sp[:6]] + [l_sub(x, y) for x in sp[:6] for y in sp[:6]]
        loose += [[rng.randrange(CARRY_MAX) for _ in range(10)] for _ in range(200)]
        rows = _pad_random([[x] for x in sp + loose], rng, 1, 601)
    elif op == PRED:
        loose = [[CARRY_MAX - 1] * 10] + [[rng.randrange(CARRY_MAX) for _ in range(10)] for _ in range(50)]
        rows = [[x, y] for x in sp for y in sp[-len(FIELD_VALUES):]]                   # includes x = 0 against p, 18 against 2^255 - 1, ...
        rows += [[x, l_add(x, from_int(P))] for x in sp] + [[x, l_carry(x)] for x in loose] + [[x, y] for x in loose[:8] for y in loose[:8]]
        rows = _pad_random(rows, rng, 2, (len(rows) + 101) | 1)
    elif op == ADD:
        rows = [[x, y] for x in sp for y in sp]
        rows += [[[2 ** 32 - 1 - v for v in y], y] for y in sp]                        # sums of 2^32 - 1 in every limb
        rows += [[[2 ** 31 - 1] * 10, [2 ** 31] * 10], [[2 ** 32 - 1] * 10, zero]]
        rows = _pad_random(rows, rng, 2, 1401)
    elif op == SUB:
        rows = [[x, y] for x in sp for y in sp]
        rows += [[[2 ** 32 - 1 - k for k in SUB_BIAS], y] for y in sp]                 # the largest minuend the bias leaves room for
        rows += [[[2 ** 32 - 1 - k for k in SUB_BIAS], zero], [zero, mx]]
        rows = _pad_random(rows, rng, 2, 1401)
    elif op == NEG:
        rows = _pad_random([[x] for x in sp], rng, 1, 301)
    elif op == MUL:
        fmax, gmax = [MUL_F_MAX - 1] * 10, [G19_MAX] * 10
        rows = [[fmax, gmax]]                                                          # the contract's extreme
        rows += [[x, y] for x in sp for y in sp]
        rows += [[fmax, y] for y in sp] + [[x, gmax] for x in sp]
        rows += [[[MUL_F_MAX - 1 if i == k else 0 for i in range(10)], gmax] for k in range(10)]
        rows += [[fmax, [G19_MAX if i == k else 0 for i in range(10)]] for k in range(10)]
        rows += [[[rng.randrange(MUL_F_MAX) for _ in range(10)], [rng.randrange(G19_MAX + 1) for _ in range(10)]] for _ in range(300)]
        rows = _pad_random(rows, rng, 2, 1601)
    elif op == SQ:
        smax = [G38_MAX if i % 2 else G19_MAX for i in range(10)]
        rows = [[smax]] + [[x] for x in sp]
        rows += [[[smax[i] if i == k else 0 for i in range(10)]] for k in range(10)]
        rows += [[[smax[i] if i != k else 0 for i in range(10)]] for k in range(10)]
        rows += [[[rng.randrange(smax[i] + 1) for i in range(10)]] for _ in range(300)]
        rows = _pad_random(rows, rng, 1, 901)
    elif op == MUL_LOOSE:
        rows = [[mx, zero, mx, mx], [zero, mx, mx, mx], [mx, mx, mx, mx], [mx, zero, zero, zero], [zero, zero, mx, mx]]
        rows += [[x, y, x, y] for x in sp for y in sp[:12]]
        rows += [[rng.choice(sp) for _ in range(4)] for _ in range(600)]
        rows = _pad_random(rows, rng, 4, 1401)
    elif op == SQ_LOOSE:
        rows = [[x, y] for x in sp for y in sp]
        rows = _pad_random(rows, rng, 2, 1201)
    elif op in (INVERT, POW22523):
        rows = _pad_random([[x] for x in sp], rng, 1, 61)
    elif op == SQRT_RATIO:
        vs = [x for x in sp if value(x) != 0]
        rs = [2, 3, P - 1, SQRTM1, D, (P - 1) // 2]
        rows = [[zero, v] for v in vs[:6]] + [[from_int(P), from_int(P + 1)], [zero, zero]]
        rows += [[u, zero] for u in vs[:6]] + [[u, from_int(P)] for u in vs[:3]]                             # v = 0, also as the limbs of p
        for k, v in enumerate(vs):
            r = rs[k % len(rs)]
            vv = value(v)
            rows.append([from_int(r * r * vv % P), v])                                                       # a square
            rows.append([from_int(2 * r * r * vv % P), v])                                                   # a non-square (2 is none, p = 5 mod 8)
            rows.append([from_int(SQRTM1 * r * r * vv % P), v])                                              # sqrt(-1) times a square
            rows.append([v, v])                                                                              # u = v
            rows.append([l_carry(l_neg(v)), v])                                                              # u = -v
        rows = _pad_random(rows, rng, 2, (len(rows) + 21) | 1)
    elif op in (MADD, MSUB, GD_ADD, GQ_ADD, GD_DOUBLE, GQ_DOUBLE, GD_DOUBLE_NOT, TO_NIELS, TO_NIELS_ZINV):
        k = {MADD: 7, MSUB: 7, GD_ADD: 8, GQ_ADD: 8, TO_NIELS_ZINV: 5}.get(op, 4)
        heavy = op in (TO_NIELS, TO_NIELS_ZINV)
        one = from_int(1)
        base = [mx, zero, list(M), one]
        rows = [[b] * k for b in base]
        rows += [[mx if (m >> i) & 1 else zero for i in range(k)] for m in range(1, 2 ** k - 1)] if not heavy else []
        n_mix = 40 if heavy else 700
        for _ in range(n_mix):
            rows.append([rng.choice((mx, mx, zero, list(M), one, random_tight(rng), random_tight(rng))) for _ in range(k)])
        rows = _pad_random(rows, rng, k, (len(rows) + (24 if heavy else 200)) | 1)
    else:
        raise ValueError(op)
    return _finish(rows, FD_IN)


# ---------------------------------------------------------------- scalar field mod l
SC_VALUES = [0, 1, L - 1, L, L + 1, 2 ** 252, 2 ** 253 - 1, 2 ** 256 - 1]
SC_WIDE = [2 ** 512 - 1, L * 2 ** 256, (L - 1) * (2 ** 256 + 1), 0, 1, L, 2 ** 256, L * L, (L - 1) * (L - 1)]


def sc_int(w):
    return sum(int(w[i]) << (32 * i) for i in range(8))


def sc_expect(op, case):
    """the canonical result of a scalar op; BoundError if the operands leave the op's stated domain"""
    a, b = sc_int(case[0:8]), sc_int(case[8:16])
    if op == SC_MONTMUL:
        if a * b >= L * R:
            raise BoundError("sc_montmul needs a b < l R")
        return a * b * RINV % L
    if op == SC_TO_MONT:
        return a * R % L
    if op == SC_FROM_MONT:
        return a * RINV % L
    if op == SC_MUL_PLAIN:
        if a * b >= L * R:
            raise BoundError("sc_mul_plain needs a b < l R")
        return a * b % L
    if op in (SC_ADD, SC_SUB, SC_NEG, SC_INVERT_MONT):
        if a >= L or (b >= L and op in (SC_ADD, SC_SUB)):
            raise BoundError("operand >= l")
        return {SC_ADD: (a + b) % L, SC_SUB: (a - b) % L, SC_NEG: -a % L, SC_INVERT_MONT: pow(a * RINV % L, L - 2, L) * R % L}[op]
    if op == SC_LOAD_REDUCED:
        return a % L
    if op == SC_FROM_WIDE:
        return (a + b * R) % L
    if op == SC_FROM_WIDE_MONT:
        return (a + b * R) * R % L
    if op == SC_MAC:
        count = int(case[256])
        if not 1 <= count <= 16:
            raise BoundError("sc_redc_wide holds sixteen products")
        t = 0
        for k in range(count):
            x, y = sc_int(case[16 * k:16 * k + 8]), sc_int(case[16 * k + 8:16 * k + 16])
            if x >= L or y >= L:
                raise BoundError("sc_mac_wide operand >= l")
            t += x * y
        return t * RINV % L
    raise ValueError(op)


def sc_corpus(op):
    """uint32 [n][264]"""
    import numpy as np
    rng = random.Random(0x5c00 + op)
    small = [x for x in SC_VALUES if x < L]
    rnd_l = [rng.randrange(L) for _ in range(24)] + [L - 1 - rng.randrange(2 ** 32) for _ in range(4)]
    rnd_any = [rng.randrange(2 ** 256) for _ in range(24)] + [2 ** 256 - 1 - rng.randrange(2 ** 32) for _ in range(4)] + [L + rng.randrange(2 ** 64) for _ in range(4)]
    lt, anyv = small + rnd_l, SC_VALUES + rnd_l[:8] + rnd_any
    rows = []
    if op in (SC_MONTMUL, SC_MUL_PLAIN):
        rows = [[x, y] for x in anyv for y in lt] + [[y, x] for x in SC_VALUES + rnd_any[:6] for y in small + rnd_l[:6]]
    elif op in (SC_TO_MONT, SC_FROM_MONT, SC_LOAD_REDUCED):
        rows = [[x] for x in anyv + [rng.randrange(2 ** 256) for _ in range(60)]]
    elif op in (SC_ADD, SC_SUB):
        rows = [[x, y] for x in lt for y in lt]
    elif op == SC_NEG:
        rows = [[x] for x in lt + [rng.randrange(L) for _ in range(40)]]
    elif op in (SC_FROM_WIDE, SC_FROM_WIDE_MONT):
        rows = [[w % R, w // R] for w in SC_WIDE] + [[x, y] for x in SC_VALUES + rnd_any[:8] for y in SC_VALUES + rnd_any[8:16]]
        rows += [[rng.randrange(R), rng.randrange(R)] for _ in range(100)]
    elif op == SC_MAC:
        for count in range(1, 17):
            rows.append([L - 1] * (2 * count) + [0] * (32 - 2 * count) + [count])     # count products of (l-1)(l-1)
            rows.append([0] * 32 + [count])
            for _ in range(6):
                rows.append([rng.choice(lt) for _ in range(2 * count)] + [0] * (32 - 2 * count) + [count])
            rows.append([rng.randrange(L) for _ in range(32)] + [count])               # operands past `count` must not be read into the sum
    elif op == SC_INVERT_MONT:
        rows = [[x] for x in small + rnd_l[:20] + [R % L, R * R % L]]
    else:
        raise ValueError(op)
    while not _odd_count(len(rows)):
        rows.append([rng.randrange(L), rng.randrange(L)] if op != SC_MAC else [rng.randrange(L) for _ in range(32)] + [16])
    out = np.zeros((len(rows), SC_IN), np.uint32)
    for i, r in enumerate(rows):
        scal, count = (r[:32], r[32]) if op == SC_MAC else (r, 0)
        for k, x in enumerate(scal):
            out[i, 8 * k:8 * k + 8] = _words(x)
        out[i, 256] = count
    return out


def check_sc_outputs(op, cases, outs):
    assert len(cases) == len(outs)
    for n, (case, out) in enumerate(zip(cases, outs)):
        assert sc_int(out) == sc_expect(op, case), "%s case %d" % (SC_OP_NAMES[op], n)
