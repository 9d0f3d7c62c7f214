"""Edwards representatives of Ristretto classes, shifted by every 4-torsion point -- pure Python on tests/golden/pyref.py, seeded, no GPU.

Every point the library holds stands for a Ristretto class, and K + T is a legal stand-in for the class K for each of the four
T in E[4] = {(0, 1), (0, -1), (i, 0), (-i, 0)}.  An encoder or an identity predicate that treats one of them differently is wrong only
where that representative turns up, and which one turns up is decided by the encodings that were summed.  So the corpus holds, per class
and per T,

  tuples()   a pair and a triple of valid, non-identity Ristretto encodings whose decoded Edwards sum is, in affine coordinates, exactly
             K + T: what drives a public sum-then-encode entry point to that representative from bytes alone.  Two decoded points cannot sum
             to (0, 1) or (0, -1) (decode(enc(-P)) is never -decode(enc(P)) nor its (0, -1) shift: both have a negative x or a negative
             x y): those two pair cells of the identity class stay empty, which the search asserts, and the triples cover them.
  raw_reps() the same K + T as projective (X, Y, Z, T) of canonical 32-byte coordinates with Z = 1, Z = 7 and a random Z: what
             rofl_dbg_encode_reps loads into each encoder's own point type.

The expected encoding is pyref.ristretto_encode(K): 32 zero bytes for the identity class."""
import functools
import hashlib
import os
import random
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import bsgs_model  # noqa: E402
import pyref  # noqa: E402

P, L = pyref.P, pyref.L
I = pyref.SQRT_M1
# affine (x, y) of E[4], in the order every table here uses
TORSION = (("(0,1)", (0, 1)), ("(0,-1)", (0, P - 1)), ("(i,0)", (I, 0)), ("(-i,0)", (P - I, 0)))
TORSION_ORDERS = (1, 2, 4, 4)
Z_KINDS = ("1", "7", "random")
SEED = 1
EXTRACT_M = 1 << 10      # the table size of the extraction tests: the classes v B of v = 0, 1, -1, m, -m are all here
ZERO32 = bytes(32)


def ext(xy):
    x, y = xy
    return (x % P, y % P, 1, x * y % P)


def affine(p):
    X, Y, Z, _ = p
    zi = pow(Z, P - 2, P)
    return (X * zi % P, Y * zi % P)


def shifted(K, t):
    """affine K + T_t"""
    return affine(pyref.pt_add(K, ext(TORSION[t][1])))


def which_torsion(p, K):
    """t with p == K + T_t in affine coordinates, None when p is not a representative of the class of K"""
    a = affine(p)
    for t in range(4):
        if a == shifted(K, t):
            return t
    return None


@functools.lru_cache(maxsize=None)
def mul_base(v):
    return pyref.pt_mul(v % L, pyref.BASE)


def decode_shift(v):
    """name of T = decode(enc(v B)) - v B: the representative a decoder hands on for the class v B"""
    K = mul_base(v)
    return TORSION[which_torsion(pyref.ristretto_decode(pyref.ristretto_encode(K)), K)][0]


@functools.lru_cache(maxsize=None)
def classes():
    """[(name, K)]: K is the class's representative in the prime-order subgroup (extended coordinates)"""
    out = [("0", pyref.IDENT), ("B", pyref.BASE), ("2B", mul_base(2)), ("(l-1)B", mul_base(L - 1)), ("Bblind", pyref.b_blinding()),
           ("uniform", pyref.from_uniform_bytes(hashlib.sha3_512(b"torsion corpus").digest()))]
    out += [("%dB" % m, mul_base(m)) for m in bsgs_model.TABLE_SIZES]
    out += [("-%dB" % EXTRACT_M, mul_base(-EXTRACT_M))]
    return tuple(out)


def class_point(name):
    return dict(classes())[name]


def expected(name):
    return pyref.ristretto_encode(class_point(name))


def impossible(name, t, arity):
    return name == "0" and arity == 2 and t in (0, 1)


@functools.lru_cache(maxsize=None)
def _pool():
    """random points k B and the point their encoding decodes to"""
    rng = random.Random(SEED)
    out = []
    for _ in range(24):
        pt = mul_base(rng.randrange(1, L))
        enc = pyref.ristretto_encode(pt)
        out.append((pt, enc, pyref.ristretto_decode(enc)))
    return out


def _fill(K, arity, rng, tries):
    """{t: tuple of encodings} found in `tries` draws: arity - 1 pool points and the encoding of what is missing to K"""
    cells = {}
    pool = _pool()
    for _ in range(tries):
        picks = rng.sample(pool, arity - 1)
        rest, total = K, None
        for pt, _, dec in picks:
            rest = pyref.pt_add(rest, pyref.pt_neg(pt))
            total = dec if total is None else pyref.pt_add(total, dec)
        enc = pyref.ristretto_encode(rest)
        if enc == ZERO32:
            continue
        t = which_torsion(pyref.pt_add(total, pyref.ristretto_decode(enc)), K)
        assert t is not None
        cells.setdefault(t, tuple(e for _, e, _ in picks) + (enc,))
        if len(cells) == 4:
            break
    return cells


@functools.lru_cache(maxsize=None)
def cells_for(K):
    """{(t, arity): tuple of `arity` encodings whose decoded sum is K + T_t} for any class K (a point of the prime-order subgroup, extended
    coordinates): every cell, but for the identity class no pair at t = 0, 1.  Seeded by the class, so the same K gives the same bytes."""
    ident = pyref.ristretto_encode(K) == ZERO32
    rng = random.Random("%d:%d:%d" % ((SEED,) + affine(K)))
    out = {}
    for arity in (2, 3):
        cells = _fill(K, arity, rng, 200)
        want = [t for t in range(4) if not (ident and arity == 2 and t in (0, 1))]
        if ident and arity == 2:
            assert set(cells) <= {2, 3}, "two decoded points summed to (0, +-1)"
        assert set(want) <= set(cells), (arity, sorted(cells))
        for t in want:
            out[(t, arity)] = cells[t]
    return out


@functools.lru_cache(maxsize=None)
def tuples():
    """{(class name, t, arity): encodings} over classes(): every cell but the two impossible ones"""
    return {(name, t, arity): encs for name, K in classes() for (t, arity), encs in cells_for(K).items()}


def rows(arity):
    """the filled cells of one arity as [(class name, t)], T-major: the identity-class rows lie between generic ones"""
    return [(name, t) for t in range(4) for name, _ in classes() if (name, t, arity) in tuples()]


def fe_bytes(x):
    return (x % P).to_bytes(32, "little")


@functools.lru_cache(maxsize=None)
def raw_reps():
    """[dict(name, t, z, xyzt = 128 bytes X | Y | Z | T, expect = 32 bytes, identity = bool)], class-major, then T, then Z"""
    rng = random.Random(SEED + 1)
    out = []
    for name, K in classes():
        want = expected(name)
        for t in range(4):
            x, y = shifted(K, t)
            for zk in Z_KINDS:
                z = {"1": 1, "7": 7}.get(zk) or rng.randrange(2, P)
                xyzt = b"".join(fe_bytes(c) for c in (x * z, y * z, z, x * y % P * z))
                out.append(dict(name=name, t=t, z=zk, xyzt=xyzt, expect=want, identity=(name == "0")))
    return tuple(out)


def rep_point(r):
    return tuple(int.from_bytes(r["xyzt"][32 * k:32 * k + 32], "little") for k in range(4))


# ---------------------------------------------------------------- cancelling multi-scalar multiplications
MSM_KS = (1, 2, 3, 4, L - 1)      # k (+-i, 0): order 4, order 2, order 4, then (0, 1) twice (l = 1 mod 4)
MSM_SIZES = (2, 66, 130)


@functools.lru_cache(maxsize=None)
def _filler():
    """64 pairs (enc(Q), enc(-Q)) and one scalar per pair: r decode(enc(Q)) + r decode(enc(-Q)) = r (+-i, 0)"""
    rng = random.Random(SEED + 2)
    out = []
    for _ in range(64):
        q = mul_base(rng.randrange(1, L))
        out.append((pyref.ristretto_encode(q), pyref.ristretto_encode(pyref.pt_neg(q)), rng.randrange(1, L)))
    return out


@functools.lru_cache(maxsize=None)
def msm_cases():
    """[dict(what, points = n encodings, scalars = one list of n integers per k of MSM_KS, expect = 32 bytes)].  Terms 0 and 1 are a pair
    (enc(P), enc(-P)) under the SAME scalar k: k (i, 0) or k (-i, 0), by the pair.  Behind them cancelling filler pairs up to n = 2, 66, 130
    terms.  `third`: one more term s C of a class that is not the identity (the filler is one pair shorter: n = 3, 65, 129); then every
    problem's result is s C, else the identity."""
    s3 = random.Random(SEED + 3).randrange(1, L)
    C = class_point("uniform")
    out = []
    for t in (2, 3):
        a, b = tuples()[("0", t, 2)]
        for n in MSM_SIZES:
            for third in (False, True):
                pairs = (n - 2) // 2 - (1 if third and n > 2 else 0)
                points, tail = [a, b], []
                if third:
                    points.append(pyref.ristretto_encode(C))
                    tail.append(s3)
                for qa, qb, r in _filler()[:pairs]:
                    points += [qa, qb]
                    tail += [r, r]
                out.append(dict(what="%s n=%d%s" % (TORSION[t][0], len(points), " + s C" if third else ""), points=tuple(points),
                                scalars=tuple(tuple([k, k] + tail) for k in MSM_KS),
                                expect=pyref.ristretto_encode(pyref.pt_mul(s3, C)) if third else ZERO32))
    return tuple(out)
