"""Forgeries whose errors cancel under EQUAL weights -- the inputs of tests/test_cancellation_corpus.py (CPU: the corpus has teeth) and
tests/test_gpu_batch_cancellation.py (GPU: every entry point that folds equations into a random linear combination rejects them).

A verifier that sums equations with random weights is sound only when every equation of the sum has its own independent weight.  A set of
errors whose residuals add up to the identity passes such a sum exactly when its members share a weight, so these sets tell independent
weights from shared ones (a single tampered member cannot: any non-zero weight rejects it).  They are easy to build because the response
scalars of a proof are not hashed into its transcript: the challenges stay what they were.

  Sigma-proofs (per element: points | Z_m | Z_r1 | [Z_r2]); equations e1, e2 (kinds 0, 1), e3 (kinds 1, 2), see k_sigma_vprep:
    S1  Z_m[i] + delta, Z_m[j] - delta          (kind 0)        -/+ delta B in e1
    S2  Z_r1[i] + delta, Z_r1[j] - delta        (kinds 0, 1, 2) e1 on B_blinding, and e2 on B in kinds 0, 1
    S3  Z_r2[i] + delta, Z_r2[j] - delta        (kinds 1, 2)    e3 on B_blinding
    S4  Z_r1[i] + delta, Z_r2[j] - delta        (kind 2)        e1 of element i against e3 of element j
    S5  Z_r1 of three elements + 2 delta, - delta, - delta
  Range proofs (a at byte 7 * 32 + 64 lg of a proof, b behind it): the check is affine in a (and in b) for fixed challenges, and members with
  identical bytes have identical challenges, so a + delta in one copy and a - delta in another leave residuals +E and -E.
    R1  two chunks of ONE client with equal values and blindings, the second chunk's proof overwritten with the first's, then a +- delta
    R2  the same update submitted twice (or three times: + 2 delta, - delta, - delta), a +- delta on the same chunk of the copies
    R3  R2 on b

Everything honest comes from the oracle with seeded inputs and seeded nonces (the product's proofs are the oracle's byte for byte), so the
module needs no GPU.  Arrays handed out are shared between tests: they are read-only, every builder returns a fresh copy."""
import functools

import numpy as np

import orc

ELL = orc.L_ORDER
FP = (16, 7)
NB = 8
DELTA_BIG = (1 << 249) + 0x2545F4914F6CDD1D9E3779B97F4A7C15F39CC0605CEDC834      # one fixed 250-bit delta
DELTAS = (1, DELTA_BIG)
assert DELTA_BIG.bit_length() == 250 and DELTA_BIG < ELL

# kind -> (points per element, proof bytes, commitment bytes): RandProof, SquareRandProof, SquareProof
SIGMA = {0: (2, 128, 64), 1: (3, 192, 96), 2: (2, 160, 64)}
SIGMA_LABEL = {0: b"RandProof", 1: b"SquareRandProof", 2: b"SquareProof"}
Z_FIELDS = {"z_m": 0, "z_r1": 32, "z_r2": 64}


def edit(row, delta):
    """row (a 32-byte view of a canonical scalar z) := (z + delta) mod l, canonical; delta may be negative"""
    z = (int.from_bytes(row.tobytes(), "little") + delta) % ELL
    row[:] = np.frombuffer(z.to_bytes(32, "little"), np.uint8)


def _frozen(a):
    a = np.ascontiguousarray(a)
    a.setflags(write=False)
    return a


def _scalars(rng, d):
    b = rng.integers(0, 256, size=(d, 32), dtype=np.uint8)
    b[:, 31] &= 0x0F      # < 2^252 < l: canonical
    return b


# ---------------------------------------------------------------- Sigma-proofs
@functools.lru_cache(maxsize=None)
def sigma_honest(kind, d, seed=0):
    """(proofs u8[d, plen], commitments u8[d, clen]) of an honest vector of d elements, read-only"""
    rng = np.random.default_rng(1000 + 100 * kind + seed)
    x = (rng.integers(-100, 101, size=d) / 128.0).astype(np.float32)
    r1 = _scalars(rng, d)
    r2 = _scalars(rng, d) if kind else None
    rc, pr, cm = orc.sigma_create(kind, x, r1, r2, FP[0], FP[1], seed=bytes([17 + kind + seed]) * 32)
    assert rc == 0
    return _frozen(pr.copy()), _frozen(cm.copy())


def sigma_apply(kind, proofs, edits, delta):
    """a copy of `proofs` (u8[d, plen] of `kind`) with field[elem] += mult * delta for every (elem, field, mult) of `edits`"""
    npts, plen, _ = SIGMA[kind]
    out = np.array(proofs, dtype=np.uint8, copy=True).reshape(-1, plen)
    for elem, field, mult in edits:
        assert field != "z_r2" or kind != 0
        off = 32 * npts + Z_FIELDS[field]
        edit(out[elem, off:off + 32], mult * delta)
    return out


def s1(i, j):
    return [(i, "z_m", 1), (j, "z_m", -1)]


def s2(i, j):
    return [(i, "z_r1", 1), (j, "z_r1", -1)]


def s3(i, j):
    return [(i, "z_r2", 1), (j, "z_r2", -1)]


def s4(i, j):
    return [(i, "z_r1", 1), (j, "z_r2", -1)]


def s5(i, j, k):
    return [(i, "z_r1", 2), (j, "z_r1", -1), (k, "z_r1", -1)]


# the element pairs of every vector length: two elements; two blocks of 256 threads (two partial sums of the fixed-base coefficients) and a
# wave boundary; the same thread of two blocks
SIGMA_PAIRS = {2: [(0, 1)], 257: [(255, 256), (0, 256), (63, 64)], 300: [(0, 299), (7, 263)]}
SIGMA_TRIPLES = {2: [], 257: [(0, 255, 256)], 300: [(43, 44, 299)]}
S4_FIRST = {2: [0, 1], 257: [254], 300: [255]}      # i of S4; j = i - 2 .. i + 2 where it exists


def sigma_cases(kind, d):
    """[(name, edits)] of the constructions that apply to `kind` at vector length d"""
    out = []
    for (i, j) in SIGMA_PAIRS[d]:
        if kind == 0:
            out.append(("S1(%d,%d)" % (i, j), s1(i, j)))
        out.append(("S2(%d,%d)" % (i, j), s2(i, j)))
        if kind != 0:
            out.append(("S3(%d,%d)" % (i, j), s3(i, j)))
    if kind == 2:
        for i in S4_FIRST[d]:
            for j in range(i - 2, i + 3):
                if 0 <= j < d:
                    out.append(("S4(%d,%d)" % (i, j), s4(i, j)))
    for t in SIGMA_TRIPLES[d]:
        out.append(("S5(%d,%d,%d)" % t, s5(*t)))
    return out


def sigma_equations(kind, field):
    """the equations (1, 2, 3) that a change of `field` leaves a residual in"""
    return {"z_m": [1] + ([3] if kind else []), "z_r1": [1] + ([2] if kind != 2 else []), "z_r2": [3]}[field]


# ---------------------------------------------------------------- range proofs
def ab_offset(proof_len, field="a"):
    lg = (proof_len // 32 - 9) // 2
    return 7 * 32 + 64 * lg + (32 if field == "b" else 0)


def range_apply(proofs, edits, delta, field="a"):
    """a copy of one client's proofs u8[n_proofs, plen] with a (or b) of chunk c += mult * delta for every (c, mult) of `edits`"""
    out = np.array(proofs, dtype=np.uint8, copy=True)
    off = ab_offset(out.shape[1], field)
    for c, mult in edits:
        edit(out[c, off:off + 32], mult * delta)
    return out


def _values(rng, d):
    return (rng.integers(-100, 101, size=d) / 128.0).astype(np.float32)


@functools.lru_cache(maxsize=None)
def range_client(d, P, seed, nb=NB):
    """(proofs, commitments) of an honest client, read-only"""
    rng = np.random.default_rng(2000 + seed)
    rc, pr, cm = orc.create_rangeproof(_values(rng, d), _scalars(rng, d), nb, P, FP[0], FP[1], seed=bytes([31 + seed % 200]) * 32)
    assert rc == 0
    return _frozen(pr), _frozen(cm.copy())


@functools.lru_cache(maxsize=None)
def range_r1(d, P, p, q, nb=NB):
    """R1's honest input: a client whose chunks p and q hold equal values and equal blindings, proof q overwritten with proof p (still a
    valid set: the two chunks' statements are the same).  (proofs, commitments), read-only"""
    rng = np.random.default_rng(3000 + 64 * p + q)
    x, bl = _values(rng, d), _scalars(rng, d)
    m = d // P
    assert m * P == d and d & (d - 1) == 0 and p != q
    x[q * m:(q + 1) * m] = x[p * m:(p + 1) * m]
    bl[q * m:(q + 1) * m] = bl[p * m:(p + 1) * m]
    rc, pr, cm = orc.create_rangeproof(x, bl, nb, P, FP[0], FP[1], seed=bytes([77]) * 32)
    assert rc == 0 and pr.shape[0] == P and (cm[q * m:(q + 1) * m] == cm[p * m:(p + 1) * m]).all()
    assert (pr[q] != pr[p]).any()      # (their nonces differ)
    pr = pr.copy()
    pr[q] = pr[p]
    return _frozen(pr), _frozen(cm.copy())


R1_SHAPES = [(8, 4, 0, 1), (8, 4, 0, 3), (8, 4, 2, 3), (128, 64, 0, 63), (128, 64, 31, 32)]      # (d, P, p, q)
R1_RUN = (8, 4, 1, 2)      # the pair inside the run of chunks [1, 3)


def copies_batch(n, copies, d=8, P=4, seed0=0):
    """R2 / R3's honest input: n clients, those at the positions `copies` one and the same update, the others distinct.
    -> (list of proofs, list of commitments), fresh writable copies"""
    dup = range_client(d, P, seed0 + 99)
    mem = [dup if i in copies else range_client(d, P, seed0 + i) for i in range(n)]
    return [np.array(p) for p, _ in mem], [np.array(c) for _, c in mem]


def copies_edits(copies):
    """multipliers of delta over the copies: +1, -1 for two, +2, -1, -1 for three"""
    return dict(zip(copies, (1, -1) if len(copies) == 2 else (2, -1, -1)))


# positions of the copies in a batch of nine: verify_chunks' closer look takes groups of ceil(sqrt(9)) = 3 units -- {0,1,2} {3,4,5} {6,7,8}
COPIES_OF_NINE = {"one group": (3, 4), "adjacent, two groups": (2, 3), "first and last": (0, 8), "three copies": (1, 5, 6)}

L2_BITS = 32


@functools.lru_cache(maxsize=None)
def l2_member(seed):
    """(sum proof, commitment) of an honest client of the L2 sum-proof batch (one value, the (32, 1) generators), read-only"""
    rng = np.random.default_rng(4000 + seed)
    d = 4
    x = (rng.integers(-100, 101, size=d) / 128.0).astype(np.float32)
    rc, pr, cm = orc.create_rangeproof_l2(x, _scalars(rng, d), L2_BITS, 1, FP[0], FP[1], seed=bytes([131 + seed % 100]) * 32)
    assert rc == 0
    return _frozen(pr), _frozen(cm.copy())


def l2_batch(n, copies):
    dup = l2_member(99)
    mem = [dup if i in copies else l2_member(i) for i in range(n)]
    return [np.array(p) for p, _ in mem], [np.array(c) for _, c in mem]
