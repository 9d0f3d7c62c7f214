"""BSGSTable (bsgs32.rs:20-73) in plain integers mod l -- no curve: a point v B is the integer v, the table key compress(x B) is x.

    table     {x: x mod 2^bits for x in 0 .. m}                 (new: the identity, then B .. m B; the value is `x as BSGS_URawFix`)
    step      m mod 2^bits                                       (mG = B * Scalar::from(m as BSGS_URawFix))
    max_it    2^bits // m                                        (solve_discrete_log_default; get_size() = m)
    result    (it m + pw) mod 2^bits at the first hit            (`(i * get_size + pow) as BSGS_URawFix`)
    signs     the walk from M first, then the walk from -M and the negated result; None where the reference unwraps None

The model says what the reference RETURNS, which is not always the logarithm: with m = 2^15 and 16 bits the point 2^16 B is found at the
last iteration in the entry x = m and comes back as 0, and a table of 2^bits entries has a step of 0 and finds nothing above m.

The table is not materialised: `x in table` is 0 <= x <= m and table[x] is x mod 2^bits, which is the dictionary above for every m.

Also here: the (m, bits) pairs and the edge values of tests/test_gpu_torsion.py, so that the corpus (tests/torsion_corpus.py) can hold the
class m B of every table size and the host tests can check the inputs without a GPU."""
import random

L = 2 ** 252 + 27742317777372353535851937790883648493

# (table size, bsgs_bits); the last one is the 32-bit case, for which this model is the only reference
CASES = [(1 << 15, 16), (1 << 16, 16), (1 << 10, 16), (3000, 16), (1 << 7, 8), (1 << 8, 8), (100, 8), (1 << 20, 32)]
TABLE_SIZES = tuple(dict.fromkeys(m for m, _ in CASES))


def max_it(m, bits):
    return (1 << bits) // m


def _walk(cur, m, bits):
    mod = 1 << bits
    step = m % mod
    for it in range(max_it(m, bits)):
        if cur <= m:                                  # self.table.get(...): the keys are 0 .. m
            return (it * m + cur % mod) % mod
        cur = (cur - step) % L
    return None


def solve(v, m, bits):
    """solve_discrete_log_with_neg on the point v B -> the scalar it returns (an integer mod l), or None"""
    v %= L
    r = _walk(v, m, bits)
    if r is not None:
        return r
    r = _walk((-v) % L, m, bits)
    return None if r is None else (-r) % L


def edge_magnitudes(m, bits):
    """the magnitudes the issue lists (each is used with both signs): around the table's end, the giant steps j m for j = 1, 2 and
    max_it - 1, the entry x = m at the last iteration, around 2^bits, and one value that neither walk reaches"""
    mi = max_it(m, bits)
    step = m % (1 << bits)
    vals = [0, 1, m - 1, m, m + 1, 1 * m, 2 * m, (mi - 1) * m, (mi - 1) * m + m, (1 << bits) - 1, 1 << bits, (1 << bits) + 1,
            (mi - 1) * step + m + 1 + (1 << bits)]
    return list(dict.fromkeys(vals))


def unreachable(m, bits):
    """the last of edge_magnitudes: above the last entry of the last iteration by more than 2^bits, so None with either sign"""
    return edge_magnitudes(m, bits)[-1]


def giant_steps(m, bits, torsion_of, want=3, seed=1):
    """j values (1, 2, max_it - 1 first, then a seeded search) such that over the inputs +-j m the representative decode(enc(v B)) - v B
    takes at least `want` distinct values; torsion_of(v) names that value (tests/torsion_corpus.py decode_shift).  -> (js, set of names)"""
    mi = max_it(m, bits)
    js = [j for j in dict.fromkeys([1, 2, mi - 1]) if j >= 1]
    seen = set()
    for j in js:
        seen |= {torsion_of(j * m), torsion_of(-j * m)}
    rng = random.Random(seed * 1000003 + m * 64 + bits)
    for _ in range(64):
        if len(seen) >= want:
            break
        j = rng.randrange(1, max(mi, 8) + 1)
        if j in js:
            continue
        js.append(j)
        seen |= {torsion_of(j * m), torsion_of(-j * m)}
    return js, seen


def values(m, bits, torsion_of, seed=1):
    """every signed input of the case (m, bits), in a fixed order, without duplicates mod l"""
    js, _ = giant_steps(m, bits, torsion_of, seed=seed)
    mags = edge_magnitudes(m, bits) + [j * m for j in js]
    out = []
    for a in mags:
        for v in (a, -a):
            if v % L not in [x % L for x in out]:
                out.append(v)
    return out
