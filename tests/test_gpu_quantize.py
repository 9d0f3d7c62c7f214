"""Every device site of the float-to-fixed rule (conversion32.rs:11-18) at ties, the closed clip bounds and saturation, ON THE DEVICE.

Directly, through rofl_dbg_quantize, for all 47 supported formats and every range nb <= fp_bits: k_quantize_shift (site 0), k_l2_sumsq_batch +
k_l2_sumsq_combine (site 1) and sg_f32_to_sc (site 2) against the exact model of tests/quant_model.py.  Then through the operator API at the
smallest shapes, bit for bit against the oracle under a seeded nonce: create_rangeproof (single, batch), the Sigma-proof vectors and the
CompressedRandProof (single, batch), create_rangeproof_l2 (single, batch) and EncParamsRange.  Integers only: every assertion is equality.

The closed bound matters: at a 32-bit (and 64-bit) range get_clip_bounds rounds up to a power of two in f32, +max quantizes to 2^(nb-1), the
shift wraps it to 0 and it commits as -max; the reference's composition then rejects the update.  That is the reference's behaviour (pinned
on the oracle in tests/test_quantize_host.py); the tests here hold the HIP path to it."""
import ctypes
import math

import numpy as np
import pytest

import orc
import quant_model as m
from test_quantize_host import _bits, _sc, full_corpus

pytestmark = pytest.mark.gpu
TPB, L2_BLOCKS = 256, 8      # csrc/kernels.hpp TPB, csrc/rofl_zk.hip kL2SumBlocks
FP_IDS = ["fp%d_%d" % p for p in m.VALID_FP]
sz = ctypes.c_size_t


@pytest.fixture(scope="module")
def R():
    import rofl_project_code_amd as R
    from rofl_project_code_amd import build
    build.build()
    R.set_device(0)     # fails loudly when there is no HIP device / library
    yield R
    R.api.set_fp(16, 7)


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def dbg_quantize(R, site, vals, nb, fb, ff, dpad=0, blind=None):
    """rofl_dbg_quantize on vals[rows][d] -> site 0: (vshift u64[rows][dpad], status); 1: (terms, sums u8[rows][2][32], status); 2: scalars u8[rows][d][32]"""
    vals = np.ascontiguousarray(vals, np.float32)
    rows, d = vals.shape
    status = np.full(rows, 0xdeadbeef, np.uint32)
    terms = np.full((rows, d), np.nan, np.float32)
    out = {0: np.full((rows, max(dpad, 1)), 0xdeadbeefdeadbeef, np.uint64), 1: np.full((rows, 2, 32), 0xee, np.uint8), 2: np.full((rows, d, 32), 0xee, np.uint8)}[site]
    rc = R.lib().rofl_dbg_quantize(ctypes.c_uint(site), sz(rows), sz(d), sz(dpad), sz(nb), ctypes.c_uint(fb), ctypes.c_uint(ff), _p(vals), _p(blind), _p(out), _p(terms), _p(status))
    assert rc == 0
    return {0: (out, status), 1: (terms, out, status), 2: out}[site]


def ranges(fb):
    return [nb for nb in m.RANGES if nb <= fb]


def cyc(src, n, off=0):
    return np.array([src[(off + i) % len(src)] for i in range(n)], np.float32)


# ---------------------------------------------------------------- site 0: k_quantize_shift
@pytest.mark.parametrize("fb,ff", m.VALID_FP, ids=FP_IDS)
def test_quantize_shift_kernel(R, fb, ff):
    for nb in ranges(fb):
        vals, nans, inr = m.corpus(fb, ff, nb)
        mx = m.f32(m.clip_bounds(nb, fb, ff)[1] + 1)
        # rows of three values (a status is attributable to them), one padding word; the corpus, the NaNs, and NaN beside an out-of-range value
        flat = np.concatenate([vals, nans])
        flat = np.concatenate([flat, np.zeros(-flat.size % 3, np.float32), np.array([nans[0], mx, 1.0, -mx, nans[1], 0.0], np.float32)]).reshape(-1, 3)
        # and rows that cross a block: the in-range values, one of them with a flagged value in the second block
        long = np.stack([cyc(inr, TPB + 1), cyc(inr, TPB + 1, 5)]); long[1, TPB] = mx
        seen = set()
        for rows, dpad in ((flat, 4), (long, 2 * TPB)):
            got, st = dbg_quantize(R, 0, rows, nb, fb, ff, dpad=dpad)
            bits = [[m.status(v, nb, fb, ff) for v in row] for row in rows]
            want = np.zeros_like(got)                                        # (the padding words i >= d stay 0)
            for i, row in enumerate(rows):
                for j, v in enumerate(row):
                    want[i, j] = 0 if bits[i][j] else m.shifted(v, nb, fb, ff)
            assert (got == want).all(), (nb, np.argwhere(got != want)[:4])
            assert st.tolist() == [int(np.bitwise_or.reduce(b)) for b in bits], nb
            seen |= set(st.tolist())
        assert seen == {0, 1, 2, 3}, nb      # (every kind of row was there)


# ---------------------------------------------------------------- site 2: sg_f32_to_sc
@pytest.mark.parametrize("fb,ff", m.VALID_FP, ids=FP_IDS)
def test_sigma_quantizer(R, fb, ff):
    """the full un-clipped corpus -- infinities, FLT_MAX, subnormals, the zeros, negatives that quantize to zero (0, not l) -- against the model and,
    bit for bit, the host copy; more than one block"""
    vals = full_corpus(fb, ff)
    vals = cyc(vals, max(vals.size, 2 * TPB + 3))[None, :]
    got = dbg_quantize(R, 2, vals, 8, fb, ff)
    want = _sc([m.scalar(v, fb, ff) for v in vals.reshape(-1)]).reshape(got.shape)
    assert (got == want).all(), np.argwhere((got != want).any(axis=2))[:4]
    assert (got.reshape(-1, 32) == R.conversion32.f32_to_scalar_vec(vals.reshape(-1), fp=(fb, ff))).all()


# ---------------------------------------------------------------- site 1: k_l2_sumsq_batch + k_l2_sumsq_combine
def all_ones_terms():
    """k_i of at most 24 significant bits (each is some f32 times 2^ff) with sum k_i^2 = 2^128 - 1: greedily the largest such k below the root of the rest"""
    rest, ks = 2 ** 128 - 1, []
    while rest:
        k = math.isqrt(rest)
        k = k >> max(k.bit_length() - 24, 0) << max(k.bit_length() - 24, 0)
        ks.append(k); rest -= k * k
    assert sum(k * k for k in ks) == 2 ** 128 - 1 and len(ks) <= 24
    return ks


def l2_blocks(d):
    return min(L2_BLOCKS, (d + TPB - 1) // TPB)


def all_ones_row(d, ff):
    """A row whose sum of squares is 2^128 - 1 before the LAST 192-bit addition, which adds 1: both carries ripple, the second through the
    limb that the first made zero.  d <= TPB: one block, the last addition of the tree adds the odd threads' sum to the even threads' (the
    terms sit at even indices, the 1 at index 1).  d > TPB: k_l2_sumsq_combine adds the blocks' partial sums in order (the terms sit in block 0,
    the 1 in the last block)."""
    ks, row = all_ones_terms(), np.zeros(d, np.float32)
    idx = [2 * i for i in range(len(ks))] if d <= TPB else list(range(len(ks)))
    for i, k in zip(idx, ks):
        row[i] = m.f32(m.round_f32(m.Fraction(k, 1 << ff)))
    row[1 if d <= TPB else (l2_blocks(d) - 1) * TPB] = m.f32(m.round_f32(m.Fraction(1, 1 << ff)))
    return row


@pytest.mark.parametrize("fb,ff", m.VALID_FP, ids=FP_IDS)
def test_l2_sum_kernels(R, fb, ff):
    """terms bit-equal to the model, the sum of squares the exact integer (across 2^64 and 2^128), blinding sums mod l with inputs >= l, status per row:
    one value, one block less one / exactly / plus one thread, and a second, partial pass of the grid-stride loop"""
    rng = np.random.default_rng(fb * 16 + ff)
    term, kk, stat = {}, {}, {}
    for nb in ranges(fb):
        vals, nans, inr = m.corpus(fb, ff, nb)
        sat = np.array([np.inf, -np.inf], np.float32)
        for d in (1, TPB - 1, TPB, TPB + 1, L2_BLOCKS * TPB + 5):
            rows = [cyc(vals, d, d), cyc(inr, d, 1), cyc(sat, d), cyc(inr, d, 2), cyc(inr, d, 3)]
            rows[3][0] = nans[0]; rows[3][d - 1] = nans[d % 4]; rows[3][d // 2] = nans[2]
            if fb == 64 and d >= 64:
                rows[4] = all_ones_row(d, ff)
                assert sum(m.fix_bits(v, fb, ff) ** 2 for v in rows[4]) == 2 ** 128
            rows = np.stack(rows)
            bl = rng.integers(0, 256, size=(rows.shape[0], d, 32), dtype=np.uint8)
            for j, s in enumerate((2 ** 256 - 1, m.L, m.L + 1, m.L - 1, 0, 2 ** 255)):      # (inputs at and above l: reduced first)
                bl[j % rows.shape[0], (7 * j) % d] = m.scalar_bytes(s)
            terms, sums, st = dbg_quantize(R, 1, rows, nb, fb, ff, blind=bl)
            for i, row in enumerate(rows):
                for b in set(_bits(row).tolist()) - set(term):
                    nan = m.is_nan(b)
                    term[b], kk[b] = (0 if nan else m.l2_term(b, fb, ff)), (0 if nan else m.fix_bits(b, fb, ff))      # (the kernel takes k = 0 for a NaN; its client is rejected)
                rb = _bits(row).tolist()
                assert _bits(terms[i]).tolist() == [term[b] for b in rb], (nb, d, i)
                assert int.from_bytes(sums[i, 0].tobytes(), "little") == sum(kk[b] ** 2 for b in rb), (nb, d, i)
                assert int.from_bytes(sums[i, 1].tobytes(), "little") == sum(int.from_bytes(x.tobytes(), "little") for x in bl[i]) % m.L, (nb, d, i)
                for b in set(rb):
                    if (b, nb) not in stat:
                        stat[b, nb] = m.status(b, nb, fb, ff)
                assert int(st[i]) == int(np.bitwise_or.reduce([stat[b, nb] for b in set(rb)])), (nb, d, i)
            assert st[1] == 0 and st[2] == 1 and st[3] == 2
            if fb == 64 and d > 1:      # the rows of saturated values cross 2^128
                assert int.from_bytes(sums[2, 0].tobytes(), "little") == d * (2 ** 64 - 1) ** 2 > 2 ** 128


def test_hook_rejects_bad_parameters(R):
    v = np.zeros((2, 3), np.float32); out = np.zeros((2, 4, 32), np.uint8); st = np.zeros(2, np.uint32); t = np.zeros((2, 3), np.float32); bl = np.zeros((2, 3, 32), np.uint8)
    def call(site=0, rows=2, d=3, dpad=4, nb=8, fb=16, ff=7, vals=v, blind=bl, o=out, terms=t, status=st):
        return R.lib().rofl_dbg_quantize(ctypes.c_uint(site), sz(rows), sz(d), sz(dpad), sz(nb), ctypes.c_uint(fb), ctypes.c_uint(ff), _p(vals), _p(blind), _p(o), _p(terms), _p(status))
    assert call() == 0 and call(site=1) == 0 and call(site=2) == 0
    for bad in (dict(site=3), dict(rows=0), dict(d=0), dict(dpad=2), dict(nb=0), dict(nb=17), dict(fb=24), dict(fb=16, ff=13), dict(fb=8, ff=8), dict(vals=None), dict(o=None),
                dict(status=None), dict(site=1, blind=None), dict(site=1, terms=None), dict(site=1, nb=129), dict(rows=1 << 21)):
        assert call(**bad) == 11, bad


# ---------------------------------------------------------------- create_rangeproof
RANGE_CASES = [(8, 8, 3), (8, 16, 7), (16, 16, 7), (32, 32, 7), (32, 32, 12), (64, 64, 7), (64, 64, 12)]


@pytest.mark.parametrize("nb,fb,ff", RANGE_CASES, ids=["n%d_fp%d_%d" % c for c in RANGE_CASES])
def test_create_rangeproof_on_the_in_range_corpus(R, nb, fb, ff):
    vals = m.corpus(fb, ff, nb)[2]
    d, P, seed = vals.size, 4, bytes([nb, fb, ff]) * 10 + b"\0\0"
    mn_b, mx_b = m.clip_bounds(nb, fb, ff)
    ip, im = _bits(vals).tolist().index(mx_b), _bits(vals).tolist().index(mn_b)      # both closed bounds are in
    bl = orc.rand_scalars(np.random.default_rng(nb + fb + ff), d); bl[im] = bl[ip]
    pr, cm = R.range_proof_vec.create_rangeproof(vals, bl, nb, P, nonce=R.Nonce.seeded(seed), fp=(fb, ff))
    rc, opr, ocm = orc.create_rangeproof(vals, bl, nb, P, fb, ff, seed=seed)
    assert rc == 0 and (pr == opr).all() and (cm == ocm).all()
    assert R.range_proof_vec.verify_rangeproof(pr, cm, nb, fp=(fb, ff)) and orc.verify_rangeproof(pr, cm, nb, fb, ff) == (0, True)
    assert R.range_proof_vec.verify_rangeproof(opr, ocm, nb, fp=(fb, ff))
    # +max commits as -max exactly when the shift wraps it
    same = m.shifted(m.f32(mx_b), nb, fb, ff) == m.shifted(m.f32(mn_b), nb, fb, ff)
    assert bool((cm[ip] == cm[im]).all()) == same and same == (nb >= 32)
    # against what an ElGamal L of the same plaintext and blinding is, commit(f32_to_scalar(v), r): rejected exactly when a value wrapped
    wraps = [(m.scalar(v, fb, ff) + (1 << (nb - 1))) % m.L != m.shifted(v, nb, fb, ff) for v in vals]
    assert wraps.count(True) == (1 if same else 0) and wraps[ip] == same
    eg = orc.commit_vec(_sc([m.scalar(v, fb, ff) for v in vals]), bl)
    assert [i for i in range(d) if (eg[i] != cm[i]).any()] == [i for i in range(d) if wraps[i]]
    assert R.range_proof_vec.verify_rangeproof(pr, eg, nb, fp=(fb, ff)) == (not same)
    assert orc.verify_rangeproof(pr, eg, nb, fb, ff) == (0, not same)


def _outcome(fn):
    try:
        return fn()
    except Exception as e:      # RoflError: compared by its code
        return e


def _same(a, b):
    if isinstance(a, Exception) or isinstance(b, Exception):
        return isinstance(a, Exception) and isinstance(b, Exception) and a.code == b.code
    return all((np.asarray(x) == np.asarray(y)).all() for x, y in zip(a, b))


def test_create_rangeproof_batch_at_the_closed_bound(R):
    nb, fb, ff, P, d = 32, 32, 7, 2, 6
    mn_b, mx_b = m.clip_bounds(nb, fb, ff)
    mx, mn, out, nan = m.f32(mx_b), m.f32(mn_b), m.f32(mx_b + 1), np.float32(np.nan)
    members = [np.array([1, -1, 0.5, -0.0, 3.0, 100.25], np.float32), np.array([mx, mn, 1, -1, mx, 0], np.float32),
               np.array([1, 2, out, 3, 4, 5], np.float32), np.array([1, nan, 2, -out, 3, 4], np.float32)]
    rng = np.random.default_rng(5)
    bls = [orc.rand_scalars(rng, d) for _ in members]
    seeds = [bytes([0x60 + i]) * 32 for i in range(4)]
    got = R.range_proof_vec.create_rangeproof_batch(members, bls, nb, P, nonces=[R.Nonce.seeded(s) for s in seeds], fp=(fb, ff))
    codes = []
    for i, v in enumerate(members):
        one = _outcome(lambda: R.range_proof_vec.create_rangeproof(v, bls[i], nb, P, nonce=R.Nonce.seeded(seeds[i]), fp=(fb, ff)))
        rc, opr, ocm = orc.create_rangeproof(v, bls[i], nb, P, fb, ff, seed=seeds[i])
        assert _same(got[i], one), i
        codes.append(getattr(got[i], "code", 0))
        assert codes[-1] == rc
        if rc == 0:
            assert (got[i][0] == opr).all() and (got[i][1] == ocm).all()
    assert codes == [0, 0, 2, 2]      # (out of range wins over the NaN in front of it)


# ---------------------------------------------------------------- Sigma-proof vectors and the CompressedRandProof: the un-clipped plaintext
SIGMA_FP = [(16, 7), (32, 12), (64, 7)]


def _sigma_api(R, kind):
    if kind == 0:
        return (lambda v, r1, r2, n, fp: R.rand_proof_vec.create_randproof_vec(v, r1, nonce=n, fp=fp),
                lambda vs, r1s, r2s, ns, fp: R.rand_proof_vec.create_randproof_vec_batch(vs, r1s, nonces=ns, fp=fp), R.rand_proof_vec.verify_randproof_vec)
    cls = R.square_rand_proof_vec if kind == 1 else R.square_proof_vec
    return (lambda v, r1, r2, n, fp: cls.create_l2rangeproof_vec(v, r1, r2, nonce=n, fp=fp),
            lambda vs, r1s, r2s, ns, fp: cls.create_l2rangeproof_vec_batch(vs, r1s, r2s, nonces=ns, fp=fp), cls.verify_l2rangeproof_vec)


def _with_nan(v, i):
    w = v.copy(); w[i] = np.nan
    return w


@pytest.mark.parametrize("fb,ff", SIGMA_FP, ids=["fp%d_%d" % p for p in SIGMA_FP])
@pytest.mark.parametrize("kind", [0, 1, 2, 3], ids=["rand", "square_rand", "square", "compressed"])
def test_sigma_creators_on_the_unclipped_corpus(R, kind, fb, ff):
    """single and batch creators: the full corpus (infinities, FLT_MAX, subnormals, the zeros, negatives that quantize to zero) and its reverse are
    proved as the oracle proves them and both verifiers accept; a NaN at the first, a middle or the last index is error 10 for its member alone"""
    fp = (fb, ff)
    v0 = full_corpus(fb, ff)
    d = TPB + 9                                      # more than one block of threads, whatever the kernel's unit is
    assert v0.size <= d
    v0 = cyc(v0, d)
    rng = np.random.default_rng(100 * kind + fb + ff)
    members = [v0, v0[::-1].copy(), _with_nan(v0, 0), _with_nan(v0, d // 2), _with_nan(v0, d - 1)]
    r1 = [orc.rand_scalars(rng, d) for _ in members]
    r2 = [orc.rand_scalars(rng, d) for _ in members]
    seeds = [bytes([0x70 + 8 * kind + i]) * 32 for i in range(len(members))]
    if kind == 3:
        single = lambda v, a, b, n, fp: R.compressed_rand_proof.helper_prove(v, a, nonce=n, fp=fp)
        batch = lambda vs, a, b, ns, fp: R.compressed_rand_proof.helper_prove_batch(vs, a, nonces=ns, fp=fp)
        verify, ocreate, overify = R.compressed_rand_proof.helper_verify, (lambda v, a, b, s: orc.compressed_create(v, a, fb, ff, seed=s)), orc.compressed_verify
    else:
        single, batch, verify = _sigma_api(R, kind)
        ocreate, overify = (lambda v, a, b, s: orc.sigma_create(kind, v, a, b if kind else None, fb, ff, seed=s)), (lambda p, c: orc.sigma_verify(kind, p, c))
    got = batch(members, r1, r2, [R.Nonce.seeded(s) for s in seeds], fp)
    for i, v in enumerate(members):
        one = _outcome(lambda: single(v, r1[i], r2[i], R.Nonce.seeded(seeds[i]), fp))
        rc, opf, ocm = ocreate(v, r1[i], r2[i], seeds[i])
        assert _same(got[i], one), i
        assert getattr(one, "code", 0) == rc == (0 if i < 2 else 10), i
        if rc == 0:
            assert (one[0] == opf).all() and (one[1] == ocm).all(), i
            assert verify(one[0], one[1]) and overify(one[0], one[1]) == (0, True), i


# ---------------------------------------------------------------- create_rangeproof_l2
@pytest.mark.parametrize("nb,fb,ff", m.L2_FORMATS, ids=["n%d_fp%d_%d" % c for c in m.L2_FORMATS])
def test_create_rangeproof_l2_outcomes(R, nb, fb, ff):
    """single and batch: the bytes where the oracle proves, its error code where it does not (tests/test_quantize_host.py holds the vectors to
    every outcome: 0, 2, 7, 8, 10)"""
    fp = (fb, ff)
    vecs = m.l2_vectors(nb, fb, ff)
    want, one = [], []
    for k, v in enumerate(vecs):
        bl = orc.rand_scalars(np.random.default_rng(k), v.size)
        seed = bytes([0x40 + k]) * 32
        rc, opr, ocm = orc.create_rangeproof_l2(v, bl, nb, 1, fb, ff, seed=seed)
        got = _outcome(lambda: R.l2_range_proof_vec.create_rangeproof_l2(v, bl, nb, 1, nonce=R.Nonce.seeded(seed), fp=fp))
        assert getattr(got, "code", 0) == rc, (k, v[:5])
        if rc == 0:
            assert (got[0] == opr).all() and (got[1] == ocm).all(), k
            assert R.l2_range_proof_vec.verify_rangeproof_l2(got[0], got[1], nb, fp=fp) and orc.verify_rangeproof_l2(got[0], got[1], nb, fb, ff) == (0, True)
        want.append((bl, seed)); one.append(got)
    for d in (1, 2, 5, 64):
        idx = [k for k, v in enumerate(vecs) if v.size == d]
        got = R.l2_range_proof_vec.create_rangeproof_l2_batch([vecs[k] for k in idx], [want[k][0] for k in idx], nb, 1, nonces=[R.Nonce.seeded(want[k][1]) for k in idx], fp=fp)
        for k, g in zip(idx, got):
            assert _same(g, one[k]), k


# ---------------------------------------------------------------- EncParamsRange at the closed bound
def test_enc_params_range_at_the_closed_bound(R):
    """nb 32, fp (32, 7), everything checked: the range proof is over the clipped values, the ElGamal pairs and the rand proofs over the plaintext,
    completing the range proof's commitments.  +max is inside the clip range and yet the container does not verify (+max commits as -max in the
    range proof, the rand proof is about 2^31 B); -max verifies; 1e12 is clipped (to +max) and does not."""
    from test_gpu_params import _sub
    nb, fb, ff, P = 32, 32, 7, 2
    fp = (fb, ff)
    R.api.set_fp(fb, ff)
    try:
        mn_b, mx_b = m.clip_bounds(nb, fb, ff)
        cases = [np.array([1.5, m.f32(mx_b), -2.0], np.float32), np.array([0.25, -1.0, m.f32(mn_b), 7.0], np.float32), np.array([1.0, -3.0, 0.5, 1e12, 2.0], np.float32)]
        verdicts = []
        for c, x in enumerate(cases):
            d = x.size
            bl = orc.rand_scalars(np.random.default_rng(40 + c), d)
            seed = bytes([0x50 + c]) * 32
            enc = R.EncParamsRange.encrypt(x, bl, nb, P, 1.0, nonce_seed=seed, fp=fp)
            clipped = np.zeros_like(x)
            orc.lib().orc_clip_f32(_p(x), sz(d), nb, fb, ff, _p(clipped))
            assert (_bits(clipped) == [mx_b if m.status(v, nb, fb, ff) else b for v, b in zip(x, _bits(x))]).all()
            rc, opr, ocm = orc.create_rangeproof(clipped, bl, nb, P, fb, ff, seed=_sub(seed, b"range", x, bl))
            assert rc == 0 and (enc.range_proofs == opr).all()
            rc, opf, opairs = orc.sigma_create(0, x, bl, None, fb, ff, seed=_sub(seed, b"rand", x, bl), existing=ocm)
            assert rc == 0 and (enc.rand_proofs == opf).all() and (enc.enc_values == opairs).all()
            back = R.EncParamsRange.deserialize(enc.serialize())
            o_rand, o_range = orc.sigma_verify(0, opf, opairs), orc.verify_rangeproof(opr, opairs[:, :32].copy(), nb, fb, ff)
            assert o_rand[0] == 0 and o_range == (0, True)
            assert back.verify(verifier_seed=b"\x07" * 32, fp=fp) == (o_rand[1] and o_range[1])
            verdicts.append(o_rand[1] and o_range[1])
            # the batch entry and the compressed container complete the same commitments
            (eb,) = R.EncParamsRange.encrypt_batch([(x, bl)], nb, P, 1.0, nonce_seeds=[seed], fp=fp)
            assert eb.serialize() == enc.serialize()
            comp = R.EncParamsRangeCompressed.encrypt(x, bl, nb, P, 1.0, nonce_seed=seed, fp=fp)
            rc, ocp, ocpairs = orc.compressed_create(x, bl, fb, ff, seed=_sub(seed, b"rand", x, bl), existing=ocm)
            assert rc == 0 and (comp.range_proofs == opr).all() and (comp.rand_proof == ocp).all() and (comp.enc_values == ocpairs).all()
            assert comp.verify(verifier_seed=b"\x07" * 32, fp=fp) == (orc.compressed_verify(ocp, ocpairs)[1] and o_range[1]) == verdicts[-1]
        assert verdicts == [False, True, False]
    finally:
        R.api.set_fp(16, 7)
