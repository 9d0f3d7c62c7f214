"""rofl_create_rangeproof_l2_batch (l2_range_proof_vec.create_rangeproof_l2_batch): the L2 sum proofs of several clients of one process in
one launch sequence -- k_l2_sumsq_batch (8 blocks of 256 per client, grid-stride: status bits, sum of squares as a 192-bit integer,
blinding sum, the per-element f32 terms of the shadow sum), the host's serial shadow sum and decision, one k_commit and one prove_chunks
over the surviving clients.  Every client's proof and commitment must be the bytes of its own single call (rofl_create_rangeproof_l2) and of
the CPU oracle (orc.create_rangeproof_l2), and every client's code the code of both, whatever its neighbours in the batch are.
The single call runs the same code as a group of one: "batch equals single" says that a client's neighbours do not matter, and the oracle
anchors the bytes and the codes of both.  The single call's own promises are here too: every outcome code with its rofl_last_error text,
the serial f32 shadow sum, a blinding >= l (every client's first), device-resident inputs.

Shapes: d around the block (255, 256, 257) and the wave (63, 64, 65), 1; d = 8 * 256 + 2, where the grid-stride loop wraps for two
threads; n = 2 and 17 (seventeen chunks of one value in one prove_chunks)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import orc

pytestmark = pytest.mark.gpu
SUM_BLOCKS = 8            # blocks of 256 per client in k_l2_sumsq_batch (kL2SumBlocks)
DS = (1, 63, 64, 65, 255, 256, 257, SUM_BLOCKS * 256 + 2)
CONFIGS = [((32, 7), 32), ((16, 7), 16), ((32, 7), 8)]


@pytest.fixture(scope="module")
def R():
    import rofl_project_code_amd as R
    from rofl_project_code_amd import build
    build.build()
    R.set_device(0)
    return R


def _nonce(R, i, mode, prove_range, short=False):
    """client i's prover randomness: (Nonce, the oracle's keyword)"""
    if mode == "seed":
        return R.Nonce.seeded(bytes([i + 1]) * 32), dict(seed=bytes([i + 1]) * 32)
    s = np.random.default_rng(9100 + i).integers(0, 256, size=64 * (2 * prove_range + 4 - (1 if short else 0)), dtype=np.uint8).tobytes()
    return R.Nonce.stream(s), dict(stream=s)


_inputs = {}


def _client(d, i):
    """(values, blindings) of client i at length d, made once and never written to: a dozen small values among zeros, so that the norm
    stays inside every bound of CONFIGS (sum k^2 <= 12 * 9 at 7 fractional bits: below 2^8 - 1)"""
    if (d, i) not in _inputs:
        rng = np.random.default_rng(7000 + 31 * d + i)
        k = np.zeros(d, np.int64)
        idx = rng.choice(d, size=min(d, 12), replace=False)
        k[idx] = rng.integers(-3, 4, size=idx.size)
        k[idx[0]] = 3 if i % 2 else -3      # (never all zero; negative values too)
        bl = rng.integers(0, 256, size=(d, 32), dtype=np.uint8); bl[:, 31] &= 0x0F
        bl[0] = 0xFF                        # a blinding >= l: reduced first, as the reference does
        _inputs[(d, i)] = ((k / 128.0).astype(np.float32), bl)
    return _inputs[(d, i)]


def _single(R, x, bl, prove_range, nonce, fp):
    """the single call's outcome: (0, proof, commit) or (code, None, None)"""
    try:
        p, c = R.l2_range_proof_vec.create_rangeproof_l2(x, bl, prove_range, 1, nonce=nonce, fp=fp)
        return 0, p, c
    except R.RoflError as e:
        return e.code, None, None


def _outcome(g):
    return (g.code, None, None) if isinstance(g, Exception) else (0, g[0], g[1])


def _equal(a, b):
    """two outcomes (code, proof, commit): the same code and, for code 0, the same bytes"""
    return a[0] == b[0] and (a[0] != 0 or (a[1].shape == b[1].shape and (a[1] == b[1]).all() and (np.asarray(a[2]) == np.asarray(b[2])).all()))


@pytest.mark.parametrize("mode", ["seed", "stream"])
@pytest.mark.parametrize("n,d", [(17, 65)] + [(2, d) for d in DS], ids=lambda v: str(v))
@pytest.mark.parametrize("fp,prove_range", CONFIGS, ids=lambda v: str(v))
def test_bytes_equal_the_single_call_and_the_oracle(R, fp, prove_range, n, d, mode):
    cl = [_client(d, i) for i in range(n)]
    got = R.l2_range_proof_vec.create_rangeproof_l2_batch([c[0] for c in cl], [c[1] for c in cl], prove_range, 1,
                                                          nonces=[_nonce(R, i, mode, prove_range)[0] for i in range(n)], fp=fp)
    assert len(got) == n
    for i in range(n):
        g = _outcome(got[i])
        assert g[0] == 0 and g[1].size == 32 * (9 + 2 * int(np.log2(prove_range))), (i, g[0])
        assert _equal(g, _single(R, cl[i][0], cl[i][1], prove_range, _nonce(R, i, mode, prove_range)[0], fp)), ("single call", i)
        assert _equal(g, orc.create_rangeproof_l2(cl[i][0], cl[i][1], prove_range, 1, fp[0], fp[1], **_nonce(R, i, mode, prove_range)[1])), ("oracle", i)
        assert orc.verify_rangeproof_l2(g[1], g[2], prove_range, fp[0], fp[1]) == (0, True)
    assert R.l2_range_proof_vec.verify_rangeproof_l2_batch([g[0] for g in got], np.stack([g[1] for g in got]), prove_range, verifier_seed=b"\x05" * 32, fp=fp) == [True] * n


@pytest.mark.parametrize("mode", ["seed", "stream"])
@pytest.mark.parametrize("d", DS)
@pytest.mark.parametrize("fp,prove_range", CONFIGS, ids=lambda v: str(v))
def test_the_single_call_equals_the_oracle(R, fp, prove_range, d, mode):
    """rofl_create_rangeproof_l2 alone against orc.create_rangeproof_l2 (client 0's blindings start with one >= l)"""
    x, bl = _client(d, 0)
    got = _single(R, x, bl, prove_range, _nonce(R, 0, mode, prove_range)[0], fp)
    assert got[0] == 0 and got[1].size == 32 * (9 + 2 * int(np.log2(prove_range)))
    assert _equal(got, orc.create_rangeproof_l2(x, bl, prove_range, 1, fp[0], fp[1], **_nonce(R, 0, mode, prove_range)[1]))
    assert orc.verify_rangeproof_l2(got[1], got[2], prove_range, fp[0], fp[1]) == (0, True)


TEXTS = {2: "ValueOutOfRangeError", 10: "non-finite value", 8: "OverflowError", 7: "NormOutOfRangeError", 3: "InvalidBitsize", 12: "nonce stream too short"}


def test_the_single_calls_outcomes_and_texts(R):
    """Every outcome of the single call with its rofl_last_error text, in the reference's order within a vector (ValueOutOfRange 2 wins over
    NaN 10 wherever they sit; then OverflowError 8, NormOutOfRange 7, InvalidBitsize 3): the code is the oracle's.  The short stream (12) is
    this library's own refusal -- the oracle reads zeros past the end of a stream -- and comes last: after the values' own outcomes."""
    d = 257
    cases = [((16, 7), 16, m[1], m[2]) for m in _parity_members(d)]                      # 0, 10, 2, 2, 8, 8 (16 bits cannot hold the sum), 12, 0
    cases += [((32, 7), 16, m[1], False) for m in _parity_members(d)[4:6]]               # norm 8.0 and [6, 6] where the sum fits: 7, 7
    cases.append(((16, 7), 24, _client(d, 0)[0], False))                                 # a bit size no proof can have
    cases.append(((16, 7), 24, _parity_members(d)[4][1], False))                         # ... after the norm
    cases.append(((32, 7), 32, (np.random.default_rng(4242).integers(200, 300, size=300) / 128.0).astype(np.float32), False))      # sum k^2 > 2^24
    cases.append(((16, 7), 16, _parity_members(d)[1][1], True))                          # a NaN before the stream's length
    seen = []
    for i, (fp, prove_range, x, short) in enumerate(cases):
        bl = _client(x.size, i % 2)[1]
        nonce, okw = _nonce(R, i % 7, "stream", prove_range, short=short)
        want = orc.create_rangeproof_l2(x, bl, prove_range, 1, fp[0], fp[1], **okw)[0]
        if short and want == 0:
            want = 12
        try:
            R.l2_range_proof_vec.create_rangeproof_l2(x, bl, prove_range, 1, nonce=nonce, fp=fp)
            code = 0
        except R.RoflError as e:
            code = e.code
            assert str(e) == "%s (%d): %s" % (e.name, code, TEXTS[code]), str(e)
        print("case", i, "single", code, "oracle", want)
        assert code == want, i
        seen.append(code)
    assert seen[:4] == [0, 10, 2, 2] and seen[6] == 12 and seen[-1] == 10 and set(seen) == {0, 2, 10, 8, 7, 3, 12}


def _parity_members(d):
    """the members of the outcome-parity batch: (name, values, short stream?)"""
    good0, good1 = _client(d, 0)[0], _client(d, 1)[0]
    nan = good0.copy(); nan[17] = np.nan
    out = good0.copy(); out[5] = 1000.0
    both = good0.copy(); both[3] = np.nan; both[200] = -1000.0
    norm = np.zeros(d, np.float32); norm[0] = 8.0          # l2_range_proof_vec/mod.rs:358-365 (test_rangeproof_bound_test_fail)
    six = np.zeros(d, np.float32); six[:2] = 6.0           # :367-373 (test_rangeproof_bound_test_fail_two)
    return [("good", good0, False), ("nan", nan, False), ("out of range", out, False), ("nan at 3, out of range at 200", both, False),
            ("norm 8.0", norm, False), ("[6, 6]", six, False), ("short stream", good1, True), ("good", good1, False)]


@pytest.mark.parametrize("prove_range", [16, 24])
def test_outcome_parity(R, prove_range):
    """rc_out[i] is the single call's code and the oracle's, member by member, in one batch at 16 bits (and at prove_range 24, which no proof
    can have: whatever the single call says first for each member).  The good members' bytes are their single calls'.  (The short
    stream is the one outcome the oracle does not have; see below.)"""
    fp, d = (16, 7), 257
    members = _parity_members(d)
    bls = [_client(d, i)[1] for i in range(len(members))]
    nonces = [_nonce(R, i, "stream", prove_range, short=m[2]) for i, m in enumerate(members)]
    got = R.l2_range_proof_vec.create_rangeproof_l2_batch([m[1] for m in members], bls, prove_range, 1, nonces=[nz[0] for nz in nonces], fp=fp)
    want = [_single(R, m[1], bls[i], prove_range, nonces[i][0], fp) for i, m in enumerate(members)]
    oracle = [orc.create_rangeproof_l2(m[1], bls[i], prove_range, 1, fp[0], fp[1], **nonces[i][1]) for i, m in enumerate(members)]
    codes = [_outcome(g)[0] for g in got]
    print("prove_range", prove_range, "batch", codes, "single", [w[0] for w in want], "oracle", [o[0] for o in oracle])
    assert codes == [w[0] for w in want]
    # the oracle knows every outcome but one: it reads zeros past the end of a stream (code 12 is this library's own refusal), so for the
    # short-stream member it is asked what it says about the VALUES -- 0 at a provable bit size -- and the 12 is the single call's
    short = [i for i, m in enumerate(members) if m[2]]
    assert [c for i, c in enumerate(codes) if i not in short] == [o[0] for i, o in enumerate(oracle) if i not in short]
    assert all(want[i][0] == (12 if oracle[i][0] == 0 else oracle[i][0]) for i in short)
    for i, m in enumerate(members):
        assert _equal(_outcome(got[i]), want[i]), m[0]
    if prove_range == 16:
        assert codes[0] == codes[7] == 0 and codes[1] == 10 and codes[2] == codes[3] == 2 and codes[6] == 12 and codes[4] != 0 and codes[5] != 0


def test_the_shadow_sums_order(R):
    """fp (32, 7), prove_range 32, d = 300.  Client 0: k in [1, 30), sum k^2 < 2^24 -- every partial f32 sum is exact, the oracle proves it
    (code 0).  Client 1: k in [200, 300), sum k^2 = ~1.9e7 > 2^24 -- the serial f32 sum rounds on the way and misses the scalar sum by more
    than f32 epsilon: the oracle answers 8 (OverflowError).  A tree sum or a device reduction would round elsewhere; the batch adds the
    terms on the host in the reference's order and must say what the single call and the oracle say, code or bytes."""
    fp, prove_range, d = (32, 7), 32, 300
    rng = np.random.default_rng(4242)
    xs = [(rng.integers(1, 30, size=d) / 128.0).astype(np.float32), (rng.integers(200, 300, size=d) / 128.0).astype(np.float32)]
    bls = [_client(d, i)[1] for i in range(2)]
    k2 = [int((np.round(x.astype(np.float64) * 128).astype(np.int64) ** 2).sum()) for x in xs]
    assert k2[0] < 2 ** 24 < k2[1]
    oracle = [orc.create_rangeproof_l2(xs[i], bls[i], prove_range, 1, fp[0], fp[1], seed=bytes([i + 1]) * 32) for i in range(2)]
    print("sum k^2", k2, "oracle codes", [o[0] for o in oracle])
    assert [o[0] for o in oracle] == [0, 8]      # (what the oracle said when this test was written; the assertions below do not depend on it)
    got = R.l2_range_proof_vec.create_rangeproof_l2_batch(xs, bls, prove_range, 1, nonces=[_nonce(R, i, "seed", prove_range)[0] for i in range(2)], fp=fp)
    for i in range(2):
        assert _equal(_single(R, xs[i], bls[i], prove_range, _nonce(R, i, "seed", prove_range)[0], fp), oracle[i]), ("single call against the oracle", i)
        assert _equal(_outcome(got[i]), oracle[i]), ("oracle", i)
        assert _equal(_outcome(got[i]), _single(R, xs[i], bls[i], prove_range, _nonce(R, i, "seed", prove_range)[0], fp)), ("single call", i)


def test_device_resident_inputs():
    """One client's values and blindings as device pointers (torch tensors on the GPU), its neighbour's in host memory: same bytes.
    (Own process: torch has to bring up its HIP runtime before the library's is loaded.)"""
    r = subprocess.run([sys.executable, os.path.join(os.path.dirname(__file__), "gpu_l2_create_batch_device_check.py")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "DEVICE_INPUTS PASS" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


def test_the_single_call_takes_device_resident_inputs():
    """rofl_create_rangeproof_l2 (the C entry itself) on device-resident values and blindings: the oracle's bytes.  (Before the single call
    became a group of one it read values[i] on the host: this case cannot run there.)"""
    r = subprocess.run([sys.executable, os.path.join(os.path.dirname(__file__), "gpu_l2_create_batch_device_check.py"), "--single"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "SINGLE_DEVICE_INPUTS PASS" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
