"""The server's side of a round of L-inf updates (EncModelParams::verify, EncRange / EncRangeCompressed arms, params.rs:185-203 and
:235-256, for every client of a round, server.rs:656-687): rofl_verify_compressed_randproof_batch (compressed_rand_proof.helper_verify_batch)
and EncParamsRange{,Compressed}.verify_batch.  Every verdict equals the single-update path's (helper_verify, verify()), tampered members are
caught one by one, the oracle agrees on every compressed proof at small d, and the verdicts do not change when the clients are dealt to two
logical devices."""
import os
import sys

import numpy as np
import pytest

import orc

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import pyref  # noqa: E402  (pure-Python Merlin)

pytestmark = pytest.mark.gpu
FP = (16, 7)
ELL = 2 ** 252 + 27742317777372353535851937790883648493
BAD_POINT = np.frombuffer(bytes([1] + [0] * 31), np.uint8)      # odd s: not a Ristretto encoding


@pytest.fixture(scope="module")
def R():
    import rofl_project_code_amd as R
    from rofl_project_code_amd import build
    build.build()
    R.set_device(0)
    yield R
    R.set_option("devices", 0)


def _blindings(rng, d):
    bl = rng.integers(0, 256, size=(d, 32), dtype=np.uint8)
    bl[:, 31] &= 0x0F      # < 2^252 < l: canonical
    return bl


def _proofs(R, n, d, seed0):
    out = []
    for i in range(n):
        rng = np.random.default_rng(seed0 + i)
        x = (rng.integers(-1000, 1000, size=d) / 128.0).astype(np.float32)
        pf, pairs = R.compressed_rand_proof.helper_prove(x, _blindings(rng, d), nonce=R.Nonce.seeded(bytes([(seed0 + i) % 251]) * 32), fp=FP)
        out.append((pf.copy(), np.ascontiguousarray(pairs)))
    return out


def _single(R, pf, pairs):
    """helper_verify's verdict; its FormatError (a malformed member) counts as False"""
    try:
        return R.compressed_rand_proof.helper_verify(pf, pairs)
    except R.RoflError as e:
        assert e.code == 5, e
        return False


def _zm_plus_one(pf):
    z = (int.from_bytes(pf[64:96].tobytes(), "little") + 1) % ELL
    pf[64:96] = np.frombuffer(z.to_bytes(32, "little"), np.uint8)


def _tampered(cl, d):
    """one member tampered per kind; returns (proofs, pairs, the members that must fail)"""
    pf = [p.copy() for p, _ in cl]
    pr = [c.copy() for _, c in cl]
    _zm_plus_one(pf[1])                                                  # Z_m + 1
    pf[2][96:128] = cl[3][0][96:128]                                     # Z_r of another client
    pf[4][0:32] = cl[5][0][0:32]                                         # C'.L: a valid point, another client's
    pr[6][d // 2, :32] = cl[7][1][d // 2, :32]                           # one pair's L replaced by a valid foreign point
    pr[8][d - 1, 32:64] = BAD_POINT                                      # one pair's R undecodable
    pf[10][96:128] = 0xFF                                                # Z_r not canonical
    return pf, pr, {1, 2, 4, 6, 8, 10}


def test_twelve_clients_at_the_e2e_size(R):
    d, n = 40000, 12
    cl = _proofs(R, n, d, 10)
    H = R.compressed_rand_proof.helper_verify_batch
    assert H([p for p, _ in cl], [c for _, c in cl]) == [True] * n
    pf, pr, bad = _tampered(cl, d)
    got = H(pf, pr)
    assert got == [i not in bad for i in range(n)]
    assert got == [_single(R, p, c) for p, c in zip(pf, pr)]


def _forged(R, d, seed, bad):
    """A proof made in Python over d pairs whose pair `bad` is undecodable in both halves, with that pair left out of Z_m and Z_r: it passes
    both equations if the pair counts as the identity -- only the pair's decoding status rejects it (the single call: FormatError).
    bad = None: the same construction over honest pairs, which must verify."""
    rng = np.random.default_rng(seed)
    x = (rng.integers(-1000, 1000, size=d) / 128.0).astype(np.float32)
    bl = _blindings(rng, d)
    _, pairs = R.compressed_rand_proof.helper_prove(x, bl, nonce=R.Nonce.seeded(bytes([seed % 251]) * 32), fp=FP)
    pairs = np.ascontiguousarray(pairs).copy()
    m = R.conversion32.f32_to_scalar_vec(x, fp=FP)
    if bad is not None:
        pairs[bad, :32] = BAD_POINT
        pairs[bad, 32:] = BAD_POINT
    nz = _blindings(rng, 2)      # m', r'
    cprime = np.concatenate([R.pedersen_ops.commit_vec(nz[:1], nz[1:]).reshape(32), R.pedersen_ops.commit_no_blinding_vec(nz[1:]).reshape(32)])
    t = pyref.Transcript(b"CompressedRandProof")
    t.append_message(b"dom-sep", b"randomness proof v1")
    for i in range(d):
        t.append_message(bytes([(3 * i) % 256, (3 * i + 1) % 256, (3 * i + 2) % 256]), pairs[i].tobytes())
    t.append_message(b"C_prime_eg", cprime.tobytes())
    c = t.challenge_scalar(b"c")
    le = lambda a: int.from_bytes(bytes(a), "little")
    zm, zr, ci = le(nz[0]), le(nz[1]), c
    for i in range(d):
        if i != bad:
            zm, zr = zm + ci * le(m[i]), zr + ci * le(bl[i])
        ci = ci * c % ELL
    z = np.frombuffer((zm % ELL).to_bytes(32, "little") + (zr % ELL).to_bytes(32, "little"), np.uint8)
    return np.concatenate([cprime, z]), pairs


def test_forty_clients_in_three_groups(R):
    """40 clients = groups of 16, 16 and 8: members tampered in the second and third groups are caught one by one, among them proofs that
    treat an undecodable pair as the identity (rejected only through their client's status word); the same over two logical devices
    (shards of 20 = two groups each)"""
    from rofl_project_code_amd import api
    d, n = 300, 40
    cl = _proofs(R, n, d, 300)
    pf, pr = [p.copy() for p, _ in cl], [c.copy() for _, c in cl]
    pr[17][40, 32:64] = BAD_POINT                   # group 2: an undecodable R
    _zm_plus_one(pf[21])                            # group 2: Z_m + 1
    pr[26][7, :32] = cl[27][1][7, :32]              # group 2: a foreign L
    pf[30], pr[30] = _forged(R, d, 930, 123)        # group 2: the undecodable pair left out of the responses
    pr[33][299, :32] = BAD_POINT                    # group 3: an undecodable L
    _zm_plus_one(pf[36])                            # group 3: Z_m + 1
    pr[38][150, :32] = cl[0][1][150, :32]           # group 3: a foreign L
    pf[39], pr[39] = _forged(R, d, 939, 0)          # group 3
    pf[5], pr[5] = _forged(R, d, 905, None)         # group 1: the same construction without a bad pair verifies
    bad = {17, 21, 26, 30, 33, 36, 38, 39}
    H = R.compressed_rand_proof.helper_verify_batch
    got = H(pf, pr)
    assert got == [i not in bad for i in range(n)]
    assert got == [_single(R, p, c) for p, c in zip(pf, pr)]
    for i in (30, 39):
        with pytest.raises(R.RoflError) as e:
            R.compressed_rand_proof.helper_verify(pf[i], pr[i])
        assert e.value.code == 5
    api.map_device(1, 0)
    try:
        R.set_option("devices", 0b11)
        assert H(pf, pr) == got
    finally:
        R.set_option("devices", 0)


def test_the_oracle_agrees_at_small_d(R):
    d, n = 1500, 12
    pf, pr, bad = _tampered(_proofs(R, n, d, 40), d)
    got = R.compressed_rand_proof.helper_verify_batch(pf, pr)
    assert got == [i not in bad for i in range(n)]
    for i in range(n):
        rc, ok = orc.compressed_verify(pf[i], pr[i])
        assert got[i] == (rc == 0 and ok) == _single(R, pf[i], pr[i]), i


def test_edge_sizes(R):
    H = R.compressed_rand_proof.helper_verify_batch
    assert H([], []) == []
    cl = _proofs(R, 9, 300, 70)
    P, C = [p for p, _ in cl], [c for _, c in cl]
    assert H(P[:1], C[:1]) == [True]
    for n in (5, 8, 9):      # one transcript group of eight with and without a scalar remainder
        pf, pr = [p.copy() for p in P[:n]], [c.copy() for c in C[:n]]
        pr[n - 2][17, 3] ^= 1
        pf[0][64] ^= 1
        want = [0 < i != n - 2 for i in range(n)]
        assert H(pf, pr) == want == [_single(R, p, c) for p, c in zip(pf, pr)], n
    one = _proofs(R, 3, 1, 90)
    assert H([p for p, _ in one], [c for _, c in one]) == [True] * 3
    zero = _proofs(R, 2, 0, 95)
    zp, zc = [p.copy() for p, _ in zero], [c for _, c in zero]
    assert all(c.shape == (0, 64) for c in zc)
    assert H(zp, zc) == [True, True] == [_single(R, p, c) for p, c in zip(zp, zc)]
    zp[1][64] ^= 1      # commit(Z_m, Z_r) != C'
    assert H(zp, zc) == [True, False] == [_single(R, p, c) for p, c in zip(zp, zc)]
    # mixed d in one list, a malformed member among them
    bad_c = C[2].copy(); bad_c[5, 32:64] = BAD_POINT
    mp = [P[0], one[0][0], zp[0], P[1], one[1][0], np.zeros(100, np.uint8), P[2], zp[1]]
    mc = [C[0], one[0][1], zc[0], C[1], one[1][1], C[2], bad_c, zc[1]]
    assert H(mp, mc) == [True, True, True, True, True, False, False, False]


def _enc(R, cls, i, d, nb, P, check, fp):
    rng = np.random.default_rng(1000 + i)
    x = (rng.integers(-100, 100, size=d) / 128.0).astype(np.float32)      # inside the 8-bit range at frac 7: nothing is clipped
    return cls.encrypt(x, _blindings(rng, d), nb, P, check, nonce_seed=bytes([i % 251 + 1]) * 32, fp=fp)


def _parsed(cls, ups):
    """serialize -> deserialize(copy=False): the round as a server holds it after parsing the messages in place"""
    bufs = [u.serialize(as_array=True) for u in ups]
    out = [cls.deserialize(b, copy=False) for b in bufs]
    assert all(np.shares_memory(u.enc_values, b) for u, b in zip(out, bufs))
    return out, bufs


def _round(R, cls, ups, fp, seed=b"\x21" * 32):
    want = [u.verify(verifier_seed=seed, fp=fp) for u in ups]
    got = cls.verify_batch(ups, verifier_seed=seed, fp=fp)
    assert got == want, (got, want)
    return got


def _tamper_round(R, cls, ups, k):
    """a member tampered per leg: randomness proof, range proof, one ElGamal pair among the checked ones"""
    t, bufs = _parsed(cls, ups)
    if cls is R.EncParamsRangeCompressed:
        t[1].rand_proof[70] ^= 1
    else:
        t[1].rand_proofs[k // 2, 70] ^= 1
    t[2].range_proofs[1, 7 * 32 + 33] ^= 2
    t[3].enc_values[min(5, k - 1), 40] ^= 1
    return t, bufs


@pytest.mark.parametrize("check,d", [(0.013, 40000), (1.0, 5000)], ids=["e2e-0.013", "d5000-1.0"])
def test_range_compressed_round(R, check, d):
    cls, nb, P, n = R.EncParamsRangeCompressed, 8, 64, 16
    ups = [_enc(R, cls, i, d, nb, P, check, FP) for i in range(n)]
    ups.append(_enc(R, cls, 99, d // 2, nb, P, check, FP))      # a member of another shape
    parsed, _keep = _parsed(cls, ups)
    assert _round(R, cls, parsed, FP) == [True] * (n + 1)
    k = R.params._num_checked(d, check)
    t, _keep2 = _tamper_round(R, cls, ups, k)
    want = [i not in (1, 2, 3) for i in range(n + 1)]
    assert _round(R, cls, t, FP) == want
    assert R.compressed_rand_proof.helper_verify_batch([u.rand_proof for u in t], [u.enc_values for u in t]) == [i not in (1, 3) for i in range(n + 1)]


def test_range_round_cfg4_shape(R):
    cls, d, nb, P, n, fp = R.EncParamsRange, 5000, 32, 4, 8, (32, 7)
    ups = [_enc(R, cls, 200 + i, d, nb, P, 1.0, fp) for i in range(n)]
    ups.append(_enc(R, cls, 299, 3000, nb, P, 1.0, fp))
    parsed, _keep = _parsed(cls, ups)
    assert _round(R, cls, parsed, fp) == [True] * (n + 1)
    t, _keep2 = _tamper_round(R, cls, ups, d)
    assert _round(R, cls, t, fp) == [i not in (1, 2, 3) for i in range(n + 1)]


def test_batch_over_two_logical_devices(R):
    """rofl_set_option("devices", 0b11) with logical device 1 mapped onto HIP device 0: the clients are dealt to the two device contexts,
    the verdicts are those of the one-device call"""
    from rofl_project_code_amd import api
    api.map_device(1, 0)
    d = 2000
    pf, pr, bad = _tampered(_proofs(R, 12, d, 130), d)
    cls = R.EncParamsRangeCompressed
    ups = [_enc(R, cls, 400 + i, 600, 8, 4, 1.0, FP) for i in range(5)]
    t, _keep = _tamper_round(R, cls, ups, 600)
    seed = b"\x44" * 32
    one = R.compressed_rand_proof.helper_verify_batch(pf, pr)
    one_c = cls.verify_batch(t, verifier_seed=seed, fp=FP)
    try:
        R.set_option("devices", 0b11)
        two = R.compressed_rand_proof.helper_verify_batch(pf, pr)
        two_c = cls.verify_batch(t, verifier_seed=seed, fp=FP)
    finally:
        R.set_option("devices", 0)
    assert one == two == [i not in bad for i in range(12)]
    assert one_c == two_c == [True, False, False, False, True]
