"""What a protocol call or an update-preparation call leaves in its lane's staging buffers (rofl_dbg_lane_scan: pinned h_misc / h_misc2,
device tmp_in / tmp_in2 / tmp_out, on every lane of the device).  Each case makes ONE call and then scans: no secret of the call may be
found in any buffer, and one public by-product of the same call must be -- the positive control, which shows that the scan finds what is
there.  Keys and payloads come from a seeded generator, every needle is at least 16 random bytes: a chance match has probability 2^-128.
The inputs a case needs from another primitive come from the Python models, so that nothing but the call under test has put them into a
lane.

The last five cases hold the two drivers that wipe with BlindWipe to the same promise: the preparation calls' driver (prepare_calls.hpp:
quantization, noise and clipping seeds) and blind_combine_launch (the term seeds of rofl_blinding_vecs and of an opening given as terms).
The quantization, noise and blinding calls leave no public by-product of 16 bytes in a scanned buffer (their vectors go through the
lane's value and byte workspaces, which the scan does not read): for them the first test of this module is the control that the scan
finds what is there.  The clipping call has one, its two scales, adjacent 64-bit words in tmp_out (8 of the 16 bytes are the scales' zero
high halves: a chance match still needs both 32-bit scales side by side)."""
import ctypes

import numpy as np
import pytest

import aead_model as A
import blind_model as B
import dh_model as D
import dleq_model as Q
import feldman_model as F
import orc
import shamir_model as S

pytestmark = pytest.mark.gpu
FP = (32, 7)
T, N_SHARES = 3, 5


@pytest.fixture(scope="module")
def R():
    import rofl_project_code_amd as R
    from rofl_project_code_amd import build
    build.build()
    R.set_device(0)
    R.api.set_fp(*FP)
    return R


def _rows(rng, n, w=32):
    return np.frombuffer(rng.bytes(n * w), np.uint8).reshape(n, w).copy()


def _pk(sks):
    return np.stack([np.frombuffer(D.public_key(k), np.uint8) for k in sks])


def _found(R, needle):
    b = bytes(needle)
    assert len(b) >= 16 and any(b)
    fn = R.lib().rofl_dbg_lane_scan
    fn.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_int)]
    found = ctypes.c_int(-1)
    assert fn(b, len(b), ctypes.byref(found)) == 0
    return found.value


def _check(R, secrets, public=None):
    """secrets: (name, bytes-like) pairs, none of which may be in a lane; public: one needle that must be"""
    left = [(name, _found(R, s)) for name, s in secrets]
    assert all(f == 0 for _, f in left), left
    if public is not None:
        assert _found(R, public) >= 1


@pytest.fixture(scope="module")
def sharing():
    """2 secrets, threshold 3, 5 shares, from the model: (secrets, coefficient seeds, shares, a_1 of secret 0 as canonical bytes)"""
    rng = np.random.default_rng(20270301)
    sec, seeds = _rows(rng, 2), _rows(rng, 2)
    a1 = S.coefficients(seeds[0], T)[0].to_bytes(32, "little")
    return sec, seeds, S.share(sec, seeds, T, N_SHARES), a1


def test_the_scan_refuses_a_short_needle_and_writes_nothing(R):
    found = ctypes.c_int(7)
    fn = R.lib().rofl_dbg_lane_scan
    fn.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_int)]
    assert fn(b"\x01" * 15, 15, ctypes.byref(found)) == 11 and fn(None, 16, ctypes.byref(found)) == 11 and fn(b"\x01" * 16, 16, None) == 11
    pk = R.key_agreement.public_keys(_rows(np.random.default_rng(20270300), 1))
    assert _found(R, pk[0]) == _found(R, pk[0]) >= 1      # a scan leaves what it found where it was


@pytest.mark.parametrize("n", [1, 65])
def test_dh_public_keys(R, n):
    sk = D.rand_keys(np.random.default_rng(20270302 + n), n)
    pk = R.key_agreement.public_keys(sk)
    _check(R, [("key %d" % i, sk[i]) for i in range(n)], public=pk[n - 1])


def test_dh_shared(R):
    rng = np.random.default_rng(20270310)
    sk, peers = D.rand_keys(rng, 2), _pk(D.rand_keys(rng, 3))
    out, status = R.key_agreement.shared_secrets(sk, peers)
    assert not status.any() and out.shape == (6, 32)
    _check(R, [("key %d" % i, sk[i]) for i in range(2)] + [("shared %d" % i, out[i]) for i in range(6)], public=peers[2])


def test_shamir_share(R, sharing):
    sec, seeds, shares, a1 = sharing
    got = R.secret_sharing.share(sec, seeds, T, N_SHARES)
    assert got.tobytes() == shares.tobytes()
    _check(R, [("secret 0", sec[0]), ("secret 1", sec[1]), ("seed 0", seeds[0]), ("seed 1", seeds[1]), ("a_1 of secret 0", a1), ("share", got[1, 4])])


def test_shamir_reconstruct(R, sharing):
    sec, _, shares, _ = sharing
    xs = np.arange(1, N_SHARES + 1)
    got = R.secret_sharing.reconstruct(xs, shares)
    assert got.tobytes() == S.reconstruct(xs, shares).tobytes()
    _check(R, [("share", shares[1, 2]), ("secret 0", got[0]), ("secret 1", got[1])])


def test_feldman_commit(R, sharing):
    sec, seeds, _, a1 = sharing
    com = R.secret_sharing.commit(sec, seeds, T)
    _check(R, [("secret 0", sec[0]), ("secret 1", sec[1]), ("seed 0", seeds[0]), ("seed 1", seeds[1]), ("a_1 of secret 0", a1)], public=com[1, 2])


def test_feldman_verify(R, sharing):
    sec, seeds, shares, _ = sharing
    com = F.commit(sec, seeds, T)
    v = R.secret_sharing.verify_shares(com, np.arange(1, N_SHARES + 1), shares)
    assert not v.any()
    _check(R, [("share", shares[0, 0]), ("last share", shares[1, 4])], public=com[1, 2])


def test_sig_sign(R):
    rng = np.random.default_rng(20270320)
    sk = D.rand_keys(rng, 2)
    sigs = R.signatures.sign(sk, [rng.bytes(33), rng.bytes(65)])
    _check(R, [("key 0", sk[0]), ("key 1", sk[1])], public=sigs[1])


def _aead_case(derive_round, salt):
    """2 records, payloads of 33 and 65 bytes: (keys, nonces, ads, payloads, the model's records, the call's secrets)"""
    rng = np.random.default_rng(20270330 + salt + (derive_round or 0))
    keys, nonces = _rows(rng, 2), _rows(rng, 2, 12)
    ads, pts = [rng.bytes(5), rng.bytes(17)], [rng.bytes(33), rng.bytes(65)]
    secrets = [("key row %d" % i, keys[i]) for i in range(2)] + [("plaintext %d" % i, pts[i][-32:]) for i in range(2)]
    if derive_round is not None:
        secrets += [("derived key %d" % i, A.derive_key(keys[i], derive_round)) for i in range(2)]
    return keys, nonces, ads, pts, A.seal_batch(keys, nonces, ads, pts, derive_round=derive_round), secrets


@pytest.mark.parametrize("derive_round", [None, 7])
def test_aead_seal(R, derive_round):
    keys, nonces, ads, pts, want, secrets = _aead_case(derive_round, 0)
    got = R.aead.seal(keys, nonces, ads, pts, derive_round=derive_round)
    assert got == want
    _check(R, secrets, public=got[1][:32])


@pytest.mark.parametrize("derive_round", [None, 7])
def test_aead_open(R, derive_round):
    keys, nonces, ads, pts, sealed, secrets = _aead_case(derive_round, 100)      # records of the model: no call has sealed them
    back, v = R.aead.open(keys, nonces, ads, sealed, derive_round=derive_round)
    assert back == pts and not v.any()
    _check(R, secrets, public=sealed[1][:32])


def _dleq_case():
    rng = np.random.default_rng(20270340)
    return D.rand_keys(rng, 1), _pk(D.rand_keys(rng, 2)), _rows(rng, 2)


def test_dleq_prove(R):
    sk, peers, ctxs = _dleq_case()
    reveals, proofs, status = R.dleq.prove(sk, peers, ctxs)
    assert not status.any() and proofs.tobytes() == Q.prove_batch(sk, peers, ctxs)[1].tobytes()
    _check(R, [("key", sk[0])], public=reveals[1])


def test_dleq_verify_with_shared_out(R):
    sk, peers, ctxs = _dleq_case()
    reveals, proofs, _ = Q.prove_batch(sk, peers, ctxs)
    verdicts, shared = R.dleq.verify(_pk(sk), peers, ctxs, reveals, proofs)      # (the wrapper always asks for shared_out32)
    assert not verdicts.any() and shared.any(axis=1).all()
    _check(R, [("shared %d" % i, shared[i]) for i in range(2)])


# ---- the calls that wipe with BlindWipe: the preparation calls' driver and blind_combine_launch ----
PREP_FP, PREP_RANGE, PREP_D = (16, 7), 8, 33      # d = 33: two XOF blocks of 32 rounding words


def _prep_case(salt):
    """2 vectors of 33 values inside the clip range of (8, fp16.7), with their seeds: (seeds, values, outs, the leading arguments of a route-1 call)"""
    rng = np.random.default_rng(20270350 + salt)
    seeds = _rows(rng, 2)
    vals = [rng.uniform(-0.9, 0.9, PREP_D).astype(np.float32) for _ in range(2)]
    outs = [np.full(PREP_D, np.nan, np.float32) for _ in range(2)]
    arr = lambda xs: (ctypes.c_void_p * 2)(*[x.ctypes.data for x in xs])
    return seeds, vals, outs, [ctypes.c_uint(1), ctypes.c_size_t(2), seeds.tobytes(), arr(vals)], arr(outs)


def _prep_tail(outs_arr):
    return [ctypes.c_size_t(PREP_RANGE), ctypes.c_uint(PREP_FP[0]), ctypes.c_uint(PREP_FP[1]), outs_arr]


def _seed_secrets(seeds):
    return [("seed %d" % i, seeds[i]) for i in range(len(seeds))]


def test_quantize_prob_kernel_route(R):
    seeds, vals, outs, head, oa = _prep_case(0)
    assert R.lib().rofl_dbg_quantize_prob_route(*head, ctypes.c_size_t(0), ctypes.c_size_t(PREP_D), *_prep_tail(oa)) == 0
    assert not np.isnan(np.stack(outs)).any()
    _check(R, _seed_secrets(seeds))


def test_noise_binomial_kernel_route(R):
    seeds, vals, outs, head, oa = _prep_case(1)
    assert R.lib().rofl_dbg_noise_binomial_route(*head, ctypes.c_size_t(0), ctypes.c_size_t(PREP_D), ctypes.c_uint32(16), *_prep_tail(oa)) == 0
    assert not np.isnan(np.stack(outs)).any()
    _check(R, _seed_secrets(seeds))


def test_clip_l2_seeded_kernel_route(R):
    """max_sq = 100 steps^2: isqrt = 10 >= ceil(sqrt(33)) = 6, and far below the sum of squares of either vector, so both are scaled"""
    seeds, vals, outs, head, oa = _prep_case(2)
    max_sq, scale = (ctypes.c_uint64 * 2)(100, 100), (ctypes.c_uint64 * 2)()
    assert R.lib().rofl_dbg_clip_l2_route(*head, ctypes.c_size_t(PREP_D), max_sq, *_prep_tail(oa), scale) == 0
    assert not np.isnan(np.stack(outs)).any() and all(0 < m < 1 << 32 for m in scale)
    _check(R, _seed_secrets(seeds), public=bytes(scale))


def test_blinding_vecs(R):
    rng = np.random.default_rng(20270360)
    seeds = _rows(rng, 4)
    terms = [[(seeds[0], 1), (seeds[1], -1)], [(seeds[2], -1), (seeds[3], 1)]]
    got = R.pedersen_ops.blinding_vecs(terms, 3)
    assert got.tobytes() == b"".join(B.combine(t, 3).tobytes() for t in terms)
    _check(R, _seed_secrets(seeds))


def test_extract_opened_terms(R):
    """one client's record of the oracle under the blinding the two terms expand to: the extraction expands them on the device"""
    rng = np.random.default_rng(20270361)
    seeds = _rows(rng, 2)
    terms = [(seeds[0], 1), (seeds[1], -1)]
    ks = (5, -3, 0)
    x = np.stack([orc.f32_to_scalar(k / 128.0, *FP)[1] for k in ks])
    r = B.combine(terms, 3)
    rec = np.ascontiguousarray(np.concatenate([orc.commit_vec(x, r), orc.commit_vec(r, None)], axis=1))
    h = R.api.accumulator.create(3)
    try:
        R.api.accumulator.add(h, [rec.ctypes.data], [3], 64)
        got, bad = R.api.accumulator.extract_opened_terms(h, 3, terms, 1 << 15, 16, FP)
    finally:
        R.api.accumulator.destroy(h)
    assert bad is None and got.tobytes() == np.array([k / 128.0 for k in ks], np.float32).tobytes()
    _check(R, _seed_secrets(seeds))
