"""What a protocol call leaves in its lane's staging buffers (rofl_dbg_lane_scan: pinned h_misc / h_misc2, device tmp_in / tmp_in2 /
tmp_out, on every lane of the device).  Each case makes ONE call and then scans: no secret of the call may be found in any buffer, and one
public by-product of the same call must be -- the positive control, which shows that the scan finds what is there.  Keys and payloads come
from a seeded generator, every needle is at least 16 random bytes: a chance match has probability 2^-128.  The inputs a case needs from
another primitive come from the Python models, so that nothing but the call under test has put them into a lane."""
import ctypes

import numpy as np
import pytest

import aead_model as A
import dh_model as D
import dleq_model as Q
import feldman_model as F
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
