"""encrypt_batch of EncParamsRange, EncParamsRangeCompressed and EncParamsL2Compressed: the clients of one process proved together (one
rofl_create_rangeproof_batch for the L-inf legs, one rofl_create_compressed_randproof_batch for the compressed randomness proofs).  Every
container must serialize to the bytes of encrypt() for that client with the same nonce seed, and the round must verify.

Three clients, d = 70, prove_range 8, n_partition 2; check_percentage 1.0 and 0.5 (k = 35: the range proofs cover a prefix, the randomness
proofs make their own commitments) for the Range kinds; l2_range 32 at fp 32/7 for EncParamsL2Compressed, as test_gpu_params.py has it."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
FP = (32, 7)
D, NB, P, L2N, N = 70, 8, 2, 32, 3


@pytest.fixture(scope="module")
def R():
    import rofl_project_code_amd as R
    from rofl_project_code_amd import build
    build.build()
    R.set_device(0)
    return R


def _inputs(i, lo=-3, hi=4):
    rng = np.random.default_rng(1200 + i)
    x = (rng.integers(lo, hi, size=D) / 128.0).astype(np.float32)
    bl = rng.integers(0, 256, size=(D, 32), dtype=np.uint8); bl[:, 31] &= 0x0F
    r2 = rng.integers(0, 256, size=(D, 32), dtype=np.uint8); r2[:, 31] &= 0x0F
    return x, bl, r2


SEEDS = [bytes([i + 0x31]) * 32 for i in range(N)]


@pytest.mark.parametrize("check", [1.0, 0.5])
@pytest.mark.parametrize("kind", ["EncParamsRange", "EncParamsRangeCompressed"])
def test_range_kinds_equal_encrypt(R, kind, check):
    cls = getattr(R, kind)
    cl = [_inputs(i)[:2] for i in range(N)]
    got = cls.encrypt_batch(cl, NB, P, check, nonce_seeds=SEEDS, fp=FP)
    assert len(got) == N and all(type(g) is cls for g in got)
    for i in range(N):
        one = cls.encrypt(cl[i][0], cl[i][1], NB, P, check, nonce_seed=SEEDS[i], fp=FP)
        assert got[i].serialize() == one.serialize(), i
    assert cls.verify_batch(got, verifier_seed=b"\x05" * 32, fp=FP) == [True] * N


def test_l2_compressed_equals_encrypt(R):
    """(on the tree before this method existed the inherited EncParamsL2.encrypt_batch ended in a TypeError: six arguments for a
    constructor of seven)"""
    cls = R.EncParamsL2Compressed
    cl = [_inputs(i) for i in range(N)]
    got = cls.encrypt_batch(cl, NB, P, L2N, nonce_seeds=SEEDS, fp=FP)
    assert len(got) == N and all(type(g) is cls for g in got)
    for i in range(N):
        one = cls.encrypt(cl[i][0], cl[i][1], NB, P, L2N, nonce_seed=SEEDS[i], rand_scalars=cl[i][2], fp=FP)
        assert got[i].serialize() == one.serialize(), i
        assert R.compressed_rand_proof.helper_verify(got[i].rand_proof, got[i].enc_values[:, :64])      # (verify() does not re-check this proof, params.rs:255-289)
    assert cls.verify_batch(got, verifier_seed=b"\x06" * 32, fp=FP) == [True] * N


@pytest.mark.parametrize("kind", ["EncParamsRange", "EncParamsRangeCompressed", "EncParamsL2Compressed"])
def test_a_client_outside_the_range_fares_as_in_encrypt(R, kind):
    """A client with a value outside the 8-bit range.  encrypt() clips every value into the range before anything is proved
    (params.rs:475-503), so no range proof ever sees such a value and encrypt() does not raise for it; its randomness proof takes the
    un-clipped plaintext, and the container does not verify.  encrypt_batch must give that client exactly encrypt()'s outcome -- the same
    bytes, or the same error -- and leave its neighbours' bytes alone."""
    cls = getattr(R, kind)
    l2 = kind == "EncParamsL2Compressed"
    cl = [_inputs(i) for i in range(N)]
    x = cl[1][0].copy(); x[7] = 3.0; x[50] = -2.5      # 8 bits at 7 fractional bits: |x| <= 127 / 128
    cl[1] = (x,) + cl[1][1:]
    args = (NB, P, L2N) if l2 else (NB, P, 1.0)
    if not l2:
        cl = [c[:2] for c in cl]

    def single(i):
        kw = dict(rand_scalars=cl[i][2]) if l2 else {}
        return cls.encrypt(cl[i][0], cl[i][1], *args, nonce_seed=SEEDS[i], fp=FP, **kw)
    try:
        want = [single(i) for i in range(N)]
    except R.RoflError as e:
        with pytest.raises(R.RoflError) as e2:
            cls.encrypt_batch(cl, *args, nonce_seeds=SEEDS, fp=FP)
        assert e2.value.code == e.code
        return
    got = cls.encrypt_batch(cl, *args, nonce_seeds=SEEDS, fp=FP)
    for i in range(N):
        assert got[i].serialize() == want[i].serialize(), i
    assert cls.verify_batch(got, verifier_seed=b"\x07" * 32, fp=FP) == [w.verify(verifier_seed=b"\x07" * 32, fp=FP) for w in want]


@pytest.mark.parametrize("check", [1.0, 0.5])
@pytest.mark.parametrize("kind", ["EncParamsRange", "EncParamsRangeCompressed"])
def test_a_client_that_fails_raises(R, kind, check):
    """A non-finite value reaches the randomness leg un-clipped: that client's error (10) is raised, as encrypt() raises it"""
    cls = getattr(R, kind)
    cl = [_inputs(i)[:2] for i in range(N)]
    x = cl[2][0].copy(); x[60] = np.nan
    cl[2] = (x, cl[2][1])
    with pytest.raises(R.RoflError) as e1:
        cls.encrypt(cl[2][0], cl[2][1], NB, P, check, nonce_seed=SEEDS[2], fp=FP)
    with pytest.raises(R.RoflError) as e2:
        cls.encrypt_batch(cl, NB, P, check, nonce_seeds=SEEDS, fp=FP)
    assert e1.value.code == e2.value.code == 10
