"""encrypt_batch of EncParamsL2 and EncParamsL2CompressedStrict with every leg batched: one rofl_create_rangeproof_batch (L-inf), one
rofl_create_rangeproof_l2_batch (the sum proofs), one rofl_create_sigmaproof_vec_batch (the square proofs) and, for the compressed kind,
one rofl_create_compressed_randproof_batch.  Every container must serialize to the bytes of encrypt() for that client with the same nonce
seed, the round must verify, and one encrypt_batch must issue exactly one call per leg and no per-client create call.

Three clients, d = 70, prove_range 8, n_partition 2, l2_range 32 at fp 32/7, seeds as in test_gpu_encrypt_batch.py."""
import collections

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
FP = (32, 7)
D, NB, P, L2N, N = 70, 8, 2, 32, 3
SEEDS = [bytes([i + 0x31]) * 32 for i in range(N)]


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


@pytest.mark.parametrize("kind", ["EncParamsL2", "EncParamsL2CompressedStrict"])
def test_l2_kinds_equal_encrypt(R, kind):
    cls = getattr(R, kind)
    cl = [_inputs(i) for i in range(N)]
    got = cls.encrypt_batch(cl, NB, P, L2N, nonce_seeds=SEEDS, fp=FP)
    assert len(got) == N and all(type(g) is cls for g in got)
    for i in range(N):
        one = cls.encrypt(cl[i][0], cl[i][1], NB, P, L2N, nonce_seed=SEEDS[i], rand_scalars=cl[i][2], fp=FP)
        assert got[i].serialize() == one.serialize(), i
    assert cls.verify_batch(got, verifier_seed=b"\x06" * 32, fp=FP) == [True] * N


class _Counting:
    """api.lib() with every rofl_create_* call counted by name"""

    def __init__(self, lib, counts):
        self._lib, self._counts = lib, counts

    def __getattr__(self, name):
        f = getattr(self._lib, name)
        if not name.startswith("rofl_create_"):
            return f

        def counted(*a):
            self._counts[name] += 1
            return f(*a)
        return counted


def _count_creates(R, monkeypatch, thunk):
    from rofl_project_code_amd import api
    counts = collections.Counter()
    wrapped = _Counting(api.lib(), counts)
    monkeypatch.setattr(api, "lib", lambda: wrapped)
    try:
        thunk()
    finally:
        monkeypatch.undo()
    return counts


@pytest.mark.parametrize("kind", ["EncParamsL2", "EncParamsL2Compressed"])
def test_one_call_per_leg_l2(R, monkeypatch, kind):
    cls = getattr(R, kind)
    cl = [_inputs(i) for i in range(N)]
    c = _count_creates(R, monkeypatch, lambda: cls.encrypt_batch(cl, NB, P, L2N, nonce_seeds=SEEDS, fp=FP))
    assert c["rofl_create_squarerandproof_vec"] == 0 and c["rofl_create_squareproof_vec"] == 0 and c["rofl_create_rangeproof_l2"] == 0, dict(c)
    assert c["rofl_create_sigmaproof_vec_batch"] == 1 and c["rofl_create_rangeproof_l2_batch"] == 1 and c["rofl_create_rangeproof_batch"] == 1, dict(c)
    assert c["rofl_create_compressed_randproof_batch"] == (1 if kind == "EncParamsL2Compressed" else 0), dict(c)
    assert sum(c.values()) == (4 if kind == "EncParamsL2Compressed" else 3), dict(c)


@pytest.mark.parametrize("check", [1.0, 0.5])
def test_one_call_per_leg_range(R, monkeypatch, check):
    cl = [_inputs(i)[:2] for i in range(N)]
    c = _count_creates(R, monkeypatch, lambda: R.EncParamsRange.encrypt_batch(cl, NB, P, check, nonce_seeds=SEEDS, fp=FP))
    assert c["rofl_create_randproof_vec"] == 0 and c["rofl_create_sigmaproof_vec_batch"] == 1 and c["rofl_create_rangeproof_batch"] == 1, dict(c)
    assert sum(c.values()) == 2, dict(c)
