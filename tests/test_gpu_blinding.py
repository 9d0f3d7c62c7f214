"""Blinding vectors generated on the GPU from seeds (rofl_blinding_vecs, k_blind_combine) against the Python model of the definition in
include/rofl_zk.h (tests/blind_model.py: hashlib's SHAKE256 and Python integers): single streams with half XOF blocks at both ends, slices,
signed combinations, the seeded dealer, pairwise masks and what a dropout leaves, device output, the containers' rand_seed keyword, and
one aggregation round end to end."""
import os
import subprocess
import sys

import numpy as np
import pytest

import blind_model as M

pytestmark = pytest.mark.gpu
FP = (32, 7)
SEED = bytes(range(1, 33))


@pytest.fixture(scope="module")
def R():
    import rofl_project_code_amd as R
    from rofl_project_code_amd import build
    build.build()
    R.set_device(0)
    return R


@pytest.fixture(scope="module")
def P(R):
    return R.pedersen_ops


def _sum_mod(vecs):
    return M.to_arr([sum(col) for col in zip(*[M.to_ints(v) for v in vecs])])


def _zero(d):
    return np.zeros((d, 32), dtype=np.uint8)


def test_definition(P):
    # d = 0..3 and odd / even first: blocks that own one scalar at either end; 513 = one scalar past a 256-thread block's 512
    ref = M.combine([(SEED, 1)], 5 + 513)
    for first in (0, 1, 5):
        for d in (0, 1, 2, 3, 513):
            got = P.rnd_scalar_vec_seeded(d, SEED, first=first)
            assert got.shape == (d, 32) and got.dtype == np.uint8
            assert (got == ref[first:first + d]).all(), (first, d)


def test_slices_concatenate(P):
    whole = P.rnd_scalar_vec_seeded(40, SEED)
    parts = np.concatenate([P.rnd_scalar_vec_seeded(7, SEED), P.rnd_scalar_vec_seeded(33, SEED, first=7)])
    assert (whole == parts).all() and (whole == M.combine([(SEED, 1)], 40)).all()


def test_combination(P):
    d = 33
    rng = np.random.default_rng(5)
    lists = {n: [(rng.bytes(32), int(rng.choice([1, -1]))) for _ in range(n)] for n in (0, 1, 2, 47)}
    lists[2] = [(lists[2][0][0], 1), (lists[2][1][0], -1)]
    assert {s for _, s in lists[47]} == {1, -1}
    for n, terms in lists.items():
        assert (P.blinding_vecs([terms], d)[0] == M.combine(terms, d)).all(), n
    assert not P.blinding_vecs([[]], d).any()                      # zero terms: 33 zero scalars
    got = P.blinding_vecs([lists[47], lists[0], lists[2]], d, first=3)      # three vectors of different term counts in one call
    assert got.shape == (3, d, 32)
    for v, n in enumerate((47, 0, 2)):
        assert (got[v] == M.combine(lists[n], d, first=3)).all(), n
    # a term and its negation cancel; a stream taken twice is twice the stream
    s = lists[1][0][0]
    assert not P.blinding_vecs([[(s, 1), (s, -1)]], d).any()
    assert (P.blinding_vecs([[(s, -1), (s, -1)]], d)[0] == M.to_arr([-2 * M.stream_int(s, k) for k in range(d)])).all()


def test_dealer(P):
    d = 33
    for n in (1, 2, 3, 48):
        vecs = P.generate_cancelling_scalar_vec_seeded(n, d, SEED)
        assert len(vecs) == n and all(v.shape == (d, 32) for v in vecs)
        assert not _sum_mod(vecs).any(), n
        for i in (0, n - 2) if n > 1 else ():
            assert (vecs[i] == P.rnd_scalar_vec_seeded(d, M.vec_seed(SEED, i))).all(), (n, i)
            assert (vecs[i] == M.combine([(M.vec_seed(SEED, i), 1)], d)).all(), (n, i)
        if n == 1:
            assert not vecs[0].any()
        if n == 2:
            assert (vecs[1] == M.to_arr([-v for v in M.to_ints(vecs[0])])).all() and vecs[0].any()


def test_pairwise(P):
    d, n = 33, 4
    pair_seed = {(i, j): M.round_seed(b"secret %d %d" % (i, j), 9) for i in range(n) for j in range(i + 1, n)}
    peers = {i: [(j, pair_seed[min(i, j), max(i, j)]) for j in range(n) if j != i] for i in range(n)}
    single = [P.pairwise_blinding_vec(i, peers[i], d) for i in range(n)]
    for i in range(n):
        model = M.combine([(s, 1 if i < j else -1) for j, s in peers[i]], d)
        assert (single[i] == model).all(), i
    assert not _sum_mod(single).any() and all(v.any() for v in single)
    hosted = P.pairwise_blinding_vecs([(i, peers[i]) for i in range(n)], d)
    assert hosted.shape == (n, d, 32) and all((hosted[i] == single[i]).all() for i in range(n))
    # a client drops out: what is left of the sum is minus its vector (the quantity a dropout correction has to supply)
    for gone in range(n):
        rest = _sum_mod([single[i] for i in range(n) if i != gone])
        assert (rest == M.to_arr([-v for v in M.to_ints(single[gone])])).all(), gone
    # a run of a vector
    assert (P.pairwise_blinding_vec(2, peers[2], 9, first=11) == single[2][11:20]).all()


def test_device_output(R):
    r = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "gpu_blinding_device_check.py")],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "BLINDING_DEVICE_OUTPUT PASS" in r.stdout, r.stdout + r.stderr[-3000:]


def _client(i, d=6):
    rng = np.random.default_rng(3100 + i)
    x = (rng.integers(-3, 4, size=d) / 128.0).astype(np.float32)
    bl = rng.integers(0, 256, size=(d, 32), dtype=np.uint8); bl[:, 31] &= 0x0F
    return x, bl


@pytest.mark.parametrize("kind", ["EncParamsL2", "EncParamsL2Compressed"])
def test_containers(R, P, kind):
    cls = getattr(R, kind)
    d, nb, part, l2n = 6, 8, 1, 32
    ns = [bytes([0x41 + i]) * 32 for i in range(3)]
    rs = [bytes([0x61 + i]) * 32 for i in range(3)]
    cl = [_client(i) for i in range(3)]
    singles = []
    for i in (0, 2):
        a = cls.encrypt(cl[i][0], cl[i][1], nb, part, l2n, nonce_seed=ns[i], rand_seed=rs[i], fp=FP)
        b = cls.encrypt(cl[i][0], cl[i][1], nb, part, l2n, nonce_seed=ns[i], rand_scalars=P.rnd_scalar_vec_seeded(d, rs[i]), fp=FP)
        assert a.serialize() == b.serialize(), i
        assert a.verify(verifier_seed=b"\x07" * 32, fp=FP)
        singles.append(a)
    r2_mid = P.rnd_scalar_vec_seeded(d, b"\x77" * 32)
    # a batch: the seeded clients' r2 are rows of ONE blinding_vecs call, handed in as rand_scalars (encrypt_batch keeps its parameter list)
    r2 = P.blinding_vecs([[(rs[0], 1)], [(rs[2], 1)]], d)
    got = cls.encrypt_batch([(cl[0][0], cl[0][1], r2[0]), (cl[1][0], cl[1][1], r2_mid), (cl[2][0], cl[2][1], r2[1])], nb, part, l2n,
                            nonce_seeds=ns, fp=FP)
    assert got[0].serialize() == singles[0].serialize() and got[2].serialize() == singles[1].serialize()
    mid = cls.encrypt(cl[1][0], cl[1][1], nb, part, l2n, nonce_seed=ns[1], rand_scalars=r2_mid, fp=FP)
    assert got[1].serialize() == mid.serialize()
    assert all(g.verify(verifier_seed=b"\x08" * 32, fp=FP) for g in got)
    with pytest.raises(ValueError):
        cls.encrypt(cl[0][0], cl[0][1], nb, part, l2n, rand_scalars=r2_mid, rand_seed=rs[0], fp=FP)


def test_a_round_end_to_end(R, P):
    R.api.set_fp(*FP)
    d, n = 8, 3
    rng = np.random.default_rng(77)
    xs = [(rng.integers(-300, 300, size=d) / 128.0).astype(np.float32) for _ in range(n)]
    bls = P.generate_cancelling_scalar_vec_seeded(n, d, SEED)

    def aggregate(blindings):
        with R.DeviceAccumulator.unity(d) as acc:
            for x, b in zip(xs, blindings):
                m = R.conversion32.f32_to_scalar_vec(x, fp=FP)
                pairs = np.ascontiguousarray(np.concatenate([P.commit_vec(m, b), P.commit_no_blinding_vec(b)], axis=1))
                acc.accumulate_pairs(pairs)
            return acc.extract()

    got = aggregate(bls)
    want = np.sum(np.stack(xs).astype(np.float64), axis=0).astype(np.float32)
    assert got is not None and got.tobytes() == want.tobytes()
    # one vector replaced by an unrelated stream: the blindings no longer cancel and the unity check refuses the round
    assert aggregate([bls[0], P.rnd_scalar_vec_seeded(d, b"\x99" * 32), bls[2]]) is None
