"""Every entry point that folds group equations into ONE random linear combination, against forgeries whose errors cancel when the weights
are equal (tests/cancel_corpus.py; tests/test_cancellation_corpus.py shows on the CPU that they do cancel and that the oracle rejects them).
The other negative tests of the suite change one member of a sum, which any non-zero weight rejects -- a verifier whose weights were all 1,
or whose weight index dropped a term (3 idx + k, y d, the client part of rho's key, chunk_first), would pass them.  It fails here.

  batched Sigma-proof check (sigma_verify_batch / k_sigma_vprep): weight w_k of element i of member y = SHAKE256(seed, 3 (widx0 + y d + i) + k)
      S1-S5 through the single calls, the batch calls (18 members: both groups of sixteen), the device round's legs
  range proofs (verify_chunks): proof c of a shared check scaled by rho = verifier_c(seed, (client << 24 | chunk) | 1 << 62)
      R1 through verify_rangeproof (verify_batch 0, 1, 2), a run of chunks, a member of a batch
      R2 / R3 through verify_rangeproof_batch (the closer look's groups), EncParamsRange.verify_batch, DeviceRound.verify,
      verify_rangeproof_l2_batch, and a batch dealt to two logical devices

Expected everywhere: the untampered input verifies (duplicates included); then every vector / member that holds a tampered element is False
and every other member True -- the verdicts of the per-member single call and of the oracle.  Exact verdicts, no tolerance."""
import numpy as np
import pytest

import cancel_corpus as K
import orc
import test_gpu_round as T

pytestmark = pytest.mark.gpu
FP = K.FP
NB = K.NB
SEEDS = (b"\x21" * 32, b"\xc4" * 32, None)


@pytest.fixture(scope="module")
def R():
    import rofl_project_code_amd as R
    from rofl_project_code_amd import api, build
    build.build()
    R.set_device(0)
    api.map_device(1, 0)      # (for the two-device test: before logical device 1 is first used)
    yield R
    R.set_option("verify_batch", 1); R.set_option("sigma_batch", 1); R.set_option("devices", 0)


def _chunks(lst, k):
    return [lst[i:i + k] for i in range(0, len(lst), k)]


# ---------------------------------------------------------------- Sigma-proofs
def _sigma_single(R, kind):
    return (R.rand_proof_vec.verify_randproof_vec, R.square_rand_proof_vec.verify_l2rangeproof_vec, R.square_proof_vec.verify_l2rangeproof_vec)[kind]


def _sigma_batch(R, kind):
    return (R.rand_proof_vec.verify_randproof_vec_batch, R.square_rand_proof_vec.verify_l2rangeproof_vec_batch, R.square_proof_vec.verify_l2rangeproof_vec_batch)[kind]


def _sigma_forgeries(kind, d):
    return [(name, edits, delta) for name, edits in K.sigma_cases(kind, d) for delta in K.DELTAS]


@pytest.mark.parametrize("d", [2, 257, 300])
@pytest.mark.parametrize("kind", [0, 1, 2])
def test_sigma_single_calls(R, kind, d):
    pr, cm = K.sigma_honest(kind, d)
    verify = _sigma_single(R, kind)
    assert R.get_option("sigma_batch") == 1
    assert verify(pr, cm) is True
    for name, edits, delta in _sigma_forgeries(kind, d):
        t = K.sigma_apply(kind, pr, edits, delta)
        assert verify(t, cm) is False, (name, delta)
        assert orc.sigma_verify(kind, t, cm) == (0, False), (name, delta)


@pytest.mark.parametrize("d", [2, 257, 300])
@pytest.mark.parametrize("kind", [0, 1, 2])
def test_sigma_batch_calls(R, kind, d):
    """18 members (two decode groups of sixteen); forged vectors at members 0, 15, 16, 17, honest ones everywhere else; the per-element path
    (sigma_batch 0) is the reference verdict"""
    nc, slots = 18, (0, 15, 16, 17)
    pr, cm = K.sigma_honest(kind, d)
    other = K.sigma_honest(kind, d, seed=1)
    single, batch = _sigma_single(R, kind), _sigma_batch(R, kind)
    honest = [other if i % 2 else (pr, cm) for i in range(nc)]
    for s in slots:
        honest[s] = (pr, cm)
    try:
        for sb in (1, 0):
            R.set_option("sigma_batch", sb)
            assert batch([p for p, _ in honest], [c for _, c in honest]) == [True] * nc, sb
        for group in _chunks(_sigma_forgeries(kind, d), len(slots)):
            proofs = [p for p, _ in honest]
            what = {}
            for s, (name, edits, delta) in zip(slots, group):
                proofs[s] = K.sigma_apply(kind, pr, edits, delta)
                what[s] = (name, delta)
            want = [i not in what for i in range(nc)]
            for sb in (1, 0):
                R.set_option("sigma_batch", sb)
                got = batch(proofs, [c for _, c in honest])
                assert got == want, (sb, what, got)
            R.set_option("sigma_batch", 1)
            assert [single(proofs[s], cm) for s in what] == [False] * len(what), what
    finally:
        R.set_option("sigma_batch", 1)


@pytest.mark.parametrize("name", ["range", "l2", "l2_compressed"])
def test_sigma_legs_of_a_device_round(R, name):
    """the same edits on EncParamsRange.rand_proofs / EncParamsL2.square_proofs / EncParamsL2Compressed.square_proofs of a round of six"""
    cls = T._names(R)[name]
    kind = {"range": 0, "l2": 1, "l2_compressed": 2}[name]
    attr = "rand_proofs" if kind == 0 else "square_proofs"
    n, d, slots = 6, 300, (0, 1, 3, 4, 5)
    _, ups = T._make_round(R, cls, n, d, 300 + kind, check=1.0)

    def commits(u):
        return u.enc_values if kind != 2 else np.ascontiguousarray(np.concatenate([u.enc_values[:, :32], u.enc_values[:, 64:96]], axis=1))
    with R.DeviceRound(cls, d, max_clients=n) as rnd:
        rnd.ingest(ups)
        assert rnd.verify(verifier_seed=T.SEED, fp=T.FP) == cls.verify_batch(ups, verifier_seed=T.SEED, fp=T.FP) == [True] * n
        for group in _chunks(_sigma_forgeries(kind, d), len(slots)):
            t = [T._copy(u) for u in ups]
            what = {}
            for s, (cname, edits, delta) in zip(slots, group):
                setattr(t[s], attr, K.sigma_apply(kind, getattr(t[s], attr), edits, delta))
                what[s] = (cname, delta)
            want = [i not in what for i in range(n)]
            rnd.reset()
            rnd.ingest(t)
            got = rnd.verify(verifier_seed=T.SEED, fp=T.FP)
            assert got == want, (what, got)
            assert cls.verify_batch(t, verifier_seed=T.SEED, fp=T.FP) == want, what
            for s in what:
                assert t[s].verify(verifier_seed=T.SEED, fp=T.FP) is False, what[s]
                assert orc.sigma_verify(kind, getattr(t[s], attr), commits(t[s])) == (0, False), what[s]


# ---------------------------------------------------------------- range proofs
def _vr(R, pr, cm, seed):
    return R.range_proof_vec.verify_rangeproof(pr, cm, NB, verifier_seed=seed, fp=FP)


def _oracle(pr, cm):
    return orc.verify_rangeproof(pr, cm, NB, FP[0], FP[1])


@pytest.mark.parametrize("shape", K.R1_SHAPES, ids=lambda s: "d%d-P%d-%d-%d" % s)
def test_r1_two_chunks_of_one_client(R, shape):
    d, P, p, q = shape
    pr, cm = K.range_r1(d, P, p, q)
    forged = [K.range_apply(pr, [(p, 1), (q, -1)], delta) for delta in K.DELTAS]
    assert _oracle(pr, cm) == (0, True) and all(_oracle(t, cm) == (0, False) for t in forged)
    try:
        for vb in (0, 1, 2):
            R.set_option("verify_batch", vb)
            for seed in SEEDS:
                assert _vr(R, pr, cm, seed) is True, (vb, seed)
                for t in forged:
                    assert _vr(R, t, cm, seed) is False, (vb, seed)
    finally:
        R.set_option("verify_batch", 1)


def test_r1_in_a_run_of_chunks(R):
    """chunks [1, 3) of a client of four, the run holding the pair (1, 2): chunk_first is part of the weights' keys"""
    d, P, p, q = K.R1_RUN
    pr, cm = K.range_r1(d, P, p, q)
    m = d // P
    forged = [K.range_apply(pr, [(p, 1), (q, -1)], delta) for delta in K.DELTAS]
    assert _oracle(pr, cm) == (0, True) and all(_oracle(t, cm) == (0, False) for t in forged)

    def run(x, seed):
        return R.range_proof_vec.verify_rangeproof_chunks(x[1:3], P, 1, cm[m:3 * m], d, NB, verifier_seed=seed, fp=FP)
    try:
        for vb in (0, 1, 2):
            R.set_option("verify_batch", vb)
            for seed in SEEDS:
                assert run(pr, seed) is True, (vb, seed)
                for t in forged:
                    assert run(t, seed) is False, (vb, seed)
                    assert _vr(R, t, cm, seed) is False, (vb, seed)
    finally:
        R.set_option("verify_batch", 1)


def test_r1_as_a_member_of_a_batch(R):
    d, P, p, q = 8, 4, 0, 3
    n, at = 5, 2
    mem = [K.range_client(d, P, 20 + i) for i in range(n)]
    mem[at] = K.range_r1(d, P, p, q)
    prs, cms = [np.array(x) for x, _ in mem], [np.array(c) for _, c in mem]
    try:
        for vb in (1, 2):
            R.set_option("verify_batch", vb)
            for seed in SEEDS:
                assert R.range_proof_vec.verify_rangeproof_batch(prs, cms, NB, verifier_seed=seed, fp=FP) == [True] * n, (vb, seed)
                for delta in K.DELTAS:
                    t = list(prs)
                    t[at] = K.range_apply(prs[at], [(p, 1), (q, -1)], delta)
                    got = R.range_proof_vec.verify_rangeproof_batch(t, cms, NB, verifier_seed=seed, fp=FP)
                    assert got == [i != at for i in range(n)], (vb, seed, got)
                    assert got == [_vr(R, x, c, seed) for x, c in zip(t, cms)]
                    assert _oracle(t[at], cms[at]) == (0, False)
    finally:
        R.set_option("verify_batch", 1)


def _copies_forgeries(prs, copies, chunks, field):
    """[(tampered proofs list, the members that must fail)]: a (or b) of chunk c of every copy moved by its multiple of delta"""
    mult = K.copies_edits(copies)
    out = []
    for c in chunks:
        for delta in K.DELTAS:
            t = list(prs)
            for i in copies:
                t[i] = K.range_apply(prs[i], [(c, mult[i])], delta, field)
            out.append(t)
    return out


@pytest.mark.parametrize("field", ["a", "b"], ids=["R2", "R3"])
@pytest.mark.parametrize("where", list(K.COPIES_OF_NINE))
def test_copies_in_a_batch_of_nine(R, where, field):
    n, copies = 9, K.COPIES_OF_NINE[where]
    prs, cms = K.copies_batch(n, copies)
    V = R.range_proof_vec.verify_rangeproof_batch
    want = [i not in copies for i in range(n)]
    forged = _copies_forgeries(prs, copies, (0, 3), field)
    for t in forged:
        assert [_oracle(x, c)[1] for x, c in zip(t, cms)] == want
        assert [_vr(R, x, c, SEEDS[0]) for x, c in zip(t, cms)] == want
    try:
        for vb in (1, 2):
            R.set_option("verify_batch", vb)
            for seed in SEEDS:
                assert V(prs, cms, NB, verifier_seed=seed, fp=FP) == [True] * n, (vb, seed)
                for t in forged:
                    got = V(t, cms, NB, verifier_seed=seed, fp=FP)
                    assert got == want, (vb, seed, got)
    finally:
        R.set_option("verify_batch", 1)


@pytest.mark.parametrize("field", ["a", "b"], ids=["R2", "R3"])
@pytest.mark.parametrize("where", list(K.COPIES_OF_NINE))
def test_copies_in_a_batch_of_nine_sum_proofs(R, where, field):
    """rofl_verify_rangeproof_l2_batch: one proof per member over the (32, 1) generators, keyed member << 24"""
    n, copies = 9, K.COPIES_OF_NINE[where]
    prs, cms = K.l2_batch(n, copies)
    prs2 = [p.reshape(1, -1) for p in prs]
    L2 = R.l2_range_proof_vec
    want = [i not in copies for i in range(n)]
    forged = [[x[0] for x in t] for t in _copies_forgeries(prs2, copies, (0,), field)]
    for t in forged:
        assert [orc.verify_rangeproof_l2(x, c, K.L2_BITS, FP[0], FP[1])[1] for x, c in zip(t, cms)] == want
        assert [L2.verify_rangeproof_l2(x, c, K.L2_BITS, verifier_seed=SEEDS[0], fp=FP) for x, c in zip(t, cms)] == want
    try:
        for vb in (1, 2):
            R.set_option("verify_batch", vb)
            for seed in SEEDS:
                assert L2.verify_rangeproof_l2_batch(prs, np.stack(cms), K.L2_BITS, verifier_seed=seed, fp=FP) == [True] * n, (vb, seed)
                for t in forged:
                    got = L2.verify_rangeproof_l2_batch(t, np.stack(cms), K.L2_BITS, verifier_seed=seed, fp=FP)
                    assert got == want, (vb, seed, got)
    finally:
        R.set_option("verify_batch", 1)


@pytest.mark.parametrize("field", ["a", "b"], ids=["R2", "R3"])
def test_copies_in_a_round_of_updates(R, field):
    """EncParamsRange.verify_batch and DeviceRound(EncParamsRange).verify(): one encrypt() output twice in a round of six (d = 300, P = 4:
    chunks of 128, the third with padding behind its values)"""
    cls, n, d = R.EncParamsRange, 6, 300
    copies = (1, 4)
    _, ups = T._make_round(R, cls, n, d, 340, check=1.0)
    ups[4] = T._copy(ups[1])
    want = [i not in copies for i in range(n)]
    forged = []
    for c, delta in ((0, K.DELTAS[0]), (2, K.DELTAS[1])):
        t = [T._copy(u) for u in ups]
        for i, mult in K.copies_edits(copies).items():
            t[i].range_proofs = K.range_apply(t[i].range_proofs, [(c, mult)], delta, field)
        forged.append(t)
        assert [orc.verify_rangeproof(u.range_proofs, u.enc_values[:, :32].copy(), NB, T.FP[0], T.FP[1])[1] for u in t] == want
        assert [u.verify(verifier_seed=SEEDS[0], fp=T.FP) for u in t] == want
    try:
        with R.DeviceRound(cls, d, max_clients=n) as rnd:
            for vb in (1, 2):
                R.set_option("verify_batch", vb)
                for seed in SEEDS:
                    rnd.reset(); rnd.ingest(ups)
                    assert rnd.verify(verifier_seed=seed, fp=T.FP) == cls.verify_batch(ups, verifier_seed=seed, fp=T.FP) == [True] * n, (vb, seed)
                    for t in forged:
                        rnd.reset(); rnd.ingest(t)
                        got = rnd.verify(verifier_seed=seed, fp=T.FP)
                        assert got == want, (vb, seed, got)
                        assert cls.verify_batch(t, verifier_seed=seed, fp=T.FP) == want, (vb, seed)
    finally:
        R.set_option("verify_batch", 1)


@pytest.mark.parametrize("copies", [(0, 2), (0, 1)], ids=["one shard", "two shards"])
def test_copies_in_a_batch_dealt_to_two_devices(R, copies):
    """rofl_set_option("devices", 0b11), logical device 1 mapped onto HIP device 0: the members are dealt round-robin (member i to shard
    i % 2), every shard keys its weights by the members' indices in the caller's batch"""
    n = 6
    prs, cms = K.copies_batch(n, copies, seed0=40)
    V = R.range_proof_vec.verify_rangeproof_batch
    want = [i not in copies for i in range(n)]
    forged = _copies_forgeries(prs, copies, (1,), "a")
    for t in forged:
        assert [_oracle(x, c)[1] for x, c in zip(t, cms)] == want
        assert [_vr(R, x, c, SEEDS[0]) for x, c in zip(t, cms)] == want
    try:
        R.set_option("devices", 0b11)
        for vb in (1, 2):
            R.set_option("verify_batch", vb)
            for seed in SEEDS:
                assert V(prs, cms, NB, verifier_seed=seed, fp=FP) == [True] * n, (vb, seed)
                for t in forged:
                    got = V(t, cms, NB, verifier_seed=seed, fp=FP)
                    assert got == want, (vb, seed, got)
    finally:
        R.set_option("devices", 0); R.set_option("verify_batch", 1)
