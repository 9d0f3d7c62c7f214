"""Every production entry point whose kernels decode Ristretto points, fed the corpus of tests/ristretto_corpus.py: above all the classes that
the decoder refuses only AFTER its square-root chain has run (a non-square, 1 / 0 at s = sqrt(-1), a negative t, y = 0 at s = p - 1) -- where
gd_ristretto_decode has returned without writing the point and everything rests on what the calling kernel does next: store the identity or
skip, set the right status word, name the right member.  Each site must report the refusal the way include/rofl_zk.h documents it (5 for the
call, the pair / row / member alone, the accumulator unchanged), agree with the oracle or the Python model where one has an answer, and accept
the valid edges (0, p - 3, the smallest valid s, B .. 16 B) with the model's bytes.

Shapes: vectors of 257 with the bad entries rotated over 0, 63, 64, 127, 128, 255, 256 (the block edges of the 64- and 256-thread kernels
and of those with two threads per element); batches of nine members, one per invalid class and two honest ones.  "Representatives" are
ristretto_corpus.representatives(): one entry per invalid class that ONLY that class's check refuses."""
import numpy as np
import pytest

import cancel_corpus as CC
import dh_model
import feldman_model as FM
import orc
import ristretto_corpus as RC

pytestmark = pytest.mark.gpu
CORPUS = RC.corpus()
REPS = RC.representatives()
EDGES = RC.valid_edges()
D, POS = RC.D, RC.POSITIONS
ELL = orc.L_ORDER
FP = CC.FP            # (16, 7): the oracle-made vectors of cancel_corpus
FPR = (32, 7)         # the containers of a round, as tests/test_gpu_round.py makes them
NB = CC.NB
SEED = b"\x3c" * 32
N_BATCH = 9           # members 0 .. 6 carry the representative of class 0 .. 6, members 7 and 8 are honest
WANT_BATCH = [False] * 7 + [True] * 2


@pytest.fixture(scope="module")
def R():
    import rofl_project_code_amd as R
    from rofl_project_code_amd import build
    build.build()
    R.set_device(0)
    return R


def _code(R, call):
    with pytest.raises(R.RoflError) as e:
        call()
    return e.value.code


def _two_positions():
    """(class index, representative, position of the first case, position of the second)"""
    return [(i, rep, POS[i], POS[(i + 3) % 7]) for i, rep in enumerate(REPS)]


def _scalar(v):
    return np.frombuffer((v % ELL).to_bytes(32, "little"), np.uint8)


def _values(rng, d):
    return (rng.integers(-100, 101, size=d) / 128.0).astype(np.float32)


def _neg(b):
    pt = RC.pyref.ristretto_decode(bytes(b))
    return np.frombuffer(RC.pyref.ristretto_encode(RC.pyref.pt_neg(pt)), np.uint8)


def _oracle_fold(records):
    """sum over clients of (d, 64) records of valid pairs, by the oracle's point addition"""
    acc = np.zeros_like(records[0][:, :64]).reshape(-1, 32)
    for r in records:
        rc, acc = orc.add_points_vec(acc, np.ascontiguousarray(r[:, :64]).reshape(-1, 32))
        assert rc == 0
    return acc.reshape(-1, 64)


# ---------------------------------------------------------------- sites that report per element: the whole corpus in one call
def test_key_agreement_peers_are_the_corpus(R):
    sk = dh_model.rand_keys(np.random.default_rng(11), 2)
    peers = RC.as_array(CORPUS)
    n = len(CORPUS)
    got, st = R.key_agreement.shared_secrets(sk, peers)      # 2 x n pairs, own-major: k_dh_decode once per peer, k_dh_shared per pair
    want, wst = dh_model.shared_batch(sk, peers)
    seen = set()
    for a in range(2):
        for j, (name, _, cls) in enumerate(CORPUS):
            i = a * n + j
            if cls != "valid":
                assert st[i] == 1 and not got[i].any(), (name, cls)
            elif name == "0":
                assert st[i] == 2 and not got[i].any(), name
            else:
                assert st[i] == 0 and got[i].any() and (got[i] == want[i]).all(), name
                seen.add(got[i].tobytes())
    assert (got == want).all() and (st == wst).all()
    assert len(seen) == 2 * (sum(1 for e in CORPUS if e[2] == "valid") - 1)      # (no two pairs share a secret)


def test_feldman_commitments_are_the_corpus(R):
    """one secret per corpus entry, the entry as C_1 at threshold 2.  For the entries whose discrete log is known (0 and k B) the shares are
    those of f(X) = s + k X and feldman_model gives the verdicts from integers; for every valid entry the verdict is also computed as the
    header defines it, y B == C_0 + x C_1, with the oracle's points (an entry of unknown log is consistent with no share)."""
    n = len(CORPUS)
    rng = np.random.default_rng(12)
    secrets = [int.from_bytes(rng.integers(0, 256, 32, dtype=np.uint8).tobytes(), "little") % ELL for _ in range(n)]
    c0 = orc.commit_vec(np.stack([_scalar(s) for s in secrets]), None)
    cm = np.stack([c0, RC.as_array(CORPUS)], axis=1)      # [n, 2, 32]
    xs = [1, 2, 7]
    known = {"0": 0, **{"%dB" % k: k for k in range(1, 17)}}
    shares = np.zeros((n, len(xs), 32), np.uint8)
    for r, (name, _, _) in enumerate(CORPUS):
        for c, x in enumerate(xs):
            shares[r, c] = _scalar(secrets[r] + known.get(name, 1) * x + (c == 1))      # (the middle share is off by one)
    got = R.secret_sharing.verify_shares(cm, xs, shares)
    yb = orc.commit_vec(shares.reshape(-1, 32), None).reshape(n, len(xs), 32)
    one = _scalar(1)
    for r, (name, _, cls) in enumerate(CORPUS):
        if cls != "valid":
            assert got[r].tolist() == [2] * len(xs), (name, cls)
            continue
        want = [0 if (yb[r, c] == orc.msm(np.stack([one, _scalar(x)]), cm[r])).all() else 1 for c, x in enumerate(xs)]
        assert got[r].tolist() == want, (name, got[r], want)
        if name in known:
            assert want == [0, 1, 0] == FM.verdicts([[secrets[r], known[name]]], xs, shares[r:r + 1])[0].tolist(), name
        else:
            assert want == [1, 1, 1], name


# ---------------------------------------------------------------- sites that report per call
def test_add_points_refuses_every_class_in_either_operand(R):
    add = R.pedersen_ops.add_rp_vec
    a, b = RC.honest_points(D), RC.honest_points(D, 7)
    rc, want = orc.add_points_vec(a, b)
    assert rc == 0 and (add(a, b) == want).all()
    for i, rep, p1, p2 in _two_positions():
        for side, pos in ((0, p1), (1, p2)):
            ops = [a.copy(), b.copy()]
            ops[side][pos] = RC.row(rep)
            assert _code(R, lambda: add(*ops)) == 5, (rep[0], side, pos)
            assert orc.add_points_vec(*ops)[0] == 5
    # the valid edges at the block edges, in either operand; then x + (-x), the entry 0 among them: every sum encodes to zeros
    for first in range(0, len(EDGES), len(POS)):
        x = a.copy()
        for pos, e in zip(POS, EDGES[first:first + len(POS)]):
            x[pos] = RC.row(e)
        for ops in ((x, b), (b, x)):
            rc, want = orc.add_points_vec(*ops)
            assert rc == 0 and (add(*ops) == want).all(), first
        for pos, e in zip(POS, EDGES[first:first + len(POS)]):
            assert want[pos].tobytes() == RC.pyref_add(b[pos].tobytes(), e[1]), e[0]
        y = b.copy()
        for pos in POS:
            y[pos] = _neg(x[pos])
        got = add(x, y)
        assert (got == orc.add_points_vec(x, y)[1]).all() and not got[list(POS)].any() and got[1].any()


def test_shift_points_refuses_every_class(R):
    shift = R.pedersen_ops.compute_shifted_values_rp
    pts, off = RC.honest_points(D, 3), RC.row(EDGES[5])
    for i, rep, p1, p2 in _two_positions():
        for pos in (p1, p2):
            bad = pts.copy(); bad[pos] = RC.row(rep)
            assert _code(R, lambda: shift(bad, off)) == 5, (rep[0], pos)
    for first in range(0, len(EDGES), len(POS)):
        x = pts.copy()
        for pos, e in zip(POS, EDGES[first:first + len(POS)]):
            x[pos] = RC.row(e)
        rc, want = orc.add_points_vec(x, np.tile(off, (D, 1)))
        assert rc == 0 and (shift(x, off) == want).all(), first
    for rep in REPS:      # (the offset is decoded on the host)
        assert _code(R, lambda: shift(pts, RC.row(rep))) == 5, rep[0]


def test_sum_points_refuses_every_class(R):
    total = R.pedersen_ops.sum_rp_vec
    pts = RC.honest_points(D, 4)
    ones = np.tile(_scalar(1), (D, 1))
    assert (total(pts) == orc.msm(ones, pts)).all()
    for i, rep, p1, p2 in _two_positions():
        for pos in (p1, p2):
            bad = pts.copy(); bad[pos] = RC.row(rep)
            assert _code(R, lambda: total(bad)) == 5, (rep[0], pos)
    for first in range(0, len(EDGES), len(POS)):
        x = pts.copy()
        for pos, e in zip(POS, EDGES[first:first + len(POS)]):
            x[pos] = RC.row(e)
        assert (total(x) == orc.msm(ones, x)).all(), first


@pytest.fixture(scope="module")
def range_honest():
    """(proofs u8[4, 928], commitments u8[257, 32]) of one honest client from the oracle, read-only"""
    return CC.range_client(D, 4, 1)


def test_range_verify_refuses_invalid_commitments(R, range_honest):
    pr, cm = range_honest
    verify = R.range_proof_vec.verify_rangeproof
    assert verify(pr, cm, NB, verifier_seed=SEED, fp=FP) is True
    for i, rep, p1, p2 in _two_positions():
        for pos in (p1, p2):
            bad = cm.copy(); bad[pos] = RC.row(rep)
            assert _code(R, lambda: verify(pr, bad, NB, verifier_seed=SEED, fp=FP)) == 5, (rep[0], pos)
            assert orc.verify_rangeproof(pr, bad, NB, *FP)[0] == 5
    # the valid edges are decoded and then fail the proof: a verdict, not an error
    for first in range(0, len(EDGES), len(POS)):
        x = cm.copy()
        for pos, e in zip(POS, EDGES[first:first + len(POS)]):
            x[pos] = RC.row(e)
        assert verify(pr, x, NB, verifier_seed=SEED, fp=FP) is False
        assert orc.verify_rangeproof(pr, x, NB, *FP) == (0, False)


def test_range_verify_with_an_undecodable_proof_point_is_false(R, range_honest):
    pr, cm = range_honest
    n_proofs, plen = pr.shape
    lg = (plen // 32 - 9) // 2
    assert CC.ab_offset(plen) == 7 * 32 + 64 * lg
    for i, rep in enumerate(REPS):
        for l, where in enumerate(("A", "S", "T1", "T2", "L", "R")):
            chunk, rnd = (i + l) % n_proofs, (3 * i + l) % lg
            off = 32 * l if l < 4 else 7 * 32 + 64 * rnd + (32 if where == "R" else 0)
            bad = np.array(pr); bad[chunk, off:off + 32] = RC.row(rep)
            assert R.range_proof_vec.verify_rangeproof(bad, cm, NB, verifier_seed=SEED, fp=FP) is False, (rep[0], where, chunk, rnd)
            assert orc.verify_rangeproof(bad, cm, NB, *FP) == (0, False)


def test_discrete_log_refuses_every_class(R):
    rng = np.random.default_rng(13)
    sc = R.conversion32.f32_to_scalar_vec(_values(rng, D), fp=FP)
    pts = R.pedersen_ops.commit_no_blinding_vec(sc)
    m = 1 << 10
    for pos in POS:
        pts[pos] = 0; sc[pos] = 0      # the entry 0: the identity, log 0
    got = R.pedersen_ops.discrete_log_vec(pts, m, 16)
    rc, want = orc.bsgs_solve(pts, m, 16)
    assert rc == 0 and (got == want).all() and (got == sc).all() and not got[list(POS)].any()
    for i, rep, p1, p2 in _two_positions():
        for pos in (p1, p2):
            bad = pts.copy(); bad[pos] = RC.row(rep)
            assert _code(R, lambda: R.pedersen_ops.discrete_log_vec(bad, m, 16)) == 5, (rep[0], pos)
            assert orc.bsgs_solve(bad, m, 16)[0] == 5


def test_accumulator_add_is_all_or_nothing(R):
    A = R.api.accumulator
    recs = [np.ascontiguousarray(np.concatenate([RC.honest_points(D, 5 * c), RC.honest_points(D, 5 * c + 61)], axis=1)) for c in range(3)]

    def add(h, rs):
        A.add(h, [r.ctypes.data for r in rs], [D] * len(rs), 64)
    h = A.create(D, 0)
    try:
        add(h, recs)
        before = A.export(h, D)
        assert (before == _oracle_fold(recs)).all()
        for i, rep, p1, p2 in _two_positions():
            for comp, pos in ((0, p1), (1, p2)):      # a bad L, a bad R, in client 1 of 3
                bad = recs[1].copy(); bad[pos, 32 * comp:32 * comp + 32] = RC.row(rep)
                assert _code(R, lambda: add(h, [recs[0], bad, recs[2]])) == 5, (rep[0], comp, pos)
                assert (A.export(h, D) == before).all(), (rep[0], comp, pos)
        # the valid edges as L of the three clients, at the block edges
        A.reset(h)
        ed = [r.copy() for r in recs]
        for c in range(3):
            for pos, e in zip(POS, EDGES[7 * c:7 * c + 7]):
                ed[c][pos, :32] = RC.row(e)
        add(h, ed)
        assert (A.export(h, D) == _oracle_fold(ed)).all()
    finally:
        A.destroy(h)


def _sigma_verify(R, kind):
    return (R.rand_proof_vec.verify_randproof_vec, R.square_rand_proof_vec.verify_l2rangeproof_vec, R.square_proof_vec.verify_l2rangeproof_vec)[kind]


@pytest.fixture
def sigma_option(R, request):
    """sigma_batch 1 (the default): k_sigma_vdecode + k_sigma_vprep and one MSM per vector; 0: k_sigma_verify, one check per element"""
    R.set_option("sigma_batch", request.param)
    yield request.param
    R.set_option("sigma_batch", 1)


@pytest.mark.parametrize("sigma_option", [1, 0], indirect=True)
@pytest.mark.parametrize("kind", [0, 1, 2])
def test_sigma_verify_refuses_every_class(R, kind, sigma_option):
    pr, cm = CC.sigma_honest(kind, D)
    npts = CC.SIGMA[kind][0]
    verify = _sigma_verify(R, kind)
    assert verify(pr, cm) is True
    for i, rep, p1, p2 in _two_positions():
        # in a commitment, then in a prime commitment (the first npts points of a proof); the component rotates with the class
        for in_proof, comp, pos in ((False, i % npts, p1), (True, (i + 1) % npts, p2)):
            p, c = np.array(pr), np.array(cm)
            (p if in_proof else c)[pos, 32 * comp:32 * comp + 32] = RC.row(rep)
            assert _code(R, lambda: verify(p, c)) == 5, (rep[0], in_proof, comp, pos)
            assert orc.sigma_verify(kind, p, c)[0] == 5


def test_create_existing_refuses_every_class(R):
    rng = np.random.default_rng(14)
    x, r1, r2 = _values(rng, D), CC._scalars(rng, D), CC._scalars(rng, D)
    ns = lambda: R.Nonce.seeded(b"\x15" * 32)      # noqa: E731
    calls = {
        "rand": lambda ex: R.rand_proof_vec.create_randproof_vec_existing(x, ex, r1, nonce=ns(), fp=FP),
        "squarerand": lambda ex: R.square_rand_proof_vec.create_l2rangeproof_vec_existing(x, ex, r1, r2, nonce=ns(), fp=FP),
        "square": lambda ex: R.square_proof_vec.create_l2rangeproof_vec_existing(x, ex, r1, r2, nonce=ns(), fp=FP),
        "compressed": lambda ex: R.compressed_rand_proof.helper_prove_existing(x, ex, r1, nonce=ns(), fp=FP),
    }
    good = RC.honest_points(D, 9)
    for j, e in enumerate(EDGES[:7]):
        good[POS[j]] = RC.row(e)      # (the identity among them: a valid commitment to complete)
    pr, cm = calls["rand"](good)
    rc, opr, ocm = orc.sigma_create(0, x, r1, None, *FP, seed=b"\x15" * 32, existing=good)
    assert rc == 0 and (pr == opr).all() and (cm == ocm).all()
    for i, rep in enumerate(REPS):
        bad = good.copy(); bad[POS[(i + 2) % 7]] = RC.row(rep)
        for name, call in calls.items():
            assert _code(R, lambda: call(bad)) == 5, (rep[0], name)
        assert orc.sigma_create(1, x, r1, r2, *FP, seed=b"\x15" * 32, existing=bad)[0] == 5
        assert orc.compressed_create(x, r1, *FP, seed=b"\x15" * 32, existing=bad)[0] == 5


# ---------------------------------------------------------------- batch sites: a bad member fails alone
def _batch_inputs(seed):
    rng = np.random.default_rng(seed)
    return [_values(rng, D) for _ in range(N_BATCH)], [CC._scalars(rng, D) for _ in range(N_BATCH)], [CC._scalars(rng, D) for _ in range(N_BATCH)]


def _nonces(R, tag):
    return [R.Nonce.seeded(bytes([tag, i + 1]) * 16) for i in range(N_BATCH)]


def test_range_batch_with_bad_commitments(R):
    xs, bls, _ = _batch_inputs(21)
    made = R.range_proof_vec.create_rangeproof_batch(xs, bls, NB, 4, nonces=_nonces(R, 0x21), fp=FP)
    prs, cms = [p for p, _ in made], [c for _, c in made]
    verify = R.range_proof_vec.verify_rangeproof_batch
    repaired = verify(prs, cms, NB, verifier_seed=SEED, fp=FP)
    assert repaired == [True] * N_BATCH
    bad = [c.copy() for c in cms]
    for i, rep in enumerate(REPS):
        bad[i][POS[i]] = RC.row(rep)
    assert verify(prs, bad, NB, verifier_seed=SEED, fp=FP) == WANT_BATCH
    for i in range(7):      # each as the single call and the oracle see it
        assert _code(R, lambda: R.range_proof_vec.verify_rangeproof(prs[i], bad[i], NB, verifier_seed=SEED, fp=FP)) == 5
        assert orc.verify_rangeproof(prs[i], bad[i], NB, *FP)[0] == 5
    # the commitments read in place from 64-byte records (the first 32 bytes of each)
    rec = [np.ascontiguousarray(np.concatenate([c, np.full((D, 32), 0xFF, np.uint8)], axis=1)) for c in bad]
    assert verify(prs, rec, NB, verifier_seed=SEED, fp=FP, commit_stride=64) == WANT_BATCH


def test_l2_sum_proof_with_a_bad_commitment(R):
    """the one commitment of an L2 sum proof (the client's sum of c_sq): k_decode over one point, a member per block in the batch"""
    V = R.l2_range_proof_vec
    prs, cms = CC.l2_batch(N_BATCH, ())
    assert V.verify_rangeproof_l2_batch(prs, cms, CC.L2_BITS, verifier_seed=SEED, fp=FP) == [True] * N_BATCH
    for i, rep in enumerate(REPS):
        cms[i][:] = RC.row(rep)
    assert V.verify_rangeproof_l2_batch(prs, cms, CC.L2_BITS, verifier_seed=SEED, fp=FP) == WANT_BATCH
    for i in range(7):
        assert _code(R, lambda: V.verify_rangeproof_l2(prs[i], cms[i], CC.L2_BITS, verifier_seed=SEED, fp=FP)) == 5, REPS[i][0]
        assert orc.verify_rangeproof_l2(prs[i], cms[i], CC.L2_BITS, *FP)[0] == 5
    for e in EDGES[:4]:      # a valid point that is not the commitment: a verdict
        assert V.verify_rangeproof_l2(prs[8], RC.row(e), CC.L2_BITS, verifier_seed=SEED, fp=FP) is False
        assert orc.verify_rangeproof_l2(prs[8], RC.row(e), CC.L2_BITS, *FP) == (0, False)


@pytest.mark.parametrize("sigma_option", [1, 0], indirect=True)
@pytest.mark.parametrize("where", ["commitments", "prime commitments"])
def test_squarerand_batch_with_bad_points(R, where, sigma_option):
    xs, r1, r2 = _batch_inputs(22)
    made = R.square_rand_proof_vec.create_l2rangeproof_vec_batch(xs, r1, r2, nonces=_nonces(R, 0x22), fp=FP)
    prs, cms = [p.copy() for p, _ in made], [c.copy() for _, c in made]
    verify = R.square_rand_proof_vec.verify_l2rangeproof_vec_batch
    ok0, sums0 = verify(prs, cms, with_csq_sums=True)
    assert ok0 == [True] * N_BATCH
    for i in range(N_BATCH):
        assert (sums0[i] == R.pedersen_ops.sum_rp_vec(np.ascontiguousarray(cms[i][:, 64:96]))).all() and sums0[i].any()
    target = cms if where == "commitments" else prs
    for i, rep in enumerate(REPS):      # L, R, c_sq (or their primes) in turn
        comp = i % 3
        target[i][POS[i], 32 * comp:32 * comp + 32] = RC.row(rep)
    ok, sums = verify(prs, cms, with_csq_sums=True)
    assert ok == WANT_BATCH
    assert not sums[:7].any() and (sums[7:] == sums0[7:]).all()
    assert verify(prs, cms) == WANT_BATCH
    for i in range(7):
        assert _code(R, lambda: R.square_rand_proof_vec.verify_l2rangeproof_vec(prs[i], cms[i])) == 5
        assert orc.sigma_verify(1, prs[i], cms[i])[0] == 5


def test_compressed_batch_with_bad_points(R):
    H = R.compressed_rand_proof
    xs, rs, _ = _batch_inputs(23)
    made = H.helper_prove_batch(xs, rs, nonces=_nonces(R, 0x23), fp=FP)
    pfs, prs = [p.copy() for p, _ in made], [np.ascontiguousarray(c).copy() for _, c in made]
    assert H.helper_verify_batch(pfs, prs) == [True] * N_BATCH
    plan = ["L", "R", "C'.L", "L", "R", "C'.R", "L"]
    for i, (rep, what) in enumerate(zip(REPS, plan)):
        if what[0] == "C":
            off = 0 if what == "C'.L" else 32
            pfs[i][off:off + 32] = RC.row(rep)
        else:
            off = 0 if what == "L" else 32
            prs[i][POS[i], off:off + 32] = RC.row(rep)
    assert H.helper_verify_batch(pfs, prs) == WANT_BATCH
    assert H.helper_verify_batch_strided(pfs, prs, 64) == WANT_BATCH
    recs = [np.ascontiguousarray(np.concatenate([c, np.full((D, 32), 0xFF, np.uint8)], axis=1)) for c in prs]      # c_sq is never read
    assert H.helper_verify_batch_strided(pfs, recs, 96) == WANT_BATCH
    for i in range(7):
        assert _code(R, lambda: H.helper_verify(pfs[i], prs[i])) == 5
        assert orc.compressed_verify(pfs[i], prs[i])[0] == 5


# ---------------------------------------------------------------- the device-resident round
def _copy(u):
    return type(u).deserialize(u.serialize())


def _round_inputs(seed):
    """values k / 128, |k| <= 3 (exact at 7 fraction bits, as tests/test_gpu_round.py draws them), blindings and second blindings"""
    xs, bls, r2 = _batch_inputs(seed)
    return [np.round(x * 3).astype(np.float32) / np.float32(128) for x in xs], bls, r2


def _ptrs(us, attr):
    return [getattr(u, attr).ctypes.data for u in us]


def _check_accumulate(R, rnd, ups, stride, refused, d=D):
    """accumulate_into over the ingested round `ups`: every accept list that holds a member of `refused` (those with an undecodable L or R)
    returns 5 and leaves the accumulator as it was; without them the sum is rofl_acc_add of the accepted members' records"""
    A = R.api.accumulator
    others = [i for i in range(len(ups)) if i not in refused]
    with R.DeviceAccumulator.unity(d) as acc, R.DeviceAccumulator.unity(d) as ref:
        acc.accumulate_pairs(ups[others[-1]].enc_values, stride=stride)      # (not empty, so that "unchanged" says something)
        before = acc.export()
        for accept in [None] + [[j == i or j in others for j in range(len(ups))] for i in refused]:
            assert _code(R, lambda: rnd.accumulate_into(acc, accept=accept)) == 5, accept
            assert (acc.export() == before).all(), accept
        rnd.accumulate_into(acc, accept=[j in others for j in range(len(ups))])
        A.add(ref._h, [ups[j].enc_values.ctypes.data for j in [others[-1]] + others], [d] * (len(others) + 1), stride)
        ex = acc.export()
        assert (ex == ref.export()).all()
        assert (ex == _oracle_fold([ups[j].enc_values for j in [others[-1]] + others])).all()


@pytest.mark.parametrize("name", ["range", "range_compressed"])
def test_round_of_range_updates(R, name):
    """64-byte records L | R: the randomness leg (per-element RandProofs, or the one CompressedRandProof) reads L and R at every index, the
    range leg the first k_checked L, the accumulation L and R"""
    cls = {"range": R.EncParamsRange, "range_compressed": R.EncParamsRangeCompressed}[name]
    check = 0.5
    k = R.params._num_checked(D, check)
    assert k == 129      # a bad L at 128 is the last the range leg reads, at 255 and 256 it is the randomness leg's alone
    xs, bls, _ = _round_inputs(24)
    ups = cls.encrypt_batch(list(zip(xs, bls)), NB, 4, check, nonce_seeds=[bytes([0x24, i + 1]) * 16 for i in range(N_BATCH)], fp=FPR)
    bad = [_copy(u) for u in ups]
    comp = ["L", "R", "L", "R", "L", "R", "L"]
    for i, rep in enumerate(REPS):
        off = 0 if comp[i] == "L" else 32
        bad[i].enc_values[POS[i], off:off + 32] = RC.row(rep)
    # the FIRST bad index of a component decides: member 4 (L at 128) also has a bad L at 256, member 6 (L at 256) also at 255
    bad[4].enc_values[256, :32] = RC.row(REPS[5])
    bad[6].enc_values[255, :32] = RC.row(REPS[3])
    dr = R.api.device_round
    n_proofs, plen = ups[0].range_proofs.shape

    def rand_leg(h, us, proofs=None):
        if name == "range":
            return dr.verify_sigma(h, 0, [p.ctypes.data for p in (proofs or [u.rand_proofs for u in us])])[0]
        return dr.verify_compressed(h, [p.ctypes.data for p in (proofs or [u.rand_proof for u in us])])
    with R.DeviceRound(cls, D, max_clients=N_BATCH) as rnd:
        rnd.ingest(bad)
        assert rand_leg(rnd._h, bad) == WANT_BATCH == cls._rand_batch(bad)
        ok_range = dr.verify_range(rnd._h, _ptrs(bad, "range_proofs"), plen, n_proofs, k, NB, verifier_seed=SEED, fp=FPR)
        assert ok_range == [not (comp[i] == "L" and POS[i] < k) for i in range(7)] + [True] * 2
        assert ok_range == R.range_proof_vec.verify_rangeproof_batch([u.range_proofs for u in bad], [u.enc_values[:k] for u in bad], NB, verifier_seed=SEED, fp=FPR, commit_stride=64)
        assert rnd.verify(verifier_seed=SEED, fp=FPR) == WANT_BATCH == cls.verify_batch(bad, verifier_seed=SEED, fp=FPR)
        _check_accumulate(R, rnd, bad, 64, refused=list(range(7)))
        # the same round with every bad entry repaired
        rnd.reset()
        rnd.ingest(ups)
        assert rand_leg(rnd._h, ups) == [True] * N_BATCH
        # an undecodable prime commitment in a member's proof (decoded per leg, not at ingest) fails that member alone
        primes = [(u.rand_proofs if name == "range" else u.rand_proof).copy() for u in ups]
        for i, rep in enumerate(REPS):
            row = primes[i][POS[i]] if name == "range" else primes[i]
            row[32 * (i % 2):32 * (i % 2) + 32] = RC.row(rep)
        assert rand_leg(rnd._h, ups, primes) == WANT_BATCH
        assert dr.verify_range(rnd._h, _ptrs(ups, "range_proofs"), plen, n_proofs, k, NB, verifier_seed=SEED, fp=FPR) == [True] * N_BATCH
        assert rnd.verify(verifier_seed=SEED, fp=FPR) == [True] * N_BATCH


def test_round_of_l2_compressed_updates(R):
    """96-byte records L | R | c_sq: the Sigma leg (SquareProof) reads L and c_sq, the randomness leg (CompressedRandProof) L and R, the
    range leg L (every index: k = d), the accumulation L and R"""
    cls = R.EncParamsL2CompressedStrict
    xs, bls, r2 = _round_inputs(25)
    ups = cls.encrypt_batch(list(zip(xs, bls, r2)), NB, 2, 32, nonce_seeds=[bytes([0x25, i + 1]) * 16 for i in range(N_BATCH)], fp=FPR)
    assert all(u.enc_values.shape == (D, 96) for u in ups)
    bad = [_copy(u) for u in ups]
    comp = ["L", "R", "csq", "L", "R", "csq", "L"]
    for i, rep in enumerate(REPS):
        off = {"L": 0, "R": 32, "csq": 64}[comp[i]]
        bad[i].enc_values[POS[i], off:off + 32] = RC.row(rep)
    dr = R.api.device_round
    n_proofs, plen = ups[0].range_proofs.shape
    with R.DeviceRound(cls, D, max_clients=N_BATCH) as rnd:
        rnd.ingest(ups)
        ok0, sums0 = dr.verify_sigma(rnd._h, 2, _ptrs(ups, "square_proofs"), want_csq=True)
        assert ok0 == [True] * N_BATCH and rnd.verify(verifier_seed=SEED, fp=FPR) == [True] * N_BATCH
        primes = [u.square_proofs.copy() for u in ups]      # an undecodable c_l' or c_sq' in a member's proofs fails that member alone
        for i, rep in enumerate(REPS):
            primes[i][POS[i], 32 * (i % 2):32 * (i % 2) + 32] = RC.row(rep)
        okp, sumsp = dr.verify_sigma(rnd._h, 2, [p.ctypes.data for p in primes], want_csq=True)
        assert okp == WANT_BATCH and not sumsp[:7].any() and (sumsp[7:] == sums0[7:]).all()
        rnd.reset()
        rnd.ingest(bad)
        ok, sums = dr.verify_sigma(rnd._h, 2, _ptrs(bad, "square_proofs"), want_csq=True)
        assert ok == [comp[i] == "R" for i in range(7)] + [True] * 2      # this arm never reads R
        for i in range(N_BATCH):
            if ok[i]:
                assert (sums[i] == sums0[i]).all() and sums[i].any(), i
            else:
                assert not sums[i].any(), i
        want, wsums = cls._square_batch(bad)
        assert ok == want and (sums == wsums).all()
        ok_rand = dr.verify_compressed(rnd._h, _ptrs(bad, "rand_proof"))
        assert ok_rand == [comp[i] == "csq" for i in range(7)] + [True] * 2      # an undecodable c_sq is the Sigma leg's failure, not this leg's
        assert ok_rand == R.compressed_rand_proof.helper_verify_batch_strided([u.rand_proof for u in bad], [u.enc_values for u in bad], 96)
        ok_range = dr.verify_range(rnd._h, _ptrs(bad, "range_proofs"), plen, n_proofs, D, NB, verifier_seed=SEED, fp=FPR)
        assert ok_range == [comp[i] != "L" for i in range(7)] + [True] * 2
        assert rnd.verify(verifier_seed=SEED, fp=FPR) == WANT_BATCH == cls.verify_batch(bad, verifier_seed=SEED, fp=FPR)
        # a member whose only bad point is c_sq can be added (the sum reads L and R), one with a bad L or R cannot
        _check_accumulate(R, rnd, bad, 96, refused=[i for i in range(7) if comp[i] != "csq"])
