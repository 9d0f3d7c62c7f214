"""GPU checks of the complaint proofs (rofl_dleq_prove: k_dh_public, k_dh_decode, k_dleq_prove; rofl_dleq_verify: k_dh_decode, k_dleq_verify),
byte for byte against the Python model tests/dleq_model.py -- no tolerance anywhere: block positions around the 64-thread block, the pair
indexing, every verdict class in one wave, the decoder's late-reject classes at every decode site, extreme scalars as keys, the joint
variable-base chain against the composition it replaces, the six-client round with five complaints judged in one call, and the shapes that
must not touch the device."""
import ctypes
import json

import numpy as np
import pytest

import dh_model as D
import dleq_model as Q
import orc
import ristretto_corpus as RC
import test_dleq_host as H

pytestmark = pytest.mark.gpu
FP = (32, 7)
ELL = Q.L
sz, vp = ctypes.c_size_t, ctypes.c_void_p


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


@pytest.fixture(scope="module")
def batch257():
    """257 pairs (key i, peer i, ctx i) proved by the model once and never changed: (sks, pks, peers, ctxs, reveals, proofs, shared)"""
    rng = np.random.default_rng(20270110)
    n = 257
    sks, peers, ctxs = D.rand_keys(rng, n), H._pk(D.rand_keys(rng, n)), _rows(rng, n)
    pairs = [(i, i) for i in range(n)]
    reveals, proofs, status = Q.prove_batch(sks, peers, ctxs, pairs)
    pks = H._pk(sks)
    verdicts, shared = Q.verify_batch(pks, peers, ctxs, reveals, proofs, pairs)
    assert not status.any() and not verdicts.any()
    return sks, pks, peers, ctxs, reveals, proofs, shared


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_block_positions(R, batch257, n):
    """the kernels' block is 64 threads: one thread, one short of a block, a block, one more, several blocks and a ragged one"""
    sks, pks, peers, ctxs, reveals, proofs, shared = (x[:n] for x in batch257)
    pairs = [(i, i) for i in range(n)]
    r, p, st, own = R.dleq.prove(sks, peers, ctxs, pairs, with_public=True)
    assert r.tobytes() == reveals.tobytes() and p.tobytes() == proofs.tobytes() and not st.any() and own.tobytes() == pks.tobytes()
    v, sh = R.dleq.verify(pks, peers, ctxs, r, p, pairs)
    assert not v.any() and sh.tobytes() == shared.tobytes()
    ka, kst = R.key_agreement.shared_secrets(sks, peers, pairs)
    assert sh.tobytes() == ka.tobytes() and not kst.any()
    # flips in the LAST proof and in proof n / 2: exactly those verdicts, zero secrets, the others untouched
    hit = sorted({n - 1, n // 2})
    bad = p.copy()
    for k, i in enumerate(hit):
        bad[i, 63 if k else 0] ^= 0x01
    v, sh = R.dleq.verify(pks, peers, ctxs, r, bad, pairs)
    mv, ms = Q.verify_batch(pks[hit], peers[hit], ctxs[hit], r[hit], bad[hit], [(i, i) for i in range(len(hit))])
    assert np.flatnonzero(v).tolist() == hit and v[hit].tolist() == mv.tolist() and not sh[hit].any()
    keep = [i for i in range(n) if i not in hit]
    assert sh[keep].tobytes() == shared[keep].tobytes()


def test_pairs_null_equals_explicit_in_shuffled_order(R):
    rng = np.random.default_rng(20270111)
    sks, peers, ctxs = D.rand_keys(rng, 3), H._pk(D.rand_keys(rng, 5)), _rows(rng, 15)
    r, p, st, pk = R.dleq.prove(sks, peers, ctxs, with_public=True)
    want = Q.prove_batch(sks, peers, ctxs)
    assert r.tobytes() == want[0].tobytes() and p.tobytes() == want[1].tobytes() and not st.any()
    order = rng.permutation(15)
    pairs = [(int(i) // 5, int(i) % 5) for i in order]
    r2, p2, st2 = R.dleq.prove(sks, peers, ctxs[order], pairs)
    assert r2.tobytes() == r[order].tobytes() and p2.tobytes() == p[order].tobytes() and not st2.any()
    v, sh = R.dleq.verify(pk, peers, ctxs, r, p)
    v2, sh2 = R.dleq.verify(pk, peers, ctxs[order], r2, p2, pairs)
    assert not v.any() and not v2.any() and sh2.tobytes() == sh[order].tobytes() == D.shared_batch(sks, peers, pairs)[0].tobytes()
    # one key in many pairs, one pair many times
    many = [(2, 4)] * 3 + [(2, b) for b in range(5)]
    cx = np.concatenate([ctxs[[14, 0, 14]], ctxs[10:15]])
    r3, p3, _ = R.dleq.prove(sks, peers, cx, many)
    assert r3.tobytes() == Q.prove_batch(sks, peers, cx, many)[0].tobytes() and p3[0].tobytes() == p3[2].tobytes() == p[14].tobytes() != p3[1].tobytes()
    assert not R.dleq.verify(pk, peers, cx, r3, p3, many)[0].any()


def test_every_verdict_class_in_one_wave(R, batch257):
    sks, pks, peers = batch257[0][:6], batch257[1][:6], batch257[2]
    own, prs, cx, reveals, proofs, want = Q.verdict_cases(sks, pks, peers[0], batch257[3][:6])
    assert len(want) <= 64 and set(want.tolist()) == {0, 1, 2}
    pairs = [(i, i) for i in range(len(want))]
    mv, ms = Q.verify_batch(own, prs, cx, reveals, proofs, pairs)
    assert (mv == want).all()
    got, shared = R.dleq.verify(own, prs, cx, reveals, proofs, pairs)
    assert (got == want).all(), (got.tolist(), want.tolist())
    assert shared.tobytes() == ms.tobytes() and all(shared[i].any() == (want[i] == 0) for i in range(len(want)))
    # the host route says the same
    hv, hs = H.lib_verify(R.lib(), own, prs, cx, reveals, proofs, pairs)
    assert (hv == got).all() and hs.tobytes() == shared.tobytes()


def test_late_reject_classes_at_every_decode_site(R, batch257):
    sks, pks, peers, ctxs = (x[:1] for x in batch257[:4])
    bad = [e for cls in H.LATE for e in RC.of_class(cls)[:2]]
    rows = RC.as_array(bad)
    n = len(rows)
    table = np.concatenate([rows, peers])
    cx = np.tile(ctxs[0], (n + 1, 1))
    r, p, st = R.dleq.prove(sks, table, cx)
    want = Q.prove_batch(sks, table, cx)
    assert st.tolist() == [1] * n + [0] == want[2].tolist() and r.tobytes() == want[0].tobytes() and p.tobytes() == want[1].tobytes()
    for site in range(3):
        own, prs, rv = np.tile(pks[0], (n + 1, 1)), np.tile(peers[0], (n + 1, 1)), np.tile(r[n], (n + 1, 1))
        (own, prs, rv)[site][:n] = rows
        pairs = [(i, i) for i in range(n + 1)]
        v, sh = R.dleq.verify(own, prs, cx, rv, np.tile(p[n], (n + 1, 1)), pairs)
        mv, ms = Q.verify_batch(own, prs, cx, rv, np.tile(p[n], (n + 1, 1)), pairs)
        assert v.tolist() == [2] * n + [0] == mv.tolist() and sh.tobytes() == ms.tobytes(), site


@pytest.mark.parametrize("family", ["random", "all_equal", "top_range", "two_pow_252", "small", "minus_one"])
def test_extreme_scalars_as_keys(R, batch257, family):
    keys = orc.extreme_scalar_cases(np.random.default_rng(20270112), 8)[family].copy()
    peers, ctxs = batch257[2][:8], batch257[3][:8]
    pairs = [(i, i) for i in range(8)]
    if family == "small":                                                           # the family starts at zero: refused by index, before the device
        with pytest.raises(R.RoflError) as e:
            R.dleq.prove(keys, peers, ctxs, pairs)
        assert e.value.code == 11 and "secret key 0 is zero" in str(e.value)
        keys, peers, ctxs, pairs = keys[1:], peers[1:], ctxs[1:], pairs[:7]
    r, p, st, pk = R.dleq.prove(keys, peers, ctxs, pairs, with_public=True)
    want = Q.prove_batch(keys, peers, ctxs, pairs)
    assert r.tobytes() == want[0].tobytes() and p.tobytes() == want[1].tobytes() and not st.any() and pk.tobytes() == H._pk(keys).tobytes()
    v, sh = R.dleq.verify(pk, peers, ctxs, r, p, pairs)
    assert not v.any() and sh.tobytes() == D.shared_batch(keys, peers, pairs)[0].tobytes()
    assert (R.dleq.verify(pk, peers, np.roll(ctxs, 1, axis=0), r, p, pairs)[0] == 1).all()


def _var_mul(R, name, k1, p1, k2, p2):
    k1, p1, k2, p2 = (np.ascontiguousarray(np.asarray(x, np.uint8).reshape(-1, 32)) for x in (k1, p1, k2, p2))
    out = np.full((len(k1), 32), 0xaa, np.uint8)
    fn = getattr(R.lib(), name)
    fn.argtypes = [sz, vp, vp, vp, vp, vp, vp]
    assert fn(len(k1), k1.ctypes.data, p1.ctypes.data, k2.ctypes.data, p2.ctypes.data, out.ctypes.data, None) == 0
    return out


def test_joint_chain_equals_the_composition_and_the_model(R, batch257):
    """sg_var_mul2 (rofl_dbg_var_mul2) against gd_add(sg_var_mul, sg_var_mul) (rofl_dbg_var_mul_sum) and the model: the edge scalars in both
    positions, sums that are the identity (the chain passes through it), and random cases"""
    rng = np.random.default_rng(20270114)
    pts = batch257[2]
    edge = [0, 1, ELL - 1, int.from_bytes(b"\x88" * 32, "little"), (2 ** 256 - 1) % ELL, 2 ** 252]
    cases = [(a, pts[0], b, pts[1]) for a in edge for b in edge]
    ks = [int.from_bytes(rng.bytes(32), "little") % ELL for _ in range(6)] + [1, ELL - 1]
    cases += [(k, pts[2], ELL - k, pts[2]) for k in ks]                               # P1 = P2, k2 = l - k1: the identity
    neg = np.frombuffer(Q.lin([(ELL - 1, pts[3])]), np.uint8)
    cases += [(k, pts[3], k, neg) for k in ks]                                        # P2 = -P1, k1 = k2: the identity
    cases += [(int.from_bytes(rng.bytes(32), "little"), pts[4 + i], int.from_bytes(rng.bytes(32), "little"), pts[100 + i]) for i in range(64)]      # (some >= l: reduced)
    k1 = np.stack([H._b32(c[0]) for c in cases]); k2 = np.stack([H._b32(c[2]) for c in cases])
    p1 = np.stack([c[1] for c in cases]); p2 = np.stack([c[3] for c in cases])
    want = b"".join(Q.lin([(c[0], c[1]), (c[2], c[3])]) for c in cases)
    joint, comp = _var_mul(R, "rofl_dbg_var_mul2", k1, p1, k2, p2), _var_mul(R, "rofl_dbg_var_mul_sum", k1, p1, k2, p2)
    assert joint.tobytes() == comp.tobytes() == want
    assert not joint[36:36 + 16].any() and joint[:36].any()


def test_the_round_with_five_complaints(R, monkeypatch):
    """test_gpu_aead.py's six clients, threshold 4, round 7: every bundle sealed and signed, five complaints judged in ONE judge_complaints call"""
    K, S, G = R.key_agreement, R.secret_sharing, R.signatures
    N, T, RND = Q.N, Q.THRESHOLD, Q.ROUND_NO
    rng = np.random.default_rng(20270113)
    ids = list(range(N))
    sk, b, cs = D.rand_keys(rng, N), rng.integers(0, 256, size=(N, 32), dtype=np.uint8), rng.integers(0, 256, size=(2 * N, 32), dtype=np.uint8)
    key_sh, self_sh = S.share(sk, cs[:N], T, N), S.share(b, cs[N:], T, N)                      # [dealer, holder, 32]
    com = S.commit(np.concatenate([sk, b]), cs, T)
    ch_sk, sig_sk = D.rand_keys(rng, N), D.rand_keys(rng, N)
    ch_pk, sig_pk = K.public_keys(ch_sk), G.public_keys(sig_sk)
    dealt = Q.deal_with_faults(key_sh)
    sent = Q.alter_before_signing(S.seal_shares(ch_sk, ids, ids, ch_pk, RND, dealt, self_sh))
    sigs = S.sign_bundles(sig_sk, RND, ids, ids, sent)
    assert not S.verify_bundle_signatures(sig_pk, RND, ids, ids, sent, sigs).any()
    # what client 3 opened from dealer 5 fails the Feldman check: the ground of the first complaint
    ks3, ss3, v3 = S.open_shares(ch_sk[3:4], [3], ids, ch_pk, RND, sent[:, 3][None].copy())
    assert not v3.any() and ks3[0, 5].tobytes() == dealt[5, 3].tobytes() != key_sh[5, 3].tobytes()
    assert S.verify_shares(com[[5, N + 5]], [4], np.stack([ks3[0, 5], ss3[0, 5]])[:, None, :]).tolist() == [[1], [0]]

    def reveal_and_proof(c, d, round_no):
        rv, pf = S.file_complaints(ch_sk[c:c + 1], [c], ids, ch_pk, round_no, [(c, d)])
        return rv[0], pf[0]

    complaints = Q.round_complaints(sent, sigs, reveal_and_proof)
    counts, kept = {}, {}

    def counted(cls, name):
        inner = getattr(cls, name)

        def call(*a, **kw):
            counts[cls.__name__ + "." + name] = counts.get(cls.__name__ + "." + name, 0) + 1
            out = inner(*a, **kw)
            if cls is R.dleq:
                kept["shared"] = out[1].copy()
            return out
        monkeypatch.setattr(cls, name, staticmethod(call))

    counted(R.signatures, "verify"); counted(R.dleq, "verify"); counted(R.aead, "open"); counted(R.secret_sharing, "verify_shares")
    got = S.judge_complaints(RND, complaints, ch_pk, sig_pk, com[:N], com[N:])
    monkeypatch.undo()
    assert got == Q.RULINGS
    assert counts == {"signatures.verify": 1, "dleq.verify": 1, "aead.open": 1, "secret_sharing.verify_shares": 1}
    # the secret the judge derived for the first complaint is the pair's, and opens dealer 5's record to the 64 bytes client 3 opened
    assert kept["shared"][0].tobytes() == K.shared_secrets(ch_sk[3:4], ch_pk[5:6])[0][0].tobytes()
    pt, v = R.aead.open(kept["shared"][:1], [S.bundle_nonce(5, 3)], [S.bundle_ad(RND, 5, 3)], sent[5, 3][None].copy(), derive_round=RND)
    assert v.tolist() == [0] and pt[0].tobytes() == ks3[0, 5].tobytes() + ss3[0, 5].tobytes()
    assert not kept["shared"][3].any() and kept["shared"][2].any()                              # no secret for the proof that failed


def test_an_empty_call_and_the_library_checks_through_the_wrapper(R):
    G = R.dleq
    z = np.zeros((0, 32), np.uint8)
    r, p, st = G.prove(z, z, z)
    assert r.shape == (0, 32) and p.shape == (0, 64) and st.shape == (0,)
    v, sh = G.verify(z, z, z, z, np.zeros((0, 64), np.uint8))
    assert v.shape == (0,) and sh.shape == (0, 32)
    with pytest.raises(R.RoflError) as e:
        G.prove(H._b32(ELL).reshape(1, 32), np.frombuffer(D.BASE_ENC, np.uint8).reshape(1, 32), np.zeros((1, 32), np.uint8))
    assert e.value.code == 11 and "secret key 0 is zero" in str(e.value)
    # shared_out32 may be NULL on the device route as well
    vec = json.load(open(H.GOLDEN))["vectors"][:3]
    col = lambda name, w: np.frombuffer(bytes.fromhex("".join(x[name] for x in vec)), np.uint8).reshape(-1, w).copy()      # noqa: E731
    got, shared = H.lib_verify(R.lib(), H._pk(col("key", 32)), col("peer", 32), col("ctx", 32), col("reveal", 32), col("proof", 64), [(i, i) for i in range(3)], name="rofl_dleq_verify")
    assert not got.any() and shared.tobytes() == col("shared", 32).tobytes()
    r, p, st, _ = H.lib_prove(R.lib(), col("key", 32), col("peer", 32), col("ctx", 32), [(i, i) for i in range(3)], name="rofl_dleq_prove")
    assert r.tobytes() == col("reveal", 32).tobytes() and p.tobytes() == col("proof", 64).tobytes() and not st.any()
