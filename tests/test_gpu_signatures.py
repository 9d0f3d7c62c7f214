"""rofl_sig_sign / rofl_sig_verify on the device against the Python model of the definition (tests/sig_model.py), byte for byte, no tolerance.

The sign and verify kernels run one thread per signature in blocks of 64, so n in {1, 63, 64, 65, 257} is one lane, a wave short of one, a
full one, a crossing, and several blocks with a ragged tail.  The digest kernel runs one thread per message: the block-end lengths of
sig_model.LENS go into ONE call, at starts that are no multiple of 8, so the lanes of a wave run different numbers of permutations and every
word is put together from two aligned ones.  Good and bad signatures of every verdict class share a wave; one key signs 65 messages and 65
keys sign one (the view shape); the extreme-scalar families serve as keys.  Then one round: the six-client, d = 257, threshold-4
double-masked round of test_gpu_feldman.py with every dealer signing its commitments."""
import ctypes

import numpy as np
import pytest

import dh_model as D
import feldman_model as F
import orc
import shamir_model as M
import sig_model as S

pytestmark = pytest.mark.gpu
FP = (32, 7)
ELL = S.L
ROUND_NO = 7
sz, vp = ctypes.c_size_t, ctypes.c_void_p


@pytest.fixture(scope="module")
def R():
    import rofl_project_code_amd as R
    from rofl_project_code_amd import build
    build.build()
    R.set_device(0)
    R.api.set_fp(*FP)
    return R


def _b32(v):
    return np.frombuffer(int(v).to_bytes(32, "little"), np.uint8)


@pytest.fixture(scope="module")
def batch257():
    """257 keys (1, l - 1, s + l, 2^256 - 1, then random bytes), 257 messages of 0 .. 299 bytes, the model's public keys and signatures:
    computed once, never changed"""
    rng = np.random.default_rng(20261110)
    s = int.from_bytes(rng.bytes(31), "little")
    sks = D.rand_keys(rng, 257)
    for i, v in enumerate((1, ELL - 1, s + ELL, 2 ** 256 - 1)):
        sks[i] = _b32(v)
    msgs = [rng.bytes(int(n)) for n in rng.integers(0, 300, size=257)]
    pks = np.frombuffer(b"".join(S.public_key(k) for k in sks), np.uint8).reshape(257, 32).copy()
    sigs = S.sign_batch(sks, msgs)
    for a in (sks, pks, sigs):
        a.setflags(write=False)
    return sks, pks, msgs, sigs


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_block_sizes(R, batch257, n):
    G = R.signatures
    sks, pks, msgs, sigs = batch257
    got, pk = G.sign(sks[:n], msgs[:n], with_public=True)
    assert got.shape == (n, 64) and got.tobytes() == sigs[:n].tobytes()
    assert pk.tobytes() == pks[:n].tobytes()
    assert not G.verify(pks[:n], msgs[:n], got).any()
    # the last signature of the call, and with it the last lane of the ragged block, is really checked
    bad = got.copy(); bad[n - 1, 40] ^= 1; bad[n // 2, 1] ^= 0x10
    want = np.zeros(n, np.uint8); want[n - 1] = 1; want[n // 2] = 1
    assert (G.verify(pks[:n], msgs[:n], bad) == want).all()


def _host(R, name, argtypes, *args):
    fn = getattr(R.api.lib(), name)
    fn.argtypes = argtypes
    return fn(*[None if a is None else a if isinstance(a, int) else a.ctypes.data for a in args])


def test_every_padding_case_in_one_call_and_the_host_route_agrees(R, batch257):
    G = R.signatures
    sks = batch257[0]
    rng = np.random.default_rng(20261111)
    msgs, where = S.misaligned_messages(rng)
    com64 = rng.integers(0, 256, size=(64, 32), dtype=np.uint8)
    for long in (S.commitment_message(7, 3, 1, com64), rng.bytes(2085), rng.bytes(10007)):      # 16, 16 and 74 blocks beside lanes of one
        msgs.append(rng.bytes(1 if sum(len(m) for m in msgs) % 2 == 0 else 2))
        msgs.append(long)
    data, off = S.pack(msgs)
    assert [len(msgs[w]) for w in where] == list(S.LENS) and {int(off[w]) % 8 for w in where} == set(range(1, 8)) and len(msgs) < 64
    keys = sks[:len(msgs)]
    want = S.sign_batch(keys, msgs)
    got, pk = G.sign(keys, msgs, with_public=True)
    assert got.tobytes() == want.tobytes()
    assert not G.verify(pk, msgs, got).any()
    # the digest of every message is really in its signature: each message with its last byte changed (the empty one: with a byte added)
    changed = [(m[:-1] + bytes([m[-1] ^ 1])) if m else b"\0" for m in msgs]
    assert (G.verify(pk, changed, got) == 1).all()
    # the host route gives the device's bytes and verdicts
    n = len(msgs)
    hs, hp, hv = np.zeros((n, 64), np.uint8), np.zeros((n, 32), np.uint8), np.full(n, 9, np.uint8)
    assert _host(R, "rofl_dbg_host_sig_sign", [sz, vp, vp, sz, vp, vp, sz, vp, vp], n, np.ascontiguousarray(keys), hp, n, data, off, n, None, hs) == 0
    assert hs.tobytes() == got.tobytes() and hp.tobytes() == pk.tobytes()
    bad = got.copy(); bad[5, 33] ^= 2
    assert _host(R, "rofl_dbg_host_sig_verify", [sz, vp, sz, vp, vp, sz, vp, vp, vp], n, hp, n, data, off, n, None, bad, hv) == 0
    assert (hv == G.verify(pk, msgs, bad)).all() and np.flatnonzero(hv).tolist() == [5]
    # empty messages alone: no message bytes at all
    e = G.sign(keys[:3], [b"", b"", b""])
    assert e.tobytes() == S.sign_batch(keys[:3], [b""] * 3).tobytes() and not G.verify(pk[:3], [b""] * 3, e).any()


def test_every_verdict_class_in_one_wave(R, batch257):
    G = R.signatures
    sks, pks, msgs, sigs = batch257
    pick = [i for i in range(4, 257) if len(msgs[i]) > 11][:5]
    keys, ms, sg, want = S.verdict_cases(pks[pick], [msgs[i] for i in pick], sigs[pick])
    assert len(want) <= 64 and set(want.tolist()) == {0, 1, 2}
    assert (S.verify_batch(keys, ms, sg) == want).all()
    got = G.verify(keys, ms, sg)
    assert (got == want).all(), (got.tolist(), want.tolist())
    # a refused key condemns its signatures, not the call: the same through refs, the refused key shared by two signatures
    refs = [(i, i) for i in range(len(want))] + [(7, 0), (0, 0)]
    assert want[7] == 2 and want[0] == 0
    got = G.verify(keys, ms, np.concatenate([sg, sg[[0, 0]]]), refs)
    assert (got == np.concatenate([want, [2, 0]])).all()


def test_one_key_many_messages_and_many_keys_one_message(R, batch257):
    G = R.signatures
    sks, pks, msgs, sigs = batch257
    refs = [(0, b) for b in range(65)]
    got = G.sign(sks[9:10], msgs[:65], refs)
    assert got.tobytes() == S.sign_batch(sks[9:10], msgs[:65], refs).tobytes() and got[9].tobytes() == sigs[9].tobytes()
    bad = got.copy(); bad[64, 0] ^= 4
    assert np.flatnonzero(G.verify(pks[9:10], msgs[:65], bad, refs)).tolist() == [64]
    # the view shape: 65 keys on ONE message
    view = msgs[200] + b"view"
    refs = [(a, 0) for a in range(65)]
    got = G.sign(sks[:65], [view], refs)
    assert got.tobytes() == S.sign_batch(sks[:65], [view], refs).tobytes()
    bad = got.copy(); bad[63, 63] ^= 0x08; bad[64] = got[0]
    assert np.flatnonzero(G.verify(pks[:65], [view], bad, refs)).tolist() == [63, 64]
    assert (R.secret_sharing.verify_views(pks[:65], view, bad) == G.verify(pks[:65], [view], bad, refs)).all()
    # refs in any order with repeats, and refs = None equal to (i, i)
    refs = [(4, 0), (0, 4), (4, 0), (1, 1)]
    assert G.sign(sks[:5], msgs[:5], refs).tobytes() == S.sign_batch(sks[:5], msgs[:5], refs).tobytes()
    assert G.sign(sks[:5], msgs[:5], [(i, i) for i in range(5)]).tobytes() == sigs[:5].tobytes()


@pytest.mark.parametrize("family", ["random", "all_equal", "top_range", "two_pow_252", "small", "minus_one"])
def test_extreme_scalars_as_keys(R, family):
    G = R.signatures
    keys = orc.extreme_scalar_cases(np.random.default_rng(20261112), 8)[family].copy()
    msgs = [b"m%d" % i * i for i in range(8)]
    if family == "small":                                                           # the family starts at zero: refused by index, before the device
        with pytest.raises(R.RoflError) as e:
            G.sign(keys, msgs)
        assert e.value.code == 11 and "secret key 0 is zero" in str(e.value)
        keys, msgs = keys[1:], msgs[1:]
    got, pk = G.sign(keys, msgs, with_public=True)
    assert got.tobytes() == S.sign_batch(keys, msgs).tobytes()
    assert pk.tobytes() == b"".join(S.public_key(k) for k in keys) == R.key_agreement.public_keys(keys).tobytes()
    assert not G.verify(pk, msgs, got).any()
    assert (G.verify(pk, msgs[1:] + msgs[:1], got) == 1).all()


def test_an_empty_call_and_the_library_checks_through_the_wrapper(R):
    G = R.signatures
    assert G.sign(np.zeros((0, 32), np.uint8), []).shape == (0, 64)
    assert G.verify(np.zeros((0, 32), np.uint8), [], np.zeros((0, 64), np.uint8)).shape == (0,)
    with pytest.raises(R.RoflError) as e:
        G.sign(_b32(ELL).reshape(1, 32), [b"x"])
    assert e.value.code == 11


# ---------------------------------------------------------------- one round end to end
N, D_DIM, THRESHOLD = 6, 257, 4
GONE = 2
SURVIVORS = [0, 1, 3, 4, 5]


def _value_scalars():
    tab = {}
    for k in range(-128, 128):
        rc, s = orc.f32_to_scalar(k / 128.0, *FP)
        assert rc == 0
        tab[k] = s.copy()
    return tab


@pytest.fixture(scope="module")
def signed_round(R):
    """the round of test_gpu_feldman.py -- six clients, d = 257, threshold 4, client 2 never submits, every dealer publishes the commitments of
    both its sharings -- with a signing key per client and every dealer's two signatures (ONE sign call).  Built once, never changed."""
    P, K, SS, G = R.pedersen_ops, R.key_agreement, R.secret_sharing, R.signatures
    rng = np.random.default_rng(20261024)
    sk, b = D.rand_keys(rng, N), rng.integers(0, 256, size=(N, 32), dtype=np.uint8)
    pk = K.public_keys(sk)
    peers = P.pairwise_peers_from_keys(clients=[(i, sk[i]) for i in range(N)], public_keys=pk, round_no=ROUND_NO)
    bl = P.double_masked_blinding_vecs([(i, peers[i], b[i]) for i in range(N)], ROUND_NO, D_DIM)
    cs = rng.integers(0, 256, size=(2 * N, 32), dtype=np.uint8)
    key_sh, self_sh = SS.share(sk, cs[:N], THRESHOLD, N), SS.share(b, cs[N:], THRESHOLD, N)      # [owner, holder, 32]
    both = SS.commit(np.concatenate([sk, b]), cs, THRESHOLD)
    key_com, self_com = both[:N].copy(), both[N:].copy()
    tab = _value_scalars()
    ks = [rng.integers(-20, 21, size=D_DIM) for _ in range(N)]
    recs = []
    for i in range(N):
        x = np.stack([tab[int(k)] for k in ks[i]])
        recs.append(np.ascontiguousarray(np.concatenate([orc.commit_vec(x, bl[i]), orc.commit_vec(bl[i], None)], axis=1)))
    want = np.sum(np.stack([(ks[i] / 128.0).astype(np.float32) for i in SURVIVORS]).astype(np.float64), axis=0).astype(np.float32)
    # signing keys of their own -- NOT the key-agreement keys, which a dropout reveals
    sig_sk = D.rand_keys(np.random.default_rng(20261113), N)
    sig_pk = G.public_keys(sig_sk)
    sigs = SS.sign_commitments(sig_sk, ROUND_NO, range(N), key_com, self_com)
    # another polynomial for dealer 1's self secret (the same secret under another coefficient seed), signed by dealer 1 as well: equivocation
    other = SS.commit(b[1:2], cs[:1], THRESHOLD)[0]
    other_sig = G.sign(sig_sk[1:2], [SS.commitment_message(ROUND_NO, 1, 1, other)])[0]
    for a in (pk, key_sh, self_sh, key_com, self_com, sig_pk, sigs, other, other_sig):
        a.setflags(write=False)
    return dict(pk=pk, key_sh=key_sh, self_sh=self_sh, key_com=key_com, self_com=self_com, recs=recs, want=want.tobytes(), sig_sk=sig_sk, sig_pk=sig_pk,
                sigs=sigs, other=other, other_sig=other_sig)


def test_every_dealer_signs_its_commitments(R, signed_round):
    rd, SS = signed_round, R.secret_sharing
    assert rd["sigs"].shape == (N, 2, 64)
    assert rd["sig_pk"].tobytes() == b"".join(S.public_key(k) for k in rd["sig_sk"])
    for d in range(N):
        assert rd["sigs"][d, 0].tobytes() == S.sign(rd["sig_sk"][d], S.commitment_message(ROUND_NO, d, 0, rd["key_com"][d]))
        assert rd["sigs"][d, 1].tobytes() == S.sign(rd["sig_sk"][d], S.commitment_message(ROUND_NO, d, 1, rd["self_com"][d]))
    assert not SS.verify_commitment_signatures(rd["sig_pk"], ROUND_NO, range(N), rd["key_com"], rd["self_com"], rd["sigs"]).any()
    # a relay that substitutes dealer 1's self commitments is seen by everyone who checks
    tam = rd["self_com"].copy(); tam[1] = rd["other"]
    assert SS.verify_commitment_signatures(rd["sig_pk"], ROUND_NO, range(N), rd["key_com"], tam, rd["sigs"]).tolist() == [[0, 0], [0, 1]] + [[0, 0]] * 4
    assert R.secret_sharing.commitment_message(ROUND_NO, 1, 1, rd["other"]) == S.commitment_message(ROUND_NO, 1, 1, rd["other"])


def _verified_args(rd, holders, self_com=None):
    self_com = {i: rd["self_com"][i] for i in SURVIVORS} if self_com is None else self_com
    return (SURVIVORS, [GONE], [h + 1 for h in holders], {GONE: rd["key_sh"][GONE, holders]}, {i: rd["self_sh"][i, holders] for i in SURVIVORS},
            {GONE: rd["key_com"][GONE]}, self_com, rd["pk"], ROUND_NO)


def test_the_signed_route_gives_the_verified_routes_terms_and_sum(R, signed_round):
    rd, P = signed_round, R.pedersen_ops
    holders = SURVIVORS
    csigs = {GONE: rd["sigs"][GONE, 0], **{i: rd["sigs"][i, 1] for i in SURVIVORS}}
    terms_v, liars_v = P.dropout_residual_terms_from_verified_shares(*_verified_args(rd, holders))
    terms, liars = P.dropout_residual_terms_from_signed_shares(*_verified_args(rd, holders), rd["sig_pk"], csigs)
    assert (terms, liars) == (terms_v, liars_v) and liars == []
    a = R.DeviceAccumulator(D_DIM)
    with a:
        for i in SURVIVORS:
            a.accumulate_pairs(rd["recs"][i])
        got = a.extract_opened(opening_terms=terms)
        assert got is not None and got.tobytes() == rd["want"]
    # dealer 1's self commitments swapped for another polynomial's after signing: the signed route names dealer 1 ...
    swapped = {i: rd["self_com"][i] for i in SURVIVORS}
    swapped[1] = rd["other"]
    with pytest.raises(ValueError, match=r"client 1\b.*self-mask commitments does not verify"):
        P.dropout_residual_terms_from_signed_shares(*_verified_args(rd, holders, swapped), rd["sig_pk"], csigs)
    # ... where the unsigned route blames the honest survivors: every share of that secret fails the foreign commitments
    with pytest.raises(ValueError, match=r"survivors \[0, 1, 3, 4, 5\]"):
        P.dropout_residual_terms_from_verified_shares(*_verified_args(rd, holders, swapped))
    # a missing signature and the key signature in the place of the self one name their dealer too
    with pytest.raises(ValueError, match=r"client 4\b.*no signature"):
        P.dropout_residual_terms_from_signed_shares(*_verified_args(rd, holders), rd["sig_pk"], {c: s for c, s in csigs.items() if c != 4})
    with pytest.raises(ValueError, match=r"client 3\b.*does not verify"):
        P.dropout_residual_terms_from_signed_shares(*_verified_args(rd, holders), rd["sig_pk"], {**csigs, 3: rd["sigs"][3, 0]})


def test_the_view_round_names_the_client_that_was_shown_something_else(R, signed_round):
    rd, SS, G = signed_round, R.secret_sharing, R.signatures
    shown = {d: rd["sigs"][d] for d in range(N)}
    view = SS.view_message(ROUND_NO, shown)
    assert view == S.view_message(ROUND_NO, shown)
    # client 4 was shown the other commitments of dealer 1, validly signed by dealer 1: its view holds another signature
    assert G.verify(rd["sig_pk"][1:2], [SS.commitment_message(ROUND_NO, 1, 1, rd["other"])], rd["other_sig"].reshape(1, 64)).tolist() == [0]
    shown4 = dict(shown); shown4[1] = np.stack([rd["sigs"][1, 0], rd["other_sig"]])
    views = [SS.view_message(ROUND_NO, shown4) if c == 4 else view for c in range(N)]
    view_sigs = G.sign(rd["sig_sk"], views)
    assert view_sigs.tobytes() == S.sign_batch(rd["sig_sk"], views).tobytes()
    assert SS.verify_views(rd["sig_pk"], view, view_sigs).tolist() == [0, 0, 0, 0, 1, 0]
    assert SS.verify_views(rd["sig_pk"], views[4], view_sigs).tolist() == [1, 1, 1, 1, 0, 1]
