"""Key agreement on the GPU (rofl_dh_public_keys / rofl_dh_shared: k_dh_public, k_dh_decode, k_dh_shared) against the Python model of the
definition in include/rofl_zk.h (tests/dh_model.py: pyref's Ristretto codec, the oracle's one-term MSM as the product, hashlib's SHAKE256):
public keys over the extreme scalar families, shared secrets for all-pairs and listed pairs, symmetry, refused peer keys, and one
round end to end -- peers from keys, masks that cancel, the residual terms after a rejection from the revealed key."""
import itertools

import numpy as np
import pytest

import blind_model as B
import dh_model as M
import orc

pytestmark = pytest.mark.gpu
L_ORDER = M.L
P_FIELD = 2 ** 255 - 19


@pytest.fixture(scope="module")
def R():
    import rofl_project_code_amd as R
    from rofl_project_code_amd import build
    build.build()
    R.set_device(0)
    return R


@pytest.fixture(scope="module")
def K(R):
    return R.key_agreement


@pytest.fixture(scope="module")
def clients():
    """seven clients: secret keys (any 32 bytes, most of them above l) and the model's public keys, computed once"""
    rng = np.random.default_rng(77)
    sk = M.rand_keys(rng, 7)
    pk = np.frombuffer(b"".join(M.public_key(s) for s in sk), np.uint8).reshape(7, 32).copy()
    return sk, pk


@pytest.mark.parametrize("n", [1, 65, 257])
def test_public_keys(K, n):
    # 65 / 257: one key past one and past four 64-thread blocks
    for family, sk in orc.extreme_scalar_cases(np.random.default_rng(n), n).items():
        if family == "small":
            sk = sk[1:]                # (the zero key is refused: test_zero_key_is_refused)
        if len(sk) == 0:
            continue
        got = K.public_keys(sk)
        assert got.shape == (len(sk), 32) and got.dtype == np.uint8
        assert (got == orc.commit_vec(sk, None)).all(), (family, n)


def test_keys_above_l_are_reduced(K, clients):
    sk, pk = clients
    assert any(int.from_bytes(s.tobytes(), "little") >= L_ORDER for s in sk)
    assert (K.public_keys(sk) == pk).all()
    k = M.sk_int(sk[0])
    both = K.public_keys([k.to_bytes(32, "little"), (k + L_ORDER).to_bytes(32, "little")])
    assert (both[0] == both[1]).all() and (both[0] == pk[0]).all()


def test_zero_key_is_refused(R, K, clients):
    sk, pk = clients
    for zero in (bytes(32), L_ORDER.to_bytes(32, "little")):
        with pytest.raises(R.RoflError) as e:
            K.public_keys([sk[0].tobytes(), zero])
        assert e.value.code == 11
        with pytest.raises(R.RoflError) as e:
            K.shared_secrets([zero], pk[:2])
        assert e.value.code == 11


def test_shared_secrets_against_the_model(K, clients):
    sk, pk = clients
    # 1 x 1 and 3 x 5, all pairs (own-major)
    for n_own, n_peer in ((1, 1), (3, 5)):
        got, st = K.shared_secrets(sk[:n_own], pk[7 - n_peer:])
        want, wst = M.shared_batch(sk[:n_own], pk[7 - n_peer:])
        assert got.shape == (n_own * n_peer, 32) and st.shape == (n_own * n_peer,)
        assert (got == want).all() and (st == wst).all() and not st.any(), (n_own, n_peer)
    # an explicit list of 257 pairs (four blocks and one pair): owns and peers repeat and are out of order; 63, 64, 65 straddle a block
    rng = np.random.default_rng(3)
    pairs = [(int(a), int(b)) for a, b in zip(rng.integers(0, 5, 257), rng.integers(0, 7, 257))]
    pairs[63], pairs[64], pairs[65] = (4, 6), (0, 0), (4, 0)
    pairs[0], pairs[256] = (3, 3), (1, 5)
    got, st, own = K.shared_secrets(sk[:5], pk, pairs, with_public=True)
    want, wst = M.shared_batch(sk[:5], pk, pairs)
    assert (got == want).all() and (st == wst).all() and not st.any()
    assert (own == K.public_keys(sk[:5])).all() and (own == pk[:5]).all()
    assert len({got[i].tobytes() for i in range(257)}) == len({(min(a, b), max(a, b)) for a, b in pairs})      # one secret per unordered pair


def test_symmetry_on_the_device(K, clients):
    sk, pk = clients
    got, st = K.shared_secrets(sk[:6], pk[:6])
    assert not st.any()
    got = got.reshape(6, 6, 32)
    for a, b in itertools.combinations(range(6), 2):
        assert (got[a, b] == got[b, a]).all() and got[a, b].any(), (a, b)
    assert len({got[a, b].tobytes() for a, b in itertools.combinations(range(6), 2)}) == 15


def test_refused_peer_keys(K, clients):
    sk, pk = clients
    neg_s = (P_FIELD - int.from_bytes(pk[1].tobytes(), "little")).to_bytes(32, "little")
    bad = [(b"\xff" * 32, 1), (bytes(32), 2), (neg_s, 1), ((P_FIELD + 1).to_bytes(32, "little"), 1)]
    peers = np.concatenate([pk, np.frombuffer(b"".join(b for b, _ in bad), np.uint8).reshape(-1, 32)])      # peers 7 .. 10 are refused
    clean = peers.copy(); clean[7:] = pk[:4]
    # 130 pairs: bad keys at the first pair, the last pair of the first block and the last pair of the call
    pairs = [(i % 3, i % 7) for i in range(130)]
    where = {0: 7, 63: 8, 129: 9, 70: 10}
    for i, p in where.items():
        pairs[i] = (pairs[i][0], p)
    got, st = K.shared_secrets(sk[:3], peers, pairs)
    ref, rst = K.shared_secrets(sk[:3], clean, pairs)
    assert not rst.any()
    for i in range(130):
        if i in where:
            assert st[i] == bad[where[i] - 7][1] and not got[i].any(), i
        else:
            assert st[i] == 0 and (got[i] == ref[i]).all(), i
    want, wst = M.shared_batch(sk[:3], peers, pairs)
    assert (got == want).all() and (st == wst).all()
    # all pairs against a refused peer: its column is refused, nothing else
    got, st = K.shared_secrets(sk[:2], peers[6:9])
    assert st.tolist() == [0, 1, 2, 0, 1, 2] and not got[[1, 2, 4, 5]].any() and got[0].any() and got[3].any()


def test_round_end_to_end(R, K, clients):
    P = R.pedersen_ops
    sk, pk = clients[0][:6], clients[1][:6]
    d, round_no = 33, 7
    # six hosted clients build their peers from keys: ONE call
    peers = P.pairwise_peers_from_keys(clients=[(i, sk[i]) for i in range(6)], public_keys=pk, round_no=round_no)
    seeds = {(i, j): B.round_seed(M.shared(sk[i], pk[j], pk[i])[0], round_no) for i, j in itertools.combinations(range(6), 2)}
    for i in range(6):
        assert peers[i] == [(j, seeds[(min(i, j), max(i, j))]) for j in range(6) if j != i], i
    assert P.pairwise_peers_from_keys(4, sk[4], pk, round_no) == peers[4]
    vecs = P.pairwise_blinding_vecs(list(zip(range(6), peers)), d)
    ints = [B.to_ints(v) for v in vecs]
    assert all(sum(col) % L_ORDER == 0 for col in zip(*ints)) and any(ints[0])
    # client 2 is rejected and its key revealed
    accepted = [0, 1, 3, 4, 5]
    terms = P.pairwise_residual_terms_from_keys(accepted, {2: sk[2]}, pk, round_no)
    assert terms == P.pairwise_residual_terms(accepted, [2], seeds)
    opening = P.blinding_vecs([terms], d)[0]
    assert (opening == B.to_arr([sum(col) for col in zip(*[ints[i] for i in accepted])])).all()
    # a key that is not client 2's is caught before any secret is derived
    with pytest.raises(ValueError, match=r"client 2\b"):
        P.pairwise_residual_terms_from_keys(accepted, {2: sk[3]}, pk, round_no)
