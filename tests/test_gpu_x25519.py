"""rofl_x25519_public_keys / rofl_x25519_shared on the device against the Python model of RFC 7748 (tests/x25519_model.py), byte for byte.

k_x25519 runs one ladder per lane (route 1, 64 a block) or per lane quad (route 2, 16 a block), so n in {1, 15, 16, 17, 63, 64, 65, 257} is
one item, a wave short of one, a full wave, a crossing and a ragged tail for both layouts.  The edge corpus goes into ONE call per route, so
zero results, non-canonical u and ordinary pairs share a wave, and so does every non-canonical u, p .. 2^255 - 1 under both values of bit 255;
route 0 is run on both sides of its rule; then a sealed round under
agreement=x25519."""
import numpy as np
import pytest

import x25519_model as X
from test_ed25519_host import call, rows
from test_gpu_signatures import R  # noqa: F401
from test_x25519_host import host, noncanonical_want

pytestmark = pytest.mark.gpu


def device(R, route, keys, us, pairs, n_pairs, with_public=True):  # noqa: F811
    """rofl_dbg_x25519_shared -> (out rows, status list, own public keys)"""
    out, st, pk = np.full((n_pairs, 32), 0xaa, np.uint8), np.full(n_pairs, 0xaa, np.uint8), np.full((len(keys), 32), 0xaa, np.uint8)
    p = None if pairs is None else np.asarray(pairs, np.uint32).reshape(-1, 2).copy()
    assert call(R.api.lib(), "rofl_dbg_x25519_shared", route, len(keys), rows(keys), pk if with_public else None, len(us), rows(us), n_pairs, p, out, st) == 0
    return out, st.tolist(), pk


@pytest.fixture(scope="module")
def batch257():
    """257 seeded (key, u) pairs with the model's secrets and public keys: computed once, never changed"""
    rng = np.random.default_rng(20261203)
    keys, us = [rng.bytes(32) for _ in range(257)], [rng.bytes(32) for _ in range(257)]
    want, pks = rows(X.x25519(k, u) for k, u in zip(keys, us)), rows(X.public_key(k) for k in keys)
    for a in (want, pks):
        a.setflags(write=False)
    return keys, us, want, pks


@pytest.mark.parametrize("n", [1, 15, 16, 17, 63, 64, 65, 257])
@pytest.mark.parametrize("route", [1, 2])
def test_block_sizes(R, batch257, route, n):  # noqa: F811
    keys, us, want, pks = batch257
    out, st, pk = device(R, route, keys[:n], us[:n], [(i, i) for i in range(n)], n)
    assert out.tobytes() == want[:n].tobytes() and st == [0] * n
    assert pk.tobytes() == pks[:n].tobytes() == R.x25519.public_keys(rows(keys[:n])).tobytes()


@pytest.mark.parametrize("route", [1, 2])
def test_the_edge_corpus_in_one_call_and_the_host_twin_agrees(R, route):  # noqa: F811
    want = [X.shared(k, u) for k in X.CORPUS_K for u in X.CORPUS_U]
    out, st, _ = device(R, route, X.CORPUS_K, X.CORPUS_U, None, len(want), with_public=False)
    assert [o.tobytes() for o in out] == [w for w, _ in want] and st == [s for _, s in want] and st.count(2) == 8 * len(X.SMALL_ORDER)
    assert host(R.api.lib(), [k for k in X.CORPUS_K for _ in X.CORPUS_U], X.CORPUS_U * len(X.CORPUS_K)) == ([o.tobytes() for o in out], st)


@pytest.mark.parametrize("route", [1, 2])
def test_every_noncanonical_u_in_one_call_and_the_host_twin_agrees(R, route):  # noqa: F811
    want = noncanonical_want()
    out, st, _ = device(R, route, X.CORPUS_K, X.NONCANONICAL_U, None, len(want), with_public=False)
    assert [o.tobytes() for o in out] == [w for w, _ in want] and st == [s for _, s in want] and st.count(2) == 4 * len(X.CORPUS_K)
    assert host(R.api.lib(), [k for k in X.CORPUS_K for _ in X.NONCANONICAL_U], X.NONCANONICAL_U * len(X.CORPUS_K)) == ([o.tobytes() for o in out], st)


@pytest.mark.parametrize("n", [16384, 16385])
def test_the_library_chooses_on_both_sides_of_its_rule(R, batch257, n):  # noqa: F811
    keys, us, want, pks = batch257
    idx = np.arange(n) % 257
    out, st, pk = device(R, 0, keys, us, np.stack([idx, idx], axis=1), n)
    assert out.tobytes() == want[idx].tobytes() and not any(st) and pk.tobytes() == pks.tobytes()


def test_all_pairs_are_own_major(R, batch257):  # noqa: F811
    keys, us, want, pks = batch257
    got, st, pk = R.x25519.shared_secrets(rows(keys[:5]), rows(us[:7]), with_public=True)
    assert got.tobytes() == b"".join(X.x25519(k, u) for k in keys[:5] for u in us[:7]) and not st.any() and pk.tobytes() == pks[:5].tobytes()
    a, b = R.x25519.shared_secrets(rows(keys[:2]), pks[2:4]), R.x25519.shared_secrets(rows(keys[2:4]), pks[:2])
    assert a[0].reshape(2, 2, 32).transpose(1, 0, 2).tobytes() == b[0].tobytes()      # both sides of a pair hold the same 32 bytes
    P = R.pedersen_ops      # the mask seeds of client 0 of a four-client round, from the raw secrets
    assert P.pairwise_peers_from_keys(0, keys[0], pks[:4], 9, agreement=R.x25519) == [(j, P.pairwise_round_seed(X.x25519(keys[0], pks[j].tobytes()), 9)) for j in (1, 2, 3)]


def test_a_sealed_round_under_x25519(R, batch257):  # noqa: F811
    S, G, K = R.secret_sharing, R.x25519, R.key_agreement
    keys, us, want, pks = batch257
    rng = np.random.default_rng(20261204)
    ids, ch_sk, ch_pk = [0, 1, 2, 3], rows(keys[:4]), pks[:4]
    key_sh, self_sh = rng.integers(0, 256, (4, 4, 32), np.uint8), rng.integers(0, 256, (4, 4, 32), np.uint8)
    hosted = [0, 1, 2]      # three hosted clients seal for, and open from, all four
    sent = S.seal_shares(ch_sk[hosted], hosted, ids, ch_pk, 9, key_sh[hosted], self_sh[hosted], agreement=G)
    full = S.seal_shares(ch_sk, ids, ids, ch_pk, 9, key_sh, self_sh, agreement=G)      # [dealer, recipient]; the hosted dealers' rows are `sent`
    assert (full[hosted] == sent).all()
    inbox = np.ascontiguousarray(full.transpose(1, 0, 2)[hosted])      # [recipient, sender]
    ks, ss, v = S.open_shares(ch_sk[hosted], hosted, ids, ch_pk, 9, inbox, agreement=G)
    assert not v.any()
    for c in hosted:
        for d in ids:
            if c != d:
                assert ks[c, d].tobytes() == key_sh[d, c].tobytes() and ss[c, d].tobytes() == self_sh[d, c].tobytes()
    # the default agreement: the bytes it always gave, and records that do not open under the other agreement
    rpk = K.public_keys(ch_sk)
    plain = S.seal_shares(ch_sk[hosted], hosted, ids, rpk, 9, key_sh[hosted], self_sh[hosted])
    assert (plain == S.seal_shares(ch_sk[hosted], hosted, ids, rpk, 9, key_sh[hosted], self_sh[hosted], agreement=K)).all()
    _, _, v = S.open_shares(ch_sk[hosted], hosted, ids, ch_pk, 9, np.ascontiguousarray(S.seal_shares(ch_sk, ids, ids, rpk, 9, key_sh, self_sh).transpose(1, 0, 2)[hosted]), agreement=G)
    assert (v == (np.array(hosted)[:, None] != np.array(ids)[None, :])).all()
