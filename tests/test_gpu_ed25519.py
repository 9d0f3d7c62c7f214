"""rofl_ed25519_public_keys / _sign / _verify on the device against the Python model of RFC 8032 (tests/ed25519_model.py), byte for byte.

Every kernel runs one thread per key or per signature in blocks of 64, so n in {1, 63, 64, 65, 257} is one lane, a wave short of one, a full
one, a crossing, and several blocks with a ragged tail.  The block-end lengths of ed25519_model.LENS go into ONE call at packed starts, so the
lanes of a wave run different numbers of SHA-512 blocks; good signatures, every class of 1 and every class of 2 share a wave; the torsion corpus
(ed25519_model.torsion_cases: keys and R with a small-order part) in one call, through refs, alone and past a block end; one key signs
65 messages and 65 keys sign one; the host twin gives the device's bytes.  Then the signed round of test_gpu_signatures.py under
scheme=ed25519, and the same helper under the default scheme with the bytes it always gave."""
import numpy as np
import pytest

import ed25519_model as E
import sig_model as S
import test_ed25519_host as H
import test_gpu_signatures as T
from test_ed25519_host import padding_batch, torsion  # noqa: F401
from test_gpu_signatures import R, signed_round  # noqa: F401

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def batch257():
    """257 seeds, 257 messages of 0 .. 299 bytes, the model's public keys and signatures: computed once, never changed"""
    rng = np.random.default_rng(20261128)
    seeds = np.frombuffer(rng.bytes(257 * 32), np.uint8).reshape(257, 32)
    msgs = [rng.bytes(int(n)) for n in rng.integers(0, 300, size=257)]
    pks, sigs = H.rows(E.public_key(s.tobytes()) for s in seeds), H.rows((E.sign(s.tobytes(), m) for s, m in zip(seeds, msgs)), 64)
    for a in (pks, sigs):
        a.setflags(write=False)
    return seeds, pks, msgs, sigs


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_block_sizes(R, batch257, n):  # noqa: F811
    G = R.ed25519
    seeds, pks, msgs, sigs = batch257
    got, pk = G.sign(seeds[:n], msgs[:n], with_public=True)
    assert got.shape == (n, 64) and got.tobytes() == sigs[:n].tobytes()
    assert pk.tobytes() == pks[:n].tobytes() == G.public_keys(seeds[:n]).tobytes()
    assert not G.verify(pks[:n], msgs[:n], got).any()
    bad = got.copy(); bad[n - 1, 40] ^= 1; bad[n // 2, 1] ^= 0x10
    want = np.zeros(n, np.uint8); want[n - 1] = 1; want[n // 2] = 1
    assert (G.verify(pks[:n], msgs[:n], bad) == want).all()


def test_every_padding_case_in_one_call_and_the_host_twin_agrees(R, padding_batch):  # noqa: F811
    G, lib = R.ed25519, R.api.lib()
    seeds, msgs, pks, sigs = padding_batch
    got, pk = G.sign(H.rows(seeds), msgs, with_public=True)
    assert got.tobytes() == sigs.tobytes() and pk.tobytes() == pks.tobytes()
    assert not G.verify(pks, msgs, got).any()
    changed = [(m[:-1] + bytes([m[-1] ^ 1])) if m else b"\0" for m in msgs]
    assert (G.verify(pks, changed, got) == 1).all()
    hs, hp = H.host_sign(lib, seeds, msgs)
    assert hs.tobytes() == got.tobytes() and hp.tobytes() == pk.tobytes()
    bad = got.copy(); bad[5, 33] ^= 2
    assert (H.host_verify(lib, pks, msgs, bad) == G.verify(pks, msgs, bad)).all()
    e = G.sign(H.rows(seeds[:3]), [b"", b"", b""])      # no message bytes at all
    assert e.tobytes() == b"".join(E.sign(s, b"") for s in seeds[:3])


def test_every_verdict_class_in_one_wave(R, padding_batch):  # noqa: F811
    seeds, msgs, pks, sigs = padding_batch
    cases = E.verdict_cases(pks[5].tobytes(), msgs[5], sigs[5].tobytes())
    keys, ms, sg, want = [pks[7]], [msgs[7]], [sigs[7]], [0]
    for k, m, s, v in cases:      # every case between two good signatures of another key
        keys += [k, pks[7]]; ms += [m, msgs[7]]; sg += [s, sigs[7]]; want += [v, 0]
    assert len(want) <= 64 and want.count(1) == 4 and want.count(2) == 16
    got = R.ed25519.verify(H.rows(keys), ms, H.rows(sg, 64))
    assert got.tolist() == want == H.host_verify(R.api.lib(), keys, ms, sg).tolist()
    # the refused key shared through refs: it condemns its signatures, not the call
    refs = [(i, i) for i in range(len(want))] + [(19, 0), (0, 0)]
    assert want[19] == 2 and R.ed25519.verify(H.rows(keys), ms, H.rows(sg + [sg[0], sg[0]], 64), refs).tolist() == want + [2, 0]


def test_the_torsion_corpus_in_one_call(R, padding_batch, torsion):  # noqa: F811
    seeds, msgs, pks, sigs = padding_batch
    keys, ms, sg = H.interleaved(torsion, (pks[7].tobytes(), msgs[7], sigs[7].tobytes()))      # 163 signatures: every wave of three blocks mixes 0, 1 and 2
    want = [0] + [v for c in torsion for v in (c[3], 0)]
    assert want[1::2] == [c[3] for c in torsion] and 128 < len(want) <= 200
    got = R.ed25519.verify(H.rows(keys), ms, H.rows(sg, 64)).tolist()
    assert got == want, [c[4] for c, g in zip(torsion, got[1::2]) if c[3] != g]
    assert got == H.host_verify(R.api.lib(), keys, ms, sg).tolist()


def test_mixed_order_keys_shared_through_refs(R, torsion):  # noqa: F811
    a = [c for c in torsion if c[4][0] == "a"]
    keys = [a[4 * i][0] for i in range(7)]      # each key once: decoded once, its torsion part intact, status 0 -- no verdict below is 2
    refs = [(j // 4, j) for j in range(28)]
    assert all(keys[k] == a[j][0] for k, j in refs) and {c[3] for c in a} == {0, 1}
    assert R.ed25519.verify(H.rows(keys), [c[1] for c in a], H.rows([c[2] for c in a], 64), refs).tolist() == [c[3] for c in a]
    # the same signatures backwards, so that neighbouring lanes that share a key change places
    back = refs[::-1]
    assert R.ed25519.verify(H.rows(keys), [c[1] for c in a], H.rows([a[j][2] for _, j in back], 64), back).tolist() == [a[j][3] for _, j in back]


def test_a_torsion_verdict_does_not_depend_on_its_lane(R, padding_batch, torsion):  # noqa: F811
    seeds, msgs, pks, sigs = padding_batch
    a = [c for c in torsion if c[4][0] == "a"]
    assert a[0][4] == "a1" and a[0][3] == 0 and a[1][3] == 1      # the order-8 key at k = 0 mod 8, accepted, and at 4 mod 8, not
    for c in a[:2]:
        assert R.ed25519.verify(H.rows([c[0]]), [c[1]], H.rows([c[2]], 64)).tolist() == [c[3]]      # n = 1
    keys, ms, sg = [pks[7].tobytes()] * 64, [msgs[7]] * 64, [sigs[7].tobytes()] * 64      # a full block of good ones, then family (a) from lane 64 on
    got = R.ed25519.verify(H.rows(keys + [c[0] for c in a]), ms + [c[1] for c in a], H.rows(sg + [c[2] for c in a], 64)).tolist()
    assert got == [0] * 64 + [c[3] for c in a]


def test_one_key_many_messages_and_many_keys_one_message(R, batch257):  # noqa: F811
    G = R.ed25519
    seeds, pks, msgs, sigs = batch257
    refs = [(0, b) for b in range(65)]
    got = G.sign(seeds[9:10], msgs[:65], refs)
    assert got.tobytes() == b"".join(E.sign(seeds[9].tobytes(), m) for m in msgs[:65]) and got[9].tobytes() == sigs[9].tobytes()
    bad = got.copy(); bad[64, 0] ^= 4
    assert np.flatnonzero(G.verify(pks[9:10], msgs[:65], bad, refs)).tolist() == [64]
    SS, root = R.secret_sharing, np.frombuffer(msgs[200][:32].ljust(32, b"r"), np.uint8)      # the view shape: 65 keys on ONE 60-byte root message
    got = SS.sign_view_root(seeds[:65], 7, 65, np.tile(root, (65, 1)), scheme=G)
    assert got.tobytes() == b"".join(E.sign(s.tobytes(), SS.view_root_message(7, 65, root)) for s in seeds[:65])
    bad = got.copy(); bad[63, 63] ^= 0x08; bad[64] = got[0]
    assert np.flatnonzero(SS.verify_view_roots(pks[:65], 7, 65, root, bad, scheme=G)).tolist() == [63, 64]


def test_the_cap_on_the_bytes_hashed(R, batch257):  # noqa: F811
    seeds, pks, msgs, sigs = batch257
    big, refs = bytes(2**20 + 1), [(0, 0)] * 1024      # 2^30 + 1024 bytes hashed from one message of 1 MiB + 1
    for call in (lambda: R.ed25519.sign(seeds[:1], [big], refs), lambda: R.ed25519.verify(pks[:1], [big], np.zeros((1024, 64), np.uint8), refs)):
        with pytest.raises(R.RoflError) as e:
            call()
        assert e.value.code == 11 and "2^30" in str(e.value)
    assert not R.ed25519.verify(pks[:1], [big[:2**20]], R.ed25519.sign(seeds[:1], [big[:2**20]], refs[:1023]), refs[:1023]).any()      # 2^30 - 2^20: allowed


def test_a_round_on_standard_signatures(R, signed_round):  # noqa: F811
    rd, SS, P, G, N, RN = signed_round, R.secret_sharing, R.pedersen_ops, R.ed25519, T.N, T.ROUND_NO
    seeds = rd["sig_sk"]      # a seed per client; any 32 bytes are one
    pk = G.public_keys(seeds)
    sigs = SS.sign_commitments(seeds, RN, range(N), rd["key_com"], rd["self_com"], scheme=G)
    for d in range(N):
        for kind, com in ((0, rd["key_com"]), (1, rd["self_com"])):
            assert sigs[d, kind].tobytes() == E.sign(seeds[d].tobytes(), S.commitment_message(RN, d, kind, com[d]))
    assert not SS.verify_commitment_signatures(pk, RN, range(N), rd["key_com"], rd["self_com"], sigs, scheme=G).any()
    bad = sigs.copy(); bad[3, 1, 7] ^= 0x20      # dealer 3's signature on its self commitments, corrupted on the way: named
    assert SS.verify_commitment_signatures(pk, RN, range(N), rd["key_com"], rd["self_com"], bad, scheme=G).tolist() == [[0, 0]] * 3 + [[0, 1]] + [[0, 0]] * 2
    args = T._verified_args(rd, T.SURVIVORS)
    csigs = {T.GONE: sigs[T.GONE, 0], **{i: sigs[i, 1] for i in T.SURVIVORS}}
    assert P.dropout_residual_terms_from_signed_shares(*args, pk, csigs, scheme=G) == P.dropout_residual_terms_from_verified_shares(*args)
    with pytest.raises(ValueError, match=r"client 3\b.*self-mask commitments does not verify"):
        P.dropout_residual_terms_from_signed_shares(*args, pk, {**csigs, 3: bad[3, 1]}, scheme=G)
    # the default scheme: the bytes the helper always gave
    assert SS.sign_commitments(seeds, RN, range(N), rd["key_com"], rd["self_com"]).tobytes() == rd["sigs"].tobytes()
    assert rd["sigs"][4, 1].tobytes() == S.sign(seeds[4], S.commitment_message(RN, 4, 1, rd["self_com"][4]))
