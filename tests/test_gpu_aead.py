"""GPU checks of the sealed shares (rofl_aead_seal / rofl_aead_open: k_aead_derive, k_aead_seal, k_aead_open), byte for byte against the
Python model tests/aead_model.py -- no tolerance anywhere: block positions around the 64-thread block, the whole payload x AD length grid at
misaligned starts in one call (lanes of one wave run different block counts and every tail case), the Poly1305 reduction boundary through
the kernels' own device function, every verdict class in one wave, shared keys and key_idx, the key derivation, the shapes that must not
touch the device, and one six-client round whose share bundles travel sealed."""
import numpy as np
import pytest

import aead_model as A
import dh_model as D
import test_aead_host as H

pytestmark = pytest.mark.gpu
FP = (32, 7)
N, THRESHOLD, ROUND_NO = 6, 4, 7


@pytest.fixture(scope="module")
def R():
    import rofl_project_code_amd as R
    from rofl_project_code_amd import build
    build.build()
    R.set_device(0)
    R.api.set_fp(*FP)
    return R


def _rows(rng, n, w):
    return np.frombuffer(rng.bytes(n * w), np.uint8).reshape(n, w).copy()


@pytest.fixture(scope="module")
def batch257():
    """257 records of random lengths 0 .. 299 (ADs 0 .. 40) under keys and nonces of their own, sealed by the model once and never changed"""
    rng = np.random.default_rng(20261210)
    n = 257
    keys, nonces = _rows(rng, n, 32), _rows(rng, n, 12)
    pts, ads = [rng.bytes(int(x)) for x in rng.integers(0, 300, n)], [rng.bytes(int(x)) for x in rng.integers(0, 41, n)]
    return keys, nonces, ads, pts, A.seal_batch(keys, nonces, ads, pts)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_block_positions(R, batch257, n):
    """the kernels' block is 64 threads: one thread, one short of a block, a block, one more, several blocks and a ragged one"""
    keys, nonces, ads, pts, want = (x[:n] for x in batch257)
    got = R.aead.seal(keys, nonces, ads, pts)
    assert got == want
    back, v = R.aead.open(keys, nonces, ads, got)
    assert back == pts and v.tolist() == [0] * n
    # flips in the LAST record and in record n / 2: exactly those two verdicts, zero plaintexts, the others untouched
    hit = sorted({n - 1, n // 2})
    bad = list(got)
    for k, i in enumerate(hit):
        r = bytearray(bad[i]); r[(len(r) - 1) if k else 0] ^= 0x01      # the tag's last byte / the record's first byte
        bad[i] = bytes(r)
    back, v = R.aead.open(keys, nonces, ads, bad)
    assert np.flatnonzero(v).tolist() == hit and (v[hit] == 1).all()
    assert back == [bytes(len(p)) if i in hit else p for i, p in enumerate(pts)]


def test_length_grid_at_misaligned_starts_equals_host_route_and_model(R):
    keys, nonces, ads, pts, want = H.sealed_grid()
    L = R.lib()
    got = H.lib_seal(L, keys, nonces, ads, pts, name="rofl_aead_seal")
    assert got == want and got == H.lib_seal(L, keys, nonces, ads, pts)
    back, v, _ = H.lib_open(L, keys, nonces, ads, got, name="rofl_aead_open")
    hb, hv, _ = H.lib_open(L, keys, nonces, ads, got)
    assert back == pts and back == hb and not v.any() and not hv.any()


def test_poly1305_boundary_family_in_one_launch(R):
    cases = A.poly_boundary_cases()
    want = [A.poly1305(k, m) for k, m, _ in cases]
    assert all(t is None or t == w for (_, _, t), w in zip(cases, want))
    L = R.lib()
    assert H.lib_poly(L, cases, name="rofl_dbg_poly1305") == want
    assert H.lib_poly(L, cases) == want


def test_every_verdict_class_in_one_wave(R):
    K, Nn, ads, recs, want_pt, want_v = A.verdict_cases(np.random.default_rng(20261203))
    assert len(recs) <= 64 and set(want_v.tolist()) == {0, 1, 2}
    got, v, raw = H.lib_open(R.lib(), K, Nn, ads, recs, name="rofl_aead_open", fill=0x5c)
    assert v.tolist() == want_v.tolist() and got == want_pt
    off = A.pack(recs)[1]
    for i, r in enumerate(recs):      # the 16 bytes behind a plaintext, and all of a record shorter than its tag, are not written
        o, n = int(off[i]), len(r)
        assert (raw[o + max(n - 16, 0):o + n] == 0x5c).all(), i
    back, wv = R.aead.open(K, Nn, ads, recs)
    assert back == want_pt and wv.tolist() == want_v.tolist()


def test_one_key_for_65_records_and_65_keys_reversed(R):
    rng = np.random.default_rng(20261211)
    n = 65
    nonces = _rows(rng, n, 12)
    ads, pts = [rng.bytes(int(x)) for x in rng.integers(0, 33, n)], [rng.bytes(int(x)) for x in rng.integers(0, 130, n)]
    one = _rows(rng, 1, 32)
    got = R.aead.seal(one, nonces, ads, pts, key_idx=[0] * n)
    assert got == A.seal_batch(one, nonces, ads, pts, key_idx=[0] * n)
    back, v = R.aead.open(one, nonces, ads, got, key_idx=[0] * n)
    assert back == pts and not v.any()
    keys, rev = _rows(rng, n, 32), list(range(n))[::-1]
    got = R.aead.seal(keys, nonces, ads, pts, key_idx=rev)
    assert got == A.seal_batch(keys, nonces, ads, pts, key_idx=rev) and got == A.seal_batch(keys[::-1], nonces, ads, pts)
    back, v = R.aead.open(keys, nonces, ads, got, key_idx=rev)
    assert back == pts and not v.any()
    assert (R.aead.open(keys, nonces, ads, got)[1] == np.array([0 if i == n // 2 else 1 for i in range(n)])).all()      # only the middle record keeps its key


def test_key_derivation_on_and_off(R):
    rng = np.random.default_rng(20261212)
    n, rnd = 70, 2 ** 64 - 3
    keys, nonces = _rows(rng, 5, 32), _rows(rng, n, 12)
    idx = [int(x) for x in rng.integers(0, 5, n)]
    rows, adr = _rows(rng, n, 64), _rows(rng, n, 32)                      # the round's shape, the 2-D form
    got = R.aead.seal(keys, nonces, adr, rows, key_idx=idx, derive_round=rnd)
    want = A.seal_batch(keys, nonces, [bytes(a) for a in adr], [bytes(r) for r in rows], key_idx=idx, derive_round=rnd)
    assert got.shape == (n, 80) and [bytes(r) for r in got] == want
    assert want == A.seal_batch([A.derive_key(k, rnd) for k in keys], nonces, [bytes(a) for a in adr], [bytes(r) for r in rows], key_idx=idx)
    plain = R.aead.seal(keys, nonces, adr, rows, key_idx=idx)
    assert [bytes(r) for r in plain] == A.seal_batch(keys, nonces, [bytes(a) for a in adr], [bytes(r) for r in rows], key_idx=idx) and (plain != got).any()
    out, v = R.aead.open(keys, nonces, adr, got, key_idx=idx, derive_round=rnd)
    assert (out == rows).all() and not v.any()
    for other in (rnd - 1, 0, None):
        out, v = R.aead.open(keys, nonces, adr, got, key_idx=idx, derive_round=other)
        assert (v == 1).all() and not out.any()
    # a derived call with one key per record (key_idx None) and several blocks of keys
    keys = _rows(rng, n, 32)
    got = R.aead.seal(keys, nonces, adr, rows, derive_round=1)
    assert [bytes(r) for r in got] == A.seal_batch(keys, nonces, [bytes(a) for a in adr], [bytes(r) for r in rows], derive_round=1)


def test_shapes_that_compute_nothing(R):
    rng = np.random.default_rng(20261213)
    assert R.aead.seal(np.zeros((0, 32), np.uint8), np.zeros((0, 12), np.uint8), [], []) == []
    p, v = R.aead.open(np.zeros((0, 32), np.uint8), np.zeros((0, 12), np.uint8), [], [])
    assert p == [] and v.shape == (0,)
    # n > 0 with a total payload of 0: 16-byte records, each the tag over its AD alone; and with no AD either
    n = 3
    keys, nonces = _rows(rng, n, 32), _rows(rng, n, 12)
    for ads in ([b"a", b"", rng.bytes(17)], [b""] * n):
        got = R.aead.seal(keys, nonces, ads, [b""] * n)
        assert got == A.seal_batch(keys, nonces, ads, [b""] * n) and all(len(r) == 16 for r in got)
        back, v = R.aead.open(keys, nonces, ads, got)
        assert back == [b""] * n and not v.any()
    # records that are all shorter than a tag, the empty one among them: nothing to write, every verdict 2
    back, v = R.aead.open(keys, nonces, [b""] * n, [b"", b"x" * 15, b""])
    assert back == [b""] * n and v.tolist() == [2] * n
    back, v = R.aead.open(keys, nonces, [b""] * n, [b""] * n)
    assert back == [b""] * n and v.tolist() == [2] * n


# ---------------------------------------------------------------- one round whose share bundles travel sealed
def test_a_round_with_sealed_shares(R):
    """The six-client, threshold-4 round of test_gpu_feldman.py: every dealer seals its bundles for all peers in one seal_shares call, every
    client opens what it was sent in one open_shares call; the opened shares are the dealt ones and pass verify_shares clean.  A record
    tampered on the way is named at exactly its (recipient, sender); one relayed to the wrong client and one of the previous round do not open."""
    K, S = R.key_agreement, R.secret_sharing
    rng = np.random.default_rng(20261214)
    ids = list(range(N))
    sk, b, cs = D.rand_keys(rng, N), rng.integers(0, 256, size=(N, 32), dtype=np.uint8), rng.integers(0, 256, size=(2 * N, 32), dtype=np.uint8)
    key_sh, self_sh = S.share(sk, cs[:N], THRESHOLD, N), S.share(b, cs[N:], THRESHOLD, N)      # [dealer, holder, 32]
    com = S.commit(np.concatenate([sk, b]), cs, THRESHOLD)                                     # [key of 0 .. 5 | self of 0 .. 5]
    ch_sk = D.rand_keys(rng, N)                                                                # the CHANNEL keys: a third pair per client
    ch_pk = K.public_keys(ch_sk)
    sent = np.stack([S.seal_shares(ch_sk[d:d + 1], [d], ids, ch_pk, ROUND_NO, key_sh[d:d + 1], self_sh[d:d + 1])[0] for d in range(N)])      # [dealer, recipient, 80]
    assert sent.shape == (N, N, 80) and all(not sent[d, d].any() for d in range(N))
    # the bytes are the model's, from the model's shared secrets
    shared = [[D.shared(ch_sk[a], ch_pk[c])[0] for c in range(N)] for a in range(N)]
    assert (sent == A.seal_shares(shared, ids, ids, ROUND_NO, key_sh, self_sh)).all()
    # a process that hosts every dealer gets the same records in one call
    assert (S.seal_shares(ch_sk, ids, ids, ch_pk, ROUND_NO, key_sh, self_sh) == sent).all()
    prev = S.seal_shares(ch_sk[5:6], [5], ids, ch_pk, ROUND_NO - 1, key_sh[5:6], self_sh[5:6])[0]      # dealer 5's bundles of the round before
    for c in range(N):
        inbox = sent[:, c][None].copy()                                                        # [1, sender, 80]
        if c == 3:
            inbox[0, 5, 33] ^= 0x04                                                            # tampered on the way from dealer 5 to client 3
        if c == 1:
            inbox[0, 4] = sent[4, 0]                                                           # what dealer 4 sealed for client 0, relayed to client 1
        if c == 2:
            inbox[0, 5] = prev[2]                                                              # dealer 5's bundle for client 2 of the previous round
        ks, ss, v = S.open_shares(ch_sk[c:c + 1], [c], ids, ch_pk, ROUND_NO, inbox)
        bad = {3: 5, 1: 4, 2: 5}.get(c)
        assert v.shape == (1, N) and np.flatnonzero(v[0]).tolist() == ([bad] if bad is not None else []) and (bad is None or v[0, bad] == 1), c
        for d in range(N):
            if d == c or d == bad:
                assert not ks[0, d].any() and not ss[0, d].any(), (c, d)
            else:
                assert (ks[0, d] == key_sh[d, c]).all() and (ss[0, d] == self_sh[d, c]).all(), (c, d)
        # what was opened passes the Feldman check; the slots of the skipped pair and of a bad record are filled from the dealing itself
        got = np.concatenate([ks[0], ss[0]])[:, None, :].copy()
        for d in {c, bad} - {None}:
            got[d, 0], got[N + d, 0] = key_sh[d, c], self_sh[d, c]
        assert not S.verify_shares(com, [c + 1], got).any(), c
