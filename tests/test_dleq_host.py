"""CPU-only checks of the complaint proofs (rofl_dleq_prove / rofl_dleq_verify): the Python model of the definition (tests/dleq_model.py)
against point arithmetic by hand, the host route rofl_dbg_host_dleq_* against the model and the known-answer vectors of
tests/golden/dleq.json, every verdict class, the decoder's late-reject classes at every decode site, every parameter check of the four C
entry points (they come before the device is touched), the Python wrappers on the host route, judge_complaints and its helpers with the
device calls replaced by the models, and the Rust declarations.  No call here reaches a GPU."""
import ctypes
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import aead_model as A
import dh_model as D
import dleq_model as Q
import feldman_model as F
import ristretto_corpus as RC
import shamir_model as M
import sig_model as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "dleq.json")
sz, vp = ctypes.c_size_t, ctypes.c_void_p
ELL = Q.L
PROVE_ARGS = [sz, vp, vp, sz, vp, sz, vp, vp, vp, vp, vp]
VERIFY_ARGS = [sz, vp, sz, vp, sz, vp, vp, vp, vp, vp, vp]
LATE = ("nonsquare", "nonsquare_v0", "tneg", "y0")      # refused only after the square-root chain has run


def _p(x):
    return None if x is None else x.ctypes.data


def _b32(v):
    return np.frombuffer(int(v).to_bytes(32, "little"), np.uint8)


def _rows(x, w=32):
    return np.ascontiguousarray(np.asarray(x, np.uint8).reshape(-1, w))


def _pairs_arr(pairs):
    return None if pairs is None else np.ascontiguousarray(np.asarray(pairs, np.uint32).reshape(-1, 2))


def _prove(L, name, n_own, sk, pk_out, n_peer, peer, n_pairs, pairs, ctx, reveal, proof, status):
    fn = getattr(L, name)
    fn.argtypes = PROVE_ARGS
    return fn(n_own, _p(sk), _p(pk_out), n_peer, _p(peer), n_pairs, _p(pairs), _p(ctx), _p(reveal), _p(proof), _p(status))


def _verify(L, name, n_own, own, n_peer, peer, n_pairs, pairs, ctx, reveal, proof, shared, verdict):
    fn = getattr(L, name)
    fn.argtypes = VERIFY_ARGS
    return fn(n_own, _p(own), n_peer, _p(peer), n_pairs, _p(pairs), _p(ctx), _p(reveal), _p(proof), _p(shared), _p(verdict))


def lib_prove(L, sks, peers, ctxs, pairs=None, name="rofl_dbg_host_dleq_prove"):
    """-> (reveals, proofs, status, own public keys); the outputs start out as 0xaa"""
    sks, peers, ctxs, p = _rows(sks), _rows(peers), _rows(ctxs), _pairs_arr(pairs)
    n = len(sks) * len(peers) if p is None else len(p)
    reveal, proof, status, pk = np.full((n, 32), 0xaa, np.uint8), np.full((n, 64), 0xaa, np.uint8), np.full(n, 0xaa, np.uint8), np.full((len(sks), 32), 0xaa, np.uint8)
    assert _prove(L, name, len(sks), sks, pk, len(peers), peers, n, p, ctxs, reveal, proof, status) == 0
    return reveal, proof, status, pk


def lib_verify(L, own, peers, ctxs, reveals, proofs, pairs=None, name="rofl_dbg_host_dleq_verify"):
    """-> (verdicts, shared secrets)"""
    own, peers, ctxs, reveals, proofs, p = _rows(own), _rows(peers), _rows(ctxs), _rows(reveals), _rows(proofs, 64), _pairs_arr(pairs)
    n = len(own) * len(peers) if p is None else len(p)
    shared, verdict = np.full((n, 32), 0xaa, np.uint8), np.full(n, 0xaa, np.uint8)
    assert _verify(L, name, len(own), own, len(peers), peers, n, p, ctxs, reveals, proofs, shared, verdict) == 0
    only = np.full(n, 0xaa, np.uint8)      # shared_out32 may be NULL: the same verdicts
    assert _verify(L, name, len(own), own, len(peers), peers, n, p, ctxs, reveals, proofs, None, only) == 0 and (only == verdict).all()
    return verdict, shared


def _last_error(L):
    err = ctypes.create_string_buffer(512)
    L.rofl_last_error(err, sz(512))
    return err


def _pk(sks):
    return np.stack([np.frombuffer(D.public_key(k), np.uint8) for k in _rows(sks)])


def golden_inputs():
    """the dozen (key, peer, ctx) of tests/golden/dleq.json: the edge keys 1, l - 1, s + l and 2^256 - 1, then random ones"""
    rng = np.random.default_rng(20270101)
    s = int.from_bytes(rng.bytes(31), "little")
    keys = [_b32(v) for v in (1, ELL - 1, s + ELL, 2 ** 256 - 1)] + list(D.rand_keys(rng, 8))
    peers = _pk(D.rand_keys(rng, 12))
    peers[1] = np.frombuffer(D.BASE_ENC, np.uint8)
    return np.stack(keys), peers, np.frombuffer(rng.bytes(12 * 32), np.uint8).reshape(12, 32).copy()


def golden_from_model():
    keys, peers, ctxs = golden_inputs()
    out = []
    for k, p, c in zip(keys, peers, ctxs):
        reveal, proof, st = Q.prove(k, p, c)
        v, shared = Q.verify(D.public_key(k), p, c, reveal, proof)
        assert st == 0 and v == 0
        out.append({"key": bytes(k).hex(), "peer": bytes(p).hex(), "ctx": bytes(c).hex(), "reveal": reveal.hex(), "proof": proof.hex(), "shared": shared.hex()})
    return json.dumps({"what": "rofl_dleq_prove / rofl_dleq_verify known answers, made by tests/dleq_model.py", "vectors": out}, indent=1) + "\n"


@pytest.fixture(scope="module")
def proved(hiplib):
    """six keys each proving against ONE peer key under a ctx of its own, through the host route: (sks, pks, peer, ctxs)"""
    rng = np.random.default_rng(20270102)
    sks = D.rand_keys(rng, 6)
    peer = _pk(D.rand_keys(rng, 1))[0]
    ctxs = np.frombuffer(rng.bytes(6 * 32), np.uint8).reshape(6, 32).copy()
    return sks, _pk(sks), peer, ctxs


def test_model_is_the_definition():
    pyref = Q.pyref
    sk, ctx = bytes(range(1, 33)), hashlib.sha3_256(b"a complaint").digest()
    y = 0x1234567
    P = pyref.ristretto_encode(pyref.pt_mul(y, pyref.BASE))
    S_, proof, st = Q.prove(sk, P, ctx, fast=False)
    assert (S_, proof, st) == Q.prove(sk, P, ctx) and st == 0 and len(proof) == 64      # fast=False equals fast=True, once
    x, A_ = D.sk_int(sk), D.public_key(sk, fast=False)
    Pp = pyref.ristretto_decode(P)
    assert S_ == pyref.ristretto_encode(pyref.pt_mul(x, Pp)) == pyref.ristretto_encode(pyref.pt_mul(y, pyref.ristretto_decode(A_)))      # the DH point, from either side
    k = int.from_bytes(hashlib.shake_256(b"rofl-zk/dleq/v1k" + x.to_bytes(32, "little") + P + ctx).digest(64), "little") % ELL
    T1, T2 = pyref.ristretto_encode(pyref.pt_mul(k, pyref.BASE)), pyref.ristretto_encode(pyref.pt_mul(k, Pp))
    c, s = int.from_bytes(proof[:32], "little"), int.from_bytes(proof[32:], "little")
    assert c == int.from_bytes(hashlib.shake_256(b"rofl-zk/dleq/v1c" + A_ + P + S_ + T1 + T2 + ctx).digest(64), "little") % ELL
    assert s == (k + c * x) % ELL and c < ELL and s < ELL
    # the two verification equations on points, by hand: s B == T1 + c A and s P == T2 + c S
    assert pyref.ristretto_encode(pyref.pt_mul(s, pyref.BASE)) == pyref.ristretto_encode(pyref.pt_add(pyref.ristretto_decode(T1), pyref.pt_mul(c, pyref.ristretto_decode(A_))))
    assert pyref.ristretto_encode(pyref.pt_mul(s, Pp)) == pyref.ristretto_encode(pyref.pt_add(pyref.ristretto_decode(T2), pyref.pt_mul(c, pyref.ristretto_decode(S_))))
    v, shared = Q.verify(A_, P, ctx, S_, proof, fast=False)
    assert (v, shared) == Q.verify(A_, P, ctx, S_, proof) and v == 0
    assert shared == D.shared(sk, P)[0] == hashlib.shake_256(b"rofl-zk/dh/v1\0\0\0" + S_ + min(A_, P) + max(A_, P)).digest(32)
    bad = bytearray(proof); bad[40] ^= 1
    assert Q.verify(A_, P, ctx, S_, bytes(bad), fast=False) == Q.verify(A_, P, ctx, S_, bytes(bad)) == (1, bytes(32))
    assert Q.verify(A_, P, ctx, S_, proof[:32] + (s + ELL).to_bytes(32, "little")) == (2, bytes(32))
    assert Q.verify(A_, P, ctx, bytes(32), proof)[0] == 2 and Q.verify(b"\xff" * 32, P, ctx, S_, proof)[0] == 2
    assert Q.prove(sk, bytes(32), ctx) == (bytes(32), bytes(64), 2) and Q.prove(sk, b"\xff" * 32, ctx) == (bytes(32), bytes(64), 1)
    # the layouts
    rec = bytes(range(80))
    assert Q.bundle_message(2 ** 40 + 5, 70000, 3, rec) == b"rofl-zk/sealed/1" + (2 ** 40 + 5).to_bytes(8, "little") + (70000).to_bytes(4, "little") + (3).to_bytes(4, "little") + rec
    assert Q.complaint_context(7, 3, 5) == hashlib.sha3_256(b"rofl-zk/complain" + (7).to_bytes(8, "little") + (3).to_bytes(4, "little") + (5).to_bytes(4, "little")).digest()


def test_golden_vectors_are_the_model_and_the_host_route(hiplib):
    text = open(GOLDEN).read()
    assert text == golden_from_model()                                              # byte for byte
    vec = json.loads(text)["vectors"]
    assert len(vec) == 12
    col = lambda name, w: np.frombuffer(bytes.fromhex("".join(v[name] for v in vec)), np.uint8).reshape(-1, w).copy()      # noqa: E731
    keys, peers, ctxs = col("key", 32), col("peer", 32), col("ctx", 32)
    pairs = [(i, i) for i in range(12)]
    reveal, proof, status, pk = lib_prove(hiplib, keys, peers, ctxs, pairs)
    assert not status.any() and reveal.tobytes() == col("reveal", 32).tobytes() and proof.tobytes() == col("proof", 64).tobytes()
    assert pk.tobytes() == _pk(keys).tobytes() and pk[0].tobytes() == D.BASE_ENC
    v, shared = lib_verify(hiplib, pk, peers, ctxs, reveal, proof, pairs)
    assert not v.any() and shared.tobytes() == col("shared", 32).tobytes()
    assert shared.tobytes() == D.shared_batch(keys, peers, pairs)[0].tobytes()       # what rofl_dh_shared gives for the pairs
    # deterministic; key s + l proves as s does
    assert lib_prove(hiplib, keys, peers, ctxs, pairs)[1].tobytes() == proof.tobytes()
    red = _b32(int.from_bytes(keys[2].tobytes(), "little") - ELL)
    assert lib_prove(hiplib, [red], peers[2:3], ctxs[2:3])[1].tobytes() == proof[2].tobytes()


def test_pairs_null_equals_explicit_and_keys_are_shared(hiplib):
    rng = np.random.default_rng(20270103)
    sks, peers = D.rand_keys(rng, 3), _pk(D.rand_keys(rng, 5))
    ctxs = np.frombuffer(rng.bytes(15 * 32), np.uint8).reshape(15, 32).copy()
    reveal, proof, status, pk = lib_prove(hiplib, sks, peers, ctxs)
    want = Q.prove_batch(sks, peers, ctxs)
    assert reveal.tobytes() == want[0].tobytes() and proof.tobytes() == want[1].tobytes() and not status.any()
    order = rng.permutation(15)
    pairs = [(int(i) // 5, int(i) % 5) for i in order]
    r2, p2, s2, _ = lib_prove(hiplib, sks, peers, ctxs[order], pairs)
    assert r2.tobytes() == reveal[order].tobytes() and p2.tobytes() == proof[order].tobytes()
    v, shared = lib_verify(hiplib, pk, peers, ctxs, reveal, proof)
    assert not v.any() and shared.tobytes() == D.shared_batch(sks, peers)[0].tobytes()
    v2, sh2 = lib_verify(hiplib, pk, peers, ctxs[order], r2, p2, pairs)
    assert not v2.any() and sh2.tobytes() == shared[order].tobytes()
    assert (lib_verify(hiplib, pk, peers, ctxs, r2, p2)[0] != 0).sum() == (order != np.arange(15)).sum()      # a proof under another pair's slot fails


def test_verdict_classes(hiplib, proved):
    sks, pks, peer, ctxs = proved
    own, peers, cx, reveals, proofs, want = Q.verdict_cases(sks, pks, peer, ctxs)
    assert set(want.tolist()) == {0, 1, 2} and len(want) <= 64
    pairs = [(i, i) for i in range(len(want))]
    mv, ms = Q.verify_batch(own, peers, cx, reveals, proofs, pairs)
    assert (mv == want).all()
    got, shared = lib_verify(hiplib, own, peers, cx, reveals, proofs, pairs)
    assert (got == want).all(), (got.tolist(), want.tolist())
    assert shared.tobytes() == ms.tobytes() and all(shared[i].any() == (want[i] == 0) for i in range(len(want)))


def test_late_reject_classes_at_every_decode_site(hiplib, proved):
    sks, pks, peer, ctxs = proved
    bad = [e for cls in LATE for e in RC.of_class(cls)[:2]]
    assert {e[2] for e in bad} == set(LATE)
    rows = RC.as_array(bad)
    n = len(rows)
    # as the peer in prove: status 1, zeros, the honest peer between them untouched
    peers = np.concatenate([rows, peer[None]])
    cx = np.tile(ctxs[0], (n + 1, 1))
    reveal, proof, status, _ = lib_prove(hiplib, sks[:1], peers, cx)
    want = Q.prove_batch(sks[:1], peers, cx)
    assert status.tolist() == [1] * n + [0] == want[2].tolist() and reveal.tobytes() == want[0].tobytes() and proof.tobytes() == want[1].tobytes()
    assert not reveal[:n].any() and not proof[:n].any()
    good_r, good_p = reveal[n], proof[n]
    # as A, as P and as S in verify: verdict 2, a zero secret; the good proof in the last slot keeps its verdict 0
    for site in range(3):
        own, prs, rv = np.tile(pks[0], (n + 1, 1)), np.tile(peer, (n + 1, 1)), np.tile(good_r, (n + 1, 1))
        (own, prs, rv)[site][:n] = rows
        pairs = [(i, i) for i in range(n + 1)]
        v, shared = lib_verify(hiplib, own, prs, cx, rv, np.tile(good_p, (n + 1, 1)), pairs)
        mv, ms = Q.verify_batch(own, prs, cx, rv, np.tile(good_p, (n + 1, 1)), pairs)
        assert v.tolist() == [2] * n + [0] == mv.tolist() and shared.tobytes() == ms.tobytes() and not shared[:n].any(), site


def test_parameter_checks_come_before_the_device(hiplib):
    L = hiplib
    rng = np.random.default_rng(20270104)
    sk = D.rand_keys(rng, 3)
    pk, peer = _pk(sk), _pk(D.rand_keys(rng, 2))
    ctx, reveal, proof, out, pko, shared = (np.zeros((6, w), np.uint8) for w in (32, 32, 64, 1, 32, 32))
    pairs = _pairs_arr([(0, 0), (1, 1), (2, 0)])
    zero_key = sk.copy(); zero_key[1] = _b32(ELL)
    zero_key0 = sk.copy(); zero_key0[0] = 0
    # (n_own, own, n_peer, peer, n_pairs, pairs, ctx), the text the error names
    common = [
        ((3, None, 2, peer, 6, None, ctx), "parameter"), ((3, "K", 2, None, 6, None, ctx), "parameter"), ((3, "K", 2, peer, 6, None, None), "parameter"),
        ((0, "K", 2, peer, 3, pairs, ctx), "without keys"), ((3, "K", 0, peer, 3, pairs, ctx), "without keys"),
        (((1 << 20) + 1, "K", 2, peer, 3, pairs, ctx), "2^20 keys"), ((3, "K", (1 << 20) + 1, peer, 3, pairs, ctx), "2^20 keys"),
        ((3, "K", 2, peer, (1 << 24) + 1, pairs, ctx), "2^24 pairs"),
        ((3, "K", 2, peer, 5, None, ctx), "n_own x n_peer"),
        ((3, "K", 2, peer, 3, _pairs_arr([(0, 0), (3, 1), (2, 0)]), ctx), "pair 1 names"), ((3, "K", 2, peer, 3, _pairs_arr([(0, 0), (1, 1), (2, 2)]), ctx), "pair 2 names"),
    ]
    for name in ("rofl_dleq_prove", "rofl_dbg_host_dleq_prove"):
        bad = common + [((3, "K", 2, peer, 6, None, ctx, None, proof, out), "parameter"), ((3, "K", 2, peer, 6, None, ctx, reveal, None, out), "parameter"),
                        ((3, "K", 2, peer, 6, None, ctx, reveal, proof, None), "parameter"),
                        ((3, zero_key, 2, peer, 6, None, ctx), "secret key 1 is zero mod l"), ((3, zero_key0, 2, peer, 3, pairs, ctx), "secret key 0 is zero mod l")]
        for args, text in bad:
            a = list(args) + [reveal, proof, out] * (len(args) == 7)
            keys = sk if isinstance(a[1], str) else a[1]
            assert _prove(L, name, a[0], keys, pko, a[2], a[3], a[4], a[5], a[6], a[7], a[8], a[9]) == 11, (name, text)
            assert text in _last_error(L).value.decode(), (name, text, _last_error(L).value)
        assert not reveal.any() and not proof.any() and not out.any() and not pko.any()
        assert _prove(L, name, 0, None, None, 0, None, 0, None, None, None, None, None) == 0      # an empty call returns 0 whatever else it is handed
        assert _prove(L, name, 3, sk, None, 2, peer, 0, pairs, None, None, None, None) == 0
    for name in ("rofl_dleq_verify", "rofl_dbg_host_dleq_verify"):
        bad = common + [((3, "K", 2, peer, 6, None, ctx, None, proof, out), "parameter"), ((3, "K", 2, peer, 6, None, ctx, reveal, None, out), "parameter"),
                        ((3, "K", 2, peer, 6, None, ctx, reveal, proof, None), "parameter")]
        for args, text in bad:
            a = list(args) + [reveal, proof, out] * (len(args) == 7)
            keys = pk if isinstance(a[1], str) else a[1]
            assert _verify(L, name, a[0], keys, a[2], a[3], a[4], a[5], a[6], a[7], a[8], shared, a[9]) == 11, (name, text)
            assert text in _last_error(L).value.decode(), (name, text, _last_error(L).value)
        assert not out.any() and not shared.any()
        assert _verify(L, name, 0, None, 0, None, 0, None, None, None, None, None, None) == 0
    # an error text holds no key bytes
    secret = np.ascontiguousarray(np.tile(np.arange(1, 33, dtype=np.uint8), (3, 1)))
    secret[2] = 0
    for name in ("rofl_dleq_prove", "rofl_dbg_host_dleq_prove"):
        assert _prove(L, name, 3, secret, pko, 2, peer, 6, None, ctx, reveal, proof, out) == 11
        err = _last_error(L)
        assert b"secret key 2 is zero" in err.value
        assert secret[0].tobytes() not in err.raw and secret[0, :8].tobytes() not in err.raw and secret[0].tobytes().hex() not in err.value.decode()


def _host_shim(hiplib, monkeypatch):
    from rofl_project_code_amd import api

    class Shim:
        rofl_dleq_prove = hiplib.rofl_dbg_host_dleq_prove
        rofl_dleq_verify = hiplib.rofl_dbg_host_dleq_verify
        rofl_last_error = hiplib.rofl_last_error

    Shim.rofl_dleq_prove.argtypes, Shim.rofl_dleq_verify.argtypes = PROVE_ARGS, VERIFY_ARGS
    monkeypatch.setattr(api, "lib", lambda: Shim)
    monkeypatch.setattr(api.key_agreement, "public_keys", staticmethod(lambda sk: _pk(sk)))
    return api


def test_wrappers_on_the_host_route(hiplib, proved, monkeypatch):
    """dleq.prove / verify with the two device entries replaced by their host routes (same parameters): shapes, dtypes, pairs"""
    api = _host_shim(hiplib, monkeypatch)
    G = api.dleq
    sks, pks, peer, ctxs = proved
    peers = np.stack([peer, pks[5]])
    cx = np.concatenate([ctxs, ctxs[::-1]])
    reveal, proof, status, own = G.prove(sks, peers, cx, with_public=True)
    assert reveal.shape == (12, 32) and proof.shape == (12, 64) and status.shape == (12,) and own.shape == (6, 32) and reveal.dtype == proof.dtype == status.dtype == np.uint8
    want = Q.prove_batch(sks, peers, cx)
    assert reveal.tobytes() == want[0].tobytes() and proof.tobytes() == want[1].tobytes() and not status.any() and (own == pks).all()
    pairs = [(5, 0), (0, 1), (5, 0)]
    r3, p3, s3 = G.prove([bytes(k) for k in sks], peers, cx[[10, 1, 10]], pairs)
    assert r3.tobytes() == reveal[[10, 1, 10]].tobytes() and p3.tobytes() == proof[[10, 1, 10]].tobytes()
    bad = proof.copy(); bad[2, 0] ^= 2
    v, shared = G.verify(pks, peers, cx, reveal, bad)
    assert v.shape == (12,) and v.dtype == np.uint8 and shared.shape == (12, 32) and np.flatnonzero(v).tolist() == [2] and v[2] == 1 and not shared[2].any()
    assert shared[[0, 1, 3]].tobytes() == D.shared_batch(sks, peers, [(0, 0), (0, 1), (1, 1)])[0].tobytes()
    assert G.verify(pks, peers, cx[[10, 1]], r3[:2], p3[:2].reshape(-1), pairs[:2])[0].tolist() == [0, 0]
    # a refused peer condemns its pairs only
    r, p, s = G.prove(sks[:2], np.stack([peer, np.zeros(32, np.uint8)]), cx[:4])
    assert s.tolist() == [0, 2, 0, 2] and not r[1].any() and not p[3].any() and r[0].any()
    # nothing to compute
    r, p, s = G.prove(sks[:0], peers, cx[:0])
    assert r.shape == (0, 32) and p.shape == (0, 64) and s.shape == (0,)
    r, p, s, own0 = G.prove(sks, peers, cx[:0], [], with_public=True)
    assert r.shape == (0, 32) and (own0 == pks).all()
    v, sh = G.verify(pks, peers, cx[:0], reveal[:0], proof[:0], [])
    assert v.shape == (0,) and sh.shape == (0, 32)
    # the wrappers' own checks, and the library's through the wrapper
    for call in (lambda: G.prove(sks, peers, cx[:11]), lambda: G.prove(sks, peers, cx[:1], [(6, 0)]), lambda: G.prove(sks, peers, cx[:1], [(0, -1)]),
                 lambda: G.prove(np.zeros((2, 31), np.uint8), peers, cx[:4]), lambda: G.verify(pks, peers, cx, reveal, proof[:11]),
                 lambda: G.verify(pks, peers, cx, reveal[:11], proof), lambda: G.verify(pks, peers, cx, reveal, np.zeros((12, 63), np.uint8)),
                 lambda: G.verify(pks, peers, cx[:1], reveal[:1], proof[:1], [(0, 2)])):
        with pytest.raises(ValueError):
            call()
    with pytest.raises(api.RoflError) as e:
        G.prove(np.zeros((1, 32), np.uint8), peers, cx[:2])
    assert e.value.code == 11 and "secret key 0" in str(e.value)


# ---------------------------------------------------------------- the round's helpers above the device calls, on the models
@pytest.fixture()
def model_device(monkeypatch):
    """signatures.sign / verify, dleq.prove / verify and aead.open replaced by the models, verify_shares by a look-up of the polynomial behind
    a commitment row (a row nobody dealt is refused: verdict 2); the list records every underlying call by name"""
    from rofl_project_code_amd import api
    calls, polys = [], {}

    def sign(sks, messages, refs=None, with_public=False):
        calls.append("sign")
        return S.sign_batch(sks, [bytes(m) for m in messages], refs)

    def sig_verify(pks, messages, sigs, refs=None):
        calls.append("sig.verify")
        return S.verify_batch(pks, [bytes(m) for m in messages], sigs, refs)

    def prove(sks, peer_pks, ctxs, pairs=None, with_public=False):
        calls.append("prove")
        return Q.prove_batch(sks, peer_pks, ctxs, pairs)

    def verify(own_pks, peer_pks, ctxs, reveals, proofs, pairs=None):
        calls.append("dleq.verify")
        return Q.verify_batch(own_pks, peer_pks, ctxs, reveals, proofs, pairs)

    def aead_open(keys, nonces, ads, sealed, key_idx=None, derive_round=None):
        calls.append("open")
        assert isinstance(sealed, np.ndarray) and sealed.ndim == 2 and key_idx is None
        pt, v = A.open_batch(keys, nonces, [bytes(a) for a in ads], [bytes(r) for r in sealed], derive_round=derive_round)
        return np.frombuffer(b"".join(pt), np.uint8).reshape(len(pt), -1).copy(), v

    def verify_shares(commitments, xs, shares):
        calls.append("verify_shares")
        out = np.zeros((len(commitments), len(xs)), np.uint8)
        for r, row in enumerate(np.asarray(commitments, np.uint8)):
            p = polys.get(row.tobytes())
            out[r] = 2 if p is None else F.verdicts([p], xs, np.asarray(shares, np.uint8)[r:r + 1])[0]
        return out

    monkeypatch.setattr(api.signatures, "sign", staticmethod(sign))
    monkeypatch.setattr(api.signatures, "verify", staticmethod(sig_verify))
    monkeypatch.setattr(api.dleq, "prove", staticmethod(prove))
    monkeypatch.setattr(api.dleq, "verify", staticmethod(verify))
    monkeypatch.setattr(api.aead, "open", staticmethod(aead_open))
    monkeypatch.setattr(api.secret_sharing, "verify_shares", staticmethod(verify_shares))
    return calls, polys


@pytest.fixture(scope="module")
def round7():
    """the six-client, threshold-4 round 7 dealt, sealed and signed by the models, with dealer 5's flipped share and dealer 4's altered record"""
    rng = np.random.default_rng(20270105)
    N, T, RND = Q.N, Q.THRESHOLD, Q.ROUND_NO
    ids = list(range(N))
    sk, b, cs = D.rand_keys(rng, N), rng.integers(0, 256, size=(N, 32), dtype=np.uint8), rng.integers(0, 256, size=(2 * N, 32), dtype=np.uint8)
    key_sh, self_sh = M.share(sk, cs[:N], T, N), M.share(b, cs[N:], T, N)
    polys = F.polynomials(np.concatenate([sk, b]), cs, T)
    com = np.stack([F.commit_ints(p) for p in polys])
    ch_sk, sig_sk = D.rand_keys(rng, N), D.rand_keys(rng, N)
    ch_pk, sig_pk = _pk(ch_sk), _pk(sig_sk)
    shared = [[D.shared(ch_sk[a], ch_pk[c])[0] for c in range(N)] for a in range(N)]
    sent = Q.alter_before_signing(A.seal_shares(shared, ids, ids, RND, Q.deal_with_faults(key_sh), self_sh))
    return dict(ids=ids, key_sh=key_sh, self_sh=self_sh, com=com, polys=polys, ch_sk=ch_sk, ch_pk=ch_pk, sig_sk=sig_sk, sig_pk=sig_pk, sent=sent, shared=shared)


def test_bundle_and_context_layouts_byte_for_byte():
    from rofl_project_code_amd.api import secret_sharing as SS
    rec = np.arange(80, dtype=np.uint8)
    m = SS.bundle_message(2 ** 40 + 5, 70000, 3, rec)
    assert m == Q.bundle_message(2 ** 40 + 5, 70000, 3, rec) and len(m) == 112 and isinstance(m, bytes) and m[:16] == b"rofl-zk/sealed/1" and m[32:] == rec.tobytes()
    assert SS.bundle_message(1, 2, 3, rec) != SS.bundle_message(1, 3, 2, rec) != SS.bundle_message(2, 3, 2, rec)
    with pytest.raises(ValueError):
        SS.bundle_message(1, 2, 3, rec[:79])
    c = SS.complaint_context(2 ** 40 + 5, 70000, 3)
    assert c == Q.complaint_context(2 ** 40 + 5, 70000, 3) and len(c) == 32 and isinstance(c, bytes)
    assert SS.complaint_context(7, 3, 5) != SS.complaint_context(7, 5, 3) != SS.complaint_context(8, 5, 3)


def test_sign_bundles_and_file_complaints_are_one_call_each(round7, model_device):
    from rofl_project_code_amd.api import secret_sharing as SS
    calls, _ = model_device
    r = round7
    sigs = SS.sign_bundles(r["sig_sk"], Q.ROUND_NO, r["ids"], r["ids"], r["sent"])
    assert calls == ["sign"] and sigs.shape == (6, 6, 64) and sigs.dtype == np.uint8
    assert sigs[4, 1].tobytes() == S.sign(r["sig_sk"][4], Q.bundle_message(Q.ROUND_NO, 4, 1, r["sent"][4, 1]))
    del calls[:]
    v = SS.verify_bundle_signatures(r["sig_pk"], Q.ROUND_NO, r["ids"], r["ids"], r["sent"], sigs)
    assert calls == ["sig.verify"] and v.shape == (6, 6) and not v.any()
    # a recipient's inbox: the senders' records for client 2, one of them changed on the way -- a missing record, not a complaint
    inbox = r["sent"][:, 2:3].copy(); inbox[3, 0, 70] ^= 1
    assert SS.verify_bundle_signatures(r["sig_pk"], Q.ROUND_NO, r["ids"], [2], inbox, sigs[:, 2:3])[:, 0].tolist() == [0, 0, 0, 1, 0, 0]
    assert SS.verify_bundle_signatures(r["sig_pk"], Q.ROUND_NO + 1, r["ids"], [2], r["sent"][:, 2:3], sigs[:, 2:3]).all()
    for bad in (lambda: SS.sign_bundles(r["sig_sk"][:5], 7, r["ids"], r["ids"], r["sent"]), lambda: SS.sign_bundles(r["sig_sk"], 7, r["ids"], r["ids"], r["sent"][:, :5]),
                lambda: SS.verify_bundle_signatures(r["sig_pk"], 7, r["ids"], r["ids"], r["sent"], sigs[:, :, :63])):
        with pytest.raises(ValueError):
            bad()
    del calls[:]
    which = [(3, 5), (1, 4), (1, 3)]
    reveals, proofs = SS.file_complaints(r["ch_sk"][[1, 3]], [1, 3], r["ids"], r["ch_pk"], Q.ROUND_NO, which)
    assert calls == ["prove"] and reveals.shape == (3, 32) and proofs.shape == (3, 64)
    for i, (c, d) in enumerate(which):
        assert (reveals[i].tobytes(), proofs[i].tobytes(), 0) == Q.prove(r["ch_sk"][c], r["ch_pk"][d], Q.complaint_context(Q.ROUND_NO, c, d))
    with pytest.raises(ValueError, match=r"\(2, 5\)"):
        SS.file_complaints(r["ch_sk"][[1, 3]], [1, 3], r["ids"], r["ch_pk"], Q.ROUND_NO, [(2, 5)])
    refused = r["ch_pk"].copy(); refused[4] = 0
    with pytest.raises(ValueError, match=r"dealer 4\b.*status 2"):
        SS.file_complaints(r["ch_sk"][[1, 3]], [1, 3], r["ids"], refused, Q.ROUND_NO, which)


def test_judge_complaints_on_the_models(round7, model_device):
    from rofl_project_code_amd.api import secret_sharing as SS
    calls, polys = model_device
    r = round7
    for row, p in zip(r["com"], r["polys"]):
        polys[row.tobytes()] = p
    sigs = SS.sign_bundles(r["sig_sk"], Q.ROUND_NO, r["ids"], r["ids"], r["sent"])

    def reveal_and_proof(c, d, round_no):
        rv, pf = SS.file_complaints(r["ch_sk"][c:c + 1], [c], [d], r["ch_pk"][d:d + 1], round_no, [(c, d)])
        return rv[0], pf[0]

    complaints = Q.round_complaints(r["sent"], sigs, reveal_and_proof)
    key_com, self_com = r["com"][:6], r["com"][6:]
    del calls[:]
    got = SS.judge_complaints(Q.ROUND_NO, complaints, r["ch_pk"], r["sig_pk"], key_com, self_com)
    assert got == Q.RULINGS
    assert calls == ["sig.verify", "dleq.verify", "open", "verify_shares"]                       # exactly one call each
    # any order, any subset, dicts for the tables; no complaint, no call
    del calls[:]
    as_dict = lambda t: {i: t[i] for i in range(6)}      # noqa: E731
    assert SS.judge_complaints(Q.ROUND_NO, complaints[::-1][:3], as_dict(r["ch_pk"]), as_dict(r["sig_pk"]), as_dict(key_com), as_dict(self_com)) == Q.RULINGS[::-1][:3]
    assert len(calls) == 4
    del calls[:]
    assert SS.judge_complaints(Q.ROUND_NO, [], r["ch_pk"], r["sig_pk"], key_com, self_com) == [] and calls == []
    # the order of the checks: a complaint that fails several at once gets the first reason
    c0 = complaints[0]
    both = [(c0[0], c0[1], c0[2], complaints[2][3], c0[4], complaints[3][5])]                   # a wrong signature AND a wrong proof
    assert SS.judge_complaints(Q.ROUND_NO, both, r["ch_pk"], r["sig_pk"], key_com, self_com) == [Q.judge(False, 1, False, False, 3, 5)] == [(3, 4)]
    judged_in_8 = SS.judge_complaints(Q.ROUND_NO + 1, complaints[:1], r["ch_pk"], r["sig_pk"], key_com, self_com)
    assert judged_in_8 == [(3, 4)]                                                              # judged in another round: nothing of it verifies
    # the self share flipped instead of the key share is reason 0 as well; the record of the judge's first complaint opens to what client 3 opened
    shared35 = r["shared"][3][5]
    pt, v = A.open_(A.derive_key(shared35, Q.ROUND_NO), A.bundle_nonce(5, 3), A.bundle_ad(Q.ROUND_NO, 5, 3), bytes(r["sent"][5, 3]))
    assert v == 0 and pt[:32] == Q.deal_with_faults(r["key_sh"])[5, 3].tobytes() != r["key_sh"][5, 3].tobytes() and pt[32:] == r["self_sh"][5, 3].tobytes()
    # a commitment row that does not decode: ValueError naming the dealer; the same pair twice: ValueError
    broken = key_com.copy(); broken[2, 1] = 0xff
    with pytest.raises(ValueError, match=r"dealer 2\b.*key"):
        SS.judge_complaints(Q.ROUND_NO, complaints, r["ch_pk"], r["sig_pk"], broken, self_com)
    with pytest.raises(ValueError, match="same"):
        SS.judge_complaints(Q.ROUND_NO, [complaints[0], complaints[0]], r["ch_pk"], r["sig_pk"], key_com, self_com)
    with pytest.raises(ValueError, match="80 bytes"):
        SS.judge_complaints(Q.ROUND_NO, [c0[:2] + (c0[2][:79],) + c0[3:]], r["ch_pk"], r["sig_pk"], key_com, self_com)


def test_judging_order_table():
    """the first reason that applies decides, over every combination of what the four calls can say"""
    for sig_ok in (True, False):
        for pv in (0, 1, 2):
            for opens in (True, False):
                for ok in (True, False):
                    who, why = Q.judge(sig_ok, pv, opens, ok, 3, 5)
                    want = 4 if not sig_ok else 3 if pv else 1 if not opens else 0 if not ok else 2
                    assert why == want and who == (5 if want in (0, 1) else 3)


def test_new_entry_points_are_exported_and_declared_for_rust(hiplib):
    names = ("rofl_dleq_prove", "rofl_dleq_verify", "rofl_dbg_host_dleq_prove", "rofl_dbg_host_dleq_verify")
    for name in names:
        assert hasattr(hiplib, name), name
    hdr = open(os.path.join(ROOT, "include", "rofl_zk.h")).read()
    dbg = open(os.path.join(ROOT, "include", "rofl_zk_debug.h")).read()
    assert all(n + "(" in hdr for n in names[:2]) and all(n + "(" in dbg for n in names[2:])
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "check_ffi.py")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    ffi = open(os.path.join(ROOT, "integration", "rofl_crypto_overlay", "src", "ffi.rs")).read()
    assert all("pub fn %s(" % n in ffi for n in names[:2])
    import rofl_project_code_amd as R
    assert R.dleq is R.api.dleq
