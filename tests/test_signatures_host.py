"""CPU-only checks of the signatures (rofl_sig_sign / rofl_sig_verify): the Python model of the definition (tests/sig_model.py) against point
arithmetic by hand, the host route rofl_dbg_host_sig_* against the model (edge keys, every padding case of the digest at misaligned starts,
every verdict class, shared keys and messages), every parameter check of the four C entry points (they come before the device is touched),
the Python wrappers on the host route, the round's helpers with the device calls replaced by the model, and the Rust declarations.  No call
here reaches a GPU."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import dh_model as D
import ristretto_corpus as RC
import sig_model as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sz, vp = ctypes.c_size_t, ctypes.c_void_p
ELL = S.L
SIGN_ARGS = [sz, vp, vp, sz, vp, vp, sz, vp, vp]
VERIFY_ARGS = [sz, vp, sz, vp, vp, sz, vp, vp, vp]
LENS = S.LENS


def _p(x):
    return None if x is None else x.ctypes.data


def _b32(v):
    return np.frombuffer(int(v).to_bytes(32, "little"), np.uint8)


def _refs_arr(refs):
    return None if refs is None else np.ascontiguousarray(np.asarray(refs, np.uint32).reshape(-1, 2))


def _sign(L, name, n_keys, sk, pk_out, n_msgs, data, off, n, refs, sig):
    fn = getattr(L, name)
    fn.argtypes = SIGN_ARGS
    return fn(n_keys, _p(sk), _p(pk_out), n_msgs, _p(data), _p(off), n, _p(refs), _p(sig))


def _verify(L, name, n_keys, pk, n_msgs, data, off, n, refs, sig, out):
    fn = getattr(L, name)
    fn.argtypes = VERIFY_ARGS
    return fn(n_keys, _p(pk), n_msgs, _p(data), _p(off), n, _p(refs), _p(sig), _p(out))


def host_sign(L, sks, msgs, refs=None, name="rofl_dbg_host_sig_sign"):
    sks = np.ascontiguousarray(np.asarray(sks, np.uint8).reshape(-1, 32))
    data, off = S.pack(msgs)
    r = _refs_arr(refs)
    n = len(sks) if r is None else len(r)
    sig, pk = np.full((n, 64), 0xaa, np.uint8), np.full((len(sks), 32), 0xaa, np.uint8)
    assert _sign(L, name, len(sks), sks, pk, len(msgs), data if data.size else None, off, n, r, sig) == 0
    return sig, pk


def host_verify(L, pks, msgs, sigs, refs=None, name="rofl_dbg_host_sig_verify"):
    pks = np.ascontiguousarray(np.asarray(pks, np.uint8).reshape(-1, 32))
    sigs = np.ascontiguousarray(np.asarray(sigs, np.uint8).reshape(-1, 64))
    data, off = S.pack(msgs)
    r = _refs_arr(refs)
    out = np.full(len(sigs), 0xaa, np.uint8)
    assert _verify(L, name, len(pks), pks, len(msgs), data if data.size else None, off, len(sigs), r, sigs, out) == 0
    return out


def _last_error(L):
    err = ctypes.create_string_buffer(512)
    L.rofl_last_error(err, sz(512))
    return err


@pytest.fixture(scope="module")
def edge_keys():
    """1, l - 1, s + l, 2^256 - 1"""
    rng = np.random.default_rng(20261101)
    s = int.from_bytes(rng.bytes(31), "little")
    assert s + ELL < 2 ** 256
    return np.stack([_b32(v) for v in (1, ELL - 1, s + ELL, 2 ** 256 - 1)]).copy()


@pytest.fixture(scope="module")
def signed(hiplib):
    """five keys each signing one message of its own through the host route: (sks, pks, msgs, sigs), all verdicts 0"""
    rng = np.random.default_rng(20261102)
    sks = D.rand_keys(rng, 5)
    msgs = [rng.bytes(n) for n in (40, 0, 137, 300, 9)]
    sigs, pks = host_sign(hiplib, sks, msgs)
    assert not host_verify(hiplib, pks, msgs, sigs).any()
    return sks, pks, msgs, sigs


def test_model_is_the_definition():
    import hashlib
    pyref = S.pyref
    sk, m = bytes(range(1, 33)), b"a round's commitments"
    assert S.digest(b"") == hashlib.shake_256(b"rofl-zk/sig/v1/m" + bytes(8)).digest(32)
    assert S.digest(m) == hashlib.shake_256(b"rofl-zk/sig/v1/m" + (21).to_bytes(8, "little") + m).digest(32)
    sig = S.sign(sk, m, fast=False)
    assert sig == S.sign(sk, m) and len(sig) == 64                               # fast=False equals fast=True, once
    a, A = D.sk_int(sk), S.public_key(sk, fast=False)
    h = S.digest(m)
    k = int.from_bytes(hashlib.shake_256(b"rofl-zk/sig/v1/k" + a.to_bytes(32, "little") + h).digest(64), "little") % ELL
    R, s = sig[:32], int.from_bytes(sig[32:], "little")
    assert R == pyref.ristretto_encode(pyref.pt_mul(k, pyref.BASE)) and s < ELL
    c = int.from_bytes(hashlib.shake_256(b"rofl-zk/sig/v1/c" + R + A + h).digest(64), "little") % ELL
    assert s == (k + c * a) % ELL
    # the verification equation on points, by hand: s B == R + c A
    lhs = pyref.pt_mul(s, pyref.BASE)
    rhs = pyref.pt_add(pyref.ristretto_decode(R), pyref.pt_mul(c, pyref.ristretto_decode(A)))
    assert pyref.ristretto_encode(lhs) == pyref.ristretto_encode(rhs)
    assert S.verdict(A, m, sig, fast=False) == S.verdict(A, m, sig) == 0
    bad = bytearray(sig); bad[40] ^= 1
    assert S.verdict(A, m, bytes(bad), fast=False) == S.verdict(A, m, bytes(bad)) == 1
    assert S.verdict(A, m + b"!", sig) == 1 and S.verdict(bytes(32), m, sig) == 2 and S.verdict(b"\xff" * 32, m, sig) == 2
    assert S.verdict(A, m, R + (s + ELL).to_bytes(32, "little")) == 2


def test_host_route_equals_the_model(hiplib, edge_keys):
    rng = np.random.default_rng(20261103)
    msgs, where = S.misaligned_messages(rng)
    com64 = rng.integers(0, 256, size=(64, 32), dtype=np.uint8)
    for long in (S.commitment_message(7, 3, 1, com64), rng.bytes(2085)):             # the commitment message of t = 64 (33 + 64 * 32 bytes); 2 085 bytes
        msgs.append(rng.bytes(1 if sum(len(m) for m in msgs) % 2 == 0 else 2))       # (an odd start for the two long ones as well)
        msgs.append(long)
    assert len(msgs[-3]) == 2081 and [len(msgs[w]) for w in where] == list(LENS)
    data, off = S.pack(msgs)
    assert all(int(off[w]) % 8 for w in where) and {int(off[w]) % 8 for w in where} == set(range(1, 8)) and int(off[-2]) % 2 == 1 and int(off[-4]) % 2 == 1
    refs = [(a, b) for a in range(len(edge_keys)) for b in range(len(msgs))]
    sig, pk = host_sign(hiplib, edge_keys, msgs, refs)
    want = S.sign_batch(edge_keys, msgs, refs)
    assert sig.tobytes() == want.tobytes()
    assert [p.tobytes() for p in pk] == [S.public_key(k) for k in edge_keys] and pk[0].tobytes() == D.BASE_ENC
    # deterministic: the same bytes again; key s + l signs as s does
    assert host_sign(hiplib, edge_keys, msgs, refs)[0].tobytes() == sig.tobytes()
    red = _b32(int.from_bytes(edge_keys[2].tobytes(), "little") - ELL)
    assert host_sign(hiplib, [red], msgs, [(0, b) for b in range(len(msgs))])[0].tobytes() == sig[2 * len(msgs):3 * len(msgs)].tobytes()
    got = host_verify(hiplib, pk, msgs, sig, refs)
    assert not got.any() and (got == S.verify_batch(pk, msgs, sig, refs)).all()
    # a signature under another message of the same length class, or another key, fails
    assert (host_verify(hiplib, pk, msgs, sig[[1, 0]], [(0, 0), (0, 1)]) == 1).all()
    assert (host_verify(hiplib, pk, msgs, sig[:2], [(1, 0), (1, 1)]) == 1).all()


def test_verdict_classes(hiplib, signed):
    sks, pks, msgs, sigs = signed
    keys, ms, sg, want = S.verdict_cases(pks, msgs, sigs)
    assert set(want.tolist()) == {0, 1, 2} and (S.verify_batch(keys, ms, sg) == want).all()
    got = host_verify(hiplib, keys, ms, sg)
    assert (got == want).all(), (got.tolist(), want.tolist())


def test_refs_share_keys_and_messages(hiplib, signed):
    sks, pks, msgs, sigs = signed
    # one key on every message; every key on one message (the view shape); refs = None is (i, i)
    one_key = [(2, b) for b in range(5)]
    sig_a, _ = host_sign(hiplib, sks, msgs, one_key)
    assert sig_a.tobytes() == S.sign_batch(sks, msgs, one_key).tobytes() and sig_a[2].tobytes() == sigs[2].tobytes()
    assert not host_verify(hiplib, pks, msgs, sig_a, one_key).any()
    assert not host_verify(hiplib, pks[2:3], msgs, sig_a, [(0, b) for b in range(5)]).any()
    one_msg = [(a, 3) for a in range(5)]
    sig_b, _ = host_sign(hiplib, sks, msgs[3:4], [(a, 0) for a in range(5)])
    assert sig_b.tobytes() == S.sign_batch(sks, msgs, one_msg).tobytes()
    v = sig_b.copy(); v[1, 50] ^= 4
    assert host_verify(hiplib, pks, msgs[3:4], v, [(a, 0) for a in range(5)]).tolist() == [0, 1, 0, 0, 0]
    explicit = [(i, i) for i in range(5)]
    assert host_sign(hiplib, sks, msgs, explicit)[0].tobytes() == sigs.tobytes()
    assert (host_verify(hiplib, pks, msgs, sigs, explicit) == host_verify(hiplib, pks, msgs, sigs)).all()
    # refs in any order, with repeats
    mixed = [(4, 0), (0, 4), (4, 0), (1, 1)]
    assert host_sign(hiplib, sks, msgs, mixed)[0].tobytes() == S.sign_batch(sks, msgs, mixed).tobytes()


def test_parameter_checks_come_before_the_device(hiplib):
    L = hiplib
    rng = np.random.default_rng(20261104)
    sk = D.rand_keys(rng, 3)
    pk = np.frombuffer(b"".join(S.public_key(k) for k in sk), np.uint8).reshape(3, 32).copy()
    data, off = S.pack([b"abc", b"", b"defgh"])
    sig, pko, out = np.zeros((3, 64), np.uint8), np.zeros((3, 32), np.uint8), np.zeros(3, np.uint8)
    u64 = lambda *v: np.array(v, np.uint64)      # noqa: E731
    refs = _refs_arr([(0, 0), (1, 1), (2, 2)])
    big_off = np.zeros((1 << 20) + 2, np.uint64)
    zero_key = sk.copy(); zero_key[1] = _b32(ELL)
    zero_key0 = sk.copy(); zero_key0[0] = 0
    # (n_keys, keys, n_msgs, data, off, n, refs), the text the error names
    common = [
        ((3, None, 3, data, off, 3, None), "parameter"), ((3, "K", 3, data, None, 3, None), "parameter"),
        ((3, "K", 3, None, off, 3, None), "parameter"),                              # message bytes may be NULL only when there are none
        ((3, "K", 3, data, u64(1, 3, 3, 8), 3, None), "first message offset"),
        ((3, "K", 3, data, u64(0, 3, 2, 8), 3, None), "offset 2 is below"),
        ((3, "K", 3, data, u64(0, 3, 3, (1 << 30) + 1), 3, None), "2^30 message bytes"),
        (((1 << 20) + 1, "K", 3, data, off, 3, refs), "2^20 keys"), ((3, "K", (1 << 20) + 1, data, big_off, 3, refs), "2^20 messages"),
        ((3, "K", 3, data, off, (1 << 24) + 1, refs), "2^24 signatures"),
        ((0, "K", 3, data, off, 3, refs), "without keys"), ((3, "K", 0, data, off, 3, refs), "without keys"),
        ((3, "K", 3, data, off, 3, _refs_arr([(0, 0), (3, 1), (2, 2)])), "ref 1 names"),
        ((3, "K", 3, data, off, 3, _refs_arr([(0, 0), (1, 1), (2, 3)])), "ref 2 names"),
        ((3, "K", 3, data, off, 2, None), "are equal"), ((2, "K", 3, data, off, 3, None), "are equal"), ((3, "K", 2, data, off, 3, None), "are equal"),
    ]
    for name in ("rofl_sig_sign", "rofl_dbg_host_sig_sign"):
        bad = common + [((3, "K", 3, data, off, 3, refs, None), "parameter"),
                        ((3, zero_key, 3, data, off, 3, None), "secret key 1 is zero mod l"), ((3, zero_key0, 3, data, off, 3, refs), "secret key 0 is zero mod l")]
        for args, text in bad:
            a = list(args) + [sig] * (len(args) == 7)
            keys = sk if isinstance(a[1], str) else a[1]
            assert _sign(L, name, a[0], keys, pko, a[2], a[3], a[4], a[5], a[6], a[7]) == 11, (name, text)
            assert text in _last_error(L).value.decode(), (name, text, _last_error(L).value)
        assert not sig.any() and not pko.any()
        assert _sign(L, name, 0, None, None, 0, None, None, 0, None, None) == 0      # an empty call returns 0 whatever else it is handed
        assert _sign(L, name, 3, sk, None, 3, data, u64(5, 1), 0, None, None) == 0
    for name in ("rofl_sig_verify", "rofl_dbg_host_sig_verify"):
        bad = common + [((3, "K", 3, data, off, 3, refs, None, out), "parameter"), ((3, "K", 3, data, off, 3, refs, sig, None), "parameter")]
        for args, text in bad:
            a = list(args) + [sig, out] * (len(args) == 7)
            keys = pk if isinstance(a[1], str) else a[1]
            assert _verify(L, name, a[0], keys, a[2], a[3], a[4], a[5], a[6], a[7], a[8]) == 11, (name, text)
            assert text in _last_error(L).value.decode(), (name, text, _last_error(L).value)
        assert not out.any()
        assert _verify(L, name, 0, None, 0, None, None, 0, None, None, None) == 0
    # pk_out32, refs and the bytes of empty messages may be NULL (the host route; the device entries are the GPU suite's)
    empty = u64(0, 0, 0, 0)
    s3 = np.zeros((3, 64), np.uint8)
    assert _sign(L, "rofl_dbg_host_sig_sign", 3, sk, None, 3, None, empty, 3, None, s3) == 0
    assert s3.tobytes() == S.sign_batch(sk, [b""] * 3).tobytes()
    assert _verify(L, "rofl_dbg_host_sig_verify", 3, pk, 3, None, empty, 3, None, s3, out) == 0 and not out.any()
    # an error text holds no key bytes
    secret = np.ascontiguousarray(np.tile(np.arange(1, 33, dtype=np.uint8), (3, 1)))
    secret[2] = 0
    for name in ("rofl_sig_sign", "rofl_dbg_host_sig_sign"):
        assert _sign(L, name, 3, secret, pko, 3, data, off, 3, None, sig) == 11
        err = _last_error(L)
        assert b"secret key 2 is zero" in err.value
        assert secret[0].tobytes() not in err.raw and secret[0, :8].tobytes() not in err.raw and secret[0].tobytes().hex() not in err.value.decode()


def test_wrappers_on_the_host_route(hiplib, edge_keys, monkeypatch):
    """signatures.sign / verify with the two device entries replaced by their host routes (same parameters): shapes, dtypes, packing, refs"""
    from rofl_project_code_amd import api

    class Shim:
        rofl_sig_sign = hiplib.rofl_dbg_host_sig_sign
        rofl_sig_verify = hiplib.rofl_dbg_host_sig_verify
        rofl_last_error = hiplib.rofl_last_error

    Shim.rofl_sig_sign.argtypes, Shim.rofl_sig_verify.argtypes = SIGN_ARGS, VERIFY_ARGS
    monkeypatch.setattr(api, "lib", lambda: Shim)
    monkeypatch.setattr(api.key_agreement, "public_keys", staticmethod(lambda sk: np.stack([np.frombuffer(S.public_key(k), np.uint8) for k in np.asarray(sk, np.uint8).reshape(-1, 32)])))
    G = api.signatures
    msgs = [b"one", bytearray(b""), memoryview(b"three33"), np.arange(200, dtype=np.uint8)]
    plain = [bytes(m) for m in msgs]
    sig, pk = G.sign(edge_keys, msgs, with_public=True)
    assert sig.shape == (4, 64) and sig.dtype == np.uint8 and pk.shape == (4, 32)
    assert sig.tobytes() == S.sign_batch(edge_keys, plain).tobytes() and [p.tobytes() for p in pk] == [S.public_key(k) for k in edge_keys]
    assert (G.public_keys(edge_keys) == pk).all()
    refs = [(3, 0), (0, 3), (0, 0)]
    assert G.sign([bytes(k) for k in edge_keys], msgs, refs).tobytes() == S.sign_batch(edge_keys, plain, refs).tobytes()
    bad = sig.copy(); bad[2, 0] ^= 2
    v = G.verify(pk, msgs, bad)
    assert v.shape == (4,) and v.dtype == np.uint8 and v.tolist() == [0, 0, 1, 0]
    assert G.verify(pk, msgs, sig[[3, 0]], [(3, 3), (0, 0)]).tolist() == [0, 0]
    assert G.verify(pk[:, ::1][::-1][::-1], msgs, sig.reshape(-1)).tolist() == [0, 0, 0, 0]
    # nothing to compute
    assert G.sign(edge_keys[:0], []).shape == (0, 64) and G.verify(pk, msgs, np.zeros((0, 64), np.uint8), []).shape == (0,)
    out, p0 = G.sign(edge_keys, msgs, [], with_public=True)
    assert out.shape == (0, 64) and (p0 == pk).all()
    # the wrappers' own checks, and the library's through the wrapper
    for call in (lambda: G.sign(edge_keys, msgs[:3]), lambda: G.sign(edge_keys, msgs, [(4, 0)]), lambda: G.sign(edge_keys, msgs, [(0, -1)]),
                 lambda: G.sign(np.zeros((2, 31), np.uint8), msgs[:2]), lambda: G.verify(pk, msgs, sig[:3]), lambda: G.verify(pk, msgs, sig, [(0, 4)] * 4),
                 lambda: G.verify(pk, msgs, np.zeros((4, 63), np.uint8))):
        with pytest.raises(ValueError):
            call()
    with pytest.raises(api.RoflError) as e:
        G.sign(np.zeros((1, 32), np.uint8), [b"m"])
    assert e.value.code == 11 and "secret key 0" in str(e.value)


# ---------------------------------------------------------------- the round's helpers above the device calls, on the model
@pytest.fixture()
def model_device(monkeypatch):
    """signatures.sign / verify replaced by the model; the list records every underlying call as (name, n_keys, n_msgs, refs)"""
    from rofl_project_code_amd import api
    calls = []

    def sign(sks, messages, refs=None, with_public=False):
        sks = np.asarray(sks, np.uint8).reshape(-1, 32)
        calls.append(("sign", len(sks), len(messages), None if refs is None else [tuple(r) for r in refs]))
        return S.sign_batch(sks, [bytes(m) for m in messages], refs)

    def verify(pks, messages, sigs, refs=None):
        pks = np.asarray(pks, np.uint8).reshape(-1, 32)
        calls.append(("verify", len(pks), len(messages), None if refs is None else [tuple(r) for r in refs]))
        return S.verify_batch(pks, [bytes(m) for m in messages], sigs, refs)

    monkeypatch.setattr(api.signatures, "sign", staticmethod(sign))
    monkeypatch.setattr(api.signatures, "verify", staticmethod(verify))
    return calls


@pytest.fixture(scope="module")
def dealt():
    """four dealers of round 9 with signing keys of their own and two rows of three (made-up) commitments each"""
    rng = np.random.default_rng(20261105)
    sks = D.rand_keys(rng, 4)
    pks = np.stack([np.frombuffer(S.public_key(k), np.uint8) for k in sks])
    key_com, self_com = RC.honest_points(12).reshape(4, 3, 32), RC.honest_points(12, offset=12).reshape(4, 3, 32)
    return dict(sks=sks, pks=pks, key_com=key_com, self_com=self_com, dealers=[5, 0, 2, 9])


def test_message_layouts_byte_for_byte():
    from rofl_project_code_amd.api import secret_sharing as SS
    com = RC.honest_points(64)
    m = SS.commitment_message(2 ** 40 + 5, 70000, 1, com)
    assert m == b"rofl-zk/vss/v1\0\0" + (2 ** 40 + 5).to_bytes(8, "little") + (70000).to_bytes(4, "little") + b"\x01" + (64).to_bytes(4, "little") + com.tobytes()
    assert m == S.commitment_message(2 ** 40 + 5, 70000, 1, com) and len(m) == 33 + 64 * 32 and isinstance(m, bytes)
    assert SS.commitment_message(1, 2, 0, com[:1]) == S.commitment_message(1, 2, 0, com[:1]) != SS.commitment_message(1, 2, 1, com[:1])
    for bad in (lambda: SS.commitment_message(1, 2, 2, com), lambda: SS.commitment_message(1, 2, 0, com[:, :31]), lambda: SS.commitment_message(1, 2, 0, com[:0])):
        with pytest.raises(ValueError):
            bad()
    sg = {7: np.arange(128, dtype=np.uint8).reshape(2, 64), 3: np.full((2, 64), 9, np.uint8), 2 ** 31: np.zeros((2, 64), np.uint8)}
    v = SS.view_message(11, sg)
    want = b"rofl-zk/view/v1\0" + (11).to_bytes(8, "little") + (3).to_bytes(4, "little")
    for d in (3, 7, 2 ** 31):                                                       # dealers ascending, whatever the dict's order
        want += d.to_bytes(4, "little") + sg[d][0].tobytes() + sg[d][1].tobytes()
    assert v == want == S.view_message(11, sg) and len(v) == 28 + 3 * 132
    assert SS.view_message(11, {}) == b"rofl-zk/view/v1\0" + (11).to_bytes(8, "little") + bytes(4)
    with pytest.raises(ValueError, match=r"dealer 7\b"):
        SS.view_message(11, {7: np.zeros((1, 64), np.uint8)})


def test_commitment_and_view_helpers_are_one_call_each(dealt, model_device):
    from rofl_project_code_amd.api import secret_sharing as SS
    d = dealt
    sigs = SS.sign_commitments(d["sks"], 9, d["dealers"], d["key_com"], d["self_com"])
    want_refs = [(0, 0), (0, 1), (1, 2), (1, 3), (2, 4), (2, 5), (3, 6), (3, 7)]
    assert model_device == [("sign", 4, 8, want_refs)] and sigs.shape == (4, 2, 64) and sigs.dtype == np.uint8
    for r, dealer in enumerate(d["dealers"]):
        assert sigs[r, 0].tobytes() == S.sign(d["sks"][r], S.commitment_message(9, dealer, 0, d["key_com"][r]))
        assert sigs[r, 1].tobytes() == S.sign(d["sks"][r], S.commitment_message(9, dealer, 1, d["self_com"][r]))
    del model_device[:]
    v = SS.verify_commitment_signatures(d["pks"], 9, d["dealers"], d["key_com"], d["self_com"], sigs)
    assert model_device == [("verify", 4, 8, want_refs)] and v.shape == (4, 2) and not v.any()
    # another round, another dealer index, the rows swapped, a tampered commitment: each named where it is
    assert SS.verify_commitment_signatures(d["pks"], 10, d["dealers"], d["key_com"], d["self_com"], sigs).all()
    assert SS.verify_commitment_signatures(d["pks"], 9, [5, 0, 3, 9], d["key_com"], d["self_com"], sigs).tolist() == [[0, 0], [0, 0], [1, 1], [0, 0]]
    assert SS.verify_commitment_signatures(d["pks"], 9, d["dealers"], d["self_com"], d["key_com"], sigs).all()
    tam = d["self_com"].copy(); tam[1, 2] = d["self_com"][0, 2]
    assert SS.verify_commitment_signatures(d["pks"], 9, d["dealers"], d["key_com"], tam, sigs).tolist() == [[0, 0], [0, 1], [0, 0], [0, 0]]
    with pytest.raises(ValueError):
        SS.sign_commitments(d["sks"][:3], 9, d["dealers"], d["key_com"], d["self_com"])
    with pytest.raises(ValueError):
        SS.verify_commitment_signatures(d["pks"], 9, d["dealers"], d["key_com"], d["self_com"][:3], sigs)
    with pytest.raises(ValueError):
        SS.verify_commitment_signatures(d["pks"], 9, d["dealers"], d["key_com"], d["self_com"], sigs[:, 0])
    # the view round: everybody signs the same bytes; a client that was shown other commitments of dealer 2 signs other bytes and is named
    view = SS.view_message(9, {dealer: sigs[r] for r, dealer in enumerate(d["dealers"])})
    other_sig = S.sign(d["sks"][2], S.commitment_message(9, 2, 1, tam[1]))
    shown = {dealer: sigs[r].copy() for r, dealer in enumerate(d["dealers"])}
    shown[2][1] = np.frombuffer(other_sig, np.uint8)
    views = [view, view, SS.view_message(9, shown), view]
    assert views[2] != view
    del model_device[:]
    vs = S.sign_batch(d["sks"], views)
    got = SS.verify_views(d["pks"], view, vs)
    assert model_device == [("verify", 4, 1, [(0, 0), (1, 0), (2, 0), (3, 0)])] and got.tolist() == [0, 0, 1, 0]


def test_signed_shares_check_signatures_then_delegate(dealt, model_device, monkeypatch):
    from rofl_project_code_amd import api
    P = api.pedersen_ops
    d = dealt
    seen = []

    def verified(*args):
        seen.append(args)
        return ["terms"], [3]

    monkeypatch.setattr(P, "dropout_residual_terms_from_verified_shares", staticmethod(verified))
    surv, dropped = [3, 0, 1], [2]
    key_com = {2: d["key_com"][2]}
    self_com = {i: d["self_com"][i] for i in surv}
    spk = d["pks"]                                                                  # client c signs with key c
    sigs = {2: np.frombuffer(S.sign(d["sks"][2], S.commitment_message(9, 2, 0, key_com[2])), np.uint8)}
    for i in surv:
        sigs[i] = np.frombuffer(S.sign(d["sks"][i], S.commitment_message(9, i, 1, self_com[i])), np.uint8)
    args = (surv, dropped, [1, 2, 4], "KS", "SS", key_com, self_com, "PK", 9)
    assert P.dropout_residual_terms_from_signed_shares(*args, spk, sigs) == (["terms"], [3])
    # ONE verify call over the rows actually used, dropped first, then the survivors ascending; then the verified route with its own arguments
    assert model_device == [("verify", 4, 4, None)]
    assert len(seen) == 1 and seen[0][:5] == args[:5] and seen[0][7:] == ("PK", 9) and set(seen[0][5]) == {2} and set(seen[0][6]) == set(self_com)
    # a missing signature, a signature on the other kind, on another round, by another key: ValueError naming the dealer, nothing delegated
    del seen[:]
    with pytest.raises(ValueError, match=r"client 1\b.*no signature"):
        P.dropout_residual_terms_from_signed_shares(*args, spk, {c: s for c, s in sigs.items() if c != 1})
    wrong_kind = dict(sigs); wrong_kind[2] = np.frombuffer(S.sign(d["sks"][2], S.commitment_message(9, 2, 1, key_com[2])), np.uint8)
    with pytest.raises(ValueError, match=r"client 2\b.*key commitments does not verify"):
        P.dropout_residual_terms_from_signed_shares(*args, spk, wrong_kind)
    with pytest.raises(ValueError, match=r"client 2\b.*key commitments does not verify"):
        P.dropout_residual_terms_from_signed_shares(*args[:8], 10, spk, sigs)
    swapped = spk.copy(); swapped[[1, 3]] = swapped[[3, 1]]
    with pytest.raises(ValueError, match=r"client 1\b.*does not verify"):
        P.dropout_residual_terms_from_signed_shares(*args, swapped, sigs)
    refused = spk.copy(); refused[3] = 0xff
    with pytest.raises(ValueError, match=r"client 3\b.*verdict 2"):
        P.dropout_residual_terms_from_signed_shares(*args, refused, sigs)
    tam = dict(self_com); tam[0] = d["self_com"][1]                                 # commitments swapped after signing
    with pytest.raises(ValueError, match=r"client 0\b.*self-mask commitments does not verify"):
        P.dropout_residual_terms_from_signed_shares(*args[:6], tam, "PK", 9, spk, sigs)
    with pytest.raises(ValueError, match=r"survivor 3\b.*commitments"):
        P.dropout_residual_terms_from_signed_shares(*args[:6], {0: self_com[0], 1: self_com[1]}, "PK", 9, spk, sigs)
    with pytest.raises(ValueError, match=r"client 3\b.*signing key"):
        P.dropout_residual_terms_from_signed_shares(*args, spk[:3], sigs)
    assert seen == []
    # the verified route keeps its signature
    import inspect
    monkeypatch.undo()
    assert list(inspect.signature(P.dropout_residual_terms_from_signed_shares).parameters)[:9] == list(inspect.signature(P.dropout_residual_terms_from_verified_shares).parameters)


def test_new_entry_points_are_exported_and_declared_for_rust(hiplib):
    names = ("rofl_sig_sign", "rofl_sig_verify", "rofl_dbg_host_sig_sign", "rofl_dbg_host_sig_verify")
    for name in names:
        assert hasattr(hiplib, name), name
    hdr = open(os.path.join(ROOT, "include", "rofl_zk.h")).read()
    dbg = open(os.path.join(ROOT, "include", "rofl_zk_debug.h")).read()
    assert all(n + "(" in hdr for n in names[:2]) and all(n + "(" in dbg for n in names[2:]) and "rofl_sig_ref_t" in hdr
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "check_ffi.py")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    ffi = open(os.path.join(ROOT, "integration", "rofl_crypto_overlay", "src", "ffi.rs")).read()
    assert all("pub fn %s(" % n in ffi for n in names[:2]) and "pub struct RoflSigRef" in ffi and "pub mod signatures" in ffi
    import rofl_project_code_amd as R
    assert R.signatures is R.api.signatures
