"""CPU-only checks of the key agreement (rofl_dh_public_keys / rofl_dh_shared): the host route rofl_dbg_host_dh against the Python model of the
definition (tests/dh_model.py), the refused peer keys, symmetry, every parameter check of the two C entry points (they come before the device
is touched), the Python wrappers' own checks, the two pedersen_ops helpers with the device call replaced by the model, and the Rust
declarations.  No call here reaches a GPU."""
import ctypes
import hashlib
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest

import blind_model as B
import dh_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sz = ctypes.c_size_t
L_ORDER = M.L
P_FIELD = 2 ** 255 - 19


class Pair(ctypes.Structure):
    _fields_ = [("own", ctypes.c_uint32), ("peer", ctypes.c_uint32)]


def _host_dh(L, sk, own_pk, peer_pk):
    out, st = ctypes.create_string_buffer(b"\xaa" * 32, 32), ctypes.c_ubyte(99)
    rc = L.rofl_dbg_host_dh(bytes(sk), None if own_pk is None else bytes(own_pk), bytes(peer_pk), out, ctypes.byref(st))
    return rc, out.raw, st.value


def _last_error(L):
    err = ctypes.create_string_buffer(512)
    L.rofl_last_error(err, sz(512))
    return err


@pytest.fixture(scope="module")
def keys():
    """five clients: secret keys (any 32 bytes) and the model's public keys, computed once"""
    rng = np.random.default_rng(20261019)
    sk = M.rand_keys(rng, 5)
    pk = np.frombuffer(b"".join(M.public_key(s) for s in sk), np.uint8).reshape(5, 32).copy()
    return sk, pk


def test_model_products_agree():
    # the oracle's one-term MSM and pyref's double-and-add give the same encodings
    sk = bytes(range(1, 33))
    assert M.public_key(sk, fast=True) == M.public_key(sk, fast=False)
    peer = M.public_key(b"\x07" * 32)
    assert M.shared(sk, peer, fast=True) == M.shared(sk, peer, fast=False)
    assert M.DOM == b"rofl-zk/dh/v1" + bytes(3) and len(M.DOM) == 16


def test_host_route_equals_the_model(hiplib, keys):
    sk, pk = keys
    for a, b in ((0, 1), (1, 0), (2, 4), (3, 3)):
        want = M.shared(sk[a], pk[b])
        assert want[1] == 0
        assert _host_dh(hiplib, sk[a], None, pk[b]) == (0,) + want, (a, b)          # own public key computed
        assert _host_dh(hiplib, sk[a], pk[a], pk[b]) == (0,) + want, (a, b)         # ... and given
    # sk + l is the same secret as sk; l - 1 is the largest one
    k = M.sk_int(sk[0])
    assert k + L_ORDER < 2 ** 256
    assert _host_dh(hiplib, (k + L_ORDER).to_bytes(32, "little"), None, pk[1]) == (0,) + M.shared(k.to_bytes(32, "little"), pk[1])
    assert _host_dh(hiplib, (k + L_ORDER).to_bytes(32, "little"), None, pk[1])[1] == _host_dh(hiplib, k.to_bytes(32, "little"), None, pk[1])[1]
    top = (L_ORDER - 1).to_bytes(32, "little")
    assert _host_dh(hiplib, top, None, pk[2]) == (0,) + M.shared(top, pk[2])
    # the layout, spelled out once: SHAKE256(D || S || lo || hi), lo <= hi as byte strings
    s = M._product(k, pk[1].tobytes(), True)
    lo, hi = sorted([pk[0].tobytes(), pk[1].tobytes()])
    assert _host_dh(hiplib, sk[0], None, pk[1])[1] == hashlib.shake_256(b"rofl-zk/dh/v1\0\0\0" + s + lo + hi).digest(32)


def test_refused_peer_keys(hiplib, keys):
    sk, pk = keys
    neg_s = (P_FIELD - int.from_bytes(pk[1].tobytes(), "little")).to_bytes(32, "little")       # -s of a valid encoding: odd, "negative"
    assert neg_s[0] & 1
    cases = [(b"\xff" * 32, 1), ((P_FIELD + 1).to_bytes(32, "little"), 1), (neg_s, 1), (bytes(32), 2)]
    for enc, status in cases:
        assert M.shared(sk[0], enc) == (bytes(32), status)
        assert _host_dh(hiplib, sk[0], None, enc) == (0, bytes(32), status), enc.hex()


def test_symmetry_all_to_all(hiplib, keys):
    sk, pk = keys
    for a, b in itertools.combinations(range(5), 2):
        ab, ba = _host_dh(hiplib, sk[a], pk[a], pk[b]), _host_dh(hiplib, sk[b], pk[b], pk[a])
        assert ab == ba and ab[0] == 0 and ab[2] == 0 and ab[1] != bytes(32), (a, b)
    secrets = {_host_dh(hiplib, sk[a], pk[a], pk[b])[1] for a, b in itertools.combinations(range(5), 2)}
    assert len(secrets) == 10


def _shared(L, n_own, sk, own_pk, n_peer, pk, n_pairs, pairs, out, st):
    L.rofl_dh_shared.argtypes = [sz, ctypes.c_void_p, ctypes.c_void_p, sz, ctypes.c_void_p, sz, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    p = lambda x: None if x is None else (ctypes.addressof(x) if isinstance(x, ctypes.Array) else x.ctypes.data)      # noqa: E731
    return L.rofl_dh_shared(n_own, p(sk), p(own_pk), n_peer, p(pk), n_pairs, p(pairs), p(out), p(st))


def test_parameter_checks_come_before_the_device(hiplib, keys):
    L = hiplib
    sk, pk = keys
    sk2, pk3 = np.ascontiguousarray(sk[:2]), np.ascontiguousarray(pk[:3])
    out, st = np.zeros((6, 32), np.uint8), np.zeros(6, np.uint8)
    L.rofl_dh_public_keys.argtypes = [sz, ctypes.c_void_p, ctypes.c_void_p]
    # rofl_dh_public_keys
    assert L.rofl_dh_public_keys(2, None, out.ctypes.data) == 11
    assert L.rofl_dh_public_keys(2, sk2.ctypes.data, None) == 11
    assert L.rofl_dh_public_keys((1 << 20) + 1, sk2.ctypes.data, out.ctypes.data) == 11
    for zero in (bytes(32), L_ORDER.to_bytes(32, "little"), (2 * L_ORDER).to_bytes(32, "little")):
        bad = np.frombuffer(sk[0].tobytes() + zero, np.uint8).copy()
        assert L.rofl_dh_public_keys(2, bad.ctypes.data, out.ctypes.data) == 11
    # rofl_dh_shared: null pointers
    assert _shared(L, 2, None, None, 3, pk3, 6, None, out, st) == 11
    assert _shared(L, 2, sk2, None, 3, None, 6, None, out, st) == 11
    assert _shared(L, 2, sk2, None, 3, pk3, 6, None, None, st) == 11
    assert _shared(L, 2, sk2, None, 3, pk3, 6, None, out, None) == 11
    # sizes
    assert _shared(L, (1 << 20) + 1, sk2, None, 3, pk3, 6, None, out, st) == 11
    assert _shared(L, 2, sk2, None, (1 << 20) + 1, pk3, 6, None, out, st) == 11
    assert _shared(L, 1 << 20, sk2, None, 1 << 20, pk3, (1 << 24) + 1, None, out, st) == 11
    assert _shared(L, 2, sk2, None, 3, pk3, 5, None, out, st) == 11                  # all pairs: n_pairs is the product
    assert _shared(L, 2, sk2, None, 3, pk3, 7, None, out, st) == 11
    assert _shared(L, 0, sk2, None, 3, pk3, 1, None, out, st) == 11                  # pairs without keys
    # a pair index out of range
    for own, peer in ((2, 0), (0, 3), (0xffffffff, 0)):
        pairs = (Pair * 2)(Pair(0, 0), Pair(own, peer))
        assert _shared(L, 2, sk2, None, 3, pk3, 2, pairs, out, st) == 11, (own, peer)
    # an own key that is 0 mod l: the text names the index and holds no key bytes
    bad = np.frombuffer(sk[0].tobytes() + L_ORDER.to_bytes(32, "little"), np.uint8).copy()
    assert _shared(L, 2, bad, None, 3, pk3, 6, None, out, st) == 11
    err = _last_error(L)
    text = err.value.decode()
    assert "1" in text and "zero" in text, text
    for secret in (sk[0].tobytes(), L_ORDER.to_bytes(32, "little")):
        assert secret.hex() not in text and secret not in err.raw and secret[:8] not in err.raw
    assert not out.any() and not st.any()
    # the host route refuses a zero key too
    assert _host_dh(L, L_ORDER.to_bytes(32, "little"), None, pk[0])[0] == 11


def test_empty_calls_return_zero_without_a_device(hiplib, keys):
    L = hiplib
    sk, pk = keys
    L.rofl_dh_public_keys.argtypes = [sz, ctypes.c_void_p, ctypes.c_void_p]
    assert L.rofl_dh_public_keys(0, None, None) == 0
    assert _shared(L, 0, None, None, 0, None, 0, None, None, None) == 0
    sk2, pk3 = np.ascontiguousarray(sk[:2]), np.ascontiguousarray(pk[:3])
    assert _shared(L, 2, sk2, None, 3, pk3, 0, (Pair * 1)(), None, None) == 0
    assert _shared(L, 2, sk2, None, 0, None, 0, None, None, None) == 0               # all pairs of nothing


def test_wrappers_own_checks(hiplib, keys):
    from rofl_project_code_amd.api import key_agreement as K, pedersen_ops as P
    sk, pk = keys
    with pytest.raises(ValueError):
        K.public_keys([b"\x01" * 31])
    with pytest.raises(ValueError):
        K.public_keys(np.zeros((2, 31), np.uint8))
    with pytest.raises(ValueError):
        K.shared_secrets(sk[:2], pk[:3], pairs=[(0, 3)])
    with pytest.raises(ValueError):
        K.shared_secrets(sk[:2], pk[:3], pairs=[(2, 0)])
    with pytest.raises(ValueError):
        K.shared_secrets(sk[:2], pk[:3], pairs=[(-1, 0)])
    with pytest.raises(ValueError):
        P.pairwise_peers_from_keys(0, sk[0], pk, 7, clients=[(0, sk[0])])
    with pytest.raises(ValueError):
        P.pairwise_peers_from_keys(5, sk[0], pk, 7)                                   # no such client in the round
    with pytest.raises(ValueError):
        P.pairwise_residual_terms_from_keys([0, 1], {1: sk[1]}, pk, 7)                # both accepted and rejected
    # nothing to compute never reaches the device
    assert K.public_keys([]).shape == (0, 32)
    out, st = K.shared_secrets(sk[:2], pk[:3], pairs=[])
    assert out.shape == (0, 32) and st.shape == (0,)
    assert P.pairwise_residual_terms_from_keys([0, 1, 2], {}, pk, 7) == []
    # a zero key: RoflError 11 from the library's own check
    from rofl_project_code_amd.api import RoflError
    with pytest.raises(RoflError) as e:
        K.public_keys([bytes(32)])
    assert e.value.code == 11


@pytest.fixture()
def model_device(monkeypatch):
    """key_agreement's two device calls replaced by the model: the pedersen_ops helpers above them run without a GPU"""
    from rofl_project_code_amd import api
    calls = []

    def shared_secrets(sk, peer_pks, pairs=None, with_public=False):
        assert not with_public
        calls.append(len(pairs) if pairs is not None else len(sk) * len(peer_pks))
        return M.shared_batch(np.asarray(sk, np.uint8).reshape(-1, 32), np.asarray(peer_pks, np.uint8).reshape(-1, 32), pairs)

    def public_keys(sk):
        sk = np.asarray(sk, np.uint8).reshape(-1, 32)
        return np.frombuffer(b"".join(M.public_key(s) for s in sk), np.uint8).reshape(-1, 32).copy()

    monkeypatch.setattr(api.key_agreement, "shared_secrets", staticmethod(shared_secrets))
    monkeypatch.setattr(api.key_agreement, "public_keys", staticmethod(public_keys))
    return calls


def _model_seeds(sk, pk, round_no):
    """seeds[(i, j)], i < j, as the definition gives them"""
    return {(i, j): B.round_seed(M.shared(sk[i], pk[j], pk[i])[0], round_no) for i, j in itertools.combinations(range(len(sk)), 2)}


def test_peers_from_keys(hiplib, keys, model_device):
    from rofl_project_code_amd.api import pedersen_ops as P
    sk, pk = keys
    seeds = _model_seeds(sk, pk, 7)
    single = []
    for i in range(5):
        peers = P.pairwise_peers_from_keys(i, sk[i], pk, 7)
        assert peers == [(j, seeds[(min(i, j), max(i, j))]) for j in range(5) if j != i], i
        single.append(peers)
    assert model_device == [4] * 5
    # the several-clients form: ONE call, the same lists
    del model_device[:]
    hosted = P.pairwise_peers_from_keys(clients=[(3, sk[3]), (0, sk[0]), (4, sk[4])], public_keys=pk, round_no=7)
    assert model_device == [12]
    assert hosted == [single[3], single[0], single[4]]
    # another round, other seeds
    assert P.pairwise_peers_from_keys(1, sk[1], pk, 8) != single[1]
    # a refused key raises and names the client and the status
    bad = pk.copy(); bad[2] = 0xff
    with pytest.raises(ValueError, match=r"client 2\b.*status 1"):
        P.pairwise_peers_from_keys(0, sk[0], bad, 7)
    bad[2] = 0
    with pytest.raises(ValueError, match=r"client 2\b.*status 2"):
        P.pairwise_peers_from_keys(clients=[(0, sk[0]), (1, sk[1])], public_keys=bad, round_no=7)
    # (the owner's own row is never read: client 2 itself is not stopped by its own bad row)
    assert P.pairwise_peers_from_keys(2, sk[2], bad, 7) == single[2]


def test_residual_terms_from_keys_over_every_accept_set(hiplib, keys, model_device):
    from rofl_project_code_amd.api import pedersen_ops as P
    sk, pk = keys
    seeds = _model_seeds(sk, pk, 7)
    for mask in range(32):
        accepted = [i for i in range(5) if mask >> i & 1]
        rejected = [i for i in range(5) if not mask >> i & 1]
        del model_device[:]
        got = P.pairwise_residual_terms_from_keys(accepted, {j: sk[j] for j in reversed(rejected)}, pk, 7)
        assert got == P.pairwise_residual_terms(accepted, rejected, seeds), mask
        assert len(got) == len(accepted) * len(rejected)
        assert model_device == ([len(accepted) * len(rejected)] if accepted and rejected else [])      # ONE call
    # a wrong revealed key raises and names the client
    with pytest.raises(ValueError, match=r"client 3\b"):
        P.pairwise_residual_terms_from_keys([0, 1, 2], {3: sk[4], 4: sk[4]}, pk, 7)


def test_new_entry_points_are_exported_and_declared_for_rust(hiplib):
    for name in ("rofl_dh_public_keys", "rofl_dh_shared", "rofl_dbg_host_dh"):
        assert hasattr(hiplib, name), name
    hdr = open(os.path.join(ROOT, "include", "rofl_zk.h")).read()
    assert "rofl_dh_public_keys(" in hdr and "rofl_dh_shared(" in hdr and "rofl_dh_pair_t" in hdr
    assert "rofl_dbg_host_dh(" in open(os.path.join(ROOT, "include", "rofl_zk_debug.h")).read()
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "check_ffi.py")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    ffi = open(os.path.join(ROOT, "integration", "rofl_crypto_overlay", "src", "ffi.rs")).read()
    assert "pub fn rofl_dh_public_keys(" in ffi and "pub fn rofl_dh_shared(" in ffi and "pub struct RoflDhPair" in ffi
