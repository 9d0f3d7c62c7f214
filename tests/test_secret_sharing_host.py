"""CPU-only checks of the secret sharing (rofl_shamir_share / rofl_shamir_reconstruct) and of the double-masking helpers: the host route
rofl_dbg_host_shamir_* against the Python model of the definition (tests/shamir_model.py), reconstruction from every threshold subset, every
parameter check of the two C entry points (they come before the device is touched), the Python wrappers' own checks, the Rust declarations,
the pedersen_ops helpers with the device calls replaced by the model, and the recovery identity itself in the model.  No call here reaches a
GPU."""
import ctypes
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest

import blind_model as B
import dh_model as D
import shamir_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sz = ctypes.c_size_t
L_ORDER = M.L
SHARE_ARGS = [sz, ctypes.c_void_p, ctypes.c_void_p, sz, sz, ctypes.c_void_p, ctypes.c_void_p]
RECON_ARGS = [sz, sz, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]


def _p(x):
    return None if x is None else x.ctypes.data


def _share(L, name, secrets, seeds, t, n_shares, xs, out, n=None):
    fn = getattr(L, name)
    fn.argtypes = SHARE_ARGS
    return fn(len(secrets) if n is None else n, _p(secrets), _p(seeds), t, n_shares, _p(xs), _p(out))


def _recon(L, name, n, n_shares, xs, shares, out):
    fn = getattr(L, name)
    fn.argtypes = RECON_ARGS
    return fn(n, n_shares, _p(xs), _p(shares), _p(out))


def _last_error(L):
    err = ctypes.create_string_buffer(512)
    L.rofl_last_error(err, sz(512))
    return err


def _b32(v):
    return np.frombuffer(int(v).to_bytes(32, "little"), np.uint8)


@pytest.fixture(scope="module")
def edge_secrets():
    """0, 1, l - 1, l (= 0), s + l, 2^256 - 1, and their coefficient seeds"""
    rng = np.random.default_rng(20261019)
    s = int.from_bytes(rng.bytes(31), "little")
    assert s + L_ORDER < 2 ** 256
    sec = np.stack([_b32(v) for v in (0, 1, L_ORDER - 1, L_ORDER, s + L_ORDER, 2 ** 256 - 1)]).copy()
    seeds = rng.integers(0, 256, size=(len(sec), 32), dtype=np.uint8)
    return sec, seeds


def test_model_is_the_definition():
    # the label is sixteen bytes, coefficient k is scalar k - 1 of the stream, and the stream is the blinding stream under another label
    import hashlib
    import struct
    assert M.LABEL == b"rofl-zk/share/v1" and len(M.LABEL) == 16
    seed = bytes(range(32))
    a = M.coefficients(seed, 4)
    blk0 = hashlib.shake_256(M.LABEL + seed + struct.pack("<Q", 0)).digest(128)
    blk1 = hashlib.shake_256(M.LABEL + seed + struct.pack("<Q", 1)).digest(128)
    assert a == [int.from_bytes(blk0[:64], "little") % L_ORDER, int.from_bytes(blk0[64:], "little") % L_ORDER, int.from_bytes(blk1[:64], "little") % L_ORDER]
    assert a[0] != B.stream_int(seed, 0)
    assert M.coefficients(seed, 1) == []
    # f(x) by hand at t = 3
    s, (a1, a2) = 5, M.coefficients(seed, 3)
    assert M.share_ints(_b32(s), seed, 3, [7]) == [(s + a1 * 7 + a2 * 49) % L_ORDER]
    assert M.self_mask_seed(_b32(3 + L_ORDER), 9) == hashlib.sha3_256(b"rofl-zk/blind/v1/self" + (3).to_bytes(32, "little") + struct.pack("<Q", 9)).digest()


@pytest.mark.parametrize("t", [1, 2, 3, 40])
def test_host_share_equals_the_model(hiplib, edge_secrets, t):
    sec, seeds = edge_secrets
    n = max(t, 5)
    want = M.share(sec, seeds, t, n)
    out = np.full((len(sec), n, 32), 0xaa, np.uint8)
    assert _share(hiplib, "rofl_dbg_host_shamir_share", sec, seeds, t, n, None, out) == 0
    assert (out == want).all()
    if t == 1:      # the reduced secret at every point
        assert B.to_ints(out[:, 0]) == [v % L_ORDER for v in B.to_ints(sec)]
        assert B.to_ints(out[3, 2:3]) == [0] and B.to_ints(out[4, :1]) == [B.to_ints(sec[4:5])[0] - L_ORDER]
    # listed points, the largest uint32 among them, in no order
    xs = np.array([2 ** 32 - 1, 3, 1, 70000, 2 ** 31] + list(range(100, 100 + n - 5)), dtype=np.uint32)
    want = M.share(sec, seeds, t, n, xs)
    out[...] = 0xaa
    assert _share(hiplib, "rofl_dbg_host_shamir_share", sec, seeds, t, n, xs, out) == 0
    assert (out == want).all()
    # a subset of the points: those columns
    sub = np.ascontiguousarray(xs[[4, 0]]) if t <= 2 else np.ascontiguousarray(xs[:t][::-1])
    part = np.zeros((len(sec), len(sub), 32), np.uint8)
    assert _share(hiplib, "rofl_dbg_host_shamir_share", sec, seeds, t, len(sub), sub, part) == 0
    assert (part == M.share(sec, seeds, t, len(sub), sub)).all()
    # reconstruction of what was shared: the model and the host route agree and return the reduced secrets
    back = np.full((len(sec), 32), 0xaa, np.uint8)
    assert _recon(hiplib, "rofl_dbg_host_shamir_reconstruct", len(sec), n, xs, out, back) == 0
    assert (back == M.reconstruct(xs, out)).all()
    assert B.to_ints(back) == [v % L_ORDER for v in B.to_ints(sec)]


def test_reconstruction_from_every_threshold_subset(hiplib):
    rng = np.random.default_rng(4)
    sec, seeds = rng.integers(0, 256, size=(2, 32), dtype=np.uint8), rng.integers(0, 256, size=(2, 32), dtype=np.uint8)
    xs = np.array([1, 2, 3, 4, 5, 6], np.uint32)
    sh = M.share(sec, seeds, 4, 6)
    want = B.to_arr(B.to_ints(sec))
    back = np.zeros((2, 32), np.uint8)
    for sub in list(itertools.combinations(range(6), 4)) + [tuple(range(6)), (5, 0, 3, 1, 2)]:
        idx = list(sub)
        x, s = np.ascontiguousarray(xs[idx]), np.ascontiguousarray(sh[:, idx])
        back[...] = 0xaa
        assert _recon(hiplib, "rofl_dbg_host_shamir_reconstruct", 2, len(idx), x, s, back) == 0
        assert (back == want).all(), sub
        assert (M.reconstruct(x, s) == want).all(), sub
    # three shares of a threshold-4 sharing reconstruct something else, without an error: the sharing is not verifiable
    assert _recon(hiplib, "rofl_dbg_host_shamir_reconstruct", 2, 3, np.ascontiguousarray(xs[:3]), np.ascontiguousarray(sh[:, :3]), back) == 0
    assert (back != want).any(axis=1).all()
    # shares that are not canonical are reduced
    big = sh.copy()
    v = B.to_ints(sh[0, 2:3])[0]
    assert v + L_ORDER < 2 ** 256
    big[0, 2] = _b32(v + L_ORDER)
    assert _recon(hiplib, "rofl_dbg_host_shamir_reconstruct", 2, 6, xs, big, back) == 0
    assert (back == want).all()
    assert (M.reconstruct(xs, big) == want).all()


def test_parameter_checks_come_before_the_device(hiplib, edge_secrets):
    L = hiplib
    sec, seeds = edge_secrets
    sec, seeds = np.ascontiguousarray(sec[:3]), np.ascontiguousarray(seeds[:3])
    out = np.zeros((3, 4, 32), np.uint8)
    xs = np.array([5, 9, 2, 7], np.uint32)
    for name in ("rofl_shamir_share", "rofl_dbg_host_shamir_share"):
        bad = [
            ((None, seeds, 2, 4, None, out), "parameter"), ((sec, None, 2, 4, None, out), "parameter"), ((sec, seeds, 2, 4, None, None), "parameter"),
            ((sec, seeds, 0, 4, None, out), "threshold"), ((sec, seeds, 5, 4, None, out), "threshold"),
            ((sec, seeds, 65537, 1 << 17, None, out), "65536"),
            ((sec, seeds, 2, 0, None, out), "without shares"),
            ((sec, seeds, 2, (1 << 20) + 1, None, out), "2^20"),
            ((sec, seeds, 2, 4, np.array([5, 0, 2, 7], np.uint32), out), "point 1 is zero"),
            ((sec, seeds, 2, 4, np.array([5, 9, 2, 9], np.uint32), out), "points 1 and 3 are equal"),
        ]
        for args, text in bad:
            assert _share(L, name, *args, n=3) == 11, (name, text)
            assert text in _last_error(L).value.decode(), (name, text)
        assert _share(L, name, sec, seeds, 2, 4, None, out, n=65536) == 11
        assert "65535" in _last_error(L).value.decode()
        assert _share(L, name, sec, seeds, 2, 1 << 20, None, out, n=17) == 11              # 17 x 2^20 shares
        assert "2^24 shares" in _last_error(L).value.decode()
        # (n_secrets x (threshold - 1) > 2^24 cannot be reached past the check before it: threshold - 1 < n_shares)
        assert not out.any()
        # an empty call returns 0 whatever else it is handed
        assert _share(L, name, None, None, 0, 0, None, None, n=0) == 0
    sh = np.zeros((3, 4, 32), np.uint8)
    back = np.zeros((3, 32), np.uint8)
    for name in ("rofl_shamir_reconstruct", "rofl_dbg_host_shamir_reconstruct"):
        bad = [
            ((3, 4, None, sh, back), "parameter"), ((3, 4, xs, None, back), "parameter"), ((3, 4, xs, sh, None), "parameter"),
            ((3, 0, xs, sh, back), "without shares"), ((65536, 4, xs, sh, back), "65535"), ((3, 65537, xs, sh, back), "65536"),
            ((257, 65536, xs, sh, back), "2^24 shares"),
            ((3, 4, np.array([5, 9, 0, 7], np.uint32), sh, back), "point 2 is zero"),
            ((3, 4, np.array([7, 9, 2, 7], np.uint32), sh, back), "points 0 and 3 are equal"),
        ]
        for args, text in bad:
            assert _recon(L, name, *args) == 11, (name, text)
            assert text in _last_error(L).value.decode(), (name, text)
        assert not back.any()
        assert _recon(L, name, 0, 0, None, None, None) == 0
    # an error text holds no secret, seed or share bytes
    secret = np.ascontiguousarray(np.tile(np.arange(1, 33, dtype=np.uint8), (3, 1)))
    assert _share(L, "rofl_shamir_share", secret, secret, 2, 4, np.array([5, 9, 2, 9], np.uint32), out, n=3) == 11
    err = _last_error(L)
    assert secret[0].tobytes() not in err.raw and secret[0, :8].tobytes() not in err.raw and secret[0].tobytes().hex() not in err.value.decode()


def test_wrappers_own_checks(hiplib):
    from rofl_project_code_amd.api import secret_sharing as S, pedersen_ops as P, RoflError
    sec = np.zeros((2, 32), np.uint8)
    with pytest.raises(ValueError):
        S.share(np.zeros((2, 31), np.uint8), sec, 2, 3)
    with pytest.raises(ValueError):
        S.share(sec, sec[:1], 2, 3)                                         # one seed per secret
    with pytest.raises(ValueError):
        S.share(sec, sec, 0, 3)
    with pytest.raises(ValueError):
        S.share(sec, sec, 4, 3)
    for xs in ([1, 2], [1, 2, 0], [1, 2, 2], [1, 2, 2 ** 32], [1.0, 2.0, 3.0], [[1, 2, 3]]):
        with pytest.raises(ValueError):
            S.share(sec, sec, 2, 3, xs=xs)
    with pytest.raises(ValueError):
        S.reconstruct([1, 2, 3], np.zeros((2, 2, 32), np.uint8))
    with pytest.raises(ValueError):
        S.reconstruct([1, 1], np.zeros((2, 2, 32), np.uint8))
    with pytest.raises(ValueError):
        S.reconstruct([], np.zeros((2, 0, 32), np.uint8))
    with pytest.raises(ValueError):
        P.self_mask_seed(b"\x01" * 31, 0)
    # nothing to compute never reaches the device
    assert S.share(sec[:0], sec[:0], 2, 3).shape == (0, 3, 32)
    assert S.reconstruct([1, 2], np.zeros((0, 2, 32), np.uint8)).shape == (0, 32)
    # the library's own check, through the wrapper
    with pytest.raises(RoflError) as e:
        S.share(np.zeros((65536, 32), np.uint8), np.zeros((65536, 32), np.uint8), 1, 1)
    assert e.value.code == 11
    assert P.self_mask_seed(_b32(L_ORDER + 5).tobytes(), 3) == M.self_mask_seed(_b32(5), 3) != M.self_mask_seed(_b32(5), 4)


def test_new_entry_points_are_exported_and_declared_for_rust(hiplib):
    names = ("rofl_shamir_share", "rofl_shamir_reconstruct", "rofl_dbg_host_shamir_share", "rofl_dbg_host_shamir_reconstruct")
    for name in names:
        assert hasattr(hiplib, name), name
    hdr = open(os.path.join(ROOT, "include", "rofl_zk.h")).read()
    dbg = open(os.path.join(ROOT, "include", "rofl_zk_debug.h")).read()
    assert all(n + "(" in hdr for n in names[:2]) and all(n + "(" in dbg for n in names[2:])
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "check_ffi.py")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    ffi = open(os.path.join(ROOT, "integration", "rofl_crypto_overlay", "src", "ffi.rs")).read()
    assert all("pub fn %s(" % n in ffi for n in names)
    import rofl_project_code_amd as R
    assert R.secret_sharing is R.api.secret_sharing


# ---------------------------------------------------------------- the helpers above the device calls, on the model
@pytest.fixture(scope="module")
def round5():
    """five clients of round 7: DH keys, public keys, self-mask secrets, and the pairwise seeds the definition gives"""
    rng = np.random.default_rng(20261020)
    sk = D.rand_keys(rng, 5)
    pk = np.frombuffer(b"".join(D.public_key(s) for s in sk), np.uint8).reshape(5, 32).copy()
    b = rng.integers(0, 256, size=(5, 32), dtype=np.uint8)
    seeds = {(i, j): B.round_seed(D.shared(sk[i], pk[j], pk[i])[0], 7) for i, j in itertools.combinations(range(5), 2)}
    return sk, pk, b, seeds


@pytest.fixture()
def model_device(monkeypatch):
    """the device calls under the helpers replaced by the models; the list records the reconstruct calls (secrets per call)"""
    from rofl_project_code_amd import api
    calls = []

    def shared_secrets(sk, peer_pks, pairs=None, with_public=False):
        return D.shared_batch(np.asarray(sk, np.uint8).reshape(-1, 32), np.asarray(peer_pks, np.uint8).reshape(-1, 32), pairs)

    def public_keys(sk):
        return np.frombuffer(b"".join(D.public_key(s) for s in np.asarray(sk, np.uint8).reshape(-1, 32)), np.uint8).reshape(-1, 32).copy()

    def reconstruct(xs, shares):
        calls.append(len(shares))
        return M.reconstruct(xs, shares).copy()

    monkeypatch.setattr(api.key_agreement, "shared_secrets", staticmethod(shared_secrets))
    monkeypatch.setattr(api.key_agreement, "public_keys", staticmethod(public_keys))
    monkeypatch.setattr(api.secret_sharing, "reconstruct", staticmethod(reconstruct))
    return calls


def test_dropout_residual_terms(hiplib, round5, model_device):
    from rofl_project_code_amd.api import pedersen_ops as P
    sk, pk, b, _ = round5
    for surv in ([0, 1, 3, 4], [4, 2, 0], [0, 1, 2, 3, 4]):
        dropped = [j for j in range(5) if j not in surv]
        got = P.dropout_residual_terms(surv, {j: sk[j].tobytes() for j in dropped}, {i: b[i].tobytes() for i in surv}, pk, 7)
        want = P.pairwise_residual_terms_from_keys(surv, {j: sk[j] for j in dropped}, pk, 7) + [(M.self_mask_seed(b[i], 7), 1) for i in sorted(surv)]
        assert got == want, surv
        assert len(got) == len(surv) * len(dropped) + len(surv)
    # the three refusals name the client
    with pytest.raises(ValueError, match=r"client 2\b"):
        P.dropout_residual_terms([0, 1, 3, 4], {2: sk[2]}, {i: b[i] for i in (0, 1, 2, 3, 4)}, pk, 7)      # both secrets of client 2
    with pytest.raises(ValueError, match=r"survivor 3\b"):
        P.dropout_residual_terms([0, 1, 3, 4], {2: sk[2]}, {i: b[i] for i in (0, 1, 4)}, pk, 7)
    with pytest.raises(ValueError, match=r"client 1\b"):
        P.dropout_residual_terms([0, 1, 3, 4], {2: sk[2], 1: sk[1]}, {i: b[i] for i in (0, 3, 4)}, pk, 7)
    # a wrong key is caught by the public-key check underneath
    with pytest.raises(ValueError, match=r"client 2\b"):
        P.dropout_residual_terms([0, 1, 3, 4], {2: sk[3]}, {i: b[i] for i in (0, 1, 3, 4)}, pk, 7)


def test_dropout_residual_terms_from_shares(hiplib, round5, model_device):
    from rofl_project_code_amd.api import pedersen_ops as P
    sk, pk, b, _ = round5
    rng = np.random.default_rng(5)
    cs = rng.integers(0, 256, size=(10, 32), dtype=np.uint8)
    key_sh, self_sh = M.share(sk, cs[:5], 3, 5), M.share(b, cs[5:], 3, 5)          # [client, holder, 32]
    surv, dropped = [0, 1, 3, 4], [2]
    holders = [4, 0, 3]                                                               # three survivors answer
    xs = [h + 1 for h in holders]
    got = P.dropout_residual_terms_from_shares(surv, dropped, xs, {j: key_sh[j, holders] for j in dropped}, {i: self_sh[i, holders] for i in surv}, pk, 7)
    assert model_device == [5]                                                        # ONE reconstruct call: one key, four self secrets
    # (the reconstructed secrets are the reduced ones: the same key, the same seeds)
    assert got == P.dropout_residual_terms(surv, {2: sk[2]}, {i: b[i] for i in surv}, pk, 7)
    # a wrong key share: the public-key check names the dropped client; a wrong self share gives other terms, no error
    bad = key_sh[2, holders].copy(); bad[1, 0] ^= 1
    with pytest.raises(ValueError, match=r"client 2\b"):
        P.dropout_residual_terms_from_shares(surv, dropped, xs, {2: bad}, {i: self_sh[i, holders] for i in surv}, pk, 7)
    bad = self_sh[0, holders].copy(); bad[2, 31] ^= 1
    other = P.dropout_residual_terms_from_shares(surv, dropped, xs, {2: key_sh[2, holders]}, {**{i: self_sh[i, holders] for i in surv}, 0: bad}, pk, 7)
    assert other[:4] == got[:4] and other[4] != got[4] and other[5:] == got[5:]
    # client 2 in both sets, missing shares, a wrong shape
    with pytest.raises(ValueError, match=r"client 2\b"):
        P.dropout_residual_terms_from_shares(surv, dropped, xs, {2: key_sh[2, holders]}, {i: self_sh[i, holders] for i in surv + [2]}, pk, 7)
    with pytest.raises(ValueError, match=r"client 2\b"):
        P.dropout_residual_terms_from_shares(surv + [2], dropped, xs, {2: key_sh[2, holders]}, {i: self_sh[i, holders] for i in surv}, pk, 7)
    with pytest.raises(ValueError, match=r"client 2\b"):
        P.dropout_residual_terms_from_shares(surv, dropped, xs, {}, {i: self_sh[i, holders] for i in surv}, pk, 7)
    with pytest.raises(ValueError, match=r"survivor 3\b"):
        P.dropout_residual_terms_from_shares(surv, dropped, xs, {2: key_sh[2, holders]}, {i: self_sh[i, holders] for i in (0, 1, 4)}, pk, 7)
    with pytest.raises(ValueError, match=r"client 1\b"):
        P.dropout_residual_terms_from_shares(surv, dropped, xs, {2: key_sh[2, holders]}, {**{i: self_sh[i, holders] for i in surv}, 1: self_sh[1, :2]}, pk, 7)


def test_double_masked_terms_are_the_pairwise_terms_plus_one(hiplib, round5, monkeypatch):
    from rofl_project_code_amd import api
    P = api.pedersen_ops
    _, _, b, seeds = round5
    seen = []
    monkeypatch.setattr(P, "blinding_vecs", staticmethod(lambda term_lists, d, first=0, out=None: seen.append((term_lists, d, first, out)) or np.zeros((len(term_lists), d, 32), np.uint8)))
    peers = {i: [(j, seeds[(min(i, j), max(i, j))]) for j in range(5) if j != i] for i in range(5)}
    P.double_masked_blinding_vec(1, peers[1], b[1], 7, 9, first=4)
    assert seen.pop() == ([P._pairwise_terms(1, peers[1]) + [(M.self_mask_seed(b[1], 7), 1)]], 9, 4, None)
    P.double_masked_blinding_vecs([(3, peers[3], b[3]), (0, peers[0], b[0])], 7, 9)
    assert seen.pop() == ([P._pairwise_terms(i, peers[i]) + [(M.self_mask_seed(b[i], 7), 1)] for i in (3, 0)], 9, 0, None)      # ONE call
    P.pairwise_blinding_vec(1, peers[1], 9)
    assert seen.pop() == ([P._pairwise_terms(1, peers[1])], 9, 0, None)               # the pairwise form is what it was


def test_recovery_identity_over_every_survivor_set(hiplib, round5, model_device):
    """model only: the residual terms of a survivor set combine to the sum of the survivors' double-masked vectors"""
    from rofl_project_code_amd.api import pedersen_ops as P
    sk, pk, b, seeds = round5
    d = 3
    vec = []
    for i in range(5):
        terms = [(seeds[(min(i, j), max(i, j))], 1 if i < j else -1) for j in range(5) if j != i] + [(M.self_mask_seed(b[i], 7), 1)]
        vec.append(B.to_ints(B.combine(terms, d)))
    n_sets = 0
    for size in (3, 4, 5):
        for surv in itertools.combinations(range(5), size):
            dropped = [j for j in range(5) if j not in surv]
            terms = P.dropout_residual_terms(list(surv), {j: sk[j] for j in dropped}, {i: b[i] for i in surv}, pk, 7)
            want = [sum(vec[i][k] for i in surv) % L_ORDER for k in range(d)]
            assert B.to_ints(B.combine(terms, d)) == want, surv
            n_sets += 1
    assert n_sets == 16
