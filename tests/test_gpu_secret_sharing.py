"""Secret sharing on the device (rofl_shamir_share / rofl_shamir_reconstruct: k_shamir_coeffs, k_shamir_eval, k_shamir_weights,
k_shamir_combine) and one double-masked round that loses an honest client.  Every comparison is of bytes against the Python model
(tests/shamir_model.py, tests/blind_model.py, tests/dh_model.py); no tolerance is involved.

Sizes: a block is 256 threads and serves one secret, so n_shares in {1, 255, 256, 257, 600} is one lane, a block short of one, a full one,
a crossing, and several blocks with a ragged tail.  k_shamir_eval stages its coefficients in LDS in tiles of 256 (SHAMIR_TILE in
csrc/kernels.hpp): thresholds 256, 257 and 513 have 255, 256 and 512 coefficients -- a tile short of one, one full tile, two full tiles;
k_shamir_weights stages the points in the same tiles, crossed by n_shares = 257 and 600."""
import ctypes
import itertools

import numpy as np
import pytest

import blind_model as B
import dh_model as D
import orc
import shamir_model as M

pytestmark = pytest.mark.gpu
FP = (32, 7)
ELL = M.L
TILE = 256
ROUND_NO = 7


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


def _seeds(rng, n):
    return rng.integers(0, 256, size=(n, 32), dtype=np.uint8)


def _mixed_secrets(rng):
    """three secrets: a random canonical one, one given as s + l, and 2^256 - 1"""
    s = int.from_bytes(rng.bytes(31), "little")
    return np.stack([orc.rand_scalars(rng, 1)[0], _b32(s + ELL), _b32(2 ** 256 - 1)]).copy()


# ---------------------------------------------------------------- share
@pytest.mark.parametrize("n_shares,t", [(n, t) for n in (1, 255, 256, 257, 600) for t in (1, 2, 3) if t <= n])
def test_share_block_sizes(R, n_shares, t):
    rng = np.random.default_rng(1000 * n_shares + t)
    sec, seeds = _mixed_secrets(rng), _seeds(rng, 3)
    got = R.secret_sharing.share(sec, seeds, t, n_shares)
    assert got.shape == (3, n_shares, 32) and got.dtype == np.uint8
    assert got.tobytes() == M.share(sec, seeds, t, n_shares).tobytes()
    if t == 1:
        assert B.to_ints(got[:, -1]) == [v % ELL for v in B.to_ints(sec)]


@pytest.mark.parametrize("t", [TILE, TILE + 1, 2 * TILE + 1])
def test_share_thresholds_across_the_coefficient_tile(R, t):
    """the tile of k_shamir_eval is 256 coefficients: t - 1 = 255, 256, 512"""
    n_shares = max(257, t)
    rng = np.random.default_rng(t)
    sec, seeds = _mixed_secrets(rng)[:2], _seeds(rng, 2)
    got = R.secret_sharing.share(sec, seeds, t, n_shares)
    assert got.tobytes() == M.share(sec, seeds, t, n_shares).tobytes()


@pytest.mark.parametrize("family", ["all_equal", "minus_one", "random", "small", "top_range", "two_pow_252"])
def test_share_extreme_secrets(R, family):
    rng = np.random.default_rng(31)
    sec = orc.extreme_scalar_cases(rng, 3)[family]
    seeds = _seeds(rng, 3)
    for n in (1, 3):
        got = R.secret_sharing.share(sec[:n], seeds[:n], 3, 257)
        assert got.tobytes() == M.share(sec[:n], seeds[:n], 3, 257).tobytes(), n
    # (one secret of a call of three is that secret's call of one: the rows do not depend on their neighbours)
    assert got[0].tobytes() == R.secret_sharing.share(sec[:1], seeds[:1], 3, 257)[0].tobytes()


def test_share_a_subset_of_the_points_is_those_columns(R):
    rng = np.random.default_rng(8)
    sec, seeds = _mixed_secrets(rng), _seeds(rng, 3)
    whole = R.secret_sharing.share(sec, seeds, 5, 600)
    pick = [599, 0, 256, 255, 300, 17, 4]                       # positions, in no order; point = position + 1
    part = R.secret_sharing.share(sec, seeds, 5, len(pick), xs=[p + 1 for p in pick])
    assert part.tobytes() == np.ascontiguousarray(whole[:, pick]).tobytes()
    # listed points that are no client numbers, the largest uint32 among them
    xs = [2 ** 32 - 1, 1, 2 ** 31, 65537, 99] + list(range(1000, 1000 + 252))
    got = R.secret_sharing.share(sec, seeds, 5, len(xs), xs=xs)
    assert got.tobytes() == M.share(sec, seeds, 5, len(xs), xs).tobytes()


def _dbg(R, name, argtypes, *args):
    fn = getattr(R.api.lib(), name)
    fn.argtypes = argtypes
    return fn(*args)


def test_device_route_equals_host_route(R):
    sz, vp = ctypes.c_size_t, ctypes.c_void_p
    rng = np.random.default_rng(9)
    sec, seeds = _mixed_secrets(rng), _seeds(rng, 3)
    xs = np.array([7, 2 ** 32 - 1, 3, 260, 12, 1, 99, 4096, 5], np.uint32)
    dev = R.secret_sharing.share(sec, seeds, 4, 9, xs=xs)
    host = np.zeros_like(dev)
    assert _dbg(R, "rofl_dbg_host_shamir_share", [sz, vp, vp, sz, sz, vp, vp], 3, sec.ctypes.data, seeds.ctypes.data, 4, 9, xs.ctypes.data, host.ctypes.data) == 0
    assert dev.tobytes() == host.tobytes()
    back_dev = R.secret_sharing.reconstruct(xs, dev)
    back_host = np.zeros((3, 32), np.uint8)
    assert _dbg(R, "rofl_dbg_host_shamir_reconstruct", [sz, sz, vp, vp, vp], 3, 9, xs.ctypes.data, host.ctypes.data, back_host.ctypes.data) == 0
    assert back_dev.tobytes() == back_host.tobytes() == B.to_arr(B.to_ints(sec)).tobytes()


# ---------------------------------------------------------------- reconstruct
@pytest.fixture(scope="module")
def shared600():
    """257 secrets shared at threshold 3 over the points 1 .. 600 by the model, computed once and never changed"""
    rng = np.random.default_rng(600)
    sec = np.concatenate([_mixed_secrets(rng), orc.rand_scalars(rng, 254)])
    seeds = _seeds(rng, 257)
    sh = M.share(sec, seeds, 3, 600)
    sh.setflags(write=False)
    return B.to_arr(B.to_ints(sec)), sh


@pytest.mark.parametrize("n_secrets", [1, 3, 257])
@pytest.mark.parametrize("n_shares", [1, 2, 255, 256, 257, 600])
def test_reconstruct_block_sizes(R, shared600, n_shares, n_secrets):
    """the first n_shares shares of a threshold-3 sharing: from 3 on they give the secret (more shares than the threshold included), below
    they give what the definition gives -- the model's bytes either way"""
    want_secret, sh = shared600
    xs = list(range(1, n_shares + 1))
    part = np.ascontiguousarray(sh[:n_secrets, :n_shares])
    got = R.secret_sharing.reconstruct(xs, part)
    assert got.shape == (n_secrets, 32)
    assert got.tobytes() == M.reconstruct(xs, part).tobytes()
    if n_shares >= 3:
        assert got.tobytes() == want_secret[:n_secrets].tobytes()


def test_reconstruct_shuffled_and_odd_points(R, shared600):
    want_secret, sh = shared600
    rng = np.random.default_rng(12)
    pick = rng.permutation(600)[:300]
    got = R.secret_sharing.reconstruct(pick + 1, np.ascontiguousarray(sh[:3, pick]))
    assert got.tobytes() == want_secret[:3].tobytes()
    # points that are no client numbers, the largest uint32 first; a share given as share + l is the same share
    xs = [2 ** 32 - 1, 5, 2 ** 31, 1, 65537, 2 ** 32 - 2]
    sec, seeds = _mixed_secrets(rng), _seeds(rng, 3)
    sh6 = M.share(sec, seeds, 4, 6, xs)
    want = B.to_arr(B.to_ints(sec)).tobytes()
    assert R.secret_sharing.reconstruct(xs, sh6).tobytes() == want == M.reconstruct(xs, sh6).tobytes()
    big = sh6.copy()
    v = min(B.to_ints(sh6[1]))
    j = B.to_ints(sh6[1]).index(v)
    assert v + ELL < 2 ** 256
    big[1, j] = _b32(v + ELL)
    assert R.secret_sharing.reconstruct(xs, big).tobytes() == want
    # every threshold subset, and a wrong share gives another secret without an error
    for sub in itertools.combinations(range(6), 4):
        idx = list(sub)
        assert R.secret_sharing.reconstruct([xs[i] for i in idx], np.ascontiguousarray(sh6[:, idx])).tobytes() == want, sub
    bad = sh6.copy(); bad[0, 3, 0] ^= 1
    got = R.secret_sharing.reconstruct(xs, bad)
    assert got[0].tobytes() != want[:32] and got[1:].tobytes() == want[32:]
    assert got.tobytes() == M.reconstruct(xs, bad).tobytes()


@pytest.mark.parametrize("t,n_shares", [(1, 1), (2, 5), (256, 257), (257, 257), (300, 600)])
def test_reconstruct_of_share_is_the_identity(R, t, n_shares):
    rng = np.random.default_rng(77 + t)
    sec, seeds = _mixed_secrets(rng), _seeds(rng, 3)
    sh = R.secret_sharing.share(sec, seeds, t, n_shares)
    want = B.to_arr(B.to_ints(sec)).tobytes()
    assert R.secret_sharing.reconstruct(list(range(1, n_shares + 1)), sh).tobytes() == want
    pick = rng.permutation(n_shares)[:t]                          # exactly the threshold, any t of them
    assert R.secret_sharing.reconstruct(pick + 1, np.ascontiguousarray(sh[:, pick])).tobytes() == want


# ---------------------------------------------------------------- one round end to end
N, D_DIM, THRESHOLD = 6, 257, 4
GONE = 2
SURVIVORS = [0, 1, 3, 4, 5]
HOLDERS = [0, 1, 3, 5]                                            # the survivors that answer: the threshold, no more
TABLE, BITS = 1 << 15, 16


def _value_scalars():
    tab = {}
    for k in range(-128, 128):
        rc, s = orc.f32_to_scalar(k / 128.0, *FP)
        assert rc == 0
        tab[k] = s.copy()
    return tab


@pytest.fixture(scope="module")
def dropout_round(R):
    """six clients, d = 257: keys and self secrets random, every client shares both secrets with all six at threshold 4 (the device calls),
    double-masked ElGamal records from the oracle's commitments; client 2 never submits.  Built once, never changed."""
    P, K, S = R.pedersen_ops, R.key_agreement, R.secret_sharing
    rng = np.random.default_rng(20261021)
    sk, b = D.rand_keys(rng, N), rng.integers(0, 256, size=(N, 32), dtype=np.uint8)
    pk = K.public_keys(sk)
    peers = P.pairwise_peers_from_keys(clients=[(i, sk[i]) for i in range(N)], public_keys=pk, round_no=ROUND_NO)
    bl = P.double_masked_blinding_vecs([(i, peers[i], b[i]) for i in range(N)], ROUND_NO, D_DIM)
    # the model's vectors: pairwise seeds from the definition of the key agreement, the self-mask seed from the definition above
    seeds = {(i, j): B.round_seed(D.shared(sk[i], pk[j], pk[i])[0], ROUND_NO) for i, j in itertools.combinations(range(N), 2)}
    for i in range(N):
        terms = [(seeds[(min(i, j), max(i, j))], 1 if i < j else -1) for j in range(N) if j != i] + [(M.self_mask_seed(b[i], ROUND_NO), 1)]
        assert bl[i].tobytes() == B.combine(terms, D_DIM).tobytes(), i
    cs = _seeds(rng, 2 * N)
    key_sh, self_sh = S.share(sk, cs[:N], THRESHOLD, N), S.share(b, cs[N:], THRESHOLD, N)      # [owner, holder, 32]
    assert key_sh.tobytes() == M.share(sk, cs[:N], THRESHOLD, N).tobytes() and self_sh.tobytes() == M.share(b, cs[N:], THRESHOLD, N).tobytes()
    tab = _value_scalars()
    ks = [rng.integers(-20, 21, size=D_DIM) for _ in range(N)]
    recs = []
    for i in range(N):
        x = np.stack([tab[int(k)] for k in ks[i]])
        recs.append(np.ascontiguousarray(np.concatenate([orc.commit_vec(x, bl[i]), orc.commit_vec(bl[i], None)], axis=1)))
    want = np.sum(np.stack([(ks[i] / 128.0).astype(np.float32) for i in SURVIVORS]).astype(np.float64), axis=0).astype(np.float32)
    for a in (pk, key_sh, self_sh):
        a.setflags(write=False)
    return dict(pk=pk, key_sh=key_sh, self_sh=self_sh, recs=recs, want=want.tobytes(), xs=[h + 1 for h in HOLDERS])


def _acc(R, rd):
    a = R.DeviceAccumulator(D_DIM)
    for i in SURVIVORS:
        a.accumulate_pairs(rd["recs"][i])
    return a


def test_a_round_that_loses_an_honest_client_still_finishes(R, dropout_round):
    rd, P = dropout_round, R.pedersen_ops
    with _acc(R, rd) as a:
        before = a.export().tobytes()
        assert a.extract() is None                                # the self-masks never cancel, and client 2's pairwise masks are missing
        terms = P.dropout_residual_terms_from_shares(SURVIVORS, [GONE], rd["xs"], {GONE: rd["key_sh"][GONE, HOLDERS]},
                                                     {i: rd["self_sh"][i, HOLDERS] for i in SURVIVORS}, rd["pk"], ROUND_NO)
        assert len(terms) == len(SURVIVORS) + len(SURVIVORS) and all(sign == 1 for _, sign in terms[len(SURVIVORS):])
        got = a.extract_opened(opening_terms=terms)
        assert got is not None and got.tobytes() == rd["want"]
        assert a.last_first_bad is None
        assert a.export().tobytes() == before


def test_a_wrong_self_share_fails_every_r_equation(R, dropout_round):
    rd, P = dropout_round, R.pedersen_ops
    selfs = {i: rd["self_sh"][i, HOLDERS] for i in SURVIVORS}
    selfs[3] = selfs[3].copy(); selfs[3][1, 0] ^= 1               # the share survivor 1 holds of client 3's self secret
    with _acc(R, rd) as a:
        before = a.export().tobytes()
        terms = P.dropout_residual_terms_from_shares(SURVIVORS, [GONE], rd["xs"], {GONE: rd["key_sh"][GONE, HOLDERS]}, selfs, rd["pk"], ROUND_NO)
        assert a.extract_opened(opening_terms=terms) is None and a.last_first_bad == 0
        assert a.export().tobytes() == before


def test_a_wrong_key_share_names_the_dropped_client(R, dropout_round):
    rd, P = dropout_round, R.pedersen_ops
    keys = rd["key_sh"][GONE, HOLDERS].copy(); keys[2, 31] ^= 0x08
    with pytest.raises(ValueError, match=r"client 2\b"):
        P.dropout_residual_terms_from_shares(SURVIVORS, [GONE], rd["xs"], {GONE: keys}, {i: rd["self_sh"][i, HOLDERS] for i in SURVIVORS}, rd["pk"], ROUND_NO)


def test_both_secrets_of_one_client_are_refused(R, dropout_round):
    rd, P = dropout_round, R.pedersen_ops
    with pytest.raises(ValueError, match=r"client 2\b"):
        P.dropout_residual_terms_from_shares(SURVIVORS, [GONE], rd["xs"], {GONE: rd["key_sh"][GONE, HOLDERS]},
                                             {i: rd["self_sh"][i, HOLDERS] for i in SURVIVORS + [GONE]}, rd["pk"], ROUND_NO)
