"""Verifiable sharing on the device (rofl_feldman_commit / rofl_feldman_verify: k_shamir_coeffs, k_feldman_commit, k_dh_decode,
k_feldman_check) and one double-masked round in which a dealer and a survivor lie.  Commitments are compared as bytes against the Python model
(tests/feldman_model.py), verdicts against the model's integers (y mod l == f(x)); no tolerance is involved.

Sizes: k_feldman_commit and k_feldman_check run blocks of 64 threads over a flat index -- (secret, k) with k fastest, (secret, share) with the
share fastest -- so n_shares in {1, 63, 64, 65, 257} is one lane per secret, a wave short of one, a full one, a crossing and several blocks
with a ragged tail, and with n_secrets in {1, 3, 257} the waves hold one secret, parts of two, or 64 secrets of one share each (the client's
shape).  One secret at t = 257 crosses the commit kernel's 64-thread blocks four times and ends one thread into a fifth; its 256 coefficients
are half a block of k_shamir_coeffs (256 threads, two coefficients each), so one secret at t = 515 -- 514 coefficients, 257 XOF blocks --
crosses that block as well.  k_feldman_check reads the decoded commitments from global memory: there is no tile edge."""
import ctypes
import itertools

import numpy as np
import pytest

import blind_model as B
import dh_model as D
import feldman_model as F
import orc
import shamir_model as M

pytestmark = pytest.mark.gpu
FP = (32, 7)
ELL = M.L
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


def _mixed_secrets(rng, n):
    """n secrets: a random canonical one, one given as s + l, 2^256 - 1, zero, then random ones"""
    s = int.from_bytes(rng.bytes(31), "little")
    head = [orc.rand_scalars(rng, 1)[0], _b32(s + ELL), _b32(2 ** 256 - 1), _b32(0)]
    return np.stack((head + list(orc.rand_scalars(rng, max(n - 4, 0))))[:n]).copy()


# ---------------------------------------------------------------- commit
@pytest.mark.parametrize("n,t", [(n, t) for n in (1, 3, 65) for t in (1, 2, 5)] + [(1, 257), (1, 515)])
def test_commit_bytes(R, n, t):
    rng = np.random.default_rng(1000 * n + t)
    sec, seeds = _mixed_secrets(rng, n), _seeds(rng, n)
    got = R.secret_sharing.commit(sec, seeds, t)
    assert got.shape == (n, t, 32) and got.dtype == np.uint8
    assert got.tobytes() == F.commit(sec, seeds, t).tobytes()


@pytest.mark.parametrize("family", ["all_equal", "minus_one", "random", "small", "top_range", "two_pow_252"])
def test_commit_extreme_secrets(R, family):
    rng = np.random.default_rng(41)
    sec = orc.extreme_scalar_cases(rng, 3)[family]
    seeds = _seeds(rng, 3)
    got = R.secret_sharing.commit(sec, seeds, 3)
    assert got.tobytes() == F.commit(sec, seeds, 3).tobytes()
    if family == "small":
        assert got[0, 0].tobytes() == bytes(32)                     # the zero secret: the identity encoding
    # (one secret of a call of three is that secret's call of one)
    assert got[1:2].tobytes() == R.secret_sharing.commit(sec[1:2], seeds[1:2], 3).tobytes()


def _dbg(R, name, argtypes, *args):
    fn = getattr(R.api.lib(), name)
    fn.argtypes = argtypes
    return fn(*args)


def test_commit_of_a_key_is_its_public_key_and_the_host_route_agrees(R):
    sz, vp = ctypes.c_size_t, ctypes.c_void_p
    rng = np.random.default_rng(42)
    sk, seeds = D.rand_keys(rng, 5), _seeds(rng, 5)
    dev = R.secret_sharing.commit(sk, seeds, 4)
    assert dev[:, 0].tobytes() == R.key_agreement.public_keys(sk).tobytes()
    host = np.zeros_like(dev)
    assert _dbg(R, "rofl_dbg_host_feldman_commit", [sz, vp, vp, sz, vp], 5, sk.ctypes.data, seeds.ctypes.data, 4, host.ctypes.data) == 0
    assert dev.tobytes() == host.tobytes()
    # and the verdicts of the two routes, with a wrong share, a swapped pair and a refused commitment among them
    xs = np.array([7, 2 ** 32 - 1, 3, 2 ** 31, 1], np.uint32)
    sh = M.share(sk, seeds, 4, 5, xs)
    sh[0, 1, 0] ^= 1; sh[3, [0, 4]] = sh[3, [4, 0]]
    com = dev.copy(); com[2, 3] = 0xff
    got = R.secret_sharing.verify_shares(com, xs, sh)
    hv = np.zeros((5, 5), np.uint8)
    assert _dbg(R, "rofl_dbg_host_feldman_verify", [sz, sz, vp, sz, vp, vp, vp], 5, 4, com.ctypes.data, 5, xs.ctypes.data, sh.ctypes.data, hv.ctypes.data) == 0
    assert got.tobytes() == hv.tobytes()
    want = np.zeros((5, 5), np.uint8); want[0, 1] = 1; want[3, [0, 4]] = 1; want[2] = 2
    assert (got == want).all()


# ---------------------------------------------------------------- verify
@pytest.fixture(scope="module")
def dealt257():
    """257 secrets dealt at threshold 3 over the points 1 .. 257 by the model, computed once and never changed: shares, commitments and the
    polynomials behind them"""
    rng = np.random.default_rng(257)
    sec, seeds = _mixed_secrets(rng, 257), _seeds(rng, 257)
    sh, com = M.share(sec, seeds, 3, 257), F.commit(sec, seeds, 3)
    sh.setflags(write=False); com.setflags(write=False)
    return sh, com, F.polynomials(sec, seeds, 3)


@pytest.mark.parametrize("n_secrets", [1, 3, 257])
@pytest.mark.parametrize("n_shares", [1, 63, 64, 65, 257])
def test_verify_block_sizes(R, dealt257, n_shares, n_secrets):
    sh, com, polys = dealt257
    xs = list(range(1, n_shares + 1))
    c, s = np.ascontiguousarray(com[:n_secrets]), np.ascontiguousarray(sh[:n_secrets, :n_shares])
    got = R.secret_sharing.verify_shares(c, xs, s)
    assert got.shape == (n_secrets, n_shares) and got.dtype == np.uint8
    assert not got.any()                                            # honest shares: all 0 (secret 3 is zero: the identity as C_0)
    # one flipped bit at the first pair, at the last pair of the first block and at the last pair of the call: exactly those verdicts
    total = n_secrets * n_shares
    bad = s.copy()
    hit = sorted({0, min(63, total - 1), total - 1})
    for f in hit:
        bad[f // n_shares, f % n_shares, (f * 7) % 32] ^= 1 << (f % 8)
    got = R.secret_sharing.verify_shares(c, xs, bad)
    assert np.flatnonzero(got.reshape(-1)).tolist() == hit and got.max() == 1
    assert (got == F.verdicts(polys[:n_secrets], xs, bad)).all()


@pytest.mark.parametrize("t", [1, 2, 33])
def test_verify_thresholds(R, t):
    rng = np.random.default_rng(300 + t)
    sec, seeds = _mixed_secrets(rng, 4), _seeds(rng, 4)
    xs = list(range(1, 66))
    sh, com = M.share(sec, seeds, t, 65, xs), R.secret_sharing.commit(sec, seeds, t)
    assert com.tobytes() == F.commit(sec, seeds, t).tobytes()
    assert not R.secret_sharing.verify_shares(com, xs, sh).any()
    bad = sh.copy(); bad[2, 64, 31] ^= 0x01; bad[0, 0] = sh[1, 0]
    got = R.secret_sharing.verify_shares(com, xs, bad)
    assert (got == F.verdicts(F.polynomials(sec, seeds, t), xs, bad)).all() and got.sum() == 2


@pytest.mark.parametrize("xs", [[1], [2 ** 32 - 1], [1, 2 ** 31], [2 ** 31, 1, 2 ** 32 - 1, 3, 65537, 2 ** 32 - 2, 6, 255, 256]], ids=["one", "max", "one_beside_2^31", "mixed"])
def test_verify_points(R, xs):
    """xbits is the bit length of the call's largest point: 1, 32, and lanes of both bit patterns in one wave under 32"""
    rng = np.random.default_rng(len(xs))
    sec, seeds = _mixed_secrets(rng, 5), _seeds(rng, 5)
    sh, com = M.share(sec, seeds, 3, len(xs), xs), F.commit(sec, seeds, 3)
    assert not R.secret_sharing.verify_shares(com, xs, sh).any()
    bad = sh.copy(); bad[4, -1, 0] ^= 0x80; bad[1, 0, 13] ^= 0x02
    got = R.secret_sharing.verify_shares(com, xs, bad)
    assert (got == F.verdicts(F.polynomials(sec, seeds, 3), xs, bad)).all() and got.sum() == 2 and got[4, -1] == got[1, 0] == 1


def test_verify_the_clients_shape(R, dealt257):
    """65 secrets x 1 share: a client checks what it received from 65 dealers against three commitments each (threshold > n_shares)"""
    sh, com, polys = dealt257
    c, s = np.ascontiguousarray(com[:65]), np.ascontiguousarray(sh[:65, 3:4])
    assert not R.secret_sharing.verify_shares(c, [4], s).any()
    bad = s.copy(); bad[64, 0, 1] ^= 1; bad[17, 0, 30] ^= 1
    got = R.secret_sharing.verify_shares(c, [4], bad)
    assert np.flatnonzero(got[:, 0]).tolist() == [17, 64] and (got == F.verdicts(polys[:65], [4], bad)).all()
    assert R.secret_sharing.verify_shares(c, [5], s).all()          # the same shares at another point: none fits


def test_tampering(R):
    rng = np.random.default_rng(77)
    sec, seeds = _mixed_secrets(rng, 5), _seeds(rng, 5)
    t, xs = 4, list(range(1, 71))
    sh, com = M.share(sec, seeds, t, 70, xs), F.commit(sec, seeds, t)
    polys = F.polynomials(sec, seeds, t)
    V = R.secret_sharing.verify_shares
    # two columns swapped: exactly those two columns, in every row
    bad = sh.copy(); bad[:, [5, 66]] = bad[:, [66, 5]]
    got = V(com, xs, bad)
    want = np.zeros((5, 70), np.uint8); want[:, [5, 66]] = 1
    assert (got == want).all() and (got == F.verdicts(polys, xs, bad)).all()
    # a share + l is the same share
    v = B.to_ints(sh[1])
    j = v.index(min(v))
    assert v[j] + ELL < 2 ** 256
    big = sh.copy(); big[1, j] = _b32(v[j] + ELL)
    assert not V(com, xs, big).any()
    # one commitment replaced by another valid point a' B: that whole row 1 (what the integers say of the other polynomial), every other row 0
    for k in (0, 2, 3):
        other = list(polys[2]); other[k] = (other[k] + 1) % ELL
        tam = com.copy(); tam[2] = F.commit_ints(other)
        assert (tam[2] != com[2]).any(axis=1).tolist() == [q == k for q in range(t)]
        got = V(tam, xs, sh)
        assert (got[2] == 1).all() and not got[[0, 1, 3, 4]].any(), k
        assert (got == F.verdicts(polys[:2] + [other] + polys[3:], xs, sh)).all()
    # a commitment that is no canonical encoding: that row 2, every other row 0 -- and 2 wins over wrong shares in that row
    assert D.pyref.ristretto_decode(b"\xff" * 32) is None
    ref = com.copy(); ref[4, 1] = 0xff
    got = V(ref, xs, bad)
    assert (got[4] == 2).all() and (got[:4] == want[:4]).all()
    # the zero secret (row 3): C_0 is the identity encoding and its shares verify; so does the zero polynomial at t = 1
    assert com[3, 0].tobytes() == bytes(32) and not V(com[3:4], xs, sh[3:4]).any()
    zero = np.zeros((1, 1, 32), np.uint8)
    assert not V(zero, [9], zero).any() and V(zero, [9], _b32(1).reshape(1, 1, 32)).tolist() == [[1]]


def test_a_subset_of_the_rows_or_columns_is_those_rows_or_columns(R, dealt257):
    sh, com, _ = dealt257
    S = R.secret_sharing
    bad = sh[:70, :130].copy()
    for r, c in ((0, 0), (1, 63), (5, 64), (69, 129), (33, 100), (64, 1)):
        bad[r, c, (r + c) % 32] ^= 1
    xs = np.arange(1, 131)
    whole = S.verify_shares(com[:70], xs, bad)
    assert whole.sum() == 6
    rows = [69, 0, 5, 33, 2]
    assert (S.verify_shares(com[rows], xs, bad[rows]) == whole[rows]).all()
    cols = [129, 0, 63, 64, 100, 7]
    assert (S.verify_shares(com[:70], xs[cols], bad[:, cols]) == whole[:, cols]).all()
    cols = [1, 0, 2]                                                # (a subset whose own largest point is small: another xbits)
    assert (S.verify_shares(com[:70], xs[cols], bad[:, cols]) == whole[:, cols]).all()
    assert (S.verify_shares(com[rows], xs[[100]], bad[rows][:, [100]]) == whole[rows][:, [100]]).all()
    # commit: the rows of a call do not depend on their neighbours
    rng = np.random.default_rng(5)
    sec, seeds = _mixed_secrets(rng, 6), _seeds(rng, 6)
    c6 = S.commit(sec, seeds, 5)
    assert S.commit(sec[[4, 1]], seeds[[4, 1]], 5).tobytes() == np.ascontiguousarray(c6[[4, 1]]).tobytes()


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
def vss_round(R):
    """the round of test_gpu_secret_sharing.py -- six clients, d = 257, threshold 4, client 2 never submits -- with every dealer publishing
    the commitments of both its sharings (the device calls).  Built once, never changed."""
    P, K, S = R.pedersen_ops, R.key_agreement, R.secret_sharing
    rng = np.random.default_rng(20261024)
    sk, b = D.rand_keys(rng, N), rng.integers(0, 256, size=(N, 32), dtype=np.uint8)
    pk = K.public_keys(sk)
    peers = P.pairwise_peers_from_keys(clients=[(i, sk[i]) for i in range(N)], public_keys=pk, round_no=ROUND_NO)
    bl = P.double_masked_blinding_vecs([(i, peers[i], b[i]) for i in range(N)], ROUND_NO, D_DIM)
    cs = _seeds(rng, 2 * N)
    key_sh, self_sh = S.share(sk, cs[:N], THRESHOLD, N), S.share(b, cs[N:], THRESHOLD, N)      # [owner, holder, 32]
    both = S.commit(np.concatenate([sk, b]), cs, THRESHOLD)                                     # ONE call: [key of 0 .. 5 | self of 0 .. 5]
    assert both.tobytes() == F.commit(np.concatenate([sk, b]), cs, THRESHOLD).tobytes()
    key_com, self_com = both[:N].copy(), both[N:].copy()
    assert key_com[:, 0].tobytes() == pk.tobytes()
    tab = _value_scalars()
    ks = [rng.integers(-20, 21, size=D_DIM) for _ in range(N)]
    recs = []
    for i in range(N):
        x = np.stack([tab[int(k)] for k in ks[i]])
        recs.append(np.ascontiguousarray(np.concatenate([orc.commit_vec(x, bl[i]), orc.commit_vec(bl[i], None)], axis=1)))
    want = np.sum(np.stack([(ks[i] / 128.0).astype(np.float32) for i in SURVIVORS]).astype(np.float64), axis=0).astype(np.float32)
    for a in (pk, key_sh, self_sh, key_com, self_com):
        a.setflags(write=False)
    return dict(pk=pk, key_sh=key_sh, self_sh=self_sh, key_com=key_com, self_com=self_com, recs=recs, want=want.tobytes())


def test_every_client_checks_what_every_dealer_sent_it(R, vss_round):
    """a 12 x 1 call per client: its shares of the six keys and the six self secrets against the dealers' commitments.  Dealer 5 sends client 3
    a wrong share of its self secret: client 3's verdicts name that dealing, everybody else's are clean."""
    rd, S = vss_round, R.secret_sharing
    com = np.concatenate([rd["key_com"], rd["self_com"]])
    for c in range(N):
        got = np.concatenate([rd["key_sh"][:, c], rd["self_sh"][:, c]])[:, None, :].copy()
        if c == 3:
            got[N + 5, 0, 9] ^= 0x04
        verdict = S.verify_shares(com, [c + 1], got)
        assert verdict.shape == (2 * N, 1)
        assert np.flatnonzero(verdict[:, 0]).tolist() == ([N + 5] if c == 3 else []), c


def _acc(R, rd):
    a = R.DeviceAccumulator(D_DIM)
    for i in SURVIVORS:
        a.accumulate_pairs(rd["recs"][i])
    return a


def _verified_args(rd, holders, selfs):
    return (SURVIVORS, [GONE], [h + 1 for h in holders], {GONE: rd["key_sh"][GONE, holders]}, selfs, {GONE: rd["key_com"][GONE]},
            {i: rd["self_com"][i] for i in SURVIVORS}, rd["pk"], ROUND_NO)


def test_a_lying_survivor_is_named_and_the_round_still_finishes(R, vss_round):
    rd, P = vss_round, R.pedersen_ops
    holders = SURVIVORS                                               # all five survivors answer
    selfs = {i: rd["self_sh"][i, holders].copy() for i in SURVIVORS}
    selfs[1][holders.index(4), 17] ^= 0x20                            # survivor 4 flips a bit in its share of client 1's self secret
    with _acc(R, rd) as a:
        before = a.export().tobytes()
        # the old call interpolates all five columns and the opening is refused: nobody is named
        old = P.dropout_residual_terms_from_shares(SURVIVORS, [GONE], [h + 1 for h in holders], {GONE: rd["key_sh"][GONE, holders]}, selfs, rd["pk"], ROUND_NO)
        assert a.extract_opened(opening_terms=old) is None
        terms, liars = P.dropout_residual_terms_from_verified_shares(*_verified_args(rd, holders, selfs))
        assert liars == [4]
        assert len(terms) == len(SURVIVORS) + len(SURVIVORS)
        got = a.extract_opened(opening_terms=terms)
        assert got is not None and got.tobytes() == rd["want"]
        assert a.last_first_bad is None
        assert a.export().tobytes() == before
    # nobody lies: no liars, the same terms
    honest = {i: rd["self_sh"][i, holders] for i in SURVIVORS}
    terms2, liars2 = P.dropout_residual_terms_from_verified_shares(*_verified_args(rd, holders, honest))
    assert liars2 == [] and terms2 == terms


def test_two_liars_of_four_answering_leave_too_few(R, vss_round):
    rd, P = vss_round, R.pedersen_ops
    holders = [0, 1, 3, 4]
    selfs = {i: rd["self_sh"][i, holders].copy() for i in SURVIVORS}
    selfs[0][holders.index(3), 0] ^= 1
    selfs[5][holders.index(4), 31] ^= 0x08
    with pytest.raises(ValueError, match=r"\[3, 4\]"):
        P.dropout_residual_terms_from_verified_shares(*_verified_args(rd, holders, selfs))
    # a dealer whose published C_0 is not its public key is refused before anything else
    args = list(_verified_args(rd, holders, {i: rd["self_sh"][i, holders] for i in SURVIVORS}))
    args[5] = {GONE: rd["self_com"][GONE]}
    with pytest.raises(ValueError, match=r"client 2\b"):
        P.dropout_residual_terms_from_verified_shares(*args)
