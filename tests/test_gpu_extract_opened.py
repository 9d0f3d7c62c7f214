"""Extraction of a round that rejected somebody (rofl_acc_extract_opened / _terms, k_acc_open, DeviceAccumulator.extract_opened).
Nothing expected comes from the code under test: records are the oracle's (L = orc.commit_vec(x, r), R = orc.commit_vec(r, None)), the
openings are sums mod l of blind_model.combine vectors, points and logs are the oracle's, and the aggregate is the plain f32 sum of the
accepted clients' grid-aligned values, compared by .tobytes().

6 clients, 8-bit values k / 128, d in {1, 257, 600}: one lane; a crossing of one 256-thread block of the grid that takes the L half and the
R half of a pair in separate blocks; several blocks with a ragged tail."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import blind_model as M
import orc

pytestmark = pytest.mark.gpu
FP = (32, 7)
ELL = M.L
N = 6
DS = (1, 257, 600)
ACCEPTED, REJECTED = (0, 2, 3, 5), (1, 4)
TABLE, BITS = 1 << 15, 16      # BSGSTable::default() of fp32 (api.default_bsgs)
SEED = b"\x21" * 32


@pytest.fixture(scope="module")
def R():
    import rofl_project_code_amd as R
    from rofl_project_code_amd import build
    build.build()
    R.set_device(0)
    R.api.set_fp(*FP)
    return R


def _value_scalars():
    """the oracle's scalar of every 8-bit value k / 128"""
    tab = {}
    for k in range(-128, 128):
        rc, s = orc.f32_to_scalar(k / 128.0, *FP)
        assert rc == 0
        tab[k] = s.copy()
    return tab


def _records(tab, ks, r):
    x = np.stack([tab[int(k)] for k in ks])
    return np.ascontiguousarray(np.concatenate([orc.commit_vec(x, r), orc.commit_vec(r, None)], axis=1))


def _sum_scalars(vecs, d):
    return M.to_arr([sum(col) for col in zip(*[M.to_ints(v) for v in vecs])] if vecs else [0] * d)


def _sum_f32(ks, init=0):
    """plain f32 sum of the values k / 128 (exact: small multiples of 2^-7); init 1 adds the one raw unit of ElGamalPair::unity()"""
    s = np.sum(np.stack([(k / 128.0).astype(np.float32) for k in ks]).astype(np.float64), axis=0)
    return (s + init / 128.0).astype(np.float32)


def _oracle_fold(d, recs):
    acc = np.zeros((d, 64), np.uint8)
    for p in recs:
        rc, part = orc.add_points_vec(acc.reshape(-1, 32), p.reshape(-1, 32))
        assert rc == 0
        acc = part.reshape(d, 64)
    return acc


def _build_rounds(ds):
    """per d: a round of N clients with pairwise blindings from the model"""
    tab = _value_scalars()
    out = {}
    for d in ds:
        rng = np.random.default_rng(900 + d)
        seeds = {(i, j): bytes(rng.integers(0, 256, 32, dtype=np.uint8)) for i in range(N) for j in range(i + 1, N)}
        ks = [rng.integers(-127, 128, size=d) for _ in range(N)]
        r = [M.combine([(seeds[(min(i, j), max(i, j))], 1 if i < j else -1) for j in range(N) if j != i], d) for i in range(N)]
        assert not _sum_scalars(r, d).any()
        out[d] = dict(d=d, seeds=seeds, ks=ks, r=r, recs=[_records(tab, ks[i], r[i]) for i in range(N)],
                      s=_sum_scalars([r[i] for i in ACCEPTED], d))
    return out


@pytest.fixture(scope="module")
def rounds():
    """built once, never changed"""
    return _build_rounds(DS)


def _acc(R, rd, members, init=0):
    a = R.DeviceAccumulator(rd["d"], reference_unity=bool(init))
    for i in members:
        a.accumulate_pairs(rd["recs"][i])
    return a


def _raw_opened(R, acc, opening, fill=7.0):
    """rofl_acc_extract_opened itself, with an output buffer of the test's -> (rc, ok, first_bad, out)"""
    L = R.api.lib()
    s = np.ascontiguousarray(opening, dtype=np.uint8)
    out = np.full(acc.size, fill, np.float32)
    ok, bad = ctypes.c_int(-1), ctypes.c_size_t(12345)
    rc = L.rofl_acc_extract_opened(ctypes.c_uint64(acc._h), s.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(TABLE), BITS, FP[0], FP[1],
                                   out.ctypes.data_as(ctypes.c_void_p), ctypes.byref(ok), ctypes.byref(bad))
    return rc, ok.value, bad.value, out


def _plus(s, k, delta):
    s = s.copy()
    s[k] = M.to_arr([M.to_ints(s[k:k + 1])[0] + delta])[0]
    return s


# ---- 1. recovery ----
@pytest.mark.parametrize("init", [0, 1])
@pytest.mark.parametrize("d", DS)
def test_accepted_sum_is_recovered_from_the_opening(R, rounds, d, init):
    rd = rounds[d]
    want = _sum_f32([rd["ks"][i] for i in ACCEPTED], init).tobytes()
    terms = R.pedersen_ops.pairwise_residual_terms(ACCEPTED, REJECTED, rd["seeds"])
    assert M.combine(terms, d).tobytes() == rd["s"].tobytes()
    with _acc(R, rd, ACCEPTED, init) as a:
        before = a.export()
        if init == 0:
            assert before.tobytes() == _oracle_fold(d, [rd["recs"][i] for i in ACCEPTED]).tobytes()
        assert a.extract() is None      # a member left out: the blindings do not cancel
        got = a.extract_opened(opening=rd["s"])
        assert got is not None and got.tobytes() == want
        got = a.extract_opened(opening_terms=terms)
        assert got is not None and got.tobytes() == want
        assert a.last_first_bad is None
        rc, ok, bad, out = _raw_opened(R, a, rd["s"])
        assert (rc, ok, bad) == (0, 1, ctypes.c_size_t(-1).value) and out.tobytes() == want
        assert a.extract() is None
        assert a.export().tobytes() == before.tobytes()


def test_the_opening_as_a_device_tensor(R):
    """the opening handed over as a GPU torch tensor, read in place (torch in a child process, as the other device-pointer tests do)"""
    r = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "gpu_extract_opened_device_check.py")],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "OPENING_DEVICE_TENSOR PASS" in r.stdout, r.stdout + r.stderr[-3000:]


def test_stripped_points_equal_the_oracles(R, rounds):
    """L' = L_sum - s B~ through the oracle alone: its logs are what the device path returns"""
    d = 257
    rd = rounds[d]
    fold = _oracle_fold(d, [rd["recs"][i] for i in ACCEPTED])
    assert fold[:, 32:].tobytes() == orc.commit_vec(rd["s"], None).tobytes()      # R_sum = s B
    minus = M.to_arr([-v for v in M.to_ints(rd["s"])])
    rc, stripped = orc.add_points_vec(fold[:, :32], orc.commit_vec(np.zeros((d, 32), np.uint8), minus))
    assert rc == 0
    rc, logs = orc.bsgs_solve(stripped, TABLE, BITS)
    assert rc == 0
    want = np.array([orc.scalar_to_f32(logs[k], *FP) for k in range(d)], np.float32)
    assert want.tobytes() == _sum_f32([rd["ks"][i] for i in ACCEPTED]).tobytes()
    with _acc(R, rd, ACCEPTED) as a:
        assert a.extract_opened(opening=rd["s"]).tobytes() == want.tobytes()


# ---- 2. scalar edge cases ----
def test_openings_at_the_edges_of_the_scalar_range(R):
    """the opening runs through the signed-digit carries of the radix-256 multiplication and the product with the identity; the same
    opening as s + l (not canonical, fits 256 bits) and, for one entry, as the raw bytes 0x80 .. 0x80, gives the same answer"""
    d = 257
    rng = np.random.default_rng(77)
    fam = orc.extreme_scalar_cases(rng, 40)
    all80 = int.from_bytes(b"\x80" * 32, "little")
    special = [0, 1, ELL - 1, 1 << 252, all80 % ELL]
    s_int = [v for name in sorted(fam) for v in M.to_ints(fam[name])] + special
    s_int += M.to_ints(orc.rand_scalars(rng, d - len(s_int)))
    assert len(s_int) == d
    i80 = 240 + 4
    s = M.to_arr(s_int)
    r0 = orc.rand_scalars(rng, d)
    r1 = M.to_arr([a - b for a, b in zip(s_int, M.to_ints(r0))])
    tab = _value_scalars()
    ks = [rng.integers(-127, 128, size=d) for _ in range(2)]
    recs = [_records(tab, ks[0], r0), _records(tab, ks[1], r1)]
    want = _sum_f32(ks).tobytes()
    raw80 = s.copy(); raw80[i80] = 0x80
    plus_l = np.frombuffer(b"".join((v + ELL).to_bytes(32, "little") for v in s_int), np.uint8).reshape(d, 32)
    with R.DeviceAccumulator(d) as a:
        a.accumulate_pairs(recs[0]); a.accumulate_pairs(recs[1])
        for name, op in (("canonical", s), ("0x80 bytes", raw80), ("s + l", plus_l)):
            got = a.extract_opened(opening=op)
            assert got is not None and got.tobytes() == want, (name, a.last_first_bad)
        bad = _plus(s, i80 - 2, 1)      # l - 1 -> 0
        assert a.extract_opened(opening=bad) is None and a.last_first_bad == i80 - 2


# ---- 3. a wrong opening is caught and located ----
@pytest.mark.parametrize("d", DS)
def test_a_wrong_opening_is_caught_and_located(R, rounds, d):
    rd = rounds[d]
    s = rd["s"]
    want = _sum_f32([rd["ks"][i] for i in ACCEPTED]).tobytes()
    with _acc(R, rd, ACCEPTED) as a:
        before = a.export().tobytes()
        for k in sorted({0, min(255, d - 1), d - 1}):      # the first, the last of the first block, the last
            bad = s.copy(); bad[k, 5] ^= 0x10
            rc, ok, first, out = _raw_opened(R, a, bad)
            assert (rc, ok, first) == (0, 0, k) and (out == 7.0).all()
            assert a.extract_opened(opening=bad) is None and a.last_first_bad == k
            assert a.export().tobytes() == before
            got = a.extract_opened(opening=s)
            assert got is not None and got.tobytes() == want and a.last_first_bad is None
        if d > 1:
            lo, hi = d // 3, d - 2
            two = s.copy(); two[hi, 0] ^= 1; two[lo, 31] ^= 1
            assert _raw_opened(R, a, two)[1:3] == (0, lo)
            comp = _plus(_plus(s, lo, 12345), hi, -12345)      # errors that cancel in any sum over the coordinates
            assert _raw_opened(R, a, comp)[1:3] == (0, lo)
            assert a.extract_opened(opening=comp) is None and a.last_first_bad == lo
        assert a.export().tobytes() == before
    # an opening of another accept set: valid for {0, 2, 3, 5}, the sum is over {0, 2, 3}
    r5 = M.to_ints(rd["r"][5])
    first = next(k for k in range(d) if r5[k])
    with _acc(R, rd, (0, 2, 3)) as a:
        assert _raw_opened(R, a, s)[1:3] == (0, first)
        assert a.extract_opened(opening_terms=R.pedersen_ops.pairwise_residual_terms(ACCEPTED, REJECTED, rd["seeds"])) is None and a.last_first_bad == first
        got = a.extract_opened(opening=_sum_scalars([rd["r"][i] for i in (0, 2, 3)], d))
        assert got is not None and got.tobytes() == _sum_f32([rd["ks"][i] for i in (0, 2, 3)]).tobytes()


# ---- 4. consistency ----
@pytest.mark.parametrize("init", [0, 1])
@pytest.mark.parametrize("d", DS)
def test_a_zero_opening_is_the_plain_extraction(R, rounds, d, init):
    rd = rounds[d]
    with _acc(R, rd, range(N), init) as a:
        plain = a.extract()
        assert plain is not None and plain.tobytes() == _sum_f32(rd["ks"], init).tobytes()
        zero = a.extract_opened(opening=np.zeros((d, 32), np.uint8))
        none = a.extract_opened(opening_terms=[])
        assert zero is not None and none is not None and zero.tobytes() == plain.tobytes() == none.tobytes()
    with _acc(R, rd, ACCEPTED, init) as a:      # and where the plain extraction says None, so do they -- with the place
        assert a.extract() is None and a.extract_opened(opening_terms=[]) is None
        assert a.last_first_bad == next(k for k, v in enumerate(M.to_ints(rd["s"])) if v)


def test_the_composed_host_route_agrees(R, rounds):
    d = 257
    rd = rounds[d]
    host = R.EncModelParamsAccumulator(d)
    host.acc = _oracle_fold(d, [rd["recs"][i] for i in ACCEPTED])
    want = _sum_f32([rd["ks"][i] for i in ACCEPTED]).tobytes()
    assert host.extract() is None
    got = host.extract(opening=rd["s"])
    assert got is not None and got.tobytes() == want
    bad = rd["s"].copy(); bad[200, 0] ^= 1
    assert host.extract(opening=bad) is None
    with _acc(R, rd, ACCEPTED) as a:
        assert a.extract_opened(opening=rd["s"]).tobytes() == got.tobytes()
        assert a.extract_opened(opening=bad) is None


def test_any_representative_of_the_sums_gives_the_same_verdict(R, rounds):
    """the same sums reached through additions in two groupings (one record at a time in order; one call with the records in reverse, and
    the exported pairs of a part added to the rest) are held in different coordinates: verdicts and values are those of the points"""
    d = 257
    rd = rounds[d]
    want = _sum_f32([rd["ks"][i] for i in ACCEPTED]).tobytes()
    bad = rd["s"].copy(); bad[256, 9] ^= 4
    res = []
    with _acc(R, rd, ACCEPTED) as a, R.DeviceAccumulator(d) as b, R.DeviceAccumulator(d) as c:
        b._add([rd["recs"][i] for i in reversed(ACCEPTED)], 64)
        with _acc(R, rd, ACCEPTED[2:]) as part:
            c._add([rd["recs"][i] for i in ACCEPTED[:2]] + [part.export()], 64)
        assert a.export().tobytes() == b.export().tobytes() == c.export().tobytes()
        for acc in (a, b, c):
            got = acc.extract_opened(opening=rd["s"])
            assert got is not None and got.tobytes() == want
            assert acc.extract_opened(opening=bad) is None
            res.append(acc.last_first_bad)
    assert res == [256] * 3


# ---- 5. end to end ----
def _e2e(R, xs, bls, residual):
    """a DeviceRound of EncParamsRangeCompressed updates, one proof byte flipped: verify, accumulate the accepted, extract with the terms
    residual(verdicts) gives"""
    n, d = len(xs), xs[0].size
    cls = R.EncParamsRangeCompressed
    ups = [cls.encrypt(x, b, 8, 1, 1.0, nonce_seed=bytes([i + 1]) * 32, fp=FP) for i, (x, b) in enumerate(zip(xs, bls))]
    ups[4] = cls.deserialize(ups[4].serialize())
    ups[4].rand_proof[70] ^= 1
    with R.DeviceRound(cls, d, max_clients=n) as rnd, R.DeviceAccumulator(d) as acc:
        rnd.ingest(ups)
        verdicts = rnd.verify(verifier_seed=SEED, fp=FP)
        assert verdicts == [i != 4 for i in range(n)]
        rnd.accumulate_into(acc, accept=verdicts)
        assert acc.extract() is None
        got = acc.extract_opened(opening_terms=residual(verdicts))
        want = np.sum(np.stack([x for x, v in zip(xs, verdicts) if v]).astype(np.float64), axis=0).astype(np.float32)
        assert got is not None and got.tobytes() == want.tobytes()


def test_a_round_that_rejects_a_client_still_finishes(R):
    n, d = 6, 64
    rng = np.random.default_rng(5)
    xs = [(rng.integers(-100, 101, size=d) / 128.0).astype(np.float32) for _ in range(n)]
    P = R.pedersen_ops
    seeds = {(i, j): bytes(rng.integers(0, 256, 32, dtype=np.uint8)) for i in range(n) for j in range(i + 1, n)}
    bls = P.pairwise_blinding_vecs([(i, [(j, seeds[(min(i, j), max(i, j))]) for j in range(n) if j != i]) for i in range(n)], d)
    _e2e(R, xs, list(bls), lambda v: P.pairwise_residual_terms([i for i in range(n) if v[i]], [i for i in range(n) if not v[i]], seeds))
    dealer = bytes(range(32))
    _e2e(R, xs, P.generate_cancelling_scalar_vec_seeded(n, d, dealer), lambda v: P.cancelling_residual_terms(n, dealer, v))
