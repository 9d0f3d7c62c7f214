"""The device-resident round (rofl_round_*, DeviceRound): a round's updates uploaded once and decoded once, both verification legs and the
accumulation reading the decoded points.  Everything is compared with the paths that exist without it: verdicts with cls.verify_batch and
every update's own verify(), each C leg with the existing batched call on the same bytes, sums with DeviceAccumulator.accumulate_batch and a
fold of the oracle's point additions; and the decode counter shows that the repeats are gone.

Rounds are real encrypt() outputs with nonce seeds; the blindings of a round cancel, so that an honest round both verifies and extracts."""
import ctypes
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

import orc

pytestmark = pytest.mark.gpu
FP = (32, 7)
ELL = 2 ** 252 + 27742317777372353535851937790883648493
BAD_POINT = np.frombuffer(bytes([1] + [0] * 31), np.uint8)      # odd s: not a Ristretto encoding
SEED = b"\x21" * 32


@pytest.fixture(scope="module")
def R():
    import rofl_project_code_amd as R
    from rofl_project_code_amd import build
    build.build()
    R.set_device(0)
    R.api.set_fp(*FP)
    yield R
    R.set_option("verify_batch", 1)


def _names(R):
    return {"range": R.EncParamsRange, "range_compressed": R.EncParamsRangeCompressed, "l2": R.EncParamsL2, "l2_compressed": R.EncParamsL2Compressed}


def _make_round(R, cls, n, d, seed0, nb=8, P=4, check=1.0, l2n=32):
    """n honest updates of d elements (values k / 128, |k| <= 3) whose blindings sum to zero; returns (values, updates)"""
    rng = np.random.default_rng(seed0)
    xs = [(rng.integers(-3, 4, size=d) / 128.0).astype(np.float32) for _ in range(n)]
    bls = []
    for _ in range(n - 1):
        b = rng.integers(0, 256, size=(d, 32), dtype=np.uint8); b[:, 31] &= 0x0F      # < 2^252: canonical
        bls.append(b)
    bls.append(R.pedersen_ops.add_scalar_vec(np.zeros((d, 32), np.uint8), R.pedersen_ops.add_scalar_vec_vec(bls), subtract=True))
    ups = []
    for i, (x, b) in enumerate(zip(xs, bls)):
        ns = bytes([(seed0 + i) % 251 + 1]) * 32
        if issubclass(cls, R.EncParamsL2):
            r2 = rng.integers(0, 256, size=(d, 32), dtype=np.uint8); r2[:, 31] &= 0x0F
            ups.append(cls.encrypt(x, b, nb, P, l2n, nonce_seed=ns, rand_scalars=r2, fp=FP))
        else:
            ups.append(cls.encrypt(x, b, nb, P, check, nonce_seed=ns, fp=FP))
    return xs, ups


def _copy(u):
    return type(u).deserialize(u.serialize())


def _sum_f32(xs):
    return np.sum(np.stack(xs).astype(np.float64), axis=0).astype(np.float32)


def _plus_one(row):
    z = (int.from_bytes(row.tobytes(), "little") + 1) % ELL
    row[:] = np.frombuffer(z.to_bytes(32, "little"), np.uint8)


def _tampered(R, cls, ups, d):
    """one member tampered per kind (the kinds of test_gpu_range_batch.py::_tampered / test_gpu_l2_batch.py); returns the list and, per
    tampered member, what was done to it"""
    t = [_copy(u) for u in ups]
    what = {}
    l2 = issubclass(cls, R.EncParamsL2)
    zm = {R.EncParamsRange: 64, R.EncParamsL2: 96, R.EncParamsL2Compressed: 64}.get(cls)      # offset of Z_m in a per-element proof
    if cls is R.EncParamsRangeCompressed:
        t[1].rand_proof[70] ^= 1; what[1] = "rand"
    else:
        pr = t[1].square_proofs if l2 else t[1].rand_proofs
        _plus_one(pr[d // 2, zm:zm + 32]); what[1] = "sigma"                                   # a response + 1
        pr = t[6].square_proofs if l2 else t[6].rand_proofs
        pr[3, zm + 32:zm + 64] = 0xFF; what[6] = "sigma"                                       # a non-canonical scalar
    t[2].enc_values[7, :32] = ups[3].enc_values[7, :32]; what[2] = "L"                          # a foreign valid point as L
    t[4].enc_values[9, 32:64] = BAD_POINT; what[4] = "R"                                        # an undecodable R
    if l2:
        t[5].enc_values[11, 64:96] = BAD_POINT; what[5] = "csq"                                 # an undecodable c_sq
        t[9].square_range_proof[5 * 32 + 3] ^= 1; what[9] = "sum"                               # a wrong sum proof
    else:
        t[5].enc_values[d - 1, :32] = BAD_POINT; what[5] = "L-late"                             # an undecodable L at an index >= k (check 0.5)
    t[8].range_proofs[1, 7 * 32 + 33] ^= 2; what[8] = "range"                                   # a bit flipped in a range proof
    return t, what


def _c_legs(R, cls, rnd, us, k):
    """the round's C legs next to the existing batched calls on the same bytes"""
    api = R.api
    stride = rnd.record_len
    h = rnd._h
    if cls is not R.EncParamsRangeCompressed:
        if cls is R.EncParamsRange:
            got, _ = api.device_round.verify_sigma(h, 0, [u.rand_proofs.ctypes.data for u in us])
            want = R.rand_proof_vec.verify_randproof_vec_batch([u.rand_proofs for u in us], [u.enc_values for u in us])
        else:
            kind = 2 if cls is R.EncParamsL2Compressed else 1
            got, gs = api.device_round.verify_sigma(h, kind, [u.square_proofs.ctypes.data for u in us], want_csq=True)
            want, ws = cls._square_batch(us)
            assert (gs == ws).all()
        assert got == want, (got, want)
    rp = us[0].range_proofs
    got = api.device_round.verify_range(h, [u.range_proofs.ctypes.data for u in us], rp.shape[1], rp.shape[0], k, us[0].prove_range, verifier_seed=SEED, fp=FP)
    want = R.range_proof_vec.verify_rangeproof_batch([u.range_proofs for u in us], [u.enc_values[:k] for u in us], us[0].prove_range, verifier_seed=SEED, fp=FP, commit_stride=stride)
    assert got == want, (got, want)
    return got


def _oracle_fold(d, accepted):
    acc = np.zeros((d, 64), np.uint8)
    for u in accepted:
        pairs = np.ascontiguousarray(u.pedersen_part()).reshape(-1, 64)
        m = min(d, pairs.shape[0])      # zip() truncates
        rc, part = orc.add_points_vec(np.ascontiguousarray(acc[:m]).reshape(-1, 32), np.ascontiguousarray(pairs[:m]).reshape(-1, 32))
        assert rc == 0
        acc[:m] = part.reshape(m, 64)
    return acc


def _check_sums(R, rnd, ups, accept, d, oracle=True):
    """accumulate_into(accept) against accumulate_batch of the accepted updates (and the oracle's fold)"""
    accepted = list(ups) if accept is None else [u for u, a in zip(ups, accept) if a]
    with R.DeviceAccumulator.unity(d) as a, R.DeviceAccumulator.unity(d) as b:
        rnd.accumulate_into(a, accept=accept)
        b.accumulate_batch(accepted)
        ex = a.export()
        assert (ex == b.export()).all()
        if oracle:
            assert (ex == _oracle_fold(d, accepted)).all()
        return ex, a.extract()


@pytest.mark.parametrize("name", ["range", "range_compressed", "l2", "l2_compressed"])
def test_verdicts_and_sums_of_twelve_clients(R, name):
    cls = _names(R)[name]
    n, d, nb, P = 12, 300, 8, 4
    check = 0.5
    l2 = issubclass(cls, R.EncParamsL2)
    k = d if l2 else R.params._num_checked(d, check)
    xs, ups = _make_round(R, cls, n, d, 40 + len(name), nb=nb, P=P, check=check)
    try:
        with R.DeviceRound(cls, d, max_clients=n) as rnd:
            # the honest round: all true, the sum is the sum of the values
            rnd.ingest(ups)
            for vb in (2, 1):
                R.set_option("verify_batch", vb)
                assert rnd.verify(verifier_seed=SEED, fp=FP) == cls.verify_batch(ups, verifier_seed=SEED, fp=FP) == [True] * n
                assert _c_legs(R, cls, rnd, ups, k) == [True] * n
            ex, agg = _check_sums(R, rnd, ups, None, d)
            assert agg is not None and agg.tobytes() == _sum_f32(xs).tobytes()
            # one tampered member per kind
            t, what = _tampered(R, cls, ups, d)
            rnd.reset()
            rnd.ingest(t)
            single = [u.verify(verifier_seed=SEED, fp=FP) for u in t]
            for vb in (2, 1):
                R.set_option("verify_batch", vb)
                got = rnd.verify(verifier_seed=SEED, fp=FP)
                assert got == cls.verify_batch(t, verifier_seed=SEED, fp=FP) == single, (vb, got, single)
                ok_range = _c_legs(R, cls, rnd, t, k)
                assert ok_range == [what.get(i) not in ("range", "L") for i in range(n)]      # an undecodable L at an index >= k is not the range leg's
            want = [i not in what for i in range(n)]
            if cls is R.EncParamsL2Compressed:
                want[4] = True      # this arm never reads R (params.rs:257-267): the verdict verify_batch gives
            assert single == want
            # the oracle rejects every tampered component
            fpb, fpf = FP
            for i, w in what.items():
                u = t[i]
                if w == "sum":
                    assert orc.verify_rangeproof_l2(u.square_range_proof, u._sum_c_sq(), u.l2_prove_range, fpb, fpf)[1] is False
                elif w == "range":
                    assert orc.verify_rangeproof(u.range_proofs, u.enc_values[:k, :32].copy(), nb, fpb, fpf)[1] is False
                elif cls is R.EncParamsRangeCompressed:
                    rc, ok = orc.compressed_verify(u.rand_proof, u.enc_values)
                    assert not (rc == 0 and ok)
                elif cls is R.EncParamsL2Compressed:
                    if w != "R":
                        assert orc.sigma_verify(2, u.square_proofs, np.ascontiguousarray(np.concatenate([u.enc_values[:, :32], u.enc_values[:, 64:96]], axis=1)))[1] is False
                else:
                    assert orc.sigma_verify(1 if l2 else 0, u.square_proofs if l2 else u.rand_proofs, u.enc_values)[1] is False
            # sums of the accepted members; a member whose R does not decode cannot be added, whatever its verdict
            accept = list(single)
            if cls is R.EncParamsL2Compressed:
                with R.DeviceAccumulator.unity(d) as a, R.DeviceAccumulator.unity(d) as b:
                    for call in (lambda: rnd.accumulate_into(a, accept=accept), lambda: b.accumulate_batch([u for u, s in zip(t, accept) if s])):
                        with pytest.raises(R.RoflError) as e:
                            call()
                        assert e.value.code == 5
                    assert (a.export() == 0).all() and (b.export() == 0).all()
                accept[4] = False
            _check_sums(R, rnd, t, accept, d)
            # accept = None with an undecodable member: FormatError, the accumulator unchanged; an accumulator of another length: 11
            with R.DeviceAccumulator.unity(d) as a:
                rnd.accumulate_into(a, accept=[i == 0 for i in range(n)])
                before = a.export()
                with pytest.raises(R.RoflError) as e:
                    rnd.accumulate_into(a)
                assert e.value.code == 5 and (a.export() == before).all()
            with R.DeviceAccumulator.unity(d + 1) as a:
                with pytest.raises(R.RoflError) as e:
                    rnd.accumulate_into(a, accept=accept)
                assert e.value.code == 11 and (a.export() == 0).all()
    finally:
        R.set_option("verify_batch", 1)


def test_ingest_in_pieces_reset_and_destroy(R):
    cls, n, d = R.EncParamsL2, 12, 300
    xs, ups = _make_round(R, cls, n, d, 70)
    t, what = _tampered(R, cls, ups, d)
    xs2, ups2 = _make_round(R, cls, 5, d, 90)
    with R.DeviceRound(cls, d, max_clients=n) as whole, R.DeviceRound(cls, d, max_clients=n) as parts:
        whole.ingest(t)
        parts.ingest(t[:1]); parts.ingest(t[1:6]); parts.ingest(t[6:])
        assert len(parts) == n
        want = whole.verify(verifier_seed=SEED, fp=FP)
        assert parts.verify(verifier_seed=SEED, fp=FP) == want == [i not in what for i in range(n)]
        ex, _ = _check_sums(R, whole, t, want, d, oracle=False)
        ex2, _ = _check_sums(R, parts, t, want, d, oracle=False)
        assert (ex == ex2).all()
        # a thirteenth client: 11, nothing changes (Python and C)
        with pytest.raises(R.RoflError) as e:
            parts.ingest(ups2[:1])
        assert e.value.code == 11 and len(parts) == n
        recs = (ctypes.c_void_p * 1)(ups2[0].enc_values.ctypes.data)
        assert R.api.lib().rofl_round_ingest(ctypes.c_uint64(parts._h), ctypes.c_size_t(1), recs, None) == 11
        assert parts.verify(verifier_seed=SEED, fp=FP) == want
        ex3, _ = _check_sums(R, parts, t, want, d, oracle=False)
        assert (ex3 == ex).all()
        # reset, then another round in the same memory
        parts.reset()
        assert len(parts) == 0 and parts.verify() == []
        parts.ingest(ups2)
        assert parts.verify(verifier_seed=SEED, fp=FP) == [True] * 5
        _, agg = _check_sums(R, parts, ups2, None, d)
        assert agg.tobytes() == _sum_f32(xs2).tobytes()
        # a leg whose kind does not fit the records
        with pytest.raises(R.RoflError) as e:
            R.api.device_round.verify_sigma(parts._h, 0, [u.square_proofs.ctypes.data for u in ups2])
        assert e.value.code == 11
    # after destroy every call is 11
    L, h = R.api.lib(), ctypes.c_uint64(parts._h)
    parts.close()      # (the Python object frees once)
    ok = (ctypes.c_int * 12)()
    prf = (ctypes.c_void_p * 12)(*[u.square_proofs.ctypes.data for u in t])
    assert L.rofl_round_destroy(h) == 11 and L.rofl_round_reset(h) == 11
    assert L.rofl_round_ingest(h, ctypes.c_size_t(1), recs, None) == 11
    assert L.rofl_round_verify_sigma(h, 1, prf, ok, None) == 11
    assert L.rofl_round_verify_range(h, prf, ctypes.c_size_t(608), ctypes.c_size_t(4), ctypes.c_size_t(d), ctypes.c_size_t(8), 32, 7, SEED, ok) == 11
    with R.DeviceAccumulator.unity(d) as a:
        assert L.rofl_round_accumulate(h, ctypes.c_uint64(a._h), None) == 11
    for call in (lambda: parts.verify(), lambda: parts.ingest(ups2[:1]), lambda: parts.reset()):
        with pytest.raises(R.RoflError) as e:
            call()
        assert e.value.code == 11
    # device memory is back (the check of test_gpu_accumulator.py::test_handles_after_destroy_and_no_leak)
    hip_path = next(ln.split()[-1] for ln in open("/proc/self/maps") if "libamdhip64" in ln)
    hip = ctypes.CDLL(hip_path)
    free, total = ctypes.c_size_t(), ctypes.c_size_t()

    def free_now():
        assert hip.hipMemGetInfo(ctypes.byref(free), ctypes.byref(total)) == 0
        return free.value
    for _ in range(3):
        R.DeviceRound(cls, 55000, 12).close()
    f0 = free_now()
    for _ in range(50):
        R.DeviceRound(cls, 55000, 12).close()
    assert abs(free_now() - f0) <= (1 << 20)


def test_records_from_device_memory(R):
    """some clients' records handed over as GPU torch tensors (torch in a child process, as the other device-pointer tests do)"""
    code = r"""
import os, sys
import numpy as np
import torch
torch.cuda.init()
sys.path.insert(0, %r); sys.path.insert(0, %r)
import rofl_project_code_amd as R
import test_gpu_round as T
R.set_device(0); R.api.set_fp(32, 7)
cls, n, d = R.EncParamsRange, 12, 300
xs, ups = T._make_round(R, cls, n, d, 130)
t, what = T._tampered(R, cls, ups, d)
dev = [torch.from_numpy(u.enc_values).cuda() if i %% 3 != 1 else None for i, u in enumerate(t)]
with R.DeviceRound(cls, d, max_clients=n) as host, R.DeviceRound(cls, d, max_clients=n) as mixed:
    host.ingest(t)
    mixed.ingest(t[:1], device_records=dev[:1]); mixed.ingest(t[1:6], device_records=dev[1:6]); mixed.ingest(t[6:], device_records=dev[6:])
    want = host.verify(verifier_seed=T.SEED, fp=T.FP)
    assert mixed.verify(verifier_seed=T.SEED, fp=T.FP) == want == [u.verify(verifier_seed=T.SEED, fp=T.FP) for u in t]
    assert want == [i not in what for i in range(n)]
    a, _ = T._check_sums(R, host, t, want, d)
    b, _ = T._check_sums(R, mixed, t, want, d)
    assert (a == b).all()
print("DEVICE_RECORDS PASS")
""" % (os.path.dirname(os.path.dirname(os.path.abspath(__file__))), os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "DEVICE_RECORDS PASS" in r.stdout, r.stdout + r.stderr[-3000:]


@pytest.mark.parametrize("name", ["range", "l2"])
def test_off_shape_members(R, name):
    """one update with d - 7 records and one with another range-proof count inside a round of ten: each gets its own verify()'s verdict,
    the sum is accumulate_batch's (zip truncation included)"""
    cls = _names(R)[name]
    n, d = 10, 300
    xs, ups = _make_round(R, cls, n, d, 150)
    _, short = _make_round(R, cls, 2, d - 7, 160)
    _, other = _make_round(R, cls, 2, d, 170, P=2)
    ups = ups[:3] + [short[0]] + ups[4:7] + [other[0]] + ups[8:]
    assert ups[3].enc_values.shape[0] == d - 7 and ups[7].range_proofs.shape[0] == 2 != ups[0].range_proofs.shape[0]
    ups = [_copy(u) for u in ups]
    ups[5].range_proofs[0, 40] ^= 1
    try:
        with R.DeviceRound(cls, d, max_clients=n) as rnd:
            rnd.ingest(ups[:4]); rnd.ingest(ups[4:])
            assert rnd._slot[3] is None and rnd._slot[7] is not None
            single = [u.verify(verifier_seed=SEED, fp=FP) for u in ups]
            assert single == [i != 5 for i in range(n)]
            for vb in (2, 1):
                R.set_option("verify_batch", vb)
                assert rnd.verify(verifier_seed=SEED, fp=FP) == cls.verify_batch(ups, verifier_seed=SEED, fp=FP) == single
            _check_sums(R, rnd, ups, single, d)
            _check_sums(R, rnd, ups, None, d)
    finally:
        R.set_option("verify_batch", 1)


def test_an_undecodable_member_outside_the_cache_leaves_the_sum_unchanged(R):
    """all or nothing also when the bad record belongs to a member that cannot sit in the cache (added through accumulate_batch)"""
    cls, n, d = R.EncParamsRange, 6, 300
    xs, ups = _make_round(R, cls, n, d, 180)
    _, short = _make_round(R, cls, 2, d - 7, 185)
    bad = _copy(short[0]); bad.enc_values[5, 32:64] = BAD_POINT
    with R.DeviceRound(cls, d, max_clients=n + 1) as rnd, R.DeviceAccumulator.unity(d) as a, R.DeviceAccumulator.unity(d) as b:
        rnd.ingest(ups + [bad])
        a.accumulate_other(ups[0]); b.accumulate_other(ups[0])
        before = a.export()
        for call in (lambda: rnd.accumulate_into(a), lambda: b.accumulate_batch(ups + [bad])):
            with pytest.raises(R.RoflError) as e:
                call()
            assert e.value.code == 5
        assert (a.export() == before).all() and (b.export() == before).all()
        rnd.accumulate_into(a, accept=[True] * n + [False])
        b.accumulate_batch(ups)
        assert (a.export() == b.export()).all()


@pytest.mark.parametrize("name,check", [("range", 1.0), ("l2", 1.0), ("range", 0.5)])
def test_every_record_point_is_decoded_once(R, name, check):
    """The decode counter around (a) verify_batch + accumulate_batch and (b) ingest + verify + accumulate_into of an honest round (no closer
    look, no MSM retry: nothing is decoded twice on either side).  Counting the clients' records only, (a) decodes L, R for the Sigma leg,
    L for the range leg and L, R for the accumulator (L2: one c_sq more), (b) every point once: the difference is 3 n d (2 n d + n k when
    only the first k are range-checked); the proofs' own points cost the same both ways."""
    cls = _names(R)[name]
    n, d = 6, 300
    k = R.params._num_checked(d, check)
    xs, ups = _make_round(R, cls, n, d, 190, check=check)
    pd = R.api.point_decodes
    assert R.get_option("sigma_batch") == 1 and R.get_option("devices") == 0
    retries = R.api.msm_retries()
    with R.DeviceAccumulator.unity(d) as a, R.DeviceAccumulator.unity(d) as b, R.DeviceRound(cls, d, max_clients=n) as rnd:
        c0 = pd()
        assert cls.verify_batch(ups, verifier_seed=SEED, fp=FP) == [True] * n
        a.accumulate_batch(ups)
        c1 = pd()
        rnd.ingest(ups)
        assert rnd.verify(verifier_seed=SEED, fp=FP) == [True] * n
        rnd.accumulate_into(b)
        c2 = pd()
        assert (a.export() == b.export()).all()
    after = R.api.msm_retries()
    assert all(after[key] == retries[key] for key in after if key != "done")
    npts = 3 if name == "l2" else 2
    assert c2 - c1 >= npts * n * d
    assert (c1 - c0) - (c2 - c1) == (3 * n * d if check == 1.0 else 2 * n * d + n * k), (c0, c1, c2)


@pytest.fixture(scope="module")
def full_size(R):
    """twelve clients of d = 55 000 in BASELINE's cfg-4 shape (EncParamsRange, fp 32/7, 32-bit range, n_partition 4) and cfg-5 shape
    (EncParamsL2, 8-bit L-inf legs, 32-bit sum proofs), one tampered member each; built once for the module"""
    n, d = 12, 55000
    out = {}
    for name, kw in (("range", dict(nb=32, P=4, check=1.0)), ("l2", dict(nb=8, P=4, l2n=32))):
        cls = _names(R)[name]
        xs, ups = _make_round(R, cls, n, d, 210 + len(name), **kw)
        t = [_copy(u) for u in ups]
        if name == "range":
            t[7].rand_proofs[54321, 64 + 9] ^= 1
        else:
            t[3].square_proofs[54321, 128 + 9] ^= 1      # Z_r1 of a late element
        out[name] = (cls, xs, ups, t)
    return out


def _run_round(R, cls, ups, d):
    with R.DeviceRound(cls, d, max_clients=len(ups)) as rnd, R.DeviceAccumulator.unity(d) as a:
        rnd.ingest(ups[:5]); rnd.ingest(ups[5:])
        ok = rnd.verify(verifier_seed=SEED, fp=FP)
        rnd.accumulate_into(a, accept=ok)
        return ok, a.export(), a.extract()


@pytest.mark.parametrize("name", ["range", "l2"])
def test_full_size_round(R, full_size, name):
    cls, xs, ups, t = full_size[name]
    n, d = len(ups), 55000
    bad = 7 if name == "range" else 3
    try:
        R.set_option("verify_batch", 2)
        ok, ex, agg = _run_round(R, cls, ups, d)
        assert ok == [True] * n == cls.verify_batch(ups, verifier_seed=SEED, fp=FP)
        assert agg is not None and agg.tobytes() == _sum_f32(xs).tobytes()
        with R.DeviceAccumulator.unity(d) as b:
            b.accumulate_batch(ups)
            assert (b.export() == ex).all()
        assert (ex == _oracle_fold(d, ups)).all()
        want = [i != bad for i in range(n)]
        for vb in (2, 1):
            R.set_option("verify_batch", vb)
            ok, ex, agg = _run_round(R, cls, t, d)
            assert ok == want == cls.verify_batch(t, verifier_seed=SEED, fp=FP), vb
        assert t[bad].verify(verifier_seed=SEED, fp=FP) is False and agg is None      # a member left out: the blindings do not cancel
        with R.DeviceAccumulator.unity(d) as b:
            b.accumulate_batch([u for u, o in zip(t, want) if o])
            assert (b.export() == ex).all()
        sl = slice(54300, 54340)
        kind, pr = (0, t[bad].rand_proofs) if name == "range" else (1, t[bad].square_proofs)
        assert orc.sigma_verify(kind, pr[sl].copy(), t[bad].enc_values[sl].copy())[1] is False
    finally:
        R.set_option("verify_batch", 1)


def test_two_rounds_from_two_threads(R, full_size):
    """a cfg-4 and a cfg-5 round driven at the same time give the results of running them one after the other"""
    d = 55000
    jobs = [(full_size["range"][0], full_size["range"][3]), (full_size["l2"][0], full_size["l2"][3])]
    try:
        R.set_option("verify_batch", 2)
        want = [_run_round(R, cls, t, d) for cls, t in jobs]
        got, errs = [None, None], []

        def work(i):
            try:
                R.api.bind_device(0)
                R.api.set_fp(*FP)
                got[i] = _run_round(R, jobs[i][0], jobs[i][1], d)
            except Exception as e:      # noqa: BLE001
                errs.append(e)
        ts = [threading.Thread(target=work, args=(i,)) for i in range(2)]
        [th.start() for th in ts]
        [th.join() for th in ts]
        assert not errs, errs
        for g, w in zip(got, want):
            assert g[0] == w[0] and (g[1] == w[1]).all() and g[2] is None and w[2] is None
        assert want[0][0] == [i != 7 for i in range(12)] and want[1][0] == [i != 3 for i in range(12)]
    finally:
        R.set_option("verify_batch", 1)
