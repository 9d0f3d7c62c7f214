"""The compressed randomness leg of a device-resident round (rofl_round_create_ex + ROFL_ROUND_COMPRESSED, rofl_round_verify_compressed,
DeviceRound of EncParamsRangeCompressed): the transcript prefix is hashed at ingest from the bytes that are decoded, the leg continues it over
the cached points.  Verdicts are compared with rofl_verify_compressed_randproof_batch on the same bytes, with cls.verify_batch, with every
update's own verify() and with the oracle; the decode counter shows that the leg neither uploads nor decodes a record.

Rounds are built as in test_gpu_round.py: real encrypt() outputs with nonce seeds whose blindings cancel."""
import ctypes
import threading

import numpy as np
import pytest

import orc
from test_gpu_round import BAD_POINT, FP, SEED, _copy, _make_round, _oracle_fold, _plus_one, _sum_f32

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def R():
    import rofl_project_code_amd as R
    from rofl_project_code_amd import build
    build.build()
    R.set_device(0)
    R.api.set_fp(*FP)
    yield R
    R.set_option("verify_batch", 1)
    R.api.set_fp(*FP)


def _tamper_c(ups, d):
    """one member per tamper kind of the compressed leg; returns (updates, {member: kind}); member 10's proof is to be passed as NULL"""
    t = [_copy(u) for u in ups]
    what = {}
    _plus_one(t[1].rand_proof[64:96]); what[1] = "Z_m + 1"
    t[2].rand_proof[96:128] = 0xFF; what[2] = "non-canonical Z_r"
    t[3].rand_proof[0:32] = BAD_POINT; what[3] = "undecodable C'.L"
    j = min(7, d - 1)
    assert (ups[4].enc_values[j, :32] != ups[5].enc_values[j, :32]).any()
    t[4].enc_values[j, :32] = ups[5].enc_values[j, :32]; what[4] = "a foreign valid L"
    t[6].enc_values[d - 1, :32] = BAD_POINT; what[6] = "undecodable L at d - 1"
    t[7].enc_values[min(9, d - 1), 32:64] = BAD_POINT; what[7] = "undecodable R"
    a, b = t[8].rand_proof.copy(), t[9].rand_proof.copy()
    t[8].rand_proof[:] = b; t[9].rand_proof[:] = a; what[8] = what[9] = "proofs swapped"
    what[10] = "NULL proof"
    return t, what


def _host_batch(R, us):
    return R.compressed_rand_proof.helper_verify_batch([u.rand_proof for u in us], [u.enc_values for u in us])


def _leg(R, h, us, null=()):
    return R.api.device_round.verify_compressed(h, [None if i in null else u.rand_proof.ctypes.data for i, u in enumerate(us)])


def _raw_round(R, us, d, flags=1, pieces=None):
    h = R.api.device_round.create(d, 64, len(us), flags)
    for lo, hi in pieces or [(0, len(us))]:
        assert R.api.device_round.ingest(h, [u.enc_values.ctypes.data for u in us[lo:hi]]) == lo
    return h


# ---- 1. the C leg against the existing call on the same bytes
@pytest.mark.parametrize("d", [1, 7, 300, 5000])
def test_c_leg_equals_the_host_bytes_call(R, d):
    n = 12
    xs, ups = _make_round(R, R.EncParamsRangeCompressed, n, d, 300 + d % 97, P=4 if d >= 8 else 1, check=1.0)
    pd = R.api.point_decodes
    h = _raw_round(R, ups, d)
    try:
        c0 = pd()
        got = _leg(R, h, ups)
        assert pd() == c0                                   # no record and no proof point went to the device's decoder
        print("d", d, "honest", got)
        assert got == _host_batch(R, ups) == [True] * n
        t, what = _tamper_c(ups, d)
        R.api.device_round.reset(h)
        assert R.api.device_round.ingest(h, [u.enc_values.ctypes.data for u in t]) == 0
        c0 = pd()
        got = _leg(R, h, t, null=(10,))
        assert pd() == c0
        want = _host_batch(R, t)
        print("d", d, "tampered", got, want)
        assert want[10] is True                              # (the member left out is an honest one: only the NULL makes it false)
        assert [g for i, g in enumerate(got) if i != 10] == [w for i, w in enumerate(want) if i != 10]
        assert got == [i not in what for i in range(n)]
        assert _leg(R, h, t, null=(10,)) == got              # the call only reads the round
        for i, w in what.items():
            if i != 10:
                rc, ok = orc.compressed_verify(t[i].rand_proof, t[i].enc_values)
                assert not (rc == 0 and ok), w
    finally:
        R.api.device_round.destroy(h)


def test_flag_rules_on_the_device(R):
    d, n = 7, 3
    xs, ups = _make_round(R, R.EncParamsRangeCompressed, n, d, 411, P=1)
    h = _raw_round(R, ups, d, flags=0)
    try:
        with pytest.raises(R.RoflError) as e:
            _leg(R, h, ups)
        assert e.value.code == 11
    finally:
        R.api.device_round.destroy(h)
    with pytest.raises(R.RoflError) as e:
        R.api.device_round.create(d, 96, n, 1)
    assert e.value.code == 11
    h = R.api.device_round.create(d, 64, n, 1)             # a round with no clients: 0, nothing written
    try:
        ok = (ctypes.c_int * 1)(7)
        prf = (ctypes.c_void_p * 1)(ups[0].rand_proof.ctypes.data)
        assert R.api.lib().rofl_round_verify_compressed(ctypes.c_uint64(h), prf, ok) == 0 and ok[0] == 7
    finally:
        R.api.device_round.destroy(h)
    ok = (ctypes.c_int * 1)(7)
    assert R.api.lib().rofl_round_verify_compressed(ctypes.c_uint64(h), prf, ok) == 11 and ok[0] == 7      # destroyed


# ---- 2. no decode, no upload
@pytest.mark.parametrize("check", [1.0, 0.5])
def test_compressed_round_decodes_every_record_point_once(R, check):
    """(a) verify_batch + accumulate_batch decodes L, R for the randomness leg, the first k L for the range leg and L, R for the
    accumulator: 4 n d + n k record points; (b) ingest + verify + accumulate_into decodes every point once: 2 n d.  The proofs' own points
    cost the same both ways, so (a) - (b) = 2 n d + n k."""
    cls = R.EncParamsRangeCompressed
    n, d = 6, 300
    k = R.params._num_checked(d, check)
    xs, ups = _make_round(R, cls, n, d, 190, check=check)
    pd = R.api.point_decodes
    assert R.get_option("devices") == 0
    retries = R.api.msm_retries()
    with R.DeviceAccumulator.unity(d) as a, R.DeviceAccumulator.unity(d) as b, R.DeviceRound(cls, d, max_clients=n) as rnd:
        c0 = pd()
        assert cls.verify_batch(ups, verifier_seed=SEED, fp=FP) == [True] * n
        a.accumulate_batch(ups)
        c1 = pd()
        rnd.ingest(ups)
        c_in = pd()
        assert rnd.verify(verifier_seed=SEED, fp=FP) == [True] * n
        rnd.accumulate_into(b)
        c2 = pd()
        assert _leg(R, rnd._h, ups) == [True] * n
        assert pd() == c2
        assert (a.export() == b.export()).all()
    after = R.api.msm_retries()
    assert all(after[key] == retries[key] for key in after if key != "done")
    print("decodes: host way", c1 - c0, "round", c2 - c1, "of which ingest", c_in - c1, "expected difference", 2 * n * d + n * k)
    assert c_in - c1 == 2 * n * d
    assert (c1 - c0) - (c2 - c1) == 2 * n * d + n * k, (c0, c1, c2)


# ---- 3. the verdict is about the snapshot
def test_the_verdict_is_about_the_ingested_bytes(R):
    cls = R.EncParamsRangeCompressed
    n, d = 6, 300
    xs, ups = _make_round(R, cls, n, d, 520, check=0.5)
    ingested = [_copy(u) for u in ups]
    with R.DeviceRound(cls, d, max_clients=n) as rnd:
        rnd.ingest(ups)
        ups[2].enc_values[5, :32] = ups[3].enc_values[5, :32]      # the caller's memory changes after the ingest
        assert ups[2].verify(verifier_seed=SEED, fp=FP) is False
        got = rnd.verify(verifier_seed=SEED, fp=FP)
        print("after the change in host memory", got)
        assert got == [True] * n
        with R.DeviceAccumulator.unity(d) as a:
            rnd.accumulate_into(a, accept=got)
            ex, agg = a.export(), a.extract()
        assert (ex == _oracle_fold(d, ingested)).all()
        assert agg is not None and agg.tobytes() == _sum_f32(xs).tobytes()
        rnd.reset()
        rnd.ingest(ups)
        got = rnd.verify(verifier_seed=SEED, fp=FP)
        assert got == [i != 2 for i in range(n)] == cls.verify_batch(ups, verifier_seed=SEED, fp=FP)


# ---- 4. every ingest path gives one state
class _DevBytes:
    """the bytes of a numpy array in device memory, with the few methods DeviceRound.ingest asks a device tensor for"""

    def __init__(self, arr):
        path = next(ln.split()[-1] for ln in open("/proc/self/maps") if "libamdhip64" in ln)
        self.hip = ctypes.CDLL(path)
        self.n = arr.size
        self.p = ctypes.c_void_p()
        assert self.hip.hipMalloc(ctypes.byref(self.p), ctypes.c_size_t(self.n)) == 0
        assert self.hip.hipMemcpy(self.p, ctypes.c_void_p(arr.ctypes.data), ctypes.c_size_t(self.n), 1) == 0      # hipMemcpyHostToDevice

    def is_contiguous(self):
        return True

    def element_size(self):
        return 1

    def numel(self):
        return self.n

    def data_ptr(self):
        return self.p.value

    def free(self):
        if self.p:
            assert self.hip.hipFree(self.p) == 0
            self.p = ctypes.c_void_p()


def test_every_ingest_path_gives_the_same_states(R):
    cls = R.EncParamsRangeCompressed
    n, d = 12, 300
    xs, ups = _make_round(R, cls, n, d, 610, check=1.0)
    t, what = _tamper_c(ups, d)
    want_h, want_t = [True] * n, [i not in what for i in range(n)]
    dev = []
    try:
        for us, want, null in ((ups, want_h, ()), (t, want_t, (10,))):
            dev = [_DevBytes(u.enc_values) if i % 3 != 1 else None for i, u in enumerate(us)]
            with R.DeviceRound(cls, d, max_clients=n) as whole, R.DeviceRound(cls, d, max_clients=n) as parts, R.DeviceRound(cls, d, max_clients=n) as mixed:
                whole.ingest(us)
                parts.ingest(us[:5]); parts.ingest(us[5:])
                mixed.ingest(us[:1], device_records=dev[:1]); mixed.ingest(us[1:6], device_records=dev[1:6]); mixed.ingest(us[6:], device_records=dev[6:])
                for rnd in (whole, parts, mixed):
                    got = _leg(R, rnd._h, us, null=null)
                    assert got == want, (got, want)
                    assert _leg(R, rnd._h, us, null=null) == got      # a second call on the same round
                # more than eight (one x8 stream + scalar transcripts) and fewer than five clients (scalar transcripts only)
                for cnt in (11, 9, 8, 5, 4, 1):
                    whole.reset()
                    whole.ingest(us[:cnt])
                    assert _leg(R, whole._h, us[:cnt], null=null) == want[:cnt], cnt
                # after reset() the round is reusable: the other list's states replace these
                parts.reset()
                assert R.api.device_round.verify_compressed(parts._h, []) == []
                other = ups if us is t else t
                parts.ingest(other)
                assert _leg(R, parts._h, other, null=() if us is t else (10,)) == (want_h if us is t else want_t)
            for x in dev:
                if x is not None:
                    x.free()
            dev = []
    finally:
        for x in dev:
            if x is not None:
                x.free()


# ---- 5. side by side with the range leg
def test_compressed_and_range_legs_from_two_threads(R):
    cls = R.EncParamsRangeCompressed
    n, d, check = 12, 5000, 0.5
    k = R.params._num_checked(d, check)
    xs, ups = _make_round(R, cls, n, d, 700, check=check)
    t, what = _tamper_c(ups, d)
    t[11].range_proofs[1, 7 * 32 + 33] ^= 2
    rp = t[0].range_proofs
    h = _raw_round(R, t, d)

    def range_leg():
        return R.api.device_round.verify_range(h, [u.range_proofs.ctypes.data for u in t], rp.shape[1], rp.shape[0], k, t[0].prove_range, verifier_seed=SEED, fp=FP)
    try:
        R.set_option("verify_batch", 2)
        want_c, want_r = _leg(R, h, t, null=(10,)), range_leg()
        assert want_c == [i not in what for i in range(n)]
        assert want_r == [i not in (4, 11) for i in range(n)]      # the foreign L sits below k; the bad L at d - 1 does not
        for _ in range(3):
            got, errs = [None, None], []

            def work(i):
                try:
                    R.api.bind_device(0)
                    R.api.set_fp(*FP)
                    got[i] = _leg(R, h, t, null=(10,)) if i == 0 else range_leg()
                except Exception as e:      # noqa: BLE001
                    errs.append(e)
            ts = [threading.Thread(target=work, args=(i,)) for i in range(2)]
            [th.start() for th in ts]
            [th.join() for th in ts]
            assert not errs, errs
            assert got == [want_c, want_r]
    finally:
        R.set_option("verify_batch", 1)
        R.api.device_round.destroy(h)


# ---- 6. full size: the shape of the reference's end-to-end experiments
E2E_FP = (16, 7)


@pytest.fixture(scope="module")
def e2e_round(R):
    """twelve clients of d = 40 000, fp 16/7, 8-bit range, n_partition 64, check_percentage 0.013 (k = 520); member 4 with a tampered pair
    far beyond k, member 9 with a tampered proof; built once for the module"""
    n, d = 12, 40000
    R.api.set_fp(*E2E_FP)
    try:
        rng = np.random.default_rng(805)
        xs = [(rng.integers(-3, 4, size=d) / 128.0).astype(np.float32) for _ in range(n)]
        bls = []
        for _ in range(n - 1):
            b = rng.integers(0, 256, size=(d, 32), dtype=np.uint8); b[:, 31] &= 0x0F
            bls.append(b)
        bls.append(R.pedersen_ops.add_scalar_vec(np.zeros((d, 32), np.uint8), R.pedersen_ops.add_scalar_vec_vec(bls), subtract=True))
        ups = [R.EncParamsRangeCompressed.encrypt(x, b, 8, 64, 0.013, nonce_seed=bytes([i + 1]) * 32, fp=E2E_FP) for i, (x, b) in enumerate(zip(xs, bls))]
    finally:
        R.api.set_fp(*FP)
    t = [_copy(u) for u in ups]
    t[4].enc_values[39123, 32:64] = ups[5].enc_values[39123, 32:64]      # a late pair with a foreign (valid) R
    _plus_one(t[9].rand_proof[96:128])                                    # Z_r + 1
    return xs, ups, t


def test_full_size_compressed_round(R, e2e_round):
    cls = R.EncParamsRangeCompressed
    xs, ups, t = e2e_round
    n, d = len(ups), 40000
    assert R.params._num_checked(d, 0.013) == 520

    def run(us):
        with R.DeviceRound(cls, d, max_clients=n) as rnd, R.DeviceAccumulator.unity(d) as a:
            rnd.ingest(us[:5]); rnd.ingest(us[5:])
            ok = rnd.verify(verifier_seed=SEED, fp=E2E_FP)
            rnd.accumulate_into(a, accept=ok)
            return ok, a.export(), a.extract(fp=E2E_FP)
    try:
        R.api.set_fp(*E2E_FP)
        R.set_option("verify_batch", 2)
        ok, ex, agg = run(ups)
        assert ok == [True] * n == cls.verify_batch(ups, verifier_seed=SEED, fp=E2E_FP)
        assert agg is not None and agg.tobytes() == _sum_f32(xs).tobytes()
        want = [i not in (4, 9) for i in range(n)]
        ok, ex, agg = run(t)
        single = [u.verify(verifier_seed=SEED, fp=E2E_FP) for u in t]
        print("full size", ok, single)
        assert ok == cls.verify_batch(t, verifier_seed=SEED, fp=E2E_FP) == single == want
        accepted = [u for u, o in zip(t, want) if o]
        with R.DeviceAccumulator.unity(d) as b:
            b.accumulate_batch(accepted)
            assert (b.export() == ex).all()
        for i in (4, 9):
            rc, o = orc.compressed_verify(t[i].rand_proof, t[i].enc_values)
            assert not (rc == 0 and o)
        assert agg is None      # two members are left out: the blindings of the accepted no longer cancel (the honest round's sum extracted above)
    finally:
        R.set_option("verify_batch", 1)
        R.api.set_fp(*FP)

