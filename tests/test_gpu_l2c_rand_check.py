"""The opt-in check of the CompressedRandProof of EncL2Compressed updates: rofl_verify_compressed_randproof_batch_strided over 96-byte
SquareRandProofCommitments records in place, rofl_round_create_rand + rofl_round_verify_compressed over a device-resident round of them,
EncParamsL2CompressedStrict and DeviceRound of it.

The reference's EncL2Compressed arm (params.rs:257-289) never reads rand_proof, so nothing there constrains R: every forgery of R below
passes EncParamsL2Compressed -- asserted, that verdict must stay -- and is rejected, for that member alone, by the strict class.

Shapes as in test_gpu_encrypt_batch.py: prove_range 8, n_partition 2, l2_range 32, fp (32, 7); containers from encrypt_batch with fixed
nonce seeds."""
import numpy as np
import pytest

import orc
from test_gpu_round import BAD_POINT, ELL, FP, SEED, _sum_f32

pytestmark = pytest.mark.gpu
NB, P, L2N = 8, 2, 32
D, N = 70, 6


@pytest.fixture(scope="module")
def R():
    import rofl_project_code_amd as R
    from rofl_project_code_amd import build
    build.build()
    R.set_device(0)
    R.api.set_fp(*FP)
    yield R
    R.set_option("devices", 0)
    R.api.set_fp(*FP)


def _scalars(rng, d):
    b = rng.integers(0, 256, size=(d, 32), dtype=np.uint8); b[:, 31] &= 0x0F      # < 2^252: canonical
    return b


def _encrypt(R, cls, n, d, seed0, bls=None):
    """n updates of class cls from ONE encrypt_batch (values k / 128, |k| <= 3: exact at 7 fraction bits); returns (values, updates)"""
    rng = np.random.default_rng(seed0)
    xs = [(rng.integers(-3, 4, size=d) / 128.0).astype(np.float32) for _ in range(n)]
    bls = [_scalars(rng, d) for _ in range(n)] if bls is None else bls
    cl = [(x, b, _scalars(rng, d)) for x, b in zip(xs, bls)]
    ups = cls.encrypt_batch(cl, NB, P, L2N, nonce_seeds=[bytes([(seed0 + i) % 251 + 1]) * 32 for i in range(n)], fp=FP)
    assert all(type(u) is cls for u in ups)
    return xs, ups


def _as(cls, u):
    """the same bytes as an update of class cls (a copy: the wire round trip)"""
    return cls.deserialize(u.serialize())


def _point(R, k):
    """k B as 32 bytes (commit_no_blinding_vec of the scalar k mod l)"""
    s = np.frombuffer((k % ELL).to_bytes(32, "little"), np.uint8).reshape(1, 32)
    return R.pedersen_ops.commit_no_blinding_vec(s).reshape(32)


# the forgeries of R that every leg of the reference's arm lets through, and the two of the proof itself
def _f_replace(R, u):
    assert (u.enc_values[3, 32:64] != u.enc_values[11, 32:64]).any()
    u.enc_values[3, 32:64] = u.enc_values[11, 32:64]


def _f_swap(R, u):
    a = u.enc_values[5, 32:64].copy()
    assert (a != u.enc_values[60, 32:64]).any()
    u.enc_values[5, 32:64] = u.enc_values[60, 32:64]; u.enc_values[60, 32:64] = a


def _f_cancel(R, u):
    """R_j + B and R_k - B: the errors cancel in an unweighted sum of the R (and in the round's aggregate they do not: j != k)"""
    both = R.pedersen_ops.add_rp_vec(np.stack([u.enc_values[2, 32:64], u.enc_values[69, 32:64]]), np.stack([_point(R, 1), _point(R, -1)]))
    u.enc_values[2, 32:64] = both[0]; u.enc_values[69, 32:64] = both[1]


def _f_zr(R, u):
    z = int.from_bytes(u.rand_proof[96:128].tobytes(), "little") + ELL      # the same residue, not canonical
    u.rand_proof[96:128] = np.frombuffer(z.to_bytes(32, "little"), np.uint8)


def _f_cprime(R, u):
    u.rand_proof[32:64] = BAD_POINT


R_FORGERIES = {"R_j replaced by R_k": _f_replace, "R_j and R_k swapped": _f_swap, "R_j + B, R_k - B": _f_cancel}
PROOF_FORGERIES = {"Z_r + l": _f_zr, "C'.R undecodable": _f_cprime}


@pytest.fixture(scope="module")
def honest(R):
    """N honest strict updates of D elements, built once and never changed (the tests copy them)"""
    return _encrypt(R, R.EncParamsL2CompressedStrict, N, D, 2100)


# ---- 1. the strided call against the dense call and the oracle
_PROOFS = {}


def _proofs(R, d):
    """17 (proof, pairs) of helper_prove per d, made once; members 1, 3 and 16 are forged where d allows: a wrong proof scalar, R_0 and
    R_{d-1} swapped, an undecodable L in the last pair (member 16 is the second group of 17, a group of one)"""
    if d not in _PROOFS:
        rng = np.random.default_rng(3000 + d)
        out = []
        for i in range(17):
            x = (rng.integers(-3, 4, size=d) / 128.0).astype(np.float32)
            pf, pr = R.compressed_rand_proof.helper_prove(x, _scalars(rng, d), nonce=R.Nonce.seeded(bytes([i + 1]) * 32), fp=FP)
            out.append((pf.copy(), np.ascontiguousarray(pr).copy()))
        out[1][0][64] ^= 1                                     # Z_m
        if d >= 2:
            a = out[3][1][0, 32:64].copy(); out[3][1][0, 32:64] = out[3][1][d - 1, 32:64]; out[3][1][d - 1, 32:64] = a
        if d >= 1:
            out[16][1][d - 1, :32] = BAD_POINT
        _PROOFS[d] = out
    return _PROOFS[d]


@pytest.mark.parametrize("filler", ["0xFF", "random"])
@pytest.mark.parametrize("n", [1, 2, 17])
@pytest.mark.parametrize("d", [0, 1, 127, 128, 129])
def test_strided_call_equals_the_dense_call_and_the_oracle(R, d, n, filler):
    """2 d threads per client: d = 127, 128, 129 straddle one block of 256; n = 17 is a second group, of one.  The 0xFF filler is an
    undecodable c_sq in every record, which this call must never read."""
    H = R.compressed_rand_proof
    sel = _proofs(R, d)[17 - n:]                               # (the last n: the forged member 16 is in every selection)
    pf, pr = [p for p, _ in sel], [c for _, c in sel]
    rng = np.random.default_rng(d * 31 + n)
    recs = []
    for c in pr:
        fill = np.full((d, 32), 0xFF, np.uint8) if filler == "0xFF" else rng.integers(0, 256, size=(d, 32), dtype=np.uint8)
        recs.append(np.ascontiguousarray(np.concatenate([c.reshape(d, 64), fill], axis=1)))
    want = H.helper_verify_batch(pf, pr)
    got96 = H.helper_verify_batch_strided(pf, recs, 96)
    got64 = H.helper_verify_batch_strided(pf, pr, 64)
    print("d", d, "n", n, filler, got96)
    assert got96 == want and got64 == want
    for i in range(n):
        rc, ok = orc.compressed_verify(pf[i], pr[i])
        assert bool(rc == 0 and ok) == want[i], i
    forged = {1} | ({16} if d >= 1 else set()) | ({3} if d >= 2 else set())
    assert want == [m not in forged for m in range(17 - n, 17)]


# ---- 2. forgeries
@pytest.mark.parametrize("name", list(R_FORGERIES) + list(PROOF_FORGERIES))
def test_the_strict_class_rejects_the_forger_alone(R, honest, name):
    S, B = R.EncParamsL2CompressedStrict, R.EncParamsL2Compressed
    strict = [_as(S, u) for u in honest[1]]
    (R_FORGERIES.get(name) or PROOF_FORGERIES[name])(R, strict[2])
    loose = [_as(B, u) for u in strict]
    assert all(type(u) is B for u in loose) and all(type(u) is S for u in strict)
    got_loose = B.verify_batch(loose, verifier_seed=SEED, fp=FP)
    print(name, "reference-faithful:", got_loose, loose[2].verify(verifier_seed=SEED, fp=FP))
    # the reference's arm never reads the proof and none of its legs reads R: unchanged, the forger passes
    assert got_loose == [True] * N and loose[2].verify(verifier_seed=SEED, fp=FP) is True
    want = [i != 2 for i in range(N)]
    got = S.verify_batch(strict, verifier_seed=SEED, fp=FP)
    print(name, "strict:", got)
    assert got == want
    assert strict[2].verify(verifier_seed=SEED, fp=FP) is False and strict[1].verify(verifier_seed=SEED, fp=FP) is True
    rc, ok = orc.compressed_verify(strict[2].rand_proof, strict[2].enc_values[:, :64])
    assert not (rc == 0 and ok)


# ---- 3. honest updates and the wire round trip
def test_honest_updates_pass_every_way_and_round_trip(R, honest):
    S = R.EncParamsL2CompressedStrict
    ups = honest[1]
    single = [u.verify(verifier_seed=SEED, fp=FP) for u in ups]
    batch = S.verify_batch(ups, verifier_seed=SEED, fp=FP)
    with R.DeviceRound(S, D, max_clients=N) as rnd:
        rnd.ingest(ups[:2]); rnd.ingest(ups[2:])
        dev = rnd.verify(verifier_seed=SEED, fp=FP)
    assert single == batch == dev == [True] * N
    for u in ups:
        v = S.deserialize(u.serialize())
        assert type(v) is S and v.serialize() == u.serialize()
        assert (v.enc_values == u.enc_values).all() and (v.rand_proof == u.rand_proof).all() and (v.square_proofs == u.square_proofs).all()
        assert R.EncParamsL2Compressed.deserialize(u.serialize()).serialize() == u.serialize()      # the same wire kind, the same bytes
        rc, ok = orc.compressed_verify(u.rand_proof, u.enc_values[:, :64])
        assert rc == 0 and ok


# ---- 4. the strict DeviceRound
def test_strict_round_equals_strict_verify_batch(R, honest):
    """the forgeries above, a member of another d (outside the cache) and a member with a 127-byte proof (off the majority shape)"""
    S = R.EncParamsL2CompressedStrict
    ups = [_as(S, u) for u in honest[1]]
    for i, f in zip((0, 1, 2), R_FORGERIES.values()):
        f(R, ups[i])
    _f_zr(R, ups[3])
    other = _encrypt(R, S, 2, 33, 2200)[1]
    _f_cprime(R, other[1])
    ups += other
    short = _as(S, honest[1][5]); short.rand_proof = short.rand_proof[:127].copy()
    ups.append(short)
    want = [False, False, False, False, True, True, True, False, False]
    assert S.verify_batch(ups, verifier_seed=SEED, fp=FP) == want
    with R.DeviceRound(S, D, max_clients=len(ups)) as rnd:
        rnd.ingest(ups)
        assert rnd._compressed and rnd._n_cached == 7
        got = rnd.verify(verifier_seed=SEED, fp=FP)
        print("strict round", got)
        assert got == want
        # the C leg on the cache against the host-bytes strided call on the same bytes
        cached = [u for u, sl in zip(ups, rnd._slot) if sl is not None and u.rand_proof.size == 128]
        leg = R.api.device_round.verify_compressed(rnd._h, [u.rand_proof.ctypes.data if u.rand_proof.size == 128 else None for u, sl in zip(ups, rnd._slot) if sl is not None])
        host = R.compressed_rand_proof.helper_verify_batch_strided([u.rand_proof for u in cached], [u.enc_values for u in cached], 96)
        assert leg[:len(cached)] == host == [False, False, False, False, True, True]
    # the reference-faithful round of the same bytes is as it was: it hashes nothing and cannot run the leg
    B = R.EncParamsL2Compressed
    loose = [_as(B, u) for u in ups[:6]]
    with R.DeviceRound(B, D, max_clients=6) as rnd:
        rnd.ingest(loose)
        assert not rnd._compressed
        assert rnd.verify(verifier_seed=SEED, fp=FP) == [True] * 6
        with pytest.raises(R.RoflError) as e:
            R.api.device_round.verify_compressed(rnd._h, [u.rand_proof.ctypes.data for u in loose])
        assert e.value.code == 11


def test_the_randomness_leg_decodes_no_record_point(R, honest):
    S, B = R.EncParamsL2CompressedStrict, R.EncParamsL2Compressed
    ups = honest[1]
    loose = [_as(B, u) for u in ups]
    pd = R.api.point_decodes
    counts = []
    for cls, us in ((B, loose), (S, ups)):
        with R.DeviceRound(cls, D, max_clients=N) as rnd, R.DeviceAccumulator.unity(D) as a:
            c0 = pd()
            rnd.ingest(us)
            c1 = pd()
            assert rnd.verify(verifier_seed=SEED, fp=FP) == [True] * N
            rnd.accumulate_into(a)
            counts.append((c1 - c0, pd() - c0))
            if cls is S:
                c2 = pd()
                assert R.api.device_round.verify_compressed(rnd._h, [u.rand_proof.ctypes.data for u in us]) == [True] * N
                assert pd() == c2
    print("decodes (ingest, ingest + verify + accumulate): reference-faithful", counts[0], "strict", counts[1])
    assert counts[0][0] == counts[1][0] == 3 * N * D
    assert counts[0] == counts[1]


def test_an_undecodable_R_fails_the_randomness_leg_alone(R, honest):
    S, B = R.EncParamsL2CompressedStrict, R.EncParamsL2Compressed
    ups = [_as(S, u) for u in honest[1]]
    ups[4].enc_values[9, 32:64] = BAD_POINT
    ups[1].enc_values[11, 64:96] = BAD_POINT      # an undecodable c_sq: the Sigma leg's failure, not the randomness leg's
    want = [i not in (1, 4) for i in range(N)]
    assert B.verify_batch([_as(B, u) for u in ups], verifier_seed=SEED, fp=FP) == [i != 1 for i in range(N)]      # R is never read there
    with R.DeviceRound(S, D, max_clients=N) as rnd:
        rnd.ingest(ups)
        ok = rnd.verify(verifier_seed=SEED, fp=FP)
        assert ok == want == S.verify_batch(ups, verifier_seed=SEED, fp=FP)
        sig, _ = R.api.device_round.verify_sigma(rnd._h, 2, [u.square_proofs.ctypes.data for u in ups], want_csq=True)
        rp = ups[0].range_proofs
        rng_leg = R.api.device_round.verify_range(rnd._h, [u.range_proofs.ctypes.data for u in ups], rp.shape[1], rp.shape[0], D, NB, verifier_seed=SEED, fp=FP)
        comp = R.api.device_round.verify_compressed(rnd._h, [u.rand_proof.ctypes.data for u in ups])
        print("sigma", sig, "range", rng_leg, "compressed", comp)
        assert sig == [i != 1 for i in range(N)] and rng_leg == [True] * N and comp == [i != 4 for i in range(N)]
        with R.DeviceAccumulator.unity(D) as a, R.DeviceAccumulator.unity(D) as b:
            assert rnd.accumulate_into(a, accept=ok)
            b.accumulate_batch([u for u, o in zip(ups, ok) if o])
            assert (a.export() == b.export()).all()
            with pytest.raises(R.RoflError) as e:      # accepting the member anyway is still all or nothing
                rnd.accumulate_into(a, accept=[True] * N)
            assert e.value.code == 5
            assert (a.export() == b.export()).all()


def test_the_strict_verdict_is_about_the_ingested_bytes(R, honest):
    S = R.EncParamsL2CompressedStrict
    ups = [_as(S, u) for u in honest[1]]
    with R.DeviceRound(S, D, max_clients=N) as rnd:
        rnd.ingest(ups)
        _f_swap(R, ups[2])                          # the caller's memory changes after the ingest
        assert ups[2].verify(verifier_seed=SEED, fp=FP) is False
        assert rnd.verify(verifier_seed=SEED, fp=FP) == [True] * N
        rnd.reset()
        rnd.ingest(ups)
        assert rnd.verify(verifier_seed=SEED, fp=FP) == [i != 2 for i in range(N)]


# ---- 5. end to end: the round the forger would have cost
def test_end_to_end_the_forger_no_longer_costs_the_round(R):
    S, B = R.EncParamsL2CompressedStrict, R.EncParamsL2Compressed
    d = 65
    rng = np.random.default_rng(2300)
    bls = list(R.pedersen_ops.generate_cancelling_scalar_vec(4, d)) + [_scalars(rng, d)]
    xs, ups = _encrypt(R, S, 5, d, 2301, bls=[np.ascontiguousarray(b) for b in bls])
    ups = [_as(S, u) for u in ups]
    ups[4].enc_values[7, 32:64] = ups[4].enc_values[8, 32:64]      # the forger (a blinding of its own): a wrong (valid) R
    loose = [_as(B, u) for u in ups]
    with R.DeviceRound(B, d, max_clients=5) as rnd, R.DeviceAccumulator.unity(d) as a:
        rnd.ingest(loose)
        ok = rnd.verify(verifier_seed=SEED, fp=FP)
        assert ok == [True] * 5                     # the reference's arm accepts all five
        rnd.accumulate_into(a, accept=ok)
        assert a.extract(fp=FP) is None             # and the round is lost
    with R.DeviceRound(S, d, max_clients=5) as rnd, R.DeviceAccumulator.unity(d) as a:
        rnd.ingest(ups)
        ok = rnd.verify(verifier_seed=SEED, fp=FP)
        assert ok == [True, True, True, True, False] == S.verify_batch(ups, verifier_seed=SEED, fp=FP)
        rnd.accumulate_into(a, accept=ok)
        agg = a.extract(fp=FP)
    assert agg is not None and list(agg) == list(_sum_f32(xs[:4]))
    # the host accumulator over the accepted updates agrees
    acc = R.EncModelParamsAccumulator.unity(d)
    for u, o in zip(ups, ok):
        if o:
            acc.accumulate_other(u)
    assert list(acc.extract(fp=FP)) == list(agg)


# ---- 6. the `devices` option
def test_strided_call_over_two_logical_devices(R):
    """rofl_set_option("devices", 0b11) with logical device 1 mapped onto HIP device 0: five clients dealt round-robin, the verdicts of
    the one-device call"""
    d = 129
    sel = _proofs(R, d)[12:]                        # members 12 .. 16; 16 is forged
    pf = [p for p, _ in sel]
    recs = [np.ascontiguousarray(np.concatenate([c, np.full((d, 32), 0xFF, np.uint8)], axis=1)) for _, c in sel]
    H = R.compressed_rand_proof
    one = H.helper_verify_batch_strided(pf, recs, 96)
    assert one == [True, True, True, True, False]
    R.api.map_device(1, 0)
    try:
        R.set_option("devices", 0b11)
        assert H.helper_verify_batch_strided(pf, recs, 96) == one
    finally:
        R.set_option("devices", 0)
