"""The wide discrete-log solver (bsgs_bits 24 and 40: k_wdlog_build / k_wdlog_solve) against tests/bsgs_model.py, byte for byte.

Its hash key (x y)^2 has to be constant on a Ristretto class whatever representative the decoder hands over, so the inputs are the table
edges and the +-j m values of tests/test_gpu_torsion.py (chosen for their decode shifts), filled up to d = 67 with seeded logs."""
import random

import numpy as np
import pytest

import bsgs_model as BM
import torsion_corpus as TC

pytestmark = pytest.mark.gpu
pyref = TC.pyref
CASES = [(1 << 10, 24), (3000, 24), (1 << 20, 40)]
IDS = ["m%d-bits%d" % c for c in CASES]
D = 67
FP = (32, 7)


@pytest.fixture(scope="module")
def R():
    import rofl_project_code_amd as R
    from rofl_project_code_amd import build
    build.build()
    R.set_device(0)
    return R


def _points(vs):
    return np.frombuffer(b"".join(pyref.ristretto_encode(TC.mul_base(v)) for v in vs), np.uint8).reshape(-1, 32).copy()


def _ints(rows):
    return [int.from_bytes(r.tobytes(), "little") for r in rows]


def _code(R, call):
    with pytest.raises(R.RoflError) as e:
        call()
    return e.value.code


@pytest.mark.parametrize("m,bits", CASES, ids=IDS)
def test_wide_discrete_log_matches_the_model(R, m, bits):
    rng = random.Random(m * 64 + bits)
    far, near = -((BM.max_it(m, bits) - 1) * m + 5), 3
    edges = BM.values(m, bits, TC.decode_shift)
    want = {v: BM.solve(v, m, bits) for v in edges + [far, near]}      # (the model walks in Python: once per value)
    vs = [v for v in edges if want[v] is not None]
    while len(vs) < D:
        v = rng.randrange(1 << bits) * rng.choice((1, -1))
        want[v] = BM.solve(v, m, bits)
        if want[v] is not None and v not in vs:
            vs.append(v)
    assert len({TC.decode_shift(v) for v in vs}) >= 3
    got = R.pedersen_ops.discrete_log_vec(_points(vs), m, bits)
    assert _ints(got) == [want[v] for v in vs]
    # 67 copies of a hit at the far end of the walk and one near point: the walkers that share a point agree on its hit
    got = R.pedersen_ops.discrete_log_vec(_points([far] * D + [near]), m, bits)
    assert _ints(got) == [want[far]] * D + [want[near]]
    for v in (BM.unreachable(m, bits), -BM.unreachable(m, bits)):
        assert _code(R, lambda: R.pedersen_ops.discrete_log_vec(_points([v]), m, bits)) == 11
    bad = _points([5, 6, 7])
    bad[1] = 0xFF      # s >= p: not canonical
    assert _code(R, lambda: R.pedersen_ops.discrete_log_vec(bad, m, bits)) == 5


def test_accumulator_extracts_sums_beyond_16_bits(R):
    """three clients, d = 40, fp (32, 7): raw sums up to 3 * 300 * 128 > 2^16 with both signs, and small ones beside them"""
    d, m = 40, 1 << 10
    rng = np.random.default_rng(24)
    raw = np.stack([rng.choice((-1, 1), size=d) * rng.integers(290 * 128, 300 * 128, size=d) for _ in range(3)])
    raw[:, ::4] = rng.integers(-50, 50, size=raw[:, ::4].shape)      # every fourth coordinate stays below 16 bits
    raw[:, 1], raw[:, 2] = 299 * 128, -299 * 128
    xs = [(r / 128.0).astype(np.float32) for r in raw]
    total = raw.sum(axis=0)
    assert (abs(total) > 1 << 16).sum() >= 8 and (total < -(1 << 16)).any() and (abs(total) < 1 << 16).sum() >= 10
    bls = [rng.integers(0, 256, size=(d, 32), dtype=np.uint8) for _ in range(2)]
    for b in bls:
        b[:, 31] &= 0x0F
    bls.append(R.pedersen_ops.add_scalar_vec(np.zeros((d, 32), np.uint8), R.pedersen_ops.add_scalar_vec_vec(bls), subtract=True))
    want = np.sum(np.stack(xs).astype(np.float64), axis=0).astype(np.float32)
    with R.DeviceAccumulator.unity(d) as dev:
        for x, b in zip(xs, bls):
            msg = R.conversion32.f32_to_scalar_vec(x, fp=FP)
            pairs = np.ascontiguousarray(np.concatenate([R.pedersen_ops.commit_vec(msg, b), R.pedersen_ops.commit_no_blinding_vec(b)], axis=1))
            assert dev.accumulate_pairs(pairs)
        got = dev.extract(m, 24, FP)
        assert got is not None and got.tobytes() == want.tobytes()
        assert dev.extract_opened(opening=np.zeros((d, 32), np.uint8), table_size=m, bsgs_bits=24, fp=FP).tobytes() == want.tobytes()
        # at width 16 the model finds no log for the wide coordinates: the reference's None, error 11
        assert any(BM.solve(int(t), m, 16) is None for t in total)
        assert _code(R, lambda: dev.extract(m, 16, FP)) == 11
