"""Norm clipping ON THE DEVICE (rofl_clip_l2: k_clip_l2_sumsq, k_clip_l2_apply / _seeded) against the Python model of
tests/l2clip_model.py, byte for byte: the grid of the host test, the shapes only the kernels can get wrong (the edges of a wave's 2 048
elements, more elements than one pass of the reduction grid, fewer elements than it has blocks) with three vectors per launch that take
the three branches, the 192-bit sums, trunc24, step 4 as the device compiles it, the memory spaces, and whole updates through the L2
containers: an update over the norm bound fails today, passes with l2_clip, and a round of clipped updates aggregates to the sum of the
model's clipped vectors.

A call whose pointers are all host memory and which is small runs on the host (the threshold is the library's); the tests that mean the
kernels go through rofl_dbg_clip_l2_route(1, ...) or hand in device memory, which always takes the kernels."""
import os
import subprocess
import sys

import numpy as np
import pytest

import l2clip_model as M
import pq_model
from test_l2_clip_host import (D_HOST, FORMATS, GRID_SEEDS, SEED, check_bound, check_grid, check_square_scale, check_trunc, check_wide, clip_call, dbg_round,
                               grid_cases, inputs)

pytestmark = pytest.mark.gpu
D_KERNEL = (5, 63, 64, 65, 2047, 2048, 2049, 4100)


@pytest.fixture(scope="module")
def R():
    import rofl_project_code_amd as R
    from rofl_project_code_amd import build
    build.build()
    R.set_device(0)     # fails loudly when there is no HIP device / library
    yield R
    R.api.set_fp(16, 7)


@pytest.mark.parametrize("seeded", (False, True), ids=("truncated", "seeded"))
@pytest.mark.parametrize("nb,fb,ff", FORMATS, ids=["r%d_fp%d_%d" % f for f in FORMATS])
def test_kernels_equal_the_model_on_the_host_grid(R, nb, fb, ff, seeded):
    """the grid of the host test (the model's outputs are computed once for both tests)"""
    check_grid(R.lib(), 1, nb, fb, ff, seeded, D_HOST)


@pytest.mark.parametrize("nb,fb,ff,seeded", ((32, 32, 7, False), (32, 32, 7, True), (8, 8, 7, True)), ids=("fp32_7", "fp32_7_seeded", "fp8_7_seeded"))
def test_shapes_only_the_kernels_can_get_wrong(R, nb, fb, ff, seeded):
    """d = 5 (fewer elements than the reduction grid has blocks), 63 / 64 / 65 (a wave), 2047 / 2048 / 2049 (the elements of one block of
    the scaling kernel, and one pass of the 2 048 threads of the reduction grid) and 4100 (three blocks, more than two passes); the three
    vectors of a launch fit, are scaled and are sent to zero, so the blocks of one grid take all three branches"""
    check_grid(R.lib(), 1, nb, fb, ff, seeded, D_KERNEL, variants=(1,))      # (S = T and S = T + 1 are on the host grid above)


def test_wide_sums_trunc24_and_square_scales_on_the_device(R):
    check_wide(R.lib(), 1)
    check_trunc(R.lib(), 1)
    check_square_scale(R.lib(), 1)


def test_device_rounding_equals_the_host_rounding(R):
    """rofl_dbg_clip_l2_round: site 1 (one thread per case) against site 0 and the model, on 64-bit steps, every kind of word and scale"""
    rng = np.random.default_rng(77)
    q = [0, 1, 2, (1 << 24) - 1, 1 << 24, (1 << 24) + 1, (1 << 32) - 1, 1 << 32, (1 << 63), (1 << 64) - 1] + [int(v) for v in rng.integers(0, 1 << 63, 54, dtype=np.uint64) >> rng.integers(0, 63, 54, dtype=np.uint64)]
    for m in (0, 1, 1 << 31, 0x9e3779b9, (1 << 32) - 1):
        for words in (None, [0] * len(q), [0xffffffff] * len(q), [int(w) for w in rng.integers(0, 1 << 32, len(q))]):
            dev = dbg_round(R.lib(), 1, q, m, words, 7)
            assert dev == dbg_round(R.lib(), 0, q, m, words, 7) == [M.round_steps(v, m, None if words is None else w) for v, w in zip(q, words or q)], (m, words is None)


def test_host_route_equals_device_route(R):
    nb, fb, ff = 16, 16, 7
    d = 5000
    rng = np.random.default_rng(33)
    vals = [inputs(rng, d, nb, fb, ff) for _ in range(3)]
    S = [M.sum_sq(x, nb, fb, ff) for x in vals]
    T = [S[0], S[1] // 2, 71 ** 2]
    for seeds in (None, b"".join(GRID_SEEDS)):
        res = []
        for route in (1, 0, None):
            outs = [np.full(d, np.nan, np.float32) for _ in range(3)]
            rc, scale = clip_call(R.lib(), route, seeds, vals, d, T, nb, fb, ff, outs)
            assert rc == 0
            res.append((b"".join(o.tobytes() for o in outs), scale))
        assert res[0] == res[1] == res[2]
        got = np.frombuffer(res[0][0], np.float32).reshape(3, d)
        want = M.clip_l2(vals[1], T[1], nb, fb, ff, GRID_SEEDS[1] if seeds else None)
        assert got[1].tobytes() == want[0].tobytes() and res[0][1][1] == want[1] and res[0][1][0] == M.ONE
        for v in range(3):
            check_bound(got[v], T[v], nb, fb, ff)


def test_memory_spaces_and_in_place(R):
    """host memory in place through the kernels here; host and device vectors mixed within one call of three, device in place and the
    Python wrappers over GPU tensors in tests/gpu_l2_clip_device_check.py (torch in a child process, as the other device-pointer tests do)"""
    nb, fb, ff = 16, 16, 7
    h = inputs(np.random.default_rng(12), 257, nb, fb, ff)
    T = M.sum_sq(h, nb, fb, ff) // 2
    want = M.clip_l2(h, T, nb, fb, ff, SEED)[0].tobytes()
    assert clip_call(R.lib(), 1, SEED, [h], 257, [T], nb, fb, ff, [h])[0] == 0
    assert h.tobytes() == want
    r = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "gpu_l2_clip_device_check.py")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "L2_CLIP_DEVICE PASS" in r.stdout, r.stdout + r.stderr[-3000:]


# ---------------------------------------------------------------- whole updates and a whole round through the L2 containers
FP, NB, D, L2N, P, N_CLIENTS = (32, 7), 8, 70, 16, 2, 3
QSEEDS = [bytes([c + 1]) * 32 for c in range(N_CLIENTS)]
CSEEDS = [bytes([c + 0x31]) * 32 for c in range(N_CLIENTS)]      # the clip seeds
NSEEDS = [bytes([c + 0x61]) * 32 for c in range(N_CLIENTS)]      # the nonce seeds


def _clients(R):
    """three clients of d = 70 whose every coordinate is +-127 steps -- S = 70 x 127^2 = 1 129 030 > 65 535 -- with blindings that cancel"""
    bls = R.pedersen_ops.generate_cancelling_scalar_vec_seeded(N_CLIENTS, D, b"\x77" * 32)
    out = []
    for c in range(N_CLIENTS):
        rng = np.random.default_rng(70 + c)
        x = (rng.choice((-127, 127), D) / 128.0).astype(np.float32)
        r2 = rng.integers(0, 256, size=(D, 32), dtype=np.uint8); r2[:, 31] &= 0x0F
        out.append((x, bls[c], r2))
    return out


def _classes(R):
    return (R.EncParamsL2, R.EncParamsL2Compressed, R.EncParamsL2CompressedStrict)


def test_an_update_over_the_norm_bound_fails_without_the_clip_and_passes_with_it(R):
    budget = R.l2_range_proof_vec.norm_budget(L2N, FP)
    assert budget == 255 ** 2
    x, bl, r2 = _clients(R)[0]
    assert M.sum_sq(x, NB, *FP) == 70 * 127 ** 2 > 65535
    for cls in _classes(R):
        with pytest.raises(R.RoflError) as e:
            cls.encrypt(x, bl, NB, P, L2N, nonce_seed=NSEEDS[0], rand_scalars=r2, fp=FP)
        assert e.value.code == 7, cls
        for kw, seed in ((dict(l2_clip=budget), None), (dict(l2_clip=budget, quant_seed=QSEEDS[0], clip_seed=CSEEDS[0]), CSEEDS[0])):
            up = cls.encrypt(x, bl, NB, P, L2N, nonce_seed=NSEEDS[0], rand_scalars=r2, fp=FP, **kw)
            assert up.verify(verifier_seed=b"\x05" * 32, fp=FP) is True, (cls, kw)
            assert list(cls.verify_batch([up], verifier_seed=b"\x05" * 32, fp=FP)) == [True]
            want, m, ks = M.clip_l2(x, budget, NB, *FP, seed=seed)      # (x is on the grid: the rounding of a quant seed is the identity)
            assert 0 < m < M.ONE and sum(k * k for k in ks) <= 65535 and sum(k * k for k in ks) > 65535 // 2
            # the clipped vector is the plaintext: a plain encrypt of the model's vector gives the same bytes
            assert cls.encrypt(want, bl, NB, P, L2N, nonce_seed=NSEEDS[0], rand_scalars=r2, fp=FP).serialize() == up.serialize(), (cls, kw)


def test_encrypt_batch_clipped_single_equals_batch_one_call_and_the_aggregate(R, monkeypatch):
    budget = R.l2_range_proof_vec.norm_budget(L2N, FP)
    cl = _clients(R)
    calls = []
    real = R.lib().rofl_clip_l2
    monkeypatch.setattr(R.lib(), "rofl_clip_l2", lambda *a: (calls.append(a[0].value), real(*a))[1])
    for cls in _classes(R):
        del calls[:]
        batch = cls.encrypt_batch_clipped(cl, NB, P, L2N, nonce_seeds=NSEEDS, fp=FP, quant_seeds=QSEEDS, l2_clip=budget, clip_seeds=CSEEDS)
        assert calls == [N_CLIENTS], "exactly one rofl_clip_l2 call for the three hosted clients"
        ones = [cls.encrypt(x, bl, NB, P, L2N, nonce_seed=NSEEDS[c], rand_scalars=r2, fp=FP, quant_seed=QSEEDS[c], l2_clip=budget, clip_seed=CSEEDS[c])
                for c, (x, bl, r2) in enumerate(cl)]
        assert [b.serialize() for b in batch] == [o.serialize() for o in ones], cls
        assert list(cls.verify_batch(batch, verifier_seed=b"\x05" * 32, fp=FP)) == [True] * N_CLIENTS
        # without l2_clip: the bytes of encrypt_batch_private, and no clip call (small updates that pass the norm check as they are)
        small = [((x / 16).astype(np.float32), bl, r2) for x, bl, r2 in cl]
        del calls[:]
        a = cls.encrypt_batch_clipped(small, NB, P, L2N, nonce_seeds=NSEEDS, fp=FP, quant_seeds=QSEEDS)
        b = cls.encrypt_batch_private(small, NB, P, L2N, nonce_seeds=NSEEDS, fp=FP, quant_seeds=QSEEDS)
        assert calls == [] and [u.serialize() for u in a] == [u.serialize() for u in b]
        if cls is R.EncParamsL2:
            clipped = [M.clip_l2(pq_model.quantize(x, QSEEDS[c], NB, *FP), budget, NB, *FP, seed=CSEEDS[c])[0] for c, (x, _, _) in enumerate(cl)]
            want = np.sum(np.array(clipped, np.float64), axis=0)
            with R.DeviceAccumulator.unity(D) as acc:
                acc.accumulate_batch(batch)
                got = acc.extract(fp=FP)
            assert got is not None and got.tobytes() == want.astype(np.float32).tobytes() and want.any()
