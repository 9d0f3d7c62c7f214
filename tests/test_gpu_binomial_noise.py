"""Distributed noise ON THE DEVICE (rofl_noise_binomial, k_noise_binomial) against the Python model of tests/noise_model.py, byte for byte:
the kernel's segmented popcount sums on the shape grid of the host test and on the shapes only the kernel can get wrong (an element wider
than a wave's 64 blocks, the widest element, a run that crosses a workgroup's group of elements), the value rule as the device compiles
it on the clip bounds, the memory spaces, and whole updates and a whole round through the containers: the aggregate of a round of eight
noised updates is exactly the sum of the model's noised values.

A call whose pointers are all host memory and which is small runs on the host (the threshold is the library's); the tests that mean the
kernel go through rofl_dbg_noise_binomial_route(1, ...) or hand in device memory, which always takes the kernel."""
import os
import subprocess
import sys

import numpy as np
import pytest

import noise_model as M
import pq_model
from test_binomial_noise_host import FORMATS, WIDTHS, boundary_cases, check_grid, inputs, noise_apply, noise_call

pytestmark = pytest.mark.gpu
FP = (16, 7)


@pytest.fixture(scope="module")
def R():
    import rofl_project_code_amd as R
    from rofl_project_code_amd import build
    build.build()
    R.set_device(0)     # fails loudly when there is no HIP device / library
    yield R
    R.api.set_fp(16, 7)


def run(R, route, seeds, values, first, k, nb, fb, ff, outs):
    d = values[0].numel() if hasattr(values[0], "numel") else values[0].size
    rc = noise_call(R.lib(), route, len(values), b"".join(seeds), values, first, d, k, nb, fb, ff, outs)
    assert rc == 0, rc


@pytest.mark.parametrize("nb,fb,ff", FORMATS, ids=["r%d_fp%d_%d" % f for f in FORMATS])
def test_kernel_equals_the_model_on_the_shape_grid(R, nb, fb, ff):
    """the shape grid of the host test, three vectors with their own seeds per call (the model's outputs are computed once for both tests)"""
    for W in WIDTHS:
        check_grid(R.lib(), 1, nb, fb, ff, W)


@pytest.mark.parametrize("W,d,first", ((2049, 3, 0), (2049, 3, 2 ** 40 + 5), (65536, 2, 0), (65536, 2, 7), (3, 2049, 2047), (1, 4100, 13), (512, 130, 3), (40, 1000, 1)),
                         ids=lambda v: str(v))
def test_shapes_only_the_kernel_can_get_wrong(R, W, d, first):
    """an element wider than a wave's 64 blocks (W = 2049), the widest element (k = 2^20), W = 3 from first = 2047 over 2049 elements (four
    groups of 672 elements, the run starts in the middle of a block), more than two groups at W = 1, several groups of 63 at the width of
    sigma = 64, and a width that neither divides nor is divided by 32 over several groups.  A 32-bit format: the outputs are the noise
    itself plus small values, nothing saturates."""
    nb, fb, ff = 32, 32, 7
    seeds = [b"\x51" * 32, b"\x52" * 32]
    rng = np.random.default_rng(W)
    vals = [inputs(rng, d, nb, fb, ff) for _ in seeds]
    outs = [np.full(d, np.nan, np.float32) for _ in seeds]
    run(R, 1, seeds, vals, first, 16 * W, nb, fb, ff, outs)
    for v in range(2):
        want = M.add_noise(vals[v], seeds[v], 16 * W, nb, fb, ff, first)
        assert outs[v].tobytes() == want.tobytes(), (v, np.nonzero(outs[v].view(np.uint32) != want.view(np.uint32))[0][:5])
    assert outs[0].tobytes() != outs[1].tobytes()


def test_host_route_equals_device_route(R):
    nb, fb, ff = 16, 16, 7
    W, d, first = 33, 5000, 11
    rng = np.random.default_rng(33)
    seeds = [b"\x07" * 32, b"\x08" * 32]
    vals = [rng.uniform(-260, 260, d).astype(np.float32) for _ in range(2)]
    res = []
    for route in (1, 0, None):
        outs = [np.full(d, np.nan, np.float32) for _ in range(2)]
        run(R, route, seeds, vals, first, 16 * W, nb, fb, ff, outs)
        res.append(b"".join(o.tobytes() for o in outs))
    assert res[0] == res[1] == res[2]
    got = np.frombuffer(res[0], np.float32).reshape(2, d)
    for lo in (0, 1980, d - 100):
        assert got[1, lo:lo + 100].tobytes() == M.add_noise(vals[1][lo:lo + 100], seeds[1], 16 * W, nb, fb, ff, first + lo).tobytes(), lo
    assert np.abs(got).max() == np.float32(32767 / 128) and (got * 128 == np.round(got * 128)).all()      # (some saturate: the inputs reach the bound)


def test_device_value_rule_equals_the_host_rule_on_the_bounds(R):
    n = 0
    for nb, fb, ff in FORMATS:
        vb, ns, want = boundary_cases(nb, fb, ff)
        dev = noise_apply(R.lib(), 1, vb, ns, nb, fb, ff)
        assert (dev == noise_apply(R.lib(), 0, vb, ns, nb, fb, ff)).all() and (dev == want).all(), (nb, fb, ff, np.nonzero(dev != want)[0][:5])
        n += vb.size
    assert n > 400


def test_memory_spaces_and_in_place(R):
    """host memory in place through the kernel here; host and device vectors mixed within one call of three, device in place and the
    Python wrappers over GPU tensors in tests/gpu_binomial_noise_device_check.py (torch in a child process, as the other device-pointer
    tests do)"""
    nb, fb, ff = 16, 16, 7
    h = inputs(np.random.default_rng(12), 257, nb, fb, ff)
    want = M.add_noise(h, b"\x32" * 32, 48, nb, fb, ff, 31).tobytes()
    run(R, 1, [b"\x32" * 32], [h], 31, 48, nb, fb, ff, [h])
    assert h.tobytes() == want
    r = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "gpu_binomial_noise_device_check.py")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "BINOMIAL_NOISE_DEVICE PASS" in r.stdout, r.stdout + r.stderr[-3000:]


# ---------------------------------------------------------------- whole updates and a whole round through the containers
N_CLIENTS, D, NB, P, K = 8, 64, 8, 2, 16
QSEEDS = [bytes([c + 1]) * 32 for c in range(N_CLIENTS)]
ZSEEDS = [bytes([c + 0x31]) * 32 for c in range(N_CLIENTS)]      # the noise seeds
NSEEDS = [bytes([c + 0x61]) * 32 for c in range(N_CLIENTS)]      # the nonce seeds


def _r2(rng, d):
    r2 = rng.integers(0, 256, size=(d, 32), dtype=np.uint8); r2[:, 31] &= 0x0F
    return r2


def test_containers_single_equals_batch_and_verifies(R):
    rng = np.random.default_rng(64)
    x = R.range_proof_vec.clip_f32_for_noise(rng.uniform(-0.1, 0.1, D).astype(np.float32), NB, K, fp=FP)
    bl = R.pedersen_ops.generate_cancelling_scalar_vec_seeded(2, D, b"\x77" * 32)[0]
    r2 = _r2(rng, D)
    noised = M.add_noise(pq_model.quantize(x, QSEEDS[0], NB, *FP), ZSEEDS[0], K, NB, *FP)
    for cls, tail, extra in ((R.EncParamsRange, (P, 1.0), ()), (R.EncParamsRangeCompressed, (P, 1.0), ()), (R.EncParamsL2, (P, 32), (r2,)),
                             (R.EncParamsL2Compressed, (P, 32), (r2,)), (R.EncParamsL2CompressedStrict, (P, 32), (r2,))):
        kw = dict(rand_scalars=r2) if extra else {}
        one = cls.encrypt(x, bl, NB, *tail, nonce_seed=NSEEDS[0], fp=FP, quant_seed=QSEEDS[0], noise_seed=ZSEEDS[0], noise_k=K, **kw)
        assert one.verify(verifier_seed=b"\x05" * 32, fp=FP), cls
        batch = cls.encrypt_batch_private([(x, bl) + extra], NB, *tail, nonce_seeds=NSEEDS[:1], fp=FP, quant_seeds=QSEEDS[:1], noise_seeds=ZSEEDS[:1], noise_k=K)
        assert [b.serialize() for b in batch] == [one.serialize()], cls
        # the noised values are what is committed: a plain encrypt of the model's noised values gives the same bytes
        plain = cls.encrypt(noised, bl, NB, *tail, nonce_seed=NSEEDS[0], fp=FP, **kw)
        assert plain.serialize() == one.serialize(), cls
        # without noise seeds: the bytes of encrypt_batch_quantized
        a = cls.encrypt_batch_private([(x, bl) + extra], NB, *tail, nonce_seeds=NSEEDS[:1], fp=FP, quant_seeds=QSEEDS[:1])
        b = cls.encrypt_batch_quantized([(x, bl) + extra], NB, *tail, QSEEDS[:1], nonce_seeds=NSEEDS[:1], fp=FP)
        assert [u.serialize() for u in a] == [u.serialize() for u in b] != [one.serialize()], cls


def test_round_of_noised_updates_aggregates_to_the_sum_of_the_models_values(R):
    """8 clients, d = 64, fp (16, 7) with an 8-bit range: inputs clipped with clip_f32_for_noise (so no noise is truncated), cancelling
    blindings, encrypt_batch_private -> verify_batch -> DeviceAccumulator -> extract: exactly the sum of the model's noised values, which
    is the sum of the rounded values plus the sum of the model's noise integers"""
    rng = np.random.default_rng(8)
    bls = R.pedersen_ops.generate_cancelling_scalar_vec_seeded(N_CLIENTS, D, b"\x77" * 32)
    xs = [R.range_proof_vec.clip_f32_for_noise(rng.uniform(-1.5, 1.5, D).astype(np.float32), NB, K, fp=FP) for _ in range(N_CLIENTS)]
    assert any(np.abs(x).max() == np.float32((127 - K) / 128) for x in xs)
    ups = R.EncParamsRange.encrypt_batch_private([(xs[c], bls[c]) for c in range(N_CLIENTS)], NB, P, 1.0, nonce_seeds=NSEEDS, fp=FP,
                                                 quant_seeds=QSEEDS, noise_seeds=ZSEEDS, noise_k=K)
    assert list(R.EncParamsRange.verify_batch(ups, verifier_seed=b"\x05" * 32, fp=FP)) == [True] * N_CLIENTS
    rounded = [pq_model.quantize(xs[c], QSEEDS[c], NB, *FP) for c in range(N_CLIENTS)]
    noised = [M.add_noise(rounded[c], ZSEEDS[c], K, NB, *FP) for c in range(N_CLIENTS)]
    steps = sum(np.array(M.unsaturated_steps(rounded[c], ZSEEDS[c], K, *FP), np.int64) for c in range(N_CLIENTS))
    want = np.sum(np.array(noised, np.float64), axis=0)
    assert (want * 128 == steps).all(), "nothing saturated"
    noise_sum = sum(M.noise(ZSEEDS[c], 0, D, K) for c in range(N_CLIENTS))
    assert (steps == np.sum(np.array(rounded, np.float64), axis=0) * 128 + noise_sum).all() and noise_sum.any()
    with R.DeviceAccumulator.unity(D) as acc:
        acc.accumulate_batch(ups)
        got = acc.extract(fp=FP)
    assert got is not None and got.tobytes() == want.astype(np.float32).tobytes()
