"""Discrete Gaussian noise ON THE DEVICE (rofl_noise_dgauss, k_noise_dgauss) against the Python model of tests/dgauss_model.py, byte for
byte: the kernel on lengths around a wave and over several workgroups, from index 0 and from a high one, at variance parameters with
one-word and with two-word draws; vectors long enough that lanes own several elements and that some element wraps the lane's LDS ring
or leaves it for the on-demand source (asserted from the model and rofl_dbg_dgauss_geometry); the sampler as the device compiles it on
crafted and random word lists; the memory spaces; the three routes; the lane-residue scan; and a whole round through the containers.

A call whose pointers are all host memory and which is small runs on the host (the threshold is the library's); the tests that mean the
kernel go through rofl_dbg_noise_dgauss_route(1, ...) or hand in device memory, which always takes the kernel."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import dgauss_model as M
import pq_model
from test_binomial_noise_host import inputs
from test_dgauss_noise_host import GOLDEN, GRID_SEEDS, SEED, check_grid, crafted_cases, dg_call, random_cases, words_call

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


def run(R, route, seeds, values, first, s2, nb, fb, ff, outs):
    d = values[0].numel() if hasattr(values[0], "numel") else values[0].size
    rc = dg_call(R.lib(), route, len(values), b"".join(seeds), values, first, d, s2, nb, fb, ff, outs)
    assert rc == 0, rc


def geometry(R, d):
    e, r = ctypes.c_uint32(0), ctypes.c_uint32(0)
    assert R.lib().rofl_dbg_dgauss_geometry(ctypes.c_size_t(d), ctypes.byref(e), ctypes.byref(r)) == 0
    return e.value, r.value


@pytest.mark.parametrize("s2", (1, 50, 4096, 1 << 16, 1 << 24))
def test_kernel_equals_the_model(R, s2):
    """three vectors with their own seeds per call; d = 1, one short of a wave, a wave, one more, several workgroups and a ragged last one"""
    check_grid(R.lib(), 1, 32, 32, 7, s2, shapes=[(d, first) for d in (1, 63, 64, 65, 257, 1000) for first in (0, 2 ** 40 + 5)])


def _noise_of_zeros(R, first, d, s2):
    out = np.full(d, np.nan, np.float32)
    run(R, 1, [SEED], [np.zeros(d, np.float32)], first, s2, 32, 32, 7, [out])
    return out.astype(np.float64) * 128


@pytest.mark.parametrize("first,d,s2,must_hold", ((0, 20000, 4096, (3565, 9406)), (11000, 2000, 1 << 24, (11567,)), (5400, 300, 1 << 24, (5546,))), ids=("4096", "2^24", "2^24-overrun"))
def test_lanes_own_several_elements_and_long_elements_leave_the_ring(R, first, d, s2, must_hold):
    """fp (32, 7) and zeros in: the outputs are the noise itself.  From the model: the vector holds elements that need more blocks than
    a lane's ring has (they wrap it), the third one an element whose single attempt spans more blocks than the ring (it takes the
    on-demand source); from the geometry: lanes own more than one element"""
    per_lane, ring = geometry(R, d)
    assert per_lane > 1
    for e in must_hold:
        assert first <= e < first + d
    blocks = [(M.element(SEED, e, s2)[1] + 31) >> 5 for e in must_hold]
    assert max(blocks) > ring, (blocks, ring)
    if d == 300:
        assert must_hold[0] in GOLDEN["ring_overruns"][str(s2)] and M.element(SEED, must_hold[0], s2, True)[2] >= ring
    want = M.noise(SEED, first, d, s2)
    got = _noise_of_zeros(R, first, d, s2)
    assert (got == want).all(), np.nonzero(got != want)[0][:5]


def test_device_sampler_equals_the_host_sampler_on_word_lists(R):
    cases = [(w, s) for w, s, _ in crafted_cases()]
    dev = words_call(R.lib(), 1, cases)
    assert dev == words_call(R.lib(), 0, cases) == [M.on_words(w, s) for w, s in cases]
    cases, want = random_cases()
    assert words_call(R.lib(), 1, cases) == want


def test_memory_spaces_and_in_place(R):
    """host memory in place through the kernel here; host and device vectors mixed within one call of three, device in place and the
    Python wrappers over GPU tensors in tests/gpu_dgauss_noise_device_check.py (torch in a child process, as the other device-pointer
    tests do)"""
    nb, fb, ff = 16, 16, 7
    h = inputs(np.random.default_rng(12), 257, nb, fb, ff)
    want = M.add_noise(h, b"\x32" * 32, 50, nb, fb, ff, 31).tobytes()
    run(R, 1, [b"\x32" * 32], [h], 31, 50, nb, fb, ff, [h])
    assert h.tobytes() == want
    r = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "gpu_dgauss_noise_device_check.py")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "DGAUSS_NOISE_DEVICE PASS" in r.stdout, r.stdout + r.stderr[-3000:]


def test_host_route_equals_device_route_equals_default_route(R):
    nb, fb, ff = 16, 16, 7
    d, first, s2 = 5000, 11, 4096
    rng = np.random.default_rng(33)
    seeds = [b"\x07" * 32, b"\x08" * 32]
    vals = [rng.uniform(-260, 260, d).astype(np.float32) for _ in range(2)]
    res = []
    for route in (1, 0, None):
        outs = [np.full(d, np.nan, np.float32) for _ in range(2)]
        run(R, route, seeds, vals, first, s2, nb, fb, ff, outs)
        res.append(b"".join(o.tobytes() for o in outs))
    assert res[0] == res[1] == res[2]
    got = np.frombuffer(res[0], np.float32).reshape(2, d)
    for lo in (0, 1980, d - 100):
        assert got[1, lo:lo + 100].tobytes() == M.add_noise(vals[1][lo:lo + 100], seeds[1], s2, nb, fb, ff, first + lo).tobytes(), lo
    assert np.abs(got).max() == np.float32(32767 / 128) and (got * 128 == np.round(got * 128)).all()      # (some saturate: the inputs reach the bound)


def test_no_seed_bytes_stay_in_the_lane(R):
    """the lane-residue scan after one call through the kernel, as for the other seeded preparation calls (tests/test_gpu_lane_residue.py)"""
    rng = np.random.default_rng(20270351)
    seeds = [rng.bytes(32) for _ in range(2)]
    vals = [rng.uniform(-0.9, 0.9, 33).astype(np.float32) for _ in range(2)]
    outs = [np.full(33, np.nan, np.float32) for _ in range(2)]
    run(R, 1, seeds, vals, 0, 9, 8, 16, 7, outs)
    assert not np.isnan(np.stack(outs)).any()
    fn = R.lib().rofl_dbg_lane_scan
    fn.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_int)]
    for s in seeds:
        found = ctypes.c_int(-1)
        assert fn(s, 32, ctypes.byref(found)) == 0 and found.value == 0
        assert fn(s[:16], 16, ctypes.byref(found)) == 0 and found.value == 0


def test_round_of_noised_updates_aggregates_to_the_sum_of_the_models_values(R):
    """8 clients, d = 100, fp (16, 7) with a 16-bit range (+-256: noise of sigma 3 on values of a few steps saturates nowhere),
    cancelling blindings, encrypt_batch_private(noise_k=DiscreteGaussian(9)) -> verify_batch -> DeviceAccumulator -> extract: exactly
    the sum of the model's noised values"""
    n, d, nb, P = 8, 100, 16, 2
    qs, zs, ns = ([bytes([c + b]) * 32 for c in range(n)] for b in (1, 0x31, 0x61))
    rng = np.random.default_rng(9)
    bls = R.pedersen_ops.generate_cancelling_scalar_vec_seeded(n, d, b"\x77" * 32)
    xs = [rng.uniform(-1.5, 1.5, d).astype(np.float32) for _ in range(n)]
    ups = R.EncParamsRange.encrypt_batch_private([(xs[c], bls[c]) for c in range(n)], nb, P, 1.0, nonce_seeds=ns, fp=FP,
                                                 quant_seeds=qs, noise_seeds=zs, noise_k=R.DiscreteGaussian(9))
    assert list(R.EncParamsRange.verify_batch(ups, verifier_seed=b"\x05" * 32, fp=FP)) == [True] * n
    rounded = [pq_model.quantize(xs[c], qs[c], nb, *FP) for c in range(n)]
    noise = [M.noise(zs[c], 0, d, 9) for c in range(n)]
    noised = [M.add_noise(rounded[c], zs[c], 9, nb, *FP, ns=noise[c]) for c in range(n)]
    want = np.sum(np.array(noised, np.float64), axis=0)
    assert (want * 128 == np.sum(np.array(rounded, np.float64), axis=0) * 128 + sum(noise)).all() and sum(noise).any(), "nothing saturated"
    with R.DeviceAccumulator.unity(d) as acc:
        acc.accumulate_batch(ups)
        got = acc.extract(fp=FP)
    assert got is not None and got.tobytes() == want.astype(np.float32).tobytes()
