"""Probabilistic quantization ON THE DEVICE (rofl_quantize_prob, k_quantize_prob) against the Python model of tests/pq_model.py, byte for
byte: the rounding rule as the device compiles it on the edge-case corpus, the kernel's stream and edges (odd `first`, ends off the
32-element XOF blocks, more than one wave, several vectors with their own seeds), the memory spaces, the exactness of the outputs at every
deterministic float-to-fixed site, and whole rounds through the containers: the aggregate of a round of quarter-step updates is the sum of
the rounded values (399 grid steps over six clients where the expectation is 385.5), and all zeros without seeds.

A call whose pointers are all host memory and which is small runs on the host (the threshold is the library's); the tests that mean the
kernel go through rofl_dbg_quantize_prob_route(1, ...) or hand in device memory, which always takes the kernel."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import pq_model as M
import quant_model as Q
from test_prob_quant_host import _round

pytestmark = pytest.mark.gpu
sz = ctypes.c_size_t
FORMATS = ((8, 8, 7), (16, 16, 7), (16, 16, 12), (32, 32, 7), (64, 64, 12))      # (prove_range, fp_bits, fp_frac)
FP = (16, 7)


@pytest.fixture(scope="module")
def R():
    import rofl_project_code_amd as R
    from rofl_project_code_amd import build
    build.build()
    R.set_device(0)     # fails loudly when there is no HIP device / library
    yield R
    R.api.set_fp(16, 7)


def _addr(x):
    return x.data_ptr() if hasattr(x, "data_ptr") else x.ctypes.data


def quant(R, route, seeds, values, first, nb, fb, ff, outs):
    """rofl_quantize_prob (route None) or rofl_dbg_quantize_prob_route on numpy arrays / GPU tensors, written into outs"""
    n, d = len(values), (values[0].numel() if hasattr(values[0], "numel") else values[0].size)
    arr = lambda xs: (ctypes.c_void_p * n)(*[_addr(x) for x in xs])
    args = [sz(n), b"".join(seeds), arr(values), sz(first), sz(d), sz(nb), ctypes.c_uint(fb), ctypes.c_uint(ff), arr(outs)]
    rc = R.lib().rofl_quantize_prob(*args) if route is None else R.lib().rofl_dbg_quantize_prob_route(ctypes.c_uint(route), *args)
    assert rc == 0, rc


def _inputs(rng, d, nb, fb, ff):
    """values around a few grid steps, both signs, with grid values, zeros, a value beyond the clip bound and a NaN mixed in"""
    mx = Q.value(Q.clip_bounds(nb, fb, ff)[1])
    x = rng.uniform(-3, 3, d).astype(np.float32) * np.float32(min(1.0, float(mx) / 3))
    put = [np.float32(2 / (1 << ff)), np.float32(-0.0), np.float32(1e30), np.float32(np.nan), np.float32(-1 / (1 << ff))]
    for i, v in enumerate(put[:max(d - 1, 0)]):
        x[(7 * i + 1) % d] = v
    return x


def test_device_rule_equals_the_host_rule_on_the_corpus(R):
    n = 0
    for fb, ff in Q.VALID_FP:
        for nb in sorted({min(8, fb), fb}):
            vb, ws = M.corpus(fb, ff, nb)
            dev, host = _round(R.lib(), 1, vb, ws, nb, fb, ff), _round(R.lib(), 0, vb, ws, nb, fb, ff)
            assert (dev == host).all(), (fb, ff, nb, np.nonzero(dev != host)[0][:5])
            n += vb.size
    for nb, fb, ff in FORMATS:      # (the host rule equals the model on all of them in test_prob_quant_host.py; here the device against the model directly)
        vb, ws = M.corpus(fb, ff, nb)
        assert (_round(R.lib(), 1, vb, ws, nb, fb, ff) == M.corpus_expected(fb, ff, nb)).all(), (fb, ff, nb)
    assert n > 10000


@pytest.mark.parametrize("nb,fb,ff", FORMATS, ids=["fp%d_%d" % f[1:] for f in FORMATS])
def test_kernel_equals_the_model(R, nb, fb, ff):
    rng = np.random.default_rng(fb * 100 + ff)
    seeds = [bytes([0x41 + v]) * 32 for v in range(3)]
    for d in (1, 31, 32, 33, 257):
        vals = [_inputs(rng, d, nb, fb, ff) for _ in range(3)]
        for first in (0, 1, 31, 2 ** 40 + 5):
            outs = [np.full(d, np.nan, np.float32) for _ in range(3)]
            quant(R, 1, seeds, vals, first, nb, fb, ff, outs)
            for v in range(3):
                want = M.quantize(vals[v], seeds[v], nb, fb, ff, first)
                assert outs[v].tobytes() == want.tobytes(), (d, first, v, np.nonzero(outs[v].view(np.uint32) != want.view(np.uint32))[0][:5])


def test_more_than_one_wave_and_the_three_routes(R):
    """2 x 70 001 elements from an odd first: 35 blocks of one wave per vector, the last one partly filled; the kernel, the host copy and the
    entry point's own choice give the same bytes, and a sample of them is the model's"""
    nb, fb, ff = 16, 16, 7
    d, first = 70001, 2 ** 33 + 17
    rng = np.random.default_rng(3)
    seeds = [b"\x07" * 32, b"\x08" * 32]
    vals = [rng.uniform(-260, 260, d).astype(np.float32) for _ in range(2)]
    res = []
    for route in (1, 0, None):
        outs = [np.full(d, np.nan, np.float32) for _ in range(2)]
        quant(R, route, seeds, vals, first, nb, fb, ff, outs)
        res.append(b"".join(o.tobytes() for o in outs))
    assert res[0] == res[1] == res[2]
    got = np.frombuffer(res[0], np.float32).reshape(2, d)
    for lo in (0, 2040, d - 100):
        assert got[1, lo:lo + 100].tobytes() == M.quantize(vals[1][lo:lo + 100], seeds[1], nb, fb, ff, first + lo).tobytes(), lo
    assert np.abs(got).max() == np.float32(32767 / 128) and (got * 128 == np.round(got * 128)).all()


def test_runs_taken_with_first_concatenate(R):
    nb, fb, ff = 16, 16, 7
    x = _inputs(np.random.default_rng(11), 257, nb, fb, ff)
    whole = np.zeros(257, np.float32)
    quant(R, 1, [b"\x21" * 32], [x], 5, nb, fb, ff, [whole])
    for cut in (1, 27, 32, 100):
        a, b = np.zeros(cut, np.float32), np.zeros(257 - cut, np.float32)
        quant(R, 1, [b"\x21" * 32], [x[:cut].copy()], 5, nb, fb, ff, [a])
        quant(R, 1, [b"\x21" * 32], [x[cut:].copy()], 5 + cut, nb, fb, ff, [b])
        assert np.concatenate([a, b]).tobytes() == whole.tobytes(), cut


def test_memory_spaces_and_in_place(R):
    """host and device pointers in every combination, mixed within one call, in place in both spaces, and the Python wrappers over GPU
    tensors (torch in a child process, as the other device-pointer tests do): tests/gpu_prob_quant_device_check.py"""
    nb, fb, ff = 16, 16, 7
    h = _inputs(np.random.default_rng(12), 257, nb, fb, ff)
    want = M.quantize(h, b"\x32" * 32, nb, fb, ff, 31).tobytes()
    quant(R, 1, [b"\x32" * 32], [h], 31, nb, fb, ff, [h])      # host memory, in place, through the kernel
    assert h.tobytes() == want
    r = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "gpu_prob_quant_device_check.py")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "PROB_QUANT_DEVICE PASS" in r.stdout, r.stdout + r.stderr[-3000:]


def test_grid_inputs_come_back_unchanged(R):
    for nb, fb, ff in FORMATS:
        mx = Q.clip_bounds(nb, fb, ff)[1]
        ks = np.arange(-150, 151, dtype=np.float64)
        x = np.concatenate([(ks / (1 << ff)).astype(np.float32), np.array([0.0, -0.0], np.float32), np.array([mx, mx | Q.SIGN], np.uint32).view(np.float32)])
        x = x[np.abs(x) <= Q.f32(mx)]
        for seed in (b"\x00" * 32, b"\xff" * 32):
            out = np.full(x.size, np.nan, np.float32)
            quant(R, 1, [seed], [x], 3, nb, fb, ff, [out])
            assert out.tobytes() == x.tobytes(), (nb, fb, ff)


@pytest.mark.parametrize("nb,fb,ff", FORMATS, ids=["fp%d_%d" % f[1:] for f in FORMATS])
def test_outputs_are_exact_at_every_deterministic_site(R, nb, fb, ff):
    """every output converts exactly: scalar -> f32 gives it back, and k_quantize_shift, the L2 sums and sg_f32_to_sc read the model's k'"""
    from test_gpu_quantize import dbg_quantize
    d, first, seed = 257, 9, b"\x55" * 32
    x = _inputs(np.random.default_rng(fb + ff), d, nb, fb, ff)
    out = np.full(d, np.nan, np.float32)
    quant(R, 1, [seed], [x], first, nb, fb, ff, [out])
    ws = M.words(seed, first, d)
    ks = [M.steps(int(b), w, nb, fb, ff) for b, w in zip(x.view(np.uint32), ws)]
    neg = [Q.is_neg(int(b)) for b in out.view(np.uint32)]
    assert any(k == 0 and (b >> 31) for k, b in zip(ks, out.view(np.uint32))), "a negative value that rounded to zero is in the sample"
    # (the sample holds the closed bound: at a 32- or 64-bit range its shift wraps, DESIGN section 9, with or without this call -- the
    # expectations below are the deterministic rule applied to the model's k', wrap included)
    sc = R.conversion32.f32_to_scalar_vec(out, fp=(fb, ff))
    back = R.conversion32.scalar_to_f32_vec(sc, fp=(fb, ff))
    assert (back == out).all() and not np.isnan(out).any()      # (as values: -0.0 comes back as 0.0)
    want_sc = [(-k) % Q.L if n else k for k, n in zip(ks, neg)]
    assert sc.tobytes() == b"".join(k.to_bytes(32, "little") for k in want_sc)
    vshift, st = dbg_quantize(R, 0, out[None, :], nb, fb, ff, dpad=d)
    assert st.tolist() == [0] and vshift[0].tolist() == [((s + (1 << (nb - 1))) % Q.L) & ((1 << fb) - 1) for s in want_sc]
    _, sums, st = dbg_quantize(R, 1, out[None, :], nb, fb, ff, blind=np.zeros((1, d, 32), np.uint8))
    assert st.tolist() == [0] and sums[0, 0].tobytes() == sum(k * k for k in ks).to_bytes(32, "little")
    assert dbg_quantize(R, 2, out[None, :], nb, fb, ff).tobytes() == sc.tobytes()


# ---------------------------------------------------------------- whole rounds through the containers
N_CLIENTS = 6
QSEEDS = [bytes([c + 1]) * 32 for c in range(N_CLIENTS)]
NSEEDS = [bytes([c + 0x61]) * 32 for c in range(N_CLIENTS)]


def _round_inputs(R, d):
    x = np.full(d, 1 / 512, np.float32)      # a quarter of a grid step at fp (16, 7): every deterministic site sends it to 0
    bls = R.pedersen_ops.generate_cancelling_scalar_vec_seeded(N_CLIENTS, d, b"\x77" * 32)
    return x, bls


def test_round_of_quarter_steps_range(R):
    d, nb, P = 257, 8, 2
    x, bls = _round_inputs(R, d)
    ups = [R.EncParamsRange.encrypt(x, bls[c], nb, P, 1.0, nonce_seed=NSEEDS[c], fp=FP, quant_seed=QSEEDS[c]) for c in range(N_CLIENTS)]
    assert all(u.verify(verifier_seed=b"\x05" * 32, fp=FP) for u in ups)
    qs = [R.range_proof_vec.quantize_probabilistic(x, nb, QSEEDS[c], fp=FP) for c in range(N_CLIENTS)]
    assert all(q.tobytes() == M.quantize(x, QSEEDS[c], nb, *FP).tobytes() for c, q in enumerate(qs))
    want = np.sum(np.array(qs, np.float64), axis=0)
    assert int(round(want.sum() * 128)) == 399                       # the expectation is 6 * 257 / 4 = 385.5
    with R.DeviceAccumulator.unity(d) as acc:
        acc.accumulate_batch(ups)
        got = acc.extract(fp=FP)
    assert got is not None and got.tobytes() == want.astype(np.float32).tobytes()
    # the batch gives the bytes of the six single calls
    batch = R.EncParamsRange.encrypt_batch_quantized([(x, bls[c]) for c in range(N_CLIENTS)], nb, P, 1.0, QSEEDS, nonce_seeds=NSEEDS, fp=FP)
    assert [b.serialize() for b in batch] == [u.serialize() for u in ups]
    # the same round without seeds aggregates to nothing
    plain = R.EncParamsRange.encrypt_batch([(x, bls[c]) for c in range(N_CLIENTS)], nb, P, 1.0, nonce_seeds=NSEEDS, fp=FP)
    with R.DeviceAccumulator.unity(d) as acc:
        acc.accumulate_batch(plain)
        zero = acc.extract(fp=FP)
    assert zero is not None and not zero.any()


def test_round_of_quarter_steps_l2_compressed(R):
    d, nb, P, l2n = 64, 8, 2, 32
    x, bls = _round_inputs(R, d)
    rng = np.random.default_rng(64)
    r2s = []
    for _ in range(N_CLIENTS):
        r2 = rng.integers(0, 256, size=(d, 32), dtype=np.uint8); r2[:, 31] &= 0x0F
        r2s.append(r2)
    cls = R.EncParamsL2Compressed
    ups = [cls.encrypt(x, bls[c], nb, P, l2n, nonce_seed=NSEEDS[c], rand_scalars=r2s[c], fp=FP, quant_seed=QSEEDS[c]) for c in range(N_CLIENTS)]
    assert all(u.verify(verifier_seed=b"\x05" * 32, fp=FP) for u in ups)
    want = np.sum(np.array([M.quantize(x, QSEEDS[c], nb, *FP) for c in range(N_CLIENTS)], np.float64), axis=0)
    assert int(round(want.sum() * 128)) == 97                        # the expectation is 96
    with R.DeviceAccumulator.unity(d) as acc:
        acc.accumulate_batch(ups)
        got = acc.extract(fp=FP)
    assert got is not None and got.tobytes() == want.astype(np.float32).tobytes()
    batch = cls.encrypt_batch_quantized([(x, bls[c], r2s[c]) for c in range(N_CLIENTS)], nb, P, l2n, QSEEDS, nonce_seeds=NSEEDS, fp=FP)
    assert [b.serialize() for b in batch] == [u.serialize() for u in ups]
    plain = cls.encrypt_batch([(x, bls[c], r2s[c]) for c in range(N_CLIENTS)], nb, P, l2n, nonce_seeds=NSEEDS, fp=FP)
    with R.DeviceAccumulator.unity(d) as acc:
        acc.accumulate_batch(plain)
        zero = acc.extract(fp=FP)
    assert zero is not None and not zero.any()
