"""The Hadamard rotation ON THE DEVICE (rofl_rotate: k_rotate_tile, k_rotate_cols) against the Python model of tests/rot_model.py, byte
for byte, at the smallest shapes at which each mechanism of the kernels can go wrong: blocks below a wave, the seams between the register,
shuffle and LDS stages of the tile kernel, blocks of one tile and longer ones (the column kernel: one, two and three passes, both strip
widths), vector lengths off the block (the padding is read as zeros, never from memory), three vectors with three seeds in one launch,
both directions, subnormal and clamped inputs (a flush-to-zero build or a scale folded into a butterfly fails here), the memory spaces,
and whole rounds through the containers: six clients whose updates are one spike each aggregate to the clip bound without the rotation and
to exactly their spikes with it.

A call whose pointers are all host memory and which is small runs on the host (the threshold is the library's); the tests that mean the
kernels go through rofl_dbg_rotate_route(1, ...) or hand in device memory, which always takes the kernels."""
import os
import subprocess
import sys

import numpy as np
import pytest

import rot_model as M
from test_rotate_host import SEEDS, check_cases, inputs, rot_call

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def R():
    import rofl_project_code_amd as R
    from rofl_project_code_amd import build
    build.build()
    R.set_device(0)     # fails loudly when there is no HIP device / library
    yield R
    R.api.set_fp(16, 7)


def _tile_log2(R):
    return int(R.lib().rofl_dbg_rotate_tile_log2())


def two_tiles_and_a_block(k):
    """dp = 2 T + B with T = 8 192 (asserted against the library below): d = dp - 1 and d = dp - B + 1, the last block short by one
    element and holding one element"""
    B = 1 << k
    dp = 2 * 8192 + B
    return sorted({dp - 1, dp - B + 1})


def test_the_tile_the_tests_aim_at(R):
    assert _tile_log2(R) == 13      # two_tiles_and_a_block and the k lists below are written for it


@pytest.mark.parametrize("k", (0, 1, 3, 5))
def test_blocks_below_a_wave(R, k):
    """several blocks per thread (k < 4: only register stages run), per wave and per tile"""
    check_cases(R.lib(), 1, (k,), two_tiles_and_a_block, seed=11)


@pytest.mark.parametrize("k", (4, 6, 7, 8, 10, 11))
def test_register_shuffle_and_lds_seams(R, k):
    """k_rotate_tile runs h < 16 in registers, h < 1 024 by __shfl_xor and h < 8 192 through LDS: k = 4 | 5 and k = 10 | 11 are the two
    sides of its seams (5 is in the test above, 12 and 13 in the one below); 6, 7, 8 end inside the shuffle stages, on an even and an odd
    scale"""
    check_cases(R.lib(), 1, (k,), two_tiles_and_a_block, seed=12)


@pytest.mark.parametrize("n_blk", (1, 3))
@pytest.mark.parametrize("dk", (-1, 0, 1, 2))
def test_tile_and_column_paths(R, dk, n_blk):
    """k = t - 1, t (one launch) and t + 1, t + 2 (two launches: the column kernel in one pass); one block short by one element, and
    three blocks of which the last holds one element"""
    k = _tile_log2(R) + dk
    check_cases(R.lib(), 1, (k,), lambda k_: [(n_blk << k_) - (1 if n_blk == 1 else (1 << k_) - 1)], seed=13)


@pytest.mark.parametrize("k", (16, 17, 20, 22))
def test_column_kernel_passes(R, k):
    """one block short by one element: k = 16 | 17 is the seam between one pass of the column kernel (no LDS) and two, k = 20 takes three
    passes, k = 22 the narrow strips of 32 columns x 512 rows"""
    check_cases(R.lib(), 1, (k,), lambda k_: [(1 << k_) - 1], seed=14, n_vec=1)


def test_routes_agree(R):
    """routes 1, 0 and the entry point's own choice at 2 x 70 001 elements, k = 12"""
    d, k = 70001, 12
    dp = M.rotated_len(d, k)
    rng = np.random.default_rng(21)
    vals = [inputs(rng, d) for _ in range(2)]
    sb = b"".join(SEEDS[:2])
    want = [M.rotate(x, s, k) for x, s in zip(vals, SEEDS)]
    for inverse, src, n_in in ((0, vals, d), (1, want, dp)):
        res = []
        for route in (1, 0, None):
            outs = [np.full(dp, np.nan, np.float32) for _ in src]
            assert rot_call(R.lib(), route, sb, src, n_in, k, inverse, outs) == 0
            res.append(b"".join(o.tobytes() for o in outs))
        assert res[0] == res[1] == res[2]
        if not inverse:
            assert res[0] == b"".join(w.tobytes() for w in want)


def test_memory_spaces_and_in_place(R):
    """host memory in place through the kernels here; host and device vectors in every combination, mixed within one call, device in
    place, unaligned device pointers and the Python wrappers over GPU tensors in tests/gpu_rotate_device_check.py (torch in a child
    process, as the other device-pointer tests do)"""
    k, d = 9, 3 * 512 + 7
    dp = M.rotated_len(d, k)
    x = inputs(np.random.default_rng(12), d)
    h = np.full(dp, np.nan, np.float32); h[:d] = x
    assert rot_call(R.lib(), 1, SEEDS[0], [h], d, k, 0, [h]) == 0
    assert h.tobytes() == M.rotate(x, SEEDS[0], k).tobytes()
    r = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "gpu_rotate_device_check.py")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ROTATE_DEVICE PASS" in r.stdout, r.stdout + r.stderr[-3000:]


# ---------------------------------------------------------------- whole rounds through the containers
FP, NB, D, K, P, N_CLIENTS = (16, 7), 8, 257, 8, 2, 6
DP = 512
ROUND_SEED = bytes(range(32))
NSEEDS = [bytes([c + 0x61]) * 32 for c in range(N_CLIENTS)]      # the nonce seeds
# the rounding seeds: the pipeline is rotate -> round -> clip -> noise -> legs, and it is the rounding call whose output -- clipped, on the
# grid -- is the plaintext of EVERY leg (without it the randomness leg takes the un-clipped value and a clipped update does not verify)
QSEEDS = [bytes([c + 1]) * 32 for c in range(N_CLIENTS)]
AT = [3 + 41 * c for c in range(N_CLIENTS)]                      # client c's spike


def _round(R, cls, spike, make, rotated):
    """six clients, client c's update one spike at AT[c]; -> the aggregate DeviceAccumulator.extract opens"""
    n = DP if rotated else D
    bls = R.pedersen_ops.generate_cancelling_scalar_vec_seeded(N_CLIENTS, n, b"\x77" * 32)
    assert all(len(b) == n for b in bls)      # blinding vectors have rotated_len entries
    xs = []
    for c in range(N_CLIENTS):
        x = np.zeros(D, np.float32); x[AT[c]] = spike
        xs.append(x)
    if rotated:
        xs = list(R.range_proof_vec.rotate_vecs(xs, ROUND_SEED, K))      # ONE call for all hosted clients
        step = spike * 128 / 16
        assert all(y.size == DP and set(np.abs(y * 128).tolist()) <= {0.0, step} and int((y != 0).sum()) == 256 for y in xs), "+-spike / 16 on the grid, in the spike's block"
    ups = [make(cls, x, bls[c], c) for c, x in enumerate(xs)]
    assert list(cls.verify_batch(ups, verifier_seed=b"\x05" * 32, fp=FP)) == [True] * N_CLIENTS
    with R.DeviceAccumulator.unity(n) as acc:
        acc.accumulate_batch(ups)
        got = acc.extract(fp=FP)
    assert got is not None
    return got


def _check_round(R, cls, spike, make):
    assert R.range_proof_vec.rotated_len(D, K) == DP
    clip_max = float(R.conversion32.get_clip_bounds(NB, fp=FP)[1])
    assert spike > clip_max > 0 and spike * 128 / 16 <= clip_max * 128      # one coordinate does not fit the 8-bit leg; its 256 rotated ones do
    # without the rotation: every spike is clipped, and the aggregate is silently wrong at exactly the coordinates that carry the signal
    plain = _round(R, cls, spike, make, rotated=False)
    want = np.zeros(D, np.float32); want[AT] = clip_max
    assert plain.tobytes() == want.tobytes()
    # with it: the aggregate of the rotated updates, rotated back once, is exactly the sum of the updates
    agg = _round(R, cls, spike, make, rotated=True)
    back = R.range_proof_vec.unrotate(agg, ROUND_SEED, K, D)
    want[AT] = spike
    assert np.array_equal(back, want)      # (exactly: by value -- the signs are the inverse's last step, so a zero comes back with either sign)


def test_round_of_spikes_range(R):
    """EncParamsRange, fp = (16, 7), prove_range = 8: a spike of 3.0 = 384 steps becomes 256 coordinates of +-24 steps"""
    _check_round(R, R.EncParamsRange, 3.0, lambda cls, x, bl, c: cls.encrypt(x, bl, NB, P, 1.0, nonce_seed=NSEEDS[c], fp=FP, quant_seed=QSEEDS[c]))


def test_round_of_spikes_l2_compressed(R):
    """EncParamsL2Compressed, fp = (16, 7), l2_range = 16: the norm check admits sum q^2 <= 65 535, and the rotation keeps the norm, so a
    spike of 3.0 = 384 steps (147 456 steps^2) cannot pass it before or after; the spike is shrunk to 1.875 = 240 steps (57 600), the
    largest multiple of 16 steps under the bound: +-15 steps rotated, and still above the clip bound of the 8-bit leg"""
    rng = np.random.default_rng(5)
    r2 = rng.integers(0, 256, size=(N_CLIENTS, DP, 32), dtype=np.uint8); r2[:, :, 31] &= 0x0F
    _check_round(R, R.EncParamsL2Compressed, 1.875, lambda cls, x, bl, c: cls.encrypt(x, bl, NB, P, 16, nonce_seed=NSEEDS[c], rand_scalars=r2[c, :x.size], fp=FP, quant_seed=QSEEDS[c]))
