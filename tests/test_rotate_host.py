"""CPU-only checks of the Hadamard rotation (rofl_rotate): the host-compiled network against the Python model (tests/rot_model.py) byte
for byte -- block sizes on both sides of the XOF word and block edges, vector lengths on and off the block, three vectors with their own
seeds in one call, both directions, inputs with zeros of both signs, subnormals, 1e30, the infinities, NaN and values beyond 2^100 -- the
sign stream across the 1 024-element edge of an XOF block, the exact cases (a one-hot input, dyadic round trips), the model's own error
bounds, every parameter check of the C entry point (they come before the device is touched), the Python helpers and the Rust
declaration.  No call here reaches a GPU: route 0 of rofl_dbg_rotate_route is the library's host route, compiled from the kernels'
source."""
import ctypes
import hashlib
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

import rot_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sz = ctypes.c_size_t
SEEDS = [bytes([v + 0x51]) * 32 for v in range(3)]
K_HOST = (0, 1, 5, 6, 10, 11)


def rot_call(L, route, seeds, values, d, k, inverse, outs, n_vec=None):
    """rofl_rotate (route None) or rofl_dbg_rotate_route with the given raw arguments (None = a null pointer) -> rc"""
    arr = lambda xs: (ctypes.c_void_p * len(xs))(*[(x.data_ptr() if hasattr(x, "data_ptr") else x.ctypes.data) if x is not None else None for x in xs]) if xs is not None else None
    n = len(values) if n_vec is None else n_vec
    args = [sz(n), seeds, arr(values), sz(d), ctypes.c_uint(k), ctypes.c_int(inverse), arr(outs)]
    return L.rofl_rotate(*args) if route is None else L.rofl_dbg_rotate_route(ctypes.c_uint(route), *args)


def lengths(k):
    B = 1 << k
    return sorted({d for d in (1, B - 1, B, B + 1, 3 * B + 7) if d > 0})


def inputs(rng, d, special=True):
    """Gaussian values of very different magnitudes; with `special`, about one element in eight is a zero of either sign, a subnormal,
    +-1e30, an infinity, a NaN or a finite value beyond 2^100"""
    x = (rng.standard_normal(d) * 10.0 ** rng.integers(-3, 4, d)).astype(np.float32)
    if special:
        sp = np.array([0.0, -0.0, 1e-45, -3e-42, 1e-39, 1e30, -1e30, np.inf, -np.inf, np.nan, 3e38, -2e35, 2.0 ** 100, -2.0 ** 100], np.float32)
        at = rng.integers(0, 8, d) == 0
        x[at] = sp[rng.integers(0, sp.size, int(at.sum()))]
    return x


_CASES = {}


def cases(ks, lens=lengths, seed=5, n_vec=3):
    """-> [(k, d, values of three vectors, the model's forward outputs, the model's inverse of those)]: computed once, shared by the host
    test and the device tests (tests/test_gpu_rotate.py), and never written"""
    key = (tuple(ks), lens, seed, n_vec)
    if key not in _CASES:
        rng = np.random.default_rng(seed)
        out = []
        for k in ks:
            for d in lens(k):
                vals = [inputs(rng, d) for _ in SEEDS[:n_vec]]
                fwd = [M.rotate(x, s, k) for x, s in zip(vals, SEEDS)]
                inv = [M.rotate(y, s, k, inverse=True) for y, s in zip(fwd, SEEDS)]
                out.append((k, d, vals, fwd, inv))
        _CASES[key] = out
    return _CASES[key]


def check_cases(L, route, ks, lens=lengths, seed=5, n_vec=3):
    sb = b"".join(SEEDS[:n_vec])
    for k, d, vals, fwd, inv in cases(ks, lens, seed, n_vec):
        dp = M.rotated_len(d, k)
        outs = [np.full(dp, np.nan, np.float32) for _ in vals]
        ins = [x.copy() for x in vals]
        assert rot_call(L, route, sb, ins, d, k, 0, outs) == 0, (k, d)
        for v in range(n_vec):
            assert outs[v].tobytes() == fwd[v].tobytes(), ("forward", k, d, v, np.nonzero(outs[v].view(np.uint32) != fwd[v].view(np.uint32))[0][:5])
            assert ins[v].tobytes() == vals[v].tobytes(), "an input was written"
        back = [np.full(dp, np.nan, np.float32) for _ in vals]
        assert rot_call(L, route, sb, outs, dp, k, 1, back) == 0, (k, d)
        for v in range(n_vec):
            assert back[v].tobytes() == inv[v].tobytes(), ("inverse", k, d, v, np.nonzero(back[v].view(np.uint32) != inv[v].view(np.uint32))[0][:5])


def test_the_model_meets_its_own_bounds():
    """forward error <= (k + 2) 2^-24 ||x|| and round trip <= (2k + 4) 2^-24 ||x|| against the float64 transform of the same signs, on
    Gaussian, Cauchy, constant and one-hot inputs; and the scale constants"""
    assert M.scale(0) == 1.0 and M.scale(8) == 2.0 ** -4 and M.scale(9).view(np.uint32) == 0x3F3504F3 - (4 << 23) and M.scale(1).view(np.uint32) == 0x3F3504F3
    rng = np.random.default_rng(1)
    worst = 0.0
    for k in (0, 1, 2, 5, 8, 11, 14):
        d = (3 << k) - (1 if k else 0)
        one_hot = np.zeros(d, np.float32); one_hot[d // 2] = 3.0
        for x in (rng.standard_normal(d), np.clip(rng.standard_cauchy(d), -1e6, 1e6), np.full(d, 0.3), one_hot):
            worst = max(worst, *M.check_bounds(np.asarray(x, np.float32), SEEDS[0], k))
    assert 0 < worst <= 1.0


@pytest.mark.parametrize("k", K_HOST)
def test_host_route_equals_the_model(hiplib, k):
    check_cases(hiplib, 0, (k,))


def test_small_all_host_calls_take_the_host_route_and_need_no_device(hiplib):
    """the entry point's own choice for a small call whose pointers are host memory: the same bytes (this test runs without a GPU)"""
    check_cases(hiplib, None, (5,))


def test_sign_stream_across_the_xof_block_edge(hiplib):
    """k = 0 is the sign flip alone.  Elements 1 023 and 1 024 take bit 31 of word 31 of block 0 and bit 0 of word 0 of block 1: computed
    here from hashlib directly, for two seeds that differ in both bits"""
    def bits(seed):
        blk = [hashlib.shake_256(b"rofl-zk/rotate/v1" + seed + struct.pack("<Q", b)).digest(128) for b in (0, 1)]
        return (blk[0][127] >> 7) & 1, blk[1][0] & 1
    seeds = [bytes([i]) * 32 for i in range(1, 40)]
    a = seeds[0]
    b = next(s for s in seeds[1:] if bits(s)[0] != bits(a)[0] and bits(s)[1] != bits(a)[1])
    d = 1030
    x = np.ones(d, np.float32)
    outs = [np.zeros(d, np.float32), np.zeros(d, np.float32)]
    assert rot_call(hiplib, 0, a + b, [x, x.copy()], d, 0, 0, outs) == 0
    for s, o in zip((a, b), outs):
        assert (np.abs(o) == 1.0).all()
        assert (int(o[1023] < 0), int(o[1024] < 0)) == bits(s)
        assert o.tobytes() == M.rotate(x, s, 0).tobytes()
    assert outs[0][1023] != outs[1][1023] and outs[0][1024] != outs[1][1024]
    # the inverse of k = 0 is the same flip
    back = [np.zeros(d, np.float32)]
    assert rot_call(hiplib, 0, a, [outs[0]], d, 0, 1, back) == 0 and back[0].tobytes() == x.tobytes()


def test_one_hot_inputs_are_spread_exactly(hiplib):
    """3.0 in one coordinate: k = 8 gives exactly +-3 / 16 everywhere, k = 9 one magnitude 3 x 2^-4 x f32(0x3F3504F3) in all 512 places"""
    for k, mag in ((8, np.float32(0.1875)), (9, np.float32(np.float32(0.1875) * M.HALF_SQRT2))):
        B = 1 << k
        x = np.zeros(B - 3, np.float32); x[B // 3] = 3.0
        out = [np.zeros(B, np.float32)]
        assert rot_call(hiplib, 0, SEEDS[0], [x], x.size, k, 0, out) == 0
        assert set(np.abs(out[0]).view(np.uint32).tolist()) == {int(mag.view(np.uint32))}
        assert 0 < int((out[0] < 0).sum()) < B
        assert out[0].tobytes() == M.rotate(x, SEEDS[0], k).tobytes()


def test_dyadic_round_trips_are_exact(hiplib):
    """integers below 2^(24 - k) / 128: every butterfly fits 24 bits, and with an even k the scale is a power of two both ways"""
    import rofl_project_code_amd as R
    rng = np.random.default_rng(3)
    for k, d in ((0, 77), (4, 100), (8, 257), (10, 3000)):
        x = (rng.integers(-(1 << (22 - k)), 1 << (22 - k), d) / 128.0).astype(np.float32)
        y = R.range_proof_vec.rotate(x, SEEDS[1], k)
        assert y.size == R.range_proof_vec.rotated_len(d, k) and y.tobytes() == M.rotate(x, SEEDS[1], k).tobytes()
        assert float(np.abs(y.astype(np.float64) - M.exact(x, SEEDS[1], k)).max()) == 0.0
        assert np.array_equal(R.range_proof_vec.unrotate(y, SEEDS[1], k, d), x)      # (by value: a zero comes back with either sign)
        assert not R.range_proof_vec.unrotate(y, SEEDS[1], k)[d:].any()


def test_in_place(hiplib):
    k, d = 6, 3 * 64 + 7
    dp = M.rotated_len(d, k)
    x = inputs(np.random.default_rng(8), d)
    buf = np.zeros(dp, np.float32); buf[:d] = x
    assert rot_call(hiplib, 0, SEEDS[2], [buf], d, k, 0, [buf]) == 0
    want = M.rotate(x, SEEDS[2], k)
    assert buf.tobytes() == want.tobytes()
    assert rot_call(hiplib, 0, SEEDS[2], [buf], dp, k, 1, [buf]) == 0
    assert buf.tobytes() == M.rotate(want, SEEDS[2], k, inverse=True).tobytes()


def test_every_bad_parameter_is_refused(hiplib):
    x, o = np.zeros(64, np.float32), np.full(64, 7.0, np.float32)
    sb = SEEDS[0]
    ok = lambda *a, **kw: rot_call(hiplib, None, *a, **kw)
    assert ok(sb, [x], 64, 23, 0, [o]) == 11                       # k > 22
    assert ok(sb, [x], 64, 5, 2, [o]) == 11 and ok(sb, [x], 64, 5, -1, [o]) == 11
    assert ok(None, [x], 64, 5, 0, [o]) == 11
    assert ok(sb, None, 64, 5, 0, [o], n_vec=1) == 11 and ok(sb, [x], 64, 5, 0, None) == 11
    assert ok(sb, [None], 64, 5, 0, [o]) == 11 and ok(sb, [x], 64, 5, 0, [None]) == 11
    assert ok(sb, [x], 64, 5, 0, [o], n_vec=65536) == 11           # (refused before an entry is read)
    assert ok(sb, [x], 1 << 28, 0, 0, [o]) == 11                   # dp >= 2^28
    assert ok(sb, [x], (1 << 28) - 1, 1, 0, [o]) == 11             # d < 2^28 <= dp
    assert ok(sb, [x], (1 << 22) * 63 + 1, 22, 0, [o]) == 11
    assert ok(sb, [x], 63, 5, 1, [o]) == 11 and ok(sb, [x], 33, 5, 1, [o]) == 11      # the inverse takes whole blocks
    assert rot_call(hiplib, 2, sb, [x], 64, 5, 0, [o]) == 11       # no such route
    assert (o == 7.0).all()
    # nothing to do: 0, and nothing is written
    assert ok(sb, [], 64, 5, 0, [], n_vec=0) == 0 and ok(None, None, 64, 5, 0, None, n_vec=0) == 0
    assert ok(sb, [x], 0, 5, 0, [o]) == 0 and ok(sb, [x], 0, 5, 1, [o]) == 0 and (o == 7.0).all()
    assert hiplib.rofl_dbg_rotate_tile_log2() in range(12, 15)


def test_python_helpers():
    import rofl_project_code_amd as R
    rl = R.range_proof_vec.rotated_len
    assert [rl(d, 12) for d in (0, 1, 4095, 4096, 4097, 55000)] == [0, 4096, 4096, 4096, 8192, 57344]
    assert rl(55000, 16) == 65536 and rl(5, 0) == 5 and rl(257, 8) == 512
    for bad in ((-1, 3), (5, 23), (5, -1)):
        with pytest.raises(ValueError):
            rl(*bad)
    pub = b"model hash of the round"
    assert R.pedersen_ops.rotate_round_seed(pub, 7) == hashlib.sha3_256(b"rofl-zk/rotate/v1/round" + pub + struct.pack("<Q", 7)).digest()
    assert R.pedersen_ops.rotate_round_seed(pub, 7) != R.pedersen_ops.rotate_round_seed(pub, 8)
    # rotate_vecs: a single seed is repeated, a list gives each vector its own; destinations of the rotated length
    xs = [inputs(np.random.default_rng(i), 70, special=False) for i in range(3)]
    same = R.range_proof_vec.rotate_vecs(xs, SEEDS[0], 5)
    own = R.range_proof_vec.rotate_vecs(xs, SEEDS, 5)
    assert same.shape == own.shape == (3, 96)
    for v in range(3):
        assert same[v].tobytes() == M.rotate(xs[v], SEEDS[0], 5).tobytes() and own[v].tobytes() == M.rotate(xs[v], SEEDS[v], 5).tobytes()
    dst = [np.zeros(96, np.float32) for _ in xs]
    assert R.range_proof_vec.rotate_vecs(xs, SEEDS, 5, out=dst) is not None and all(a.tobytes() == b.tobytes() for a, b in zip(dst, own))
    with pytest.raises(ValueError):
        R.range_proof_vec.rotate_vecs(xs, SEEDS, 5, out=[np.zeros(70, np.float32) for _ in xs])
    with pytest.raises(ValueError):
        R.range_proof_vec.rotate_vecs(xs, SEEDS[:2], 5)
    with pytest.raises(R.RoflError):
        R.range_proof_vec.unrotate(xs[0], SEEDS[0], 5)      # 70 elements are not whole blocks


def test_the_rust_declaration_matches_the_header():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "check_ffi.py")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout
    ffi = open(os.path.join(ROOT, "integration", "rofl_crypto_overlay", "src", "ffi.rs")).read()
    assert "pub fn rofl_rotate(" in ffi
