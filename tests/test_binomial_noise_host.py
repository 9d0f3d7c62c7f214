"""CPU-only checks of the distributed noise (rofl_noise_binomial): the host-compiled stream and value rule against the Python model
(tests/noise_model.py) bit for bit, splitting with `first`, in place, the value rule exactly on the clip bounds, every parameter check of
the C entry point (they come before the device is touched), the moments and the closure under addition of the definition, the Python
helpers, the containers' keywords and the Rust declaration.  No call here reaches a GPU: route 0 of rofl_dbg_noise_binomial_route is the
library's host route, compiled from the kernel's source."""
import ctypes
import inspect
import math
import os
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

import noise_model as M
import quant_model as Q

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sz = ctypes.c_size_t
SEED = bytes(range(32))
FORMATS = ((16, 16, 7), (8, 8, 7), (32, 32, 7), (64, 64, 12), (8, 16, 12))      # (prove_range, fp_bits, fp_frac): those of the prob-quant host test
WIDTHS = (1, 2, 3, 32, 33, 64)                                                    # W = k / 16
SHAPES = [(d, first) for d in (1, 31, 33, 100) for first in (0, 5, 37)]           # first W is and is not a multiple of 32


def noise_call(L, route, n_vec, seeds, values, first, d, k, nb, fb, ff, outs):
    """rofl_noise_binomial (route None) or rofl_dbg_noise_binomial_route with the given raw arguments (None = a null pointer)"""
    arr = lambda xs: (ctypes.c_void_p * len(xs))(*[(x.data_ptr() if hasattr(x, "data_ptr") else x.ctypes.data) if x is not None else None for x in xs]) if xs is not None else None
    args = [sz(n_vec), seeds, arr(values), sz(first), sz(d), ctypes.c_uint32(k), sz(nb), ctypes.c_uint(fb), ctypes.c_uint(ff), arr(outs)]
    return L.rofl_noise_binomial(*args) if route is None else L.rofl_dbg_noise_binomial_route(ctypes.c_uint(route), *args)


def noise_apply(L, site, vals_bits, noise, nb, fb, ff):
    """rofl_dbg_noise_apply -> output bits"""
    v = np.ascontiguousarray(vals_bits, np.uint32)
    n = np.ascontiguousarray(noise, np.int32)
    out = np.full(v.size, 0x7fc00001, np.uint32)
    L.rofl_dbg_noise_apply.argtypes = [ctypes.c_uint, sz, ctypes.c_void_p, ctypes.c_void_p, sz, ctypes.c_uint, ctypes.c_uint, ctypes.c_void_p]
    assert L.rofl_dbg_noise_apply(site, v.size, v.ctypes.data, n.ctypes.data, nb, fb, ff, out.ctypes.data) == 0
    return out


def inputs(rng, d, nb, fb, ff):
    """values of a few grid steps, both signs, on and off the grid, scaled into the clip range"""
    mx = float(Q.value(Q.clip_bounds(nb, fb, ff)[1]))
    return rng.uniform(-3, 3, d).astype(np.float32) * np.float32(min(1.0, mx / 3))


_BOUNDARY = {}


def boundary_cases(nb, fb, ff):
    """-> (value bits, noise, expected bits): noise chosen so that q + n lands on max, max + 1 step, min, min - 1 step, on 0 from both sides
    and one step past it; +-0.0 inputs; NaN and both infinities with and without noise; at the 32-bit format a value of 2^24 steps or more"""
    key = (nb, fb, ff)
    if key not in _BOUNDARY:
        mx_bits = Q.clip_bounds(nb, fb, ff)[1]
        MX = int(Q.value(mx_bits) * (1 << ff))
        cases = []
        for q in sorted({0, 1, 5, min(MX, 100), max(MX - 3, 0), MX}):
            for sign in (1, -1):
                cases += [(sign * q, MX - sign * q), (sign * q, MX + 1 - sign * q), (sign * q, -MX - sign * q), (sign * q, -MX - 1 - sign * q),
                          (sign * q, -sign * q), (sign * q, -sign * q + 1), (sign * q, -sign * q - 1), (sign * q, 0)]
        cases = [(q, n) for q, n in dict.fromkeys(cases) if abs(n) <= M.K_MAX]
        vb = [Q.round_f32(Fraction(q, 1 << ff)) for q, _ in cases]
        ns = [n for _, n in cases]
        for n in (0, 1, -1, 16, -M.K_MAX, M.K_MAX):
            vb += [0x00000000, 0x80000000] + list(Q.NAN_BITS) + [Q.INF, Q.INF | Q.SIGN]
            ns += [n] * (4 + len(Q.NAN_BITS))
        # off the grid: step 2 rounds to nearest, ties to even (half, one and a half, a quarter of a step)
        for num in (1, 3, 5, -1, -3, -5):
            for den in (2, 4):
                vb.append(Q.round_f32(Fraction(num, den << ff))); ns.append(3)
        if fb == 32 and nb == 32:
            for q in ((1 << 24), (1 << 24) + 2, (1 << 25) + 4, (1 << 30)):
                for n in (1, -1, 2, 3, -3, 1 << 20):
                    vb += [Q.round_f32(Fraction(q, 1 << ff)), Q.round_f32(Fraction(-q, 1 << ff))]; ns += [n, n]
        want = [M.apply_bits(b, n, nb, fb, ff) for b, n in zip(vb, ns)]
        _BOUNDARY[key] = (np.array(vb, np.uint32), np.array(ns, np.int32), np.array(want, np.uint32))
    return _BOUNDARY[key]


def test_known_answers_pin_label_and_indexing(hiplib):
    def lib_noise(e, k):
        n = ctypes.c_int32(99)
        assert hiplib.rofl_dbg_host_noise(SEED, ctypes.c_uint64(e), ctypes.c_uint32(k), ctypes.byref(n)) == 0
        return n.value
    for first, d, k, want in ((0, 4, 16, [1, -3, 1, 4]), (5, 3, 48, [-3, 5, -4]), (0, 2, 528, [2, 5])):
        assert [lib_noise(first + i, k) for i in range(d)] == want, (first, k)
        assert M.noise(SEED, first, d, k).tolist() == want
    for e, k in ((2 ** 40 + 3, 16), (77, 1 << 20), ((1 << 63) // 3 - 1, 48)):
        assert lib_noise(e, k) == int(M.noise(SEED, e, 1, k)[0]), (e, k)
    # the rounding stream of the same seed is another XOF output
    import pq_model
    assert pq_model.block(SEED, 0) != M.block(SEED, 0) and len(pq_model.LABEL) == len(M.LABEL)


GRID_SEEDS = [bytes([v + 1]) * 32 for v in range(3)]
_GRID = {}


def grid_cases(nb, fb, ff, W):
    """-> [(d, first, the values of three vectors, the model's outputs for GRID_SEEDS)] over SHAPES: computed once, shared by the host test
    and the device test (tests/test_gpu_binomial_noise.py), and never written"""
    key = (nb, fb, ff, W)
    if key not in _GRID:
        rng = np.random.default_rng(fb * 1000 + ff * 10 + W)
        _GRID[key] = []
        for d, first in SHAPES:
            vals = [inputs(rng, d, nb, fb, ff) for _ in GRID_SEEDS]
            _GRID[key].append((d, first, vals, [M.add_noise(x, s, 16 * W, nb, fb, ff, first) for x, s in zip(vals, GRID_SEEDS)]))
    return _GRID[key]


def check_grid(L, route, nb, fb, ff, W):
    for d, first, vals, want in grid_cases(nb, fb, ff, W):
        outs = [np.full(d, np.nan, np.float32) for _ in vals]
        assert noise_call(L, route, 3, b"".join(GRID_SEEDS), [x.copy() for x in vals], first, d, 16 * W, nb, fb, ff, outs) == 0
        for v in range(3):
            assert outs[v].tobytes() == want[v].tobytes(), (W, d, first, v, np.nonzero(outs[v].view(np.uint32) != want[v].view(np.uint32))[0][:5])


@pytest.mark.parametrize("W", WIDTHS)
@pytest.mark.parametrize("nb,fb,ff", FORMATS, ids=["r%d_fp%d_%d" % f for f in FORMATS])
def test_host_route_equals_the_model(hiplib, nb, fb, ff, W):
    check_grid(hiplib, 0, nb, fb, ff, W)


def test_the_entry_point_takes_the_host_route_for_small_host_calls(hiplib):
    """rofl_noise_binomial itself, all pointers in host memory, few permutations: no GPU here, so the host route it is"""
    x = inputs(np.random.default_rng(2), 33, 16, 16, 7)
    out = np.zeros(33, np.float32)
    assert noise_call(hiplib, None, 1, SEED, [x], 5, 33, 48, 16, 16, 7, [out]) == 0
    assert out.tobytes() == M.add_noise(x, SEED, 48, 16, 16, 7, 5).tobytes()


def test_runs_split_with_first_concatenate_and_in_place(hiplib):
    nb, fb, ff = 16, 16, 7
    for W in (1, 3, 33):
        x = inputs(np.random.default_rng(W), 100, nb, fb, ff)
        whole, a, b = np.zeros(100, np.float32), np.zeros(37, np.float32), np.zeros(63, np.float32)
        assert noise_call(hiplib, 0, 1, SEED, [x], 0, 100, 16 * W, nb, fb, ff, [whole]) == 0
        assert noise_call(hiplib, 0, 1, SEED, [x[:37].copy()], 0, 37, 16 * W, nb, fb, ff, [a]) == 0
        assert noise_call(hiplib, 0, 1, SEED, [x[37:].copy()], 37, 63, 16 * W, nb, fb, ff, [b]) == 0
        assert np.concatenate([a, b]).tobytes() == whole.tobytes() == M.add_noise(x, SEED, 16 * W, nb, fb, ff).tobytes(), W
        y = x.copy()
        assert noise_call(hiplib, 0, 1, SEED, [y], 0, 100, 16 * W, nb, fb, ff, [y]) == 0 and y.tobytes() == whole.tobytes()


@pytest.mark.parametrize("nb,fb,ff", FORMATS, ids=["r%d_fp%d_%d" % f for f in FORMATS])
def test_value_rule_on_the_bounds(hiplib, nb, fb, ff):
    vb, ns, want = boundary_cases(nb, fb, ff)
    got = noise_apply(hiplib, 0, vb, ns, nb, fb, ff)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, [(hex(vb[i]), int(ns[i]), hex(got[i]), hex(want[i])) for i in bad[:5]]
    mx = Q.clip_bounds(nb, fb, ff)[1]
    assert (want == mx).any() and (want == mx | Q.SIGN).any() and (want == 0).any() and vb.size > 80
    assert not (want == Q.SIGN).any(), "a zero result is +0.0"
    # what lands one step inside a bound is not the bound (at formats where a step is still a float's step there)
    if Q.value(mx) * (1 << ff) < 1 << 24:
        MX = int(Q.value(mx) * (1 << ff))
        inner = noise_apply(hiplib, 0, [0, 0], [MX - 1, 1 - MX], nb, fb, ff)
        assert [int(Q.value(int(b)) * (1 << ff)) for b in inner] == [MX - 1, 1 - MX]


def test_parameter_checks_come_before_the_device(hiplib):
    L = hiplib
    x, out = np.full(4, 0.3, np.float32), np.zeros(4, np.float32)
    ok = dict(route=None, n_vec=1, seeds=SEED, values=[x], first=0, d=4, k=16, nb=16, fb=16, ff=7, outs=[out])
    call = lambda **kw: noise_call(L, **dict(ok, **kw))
    assert call(seeds=None) == 11 and call(values=None) == 11 and call(outs=None) == 11      # null arrays with n_vec > 0
    assert call(values=[None]) == 11 and call(outs=[None]) == 11                                # null entries with d > 0
    assert call(n_vec=2, seeds=SEED * 2, values=[x, None], outs=[out, out]) == 11
    for fb, ff in ((12, 7), (16, 13), (8, 8), (0, 0)):
        assert call(fb=fb, ff=ff) == 11, (fb, ff)
    assert call(nb=0) == 11
    n = 65536
    assert call(n_vec=n, seeds=SEED * n, values=[x] * n, outs=[out] * n) == 11
    assert call(d=1 << 28) == 11
    assert call(first=(1 << 63) - 3) == 11 and call(first=(1 << 64) - 2) == 11
    for k in (0, 8, 15, 17, 24, (1 << 20) + 16, 1 << 21, 0xfffffff0):                            # not a multiple of 16, or outside [16, 2^20]
        assert call(k=k) == 11 and call(k=k, n_vec=0) == 11 and call(k=k, d=0) == 11, k
        assert call(route=0, k=k) == 11 and call(route=1, k=k) == 11
    assert call(k=48, first=(1 << 63) // 3 - 3) == 11                                            # (first + d) W = 2^63 + 2 at W = 3
    assert call(k=1 << 20, first=(1 << 47) - 3) == 11
    assert call(route=2) == 11
    assert not out.any()
    err = ctypes.create_string_buffer(512)
    L.rofl_last_error(err, sz(512))
    assert SEED.hex() not in err.value.decode() and SEED not in err.raw
    # nothing to do: 0, nothing written, no device needed
    assert noise_call(L, None, 0, None, None, 0, 4, 16, 16, 16, 7, None) == 0
    assert call(d=0) == 0 and call(d=0, first=(1 << 63)) == 0 and call(d=0, values=[None], outs=[None]) == 0
    assert not out.any()
    assert call(first=(1 << 63) - 4) == 0 and out.tobytes() == M.add_noise(x, SEED, 16, 16, 16, 7, (1 << 63) - 4).tobytes()      # (first + d) W == 2^63 is allowed
    assert call(k=48, first=(1 << 63) // 3 - 4) == 0 and out.tobytes() == M.add_noise(x, SEED, 48, 16, 16, 7, (1 << 63) // 3 - 4).tobytes()
    # the debug entries
    n32 = ctypes.c_int32(7)
    h = lambda seed=SEED, e=0, k=16, o=ctypes.byref(n32): L.rofl_dbg_host_noise(seed, ctypes.c_uint64(e), ctypes.c_uint32(k), o)
    assert h(seed=None) == 11 and h(o=None) == 11 and h(k=8) == 11 and h(k=24) == 11 and h(k=(1 << 20) + 16) == 11 and h(e=1 << 63) == 11 and h(e=(1 << 63) // 3, k=48) == 11
    assert n32.value == 7
    L.rofl_dbg_noise_apply.argtypes = [ctypes.c_uint, sz, ctypes.c_void_p, ctypes.c_void_p, sz, ctypes.c_uint, ctypes.c_uint, ctypes.c_void_p]
    ns = np.zeros(4, np.int32)
    out[:] = 0
    r = lambda site=0, n=4, v=x.ctypes.data, n_=ns.ctypes.data, nb=16, fb=16, ff=7, o=out.ctypes.data: L.rofl_dbg_noise_apply(site, n, v, n_, nb, fb, ff, o)
    assert r(site=2) == 11 and r(v=None) == 11 and r(n_=None) == 11 and r(o=None) == 11 and r(nb=0) == 11 and r(fb=12) == 11 and r(n=(1 << 20) + 1) == 11
    assert r(n=0, v=None, n_=None, o=None) == 0 and not out.any()


def _moments(ns, k, N):
    mean = ns.mean()
    var = ((ns - mean) ** 2).mean()
    assert abs(mean) <= 5 * math.sqrt(k / (2 * N)), (k, mean)
    assert abs(var - k / 2) <= 5 * (k / 2) * math.sqrt(2 / N), (k, var)
    return mean, var


@pytest.mark.parametrize("k", (16, 48, 512))
def test_moments_of_the_host_route(hiplib, k):
    """N = 65 536 zeros, seed 00 01 .. 1f, fp (32, 7): the outputs are the noise itself; mean and variance within five standard errors of
    the exact distribution, and the hashlib model inside the same bounds"""
    N = 65536
    out = np.full(N, np.nan, np.float32)
    assert noise_call(hiplib, 0, 1, SEED, [np.zeros(N, np.float32)], 0, N, k, 32, 32, 7, [out]) == 0
    got = out.astype(np.float64) * 128
    want = M.noise(SEED, 0, N, k)
    assert (got == want).all()
    mean, var = _moments(want.astype(np.float64), k, N)
    if k == 512:
        assert abs(mean - 0.033) < 0.001 and abs(var - 256.76) < 0.01, (mean, var)


def test_the_noise_of_eight_seeds_adds_up_to_the_binomial_of_eight_k(hiplib):
    k, d = 48, 8192
    total = np.zeros(d, np.float64)
    seeds = [bytes([0x70 + c]) * 32 for c in range(8)]
    outs = [np.zeros(d, np.float32) for _ in seeds]
    assert noise_call(hiplib, 0, 8, b"".join(seeds), [np.zeros(d, np.float32)] * 8, 0, d, k, 32, 32, 7, outs) == 0
    for c, o in enumerate(outs):
        assert (o.astype(np.float64) * 128 == M.noise(seeds[c], 0, d, k)).all()
        total += o.astype(np.float64) * 128
    _moments(total, 8 * k, d)
    assert np.abs(total).max() <= 8 * k and len({o.tobytes() for o in outs}) == 8


def test_python_helpers(hiplib):
    from rofl_project_code_amd.api import range_proof_vec as rp, pedersen_ops
    x = np.full(4, 0.3, np.float32)
    for bad in (lambda: rp.add_binomial_noise(x, 16, SEED[:31], 16), lambda: rp.add_binomial_noise_vecs([x, x], 16, [SEED], 16),
                lambda: rp.add_binomial_noise_vecs([x, x[:3]], 16, [SEED, SEED], 16), lambda: rp.add_binomial_noise(x, 16, SEED, 16, first=-1),
                lambda: rp.add_binomial_noise(x, 0, SEED, 16), lambda: rp.add_binomial_noise(x, 16, SEED, 24), lambda: rp.add_binomial_noise(x, 16, SEED, 0),
                lambda: rp.add_binomial_noise(x, 16, SEED, (1 << 20) + 16), lambda: rp.add_binomial_noise_vecs([x], 16, [SEED], 16, out=[np.zeros(3, np.float32)])):
        with pytest.raises(ValueError):
            bad()
    assert rp.add_binomial_noise_vecs([], 16, [], 16).shape == (0, 0)
    got = rp.add_binomial_noise(x, 16, SEED, 48, first=7, fp=(16, 7))
    assert got.dtype == np.float32 and got.tobytes() == M.add_noise(x, SEED, 48, 16, 16, 7, 7).tobytes()
    both = rp.add_binomial_noise_vecs([x, -x], 8, [SEED, SEED[::-1]], 16, fp=(8, 7))
    assert both[0].tobytes() == M.add_noise(x, SEED, 16, 8, 8, 7).tobytes() and both[1].tobytes() == M.add_noise(-x, SEED[::-1], 16, 8, 8, 7).tobytes()
    y = x.copy()
    assert rp.add_binomial_noise_vecs([y], 16, [SEED], 16, fp=(16, 7), out=[y])[0] is y and y.tobytes() == M.add_noise(x, SEED, 16, 16, 16, 7).tobytes()
    # the rounding wrapper still gives the rounding model's bytes through the marshalling the two calls share
    import pq_model
    assert rp.quantize_probabilistic(x, 16, SEED, first=7, fp=(16, 7)).tobytes() == pq_model.quantize(x, SEED, 16, 16, 7, 7).tobytes()
    # binomial_noise_k: the smallest valid k with k / 2 >= sigma^2
    for sigma in (0, 0.5, 2, 2.8284, 2.83, 4, 64, 100.5, 724):
        assert rp.binomial_noise_k(sigma) == M.smallest_k(sigma), sigma
    assert rp.binomial_noise_k(64) == 8192 and rp.binomial_noise_k(0) == 16 and rp.binomial_noise_k(724) == 1048352 and rp.binomial_noise_k(Fraction(724077, 1000)) == 1 << 20
    with pytest.raises(ValueError):
        rp.binomial_noise_k(725)
    with pytest.raises(ValueError):
        rp.binomial_noise_k(-1)
    for r in (0, 7, 2 ** 40):
        assert pedersen_ops.noise_round_seed(b"client secret", r) == M.round_seed(b"client secret", r)
        assert pedersen_ops.noise_round_seed(b"client secret", r) != pedersen_ops.quant_round_seed(b"client secret", r)
    assert "secret" in pedersen_ops.noise_round_seed.__doc__.lower() and "secret" in rp.add_binomial_noise_vecs.__doc__.lower()


@pytest.mark.parametrize("nb,fb,ff,k", ((16, 16, 7, 48), (8, 8, 7, 16), (8, 16, 12, 32), (16, 32, 7, 1024)))
def test_clipped_for_noise_never_saturates(hiplib, nb, fb, ff, k):
    """clip_f32_for_noise, then quantize onto the grid (nearest), then noise: the output is exactly q + n_e steps, no clip in between"""
    from rofl_project_code_amd.api import range_proof_vec as rp
    mx = float(Q.value(Q.clip_bounds(nb, fb, ff)[1]))
    rng = np.random.default_rng(k)
    x = np.concatenate([rng.uniform(-2 * mx, 2 * mx, 300), [mx, -mx, np.inf, -np.inf, np.nan, 0.0]]).astype(np.float32)
    c = rp.clip_f32_for_noise(x, nb, k, fp=(fb, ff))
    lim = mx - k / (1 << ff)
    assert c.dtype == np.float32 and np.abs(c).max() == np.float32(lim) and (np.abs(c) <= lim).all() and c[-2] == np.float32(-lim)
    inside = np.abs(x) <= lim
    assert inside.sum() > 50 and (c[inside] == x[inside]).all()
    grid = (np.round(c.astype(np.float64) * (1 << ff)) / (1 << ff)).astype(np.float32)      # on the grid, still inside the interval
    out = np.zeros(grid.size, np.float32)
    assert noise_call(hiplib, 0, 1, SEED, [grid], 3, grid.size, k, nb, fb, ff, [out]) == 0
    want = M.unsaturated_steps(grid, SEED, k, fb, ff, 3)
    assert (out.astype(np.float64) * (1 << ff)).tolist() == [float(w) for w in want]
    assert max(abs(w) for w in want) <= mx * (1 << ff)
    # without it the same inputs do saturate
    raw = rp.clip_f32_to_range_vec(x, nb, fp=(fb, ff))
    out2 = np.zeros(raw.size, np.float32)
    assert noise_call(hiplib, 0, 1, SEED, [raw], 3, raw.size, k, nb, fb, ff, [out2]) == 0
    assert (np.abs(out2) == np.float32(mx)).any()
    with pytest.raises(ValueError):
        rp.clip_f32_for_noise(x, nb, int(mx * (1 << ff)) + 16, fp=(fb, ff))


def test_containers_take_the_noise_keywords(hiplib, monkeypatch):
    """encrypt(noise_seed=, noise_k=) and encrypt_batch_private hand every leg the noised values -- after the rounding of a quant seed where
    there is one -- and without noise seeds exactly what encrypt_batch_quantized hands them; one noise call per batch.  The legs are
    replaced by recorders: nothing here reaches a device."""
    import pq_model
    from rofl_project_code_amd import api, params
    seen = {}

    class Stop(Exception):
        pass

    def commitments(clipped, bl, prove_range, fp):
        seen["clipped"] = np.array(clipped, np.float32)
        raise Stop()
    monkeypatch.setattr(params, "_range_commitments", commitments)
    x = np.array([0.3, -0.3, 300.0, 1 / 512, -0.0], np.float32)
    bl, r2 = np.zeros((5, 32), np.uint8), np.zeros((5, 32), np.uint8)
    QS, NS, K = SEED[::-1], SEED, 48
    rounded = pq_model.quantize(x, QS, 16, 16, 7)
    noised = M.add_noise(x, NS, K, 16, 16, 7)
    both = M.add_noise(rounded, NS, K, 16, 16, 7)
    assert len({rounded.tobytes(), noised.tobytes(), both.tobytes()}) == 3
    cases = [(params.EncParamsRange, (2, 1.0), {}), (params.EncParamsRangeCompressed, (2, 1.0), {}), (params.EncParamsL2, (2, 32), dict(rand_scalars=r2)),
             (params.EncParamsL2Compressed, (2, 32), dict(rand_scalars=r2)), (params.EncParamsL2CompressedStrict, (2, 32), dict(rand_scalars=r2))]
    calls = []
    real = api.range_proof_vec.add_binomial_noise_vecs
    monkeypatch.setattr(api.range_proof_vec, "add_binomial_noise_vecs", staticmethod(lambda *a, **k: (calls.append(len(a[0])), real(*a, **k))[1]))
    for cls, tail, kw in cases:
        p = inspect.signature(cls.encrypt).parameters
        assert p["noise_seed"].default is None and p["noise_k"].default is None, cls
        assert list(inspect.signature(cls.encrypt_batch_private).parameters)[4:] == ["nonce_seeds", "fp", "quant_seeds", "noise_seeds", "noise_k"]
        one = [(x, bl) + tuple(kw.values())]
        for want, run in ((noised, lambda: cls.encrypt(x, bl, 16, *tail, fp=(16, 7), noise_seed=NS, noise_k=K, **kw)),
                          (both, lambda: cls.encrypt(x, bl, 16, *tail, fp=(16, 7), quant_seed=QS, noise_seed=NS, noise_k=K, **kw)),
                          (noised, lambda: cls.encrypt_batch_private(one, 16, *tail, fp=(16, 7), noise_seeds=[NS], noise_k=K)),
                          (both, lambda: cls.encrypt_batch_private(one, 16, *tail, fp=(16, 7), quant_seeds=[QS], noise_seeds=[NS], noise_k=K)),
                          (rounded, lambda: cls.encrypt_batch_private(one, 16, *tail, fp=(16, 7), quant_seeds=[QS], noise_seeds=[None], noise_k=K)),
                          (rounded, lambda: cls.encrypt_batch_private(one, 16, *tail, fp=(16, 7), quant_seeds=[QS]))):
            seen.clear()
            with pytest.raises(Stop):
                run()
            assert seen["clipped"].tobytes() == want.tobytes(), cls
        del calls[:]
        with pytest.raises(Stop):
            cls.encrypt_batch_private(one * 3, 16, *tail, fp=(16, 7), noise_seeds=[NS, None, NS], noise_k=K)
        assert calls == [2], "ONE noise call for all hosted clients that have a seed"
        for bad in (dict(noise_seeds=[NS]), dict(noise_k=K), dict(noise_seeds=[NS, NS], noise_k=K), dict(noise_seeds=[NS], noise_k=24)):
            with pytest.raises(ValueError):
                cls.encrypt_batch_private(one, 16, *tail, fp=(16, 7), **bad)
        for bad in (dict(noise_seed=NS), dict(noise_k=K)):
            with pytest.raises(ValueError):
                cls.encrypt(x, bl, 16, *tail, fp=(16, 7), **dict(kw, **bad))
        assert cls.encrypt_batch_private([], 16, *tail) == []


def test_entry_points_are_exported_and_declared_for_rust(hiplib):
    for name in ("rofl_noise_binomial", "rofl_dbg_host_noise", "rofl_dbg_noise_apply", "rofl_dbg_noise_binomial_route"):
        assert hasattr(hiplib, name), name
    hdr = open(os.path.join(ROOT, "include", "rofl_zk.h")).read()
    assert "int rofl_noise_binomial(" in hdr and "rofl-zk/noise/v1" in hdr
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "check_ffi.py")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    ffi = open(os.path.join(ROOT, "integration", "rofl_crypto_overlay", "src", "ffi.rs")).read()
    assert "pub fn rofl_noise_binomial(" in ffi
    overlay = open(os.path.join(ROOT, "integration", "rofl_crypto_overlay", "src", "range_proof_vec", "mod.rs")).read()
    assert "pub fn add_binomial_noise(" in overlay and "rofl_noise_binomial(" in overlay
    assert "add_binomial_noise" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
