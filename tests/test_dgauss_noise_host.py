"""CPU-only checks of the discrete Gaussian noise (rofl_noise_dgauss): the known answers of the definition out of the Python model
(tests/dgauss_model.py), the golden file and the host-compiled sampler alike; the host route byte for byte against the model over variance
parameters, lengths, offsets and formats; splitting with `first`, in place; the value rule on the clip bounds with this noise's
magnitudes; the sampler on crafted word lists; every parameter check of the C entry point (they come before the device is touched); the
distribution against the exact pmf and its closure under addition; the Python helpers, the containers' keywords and the Rust
declaration.  No call here reaches a GPU: route 0 of rofl_dbg_noise_dgauss_route is the library's host route, compiled from the kernel's
source."""
import ctypes
import hashlib
import inspect
import json
import math
import os
import struct
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

import dgauss_model as M
import noise_model as NM
import quant_model as Q
from test_binomial_noise_host import FORMATS, inputs, noise_apply

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "dgauss.json")))
sz = ctypes.c_size_t
SEED = bytes(range(32))
SIGMA2S = (1, 2, 3, 15, 16, 4096, 1 << 16, 1 << 24)
SHAPES = [(d, first) for d in (1, 31, 33, 100) for first in (0, 5, 2 ** 40 + 3)]
GRID_SEEDS = [bytes([v + 1]) * 32 for v in range(3)]
FF = 0xffffffff


def dg_call(L, route, n_vec, seeds, values, first, d, sigma2, nb, fb, ff, outs):
    """rofl_noise_dgauss (route None) or rofl_dbg_noise_dgauss_route with the given raw arguments (None = a null pointer)"""
    arr = lambda xs: (ctypes.c_void_p * len(xs))(*[(x.data_ptr() if hasattr(x, "data_ptr") else x.ctypes.data) if x is not None else None for x in xs]) if xs is not None else None
    args = [sz(n_vec), seeds, arr(values), sz(first), sz(d), ctypes.c_uint32(sigma2), sz(nb), ctypes.c_uint(fb), ctypes.c_uint(ff), arr(outs)]
    return L.rofl_noise_dgauss(*args) if route is None else L.rofl_dbg_noise_dgauss_route(ctypes.c_uint(route), *args)


def host_element(L, e, sigma2, seed=SEED):
    """rofl_dbg_host_dgauss -> (noise, words used)"""
    n, u = ctypes.c_int32(99), ctypes.c_uint32(99)
    assert L.rofl_dbg_host_dgauss(seed, ctypes.c_uint64(e), ctypes.c_uint32(sigma2), ctypes.byref(n), ctypes.byref(u)) == 0
    return n.value, u.value


def words_call(L, site, cases):
    """rofl_dbg_dgauss_words over cases [(word list, sigma2)] -> [(finished, noise, used)] as the model's on_words gives them"""
    n = len(cases)
    stride = max(len(w) for w, _ in cases)
    buf = np.zeros((n, max(stride, 1)), np.uint32)
    for i, (w, _) in enumerate(cases):
        buf[i, :len(w)] = w
    lens, s2s = np.array([len(w) for w, _ in cases], np.uint32), np.array([s for _, s in cases], np.uint32)
    noise, used, fin = np.full(n, 77, np.int32), np.full(n, 77, np.uint32), np.full(n, 77, np.uint32)
    L.rofl_dbg_dgauss_words.argtypes = [ctypes.c_uint, sz, ctypes.c_void_p, sz] + [ctypes.c_void_p] * 5
    assert L.rofl_dbg_dgauss_words(site, n, buf.ctypes.data, stride, lens.ctypes.data, s2s.ctypes.data, noise.ctypes.data, used.ctypes.data, fin.ctypes.data) == 0
    return [(bool(f), int(x), int(u)) for f, x, u in zip(fin, noise, used)]


RESTART = [0, 0] + [0, 1] * 64      # sigma2 = 1: U = 0 accepted, then 64 steps of V: the V = 64 restart, 130 words


def crafted_cases():
    """[(word list, sigma2, what the definition gives or None)]: the lists of the definition's known answers, a list one word short of a
    finished sample, the exhaustion at exactly 8 192 words (zeros; restarts without end), and two-word draws cut between lo and hi"""
    big = 1 << 24      # (two-word draws: the stream of an element, whole and cut between the lo and the hi word of its last draw)
    noise, used = M.element(SEED, 1 << 40, big)
    stream = [w for j in range((used + 31) >> 5) for w in struct.unpack("<32I", M.block(SEED, 1 << 40, j))][:used]
    first_2w = (True, noise, used)
    return [([], 1, (False, 0, 0)), ([0] * 64, 1, (False, 0, 64)), ([FF] * 8192, 1, (True, -1, 5)), (RESTART + [FF] * 5, 1, (True, -1, 135)),
            (RESTART + [FF] * 4, 1, (False, 0, 134)), ([FF] * 4, 1, (False, 0, 4)), ([FF] * 5, 1, (True, -1, 5)),
            ([0] * 8192, 1, (False, 0, 8192)), ((RESTART * 64)[:8192], 1, (False, 0, 8192)), ([0] * 8191, 4096, (False, 0, 8191)),
            (stream, big, first_2w), (stream[:-1], big, (False, 0, used - 1)), (stream + [7, 7], big, first_2w), ([FF] * 64, 4096, None), ([0x55555555] * 200, 50, None)]


_RANDOM = []


def random_cases():
    """4 096 lists of random words, of random length: cut anywhere in or after the sample -> [(words, sigma2)], and the model's results"""
    if not _RANDOM:
        rng = np.random.default_rng(4096)
        cases = [(rng.integers(0, 1 << 32, int(rng.integers(0, 70)), dtype=np.uint64).astype(np.uint32).tolist(), int(rng.choice(SIGMA2S))) for _ in range(4096)]
        _RANDOM.extend([cases, [M.on_words(w, s) for w, s in cases]])
    return _RANDOM


def test_known_answers_out_of_model_golden_file_and_host_twin(hiplib):
    """the answers the definition was published with (typed in here), the golden file (which holds them and what the model added) and the
    library's host twin"""
    ka = {(4096, 0): [18, 17, -74, -35, 145, -61, 44, -84, 61, -45, -14, 10], (1, 0): [-1, -1, 0, 0, 1, 0, 0, -1, -1, 1, -1, 0, 0, 0, 0, 1],
          (1 << 24, 1 << 40): [1386, -3911, -2418, 2205, 4240, -4010]}
    for (s2, first), want in ka.items():
        assert M.noise(SEED, first, len(want), s2).tolist() == want
        assert [host_element(hiplib, first + i, s2)[0] for i in range(len(want))] == want
        assert GOLDEN["noise"]["%d:%d" % (s2, first)][:len(want)] == want
    for s2, e, used in ((4096, 7, 8), (4096, 3565, 157), (4096, 9406, 168), (1 << 24, 11567, 180)):
        assert M.element(SEED, e, s2)[1] == used and host_element(hiplib, e, s2) == M.element(SEED, e, s2)
        assert GOLDEN["words_used"]["%d:%d" % (s2, e)] == used
    # what the model added: longer runs at every sigma2 of the grid, from 0 and from a high index
    for key, want in GOLDEN["noise"].items():
        s2, first = map(int, key.split(":"))
        assert M.noise(SEED, first, len(want), s2).tolist() == want, key
    for key, e_list in GOLDEN["ring_overruns"].items():
        assert [e for e in e_list if M.element(SEED, e, int(key), True)[2] >= 2] == e_list
    assert (M.on_words([], 1), M.on_words([0] * 64, 1), M.on_words([FF] * 8192, 1), M.on_words(RESTART + [FF] * 30, 1)) == \
        ((False, 0, 0), (False, 0, 64), (True, -1, 5), (True, -1, 135))
    import noise_model
    assert noise_model.block(SEED, 0) != M.block(SEED, 0, 0) and len(noise_model.LABEL) == len(M.LABEL) == 16


_NOISE = {}


def model_noise(seed, first, d, s2):
    """the model's noise integers, computed once per (seed, first, d, sigma2) for every format and for the device test"""
    key = (seed, first, d, s2)
    if key not in _NOISE:
        _NOISE[key] = M.noise(seed, first, d, s2)
    return _NOISE[key]


def check_grid(L, route, nb, fb, ff, s2, shapes=SHAPES):
    rng = np.random.default_rng(fb * 1000 + ff * 10 + s2 % 997)
    for d, first in shapes:
        vals = [inputs(rng, d, nb, fb, ff) for _ in GRID_SEEDS]
        outs = [np.full(d, np.nan, np.float32) for _ in vals]
        assert dg_call(L, route, 3, b"".join(GRID_SEEDS), [x.copy() for x in vals], first, d, s2, nb, fb, ff, outs) == 0
        for v in range(3):
            want = M.add_noise(vals[v], GRID_SEEDS[v], s2, nb, fb, ff, first, ns=model_noise(GRID_SEEDS[v], first, d, s2))
            assert outs[v].tobytes() == want.tobytes(), (s2, d, first, v, np.nonzero(outs[v].view(np.uint32) != want.view(np.uint32))[0][:5])


@pytest.mark.parametrize("s2", SIGMA2S)
@pytest.mark.parametrize("nb,fb,ff", FORMATS, ids=["r%d_fp%d_%d" % f for f in FORMATS])
def test_host_route_equals_the_model(hiplib, nb, fb, ff, s2):
    assert M.uses_two_word_draws(s2) == (s2 >= 1 << 16), "from 2^16 on step 4 draws below a bound of more than 32 bits: two words a draw"
    check_grid(hiplib, 0, nb, fb, ff, s2)


def test_the_entry_point_takes_the_host_route_for_small_host_calls(hiplib):
    x = inputs(np.random.default_rng(2), 33, 16, 16, 7)
    out = np.zeros(33, np.float32)
    assert dg_call(hiplib, None, 1, SEED, [x], 5, 33, 50, 16, 16, 7, [out]) == 0
    assert out.tobytes() == M.add_noise(x, SEED, 50, 16, 16, 7, 5).tobytes()


def test_runs_split_with_first_concatenate_and_in_place(hiplib):
    nb, fb, ff = 16, 16, 7
    for s2 in (1, 50, 1 << 16):
        x = inputs(np.random.default_rng(s2), 100, nb, fb, ff)
        whole, a, b = np.zeros(100, np.float32), np.zeros(37, np.float32), np.zeros(63, np.float32)
        assert dg_call(hiplib, 0, 1, SEED, [x], 0, 100, s2, nb, fb, ff, [whole]) == 0
        assert dg_call(hiplib, 0, 1, SEED, [x[:37].copy()], 0, 37, s2, nb, fb, ff, [a]) == 0
        assert dg_call(hiplib, 0, 1, SEED, [x[37:].copy()], 37, 63, s2, nb, fb, ff, [b]) == 0
        assert np.concatenate([a, b]).tobytes() == whole.tobytes() == M.add_noise(x, SEED, s2, nb, fb, ff).tobytes(), s2
        y = x.copy()
        assert dg_call(hiplib, 0, 1, SEED, [y], 0, 100, s2, nb, fb, ff, [y]) == 0 and y.tobytes() == whole.tobytes()


_BOUNDARY = {}


def boundary_cases(nb, fb, ff):
    """-> (value bits, noise, expected bits): the value rule with the magnitudes this noise has -- up to 64 t - 1 = 262 207 steps -- landing
    on max, one step past it, min, one step past it, zero from both sides; NaN, infinities and both zeros with such noise"""
    key = (nb, fb, ff)
    if key not in _BOUNDARY:
        MX = int(Q.value(Q.clip_bounds(nb, fb, ff)[1]) * (1 << ff))
        NMAX = 262207
        cases = []
        for q in sorted({0, 1, 5, min(MX, 100), max(MX - 3, 0), MX}):
            for sign in (1, -1):
                cases += [(sign * q, MX - sign * q), (sign * q, MX + 1 - sign * q), (sign * q, -MX - sign * q), (sign * q, -MX - 1 - sign * q),
                          (sign * q, -sign * q), (sign * q, -sign * q + 1), (sign * q, NMAX), (sign * q, -NMAX), (sign * q, 4096), (sign * q, -4097)]
        cases = [(q, n) for q, n in dict.fromkeys(cases) if abs(n) <= NMAX]
        vb = [Q.round_f32(Fraction(q, 1 << ff)) for q, _ in cases]
        ns = [n for _, n in cases]
        for n in (0, 1, -1, NMAX, -NMAX):
            vb += [0x00000000, 0x80000000] + list(Q.NAN_BITS) + [Q.INF, Q.INF | Q.SIGN]
            ns += [n] * (4 + len(Q.NAN_BITS))
        want = [NM.apply_bits(b, n, nb, fb, ff) for b, n in zip(vb, ns)]
        _BOUNDARY[key] = (np.array(vb, np.uint32), np.array(ns, np.int32), np.array(want, np.uint32))
    return _BOUNDARY[key]


@pytest.mark.parametrize("nb,fb,ff", FORMATS, ids=["r%d_fp%d_%d" % f for f in FORMATS])
def test_value_rule_on_the_bounds_with_this_noise(hiplib, nb, fb, ff):
    vb, ns, want = boundary_cases(nb, fb, ff)
    got = noise_apply(hiplib, 0, vb, ns, nb, fb, ff)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, [(hex(vb[i]), int(ns[i]), hex(got[i]), hex(want[i])) for i in bad[:5]]
    mx = Q.clip_bounds(nb, fb, ff)[1]
    assert (want == mx).any() and (want == mx | Q.SIGN).any() and (want == 0).any() and vb.size > 80 and np.abs(ns).max() == 262207
    assert not (want == Q.SIGN).any(), "a zero result is +0.0"


def test_sampler_on_crafted_words(hiplib):
    cases = crafted_cases()
    got = words_call(hiplib, 0, [(w, s) for w, s, _ in cases])
    for (w, s, want), g in zip(cases, got):
        assert g == M.on_words(w, s), (len(w), s, g)
        if want is not None:
            assert g == tuple(want), (len(w), s, g, want)
    cases, want = random_cases()
    got = words_call(hiplib, 0, cases)
    assert got == want
    fin = sum(f for f, _, _ in want)
    assert 1000 < fin < 3500, "the cuts fall inside the sample and after it"
    assert any(M.uses_two_word_draws(s) and f for (_, s), (f, _, _) in zip(cases, want))


def test_parameter_checks_come_before_the_device(hiplib):
    L = hiplib
    x, out = np.full(4, 0.3, np.float32), np.zeros(4, np.float32)
    ok = dict(route=None, n_vec=1, seeds=SEED, values=[x], first=0, d=4, sigma2=9, nb=16, fb=16, ff=7, outs=[out])
    call = lambda **kw: dg_call(L, **dict(ok, **kw))

    def err():
        buf = ctypes.create_string_buffer(512)
        L.rofl_last_error(buf, sz(512))
        assert SEED.hex() not in buf.value.decode() and SEED not in buf.raw
        return buf.value.decode()
    for kw in (dict(seeds=None), dict(values=None), dict(outs=None), dict(values=[None]), dict(outs=[None]),
               dict(n_vec=2, seeds=SEED * 2, values=[x, None], outs=[out, out]), dict(nb=0), dict(fb=12, ff=7), dict(fb=16, ff=13), dict(fb=8, ff=8), dict(fb=0, ff=0)):
        assert call(**kw) == 11 and "bad parameter" in err(), kw
    n = 65536
    assert call(n_vec=n, seeds=SEED * n, values=[x] * n, outs=[out] * n) == 11 and "more than 65 535 vectors" in err()
    assert call(d=1 << 28) == 11 and "vector length of 2^28 or more" in err()
    for first in ((1 << 55) - 3, 1 << 55, (1 << 55) + 1, 1 << 63, (1 << 64) - 2):
        assert call(first=first) == 11 and "first + d exceeds 2^55" in err(), first
    for s2 in (0, (1 << 24) + 1, 1 << 25, 0xffffffff):
        assert call(sigma2=s2) == 11 and "sigma2 is an integer from 1 to 2^24" in err(), s2
        assert call(sigma2=s2, n_vec=0) == 11 and call(sigma2=s2, d=0) == 11 and call(route=0, sigma2=s2) == 11 and call(route=1, sigma2=s2) == 11
    assert call(route=2) == 11
    assert not out.any()
    # nothing to do: 0, nothing written, no device needed
    assert dg_call(L, None, 0, None, None, 0, 4, 9, 16, 16, 7, None) == 0
    assert call(d=0) == 0 and call(d=0, first=1 << 55) == 0 and call(d=0, values=[None], outs=[None]) == 0
    assert not out.any()
    assert call(first=(1 << 55) - 4) == 0 and out.tobytes() == M.add_noise(x, SEED, 9, 16, 16, 7, (1 << 55) - 4).tobytes()      # first + d == 2^55 is allowed
    assert call(sigma2=1 << 24) == 0 and call(sigma2=1) == 0
    # the debug entries
    n32, u32 = ctypes.c_int32(7), ctypes.c_uint32(7)
    h = lambda seed=SEED, e=0, s2=9, o=ctypes.byref(n32), u=ctypes.byref(u32): L.rofl_dbg_host_dgauss(seed, ctypes.c_uint64(e), ctypes.c_uint32(s2), o, u)
    assert h(seed=None) == 11 and h(o=None) == 11 and h(s2=0) == 11 and h(s2=(1 << 24) + 1) == 11 and h(e=1 << 55) == 11
    assert n32.value == 7 and u32.value == 7
    assert h(u=None) == 0 and n32.value == M.element(SEED, 0, 9)[0]
    L.rofl_dbg_dgauss_words.argtypes = [ctypes.c_uint, sz, ctypes.c_void_p, sz] + [ctypes.c_void_p] * 5
    w, ln, s2s, a, b, c = (np.zeros(8, np.uint32), np.full(1, 8, np.uint32), np.ones(1, np.uint32), np.zeros(1, np.int32), np.zeros(1, np.uint32), np.zeros(1, np.uint32))
    p = lambda z: z.ctypes.data
    g = lambda site=0, n=1, words=p(w), stride=8, lens=p(ln), s=p(s2s), o1=p(a), o2=p(b), o3=p(c): L.rofl_dbg_dgauss_words(site, n, words, stride, lens, s, o1, o2, o3)
    assert g(site=2) == 11 and g(words=None) == 11 and g(lens=None) == 11 and g(s=None) == 11 and g(o1=None) == 11 and g(o2=None) == 11 and g(o3=None) == 11
    assert g(stride=7) == 11 and g(stride=8193) == 11 and g(n=(1 << 20) + 1) == 11
    s2s[0] = 0
    assert g() == 11
    s2s[0] = 1
    assert g(n=0, words=None, lens=None, s=None, o1=None, o2=None, o3=None) == 0 and g() == 0 and b[0] == 8 and c[0] == 0
    e, r = ctypes.c_uint32(0), ctypes.c_uint32(0)
    assert L.rofl_dbg_dgauss_geometry(sz(100), None, ctypes.byref(r)) == 11 and L.rofl_dbg_dgauss_geometry(sz(1 << 28), ctypes.byref(e), ctypes.byref(r)) == 11
    assert L.rofl_dbg_dgauss_geometry(sz(1), ctypes.byref(e), ctypes.byref(r)) == 0 and e.value == 1 and r.value >= 1


@pytest.mark.parametrize("s2", (1, 2, 9, 50))
def test_distribution_of_the_host_route(hiplib, s2):
    """N = 65 536 zeros, seed 00 01 .. 1f, fp (32, 7): the outputs are the noise itself.  Chi-square against the exact pmf of the
    discrete Gaussian within cells + 4 sqrt(2 cells) (the model's figures: 6.7 on 8 cells, 7.6 on 12, 28.2 on 22, 41.1 on 46), the mean
    within five standard errors; the first 2 048 elements equal the model's, and the chi-square equals the one the model gave for all of
    them (the golden file)"""
    N = 65536
    out = np.full(N, np.nan, np.float32)
    assert dg_call(hiplib, 0, 1, SEED, [np.zeros(N, np.float32)], 0, N, s2, 32, 32, 7, [out]) == 0
    got = out.astype(np.float64) * 128
    assert (got == np.round(got)).all() and (got[:2048] == M.noise(SEED, 0, 2048, s2)).all()
    chi2, cells = M.chi2(got, s2)      # (values whose expected count is at least 20 are single cells, the rest one pooled cell)
    print("sigma2 %d: chi2 %.2f on %d cells, mean %.4f" % (s2, chi2, cells, got.mean()))
    assert cells == {1: 8, 2: 12, 9: 22, 50: 46}[s2]
    assert chi2 <= cells + 4 * math.sqrt(2 * cells), (s2, chi2, cells)
    assert abs(chi2 - GOLDEN["chi2"][str(s2)]) < 0.05, (chi2, GOLDEN["chi2"][str(s2)])
    assert abs(got.mean()) <= 5 * math.sqrt(s2 / N), (s2, got.mean())


def test_closure_under_addition(hiplib):
    """the sum over eight seeds SHA3-256(byte k) at sigma2 = 9 over 8 192 elements: variance within 5 standard errors of 72 (the model:
    71.44, s.e. 1.13)"""
    s2, d = 9, 8192
    seeds = [hashlib.sha3_256(bytes([k])).digest() for k in range(8)]
    outs = [np.zeros(d, np.float32) for _ in seeds]
    assert dg_call(hiplib, 0, 8, b"".join(seeds), [np.zeros(d, np.float32)] * 8, 0, d, s2, 32, 32, 7, outs) == 0
    total = np.sum([o.astype(np.float64) * 128 for o in outs], axis=0)
    for c in (0, 7):
        assert (outs[c][:256].astype(np.float64) * 128 == M.noise(seeds[c], 0, 256, s2)).all()
    var = ((total - total.mean()) ** 2).mean()
    se = 72 * math.sqrt(2 / d)
    print("variance of the sum %.2f (72 +- %.2f)" % (var, se))
    assert abs(var - 72) <= 5 * se and abs(var - GOLDEN["closure_variance"]) < 0.01 and len({o.tobytes() for o in outs}) == 8
    assert abs(total.mean()) <= 5 * math.sqrt(72 / d)


def test_python_helpers(hiplib):
    import rofl_project_code_amd as R
    from rofl_project_code_amd.api import range_proof_vec as rp, pedersen_ops, DiscreteGaussian
    x = np.full(4, 0.3, np.float32)
    for bad in (lambda: rp.add_dgauss_noise(x, 16, SEED[:31], 9), lambda: rp.add_dgauss_noise_vecs([x, x], 16, [SEED], 9),
                lambda: rp.add_dgauss_noise_vecs([x, x[:3]], 16, [SEED, SEED], 9), lambda: rp.add_dgauss_noise(x, 16, SEED, 9, first=-1),
                lambda: rp.add_dgauss_noise(x, 0, SEED, 9), lambda: rp.add_dgauss_noise(x, 16, SEED, 0), lambda: rp.add_dgauss_noise(x, 16, SEED, 2.5),
                lambda: rp.add_dgauss_noise(x, 16, SEED, (1 << 24) + 1), lambda: rp.add_dgauss_noise_vecs([x], 16, [SEED], 9, out=[np.zeros(3, np.float32)]),
                lambda: DiscreteGaussian(0), lambda: DiscreteGaussian(1.5), lambda: DiscreteGaussian((1 << 24) + 1)):
        with pytest.raises(ValueError):
            bad()
    assert rp.add_dgauss_noise_vecs([], 16, [], 9).shape == (0, 0)
    got = rp.add_dgauss_noise(x, 16, SEED, 50, first=7, fp=(16, 7))
    assert got.dtype == np.float32 and got.tobytes() == M.add_noise(x, SEED, 50, 16, 16, 7, 7).tobytes()
    both = rp.add_dgauss_noise_vecs([x, -x], 8, [SEED, SEED[::-1]], 2, fp=(8, 7))
    assert both[0].tobytes() == M.add_noise(x, SEED, 2, 8, 8, 7).tobytes() and both[1].tobytes() == M.add_noise(-x, SEED[::-1], 2, 8, 8, 7).tobytes()
    y = x.copy()
    assert rp.add_dgauss_noise_vecs([y], 16, [SEED], 9, fp=(16, 7), out=[y])[0] is y and y.tobytes() == M.add_noise(x, SEED, 9, 16, 16, 7).tobytes()
    for sigma in (0, 0.5, 1, 1.0001, 2, 2.8284, 3, 64, 100.5, 4096, Fraction(7, 2)):
        assert rp.dgauss_sigma2(sigma) == M.smallest_sigma2(sigma), sigma
    assert rp.dgauss_sigma2(64) == 4096 and rp.dgauss_sigma2(0) == 1 and rp.dgauss_sigma2(4096) == 1 << 24 and rp.dgauss_sigma2(Fraction(7, 2)) == 13
    for bad in (4096.001, -1):
        with pytest.raises(ValueError):
            rp.dgauss_sigma2(bad)
    g = DiscreteGaussian(9)
    assert g.sigma2 == 9 and g == DiscreteGaussian(9) and g != DiscreteGaussian(10) and g != 9 and hash(g) == hash(DiscreteGaussian(9)) and "9" in repr(g)
    assert R.DiscreteGaussian is DiscreteGaussian and rp.add_dgauss_noise(x, 16, SEED, g, fp=(16, 7)).tobytes() == y.tobytes()
    with pytest.raises(AttributeError):
        g.sigma2 = 10
    with pytest.raises(AttributeError):
        g.other = 1
    # one round seed serves both mechanisms: the streams differ by their labels
    s = pedersen_ops.noise_round_seed(b"client secret", 3)
    assert rp.add_dgauss_noise(np.zeros(64, np.float32), 16, s, 8, fp=(16, 7)).tobytes() != rp.add_binomial_noise(np.zeros(64, np.float32), 16, s, 16, fp=(16, 7)).tobytes()
    assert "secret" in rp.add_dgauss_noise_vecs.__doc__.lower() and "not constant time" in rp.add_dgauss_noise_vecs.__doc__.lower()


def test_containers_take_a_discrete_gaussian_noise_k(hiplib, monkeypatch):
    """encrypt(noise_seed=, noise_k=DiscreteGaussian(..)) and encrypt_batch_private hand every leg the model's noised values -- after the
    rounding of a quant seed where there is one; ONE dgauss call per batch and no binomial call; an int noise_k still takes the binomial
    call.  The legs are replaced by recorders: nothing here reaches a device."""
    import pq_model
    from rofl_project_code_amd import api, params
    from rofl_project_code_amd.api import DiscreteGaussian
    seen = {}

    class Stop(Exception):
        pass

    def commitments(clipped, bl, prove_range, fp):
        seen["clipped"] = np.array(clipped, np.float32)
        raise Stop()
    monkeypatch.setattr(params, "_range_commitments", commitments)
    x = np.array([0.3, -0.3, 300.0, 1 / 512, -0.0], np.float32)
    bl, r2 = np.zeros((5, 32), np.uint8), np.zeros((5, 32), np.uint8)
    QS, NS, G = SEED[::-1], SEED, DiscreteGaussian(9)
    rounded = pq_model.quantize(x, QS, 16, 16, 7)
    noised = M.add_noise(x, NS, 9, 16, 16, 7)
    both = M.add_noise(rounded, NS, 9, 16, 16, 7)
    binom = NM.add_noise(x, NS, 48, 16, 16, 7)
    assert len({rounded.tobytes(), noised.tobytes(), both.tobytes(), binom.tobytes()}) == 4
    cases = [(params.EncParamsRange, (2, 1.0), {}), (params.EncParamsRangeCompressed, (2, 1.0), {}), (params.EncParamsL2, (2, 32), dict(rand_scalars=r2)),
             (params.EncParamsL2Compressed, (2, 32), dict(rand_scalars=r2)), (params.EncParamsL2CompressedStrict, (2, 32), dict(rand_scalars=r2))]
    calls = []
    real_g, real_b = api.range_proof_vec.add_dgauss_noise_vecs, api.range_proof_vec.add_binomial_noise_vecs
    monkeypatch.setattr(api.range_proof_vec, "add_dgauss_noise_vecs", staticmethod(lambda *a, **k: (calls.append(("g", len(a[0]))), real_g(*a, **k))[1]))
    monkeypatch.setattr(api.range_proof_vec, "add_binomial_noise_vecs", staticmethod(lambda *a, **k: (calls.append(("b", len(a[0]))), real_b(*a, **k))[1]))
    for cls, tail, kw in cases:
        assert list(inspect.signature(cls.encrypt_batch_private).parameters)[4:] == ["nonce_seeds", "fp", "quant_seeds", "noise_seeds", "noise_k"]
        one = [(x, bl) + tuple(kw.values())]
        runs = [(noised, lambda: cls.encrypt(x, bl, 16, *tail, fp=(16, 7), noise_seed=NS, noise_k=G, **kw)),
                (both, lambda: cls.encrypt(x, bl, 16, *tail, fp=(16, 7), quant_seed=QS, noise_seed=NS, noise_k=G, **kw)),
                (noised, lambda: cls.encrypt_batch_private(one, 16, *tail, fp=(16, 7), noise_seeds=[NS], noise_k=G)),
                (both, lambda: cls.encrypt_batch_private(one, 16, *tail, fp=(16, 7), quant_seeds=[QS], noise_seeds=[NS], noise_k=G)),
                (rounded, lambda: cls.encrypt_batch_private(one, 16, *tail, fp=(16, 7), quant_seeds=[QS], noise_seeds=[None], noise_k=G)),
                (binom, lambda: cls.encrypt(x, bl, 16, *tail, fp=(16, 7), noise_seed=NS, noise_k=48, **kw))]
        if hasattr(cls, "encrypt_batch_clipped"):
            runs.append((noised, lambda: cls.encrypt_batch_clipped(one, 16, *tail, fp=(16, 7), noise_seeds=[NS], noise_k=G)))
        for want, run in runs:
            seen.clear()
            del calls[:]
            with pytest.raises(Stop):
                run()
            assert seen["clipped"].tobytes() == want.tobytes(), cls
            assert [c[0] for c in calls] == ([] if want is rounded else ["b"] if want is binom else ["g"]), (cls, calls)
        del calls[:]
        with pytest.raises(Stop):
            cls.encrypt_batch_private(one * 3, 16, *tail, fp=(16, 7), noise_seeds=[NS, None, NS], noise_k=G)
        assert calls == [("g", 2)], "ONE noise call for all hosted clients that have a seed"
        for bad in (dict(noise_k=G), dict(noise_seeds=[NS, NS], noise_k=G)):
            with pytest.raises(ValueError):
                cls.encrypt_batch_private(one, 16, *tail, fp=(16, 7), **bad)
        with pytest.raises(ValueError):
            cls.encrypt(x, bl, 16, *tail, fp=(16, 7), **dict(kw, noise_k=G))


def test_entry_points_are_exported_and_declared_for_rust(hiplib):
    for name in ("rofl_noise_dgauss", "rofl_dbg_host_dgauss", "rofl_dbg_dgauss_words", "rofl_dbg_noise_dgauss_route", "rofl_dbg_dgauss_geometry"):
        assert hasattr(hiplib, name), name
    hdr = open(os.path.join(ROOT, "include", "rofl_zk.h")).read()
    assert "int rofl_noise_dgauss(" in hdr and "rofl-zk/dgaus/v1" in hdr and "NOT constant time" in hdr
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "check_ffi.py")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    ffi = open(os.path.join(ROOT, "integration", "rofl_crypto_overlay", "src", "ffi.rs")).read()
    assert "pub fn rofl_noise_dgauss(" in ffi
    overlay = open(os.path.join(ROOT, "integration", "rofl_crypto_overlay", "src", "range_proof_vec", "mod.rs")).read()
    assert "pub fn add_dgauss_noise(" in overlay and "rofl_noise_dgauss(" in overlay
    assert "add_dgauss_noise" in open(os.path.join(ROOT, "INTEGRATION.md")).read() and "add_dgauss_noise" in open(os.path.join(ROOT, "README.md")).read()
