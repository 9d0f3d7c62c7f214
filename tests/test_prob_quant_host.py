"""CPU-only checks of the probabilistic quantization (rofl_quantize_prob): the host-compiled stream and rounding rule against the Python
model (tests/pq_model.py) on the edge-case corpus of all 47 formats, every parameter check of the C entry point (they come before the
device is touched), the Python wrappers' own checks, the untouched path without a seed, the statistics of the definition, and the Rust
declaration.  No call here reaches a GPU: the library's host route is compiled from the kernel's source."""
import ctypes
import hashlib
import inspect
import math
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

import blind_model as BM
import pq_model as M
import quant_model as Q

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sz = ctypes.c_size_t
SEED = bytes(range(32))


def _round(L, site, vals_bits, words, nb, fb, ff):
    """rofl_dbg_quant_round -> output bits"""
    v = np.ascontiguousarray(vals_bits, np.uint32)
    w = np.ascontiguousarray(words, np.uint32)
    out = np.full(v.size, 0x7fc00001, np.uint32)
    L.rofl_dbg_quant_round.argtypes = [ctypes.c_uint, sz, ctypes.c_void_p, ctypes.c_void_p, sz, ctypes.c_uint, ctypes.c_uint, ctypes.c_void_p]
    assert L.rofl_dbg_quant_round(site, v.size, v.ctypes.data, w.ctypes.data, nb, fb, ff, out.ctypes.data) == 0
    return out


def _call(L, n_vec, seeds, values, first, d, nb, fb, ff, outs):
    """rofl_quantize_prob with the given raw arguments (None = a null pointer)"""
    L.rofl_quantize_prob.argtypes = [sz, ctypes.c_void_p, ctypes.c_void_p, sz, sz, sz, ctypes.c_uint, ctypes.c_uint, ctypes.c_void_p]
    arr = lambda xs: (ctypes.c_void_p * len(xs))(*[x.ctypes.data if x is not None else None for x in xs]) if xs is not None else None
    return L.rofl_quantize_prob(n_vec, seeds, arr(values), first, d, nb, fb, ff, arr(outs))


def test_host_stream_equals_the_model_and_has_a_label_of_its_own(hiplib):
    for idx in (0, 1, 31, 32, 2 ** 40 + 5):
        w = ctypes.c_uint32(0)
        assert hiplib.rofl_dbg_host_quant(SEED, ctypes.c_uint64(idx), ctypes.byref(w)) == 0
        assert w.value == M.word(SEED, idx), idx
    # the nonce, blinding and share streams of the same seed are other XOF outputs: the labels differ
    q = M.block(SEED, 0)
    w = ctypes.c_uint32(0)
    assert hiplib.rofl_dbg_host_quant(SEED, ctypes.c_uint64(0), ctypes.byref(w)) == 0
    for label in (b"rofl-zk/nonce/v2", b"rofl-zk/blind/v1", b"rofl-zk/share/v1"):
        other = hashlib.shake_256(label + SEED + struct.pack("<Q", 0)).digest(128)
        assert len(label) == len(M.LABEL) and other != q and struct.unpack_from("<I", other)[0] != w.value, label
    assert BM.stream_int(SEED, 0) == int.from_bytes(hashlib.shake_256(b"rofl-zk/blind/v1" + SEED + struct.pack("<Q", 0)).digest(64), "little") % BM.L


@pytest.mark.parametrize("fb", (8, 16, 32, 64))
def test_host_rule_equals_the_model_on_the_corpus(hiplib, fb):
    n = 0
    for (b, ff) in Q.VALID_FP:
        if b != fb:
            continue
        for nb in sorted({min(8, fb), fb}):
            vb, ws = M.corpus(fb, ff, nb)
            got, want = _round(hiplib, 0, vb, ws, nb, fb, ff), M.corpus_expected(fb, ff, nb)
            bad = np.nonzero(got != want)[0]
            assert bad.size == 0, (fb, ff, nb, [(hex(vb[i]), hex(ws[i]), hex(got[i]), hex(want[i])) for i in bad[:5]])
            n += vb.size
    assert n > 1000


def test_step_one_is_rofl_clip_f32(hiplib):
    """c of step 1 is exactly what rofl_clip_f32 returns: on the grid values of the corpus (returned unchanged) the two calls agree bit for bit,
    NaN, the infinities and -0.0 included"""
    for fb, ff, nb in ((16, 7, 16), (8, 7, 8), (32, 12, 8), (64, 12, 64), (16, 0, 9)):
        vb, ws = M.corpus(fb, ff, nb)
        clipped = np.empty(vb.size, np.uint32)
        hiplib.rofl_clip_f32.argtypes = [ctypes.c_void_p, sz, sz, ctypes.c_uint, ctypes.c_uint, ctypes.c_void_p]
        assert hiplib.rofl_clip_f32(vb.ctypes.data, vb.size, nb, fb, ff, clipped.ctypes.data) == 0
        assert [M.clip(int(b), nb, fb, ff) for b in vb] == [int(c) for c in clipped]
        got = _round(hiplib, 0, vb, ws, nb, fb, ff)
        on_grid = np.array([M.threshold(int(b), nb, fb, ff)[2] == 0 and Q.value(int(c)) * (1 << ff) % 1 == 0 for b, c in zip(vb, clipped)])
        assert on_grid.sum() > 50 and (got[on_grid] == clipped[on_grid]).all()


def test_entry_point_host_route_equals_the_model(hiplib):
    """all pointers in host memory and a small size: the library runs the rule on the host (no GPU here), from the kernel's source"""
    rng = np.random.default_rng(5)
    for (fb, ff, nb), d, first in (((16, 7, 16), 33, 0), ((8, 7, 8), 1, 31), ((32, 7, 32), 257, 2 ** 40 + 5), ((64, 12, 64), 31, 1), ((16, 12, 8), 32, 0)):
        seeds = [bytes([v + 1]) * 32 for v in range(3)]
        vals = [rng.uniform(-3, 3, d).astype(np.float32) for _ in range(3)]
        outs = [np.zeros(d, np.float32) for _ in range(3)]
        assert _call(hiplib, 3, b"".join(seeds), vals, first, d, nb, fb, ff, outs) == 0
        for v in range(3):
            assert outs[v].tobytes() == M.quantize(vals[v], seeds[v], nb, fb, ff, first).tobytes(), (fb, ff, d, first, v)
        # runs taken with `first` concatenate to the unsplit bytes; in place gives the same
        if d > 2:
            a, b = np.zeros(d // 3, np.float32), np.zeros(d - d // 3, np.float32)
            assert _call(hiplib, 1, seeds[0], [vals[0][:d // 3]], first, d // 3, nb, fb, ff, [a]) == 0
            assert _call(hiplib, 1, seeds[0], [vals[0][d // 3:]], first + d // 3, d - d // 3, nb, fb, ff, [b]) == 0
            assert np.concatenate([a, b]).tobytes() == outs[0].tobytes()
        x = vals[1].copy()
        assert _call(hiplib, 1, seeds[1], [x], first, d, nb, fb, ff, [x]) == 0 and x.tobytes() == outs[1].tobytes()


def test_parameter_checks_come_before_the_device(hiplib):
    L = hiplib
    x, out = np.full(4, 0.3, np.float32), np.zeros(4, np.float32)
    ok = dict(n_vec=1, seeds=SEED, values=[x], first=0, d=4, nb=16, fb=16, ff=7, outs=[out])
    call = lambda **kw: _call(L, **dict(ok, **kw))
    assert call(seeds=None) == 11 and call(values=None) == 11 and call(outs=None) == 11      # null arrays with n_vec > 0
    assert call(values=[None]) == 11 and call(outs=[None]) == 11                                # null entries with d > 0
    assert call(n_vec=2, seeds=SEED * 2, values=[x, None], outs=[out, out]) == 11
    for fb, ff in ((12, 7), (16, 13), (8, 8), (0, 0)):
        assert call(fb=fb, ff=ff) == 11, (fb, ff)
    assert call(nb=0) == 11
    n = 65536                                                                                   # gridDim.y
    assert call(n_vec=n, seeds=SEED * n, values=[x] * n, outs=[out] * n) == 11
    assert call(d=1 << 28) == 11
    assert call(first=(1 << 63) - 3) == 11 and call(first=(1 << 64) - 2) == 11
    assert not out.any()
    err = ctypes.create_string_buffer(512)
    L.rofl_last_error(err, sz(512))
    assert SEED.hex() not in err.value.decode() and SEED not in err.raw
    # nothing to do: 0, nothing written, no device needed
    assert _call(L, 0, None, None, 0, 4, 16, 16, 7, None) == 0
    assert call(d=0) == 0 and call(d=0, first=(1 << 63)) == 0 and call(d=0, values=[None], outs=[None]) == 0
    assert not out.any()
    assert call(first=(1 << 63) - 4) == 0 and out.tobytes() == M.quantize(x, SEED, 16, 16, 7, (1 << 63) - 4).tobytes()      # first + d == 2^63 is allowed
    # the debug entries
    w = ctypes.c_uint32()
    assert L.rofl_dbg_host_quant(None, ctypes.c_uint64(0), ctypes.byref(w)) == 11 and L.rofl_dbg_host_quant(SEED, ctypes.c_uint64(0), None) == 11
    L.rofl_dbg_quant_round.argtypes = [ctypes.c_uint, sz, ctypes.c_void_p, ctypes.c_void_p, sz, ctypes.c_uint, ctypes.c_uint, ctypes.c_void_p]
    ws = np.zeros(4, np.uint32)
    r = lambda site=0, n=4, v=x.ctypes.data, w_=ws.ctypes.data, nb=16, fb=16, ff=7, o=out.ctypes.data: L.rofl_dbg_quant_round(site, n, v, w_, nb, fb, ff, o)
    assert r(site=2) == 11 and r(v=None) == 11 and r(w_=None) == 11 and r(o=None) == 11 and r(nb=0) == 11 and r(fb=12) == 11 and r(n=(1 << 20) + 1) == 11
    assert r(n=0, v=None, w_=None, o=None) == 0


def test_wrappers_make_their_own_checks(hiplib):
    from rofl_project_code_amd.api import range_proof_vec as rp, pedersen_ops
    x = np.full(4, 0.3, np.float32)
    with pytest.raises(ValueError):
        rp.quantize_probabilistic(x, 16, SEED[:31])
    with pytest.raises(ValueError):
        rp.quantize_probabilistic_vecs([x, x], 16, [SEED])
    with pytest.raises(ValueError):
        rp.quantize_probabilistic_vecs([x, x[:3]], 16, [SEED, SEED])
    with pytest.raises(ValueError):
        rp.quantize_probabilistic(x, 16, SEED, first=-1)
    with pytest.raises(ValueError):
        rp.quantize_probabilistic(x, 0, SEED)
    with pytest.raises(ValueError):
        rp.quantize_probabilistic_vecs([x], 16, [SEED], out=[np.zeros(4, np.float64)])
    with pytest.raises(ValueError):
        rp.quantize_probabilistic_vecs([x], 16, [SEED], out=[np.zeros(3, np.float32)])
    with pytest.raises(ValueError):
        rp.quantize_probabilistic_vecs([x], 16, [SEED], out=[])
    # nothing to compute never reaches the device; small host calls run on the host
    assert rp.quantize_probabilistic_vecs([], 16, []).shape == (0, 0)
    assert rp.quantize_probabilistic(np.zeros(0, np.float32), 16, SEED).shape == (0,)
    got = rp.quantize_probabilistic(x, 16, SEED, first=7, fp=(16, 7))
    assert got.dtype == np.float32 and got.tobytes() == M.quantize(x, SEED, 16, 16, 7, 7).tobytes()
    both = rp.quantize_probabilistic_vecs([x, -x], 8, [SEED, SEED[::-1]], fp=(8, 7))
    assert both[0].tobytes() == M.quantize(x, SEED, 8, 8, 7).tobytes() and both[1].tobytes() == M.quantize(-x, SEED[::-1], 8, 8, 7).tobytes()
    y = x.copy()
    assert rp.quantize_probabilistic_vecs([y], 16, [SEED], fp=(16, 7), out=[y])[0] is y and y.tobytes() == M.quantize(x, SEED, 16, 16, 7).tobytes()
    for r in (0, 7, 2 ** 40):
        assert pedersen_ops.quant_round_seed(b"client secret", r) == M.round_seed(b"client secret", r)
    assert "secret" in pedersen_ops.quant_round_seed.__doc__.lower() and "secret" in rp.quantize_probabilistic_vecs.__doc__.lower()


def test_without_a_seed_the_containers_clip_as_before(hiplib, monkeypatch):
    """encrypt(quant_seed=None) and encrypt_batch hand the legs what clip_f32_to_range_vec returns and never call the quantizer; with a seed
    the quantizer's output is the plaintext of every leg.  The legs are replaced by recorders: nothing here reaches a device."""
    from rofl_project_code_amd import api, params
    seen = {}

    class Stop(Exception):
        pass

    def commitments(clipped, bl, prove_range, fp):
        seen["clipped"] = np.array(clipped, np.float32)
        raise Stop()

    def no_quant(*a, **k):
        raise AssertionError("the quantizer was called without a seed")
    monkeypatch.setattr(params, "_range_commitments", commitments)
    x = np.array([0.3, -0.3, 300.0, 1 / 512, -0.0], np.float32)
    bl, r2 = np.zeros((5, 32), np.uint8), np.zeros((5, 32), np.uint8)
    clip = api.range_proof_vec.clip_f32_to_range_vec(x, 16, fp=(16, 7))
    quant = M.quantize(x, SEED, 16, 16, 7)
    assert quant.tobytes() != clip.tobytes()
    cases = [(params.EncParamsRange, (2, 1.0), {}), (params.EncParamsRangeCompressed, (2, 1.0), {}), (params.EncParamsL2, (2, 32), dict(rand_scalars=r2)),
             (params.EncParamsL2Compressed, (2, 32), dict(rand_scalars=r2)), (params.EncParamsL2CompressedStrict, (2, 32), dict(rand_scalars=r2))]
    for cls, tail, kw in cases:
        assert inspect.signature(cls.encrypt).parameters["quant_seed"].default is None, cls
        with monkeypatch.context() as m:
            m.setattr(api.range_proof_vec, "quantize_probabilistic_vecs", no_quant)
            m.setattr(api.range_proof_vec, "quantize_probabilistic", no_quant)
            for run in (lambda: cls.encrypt(x, bl, 16, *tail, fp=(16, 7), **kw),
                        lambda: cls.encrypt(x, bl, 16, *tail, fp=(16, 7), quant_seed=None, **kw),
                        lambda: cls.encrypt_batch([(x, bl) + tuple(kw.values())], 16, *tail, fp=(16, 7)),
                        lambda: cls.encrypt_batch_quantized([(x, bl) + tuple(kw.values())], 16, *tail, [None], fp=(16, 7))):
                seen.clear()
                with pytest.raises(Stop):
                    run()
                assert seen["clipped"].tobytes() == clip.tobytes(), cls
        for run in (lambda: cls.encrypt(x, bl, 16, *tail, fp=(16, 7), quant_seed=SEED, **kw),
                    lambda: cls.encrypt_batch_quantized([(x, bl) + tuple(kw.values())], 16, *tail, [SEED], fp=(16, 7))):
            seen.clear()
            with pytest.raises(Stop):
                run()
            assert seen["clipped"].tobytes() == quant.tobytes(), cls
        with pytest.raises(ValueError):
            cls.encrypt_batch_quantized([(x, bl) + tuple(kw.values())], 16, *tail, [SEED, SEED], fp=(16, 7))
        assert list(inspect.signature(cls.encrypt_batch_quantized).parameters)[4:] == ["quant_seeds", "nonce_seeds", "fp"]
        assert cls.encrypt_batch_quantized([], 16, *tail, []) == []


def test_statistics_of_the_definition():
    """the model alone, seed 00 01 .. 1f, fp (16, 7), elements 0 .. 4095 of the stream: the exact number of round-ups, and that it is within
    four standard deviations of N t / 2^32"""
    N = 4096
    ws = M.words(SEED, 0, N)
    for v, ups_want, expected in ((np.float32(0.3), 1643, 1638.4), (np.float32(1 / 512), 1021, 1024), (np.float32(100.004), 2136, 2096)):
        _, f, t = M.threshold(v, 16, 16, 7)
        p = t / 2 ** 32
        assert abs(N * p - expected) < 0.51, (v, N * p)
        ups = sum(w < t for w in ws)
        assert ups == ups_want, (v, ups)
        assert abs(ups - N * p) <= 4 * math.sqrt(N * p * (1 - p)), (v, ups, N * p)
        out = M.quantize(np.full(N, v, np.float32), SEED, 16, 16, 7)
        assert int(round(float(out.astype(np.float64).sum()) * 128)) == N * f + ups


def test_entry_points_are_exported_and_declared_for_rust(hiplib):
    for name in ("rofl_quantize_prob", "rofl_dbg_host_quant", "rofl_dbg_quant_round"):
        assert hasattr(hiplib, name), name
    hdr = open(os.path.join(ROOT, "include", "rofl_zk.h")).read()
    assert "int rofl_quantize_prob(" in hdr and "rofl-zk/quant/v1" in hdr
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "check_ffi.py")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    ffi = open(os.path.join(ROOT, "integration", "rofl_crypto_overlay", "src", "ffi.rs")).read()
    assert "pub fn rofl_quantize_prob(" in ffi
    overlay = open(os.path.join(ROOT, "integration", "rofl_crypto_overlay", "src", "range_proof_vec", "mod.rs")).read()
    assert "pub fn quantize_probabilistic(" in overlay and "rofl_quantize_prob(" in overlay
    assert "quantize_probabilistic" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
