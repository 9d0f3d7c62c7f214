"""CPU-only checks of the seeded blinding vectors (rofl_blinding_vecs / rofl_rnd_scalar_vec): the host-compiled stream against the Python
model, every parameter check of the C entry points (they come before the device is touched), the Python wrappers' own checks, the seed
derivations, and the Rust declarations.  No call here reaches a GPU."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import blind_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sz = ctypes.c_size_t
SEED = bytes(range(32))


class Term(ctypes.Structure):
    _fields_ = [("seed", ctypes.c_ubyte * 32), ("sign", ctypes.c_int32)]


def _call(L, n_vec, counts, term_arrays, first, d, outs):
    """rofl_blinding_vecs with the given raw arguments (None = a null pointer)"""
    L.rofl_blinding_vecs.argtypes = [sz, ctypes.c_void_p, ctypes.c_void_p, sz, sz, ctypes.c_void_p]
    c = (sz * len(counts))(*counts) if counts is not None else None
    t = (ctypes.c_void_p * len(term_arrays))(*[ctypes.addressof(a) if a is not None else None for a in term_arrays]) if term_arrays is not None else None
    o = (ctypes.c_void_p * len(outs))(*[x.ctypes.data if x is not None else None for x in outs]) if outs is not None else None
    return L.rofl_blinding_vecs(n_vec, c, t, first, d, o)


def _terms(signs):
    a = (Term * max(len(signs), 1))()
    for i, s in enumerate(signs):
        ctypes.memmove(a[i].seed, SEED, 32)
        a[i].sign = s
    return a


def test_host_stream_equals_the_model(hiplib):
    for idx in (0, 1, 77, 2 ** 40 + 5):
        out = ctypes.create_string_buffer(32)
        assert hiplib.rofl_dbg_host_blind(SEED, ctypes.c_uint64(idx), out) == 0
        assert out.raw == M.stream_int(SEED, idx).to_bytes(32, "little"), idx
        nonce = ctypes.create_string_buffer(32)
        assert hiplib.rofl_dbg_host_nonce(SEED, ctypes.c_uint64(idx), nonce) == 0
        assert nonce.raw != out.raw, "the nonce stream and the blinding stream of a seed coincide"


def test_parameter_checks_come_before_the_device(hiplib):
    L = hiplib
    out = np.zeros((4, 32), dtype=np.uint8)
    one = _terms([1])
    assert _call(L, 1, None, [one], 0, 4, [out]) == 11            # null arrays with n_vec > 0
    assert _call(L, 1, [1], None, 0, 4, [out]) == 11
    assert _call(L, 1, [1], [one], 0, 4, None) == 11
    assert _call(L, 1, [1], [None], 0, 4, [out]) == 11            # null terms[v] with term_count[v] > 0
    assert _call(L, 1, [1], [one], 0, 4, [None]) == 11            # null out32[v] with d > 0
    for bad in (0, 2, -2, 1 << 30):
        assert _call(L, 1, [1], [_terms([bad])], 0, 4, [out]) == 11, bad
    assert _call(L, 2, [1, 2], [one, _terms([1, 3])], 0, 4, [out, out]) == 11
    n = 65536                                                     # gridDim.y
    assert _call(L, n, [0] * n, [None] * n, 0, 4, [out] * n) == 11
    assert _call(L, 1, [1], [one], 0, 1 << 28, [out]) == 11       # d >= 2^28
    assert _call(L, 1, [1], [one], (1 << 63) - 3, 4, [out]) == 11  # first + d beyond 2^63
    assert _call(L, 1, [1], [one], (1 << 64) - 2, 4, [out]) == 11
    big = (1 << 22) + 1                                           # more than 2^22 terms in total (the count alone decides: nothing is read past it)
    assert _call(L, 1, [big], [one], 0, 4, [out]) == 11
    half = np.zeros((1 << 21) + 1, dtype=np.dtype([("seed", np.uint8, 32), ("sign", "<i4")]))      # the layout of rofl_blind_term_t
    half["sign"] = 1
    assert half.dtype.itemsize == ctypes.sizeof(Term)
    half_c = (Term * half.size).from_buffer(half)
    assert _call(L, 2, [half.size] * 2, [half_c, half_c], 0, 4, [out, out]) == 11
    err = ctypes.create_string_buffer(512)
    L.rofl_last_error(err, sz(512))
    assert SEED.hex() not in err.value.decode() and SEED not in err.raw
    # nothing to do: 0, nothing written, no device needed
    assert _call(L, 0, None, None, 0, 4, None) == 0
    assert _call(L, 1, [1], [one], 5, 0, [out]) == 0
    assert not out.any()
    # the single-vector entry point goes through the same checks
    L.rofl_rnd_scalar_vec.argtypes = [ctypes.c_void_p, sz, sz, ctypes.c_void_p]
    assert L.rofl_rnd_scalar_vec(None, 0, 4, out.ctypes.data) == 11
    assert L.rofl_rnd_scalar_vec(SEED, 0, 4, None) == 11
    assert L.rofl_rnd_scalar_vec(SEED, 0, 1 << 28, out.ctypes.data) == 11
    assert L.rofl_rnd_scalar_vec(SEED, 0, 0, None) == 0


def test_wrappers_raise_for_a_bad_sign_or_a_self_peer(hiplib):
    from rofl_project_code_amd.api import pedersen_ops
    with pytest.raises(ValueError):
        pedersen_ops.blinding_vecs([[(SEED, 0)]], 4)
    with pytest.raises(ValueError):
        pedersen_ops.blinding_vecs([[(SEED, 1), (SEED, 2)]], 4)
    with pytest.raises(ValueError):
        pedersen_ops.blinding_vecs([[(SEED[:31], 1)]], 4)
    with pytest.raises(ValueError):
        pedersen_ops.pairwise_blinding_vec(2, [(1, SEED), (2, SEED)], 4)
    with pytest.raises(ValueError):
        pedersen_ops.pairwise_blinding_vecs([(0, [(1, SEED)]), (1, [(1, SEED)])], 4)
    # nothing to compute never reaches the device
    assert pedersen_ops.blinding_vecs([], 4).shape == (0, 4, 32)
    assert pedersen_ops.rnd_scalar_vec_seeded(0, SEED).shape == (0, 32)


def test_containers_refuse_scalars_and_a_seed_for_one_client(hiplib):
    from rofl_project_code_amd import params
    x, bl, r2 = np.zeros(2, np.float32), np.zeros((2, 32), np.uint8), np.zeros((2, 32), np.uint8)
    for cls in (params.EncParamsL2, params.EncParamsL2Compressed):
        with pytest.raises(ValueError):
            cls.encrypt(x, bl, 8, 1, 16, rand_scalars=r2, rand_seed=SEED)


def test_seed_derivations_equal_hashlib(hiplib):
    from rofl_project_code_amd.api import pedersen_ops
    for i in (0, 1, 46, 2 ** 31):
        assert pedersen_ops.cancelling_vec_seed(SEED, i) == M.vec_seed(SEED, i)
    for r in (0, 7, 2 ** 40):
        assert pedersen_ops.pairwise_round_seed(b"shared secret", r) == M.round_seed(b"shared secret", r)
    assert "ONE round" in pedersen_ops.pairwise_round_seed.__doc__


def test_new_entry_points_are_exported_and_declared_for_rust(hiplib):
    for name in ("rofl_blinding_vecs", "rofl_rnd_scalar_vec", "rofl_dbg_host_blind"):
        assert hasattr(hiplib, name), name
    hdr = open(os.path.join(ROOT, "include", "rofl_zk.h")).read()
    assert "rofl_blinding_vecs(" in hdr and "rofl_rnd_scalar_vec(" in hdr and "rofl_blind_term_t" in hdr
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "check_ffi.py")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    ffi = open(os.path.join(ROOT, "integration", "rofl_crypto_overlay", "src", "ffi.rs")).read()
    assert "pub fn rofl_blinding_vecs(" in ffi and "pub fn rofl_rnd_scalar_vec(" in ffi and "pub struct RoflBlindTerm" in ffi
