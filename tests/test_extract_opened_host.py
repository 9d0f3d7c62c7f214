"""CPU-only checks of the extraction after rejections (rofl_acc_extract_opened / rofl_acc_extract_opened_terms): every parameter check of
the two C entry points (they come before the device is touched), the declarations, and the helpers that list the terms of the accepted set's
residual blinding, against the Python model of the blinding streams (blind_model.combine).  No call here reaches a GPU."""
import ctypes
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest

import blind_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sz, u64 = ctypes.c_size_t, ctypes.c_uint64
SEED = bytes(range(100, 132))


class Term(ctypes.Structure):
    _fields_ = [("seed", ctypes.c_ubyte * 32), ("sign", ctypes.c_int32)]


def _terms(signs):
    a = (Term * max(len(signs), 1))()
    for i, s in enumerate(signs):
        ctypes.memmove(a[i].seed, SEED, 32)
        a[i].sign = s
    return a


def _sum_mod_l(vecs, d):
    return M.to_arr([sum(col) for col in zip(*[M.to_ints(v) for v in vecs])] if vecs else [0] * d)


def test_parameter_checks_come_before_the_device(hiplib):
    L = hiplib
    vp = ctypes.c_void_p
    L.rofl_acc_extract_opened.argtypes = [u64, vp, sz, ctypes.c_uint, ctypes.c_uint, ctypes.c_uint, vp, vp, vp]
    L.rofl_acc_extract_opened_terms.argtypes = [u64, sz, vp, sz, ctypes.c_uint, ctypes.c_uint, ctypes.c_uint, vp, vp, vp]
    out = np.full(4, 7.0, np.float32)
    s = np.zeros((4, 32), np.uint8)
    ok, bad = ctypes.c_int(5), sz(9)
    o, k, b, sp = out.ctypes.data, ctypes.addressof(ok), ctypes.addressof(bad), s.ctypes.data
    one = ctypes.addressof(_terms([1]))
    res = {
        "opened null out": L.rofl_acc_extract_opened(1, sp, 2048, 16, 32, 7, None, k, b),
        "opened null ok": L.rofl_acc_extract_opened(1, sp, 2048, 16, 32, 7, o, None, b),
        "opened table 0": L.rofl_acc_extract_opened(1, sp, 0, 16, 32, 7, o, k, b),
        "opened table 2^30": L.rofl_acc_extract_opened(1, sp, 1 << 30, 16, 32, 7, o, k, b),
        "opened bsgs bits 12": L.rofl_acc_extract_opened(1, sp, 2048, 12, 32, 7, o, k, b),
        "opened fp 24": L.rofl_acc_extract_opened(1, sp, 2048, 16, 24, 7, o, k, b),
        "opened fp frac 13": L.rofl_acc_extract_opened(1, sp, 2048, 16, 32, 13, o, k, b),
        "opened null opening": L.rofl_acc_extract_opened(1, None, 2048, 16, 32, 7, o, k, b),
        "opened unknown handle": L.rofl_acc_extract_opened(77, sp, 2048, 16, 32, 7, o, k, b),
        "opened unknown handle, no first_bad": L.rofl_acc_extract_opened(77, sp, 2048, 16, 32, 7, o, k, None),
        "terms null out": L.rofl_acc_extract_opened_terms(1, 1, one, 2048, 16, 32, 7, None, k, b),
        "terms null ok": L.rofl_acc_extract_opened_terms(1, 1, one, 2048, 16, 32, 7, o, None, b),
        "terms table 0": L.rofl_acc_extract_opened_terms(1, 1, one, 0, 16, 32, 7, o, k, b),
        "terms bsgs bits 12": L.rofl_acc_extract_opened_terms(1, 1, one, 2048, 12, 32, 7, o, k, b),
        "terms fp 24": L.rofl_acc_extract_opened_terms(1, 1, one, 2048, 16, 24, 7, o, k, b),
        "terms null terms": L.rofl_acc_extract_opened_terms(1, 1, None, 2048, 16, 32, 7, o, k, b),
        "terms 2^22 + 1 terms": L.rofl_acc_extract_opened_terms(1, (1 << 22) + 1, one, 2048, 16, 32, 7, o, k, b),      # (the count alone decides: nothing is read past it)
        "terms unknown handle": L.rofl_acc_extract_opened_terms(77, 1, one, 2048, 16, 32, 7, o, k, b),
        "terms unknown handle, no terms": L.rofl_acc_extract_opened_terms(77, 0, None, 2048, 16, 32, 7, o, k, b),
    }
    for sign in (0, 2, -2, 1 << 30):
        res["terms sign %d" % sign] = L.rofl_acc_extract_opened_terms(1, 2, ctypes.addressof(_terms([1, sign])), 2048, 16, 32, 7, o, k, b)
    assert res == {name: 11 for name in res}
    assert (out == 7.0).all() and ok.value == 5 and bad.value == 9      # nothing was written
    # a refused sign leaves a text without the seed
    assert L.rofl_acc_extract_opened_terms(1, 1, ctypes.addressof(_terms([3])), 2048, 16, 32, 7, o, k, b) == 11
    err = ctypes.create_string_buffer(512)
    L.rofl_last_error(err, sz(512))
    assert b"sign" in err.value and SEED.hex() not in err.value.decode() and SEED not in err.raw


def test_new_entry_points_are_exported_and_declared(hiplib):
    hdr = open(os.path.join(ROOT, "include", "rofl_zk.h")).read()
    ffi = open(os.path.join(ROOT, "integration", "rofl_crypto_overlay", "src", "ffi.rs")).read()
    for name in ("rofl_acc_extract_opened", "rofl_acc_extract_opened_terms"):
        assert hasattr(hiplib, name), name
        assert "int %s(" % name in hdr and "pub fn %s(" % name in ffi, name
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "check_ffi.py")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    wrap = open(os.path.join(ROOT, "integration", "rofl_crypto_overlay", "src", "pedersen_ops_gpu.rs")).read()
    assert "pub fn acc_extract_opened(" in wrap and "pub fn acc_extract_opened_terms(" in wrap


def test_pairwise_residual_terms_equal_the_sum_of_the_accepted_vectors(hiplib):
    from rofl_project_code_amd.api import pedersen_ops
    n, d = 5, 3
    seeds = {(i, j): bytes([16 * i + j]) * 32 for i in range(n) for j in range(i + 1, n)}
    own = [M.combine(pedersen_ops._pairwise_terms(i, [(j, seeds[(min(i, j), max(i, j))]) for j in range(n) if j != i]), d) for i in range(n)]
    assert not _sum_mod_l(own, d).any()      # the whole round cancels
    subsets = [a for r in range(1, n) for a in itertools.combinations(range(n), r)]
    assert len(subsets) == 30
    for acc in subsets:
        rej = [j for j in range(n) if j not in acc]
        terms = pedersen_ops.pairwise_residual_terms(acc, rej, seeds)
        assert len(terms) == len(acc) * len(rej)
        want = _sum_mod_l([own[i] for i in acc], d)
        assert M.combine(terms, d).tobytes() == want.tobytes(), acc
        assert want.any()      # somebody left: the blindings do not cancel
    assert pedersen_ops.pairwise_residual_terms(range(n), [], seeds) == []


def test_cancelling_residual_terms_equal_the_sum_of_the_accepted_vectors(hiplib):
    from rofl_project_code_amd.api import pedersen_ops
    n, d = 4, 3
    seeds = [M.vec_seed(SEED, i) for i in range(n - 1)]
    own = [M.combine([(s, 1)], d) for s in seeds] + [M.combine([(s, -1) for s in seeds], d)]
    for accept in itertools.product((False, True), repeat=n):
        terms = pedersen_ops.cancelling_residual_terms(n, SEED, accept)
        want = _sum_mod_l([own[i] for i in range(n) if accept[i]], d)
        assert M.combine(terms, d).tobytes() == want.tobytes(), accept
        assert len({s for s, _ in terms}) == len(terms) and all(sg in (1, -1) for _, sg in terms)      # what cancels is gone
    assert pedersen_ops.cancelling_residual_terms(n, SEED, [True] * n) == []
    assert pedersen_ops.cancelling_residual_terms(n, SEED, [False] * n) == []
    assert pedersen_ops.cancelling_residual_terms(n, SEED, [True, True, True, False]) == [(s, 1) for s in seeds]      # the last vector rejected
    assert pedersen_ops.cancelling_residual_terms(n, SEED, [False, False, False, True]) == [(s, -1) for s in seeds]   # only the last accepted
    assert pedersen_ops.cancelling_residual_terms(n, SEED, [True, False, True, True]) == [(seeds[1], -1)]
    assert pedersen_ops.cancelling_residual_terms(1, SEED, [True]) == []
    with pytest.raises(ValueError):
        pedersen_ops.cancelling_residual_terms(n, SEED, [True] * 3)


def test_helpers_and_extract_refuse_bad_arguments(hiplib):
    from rofl_project_code_amd import params
    from rofl_project_code_amd.api import pedersen_ops
    seeds = {(0, 1): SEED, (0, 2): SEED, (1, 2): SEED}
    with pytest.raises(KeyError, match=r"\(1, 3\)"):
        pedersen_ops.pairwise_residual_terms([0, 3], [1], {**seeds, (0, 3): SEED})
    with pytest.raises(KeyError, match=r"\(0, 2\)"):
        pedersen_ops.pairwise_residual_terms([2], [0], {(0, 1): SEED})
    with pytest.raises(ValueError):
        pedersen_ops.pairwise_residual_terms([0, 1], [1, 2], seeds)
    acc = params.DeviceAccumulator.__new__(params.DeviceAccumulator)      # (no device here: the check comes before anything else)
    with pytest.raises(ValueError):
        acc.extract_opened(opening=np.zeros((2, 32), np.uint8), opening_terms=[])
    with pytest.raises(ValueError):
        acc.extract_opened()
