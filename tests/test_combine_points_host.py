"""CPU-only checks of the shared-scalar point combination (rofl_combine_points / rofl_threshold_combine) on its host twin
rofl_dbg_host_combine_points / rofl_dbg_host_threshold_combine, and the helpers tests/test_gpu_combine_points.py shares.  The reference is
plain integers: the terms are P[i][j] = y_ij B for known y_ij, so out[i] = encode((sum_j a_j y_ij mod l) B), 32 zero bytes where the sum is 0;
bytes against bytes.  Every parameter check returns 11 before a device is touched.  No call here reaches a GPU."""
import ctypes
import hashlib

import numpy as np
import pytest

import dh_model as D

ELL = D.L
sz, vp, u32 = ctypes.c_size_t, ctypes.c_void_p, ctypes.c_uint32
COMBINE_ARGS = [sz, sz, vp, vp, vp, vp]
THRESHOLD_ARGS = [sz, sz, vp, vp, vp, vp, vp, vp, vp]


def _p(x):
    return None if x is None else x.ctypes.data


def b32(v):
    return np.frombuffer(int(v).to_bytes(32, "little"), np.uint8)


def ints(rows):
    return [int.from_bytes(bytes(r), "little") for r in np.asarray(rows, np.uint8).reshape(-1, 32)]


def expected(scalars, ys):
    """uint8[n_items, 32] for scalars a_j (ints, any size) and ys[i][j] (ints): encode((sum_j a_j y_ij mod l) B)"""
    ks = [sum(a * y for a, y in zip(scalars, row)) % ELL for row in ys]
    return np.stack([np.frombuffer(D._product(k, D.BASE_ENC, True) if k else bytes(32), np.uint8) for k in ks])


def combine(L, name, scalars, points, split=None):
    """-> (out, status) of an entry of rofl_combine_points' shape; split = (window_bits, slices) for rofl_dbg_combine_points_split"""
    scalars, points = np.ascontiguousarray(scalars, np.uint8).reshape(-1, 32), np.ascontiguousarray(points, np.uint8)
    n, t = points.shape[0], scalars.shape[0]
    out, status = np.full((n, 32), 0xaa, np.uint8), np.full(n, 0xaa, np.uint8)
    fn = getattr(L, name)
    fn.argtypes = COMBINE_ARGS + ([u32, u32, vp, vp] if split is not None else [])
    assert fn(n, t, _p(scalars), _p(points), _p(out), _p(status), *(split + (None, None) if split is not None else ())) == 0
    return out, status


def lagrange(xs):
    """the weights of rofl_shamir_reconstruct at the points xs, as integers mod l"""
    out = []
    for j, xj in enumerate(xs):
        num = den = 1
        for m, xm in enumerate(xs):
            if m != j:
                num, den = num * xm % ELL, den * (xm - xj) % ELL
        out.append(num * pow(den, -1, ELL) % ELL)
    return out


def points_of(ys):
    return np.stack([np.stack([np.frombuffer(D.public_key(b32(y)), np.uint8) for y in row]) for row in ys])


@pytest.mark.parametrize("n_items", [1, 3])
@pytest.mark.parametrize("n_terms", [1, 5])
def test_host_twin_against_integers(hiplib, n_items, n_terms):
    rng = np.random.default_rng(20271101 + 10 * n_items + n_terms)
    ys = [[int.from_bytes(rng.bytes(32), "little") % (ELL - 1) + 1 for _ in range(n_terms)] for _ in range(n_items)]
    pts = points_of(ys)
    for scalars in ([int.from_bytes(rng.bytes(32), "little") % ELL for _ in range(n_terms)], [ELL - 1] * n_terms, [0] * n_terms,
                    [(1 << 252) + ELL] + [7] * (n_terms - 1)):                     # random, carry out of the top window, empty schedule, a + l
        out, status = combine(hiplib, "rofl_dbg_host_combine_points", np.stack([b32(a) for a in scalars]), pts)
        assert out.tobytes() == expected(scalars, ys).tobytes() and not status.any()
    xs = [7, 2 ** 32 - 1, 3, 2 ** 31, 1][:n_terms]
    pk, ct = (np.frombuffer(D.public_key(b32(v)), np.uint8) for v in (11, 12))
    cts = np.ascontiguousarray(np.tile(ct, (n_items, 1)))
    out, shared, status = (np.full(s, 0xaa, np.uint8) for s in ((n_items, 32), (n_items, 32), n_items))
    fn = hiplib.rofl_dbg_host_threshold_combine
    fn.argtypes = THRESHOLD_ARGS
    assert fn(n_items, n_terms, _p(np.array(xs, np.uint32)), _p(pts), _p(pk), _p(cts), _p(out), _p(shared), _p(status)) == 0
    want = expected(lagrange(xs), ys)
    lo, hi = sorted((ct.tobytes(), pk.tobytes()))
    assert out.tobytes() == want.tobytes() and not status.any()
    assert shared.tobytes() == b"".join(hashlib.shake_256(D.DOM + w.tobytes() + lo + hi).digest(32) for w in want)


def test_host_twin_refuses_one_item_only(hiplib):
    ys = [[3, 4], [5, 6], [7, 8]]
    pts = points_of(ys)
    pts[1, 1] = 0xff                                                               # not a canonical field element
    out, status = combine(hiplib, "rofl_dbg_host_combine_points", np.stack([b32(9), b32(10)]), pts)
    assert status.tolist() == [0, 2, 0] and not out[1].any()
    assert out[[0, 2]].tobytes() == expected([9, 10], [ys[0], ys[2]]).tobytes()


def test_parameter_checks_come_before_the_device(hiplib):
    L = hiplib
    pts, sc, out, st = np.zeros((2, 3, 32), np.uint8), np.zeros((3, 32), np.uint8), np.zeros((2, 32), np.uint8), np.zeros(2, np.uint8)
    xs, pk = np.array([1, 2, 3], np.uint32), np.frombuffer(D.public_key(b32(5)), np.uint8)
    ct_bad = np.stack([pk, np.zeros(32, np.uint8)])                                # ciphertext point 1 is the identity
    for name in ("rofl_combine_points", "rofl_dbg_host_combine_points"):
        fn = getattr(L, name); fn.argtypes = COMBINE_ARGS
        assert fn(0, 3, None, None, None, None) == 0
        for args in ((2, 3, None, _p(pts), _p(out), _p(st)), (2, 3, _p(sc), None, _p(out), _p(st)), (2, 3, _p(sc), _p(pts), None, _p(st)),
                     (2, 3, _p(sc), _p(pts), _p(out), None), (2, 0, _p(sc), _p(pts), _p(out), _p(st)), (2, 65537, _p(sc), _p(pts), _p(out), _p(st)),
                     ((1 << 20) + 1, 1, _p(sc), _p(pts), _p(out), _p(st)), (1 << 20, 17, _p(sc), _p(pts), _p(out), _p(st))):
            assert fn(*args) == 11, (name, args[:2])
    for name in ("rofl_threshold_combine", "rofl_dbg_host_threshold_combine"):
        fn = getattr(L, name); fn.argtypes = THRESHOLD_ARGS
        assert fn(0, 3, None, None, None, None, None, None, None) == 0
        for bad_xs in ([1, 0, 3], [4, 2, 4]):
            assert fn(2, 3, _p(np.array(bad_xs, np.uint32)), _p(pts), None, None, _p(out), None, _p(st)) == 11
        for args in ((2, 3, None, _p(pts), None, None, _p(out), None, _p(st)), (2, 3, _p(xs), _p(pts), None, None, None, None, _p(st)),
                     (2, 3, _p(xs), _p(pts), _p(pk), None, _p(out), _p(out), _p(st)), (2, 3, _p(xs), _p(pts), _p(np.zeros(32, np.uint8)), _p(ct_bad), None, _p(out), _p(st))):
            assert fn(*args) == 11, (name, args[:2])
        assert fn(2, 3, _p(xs), _p(pts), _p(pk), _p(ct_bad), None, _p(out), _p(st)) == 11
        buf = ctypes.create_string_buffer(512); L.rofl_last_error(buf, sz(512))
        assert b"ciphertext point 1 " in buf.value
