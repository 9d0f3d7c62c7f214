"""CPU-only checks of the standard key agreement (rofl_x25519_*): the Python model tests/x25519_model.py pinned to the vectors of RFC 7748
and, where one loads, to libsodium; then the host twin rofl_dbg_host_x25519 against the model, bytes and status, on the edge corpus; the
refused and the empty calls.  No call here reaches a GPU."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import x25519_model as X
from test_ed25519_host import call, rows

h = bytes.fromhex
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def host(L, keys, us):
    out, st = np.full((len(keys), 32), 0xaa, np.uint8), np.full(len(keys), 0xaa, np.uint8)
    assert call(L, "rofl_dbg_host_x25519", len(keys), rows(keys), None if us is None else rows(us), out, st) == 0
    return [o.tobytes() for o in out], st.tolist()


def test_the_model_is_rfc_7748():
    assert X.x25519(h("a546e36bf0527c9d3b16154b82465edd62144c0ac1fc5a18506a2244ba449ac4"), h("e6db6867583030db3594c1a424b15f7c726624ec26b3353b10a903a6d0ab1c4c")) \
        == h("c3da55379de9c6908e94ea4df28d084f32eccf03491c71f754b4075577a28552")
    assert X.x25519(h("4b66e9d4d1b4673c5ad22691957d6af5c11b6421e0ea01d42ca4169e7918ba0d"), h("e5210f12786811d3f4b7959d0538ae2c31dbe7106fc03c3efc4cd549c715a493")) \
        == h("95cbde9476e8907d7aade45cb4b873f88b595a68799fa152e6f8f7647aac7957")
    k = u = (9).to_bytes(32, "little")
    for i in range(1000):
        k, u = X.x25519(k, u), k
        assert i or k == h("422c8e7a6227d7bca1350b3e2bb7279f7897b87bb6854b783c60e80311ae3079")
    assert k == h("684cf59ba83309552800ef566f2f4d3c1c3887c49360e3875f2eb94d99532c51")
    a, b = h("77076d0a7318a57d3c16c17251b26645df4c2f87ebc0992ab177fba51db92c2a"), h("5dab087e624a8a4b79e17f8b83800ee66f3bb1292618b6fd1c2f8b27ff88e0eb")
    pa, pb = X.public_key(a), X.public_key(b)
    assert pa == h("8520f0098930a754748b7ddcb43ef75a0dbf3a0d26381af4eba4a98eaa9b4e6a") and pb == h("de9edb7d7b7dc1b4d35b61c2ece435373f8343c85b78674dadfc7e146f882b4f")
    assert X.shared(a, pb) == X.shared(b, pa) == (h("4a5d9d5ba4ce2de1728e3bf480350f25e07e21c947d19e3376f09b3c1e161742"), 0)


def test_the_model_is_libsodium():
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import sodium_bp
    so = sodium_bp.load_sodium()
    if so is None:
        pytest.skip("no libsodium on this box")
    for k, u in zip(X.CORPUS_K * 4, X.CORPUS_U[-16:]):
        q = ctypes.create_string_buffer(32)
        assert so.crypto_scalarmult_curve25519(q, k, u) == 0 and X.x25519(k, u) == q.raw


@pytest.mark.parametrize("k", range(len(X.CORPUS_K)))
def test_the_host_twin_on_the_edge_corpus(hiplib, k):
    key, n_small = X.CORPUS_K[k], 2 * len(X.SMALL_ORDER)
    want = [X.shared(key, u) for u in X.CORPUS_U]
    assert [w for w in want[:n_small]] == [(bytes(32), 2)] * n_small and not any(s for _, s in want[n_small:])
    assert want[n_small][0] == X.x25519(key, (18).to_bytes(32, "little")) and want[n_small + 1][0] == X.public_key(key)
    got, st = host(hiplib, [key] * len(X.CORPUS_U), X.CORPUS_U)
    assert got == [w for w, _ in want] and st == [s for _, s in want]
    assert host(hiplib, [key], None) == ([X.public_key(key)], [0])


def noncanonical_want():
    """[(32 bytes, status)] of CORPUS_K x NONCANONICAL_U, key-major, from the model -- held to what reduction says: u = p + i is u = i, so zeros
    and status 2 for i in {0, 1} and x25519(k, i) for the rest, whatever bit 255 holds"""
    want = [X.shared(k, u) for k in X.CORPUS_K for u in X.NONCANONICAL_U]
    assert len(X.NONCANONICAL_U) == 38 and len(set(X.NONCANONICAL_U)) == 38
    assert all(X.P <= int.from_bytes(u, "little") % 2**255 < 2**255 and (int.from_bytes(u, "little") >> 255) == j // 19 for j, u in enumerate(X.NONCANONICAL_U))
    assert want == [(bytes(32), 2) if j % 19 < 2 else (X.x25519(k, (j % 19).to_bytes(32, "little")), 0) for k in X.CORPUS_K for j in range(38)]
    return want


def test_the_host_twin_on_every_noncanonical_u(hiplib):
    want = noncanonical_want()
    got, st = host(hiplib, [k for k in X.CORPUS_K for _ in X.NONCANONICAL_U], X.NONCANONICAL_U * len(X.CORPUS_K))
    assert got == [w for w, _ in want] and st == [s for _, s in want] and st.count(2) == 4 * len(X.CORPUS_K)


@pytest.mark.parametrize("mask", [(0, 0x07), (31, 0x40), (31, 0x80), (31, 0xc0)])
def test_keys_that_differ_only_in_the_clamped_bits(hiplib, mask):
    rng = np.random.default_rng(20261202)
    keys = [rng.bytes(32) for _ in range(4)]
    flipped = [bytes(b ^ mask[1] if i == mask[0] else b for i, b in enumerate(k)) for k in keys]
    us = X.CORPUS_U[-4:]
    got = host(hiplib, keys + flipped, us + us)
    assert got[0][:4] == got[0][4:] == [X.x25519(k, u) for k, u in zip(keys, us)] and got[1] == [0] * 8


def test_refused_and_empty_calls(hiplib):
    k, out, st = rows(X.CORPUS_K), np.zeros((16, 32), np.uint8), np.zeros(16, np.uint8)
    pairs = np.array([[0, 0], [3, 4]], np.uint32)
    assert call(hiplib, "rofl_x25519_public_keys", 0, None, None) == 0 and call(hiplib, "rofl_x25519_shared", 0, None, None, 0, None, 0, None, None, None) == 0
    assert call(hiplib, "rofl_dbg_host_x25519", 0, None, None, None, None) == 0 and call(hiplib, "rofl_dbg_host_x25519", 1, k, k, None, st) == 11
    assert call(hiplib, "rofl_x25519_public_keys", 4, None, out) == 11 and call(hiplib, "rofl_x25519_public_keys", 4, k, None) == 11
    for args in ((4, None, None, 4, k, 16, None, out, st), (4, k, None, 4, None, 16, None, out, st), (4, k, None, 4, k, 16, None, None, st),
                 (4, k, None, 4, k, 16, None, out, None), (4, k, None, 4, k, 15, None, out, st), (4, k, None, 4, k, 2, pairs, out, st)):
        assert call(hiplib, "rofl_x25519_shared", *args) == 11 and call(hiplib, "rofl_dbg_x25519_shared", 1, *args) == 11
    assert call(hiplib, "rofl_dbg_x25519_shared", 3, 4, k, None, 4, k, 16, None, out, st) == 11
    text = open(os.path.join(ROOT, "include", "rofl_zk.h")).read()
    assert "int rofl_x25519_public_keys(" in text and "int rofl_x25519_shared(" in text
    assert subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "check_ffi.py")], capture_output=True).returncode == 0
