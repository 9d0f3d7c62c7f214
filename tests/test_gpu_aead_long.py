"""GPU checks of the long route of rofl_aead_seal / rofl_aead_open (k_aead_long_seal, k_aead_long_mac, k_aead_long_*_finish,
k_aead_long_decrypt), byte for byte against the Python model tests/aead_model.py -- no tolerance anywhere.  The debug entries send every
record of a call down the long route with segments of one pass tile, so tile and segment boundaries are reached with kilobytes."""
import ctypes

import numpy as np
import pytest

import aead_model as A
import test_aead_host as H

pytestmark = pytest.mark.gpu
AD_LENS = (0, 1, 16, 17)


@pytest.fixture(scope="module")
def R():
    import rofl_project_code_amd as R
    from rofl_project_code_amd import build
    build.build()
    R.set_device(0)
    return R


def _batch(seed, lens):
    """records of the given payload lengths x every AD length, packed back to back, sealed by the model once"""
    rng = np.random.default_rng(seed)
    pts = [rng.bytes(p) for p in lens for _ in AD_LENS]
    ads = [rng.bytes(a) for _ in lens for a in AD_LENS]
    n = len(pts)
    keys, nonces = np.frombuffer(rng.bytes(32 * n), np.uint8).reshape(n, 32), np.frombuffer(rng.bytes(12 * n), np.uint8).reshape(n, 12)
    return keys, nonces, ads, pts, A.seal_batch(keys, nonces, ads, pts)


@pytest.mark.parametrize("built", [False, True], ids=["seg=tile", "seg=built"])
def test_forced_route_equals_the_model(R, built):
    tile, seg, _ = R.aead.long_geometry()
    t, s = 16 * tile, 16 * (seg if built else tile)
    lens = [s - 1, s, s + 1, 2 * s + 17] if built else [0, 1, 15, 16, 17, 63, 64, 65, t - 1, t, t + 1, s - 1, s, s + 1, 2 * s + 17, 3 * s]
    keys, nonces, ads, pts, want = _batch(20261301 + built, lens)
    starts = np.cumsum([0] + [len(p) for p in pts])[:-1]
    assert {int(x) % 4 for x in starts} == {0, 1, 2, 3} and {int(x) % 4 for x in starts + 16 * np.arange(len(pts))} == {0, 1, 2, 3}
    sb = 0 if built else tile
    assert R.aead.seal(keys, nonces, ads, pts, long_seg_blocks=sb) == want
    back, v = R.aead.open(keys, nonces, ads, want, long_seg_blocks=sb)
    assert back == pts and v.tolist() == [0] * len(pts)


def test_verdicts_on_the_forced_route(R):
    tile = R.aead.long_geometry()[0]
    s = 16 * tile
    keys, nonces, ads, pts, good = _batch(20261303, [3 * s, 2 * s + 17, s + 1, 3 * s + 5, 40, 2 * s])
    sel = [4 * k + k % 4 for k in range(6)]      # one record per payload length, the AD lengths in turn
    keys, nonces, ads, pts, recs = keys[sel], nonces[sel], [ads[i] for i in sel], [pts[i] for i in sel], [bytearray(good[i]) for i in sel]
    recs[1][0] ^= 0x01                       # the first ciphertext byte
    recs[3][3 * s + 2] ^= 0x80               # a byte of the last segment
    recs[5][-1] ^= 0x10                      # the tag's last byte
    recs[4] = recs[4][:15]                   # shorter than a tag
    want_v = [0, 1, 0, 1, 2, 1]
    back, v = R.aead.open(keys, nonces, ads, [bytes(r) for r in recs], long_seg_blocks=tile)
    assert v.tolist() == want_v
    assert back == [p if w == 0 else b"" if w == 2 else bytes(len(p)) for p, w in zip(pts, want_v)]


def test_poly1305_boundary_through_the_long_route(R):
    """the largest clamped r over 1, T, T + 1 and S + 1 blocks of ff (the powers r^T and r^S with limbs near their bounds), and the r = 1
    family around p = 2^130 - 5; seg_blocks 0 and one pass tile"""
    tile, seg, _ = R.aead.long_geometry()
    key = A.CLAMP.to_bytes(16, "little") + (0x0123456789abcdef0123456789abcdef).to_bytes(16, "little")
    cases = [(key, b"\xff" * (16 * b)) for b in (1, tile, tile + 1, seg + 1)] + [(k, m) for k, m, _ in A.poly_boundary_cases() if m and len(m) % 16 == 0]
    want = [A.poly1305(k, m) for k, m in cases]
    keys = np.frombuffer(b"".join(k for k, _ in cases), np.uint8).reshape(-1, 32).copy()
    msg, off = A.pack([m for _, m in cases])
    for sb in (0, tile):
        out = np.full((len(cases), 16), 0xaa, np.uint8)
        assert H._call(R.lib(), "rofl_dbg_poly1305_long", H.POLY_ARGS + [ctypes.c_uint32], len(cases), keys, msg, off, out, sb) == 0
        assert [bytes(t) for t in out] == want, sb


def test_public_route_mixes_short_and_long_records(R):
    lmin = R.aead.long_geometry()[2]
    rng = np.random.default_rng(20261304)
    lens = [int(x) for x in rng.integers(0, 300, 200)] + [lmin - 1, lmin, 2 * lmin + 17]
    order = rng.permutation(len(lens))
    pts, ads = [rng.bytes(lens[i]) for i in order], [rng.bytes(int(x)) for x in rng.integers(0, 41, len(lens))]
    keys, nonces = np.frombuffer(rng.bytes(32 * 5), np.uint8).reshape(5, 32), np.frombuffer(rng.bytes(12 * len(lens)), np.uint8).reshape(-1, 12)
    idx = [int(x) for x in rng.integers(0, 5, len(lens))]
    want = A.seal_batch(keys, nonces, ads, pts, key_idx=idx)
    assert R.aead.seal(keys, nonces, ads, pts, key_idx=idx) == want
    back, v = R.aead.open(keys, nonces, ads, want, key_idx=idx)
    assert back == pts and not v.any()
