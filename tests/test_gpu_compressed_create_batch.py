"""rofl_create_compressed_randproof_batch (compressed_rand_proof.helper_prove_batch): the CompressedRandProofs of several clients of one
process in one launch sequence -- groups of sixteen clients, k_eg_pairs_batch (one thread per point, blocks of 64 elements) and
k_cpow_dot_batch (64 blocks of 256 per client, grid-stride).  Every client's proof and pairs must be the bytes of its own single call
(helper_prove / helper_prove_existing) and of the CPU oracle (orc.compressed_create), whatever its neighbours in the batch are.
The single call (rofl_create_compressed_randproof) runs the same code as a group of one: "batch equals single" says that a client's
neighbours do not matter, and the oracle -- or, at the one shape where its create is too slow, another kernel and the verifiers -- anchors
the bytes of both.  The single call's own promises are here too: its error order and texts, device-resident inputs, the caller's device
under the `devices` option.

Shapes: d around the pairs kernel's block (63, 64, 65) and the dot kernel's block (255, 256, 257), 0 and 1; n = 1, 2 and 17 (a second
group, of one); d = 64 * 256 + 1, where the dot kernel's grid-stride loop wraps for exactly one thread."""
import os
import subprocess
import sys

import numpy as np
import pytest

import orc

pytestmark = pytest.mark.gpu
FP = (16, 7)
GROUP = 16                # clients per launch (kCompCreateGroup)
DOT_BLOCKS = 64           # blocks of 256 per client in k_cpow_dot_batch (kCompDotBlocks)
DS = (0, 1, 63, 64, 65, 255, 256, 257)


@pytest.fixture(scope="module")
def R():
    import rofl_project_code_amd as R
    from rofl_project_code_amd import build
    build.build()
    R.set_device(0)
    return R


def _nonce(R, i, mode):
    """client i's prover randomness: (Nonce, the oracle's keyword)"""
    if mode == "seed":
        return R.Nonce.seeded(bytes([i + 1]) * 32), dict(seed=bytes([i + 1]) * 32)
    s = np.random.default_rng(9000 + i).integers(0, 256, size=128, dtype=np.uint8).tobytes()      # two wide scalars: m', r'
    return R.Nonce.stream(s), dict(stream=s)


_inputs, _single, _oracle = {}, {}, {}


def _client(R, d, i):
    """(values, blindings, commitments of the values) of client i at length d, made once and never written to"""
    if (d, i) not in _inputs:
        rng = np.random.default_rng(5000 + 31 * d + i)
        x = (rng.integers(-100, 100, size=d) / 128.0).astype(np.float32)
        bl = rng.integers(0, 256, size=(d, 32), dtype=np.uint8); bl[:, 31] &= 0x0F
        com = R.pedersen_ops.commit_vec(R.conversion32.f32_to_scalar_vec(x, fp=FP), bl) if d else np.zeros((0, 32), np.uint8)
        _inputs[(d, i)] = (x, bl, com)
    return _inputs[(d, i)]


def _one(R, d, i, mode, existing=False):
    """the single call's (proof, pairs) for client i, computed once per case"""
    key = (d, i, mode, existing)
    if key not in _single:
        x, bl, com = _client(R, d, i)
        _single[key] = R.compressed_rand_proof.helper_prove(x, bl, nonce=_nonce(R, i, mode)[0], existing=com if existing else None, fp=FP)
    return _single[key]


def _orc(R, d, i, mode, existing=False):
    key = (d, i, mode, existing)
    if key not in _oracle:
        x, bl, com = _client(R, d, i)
        _oracle[key] = orc.compressed_create(x, bl, FP[0], FP[1], existing=com if existing else None, **_nonce(R, i, mode)[1])
    return _oracle[key]


def _is_oracle(got, want):
    """got = (proof, pairs) against the oracle's (rc, proof, pairs)"""
    return want[0] == 0 and _same(got, want[1:])


def _same(got, want):
    return not isinstance(got, Exception) and got[0].shape == want[0].shape and got[1].shape == want[1].shape and (got[0] == want[0]).all() and (got[1] == want[1]).all()


@pytest.mark.parametrize("mode", ["seed", "stream"])
@pytest.mark.parametrize("n,d", [(GROUP + 1, 65), (1, 257)] + [(2, d) for d in DS], ids=lambda v: str(v))
def test_bytes_equal_the_single_call_and_the_oracle(R, n, d, mode):
    cl = [_client(R, d, i) for i in range(n)]
    got = R.compressed_rand_proof.helper_prove_batch([c[0] for c in cl], [c[1] for c in cl], nonces=[_nonce(R, i, mode)[0] for i in range(n)], fp=FP)
    assert len(got) == n
    for i in range(n):
        assert _same(got[i], _one(R, d, i, mode)), ("single call", i)
        assert _is_oracle(_one(R, d, i, mode), _orc(R, d, i, mode)), ("single call against the oracle", i)
        rc, oproof, opairs = _orc(R, d, i, mode)
        assert rc == 0 and _same(got[i], (oproof, opairs)), ("oracle", i)
        assert R.compressed_rand_proof.helper_verify(got[i][0], got[i][1]) is True
        assert orc.compressed_verify(got[i][0], got[i][1]) == (0, True)


@pytest.mark.parametrize("mode", ["seed", "stream"])
@pytest.mark.parametrize("d", DS)
def test_the_single_call_equals_the_oracle(R, d, mode):
    """helper_prove alone against orc.compressed_create: the single call is a group of one, so "batch equals single" compares two group
    compositions and the oracle is the anchor of the bytes."""
    got = _one(R, d, 0, mode)
    assert _is_oracle(got, _orc(R, d, 0, mode))
    assert R.compressed_rand_proof.helper_verify(got[0], got[1]) is True


@pytest.mark.parametrize("mode", ["seed", "stream"])
def test_the_single_call_with_existing_equals_the_oracle(R, mode):
    d = 65
    x, bl, com = _client(R, d, 0)
    got = R.compressed_rand_proof.helper_prove_existing(x, com, bl, nonce=_nonce(R, 0, mode)[0], fp=FP)
    assert _is_oracle(got, _orc(R, d, 0, mode, existing=True))
    assert _same(got, _one(R, d, 0, mode, existing=True))
    assert (got[1][:, :32] == com).all()


def test_the_dot_products_grid_stride_wraps(R):
    """d = 64 * 256 + 1: thread 0 of block 0 of every client takes a second element.  The oracle's create at this size takes too long, so
    the bytes of the single call and of the batch of two are anchored without it: the pairs' L are pedersen_ops.commit_vec's (another
    kernel), C' (the proof's first 64 bytes, which do not depend on d) is that of the oracle's proof at d = 1 under the same nonce, and
    the library's and the oracle's verifiers accept.  Given the pairs, C' and the challenge, the two equations fix Z_m, Z_r: all 128
    bytes are pinned."""
    d, n = DOT_BLOCKS * 256 + 1, 2
    cl = [_client(R, d, i) for i in range(n)]
    got = R.compressed_rand_proof.helper_prove_batch([c[0] for c in cl], [c[1] for c in cl], nonces=[_nonce(R, i, "seed")[0] for i in range(n)], fp=FP)
    for i in range(n):
        one = _one(R, d, i, "seed")
        assert _same(got[i], one), i
        for proof, pairs in (one, got[i]):
            assert (pairs[:, :32] == cl[i][2]).all(), i
            rc1, proof1, _ = _orc(R, 1, i, "seed")
            assert rc1 == 0 and (proof[:64] == proof1[:64]).all(), i
            assert R.compressed_rand_proof.helper_verify(proof, pairs) is True
        assert orc.compressed_verify(one[0], one[1]) == (0, True)


@pytest.mark.parametrize("with_existing", [(False, True, False), (True, False, True)], ids=["middle", "outer"])
def test_mixed_existing(R, with_existing):
    d, n = 65, 3
    cl = [_client(R, d, i) for i in range(n)]
    got = R.compressed_rand_proof.helper_prove_batch([c[0] for c in cl], [c[1] for c in cl], nonces=[_nonce(R, i, "seed")[0] for i in range(n)],
                                                      existing_list=[c[2] if e else None for c, e in zip(cl, with_existing)], fp=FP)
    for i in range(n):
        assert _same(got[i], _one(R, d, i, "seed", existing=with_existing[i])), i
        assert _is_oracle(got[i], _orc(R, d, i, "seed", existing=with_existing[i])), ("oracle", i)


def test_a_failing_member_does_not_sink_the_call(R):
    d, n = 65, 5
    cl = [_client(R, d, i) for i in range(n)]
    xs, bls = [c[0] for c in cl], [c[1] for c in cl]
    xs[1] = xs[1].copy(); xs[1][40] = np.nan
    ex = [None] * n
    ex[2] = cl[2][2].copy(); ex[2][64] = 0xFF
    nonces = [_nonce(R, i, "seed")[0] for i in range(n)]
    nonces[3] = R.Nonce.stream(bytes(range(64)))      # one wide scalar: m' without r'
    got = R.compressed_rand_proof.helper_prove_batch(xs, bls, nonces=nonces, existing_list=ex, fp=FP)      # (returns: the call's own code is 0)
    assert [g.code if isinstance(g, R.RoflError) else 0 for g in got] == [0, 10, 5, 12, 0]
    for i in (0, 4):
        assert _same(got[i], _one(R, d, i, "seed")), i
    # the single call's order for a client with both faults: the non-finite value first
    ex[1] = ex[2]
    both = R.compressed_rand_proof.helper_prove_batch(xs[:2], bls[:2], nonces=nonces[:2], existing_list=ex[:2], fp=FP)
    assert _same(both[0], _one(R, d, 0, "seed")) and isinstance(both[1], R.RoflError) and both[1].code == 10
    with pytest.raises(R.RoflError) as e:
        R.compressed_rand_proof.helper_prove(xs[1], bls[1], nonce=nonces[1], existing=ex[1], fp=FP)
    assert e.value.code == 10


def _raises(R, code, text, *args, **kw):
    """the single call fails with `code` and rofl_last_error's text `text`"""
    with pytest.raises(R.RoflError) as e:
        R.compressed_rand_proof.helper_prove(*args, **kw)
    assert e.value.code == code and str(e.value) == "%s (%d): %s" % (e.value.name, code, text), str(e.value)


def test_the_single_calls_error_order_and_texts(R):
    """WrongNumBlindingFactors (1) before a bad parameter (11) before a short stream (12), all before any device work; then a non-finite
    value (10) before an undecodable commitment (5).  Codes as rofl_zk.h numbers them, texts as rofl_last_error gives them."""
    d = 65
    x, bl, com = _client(R, d, 0)
    nonce = _nonce(R, 0, "seed")[0]
    short = R.Nonce.stream(bytes(range(64)))      # one wide scalar: m' without r'
    xnan = x.copy(); xnan[40] = np.nan
    bad = com.copy(); bad[64] = 0xFF
    NAN = "non-finite value (the reference panics in fixed::saturating_from_float)"
    _raises(R, 1, "WrongNumBlindingFactors", x, bl[:-1], nonce=nonce, fp=FP)
    _raises(R, 1, "WrongNumBlindingFactors", xnan, bl[:-1], nonce=short, existing=bad, fp=(16, 16))      # before everything else
    _raises(R, 11, "bad parameter", x, bl, nonce=nonce, fp=(16, 16))
    _raises(R, 11, "bad parameter", x, bl, nonce=nonce, fp=(12, 7))
    _raises(R, 11, "bad parameter", xnan, bl, nonce=short, existing=bad, fp=(16, 16))                    # before the stream's length
    _raises(R, 12, "nonce stream too short", x, bl, nonce=short, fp=FP)
    _raises(R, 12, "nonce stream too short", xnan, bl, nonce=short, existing=bad, fp=FP)                 # before the device sees the values
    _raises(R, 10, NAN, xnan, bl, nonce=nonce, fp=FP)
    _raises(R, 10, NAN, xnan, bl, nonce=nonce, existing=bad, fp=FP)                                      # before the commitment
    _raises(R, 5, "invalid Ristretto encoding", x, bl, nonce=nonce, existing=bad, fp=FP)
    assert _same(R.compressed_rand_proof.helper_prove(x, bl, nonce=nonce, fp=FP), _one(R, d, 0, "seed"))      # (and the next call is sound)


def test_device_resident_inputs():
    """One client's values, r and existing as device pointers (torch tensors on the GPU), its neighbours' in host memory: same bytes.
    (Own process: torch has to bring up its HIP runtime before the library's is loaded.)"""
    r = subprocess.run([sys.executable, os.path.join(os.path.dirname(__file__), "gpu_compressed_create_batch_device_check.py")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "DEVICE_INPUTS PASS" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


def test_devices_option(R):
    """rofl_set_option("devices", 0b11), both logical devices on the one GPU: five clients dealt round-robin, same bytes"""
    from rofl_project_code_amd import api
    api.map_device(1, 0)
    d, n = 65, 5
    cl = [_client(R, d, i) for i in range(n)]
    ex = [cl[i][2] if i == 3 else None for i in range(n)]
    try:
        R.set_option("devices", 0b11)
        got = R.compressed_rand_proof.helper_prove_batch([c[0] for c in cl], [c[1] for c in cl], nonces=[_nonce(R, i, "seed")[0] for i in range(n)], existing_list=ex, fp=FP)
        one = [R.compressed_rand_proof.helper_prove(cl[i][0], cl[i][1], nonce=_nonce(R, i, "seed")[0], existing=ex[i], fp=FP) for i in (0, 3)]      # the single call under the option
    finally:
        R.set_option("devices", 0)
    for i in range(n):
        assert _same(got[i], _one(R, d, i, "seed", existing=i == 3)), i
    assert _is_oracle(one[0], _orc(R, d, 0, "seed")) and _is_oracle(one[1], _orc(R, d, 3, "seed", existing=True))
