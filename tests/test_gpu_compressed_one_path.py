"""The three ways to verify a CompressedRandProof -- rofl_verify_compressed_randproof (one client), rofl_verify_compressed_randproof_batch
(host bytes, groups of sixteen) and the compressed leg of a ROFL_ROUND_COMPRESSED round (from the round's cache) -- share one verifier.
Every member's expected verdict comes from the CPU oracle (orc.compressed_verify), never from the library; the three ways must each agree
with it, and the decode counter must move by 2 d, 2 d nc and 0.

Shapes: a powers thread writes four consecutive exponents and a block 256 x 4 = 1024 of them, so d runs over 1, 3, 4, 5 (a partial run, a
whole run, a run and one more) and 1023, 1024, 1025 (a block less one, a block, a second block of one thread).  Client counts 1, 5 (from five
on eight transcripts share an AVX-512 stream) and 17 (a second group, of one).  Members: honest; a pair's L replaced by another client's L;
a pair's R undecodable; non-canonical Z_m; undecodable L'; and, for the round, a NULL proof (the host-bytes calls get that member's honest
proof).  The tampered pair is the last one, d - 1: the end of a partial run of exponents, and at d = 1025 the second block."""
import numpy as np
import pytest

import orc

pytestmark = pytest.mark.gpu
FP = (32, 7)
BAD_POINT = np.frombuffer(bytes([1] + [0] * 31), np.uint8)      # odd s: not a Ristretto encoding
KINDS = ("honest", "foreign L", "undecodable R", "non-canonical Z_m", "undecodable L'", "NULL proof")
MALFORMED = {"undecodable R": "invalid ElGamal pair", "non-canonical Z_m": "", "undecodable L'": ""}      # the single call's FormatError (text after "FormatError")
POOL = 17


@pytest.fixture(scope="module")
def R():
    import rofl_project_code_amd as R
    from rofl_project_code_amd import build
    build.build()
    R.set_device(0)
    R.api.set_fp(*FP)
    return R


_honest, _oracle = {}, {}


def _pool(R, d):
    """seventeen honest (proof, pairs) of d elements, made once per d and never written to"""
    if d not in _honest:
        rng = np.random.default_rng(4100 + d)
        out = []
        for i in range(POOL):
            x = (rng.integers(-100, 100, size=d) / 128.0).astype(np.float32)
            bl = rng.integers(0, 256, size=(d, 32), dtype=np.uint8); bl[:, 31] &= 0x0F
            out.append(R.compressed_rand_proof.helper_prove(x, bl, nonce=R.Nonce.seeded(bytes([i + 1]) * 32), fp=FP))
        _honest[d] = out
    return _honest[d]


def _member(R, d, i, kind):
    """(proof, pairs, oracle's (rc, ok)) of pool member i tampered as `kind`"""
    pool = _pool(R, d)
    proof, pairs = pool[i][0].copy(), pool[i][1].copy()
    j = d - 1
    if kind == "foreign L":
        other = pool[(i + 1) % POOL][1]
        assert (other[j, :32] != pairs[j, :32]).any()
        pairs[j, :32] = other[j, :32]
    elif kind == "undecodable R":
        pairs[j, 32:64] = BAD_POINT
    elif kind == "non-canonical Z_m":
        proof[64:96] = 0xFF
    elif kind == "undecodable L'":
        proof[0:32] = BAD_POINT
    key = (d, i, kind)
    if key not in _oracle:
        _oracle[key] = orc.compressed_verify(proof, pairs)
    return proof, pairs, _oracle[key]


@pytest.mark.parametrize("nc", [1, 5, 17])
@pytest.mark.parametrize("d", [1, 3, 4, 5, 1023, 1024, 1025])
def test_three_ways_agree_with_the_oracle(R, d, nc):
    api, crp, pd = R.api, R.compressed_rand_proof, R.api.point_decodes
    assert R.get_option("devices") == 0
    seen = set()
    h = api.device_round.create(d, 64, nc, api.device_round.COMPRESSED)
    try:
        for v in range((len(KINDS) + nc - 1) // nc):      # enough passes for every kind to have been some member's
            kinds = [KINDS[(i + v * nc) % len(KINDS)] for i in range(nc)]
            seen.update(kinds)
            ms = [_member(R, d, i, k) for i, k in enumerate(kinds)]
            want = [rc == 0 and ok for _, _, (rc, ok) in ms]
            for k, w, (_, _, (rc, _)) in zip(kinds, want, ms):
                assert w == (k in ("honest", "NULL proof")), k      # (the oracle accepts what was made honestly and nothing else)
                assert (rc != 0) == (k in MALFORMED), k
            # one client per call
            for k, w, (proof, pairs, (rc, _)) in zip(kinds, want, ms):
                c0 = pd()
                if k in MALFORMED:
                    with pytest.raises(R.RoflError) as e:
                        crp.helper_verify(proof, pairs)
                    assert e.value.code == 5 == rc
                    assert str(e.value) == "FormatError (5): FormatError" + (": " + MALFORMED[k] if MALFORMED[k] else ""), k
                    assert pd() - c0 == (2 * d if k == "undecodable R" else 0), k      # a malformed proof is refused before anything is decoded
                else:
                    assert crp.helper_verify(proof, pairs) is w, k
                    assert pd() - c0 == 2 * d
            # the batch on host bytes
            c0 = pd()
            got = crp.helper_verify_batch([m[0] for m in ms], [m[1] for m in ms])
            print("d", d, "nc", nc, "pass", v, kinds, "batch", got)
            assert got == want
            assert pd() - c0 == 2 * d * nc
            # the round's leg
            api.device_round.reset(h)
            assert api.device_round.ingest(h, [m[1].ctypes.data for m in ms]) == 0
            c0 = pd()
            leg = api.device_round.verify_compressed(h, [None if k == "NULL proof" else m[0].ctypes.data for k, m in zip(kinds, ms)])
            print("d", d, "nc", nc, "pass", v, "round", leg)
            assert leg == [w and k != "NULL proof" for k, w in zip(kinds, want)]
            assert pd() == c0
    finally:
        api.device_round.destroy(h)
    assert seen == set(KINDS)
