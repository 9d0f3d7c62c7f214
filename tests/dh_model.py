"""Python model of the key agreement of rofl_dh_public_keys / rofl_dh_shared (include/rofl_zk.h), shared by test_key_agreement_host.py and
test_gpu_key_agreement.py:
  secret key = 32 little-endian bytes reduced mod l; public key = encode(sk * B);
  shared(a, P_b) = SHAKE256("rofl-zk/dh/v1" || 000000 || encode(a * decode(P_b)) || lo || hi)[0 .. 32), lo <= hi the two public keys as byte strings;
  status 1: P_b is not a canonical Ristretto encoding, 2: it is the identity -- 32 zero bytes out.
The point arithmetic is tests/golden/pyref.py; fast=True takes the product from the oracle's MSM of one term instead (same bytes, ~100x faster)."""
import hashlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import pyref  # noqa: E402

L = pyref.L
DOM = b"rofl-zk/dh/v1\0\0\0"
BASE_ENC = pyref.ristretto_encode(pyref.BASE)


def sk_int(sk):
    return int.from_bytes(bytes(sk), "little") % L


def _product(k, enc, fast):
    """encode(k * decode(enc)) for a valid, non-identity enc and k != 0"""
    if fast:
        import orc
        return orc.msm(np.frombuffer(k.to_bytes(32, "little"), np.uint8), np.frombuffer(bytes(enc), np.uint8)).tobytes()
    return pyref.ristretto_encode(pyref.pt_mul(k, pyref.ristretto_decode(bytes(enc))))


def public_key(sk, fast=True):
    k = sk_int(sk)
    assert k != 0, "a secret key is not 0 mod l"
    return _product(k, BASE_ENC, fast)


def shared(sk, peer_pk, own_pk=None, fast=True):
    """-> (32 bytes, status)"""
    peer_pk = bytes(peer_pk)
    p = pyref.ristretto_decode(peer_pk)
    if p is None:
        return bytes(32), 1
    if peer_pk == bytes(32):
        return bytes(32), 2
    own = bytes(own_pk) if own_pk is not None else public_key(sk, fast)
    lo, hi = (own, peer_pk) if own <= peer_pk else (peer_pk, own)
    s = _product(sk_int(sk), peer_pk, fast)
    return hashlib.shake_256(DOM + s + lo + hi).digest(32), 0


def shared_batch(sks, peer_pks, pairs=None, fast=True):
    """what key_agreement.shared_secrets returns: (uint8[n_pairs, 32], uint8[n_pairs])"""
    sks, peer_pks = [bytes(s) for s in sks], [bytes(p) for p in peer_pks]
    if pairs is None:
        pairs = [(a, b) for a in range(len(sks)) for b in range(len(peer_pks))]
    own = [public_key(s, fast) for s in sks]
    res = [shared(sks[a], peer_pks[b], own[a], fast) for a, b in pairs]
    out = np.frombuffer(b"".join(r[0] for r in res), np.uint8).reshape(-1, 32).copy()
    return out, np.array([r[1] for r in res], dtype=np.uint8)


def rand_keys(rng, n):
    """n secret keys as uint8[n, 32]: any 32 bytes (reduced mod l by the library)"""
    return rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
