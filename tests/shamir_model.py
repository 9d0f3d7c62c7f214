"""Python model of the secret sharing of rofl_shamir_share / rofl_shamir_reconstruct and of the self-mask seed (include/rofl_zk.h), in Python
integers and hashlib, independent of the library; shared by test_secret_sharing_host.py and test_gpu_secret_sharing.py:
  secret = 32 little-endian bytes reduced mod l; f(X) = s + sum_{k=1..t-1} a_k X^k mod l,
  a_k = int_le(SHAKE256("rofl-zk/share/v1" || c || u64le((k - 1) >> 1))[64 ((k - 1) & 1) .. + 64]) mod l for the coefficient seed c;
  the share for the point x is canonical32(f(x)); s = sum_j lambda_j share_j, lambda_j = prod_{m != j} x_m (x_m - x_j)^-1 mod l;
  self-mask seed = SHA3-256("rofl-zk/blind/v1/self" || canonical32(b mod l) || u64le(round_no))."""
import hashlib
import struct

import numpy as np

from blind_model import L, to_arr, to_ints

LABEL = b"rofl-zk/share/v1"


def coefficients(seed, t):
    """[a_1, ..., a_{t-1}]"""
    out = []
    for k in range(1, t):
        blk = hashlib.shake_256(LABEL + bytes(seed) + struct.pack("<Q", (k - 1) >> 1)).digest(128)
        out.append(int.from_bytes(blk[64 * ((k - 1) & 1):64 * ((k - 1) & 1) + 64], "little") % L)
    return out


def share_ints(secret, seed, t, xs):
    s = int.from_bytes(bytes(secret), "little") % L
    a = [s] + coefficients(seed, t)
    return [sum(c * pow(int(x), k, L) for k, c in enumerate(a)) % L for x in xs]


def share(secrets, seeds, t, n_shares, xs=None):
    """-> uint8[n_secrets, n_shares, 32]"""
    xs = range(1, n_shares + 1) if xs is None else [int(x) for x in xs]
    assert len(xs) == n_shares
    rows = [to_arr(share_ints(sec, sd, t, xs)) for sec, sd in zip(secrets, seeds)]
    return np.stack(rows) if rows else np.zeros((0, n_shares, 32), np.uint8)


def weights(xs):
    xs = [int(x) for x in xs]
    assert all(xs) and len(set(xs)) == len(xs)
    lam = []
    for j, xj in enumerate(xs):
        num = den = 1
        for m, xm in enumerate(xs):
            if m != j:
                num, den = num * xm % L, den * (xm - xj) % L
        lam.append(num * pow(den, L - 2, L) % L)
    return lam


def reconstruct(xs, shares):
    """shares uint8[n_secrets, len(xs), 32] -> uint8[n_secrets, 32]"""
    lam = weights(xs)
    shares = np.asarray(shares, np.uint8).reshape(-1, len(lam), 32)
    return to_arr([sum(w * v for w, v in zip(lam, to_ints(row))) % L for row in shares])


def self_mask_seed(b, round_no):
    canon = (int.from_bytes(bytes(b), "little") % L).to_bytes(32, "little")
    return hashlib.sha3_256(b"rofl-zk/blind/v1/self" + canon + struct.pack("<Q", round_no)).digest()
