"""Python model of the blinding streams of rofl_blinding_vecs (include/rofl_zk.h), shared by test_blinding_host.py and test_gpu_blinding.py:
scalar k of a seed's stream = int_le(SHAKE256("rofl-zk/blind/v1" || seed || u64le(k >> 1))[64 (k & 1) .. + 64]) mod l."""
import hashlib
import struct

import numpy as np

L = 2 ** 252 + 27742317777372353535851937790883648493


def stream_int(seed, k):
    x = hashlib.shake_256(b"rofl-zk/blind/v1" + bytes(seed) + struct.pack("<Q", k >> 1)).digest(128)[64 * (k & 1):64 * (k & 1) + 64]
    return int.from_bytes(x, "little") % L


def to_arr(ints):
    """canonical 32-byte little-endian scalars -> uint8[len, 32]"""
    return np.frombuffer(b"".join((v % L).to_bytes(32, "little") for v in ints), dtype=np.uint8).reshape(-1, 32)


def to_ints(arr):
    a = np.ascontiguousarray(arr, dtype=np.uint8).reshape(-1, 32)
    return [int.from_bytes(r.tobytes(), "little") for r in a]


def combine(terms, d, first=0):
    """out[k] = sum_t sign_t * stream(seed_t)[first + k] mod l -> uint8[d, 32]"""
    return to_arr([sum(sign * stream_int(seed, first + k) for seed, sign in terms) for k in range(d)])


def vec_seed(seed, i):
    return hashlib.sha3_256(b"rofl-zk/blind/v1/vec" + bytes(seed) + struct.pack("<I", i)).digest()


def round_seed(secret, round_no):
    return hashlib.sha3_256(b"rofl-zk/blind/v1/round" + bytes(secret) + struct.pack("<Q", round_no)).digest()
