"""X25519 of RFC 7748 section 5 on Python integers, independent of the library: what rofl_x25519_* and rofl_dbg_host_x25519 are held to.
shared(k, u) -> (32 bytes, status): status 2 and zeros for an all-zero result (section 6.1), else 0; CORPUS_U / CORPUS_K are the edge inputs
the host and the device tests share, NONCANONICAL_U every u in p .. 2^255 - 1 with and without bit 255."""
import numpy as np

P = 2**255 - 19
A24 = 121665


def x25519(k, u):
    k = int.from_bytes(k, "little") & ~7 & (2**255 - 1) | 2**254
    x1 = (int.from_bytes(u, "little") & (2**255 - 1)) % P
    x2, z2, x3, z3, swap = 1, 0, x1, 1, 0
    for t in range(254, -1, -1):
        bit = (k >> t) & 1
        if swap ^ bit:
            x2, x3, z2, z3 = x3, x2, z3, z2
        swap = bit
        A, B, C, D = x2 + z2, x2 - z2, x3 + z3, x3 - z3
        DA, CB, AA, BB = D * A % P, C * B % P, A * A % P, B * B % P
        E = AA - BB
        x3, z3 = (DA + CB) ** 2 % P, x1 * (DA - CB) ** 2 % P
        x2, z2 = AA * BB % P, E * (AA + A24 * E) % P
    if swap:
        x2, z2 = x3, z3
    return (x2 * pow(z2, P - 2, P) % P).to_bytes(32, "little")


def public_key(k):
    return x25519(k, (9).to_bytes(32, "little"))


def shared(k, u):
    out = x25519(k, u)
    return out, 0 if any(out) else 2


def _le(v):
    return int(v).to_bytes(32, "little")


ORDER8 = [bytes.fromhex("e0eb7a7c3b41b8ae1656e3faf19fc46ada098deb9c32b1fd866205165f49b800"),
          bytes.fromhex("5f9c95bca3508c24b1d0b1559c83ef5b04445cc4581c8e86d8224eddd09f1157")]
SMALL_ORDER = [_le(0), _le(1), _le(P - 1), _le(P), _le(P + 1)] + ORDER8      # every one gives zeros, with or without bit 255
_rng = np.random.default_rng(20261201)
CORPUS_U = (SMALL_ORDER + [bytes(s[:31]) + bytes([s[31] | 0x80]) for s in SMALL_ORDER]
            + [_le(2**255 - 1), _le(9 + 2**255), _le(P - 2), _le(2)] + [_rng.bytes(32) for _ in range(64)])
# every non-canonical u: p + i, i = 0 .. 18, then the same 19 under bit 255.  Entry j is u = j % 19 once masked and reduced: zeros for 0 and 1 only
NONCANONICAL_U = [_le(P + i) for i in range(19)] + [_le(P + i + 2**255) for i in range(19)]
CORPUS_K = [bytes(32), b"\xff" * 32, b"\x55" * 32, b"\xaa" * 32]
