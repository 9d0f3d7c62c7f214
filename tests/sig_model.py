"""Python model of the signatures of rofl_sig_sign / rofl_sig_verify (include/rofl_zk.h), independent of the library; shared by
test_signatures_host.py and test_gpu_signatures.py:
  h(m) = SHAKE256("rofl-zk/sig/v1/m" || u64le(len m) || m)[0 .. 32);
  a = key mod l (!= 0), A = encode(a B);
  k = int_le(SHAKE256("rofl-zk/sig/v1/k" || canonical32(a) || h)[0 .. 64)) mod l, R = encode(k B);
  c = int_le(SHAKE256("rofl-zk/sig/v1/c" || R || A || h)[0 .. 64)) mod l, s = k + c a mod l; signature = R || canonical32(s);
  verdict 2: the key is no canonical encoding or the identity, or s >= l; 0: encode(s B - c decode(A)) == R; 1: anything else;
and of the two message layouts of secret_sharing.commitment_message / view_message.
The point arithmetic is tests/golden/pyref.py as dh_model.py uses it; fast=True takes products from the oracle's MSM instead -- the check
is then the two-term product encode(s B + (l - c) A) (same bytes, ~100x faster)."""
import hashlib

import numpy as np

import dh_model as D

pyref = D.pyref
L = D.L
DOM_M, DOM_K, DOM_C = b"rofl-zk/sig/v1/m", b"rofl-zk/sig/v1/k", b"rofl-zk/sig/v1/c"
assert len(DOM_M) == len(DOM_K) == len(DOM_C) == 16
# message lengths around the digest's block ends (24 bytes of prefix, a rate of 136): 112 ends the first block and 248 the second exactly,
# 111 / 247 end on the rate's last byte (suffix and final bit in one byte), 0 is the empty message
LENS = (0, 1, 111, 112, 113, 247, 248, 249)


def digest(m):
    m = bytes(m)
    return hashlib.shake_256(DOM_M + len(m).to_bytes(8, "little") + m).digest(32)


def _wide(data):
    return int.from_bytes(hashlib.shake_256(data).digest(64), "little") % L


def _base_mul(k, fast):
    """encode(k B), k = 0 included (the identity encoding)"""
    return bytes(32) if k % L == 0 else D._product(k % L, D.BASE_ENC, fast)


def public_key(sk, fast=True):
    return D.public_key(sk, fast)


def nonce(sk, h):
    return _wide(DOM_K + D.sk_int(sk).to_bytes(32, "little") + h)


def challenge(R, A, h):
    return _wide(DOM_C + bytes(R) + bytes(A) + bytes(h))


def sign(sk, m, fast=True, pk=None):
    """-> 64 bytes"""
    a = D.sk_int(sk)
    assert a != 0, "a signing key is not 0 mod l"
    h = digest(m)
    A = bytes(pk) if pk is not None else public_key(sk, fast)
    k = nonce(sk, h)
    R = _base_mul(k, fast)
    s = (k + challenge(R, A, h) * a) % L
    return R + s.to_bytes(32, "little")


def verdict(pk, m, sig, fast=True):
    pk, sig = bytes(pk), bytes(sig)
    assert len(pk) == 32 and len(sig) == 64
    R, s = sig[:32], int.from_bytes(sig[32:], "little")
    P = pyref.ristretto_decode(pk)
    if P is None or pk == bytes(32) or s >= L:
        return 2
    c = challenge(R, pk, digest(m))
    if fast:
        import orc
        sc = np.frombuffer(s.to_bytes(32, "little") + ((L - c) % L).to_bytes(32, "little"), np.uint8)
        pts = np.frombuffer(D.BASE_ENC + pk, np.uint8)
        got = orc.msm(sc, pts).tobytes()
    else:
        got = pyref.ristretto_encode(pyref.pt_add(pyref.pt_mul(s, pyref.BASE), pyref.pt_mul((L - c) % L, P)))
    return 0 if got == R else 1


def _refs(refs, n_keys, n_msgs):
    if refs is None:
        assert n_keys == n_msgs
        return [(i, i) for i in range(n_keys)]
    return [(int(a), int(b)) for a, b in refs]


def sign_batch(sks, msgs, refs=None, fast=True):
    """what signatures.sign returns: uint8[n, 64]"""
    sks = [bytes(s) for s in np.asarray(sks, np.uint8).reshape(-1, 32)]
    pks = [public_key(s, fast) for s in sks]
    out = [sign(sks[a], msgs[b], fast, pks[a]) for a, b in _refs(refs, len(sks), len(msgs))]
    return np.frombuffer(b"".join(out), np.uint8).reshape(-1, 64).copy()


def verify_batch(pks, msgs, sigs, refs=None, fast=True):
    """what signatures.verify returns: uint8[n]"""
    pks = [bytes(p) for p in np.asarray(pks, np.uint8).reshape(-1, 32)]
    sigs = np.asarray(sigs, np.uint8).reshape(-1, 64)
    return np.array([verdict(pks[a], msgs[b], sigs[i], fast) for i, (a, b) in enumerate(_refs(refs, len(pks), len(msgs)))], dtype=np.uint8)


def pack(msgs):
    """(uint8[total], uint64[n + 1]) as the C ABI takes the messages"""
    msgs = [bytes(m) for m in msgs]
    off = np.zeros(len(msgs) + 1, np.uint64)
    for j, m in enumerate(msgs):
        off[j + 1] = off[j] + np.uint64(len(m))
    return np.frombuffer(b"".join(msgs) or b"\0", np.uint8)[:int(off[-1])].copy(), off


def commitment_message(round_no, dealer, kind, commitments):
    c = np.asarray(commitments, np.uint8)
    assert c.ndim == 2 and c.shape[1] == 32 and kind in (0, 1)
    return (b"rofl-zk/vss/v1\0\0" + int(round_no).to_bytes(8, "little") + int(dealer).to_bytes(4, "little") + bytes([kind])
            + c.shape[0].to_bytes(4, "little") + c.tobytes())


def view_message(round_no, sigs_by_dealer):
    out = b"rofl-zk/view/v1\0" + int(round_no).to_bytes(8, "little") + len(sigs_by_dealer).to_bytes(4, "little")
    for d in sorted(sigs_by_dealer):
        s = np.asarray(sigs_by_dealer[d], np.uint8)
        assert s.shape == (2, 64)
        out += int(d).to_bytes(4, "little") + s[0].tobytes() + s[1].tobytes()
    return out


def misaligned_messages(rng, lens=LENS):
    """(messages, index of each tested length): fillers of 1 .. 7 bytes put every tested message at a start that is no multiple of 8, all
    seven misalignments among them"""
    msgs, where, off = [], [], 0
    for q, n in enumerate(lens):
        want = (1, 3, 5, 7, 2, 4, 6)[q % 7]
        fill = (want - off) % 8
        if fill:
            msgs.append(rng.bytes(fill)); off += fill
        assert off % 8 == want
        where.append(len(msgs))
        msgs.append(rng.bytes(n)); off += n
    return msgs, where


def verdict_cases(pks, msgs, sigs):
    """Every verdict class from five honest (key, message, signature) triples, good and bad mixed, one signature per key and message
    (refs = None) -> (keys uint8[n, 32], messages, sigs uint8[n, 64], expected verdicts uint8[n]).  The expectations are written down here,
    not computed: the callers hold the model to them as well."""
    import ristretto_corpus as RC
    ell_bytes = lambda v: np.frombuffer(int(v).to_bytes(32, "little"), np.uint8)      # noqa: E731
    reps = RC.representatives()
    noncanon_R = reps[1]
    assert noncanon_R[0] == "p+3" and pyref.ristretto_decode(noncanon_R[1]) is None and len(msgs[0]) > 11
    # a key with one bit flipped that is still a valid encoding: the equation fails, nothing is refused
    flipped = None
    for bit in range(1, 250):
        k = bytearray(bytes(pks[0])); k[bit >> 3] ^= 1 << (bit & 7)
        if pyref.ristretto_decode(bytes(k)) is not None and bytes(k) != bytes(32):
            flipped = np.frombuffer(bytes(k), np.uint8); break
    assert flipped is not None
    cases = []

    def add(key, msg, sig, want):
        cases.append((np.asarray(key, np.uint8).copy(), bytes(msg), np.asarray(sig, np.uint8).copy(), want))
    add(pks[0], msgs[0], sigs[0], 0)
    s = sigs[0].copy(); s[3] ^= 0x20; add(pks[0], msgs[0], s, 1)                   # a bit of R
    s = sigs[0].copy(); s[32 + 7] ^= 0x01; add(pks[0], msgs[0], s, 1)              # a bit of s
    m = bytearray(msgs[0]); m[11] ^= 0x80; add(pks[0], m, sigs[0], 1)              # a bit of the message
    add(flipped, msgs[0], sigs[0], 1)                                              # a bit of the key
    add(pks[1], msgs[1], sigs[1], 0)
    sv = int.from_bytes(sigs[1, 32:].tobytes(), "little")
    s = sigs[1].copy(); s[32:] = ell_bytes(sv + L); add(pks[1], msgs[1], s, 2)     # s + l: the same scalar, not canonical
    for rep in reps:                                                               # every way a key is no canonical encoding
        add(RC.row(rep), msgs[2], sigs[2], 2)
        add(pks[2], msgs[2], sigs[2], 0)                                           # ... and its neighbour is left alone
    add(np.zeros(32, np.uint8), msgs[3], sigs[3], 2)                               # the identity key
    add(pks[3], msgs[3], sigs[3], 0)
    s = sigs[4].copy(); s[:32] = RC.row(noncanon_R); add(pks[4], msgs[4], s, 1)    # an R that is no canonical encoding: simply 1
    s = sigs[4].copy(); s[:32] = 0; add(pks[4], msgs[4], s, 1)                     # R = the identity encoding
    s = sigs[4].copy(); s[32:] = 0; add(pks[4], msgs[4], s, 1)                     # s = 0
    add(RC.row(reps[0]), msgs[4], np.full(64, 0xff, np.uint8), 2)                  # malformed wins over a failing equation
    add(pks[4], msgs[4], sigs[4], 0)
    return np.stack([c[0] for c in cases]), [c[1] for c in cases], np.stack([c[2] for c in cases]), np.array([c[3] for c in cases], np.uint8)
