"""Python model of the complaint proofs of rofl_dleq_prove / rofl_dleq_verify (include/rofl_zk.h), independent of the library; shared by
test_dleq_host.py and test_gpu_dleq.py:
  A = encode(x B), P the peer's key, S = encode(x decode(P)), ctx 32 bytes;
  k = int_le(SHAKE256("rofl-zk/dleq/v1k" || canonical32(x) || P || ctx)[0 .. 64)) mod l, T1 = encode(k B), T2 = encode(k decode(P));
  c = int_le(SHAKE256("rofl-zk/dleq/v1c" || A || P || S || T1 || T2 || ctx)[0 .. 64)) mod l, s = k + c x mod l; proof = c || s;
  verdict 2: A or P is no canonical encoding or the identity, S likewise, c >= l or s >= l; 0: c is the challenge recomputed from
  T1' = encode(s B - c A), T2' = encode(s P - c S); 1: anything else.  Verdict 0 comes with the rofl_dh_shared secret of the pair;
and of the layouts of secret_sharing.bundle_message / complaint_context, and of judge_complaints' ruling.
The point arithmetic is tests/golden/pyref.py as dh_model.py uses it; fast=True takes the products from the oracle's MSM instead (same
bytes, ~100x faster)."""
import hashlib

import numpy as np

import dh_model as D

pyref = D.pyref
L = D.L
DOM_K, DOM_C = b"rofl-zk/dleq/v1k", b"rofl-zk/dleq/v1c"
assert len(DOM_K) == len(DOM_C) == 16
ZERO = bytes(32)


def _wide(data):
    return int.from_bytes(hashlib.shake_256(data).digest(64), "little") % L


def _b(v):
    return int(v).to_bytes(32, "little")


def lin(terms, fast=True):
    """encode(sum k_i decode(enc_i)) for valid encodings (the identity included) and any k_i"""
    terms = [(k % L, bytes(e)) for k, e in terms]
    if fast:
        import orc
        return orc.msm(np.frombuffer(b"".join(_b(k) for k, _ in terms), np.uint8), np.frombuffer(b"".join(e for _, e in terms), np.uint8)).tobytes()
    acc = pyref.IDENT
    for k, e in terms:
        acc = pyref.pt_add(acc, pyref.pt_mul(k, pyref.ristretto_decode(e)))
    return pyref.ristretto_encode(acc)


def refused(enc):
    """k_dh_decode's status word: 1 not a canonical encoding, 2 the identity, 0 a usable key"""
    enc = bytes(enc)
    if pyref.ristretto_decode(enc) is None:
        return 1
    return 2 if enc == ZERO else 0


def nonce(sk, P, ctx):
    return _wide(DOM_K + _b(D.sk_int(sk)) + bytes(P) + bytes(ctx))


def challenge(A, P, S, T1, T2, ctx):
    data = DOM_C + bytes(A) + bytes(P) + bytes(S) + bytes(T1) + bytes(T2) + bytes(ctx)
    assert len(data) == 208
    return _wide(data)


def prove(sk, P, ctx, fast=True, pk=None):
    """-> (reveal 32 bytes, proof 64 bytes, status)"""
    P, ctx = bytes(P), bytes(ctx)
    assert len(P) == 32 and len(ctx) == 32
    st = refused(P)
    if st:
        return ZERO, bytes(64), st
    x = D.sk_int(sk)
    assert x != 0, "a key is not 0 mod l"
    A = bytes(pk) if pk is not None else D.public_key(sk, fast)
    k = nonce(sk, P, ctx)
    S, T1, T2 = lin([(x, P)], fast), lin([(k, D.BASE_ENC)], fast), lin([(k, P)], fast)
    c = challenge(A, P, S, T1, T2, ctx)
    return S, _b(c) + _b((k + c * x) % L), 0


def verify(A, P, ctx, S, proof, fast=True):
    """-> (verdict, shared 32 bytes)"""
    A, P, ctx, S, proof = bytes(A), bytes(P), bytes(ctx), bytes(S), bytes(proof)
    assert len(A) == len(P) == len(ctx) == len(S) == 32 and len(proof) == 64
    c, s = int.from_bytes(proof[:32], "little"), int.from_bytes(proof[32:], "little")
    if refused(A) or refused(P) or refused(S) or c >= L or s >= L:
        return 2, ZERO
    T1 = lin([(s, D.BASE_ENC), (L - c, A)], fast)
    T2 = lin([(s, P), (L - c, S)], fast)
    if challenge(A, P, S, T1, T2, ctx) != c:
        return 1, ZERO
    lo, hi = (A, P) if A <= P else (P, A)
    return 0, hashlib.shake_256(D.DOM + S + lo + hi).digest(32)


def _pairs(pairs, n_own, n_peer):
    return [(a, b) for a in range(n_own) for b in range(n_peer)] if pairs is None else [(int(a), int(b)) for a, b in pairs]


def prove_batch(sks, peer_pks, ctxs, pairs=None, fast=True):
    """what dleq.prove returns: (uint8[n, 32], uint8[n, 64], uint8[n])"""
    sks = [bytes(s) for s in np.asarray(sks, np.uint8).reshape(-1, 32)]
    pks = [bytes(p) for p in np.asarray(peer_pks, np.uint8).reshape(-1, 32)]
    ctxs = np.asarray(ctxs, np.uint8).reshape(-1, 32)
    own = [D.public_key(s, fast) for s in sks]
    res = [prove(sks[a], pks[b], ctxs[i], fast, own[a]) for i, (a, b) in enumerate(_pairs(pairs, len(sks), len(pks)))]
    return (np.frombuffer(b"".join(r[0] for r in res), np.uint8).reshape(-1, 32).copy(), np.frombuffer(b"".join(r[1] for r in res), np.uint8).reshape(-1, 64).copy(),
            np.array([r[2] for r in res], np.uint8))


def verify_batch(own_pks, peer_pks, ctxs, reveals, proofs, pairs=None, fast=True):
    """what dleq.verify returns: (uint8[n], uint8[n, 32])"""
    own = [bytes(p) for p in np.asarray(own_pks, np.uint8).reshape(-1, 32)]
    pks = [bytes(p) for p in np.asarray(peer_pks, np.uint8).reshape(-1, 32)]
    ctxs, reveals, proofs = np.asarray(ctxs, np.uint8).reshape(-1, 32), np.asarray(reveals, np.uint8).reshape(-1, 32), np.asarray(proofs, np.uint8).reshape(-1, 64)
    res = [verify(own[a], pks[b], ctxs[i], reveals[i], proofs[i], fast) for i, (a, b) in enumerate(_pairs(pairs, len(own), len(pks)))]
    return np.array([r[0] for r in res], np.uint8), np.frombuffer(b"".join(r[1] for r in res), np.uint8).reshape(-1, 32).copy()


def bundle_message(round_no, sender, recipient, record):
    record = bytes(record) if isinstance(record, (bytes, bytearray)) else np.asarray(record, np.uint8).tobytes()
    assert len(record) == 80
    return b"rofl-zk/sealed/1" + int(round_no).to_bytes(8, "little") + int(sender).to_bytes(4, "little") + int(recipient).to_bytes(4, "little") + record


def complaint_context(round_no, complainant, dealer):
    return hashlib.sha3_256(b"rofl-zk/complain" + int(round_no).to_bytes(8, "little") + int(complainant).to_bytes(4, "little") + int(dealer).to_bytes(4, "little")).digest()


def flip_that_still_decodes(enc, avoid=()):
    """enc with one bit flipped so that it is still a valid non-identity encoding (another point)"""
    for bit in range(1, 250):
        k = bytearray(bytes(enc)); k[bit >> 3] ^= 1 << (bit & 7)
        if refused(bytes(k)) == 0 and bytes(k) not in avoid:
            return bytes(k)
    raise AssertionError("no such bit")


def verdict_cases(sks, pks, peer, ctxs, fast=True):
    """Every verdict class from six honest proofs of the keys sks (public keys pks) against ONE peer key, good proofs between the bad ones
    -> (own keys uint8[n, 32], peer keys uint8[n, 32], ctxs, reveals, proofs, expected verdicts uint8[n]) for a call with pairs (i, i).
    The expectations are written down here, not computed: the callers hold the model to them as well."""
    peer = bytes(peer)
    honest = [prove(sks[i], peer, ctxs[i], fast, bytes(pks[i])) for i in range(6)]
    assert all(h[2] == 0 for h in honest)
    cases = []

    def add(A, P, ctx, S, proof, want):
        cases.append((bytes(A), bytes(P), bytes(ctx), bytes(S), bytes(proof), want))

    def good(i):
        add(pks[i], peer, ctxs[i], honest[i][0], honest[i][1], 0)

    def flip(b, at, mask):
        b = bytearray(b); b[at] ^= mask
        return bytes(b)
    S0, pf0 = honest[0][:2]
    good(0)
    add(pks[0], peer, ctxs[0], S0, flip(pf0, 5, 0x10), 1)                                       # a bit of c
    good(1)
    add(pks[0], peer, ctxs[0], S0, flip(pf0, 32 + 9, 0x02), 1)                                  # a bit of s
    add(pks[0], peer, ctxs[0], flip_that_still_decodes(S0), pf0, 1)                             # a bit of S that still decodes
    good(2)
    add(pks[0], peer, flip(ctxs[0], 31, 0x80), S0, pf0, 1)                                      # a bit of ctx
    add(pks[0], peer, ctxs[0], *prove(sks[0], peer, ctxs[1], fast, bytes(pks[0]))[:2], 1)       # a proof for another ctx
    good(3)
    add(peer, pks[0], ctxs[0], S0, pf0, 1)                                                      # A and P swapped
    add(pks[0], peer, ctxs[0], *prove(sks[1], peer, ctxs[0], fast, bytes(pks[1]))[:2], 1)       # an honest proof by another key, with its own S', against A
    good(4)
    c, s = int.from_bytes(pf0[:32], "little"), int.from_bytes(pf0[32:], "little")
    assert c + L < 2 ** 256 and s + L < 2 ** 256
    add(pks[0], peer, ctxs[0], S0, _b(c + L) + pf0[32:], 2)                                     # c + l: the same scalar, not canonical
    add(pks[0], peer, ctxs[0], S0, pf0[:32] + _b(s + L), 2)                                     # s + l
    good(5)
    add(pks[0], peer, ctxs[0], ZERO, pf0, 2)                                                    # S = the identity
    add(ZERO, peer, ctxs[0], S0, pf0, 2)                                                        # A = the identity
    add(pks[0], ZERO, ctxs[0], S0, pf0, 2)                                                      # P = the identity
    add(ZERO, peer, ctxs[0], S0, b"\xff" * 64, 2)                                               # malformed wins over a failing equation
    good(0)
    col = lambda j, w: np.frombuffer(b"".join(c[j] for c in cases), np.uint8).reshape(-1, w).copy()      # noqa: E731
    return col(0, 32), col(1, 32), col(2, 32), col(3, 32), col(4, 64), np.array([c[5] for c in cases], np.uint8)


# ---- the round of test_gpu_aead.py with five complaints: six clients, threshold 4, round 7
N, THRESHOLD, ROUND_NO = 6, 4, 7
# (complainant, dealer) and the (at_fault, reason) judge_complaints must return, in this order
COMPLAINTS = ((3, 5), (1, 4), (0, 2), (1, 3), (2, 1))
RULINGS = [(5, 0), (4, 1), (0, 2), (1, 3), (2, 4)]


def deal_with_faults(key_sh):
    """the key shares dealer 5 really seals: the one for client 3 with one bit flipped"""
    bad = np.array(key_sh, np.uint8, copy=True)
    bad[5, 3, 0] ^= 0x01
    return bad


def alter_before_signing(sent):
    """dealer 4 alters the ciphertext of its record for client 1 and then signs it"""
    sent = np.array(sent, np.uint8, copy=True)
    sent[4, 1, 10] ^= 0x04
    return sent


def round_complaints(sent, sigs, reveal_and_proof):
    """The five complaints from the records sent[dealer, recipient] and their signatures sigs[dealer, recipient];
    reveal_and_proof(complainant, dealer, round_no) -> (reveal, proof) bound to complaint_context(round_no, complainant, dealer).
      0  dealer 5 dealt client 3 a key share with one bit flipped before sealing          -> (5, 0)
      1  dealer 4 signed a record for client 1 whose ciphertext it had altered            -> (4, 1)
      2  client 0 complains about dealer 2's clean record                                 -> (0, 2)
      3  client 1 complains about dealer 3 with a proof made for another ctx              -> (1, 3)
      4  client 2 complains about dealer 1 with another record's signature                -> (2, 4)"""
    out = []
    for i, (c, d) in enumerate(COMPLAINTS):
        reveal, proof = reveal_and_proof(c, d, ROUND_NO + 1 if i == 3 else ROUND_NO)
        out.append((c, d, sent[d, c].copy(), (sigs[d, 0] if i == 4 else sigs[d, c]).copy(), reveal, proof))
    return out


def judge(sig_ok, proof_verdict, opens, shares_ok, complainant, dealer):
    """the ruling of judge_complaints for one complaint, from what the four calls said"""
    if not sig_ok:
        return complainant, 4
    if proof_verdict:
        return complainant, 3
    if not opens:
        return dealer, 1
    if not shares_ok:
        return dealer, 0
    return complainant, 2
