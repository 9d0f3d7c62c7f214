"""The cancellation corpus (tests/cancel_corpus.py) has teeth -- shown on the CPU with the oracle, the pure-Python Merlin and libsodium:
for every construction (a) the untampered input, duplicates included, is accepted by the oracle, (b) the tampered one is rejected by the
oracle, and (c) the residual points of the tampered members, computed from the verification equations, are each NOT the identity while
their unweighted sum IS: a batch verifier that gave these members one weight would accept them.  With that, what
tests/test_gpu_batch_cancellation.py feeds the GPU verifiers is not just two independent tampers."""
import os
import sys

import numpy as np
import pytest

import cancel_corpus as K
import orc

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import pyref  # noqa: E402
import sodium_bp as S  # noqa: E402

L = K.ELL
ID = bytes(32)
B = pyref.ristretto_encode(pyref.BASE)
BB = pyref.ristretto_encode(pyref.b_blinding())
needs_sodium = pytest.mark.skipif(S.so is None, reason="libsodium not available")


def _sc(x):
    return np.frombuffer((x % L).to_bytes(32, "little"), np.uint8)


def _msm(scalars, points):
    return orc.msm(np.stack([_sc(s) for s in scalars]), np.stack([np.frombuffer(bytes(p), np.uint8) for p in points])).tobytes()


def _sum(points):
    return _msm([1] * len(points), points) if points else ID


# ---------------------------------------------------------------- Sigma-proofs
_challenges = {}


def _challenge(kind, d, i, pf, cm):
    """c of element i (the responses are not part of the transcript: one value per honest element, whatever was done to its Z)"""
    if (kind, d, i) not in _challenges:
        t = pyref.Transcript(K.SIGMA_LABEL[kind])
        t.append_message(b"dom-sep", b"randomness proof v1")
        if kind == 0:
            t.append_message(b"C", cm[:64]); t.append_message(b"C_prime", pf[:64])
        else:
            w = 64 if kind == 1 else 32
            t.append_message(b"C_eg", cm[:w]); t.append_message(b"C_ped", cm[w:w + 32])
            t.append_message(b"C_prime_eg", pf[:w]); t.append_message(b"C_prime_ped", pf[w:w + 32])
        _challenges[(kind, d, i)] = t.challenge_scalar(b"c")
    return _challenges[(kind, d, i)]


def sigma_residuals(kind, d, i, pf, cm):
    """{equation: residual point} of one element (the equations above k_sigma_vprep):
    e1: c L + L' - Z_m B - Z_r1 Bb    e2 (kinds 0, 1): c R + R' - Z_r1 B    e3 (kinds 1, 2): c Csq + Csq' - Z_m L - Z_r2 Bb"""
    pf, cm = bytes(pf), bytes(cm)
    npts = K.SIGMA[kind][0]
    c = _challenge(kind, d, i, pf, cm)
    z = [int.from_bytes(pf[32 * npts + 32 * k:32 * npts + 32 * k + 32], "little") for k in range(3 if kind else 2)]
    Lc, Lp = cm[:32], pf[:32]
    out = {1: _msm([c, 1, -z[0], -z[1]], [Lc, Lp, B, BB])}
    if kind != 2:
        out[2] = _msm([c, 1, -z[1]], [cm[32:64], pf[32:64], B])
    if kind != 0:
        o = 64 if kind == 1 else 32
        out[3] = _msm([c, 1, -z[0], -z[2]], [cm[o:o + 32], pf[o:o + 32], Lc, BB])
    return out


@pytest.mark.parametrize("d", [2, 257, 300])
@pytest.mark.parametrize("kind", [0, 1, 2])
def test_sigma_constructions_cancel_unweighted_and_are_rejected(kind, d):
    pr, cm = K.sigma_honest(kind, d)
    assert orc.sigma_verify(kind, pr, cm) == (0, True)                                        # (a)
    cases = K.sigma_cases(kind, d)
    assert cases
    for name, edits in cases:
        elems = sorted({e for e, _, _ in edits})
        for i in elems:      # the residual function itself: an honest element leaves none
            assert all(r == ID for r in sigma_residuals(kind, d, i, pr[i], cm[i]).values()), (name, i)
        for delta in K.DELTAS:
            t = K.sigma_apply(kind, pr, edits, delta)
            assert (t != pr).any(axis=1).sum() == len(elems)
            assert orc.sigma_verify(kind, t, cm) == (0, False), (name, delta)                 # (b)
            hit = {}      # equation -> the residuals the construction leaves in it
            for e, field, _ in edits:
                for q in K.sigma_equations(kind, field):
                    hit.setdefault(q, set()).add(e)
            res = {i: sigma_residuals(kind, d, i, t[i], cm[i]) for i in elems}
            allr = []
            for i in elems:
                for q, r in res[i].items():
                    if i in hit.get(q, ()):
                        assert r != ID, (name, delta, i, q)                                   # (c) each alone is an error ...
                        allr.append(r)
                    else:
                        assert r == ID, (name, delta, i, q)
            assert len(allr) >= 2 and _sum(allr) == ID, (name, delta)                         # ... their plain sum is none
            if not name.startswith("S4"):      # S1, S2, S3, S5 cancel inside every equation; S4 across e1 and e3
                for q, es in hit.items():
                    assert _sum([res[i][q] for i in es]) == ID, (name, delta, q)


# ---------------------------------------------------------------- range proofs
def range_residuals(proof, V, n, label=b"RangeProof"):
    """sodium_bp.verify_single restated to return what is left of its two equations, (lhs - rhs of the t(x) check, want - P of the
    inner-product check): (identity, identity) for a proof that verifies.  The same steps, libsodium group operations, Python integers."""
    proof = bytes(proof); V = [bytes(v) for v in V]
    m = len(V)
    ne = (len(proof) - 7 * 32) // 32
    lg = (ne - 2) // 2
    w32 = [proof[32 * i:32 * i + 32] for i in range(len(proof) // 32)]
    A, S_, T1, T2 = w32[0:4]
    assert all(S._canonical(x) for x in w32[4:7] + w32[-2:])
    t_x, t_x_bl, e_bl = (S._sc(x) for x in w32[4:7])
    Ls = [w32[7 + 2 * k] for k in range(lg)]; Rs = [w32[8 + 2 * k] for k in range(lg)]
    a, b = S._sc(w32[-2]), S._sc(w32[-1])
    N = n * m
    assert N == 1 << lg and all(S.is_valid(p) for p in [A, S_, T1, T2] + Ls + Rs + V)
    t = S._transcript_start(label, n, m, V)
    t.append_message(b"A", A); t.append_message(b"S", S_)
    y = t.challenge_scalar(b"y"); z = t.challenge_scalar(b"z")
    t.append_message(b"T_1", T1); t.append_message(b"T_2", T2)
    x = t.challenge_scalar(b"x")
    for lab, v in ((b"t_x", t_x), (b"t_x_blinding", t_x_bl), (b"e_blinding", e_bl)):
        t.append_message(lab, v.to_bytes(32, "little"))
    w = t.challenge_scalar(b"w")
    t.append_message(b"dom-sep", b"ipp v1"); t.append_u64(b"n", N)
    us = []
    for k in range(lg):
        t.append_message(b"L", Ls[k]); t.append_message(b"R", Rs[k])
        us.append(t.challenge_scalar(b"u"))
    zz = z * z % L
    sum_y = sum(pow(y, i, L) for i in range(N)) % L
    sum_2 = (pow(2, n, L) - 1) % L
    sum_z = sum(pow(z, j, L) for j in range(m)) % L
    delta = ((z - zz) * sum_y - zz * z % L * sum_2 % L * sum_z) % L
    lhs = S.padd(S.smul(t_x, S.B), S.smul(t_x_bl, S.B_BLINDING))
    rhs = S.padd(S.padd(S.msm([zz * pow(z, j, L) % L for j in range(m)], V), S.smul(delta, S.B)), S.padd(S.smul(x, T1), S.smul(x * x % L, T2)))
    G, H = S.gens(n, m)
    yinv = S._inv(y)
    P = S.padd(A, S.smul(x, S_))
    P = S.padd(P, S.msm([(-z) % L] * N, G))
    hs = [(z + pow(yinv, i, L) * (zz * pow(z, i // n, L) % L) % L * pow(2, i % n, L)) % L for i in range(N)]
    P = S.padd(P, S.msm(hs, H))
    P = S.psub(P, S.smul(e_bl, S.B_BLINDING))
    Q = S.smul(w, S.B)
    P = S.padd(P, S.smul(t_x, Q))
    for k in range(lg):
        P = S.padd(P, S.padd(S.smul(us[k] * us[k] % L, Ls[k]), S.smul(S._inv(us[k] * us[k] % L), Rs[k])))
    s = []
    for i in range(N):
        acc = 1
        for k in range(lg):
            acc = acc * (us[k] if (i >> (lg - 1 - k)) & 1 else S._inv(us[k])) % L
        s.append(acc)
    want = S.padd(S.msm([a * si % L for si in s], G), S.msm([b * S._inv(si) % L * pow(yinv, i, L) % L for i, si in enumerate(s)], H))
    want = S.padd(want, S.smul(a * b % L, Q))
    return S.psub(lhs, rhs), S.psub(want, P)


def _chunk_V(commits, d, P, c, nb):
    """the shifted, padded commitments of chunk c (range_proof_vec/mod.rs:155-167)"""
    off = S.smul(1 << (nb - 1), S.B)
    dp = S.next_pow2(d); m = dp // P
    return [S.padd(bytes(commits[j]), off) if j < d else S.IDENTITY for j in range(c * m, (c + 1) * m)]


def _psum(points):
    acc = S.IDENTITY
    for p in points:
        acc = S.padd(acc, p)
    return acc


def _cancels(members, honest):
    """members = [(proof, V, n, label)] of the tampered proofs, honest = the same untampered: (c)"""
    for pf, V, n, label in honest:
        assert range_residuals(pf, V, n, label) == (ID, ID)
    res = [range_residuals(pf, V, n, label) for pf, V, n, label in members]
    for r1, r2 in res:
        assert r1 == ID and r2 != ID      # a and b enter the inner-product check only; each member alone fails it
    assert _psum([r2 for _, r2 in res]) == ID


def _ok(pr, cm, nb=K.NB):
    return orc.verify_rangeproof(pr, cm, nb, K.FP[0], K.FP[1])


@pytest.mark.parametrize("shape", K.R1_SHAPES + [K.R1_RUN], ids=lambda s: "d%d-P%d-%d-%d" % s)
def test_r1_two_chunks_of_one_client(shape):
    d, P, p, q = shape
    pr, cm = K.range_r1(d, P, p, q)
    assert _ok(pr, cm) == (0, True)                                                           # (a): a proof copied onto an identical chunk verifies
    for delta in K.DELTAS:
        t = K.range_apply(pr, [(p, 1), (q, -1)], delta)
        assert _ok(t, cm) == (0, False)                                                       # (b)
        for only in ((p, 1), (q, -1)):
            assert _ok(K.range_apply(pr, [only], delta), cm) == (0, False)
        if S.so is not None:
            V = {c: _chunk_V(cm, d, P, c, K.NB) for c in (p, q)}
            assert V[p] == V[q]
            _cancels([(t[c], V[c], K.NB, b"RangeProof") for c in (p, q)], [(pr[p], V[p], K.NB, b"RangeProof")])


@pytest.mark.parametrize("field", ["a", "b"], ids=["R2", "R3"])
@pytest.mark.parametrize("ncopies", [2, 3])
def test_r2_r3_copies_of_one_update(field, ncopies):
    d, P = 8, 4
    copies = tuple(range(ncopies))
    prs, cms = K.copies_batch(ncopies, copies, d, P)
    assert all((prs[i] == prs[0]).all() and (cms[i] == cms[0]).all() for i in copies)
    assert _ok(prs[0], cms[0]) == (0, True)                                                   # (a)
    mult = K.copies_edits(copies)
    for c in (0, 3):
        V = _chunk_V(cms[0], d, P, c, K.NB) if S.so is not None else None
        for delta in K.DELTAS:
            ts = [K.range_apply(prs[i], [(c, mult[i])], delta, field) for i in copies]
            assert all(_ok(t, cms[0]) == (0, False) for t in ts)                              # (b)
            if V is not None:
                _cancels([(t[c], V, K.NB, b"RangeProof") for t in ts], [(prs[0][c], V, K.NB, b"RangeProof")])


@pytest.mark.parametrize("field", ["a", "b"], ids=["R2", "R3"])
@pytest.mark.parametrize("ncopies", [2, 3])
def test_r2_r3_copies_of_one_l2_sum_proof(field, ncopies):
    copies = tuple(range(ncopies))
    prs, cms = K.l2_batch(ncopies, copies)
    assert orc.verify_rangeproof_l2(prs[0], cms[0], K.L2_BITS, K.FP[0], K.FP[1]) == (0, True)     # (a)
    mult = K.copies_edits(copies)
    for delta in K.DELTAS:
        ts = [K.range_apply(prs[i].reshape(1, -1), [(0, mult[i])], delta, field)[0] for i in copies]
        assert all(orc.verify_rangeproof_l2(t, cms[0], K.L2_BITS, K.FP[0], K.FP[1]) == (0, False) for t in ts)      # (b)
        if S.so is not None:
            V = [bytes(cms[0])]
            _cancels([(t, V, K.L2_BITS, b"L2RangeProof") for t in ts], [(prs[0], V, K.L2_BITS, b"L2RangeProof")])


@needs_sodium
def test_r2_at_the_round_shape():
    """the (8, 128) generators of a round of d = 300, P = 4: two copies, a +- 1 on a chunk with padding behind its values"""
    d, P, c = 300, 4, 2
    pr, cm = K.range_client(d, P, 7)
    assert _ok(pr, cm) == (0, True)
    ts = [K.range_apply(pr, [(c, s)], 1) for s in (1, -1)]
    assert all(_ok(t, cm) == (0, False) for t in ts)
    V = _chunk_V(cm, d, P, c, K.NB)
    _cancels([(t[c], V, K.NB, b"RangeProof") for t in ts], [])
