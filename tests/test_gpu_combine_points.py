"""GPU checks of the shared-scalar point combination (rofl_combine_points / rofl_threshold_combine: k_shamir_weights, k_comb_schedule,
k_comb_decode, k_comb_accumulate, k_comb_finish) against plain integers, bytes against bytes: the terms are P[i][j] = y_ij B for known y_ij,
so out[i] = encode((sum_j a_j y_ij mod l) B).  rofl_dbg_combine_points_split forces the window width c and the slice count S, so that every
split is reached at small shapes; no output byte may depend on either."""
import numpy as np
import pytest

import orc
import test_combine_points_host as H

pytestmark = pytest.mark.gpu
ELL = H.ELL
SPLITS = [None, (2, 1), (5, 3), (8, 2), (10, 1), (4, 64)]      # None: chosen from the shape, and the public call beside it
XS = (7, 2 ** 32 - 1, 3, 2 ** 31, 1)


@pytest.fixture(scope="module")
def R():
    import rofl_project_code_amd as R
    from rofl_project_code_amd import build
    build.build()
    R.set_device(0)
    return R


@pytest.fixture(scope="module")
def grid(R):
    """257 x 33 terms y_ij B made once: (ys, points, {n_terms: (scalars, expected for the first n_terms columns)})"""
    rng = np.random.default_rng(20271120)
    keys = rng.integers(0, 256, size=(257 * 33, 32), dtype=np.uint8)
    ys = [[y % ELL for y in H.ints(keys[33 * i:33 * i + 33])] for i in range(257)]
    pts = R.key_agreement.public_keys(keys).reshape(257, 33, 32)
    by_terms = {}
    for t in (1, 2, 5, 33):
        a = H.ints(orc.rand_scalars(rng, t))
        by_terms[t] = (a, H.expected(a, [row[:t] for row in ys]))
    return ys, pts, by_terms


def run(R, scalars, pts, split):
    """(out, status) through the forced split; for split None through the chosen split AND the public call, which must agree"""
    sc = np.stack([H.b32(a) for a in scalars])
    out, status = H.combine(R.lib(), "rofl_dbg_combine_points_split", sc, pts, split or (0, 0))
    if split is None:
        o2, s2 = R.pedersen_ops.combine_points(sc, pts)
        assert o2.tobytes() == out.tobytes() and s2.tobytes() == status.tobytes()
    return out, status


@pytest.mark.parametrize("split", SPLITS)
@pytest.mark.parametrize("n_terms", [1, 2, 5, 33])
@pytest.mark.parametrize("n_items", [1, 63, 64, 65, 257])
def test_shapes_and_splits(R, grid, n_items, n_terms, split):
    """a lane, a wave less one, a full wave, a wave crossing, several blocks with a ragged tail; 5 terms over 3 slices, S above the terms
    (clamped), c = 10 with almost every digit value empty"""
    ys, pts, by_terms = grid
    a, want = by_terms[n_terms]
    out, status = run(R, a, np.ascontiguousarray(pts[:n_items, :n_terms]), split)
    assert out.tobytes() == want[:n_items].tobytes() and not status.any()


@pytest.mark.parametrize("split", [None, (5, 3), (10, 1)])
@pytest.mark.parametrize("family", ["random", "all_equal", "top_range", "two_pow_252", "small", "minus_one", "plus_l", "zero"])
def test_scalar_families(R, grid, family, split):
    """zero, l - 1 (the carry out of the top window), 2^252, a + l (reduced), all equal (one digit value per window), all zero (the identity
    for every item from an empty schedule)"""
    ys, pts, _ = grid
    rng = np.random.default_rng(20271121)
    fam = orc.extreme_scalar_cases(rng, 5)
    a = [0] * 5 if family == "zero" else [v + ELL for v in H.ints(fam["random"])] if family == "plus_l" else H.ints(fam[family])
    out, status = run(R, a, np.ascontiguousarray(pts[:65, :5]), split)
    assert out.tobytes() == H.expected(a, [row[:5] for row in ys[:65]]).tobytes() and not status.any()
    assert family != "zero" or not out.any()


@pytest.mark.parametrize("split", [None, (2, 1), (5, 3)])
def test_identity_terms_and_cancelling_pairs(R, grid, split):
    """the identity as a term; the same point under a and l - a; P and -P under equal scalars: the sums that vanish need complete additions"""
    ys, pts, _ = grid
    a = 0x1234567890abcdef1234567890abcdef % ELL
    y = ys[0][0]
    p, neg_p = pts[0, 0], R.key_agreement.public_keys(H.b32(ELL - y))[0]
    items = np.stack([np.stack([p, np.zeros(32, np.uint8), pts[0, 1]]), np.stack([p, p, np.zeros(32, np.uint8)]), np.stack([p, neg_p, pts[0, 2]])])
    for scalars, rows in (([a, 5, 7], [[y, 0, ys[0][1]], [y, y, 0], [y, ELL - y, ys[0][2]]]), ([a, ELL - a, 9], [[y, 0, ys[0][1]], [y, y, 0], [y, ELL - y, ys[0][2]]]),
                          ([a, a, 0], [[y, 0, 0], [y, y, 0], [y, ELL - y, 0]])):
        out, status = run(R, scalars, items, split)
        assert out.tobytes() == H.expected(scalars, rows).tobytes() and not status.any()
    assert not out[2].any()                                                        # a P + a (-P): the identity, status 0


@pytest.mark.parametrize("split", [None, (5, 3)])
def test_a_refused_term_condemns_its_item_only(R, grid, split):
    ys, pts, by_terms = grid
    a = by_terms[5][0]
    three = np.ascontiguousarray(pts[:3, :5]).copy()
    three[1, 3] = 0xff
    out, status = run(R, a, three, split)
    alone, _ = run(R, a, np.ascontiguousarray(three[[0, 2]]), split)
    assert status.tolist() == [0, 2, 0] and not out[1].any() and out[[0, 2]].tobytes() == alone.tobytes() == by_terms[5][1][[0, 2]].tobytes()
    twin, tst = H.combine(R.lib(), "rofl_dbg_host_combine_points", np.stack([H.b32(v) for v in a]), three)
    assert twin.tobytes() == out.tobytes() and tst.tolist() == [0, 2, 0]           # device and host twin, byte for byte


@pytest.fixture(scope="module")
def committee(R):
    """a key dealt at t = 3 over five points, 65 ciphertexts, every member's answers: (pk, member_pks, ct, shared, partials, proofs, ctx)"""
    rng = np.random.default_rng(20271122)
    sk, seed, eph, ctx = (rng.integers(0, 256, size=(n, 32), dtype=np.uint8) for n in (1, 1, 65, 1))
    shares = R.secret_sharing.share(sk, seed, 3, 5, xs=XS)[0]
    pk, member_pks = R.key_agreement.public_keys(sk)[0], R.key_agreement.public_keys(shares)
    ct, shared = R.threshold.encapsulate(pk, eph)
    answers = [R.threshold.partial_decrypt(shares[j], ct, ctx) for j in range(5)]
    assert not any(st.any() for _, _, st in answers)
    return pk, member_pks, ct, shared, np.stack([p for p, _, _ in answers], axis=1), np.stack([q for _, q, _ in answers], axis=1), ctx


@pytest.mark.parametrize("device", [False, True])
@pytest.mark.parametrize("members", [(0, 1, 2), (4, 2, 0), (0, 1, 2, 3, 4)])
def test_threshold_round_trip(R, committee, members, device):
    """the server derives byte for byte what the encrypting clients derived, through the public call and forced onto the device"""
    pk, member_pks, ct, shared, partials, proofs, ctx = committee
    fn = None
    if device:
        raw = R.lib().rofl_dbg_threshold_combine_split
        raw.argtypes = H.THRESHOLD_ARGS + [H.u32, H.u32]
        fn = lambda *args: raw(*[getattr(x, "value", x) for x in args], 0, 0)      # noqa: E731
    sel, xs = list(members), [XS[j] for j in members]
    got, status = R.threshold.combine(pk, xs, ct, np.ascontiguousarray(partials[:, sel]), _fn=fn)
    assert got.tobytes() == shared.tobytes() and not status.any()
    wrong = partials[:, sel].copy()
    wrong[40, 1] = partials[41, sel[1]]                                            # a valid point, not this member's answer for ciphertext 40
    got, status = R.threshold.combine(pk, xs, ct, wrong, _fn=fn)
    differs = (got != shared).any(axis=1)
    assert not status.any() and differs.tolist() == [i == 40 for i in range(65)]
    for k, j in enumerate(sel):
        verdicts = R.threshold.verify_partials(member_pks[j], ct, ctx, wrong[:, k], proofs[:, j])
        assert verdicts.tolist() == [1 if (k == 1 and i == 40) else 0 for i in range(65)]


def test_member_keys_against_the_committee_key(R, committee):
    pk, member_pks = committee[:2]
    assert R.threshold.check_member_keys(pk, XS, member_pks, 3)
    altered = member_pks.copy()
    altered[3] = member_pks[2]
    assert not R.threshold.check_member_keys(pk, XS, altered, 3)
    assert not R.threshold.check_member_keys(member_pks[0], XS, member_pks, 3)
