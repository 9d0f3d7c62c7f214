"""tests/msm_model.py against itself and against arithmetic: the window layout recomposes every scalar, the digits stay in their range,
the vectorised digits equal the integer ones, and every builder produces exactly the bucket loads it claims (the GPU tests of
test_gpu_msm_paths.py take their expected overflow words from these).  No GPU."""
import numpy as np
import pytest

import msm_model as M

CS = (4, 7, 10, 13, 15, 16)


def _corpus(c):
    P = M.plan(c)
    rng = np.random.default_rng(100 + c)
    alt = [sum(((1 << width) - 1) << pos for w, (pos, width) in enumerate(P["windows"][:-1]) if w % 2 == par) for par in (0, 1)]
    fixed = [0, 1, M.L - 1, 2 ** 252 - 1, 2 ** 252, 2 ** 252 + 1, 2 ** 252 - 2, alt[0], alt[1]]
    rnd = [M.to_int(r) for r in M.random_scalars(rng, 1000)]
    return fixed, rnd


@pytest.mark.parametrize("c", CS)
def test_layout_covers_bits_0_to_253(c):
    P = M.plan(c)
    at = 0
    for w, (pos, width) in enumerate(P["windows"]):
        assert pos == at
        assert width == (c + 1 if w + 1 == P["W"] else c if w < P["wide"] else c - 1)
        at += width
    assert at == 254 and P["B"] == 1 << (c - 1)
    assert P["W"] <= 64      # the host8 / device finishers hold the window positions in 64 words


@pytest.mark.parametrize("c", CS)
def test_digits_recompose_the_scalar(c):
    P = M.plan(c)
    fixed, rnd = _corpus(c)
    for k in fixed + rnd:
        assert k < M.L
        ds = M.digits(k, c)
        assert sum(d << pos for d, (pos, _) in zip(ds, P["windows"])) == k
        for d, (_, width) in zip(ds[:-1], P["windows"][:-1]):
            assert -(1 << (width - 1)) <= d <= 1 << (width - 1) <= P["B"]
        # canonical scalars: the top digit is in [0, B] -- one bucket entry, never two
        assert 0 <= ds[-1] <= P["B"]
        if k >= 1 << 252:
            assert ds[-1] == P["B"]


@pytest.mark.parametrize("c", CS)
def test_top_window_two_entry_case(c):
    """|d| > B needs a scalar >= 2^252 + 2^(252 - c): not canonical, but the layout still recomposes it below 2^253 and the digit takes two
    buckets, B - 1 and |d| - B - 1 (the kernels keep that branch; scalars reduced mod l never reach it)"""
    P = M.plan(c)
    B = P["B"]
    rng = np.random.default_rng(c)
    ks = [2 ** 253 - 1, 2 ** 252 + 2 ** (252 - c), 2 ** 252 + 2 ** (252 - c) - 1] + [(1 << 252) | M.to_int(r) for r in M.random_scalars(rng, 200)]
    two = 0
    for k in ks:
        ds = M.digits(k, c)
        assert sum(d << pos for d, (pos, _) in zip(ds, P["windows"])) == k
        assert B <= ds[-1] <= 2 * B
        e = M.entries(ds[-1], B)
        assert e == ([B - 1] if ds[-1] == B else [B - 1, ds[-1] - B - 1])
        two += len(e) == 2
    assert two >= 100
    assert M.entries(0, B) == [] and M.entries(-3, B) == [2] and M.entries(B, B) == [B - 1] and M.entries(-B, B) == [B - 1]
    ld = M.loads(M.from_ints(ks), c)
    assert ld[-1].sum() == len(ks) + two and ld[-1][B - 1] >= len(ks)


@pytest.mark.parametrize("c", CS)
def test_vectorised_digits_equal_the_integer_ones(c):
    fixed, rnd = _corpus(c)
    ks = fixed + rnd[:200] + [2 ** 253 - 1, 2 ** 252 + 2 ** 251]
    dn = M.digits_np(M.from_ints(ks), c)
    for i, k in enumerate(ks):
        assert dn[i].tolist() == M.digits(k, c)
    assert (M.digits_np(M.from_ints(ks), c, only=2) == dn[:, 2]).all()
    # loads: one entry per non-zero digit (two where |d| > B)
    B = M.plan(c)["B"]
    assert M.loads(M.from_ints(ks), c).sum() == sum(len(M.entries(d, B)) for k in ks for d in M.digits(k, c))


@pytest.mark.parametrize("c", (7, 10, 13, 15, 16))
def test_force_sets_one_digit(c):
    P = M.plan(c)
    rng = np.random.default_rng(7 * c)
    for w in (0, 1, P["wide"] - 1, P["wide"], P["W"] - 2, P["W"] - 1):
        pos, width = P["windows"][w]
        half = 1 << (width - 1)
        top = w + 1 == P["W"]
        cand = [1, 3, P["B"] // 2 - 1] if top else [1, -1, half - 1, -(half - 1), -half] + ([half] if pos else [])
        if top:
            cand.append(P["B"])
        for d in cand:
            s = M.random_scalars(rng, 6)
            before = M.digits_np(s, c)
            M.force(s, range(6), w, d, c)
            after = M.digits_np(s, c)
            assert (after[:, w] == d).all(), (w, d)
            far = [x for x in range(P["W"]) if abs(x - w) > 1]
            assert (after[:, far] == before[:, far]).all()
            assert all(M.to_int(r) < 1 << 252 for r in s)
    with pytest.raises(ValueError):
        M.force(M.random_scalars(rng, 1), [0], 0, 1 << (c - 1), c)      # window 0 has no borrowed bit
    with pytest.raises(ValueError):
        M.force(M.random_scalars(rng, 1), [0], 1, (1 << (c - 1)) + 1, c)


# (n, c, cap) of the shapes the GPU tests use: generic LDS scatter, generic slot scatter behind the small launch, fixed-base slot sort,
# the 15-bit fixed-base layout, and 16-bit windows at 2^17 terms
SHAPES = [(8193, 13, 16), (6000, 10, 64), (600, 10, 16), (4096, 16, 32), (8192, 16, 32), (8192, 15, 32), (1024, 7, 64)]


@pytest.mark.parametrize("n,c,cap", SHAPES)
@pytest.mark.parametrize("total", [0, 1, 300, 4096, 4097])
def test_spread_family_loads(n, c, cap, total):
    if (n, total) in ((600, 4096), (600, 4097), (1024, 4096), (1024, 4097)):
        total = 200      # (shapes too small for the large totals)
    groups = M.spread(c, cap, M.split(total))
    scal, claims = M.build(n, c, groups, seed=11)
    assert all(M.to_int(r) < M.L for r in scal)
    ld = M.loads(scal, c)
    P = M.plan(c)
    assert len(claims) == 8 and sum(claims.values()) == 8 * cap + total
    for (w, b), v in claims.items():
        assert ld[w][b] == v
    # the twins: equal bucket index in two bucket arrays; the negative digit, +-B, the top window and the scalars of [2^252, l) are there
    assert claims[(1, 4)] and claims[(3, 4)] and (2, 6) in claims and (5, P["B"] - 1) in claims and (7, P["B"] - 1) in claims
    assert (P["W"] - 1, 2) in claims and (P["W"] - 1, P["B"] - 1) in claims
    dg = M.digits_np(scal, c)
    assert (dg[:, 2] == -7).sum() == claims[(2, 6)] and (dg[:, 5] == P["B"]).sum() == claims[(5, P["B"] - 1)]
    assert (dg[:, 7] == -P["B"]).sum() == claims[(7, P["B"] - 1)]
    assert sum(M.to_int(r) >= 1 << 252 for r in scal) == claims[(P["W"] - 1, P["B"] - 1)]
    # nothing but the claimed buckets is over its capacity: the overflow word of the slot sort is the forced excess
    assert M.overflow(ld, cap) == total
    # seeded: the same call gives the same bytes
    assert (M.build(n, c, groups, seed=11)[0] == scal).all()


def test_one_bucket_loads():
    for n, c, load in ((600, 10, 64), (600, 10, 65), (6000, 10, 72), (6000, 10, 73), (1024, 7, 73), (64, 7, 64)):
        for w, d in ((4, 9), (2, -6), (M.plan(c)["W"] - 1, 2)):
            scal, claims = M.build(n, c, [(w, d, load)], seed=n + load)
            ld = M.loads(scal, c)
            assert claims == {(w, abs(d) - 1): load} and ld[w][abs(d) - 1] == load
            if n > 64:
                assert np.delete(ld[w], abs(d) - 1).max() < load


def test_overflow_and_set_merge():
    ld = np.array([[0, 5, 16, 17], [40, 0, 0, 1], [1, 1, 1, 1], [16, 16, 0, 0]])
    assert M.overflow(ld, 16) == 1 + 24 and M.overflow(ld, 64) == 0 and M.overflow(ld, 0) == ld.sum()
    m = M.merge_sets(ld, 2)
    assert m.tolist() == [[1, 6, 17, 18], [56, 16, 0, 1]]
    assert M.merge_sets(ld, 4).tolist() == ld.tolist() and M.merge_sets(ld, 1).tolist() == [ld.sum(axis=0).tolist()]


def test_generic_plan_thresholds():
    g = M.generic_plan
    assert (g(63)["c"], g(64)["c"], g(511)["c"], g(512)["c"], g(8191)["c"], g(8192)["c"], g((1 << 17) - 1)["c"], g(1 << 17)["c"]) == (4, 7, 7, 10, 10, 13, 13, 16)
    assert g(8192)["small"] and g(8192)["c_small"] == 10 and g(8192)["small_cap"] == 72 and not g(8193)["small"]
    assert g(600)["small_cap"] == 64 and g(4096)["small_cap"] == 64 and g(4097)["small_cap"] == 72 and g(6000)["cap"] == 64 and g(8193)["cap"] == 16
    assert g(1024, 8)["c"] == 10 and g(1024, 32)["c"] == 7 and g(1024, 32)["small"] and g(1024, 32)["small_cap"] == 72 and g(1024, 32)["small_group"] == 4
    assert g(64, 8)["small_group"] == 1 and g(64, 14)["small_group"] == 4 and g(1024, 14)["small_group"] == 1
    assert M.finisher(1, False, True) == "host" and M.finisher(8, False, True) == "host8" and M.finisher(14, False, False) == "host"
    assert M.finisher(32, False, False) == "device" and M.finisher(32, True, True) == "host"


def test_predict_generic_chains():
    rng = np.random.default_rng(3)
    assert M.predict_generic(M.random_scalars(rng, 600)[None]) == [("small", 10, 0, False)]
    s, _ = M.build(600, 10, [(4, 9, 65)], seed=1)
    assert M.predict_generic(s[None]) == [("small", 10, None, True), ("slots", 10, 49, False)]
    s, _ = M.build(6000, 10, [(4, 9, 64 + 4097)], seed=1)
    assert M.predict_generic(s[None]) == [("small", 10, None, True), ("slots", 10, 4097, True), ("count_sort", 10, 0, False)]
    minus_one = np.tile(M.from_int(M.L - 1), (64, 1))
    assert M.predict_generic(minus_one[None]) == [("small", 7, 0, False)]      # 64 terms fill a list of 64 exactly
    assert [a[0] for a in M.predict_generic(np.tile(M.from_int(M.L - 1), (300, 1))[None])] == ["small", "slots", "count_sort"]
