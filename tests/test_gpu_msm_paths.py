"""Every variant of the Pippenger driver (csrc/host_msm.hpp) and every repeat after an overflow, under scalars built to collide.

An MSM runs on the fastest variant whose fixed-size structures hold its input -- fixed-base two-level sort | fixed-base slot sort | fused
small launch | generic slot sort | count / scan / scatter -- and is repeated on the next one when a bucket list, the overflow list or a
coarse bin runs over.  Hash-derived scalars never do that; a malicious proof chooses the verifier's generator scalars and can.  Each case
here asserts (a) every result byte for byte against the oracle's MSM of the same scalars and points, and (b) the path: the attempts that
rofl_dbg_msm_trace reports are the expected variants in the expected order, and wherever the slot sort ran its overflow word is the
number tests/msm_model.py computes from the scalars with the capacity the trace itself reports.

What cannot be reached, and is therefore not here: a digit above B (two bucket entries) needs a scalar >= 2^252 + 2^(252 - c), and the
entries reduce mod l -- the top digit of the scalars of [2^252, l) is exactly B, which the families include; a small-launch list of 64
cannot run over with 64 terms, so the n = 64 cases sit AT the capacity; and behind the small launch of n = 6000 (lists of 72, slots of 64)
the slot sort never sees less than 9 entries over, so its boundary there is 9 / 10 with every other forced bucket exactly full."""
import ctypes

import numpy as np
import pytest

import msm_model as M
import orc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def R():
    import rofl_project_code_amd as R
    from rofl_project_code_amd import build
    build.build()
    R.set_device(0)     # fails loudly when there is no HIP device / library
    return R


@pytest.fixture(scope="module")
def host8(R):
    """the eight-lane host chains finish launches of eight and more generic problems exactly where the CPU has AVX-512 IFMA"""
    return R.lib().rofl_dbg_host_horner8_selftest(ctypes.c_uint(37), ctypes.c_uint(7), 8, None, None) != -1


@pytest.fixture(scope="module")
def points():
    """1024 oracle-made points; a case tiles them to its length (repeated points are legal input)"""
    return orc.commit_vec(orc.rand_scalars(np.random.default_rng(2024), 1024), None)


_GENS = {}


def gens(n_bits, m):
    if (n_bits, m) not in _GENS:
        _GENS[(n_bits, m)] = np.concatenate(orc.bp_gens(n_bits, m))      # [G | H], party-major
    return _GENS[(n_bits, m)]


def tiled(points, n):
    return np.ascontiguousarray(np.tile(points, ((n + 1023) // 1024, 1))[:n])


def run_generic(R, problems, pts):
    """-> (out [np][32], trace); one problem goes through rofl_dbg_msm, several through rofl_dbg_msm_many"""
    problems = np.ascontiguousarray(problems)
    if problems.shape[0] == 1:
        out = np.zeros((1, 32), np.uint8)
        assert R.lib().rofl_dbg_msm(problems.ctypes.data_as(ctypes.c_void_p), pts.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(problems.shape[1]),
                                    out.ctypes.data_as(ctypes.c_void_p)) == 0
    else:
        out = R.api.dbg_msm_many(problems, pts)
    return out, R.api.msm_trace()


def assert_results(out, problems, pts, what):
    for p in range(problems.shape[0]):
        assert (out[p] == orc.msm(problems[p], pts)).all(), "%s: problem %d differs from the oracle" % (what, p)


def slot_word(problems, a):
    """the overflow word of a slot-sort attempt, from the attempt's own layout and capacity"""
    total = 0
    for p in problems:
        ld = M.loads(p, a["c"])
        if a["kind"] == "fixed_base":
            ld = M.merge_sets(ld, a["sets"])
        total += M.overflow(ld, a["cap"])
    return total


def check_trace(trace, problems, expect, host8, what):
    """expect: [(kind, two, c)] -- the attempts, in order.  Every attempt but the last was repeated; a small launch overflowed exactly when a
    bucket of its layout holds more than its list (64 entries up to 8 B terms, else 72); the slot sort reports the model's count and is
    repeated exactly above 4096; count-sort never overflows; the finisher follows the problem count."""
    msg = "%s: trace %r" % (what, trace)
    assert [(a["kind"], a["two"], a["c"]) for a in trace] == [tuple(e) for e in expect], msg
    n, np_ = problems.shape[1], problems.shape[0]
    for i, a in enumerate(trace):
        last = i + 1 == len(trace)
        assert a["repeated"] == (not last), msg
        assert a["W"] == M.plan(a["c"])["W"], msg
        assert a["finisher"] == M.finisher(np_, a["kind"] == "fixed_base", host8), msg
        if a["kind"] == "small":
            small_cap = 64 if n <= 8 * M.plan(a["c"])["B"] else 72
            over = any(int(M.loads(p, a["c"]).max()) > small_cap for p in problems)
            assert (a["overflow"] != 0) == over == a["repeated"], msg
        elif a["kind"] == "count_sort":
            assert a["overflow"] == 0 and last, msg
        elif a["two"]:
            assert (a["overflow"] != 0) == a["repeated"] and a["cap_bin"] > 0, msg
        else:
            word = slot_word(problems, a)
            assert a["overflow"] == word, "%s: the model says %d" % (msg, word)
            assert a["repeated"] == (word > M.OVF_MAX), msg


def generic_expect(problems):
    return [(k, False, c) for k, c, _, _ in M.predict_generic(problems)]


def generic_case(R, host8, points, problems, what, kinds=None):
    """runs one generic launch, checks results and path; kinds: the variants the case is built to take (a check of the case itself)"""
    problems = np.ascontiguousarray(problems)
    pts = tiled(points, problems.shape[1])
    expect = generic_expect(problems)
    if kinds is not None:
        assert [e[0] for e in expect] == list(kinds), "%s: the case was built for %r, the model predicts %r" % (what, kinds, expect)
    out, trace = run_generic(R, problems, pts)
    check_trace(trace, problems, expect, host8, what)
    assert_results(out, problems, pts, what)
    if trace[-1]["kind"] == "count_sort":
        # nothing of the repeated MSM is left in the workspace or in the variants allowed: a random call of the same shape right after it
        # takes the first variant again, clean
        rnd = np.stack([M.random_scalars(np.random.default_rng(991 + p), problems.shape[1]) for p in range(problems.shape[0])])
        out2, trace2 = run_generic(R, rnd, pts)
        assert len(trace2) == 1 and trace2[0]["kind"] == expect[0][0] and trace2[0]["overflow"] == 0, "%s, then random: %r" % (what, trace2)
        assert_results(out2, rnd, pts, what + ", then random")
    return trace


# ---------------------------------------------------------------- generic, one problem
@pytest.mark.parametrize("n,kind,c", [(63, "small", 4), (64, "small", 7), (600, "small", 10), (8192, "small", 10), (8193, "slots", 13)])
def test_generic_benign(R, host8, points, n, kind, c):
    k = M.random_scalars(np.random.default_rng(n), n)[None]
    trace = generic_case(R, host8, points, k, "random n=%d" % n, kinds=[kind])
    a = trace[0]
    g = M.generic_plan(n)
    assert a["c"] == c and a["overflow"] == 0 and a["finisher"] == "host"
    assert a["small_group"] == (1 if kind == "small" else 0)
    if kind == "slots":
        assert a["cap"] == g["cap"] == 16


@pytest.mark.parametrize("n", [600, 6000])
@pytest.mark.parametrize("extra", [0, 1])
def test_small_list_boundary(R, host8, points, n, extra):
    """one bucket of the fused small launch at exactly its list capacity (64 at n = 600, 72 at n = 6000), and one entry more: the launch is
    repeated on the slot sort (k_msm_scatter_slots below 8192 terms), whose overflow list takes what the bucket's slots do not hold"""
    g = M.generic_plan(n)
    assert g["small"] and g["small_cap"] == (64 if n == 600 else 72)
    for w, d in ((4, 9), (2, -6), (M.plan(10)["W"] - 1, 2)):
        k, claims = M.build(n, 10, [(w, d, g["small_cap"] + extra)], seed=n + extra)
        what = "n=%d, %d entries in bucket (%d, %d)" % (n, g["small_cap"] + extra, w, abs(d) - 1)
        trace = generic_case(R, host8, points, k[None], what, kinds=["small", "slots"] if extra else ["small"])
        if extra:
            assert trace[1]["cap"] == g["cap"] and trace[1]["overflow"] == g["small_cap"] + 1 - g["cap"], what


def _excess(n, case):
    if n == 6000:      # behind the small launch: one list must hold more than 72, which is 9 over the 64 slots
        return {"cap": [9, 0, 0, 0, 0, 0, 0, 0], "cap+1": [9, 1, 0, 0, 0, 0, 0, 0]}.get(case) or M.split(int(case))
    return {"cap": [0] * 8, "cap+1": [1, 0, 0, 0, 0, 0, 0, 0]}.get(case) or M.split(int(case))


@pytest.mark.parametrize("n", [6000, 8193])
@pytest.mark.parametrize("case", ["cap", "cap+1", "300", "4096", "4097"])
def test_slot_boundary_and_overflow_list(R, host8, points, n, case):
    """Eight forced buckets (msm_model.sites: twins in two bucket arrays, a negative digit, +B, -B, the top window, the scalars of
    [2^252, l)) at cap + excess entries each: every bucket exactly full -> word 0; one over -> 1; 300 over, spread; 4096 over: the overflow
    list is exactly full and still handled in place; 4097: repeated on count-sort.  n = 8193 goes through k_msm_scatter_lds, n = 6000
    through the repeated small launch and k_msm_scatter_slots."""
    g = M.generic_plan(n)
    excess = _excess(n, case)
    k, claims = M.build(n, g["c"], M.spread(g["c"], g["cap"], excess), seed=n)
    total = sum(excess)
    assert M.overflow(M.loads(k, g["c"]), g["cap"]) == total      # (the case itself: nothing but the forced buckets is over)
    kinds = (["small"] if n == 6000 else []) + ["slots"] + (["count_sort"] if total > M.OVF_MAX else [])
    trace = generic_case(R, host8, points, k[None], "n=%d excess %s" % (n, case), kinds=kinds)
    slots = trace[1 if n == 6000 else 0]
    assert slots["cap"] == g["cap"] and slots["overflow"] == total and slots["repeated"] == (total > M.OVF_MAX)


@pytest.mark.parametrize("n,kinds", [(64, ["small"]), (65, ["small", "slots"]), (300, ["small", "slots", "count_sort"]), (8193, ["slots", "count_sort"])])
def test_total_skew(R, host8, points, n, kinds):
    """all scalars l - 1: one bucket per window holds every term (digit exactly B in the top window).  64 terms fill the small launch's lists
    of 64 exactly; 65 run over and fit the overflow list; 300 and 8193 go down to count-sort."""
    k = np.tile(M.from_int(M.L - 1), (n, 1))[None]
    generic_case(R, host8, points, k, "n=%d, all l - 1" % n, kinds=kinds)


@pytest.mark.parametrize("excess", [None, 300])
def test_sixteen_bit_windows(R, host8, points, excess):
    """n = 2^17: c = 16, B = 32768, two k_msm_reduce_level passes.  With 16 slots a bucket and a mean load of 8 in the three 15-bit windows even
    random scalars leave a few hundred entries to the overflow list: the word is the model's count either way."""
    n = 1 << 17
    g = M.generic_plan(n)
    assert g["c"] == 16 and not g["small"] and g["cap"] == 16
    if excess is None:
        k = M.random_scalars(np.random.default_rng(17), n)
    else:
        k, _ = M.build(n, 16, M.spread(16, 16, M.split(excess)), seed=17)
    word = M.overflow(M.loads(k, 16), 16)
    assert (excess or 0) <= word <= M.OVF_MAX
    trace = generic_case(R, host8, points, k[None], "n=2^17 excess %r" % excess, kinds=["slots"])
    assert trace[0]["overflow"] == word and trace[0]["cap"] == 16


# ---------------------------------------------------------------- generic, many problems
@pytest.mark.parametrize("n", [64, 1024])
@pytest.mark.parametrize("np_", [8, 14, 32, 33])
@pytest.mark.parametrize("skew", [False, True])
def test_many_problems(R, host8, points, n, np_, skew):
    """k_msm_small / k_msm_small_g (four windows per block once np W > 512 at c = 7) with k_msm_wsum + the host's eight-lane chains, or
    k_msm_horner from 32 problems where the CPU has no AVX-512 IFMA.  skew: the LAST problem alone carries one bucket with one entry more
    than a list holds (n = 64: with all its 64 terms, which fill a list of 64 exactly); the overflow word belongs to the launch, so every
    problem is repeated on the slot sort and every result must still be right."""
    g = M.generic_plan(n, np_)
    assert g["small"]
    probs = np.stack([M.random_scalars(np.random.default_rng(1000 * n + 40 * np_ + p), n) for p in range(np_)])
    kinds = ["small"]
    if skew:
        load = min(n, g["small_cap"] + 1)
        probs[-1], _ = M.build(n, g["c_small"], [(4, 9, load)], seed=n + np_)
        if load > g["small_cap"]:
            kinds = ["small", "slots"]
    trace = generic_case(R, host8, points, probs, "n=%d np=%d skew=%d" % (n, np_, skew), kinds=kinds)
    assert trace[0]["c"] == g["c_small"] and trace[0]["small_group"] == g["small_group"]
    assert trace[-1]["finisher"] == ("host8" if host8 else "device" if np_ >= 32 else "host")
    if len(trace) == 2:
        assert trace[1]["cap"] == g["cap"] and trace[1]["overflow"] >= g["small_cap"] + 1 - g["cap"]


# ---------------------------------------------------------------- fixed-base
def run_fixed(R, n_bits, m, problems):
    out = R.api.dbg_msm_fixed(n_bits, m, np.ascontiguousarray(problems))
    return out, R.api.msm_trace()


_BENIGN = {}


def fixed_benign(R, host8, n_bits, m, np_):
    """the first attempt of a random call of the shape (results and path checked): where a case takes cap, cap_bin, c and sets from"""
    key = (n_bits, m, np_)
    if key not in _BENIGN:
        n = 2 * n_bits * m
        probs = np.stack([M.random_scalars(np.random.default_rng(77 * n + p), n) for p in range(np_)])
        out, trace = run_fixed(R, n_bits, m, probs)
        assert len(trace) == 1 and trace[0]["kind"] == "fixed_base" and trace[0]["overflow"] == 0 and not trace[0]["repeated"], trace
        check_trace(trace, probs, [("fixed_base", trace[0]["two"], trace[0]["c"])], host8, "random fixed-base %r" % (key,))
        assert_results(out, probs, gens(n_bits, m), "random fixed-base %r" % (key,))
        _BENIGN[key] = trace[0]
    return _BENIGN[key]


def fixed_case(R, host8, n_bits, m, problems, fb_attempts, what):
    """fb_attempts: [(two, c)] of the fixed-base attempts the case is built for; if the last of them is repeated (the slot sort's overflow list
    ran over) the chain goes on through the generic variants as the model predicts them"""
    problems = np.ascontiguousarray(problems)
    out, trace = run_fixed(R, n_bits, m, problems)
    expect = [("fixed_base", two, c) for two, c in fb_attempts]
    if len(trace) > len(expect):
        expect += generic_expect(problems)
    check_trace(trace, problems, expect, host8, what)
    assert_results(out, problems, gens(n_bits, m), what)
    if trace[-1]["kind"] == "count_sort":
        first = fixed_benign(R, host8, n_bits, m, problems.shape[0])
        rnd = np.stack([M.random_scalars(np.random.default_rng(551 + p), problems.shape[1]) for p in range(problems.shape[0])])
        out2, trace2 = run_fixed(R, n_bits, m, rnd)
        assert len(trace2) == 1 and trace2[0]["kind"] == "fixed_base" and trace2[0]["two"] == first["two"] and trace2[0]["overflow"] == 0, "%s, then random: %r" % (what, trace2)
        assert_results(out2, rnd, gens(n_bits, m), what + ", then random")
    return trace


def test_fixed_base_shapes(R, host8):
    """random calls: (8, 256) -- 4096 terms, below the two-level sort's 8192 a side -- takes the slot sort over the window table; (8, 512) the
    two-level sort at c = 16; 32 problems of (8, 512) the 15-bit table.  A shape below ROFL_MSM_FB_MIN has no table: 11."""
    a = fixed_benign(R, host8, 8, 256, 1)
    assert (a["two"], a["c"], a["sets"], a["cap_bin"]) == (False, 16, 16, 0) and a["cap"] >= 16
    a = fixed_benign(R, host8, 8, 512, 1)
    assert (a["two"], a["c"], a["sets"]) == (True, 16, 16) and a["cap_bin"] >= 64
    a = fixed_benign(R, host8, 8, 512, 32)
    assert (a["two"], a["c"], a["sets"]) == (True, 15, 1) and a["cap_bin"] >= 64 and a["finisher"] == "host"
    k = M.random_scalars(np.random.default_rng(1), 2 * 8 * 4)[None]
    with pytest.raises(R.api.RoflError) as e:
        R.api.dbg_msm_fixed(8, 4, k)
    assert e.value.code == 11


@pytest.mark.parametrize("case", ["cap", "cap+1", "300", "4096", "4097"])
def test_fixed_base_slot_sort(R, host8, case):
    """(8, 256): k_msm_scatter_slots over the window table (entry = w * stride + i) and k_msm_overflow's gather from it.  Exactly full, one over,
    300 over spread over the eight sites, the overflow list exactly full, and one more: repeated on the generic variants (the generators as
    plain points), as far down as the model says."""
    a = fixed_benign(R, host8, 8, 256, 1)
    n, cap = 4096, a["cap"]
    excess = {"cap": [0] * 8, "cap+1": [1, 0, 0, 0, 0, 0, 0, 0]}.get(case) or M.split(int(case))
    k, _ = M.build(n, 16, M.spread(16, cap, excess), seed=256)
    total = sum(excess)
    assert M.overflow(M.loads(k, 16), cap) == total
    trace = fixed_case(R, host8, 8, 256, k[None], [(False, 16)], "(8, 256) excess %s" % case)
    assert trace[0]["overflow"] == total and trace[0]["cap"] == cap
    assert (len(trace) > 1) == (total > M.OVF_MAX)
    if total > M.OVF_MAX:
        assert trace[1]["kind"] == "small" and trace[1]["repeated"]


@pytest.mark.parametrize("case", ["half_bin", "300", "5000"])
def test_fixed_base_two_level(R, host8, case):
    """(8, 512), c = 16: one shared digit in one window.  Half a coarse bin's capacity: still one attempt (the bucket's list is as long as it
    needs to be).  300: the bin runs over, the slot sort takes the MSM with the excess in its overflow list.  5000: that list runs over too and
    the chain goes on through the generic variants to count-sort.  (Level 1 reserves bin space in multiples of 32 per tile, so the exact
    capacity of a bin is not predictable from the loads: only far below and far above are asserted.)"""
    a = fixed_benign(R, host8, 8, 512, 1)
    assert a["two"] and a["cap_bin"] < 300
    cnt = a["cap_bin"] // 2 if case == "half_bin" else int(case)
    k, claims = M.build(8192, 16, [(4, 77, cnt)], seed=512)
    fb = {"half_bin": [(True, 16)], "300": [(True, 16), (False, 16)], "5000": [(True, 16), (False, 16)]}[case]
    trace = fixed_case(R, host8, 8, 512, k[None], fb, "(8, 512), %d terms share a digit" % cnt)
    if case == "300":
        assert len(trace) == 2 and trace[1]["overflow"] == M.overflow(M.loads(k, 16), trace[1]["cap"]) >= 300 - trace[1]["cap"]
    if case == "5000":
        assert [t["kind"] for t in trace[2:]] == ["small", "slots", "count_sort"], trace


@pytest.mark.parametrize("shared", [300, 3000])
def test_fixed_base_15_bit_layout(R, host8, shared):
    """32 problems of (8, 512): the 15-bit table, one bucket set per problem for all 17 windows.  The last problem shares one digit among 300
    terms -- far below a coarse bin's capacity: one attempt -- or among 3000: the bin runs over and the slot sort over the 15-bit table
    finishes with ~3000 entries from its overflow list."""
    a = fixed_benign(R, host8, 8, 512, 32)
    assert a["c"] == 15 and 1200 <= a["cap_bin"] < 2500      # (a hot bin holds ~600 random entries)
    probs = np.stack([M.random_scalars(np.random.default_rng(15000 + p), 8192) for p in range(32)])
    probs[-1], _ = M.build(8192, 15, [(3, 1234, shared)], seed=15)
    fb = [(True, 15)] if shared == 300 else [(True, 15), (False, 15)]
    trace = fixed_case(R, host8, 8, 512, probs, fb, "32 x (8, 512), %d terms of the last problem share a digit" % shared)
    assert all(t["c"] == 15 for t in trace)
    if shared == 3000:
        assert shared - trace[1]["cap"] <= trace[1]["overflow"] <= M.OVF_MAX
