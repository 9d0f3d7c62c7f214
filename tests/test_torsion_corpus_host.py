"""The four host encoders and identity predicates (rofl_dbg_encode_reps sites 1 .. 4) on every 4-torsion-shifted representative of
tests/torsion_corpus.py, the corpus's own consistency, and tests/bsgs_model.py against the oracle's BSGS.  No GPU; every comparison is
byte for byte against pyref (the encodings) or integer for integer (the logs).

Sites: 1 gd_ristretto_encode (csrc/fe26.hpp, host build), 2 ristretto_encode (csrc/fe32.hpp), 3 h51::encode (csrc/host51.hpp), 4 h8::encode8
(csrc/host51x8.hpp, AVX-512 IFMA: skipped where the CPU has none, like the eight-lane self-tests)."""
import ctypes

import numpy as np
import pytest

import bsgs_model as BM
import orc
import torsion_corpus as TC

pyref = TC.pyref
P = TC.P
REPS = TC.raw_reps()
N_CLASSES = len(TC.classes())


def _xyzt(reps):
    return np.frombuffer(b"".join(r["xyzt"] for r in reps), np.uint8).reshape(-1, 128)


def _expect(reps):
    return np.frombuffer(b"".join(r["expect"] for r in reps), np.uint8).reshape(-1, 32)


def _run(api, site, reps):
    got = api.dbg_encode_reps(site, _xyzt(reps))
    if got is None:
        pytest.skip("no AVX-512 IFMA on this CPU")
    return got


def _check(api, site, reps, what):
    enc, ident = _run(api, site, reps)
    want = _expect(reps)
    for i, r in enumerate(reps):
        where = (what, site, r["name"], TC.TORSION[r["t"]][0], r["z"], i)
        assert enc[i].tobytes() == r["expect"], where
        assert ident[i] == (1 if r["identity"] else 0), where
    assert (enc == want).all()


@pytest.fixture(scope="module")
def api(hiplib):
    from rofl_project_code_amd import api
    return api


# ---------------------------------------------------------------- the corpus itself
def test_torsion_points_have_orders_1_2_4_4():
    for (name, xy), order in zip(TC.TORSION, TC.TORSION_ORDERS):
        x, y = xy
        assert (y * y - x * x - 1 - pyref.D * x * x % P * y * y) % P == 0, name      # on the curve
        acc, n = TC.ext(xy), 1
        while TC.affine(acc) != (0, 1):
            acc, n = pyref.pt_add(acc, TC.ext(xy)), n + 1
            assert n <= 4, name
        assert n == order, name


def test_every_cell_is_filled_and_sums_to_its_representative():
    cells = TC.tuples()
    assert N_CLASSES == 6 + len(BM.TABLE_SIZES) + 1 and TC.EXTRACT_M in BM.TABLE_SIZES
    want = {(name, t, arity) for name, _ in TC.classes() for t in range(4) for arity in (2, 3) if not TC.impossible(name, t, arity)}
    assert set(cells) == want and len(want) == 8 * N_CLASSES - 2
    assert [k for k in sorted(want) if k[0] == "0" and k[2] == 2] == [("0", 2, 2), ("0", 3, 2)]
    for (name, t, arity), encs in cells.items():
        K = TC.class_point(name)
        assert len(encs) == arity
        total = None
        for e in encs:
            assert len(e) == 32 and e != TC.ZERO32, (name, t, arity)
            pt = pyref.ristretto_decode(e)
            assert pt is not None and pyref.ristretto_encode(pt) == e, (name, t, arity)
            total = pt if total is None else pyref.pt_add(total, pt)
        assert TC.affine(total) == TC.shifted(K, t), (name, t, arity)
        assert pyref.ristretto_encode(total) == TC.expected(name), (name, t, arity)
    assert TC.tuples() is cells      # built once, shared


def test_two_decoded_points_never_cancel_to_0_1_or_0_minus_1():
    """decode(enc(P)) + decode(enc(-P)) over 40 seeded P: always (i, 0) or (-i, 0), and both occur"""
    seen = set()
    for pt, enc, dec in TC._pool() + [(TC.mul_base(v),) * 3 for v in range(1, 17)]:
        a = pyref.ristretto_decode(pyref.ristretto_encode(pt))
        b = pyref.ristretto_decode(pyref.ristretto_encode(pyref.pt_neg(pt)))
        t = TC.which_torsion(pyref.pt_add(a, b), pyref.IDENT)
        assert t in (2, 3)
        seen.add(t)
    assert seen == {2, 3}


def test_raw_representatives_are_the_class_in_the_model():
    assert len(REPS) == N_CLASSES * 4 * 3
    assert TC.expected("0") == TC.ZERO32 and sum(1 for r in REPS if r["identity"]) == 12
    for r in REPS:
        X, Y, Z, T = TC.rep_point(r)
        assert Z != 0 and X * Y % P == Z * T % P, r["name"]
        assert (Y * Y - X * X - Z * Z - pyref.D * T * T) % P == 0, r["name"]      # -x^2 + y^2 = 1 + d x^2 y^2, projectively
        assert TC.affine((X, Y, Z, T)) == TC.shifted(TC.class_point(r["name"]), r["t"])
        assert pyref.ristretto_encode((X, Y, Z, T)) == r["expect"] == pyref.ristretto_encode(TC.class_point(r["name"]))
        if r["identity"]:
            assert X == 0 or Y == 0
        else:
            assert X != 0 and Y != 0
    assert {r["z"] for r in REPS} == set(TC.Z_KINDS) and all(TC.rep_point(r)[2] == 1 for r in REPS if r["z"] == "1")


# ---------------------------------------------------------------- sites 1 .. 4
@pytest.mark.parametrize("site", [1, 2, 3, 4])
def test_host_site_encodes_every_representative_as_the_model(api, site):
    """every (class, T, Z) case, in corpus order (site 4: 21 batches of eight consecutive cases)"""
    _check(api, site, REPS, "corpus order")


def _ident(t, z):
    return next(r for r in REPS if r["identity"] and r["t"] == t and r["z"] == z)


def _generic(k):
    g = [r for r in REPS if not r["identity"]]
    return g[(37 * k) % len(g)]


def test_eight_lane_encoder_lane_arrangements(api):
    """h8::encode8 selects per lane: all eight lanes torsion identities; identity-class and generic lanes alternating (both phases); a
    single (i, 0) lane among seven generic ones, in each of the eight lanes"""
    all_ident = [_ident(t, z) for z in ("1", "random") for t in range(4)]
    assert len(all_ident) == 8
    _check(api, 4, all_ident, "eight identities")
    for phase in (0, 1):
        lanes = [_ident(l // 2 % 4, "7") if l % 2 == phase else _generic(l) for l in range(16)]
        _check(api, 4, lanes, "alternating, phase %d" % phase)
    for z in TC.Z_KINDS:
        for lane in range(8):
            lanes = [_ident(2, z) if l == lane else _generic(11 * lane + l) for l in range(8)]
            assert sum(r["identity"] for r in lanes) == 1
            _check(api, 4, lanes, "(i, 0) alone in lane %d" % lane)
    _check(api, 4, REPS[:13], "a short last batch")
    assert len(REPS) % 8 != 0      # (and so has the whole corpus)


def test_encode_reps_refuses_bad_parameters(api, hiplib):
    sz = ctypes.c_size_t
    good = _xyzt(REPS[:2]).copy()
    out, ident = np.zeros((2, 32), np.uint8), np.zeros(2, np.uint8)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)      # noqa: E731
    call = hiplib.rofl_dbg_encode_reps
    assert call(ctypes.c_uint(1), sz(2), p(good), p(out), p(ident)) == 0
    assert call(ctypes.c_uint(5), sz(2), p(good), p(out), p(ident)) == 11
    assert call(ctypes.c_uint(1), sz((1 << 20) + 1), p(good), p(out), p(ident)) == 11
    for args in ((None, p(out), p(ident)), (p(good), None, p(ident)), (p(good), p(out), None)):
        assert call(ctypes.c_uint(2), sz(2), *args) == 11
    for coord in range(4):
        for value in (P, P + 18, 2 ** 255, 2 ** 256 - 1):      # p, 2^255 - 1, bit 255 alone, all ones
            bad = good.copy()
            bad[1, 32 * coord:32 * coord + 32] = np.frombuffer(value.to_bytes(32, "little"), np.uint8)
            for site in (1, 2, 3):
                assert call(ctypes.c_uint(site), sz(2), p(bad), p(out), p(ident)) == 11, (coord, value, site)
    edge = good.copy()      # p - 1 is canonical: accepted (the point is not on the curve, which is the caller's business)
    edge[1, :32] = np.frombuffer((P - 1).to_bytes(32, "little"), np.uint8)
    assert call(ctypes.c_uint(2), sz(2), p(edge), p(out), p(ident)) == 0


# ---------------------------------------------------------------- the BSGS model against the oracle
def _points(vs):
    return np.frombuffer(b"".join(pyref.ristretto_encode(TC.mul_base(v)) for v in vs), np.uint8).reshape(-1, 32)


def _scalar(v):
    return np.frombuffer((v % BM.L).to_bytes(32, "little"), np.uint8)


@pytest.mark.parametrize("m,bits", [c for c in BM.CASES if c[1] != 32])
def test_bsgs_model_agrees_with_the_oracle_at_the_edges(m, bits):
    vs = BM.values(m, bits, TC.decode_shift)
    want = [BM.solve(v, m, bits) for v in vs]
    found = [v for v, w in zip(vs, want) if w is not None]
    assert len(found) >= 7 and len(found) < len(vs)      # (a table of 2^bits entries finds 0 .. m and nothing else)
    rc, out = orc.bsgs_solve(_points(found), m, bits)
    assert rc == 0
    for v, row in zip(found, out):
        assert int.from_bytes(row.tobytes(), "little") == BM.solve(v, m, bits), v
    for v in [v for v, w in zip(vs, want) if w is None][:3]:
        assert orc.bsgs_solve(_points([v]), m, bits)[0] == 11, v
    assert BM.solve(BM.unreachable(m, bits), m, bits) is None and BM.solve(-BM.unreachable(m, bits), m, bits) is None


@pytest.mark.parametrize("m", [100, 128, 256])
def test_bsgs_model_agrees_with_the_oracle_everywhere_at_8_bits(m):
    """every v of [-(2^8 + m + 2), 2^8 + m + 2]: found values in one oracle call, and each None on its own"""
    vs = list(range(-(256 + m + 2), 256 + m + 3))
    want = [BM.solve(v, m, 8) for v in vs]
    found = [v for v, w in zip(vs, want) if w is not None]
    rc, out = orc.bsgs_solve(_points(found), m, 8)
    assert rc == 0
    assert [int.from_bytes(r.tobytes(), "little") for r in out] == [BM.solve(v, m, 8) for v in found]
    for v, w in zip(vs, want):
        if w is None:
            assert orc.bsgs_solve(_points([v]), m, 8)[0] == 11, v


def test_bsgs_model_is_the_logarithm_where_nothing_wraps():
    """below max_it m with m < 2^bits the walk returns v itself, and -v comes back as l - v; the wraps are as the reference's casts make them"""
    for m, bits in BM.CASES:
        mi = BM.max_it(m, bits)
        if m < (1 << bits):
            for v in (0, 1, m - 1, m, m + 1, (mi - 1) * m + m - 1):
                if v < (1 << bits):
                    assert BM.solve(v, m, bits) == v and BM.solve(-v, m, bits) == (-v) % BM.L, (m, bits, v)
    assert BM.solve(1 << 16, 1 << 15, 16) == 0            # found in the entry x = m at the last iteration: (m + m) mod 2^16
    assert BM.solve(1 << 16, 1 << 16, 16) == 0            # m as u16 = 0: the entry x = m holds 0 and the step is the identity
    assert BM.solve((1 << 16) + 1, 1 << 16, 16) is None   # ... so nothing above m is ever found
    assert BM.solve(200, 100, 8) == 200 and BM.solve(201, 100, 8) is None
    assert BM.solve(1 << 32, 1 << 20, 32) == 0 and BM.solve((1 << 32) - 1, 1 << 20, 32) == (1 << 32) - 1


@pytest.mark.parametrize("m,bits", BM.CASES)
def test_giant_step_inputs_meet_three_representatives(m, bits):
    """a condition on the GPU test's inputs: over the points +-j m B the decoder hands the walker at least three different T"""
    js, seen = BM.giant_steps(m, bits, TC.decode_shift)
    assert {1, 2} <= set(js) and (BM.max_it(m, bits) - 1 in js or BM.max_it(m, bits) <= 1)
    assert len(seen) >= 3, (js, seen)
    vs = BM.values(m, bits, TC.decode_shift)
    assert all(j * m in vs and -j * m in vs for j in js)
    assert len({v % BM.L for v in vs}) == len(vs)
