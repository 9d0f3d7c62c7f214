"""The kernels' field, point and scalar arithmetic (csrc/fe26.hpp, the sc_* of csrc/fe32.hpp) at the limb bounds, on the host build of the
same source -- the build in which fd_mul / fd_sq assert their operand bounds.  Reference and corpus: tests/fd_model.py (plain integers).
All comparisons are integers: equality is exact, and no corpus case is skipped on any path."""
import ctypes

import numpy as np
import pytest

import fd_model as m

sz = ctypes.c_size_t


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def host_fd(lib, op, cases):
    out = np.full((len(cases), m.FD_OUT), 0xdeadbeef, np.uint32)
    assert lib.rofl_dbg_host_fd_ops_raw(ctypes.c_uint(op), sz(len(cases)), _ptr(cases), _ptr(out)) == 0
    return out


def host_sc(lib, op, cases):
    out = np.full((len(cases), m.SC_OUT), 0xdeadbeef, np.uint32)
    assert lib.rofl_dbg_host_sc_ops(ctypes.c_uint(op), sz(len(cases)), _ptr(cases), _ptr(out)) == 0
    return out


@pytest.mark.parametrize("op", range(24), ids=m.FD_OP_NAMES)
def test_corpus_lies_inside_the_contract(op):
    """The model's bound checker over the whole corpus: no u32 / u64 wrap and no violated precondition of the header, so a corpus case is
    never the reason for a host assertion or a mismatch.  Counts are no multiple of a quad or of the block size."""
    cases = m.fd_corpus(op)
    assert 50 < len(cases) < 5000 and len(cases) % 4 != 0 and len(cases) % 256 != 0
    assert (cases == m.fd_corpus(op)).all()          # deterministic
    for case in cases:
        m.limbs(op, case)                            # raises BoundError


def test_bound_checker_flags_what_leaves_the_contract():
    """the checker is not vacuous: one step past each documented bound is flagged"""
    mx = [t - 1 for t in m.TIGHT]
    for bad in (lambda: m.l_mul([m.MUL_F_MAX] + [0] * 9, mx), lambda: m.l_mul(mx, [m.G19_MAX + 1] + [0] * 9),
                lambda: m.l_sq([m.G19_MAX + 1] + [0] * 9), lambda: m.l_sq([0, m.G38_MAX + 1] + [0] * 8),
                lambda: m.l_sub(mx, [m.TIGHT[0]] + [0] * 9), lambda: m.l_add([2 ** 31] * 10, [2 ** 31] * 10),
                lambda: m.l_carry([m.CARRY_MAX] + [0] * 9),
                lambda: m.l_reduce_cols([2 ** 64 - 1] * 10)):
        with pytest.raises(m.BoundError):
            bad()
    for op in (m.SC_ADD, m.SC_NEG, m.SC_MONTMUL):
        with pytest.raises(m.BoundError):
            case = np.zeros(m.SC_IN, np.uint32); case[:16] = 0xffffffff
            m.sc_expect(op, case)


@pytest.mark.parametrize("op", m.FD_THREAD_OPS, ids=m.FD_OP_NAMES[:22])
def test_host_twin_against_model(hiplib, op):
    """rofl_dbg_host_fd_ops_raw: value mod p of every output, tightness where the header promises it, and the limbs the limb model predicts"""
    cases = m.fd_corpus(op)
    m.check_outputs(op, cases, host_fd(hiplib, op, cases))


def test_host_twin_rejects_quad_ops(hiplib):
    cases = m.fd_corpus(m.GD_DOUBLE)
    out = np.zeros((len(cases), m.FD_OUT), np.uint32)
    for op in (m.GQ_DOUBLE, m.GQ_ADD, 24):
        assert hiplib.rofl_dbg_host_fd_ops_raw(ctypes.c_uint(op), sz(len(cases)), _ptr(cases), _ptr(out)) == 11


@pytest.mark.parametrize("op", range(12), ids=m.SC_OP_NAMES)
def test_host_scalar_ops_against_model(hiplib, op):
    cases = m.sc_corpus(op)
    assert len(cases) % 4 != 0 and len(cases) % 256 != 0
    m.check_sc_outputs(op, cases, host_sc(hiplib, op, cases))


def test_host_scalar_ops_agree_with_the_older_hooks(hiplib):
    """the lazy accumulator and the wide reductions through the hooks test_host_lib.py uses: the same answers as the op table"""
    for op, fn in ((m.SC_FROM_WIDE, hiplib.rofl_dbg_host_sc_wide), (m.SC_FROM_WIDE_MONT, None)):
        cases = m.sc_corpus(op)
        got = host_sc(hiplib, op, cases)
        for case, g in zip(cases, got):
            o = ctypes.create_string_buffer(32)
            if fn is not None:
                assert fn(case[:16].tobytes(), o) == 0 and o.raw == g.tobytes()
            else:
                assert hiplib.rofl_dbg_host_sc_wide_mont(case[:16].tobytes(), o) == 0
                assert int.from_bytes(o.raw, "little") == m.sc_int(g) * m.RINV % m.L
    cases = m.sc_corpus(m.SC_MAC)
    got = host_sc(hiplib, m.SC_MAC, cases)
    for case, g in zip(cases, got):
        count = int(case[256])
        sc = case[:256].reshape(32, 8)
        a, b = sc[0::2][:count].tobytes(), sc[1::2][:count].tobytes()
        o1, o2 = ctypes.create_string_buffer(32), ctypes.create_string_buffer(32)
        assert hiplib.rofl_dbg_host_sc_lazy(a, b, sz(count), o1, o2) == 0
        assert o1.raw == g.tobytes() and o2.raw == g.tobytes()


def _b(x):
    return x.to_bytes(32, "little")


def test_host_fd_ops_on_field_values(hiplib):
    """rofl_dbg_host_fd_ops (bytes in, canonical bytes out; bit 255 reaches fd_unpack) against Python integers on the field-value list"""
    vals = m.FIELD_VALUES + [x + 2 ** 255 for x in m.FIELD_VALUES] + [2 ** 256 - 1]
    for a in vals:
        for b in vals:
            o = [ctypes.create_string_buffer(32) for _ in range(5)]
            assert hiplib.rofl_dbg_host_fd_ops(_b(a), _b(b), *o) == 0
            got = [int.from_bytes(x.raw, "little") for x in o]
            x, y = a % m.P, b % m.P
            assert got == [x * y % m.P, x * x % m.P, (x + y) % m.P, (x - y) % m.P, pow(x, m.P - 2, m.P)], (hex(a), hex(b))


def test_host_fd_scalarmult_on_scalar_values(hiplib):
    """rofl_dbg_host_fd_scalarmult (gd_double, gd_madd of both signs, gd_add, gd_to_niels in a ladder) against the oracle: k P for the
    scalar list -- 0, l - 1, l, l + 1, 2^256 - 1, ... -- and random P"""
    import orc
    rng = np.random.default_rng(2026)
    pts = orc.commit_vec(orc.rand_scalars(rng, 5), None)
    ks = m.SC_VALUES + [int.from_bytes(orc.rand_scalars(rng, 1)[0].tobytes(), "little") for _ in range(3)]
    for p in pts:
        for k in ks:
            o = ctypes.create_string_buffer(32)
            assert hiplib.rofl_dbg_host_fd_scalarmult(_b(k), p.tobytes(), o) == 0
            want = orc.msm(np.frombuffer(_b(k % m.L), np.uint8), p)
            assert o.raw == want.tobytes(), hex(k)
