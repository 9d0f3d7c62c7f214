"""The kernels' field, point and scalar arithmetic at the limb bounds, ON THE DEVICE: rofl_dbg_fd_ops / rofl_dbg_sc_ops (kernels k_dbg_fd,
k_dbg_sc: the op table of csrc/fd_dbg.hpp, one thread -- or one quad of lanes -- per case, one launch per op) against the exact model of
tests/fd_model.py and, bit for bit, against the host build of the same source.  Integers only: equality is exact, no case is skipped."""
import ctypes

import numpy as np
import pytest

import fd_model as m
from test_fd_arith_host import _ptr, host_fd, host_sc, sz

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    import rofl_project_code_amd as R
    from rofl_project_code_amd import build
    build.build()
    R.set_device(0)     # fails loudly when there is no HIP device / library
    return R.lib()


def dev_fd(lib, op, cases):
    out = np.full((len(cases), m.FD_OUT), 0xdeadbeef, np.uint32)
    assert lib.rofl_dbg_fd_ops(ctypes.c_uint(op), sz(len(cases)), _ptr(cases), _ptr(out)) == 0
    return out


@pytest.mark.parametrize("op", m.FD_THREAD_OPS, ids=m.FD_OP_NAMES[:22])
def test_device_field_and_point_ops(lib, op):
    """value mod p and tightness of every device result; its limbs are those of the host twin (one source: a difference would be a
    code-generation finding), words the op does not write included"""
    cases = m.fd_corpus(op)
    got = dev_fd(lib, op, cases)
    m.check_outputs(op, cases, got, with_limb_model=False)
    assert (got == host_fd(lib, op, cases)).all()


@pytest.mark.parametrize("op", (m.GQ_DOUBLE, m.GQ_ADD), ids=("gq_double", "gq_add"))
def test_device_quad_ops(lib, op):
    """csrc/quad26.hpp: one quad of lanes per case against the one-thread gd_* result of the same case (same launch), both against the
    model, and the one-thread half against the host twin's gd_double / gd_add"""
    cases = m.fd_corpus(op)
    got = dev_fd(lib, op, cases)
    m.check_outputs(op, cases, got, with_limb_model=False)
    assert (got[:, :40] == got[:, 40:]).all()
    assert (got[:, 40:] == host_fd(lib, m.GD_DOUBLE if op == m.GQ_DOUBLE else m.GD_ADD, cases)[:, :40]).all()


@pytest.mark.parametrize("op", range(12), ids=m.SC_OP_NAMES)
def test_device_scalar_ops(lib, op):
    cases = m.sc_corpus(op)
    got = np.full((len(cases), m.SC_OUT), 0xdeadbeef, np.uint32)
    assert lib.rofl_dbg_sc_ops(ctypes.c_uint(op), sz(len(cases)), _ptr(cases), _ptr(got)) == 0
    m.check_sc_outputs(op, cases, got)
    assert (got == host_sc(lib, op, cases)).all()


def test_device_hooks_reject_bad_parameters(lib):
    cases = m.fd_corpus(m.NEG)
    out = np.zeros((len(cases), m.FD_OUT), np.uint32)
    assert lib.rofl_dbg_fd_ops(ctypes.c_uint(24), sz(len(cases)), _ptr(cases), _ptr(out)) == 11
    assert lib.rofl_dbg_fd_ops(ctypes.c_uint(0), sz(0), _ptr(cases), _ptr(out)) == 11
    assert lib.rofl_dbg_sc_ops(ctypes.c_uint(12), sz(1), _ptr(cases), _ptr(out)) == 11
