"""CPU-only checks of the interface of the two batched create legs (rofl_create_sigmaproof_vec_batch, rofl_create_rangeproof_l2_batch and
their Python wrappers): the symbols are exported and declared, every whole-call parameter error answers 11 before a device is touched,
and the Python side has the documented signatures.  The GPU behaviour is in test_gpu_sigma_create_batch.py,
test_gpu_l2_create_batch.py and test_gpu_encrypt_batch_l2.py."""
import inspect
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FNS = ("rofl_create_sigmaproof_vec_batch", "rofl_create_rangeproof_l2_batch")
OVERLAY = os.path.join(ROOT, "integration", "rofl_crypto_overlay", "src")


def test_symbols_are_exported_and_declared(hiplib):
    hdr = open(os.path.join(ROOT, "include", "rofl_zk.h")).read()
    ffi = open(os.path.join(OVERLAY, "ffi.rs")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for fn in FNS:
        assert hasattr(hiplib, fn), fn
        assert "int " + fn + "(" in hdr and "fn " + fn + "(" in ffi and fn in doc, fn
    for mod, wrapper in (("rand_proof_vec", "create_randproof_vec_batch"), ("square_rand_proof_vec", "create_l2rangeproof_vec_batch"),
                         ("square_proof_vec", "create_l2rangeproof_vec_batch"), ("l2_range_proof_vec", "create_rangeproof_l2_batch")):
        assert "pub fn " + wrapper + "(" in open(os.path.join(OVERLAY, mod, "mod.rs")).read(), mod


def _run(hiplib, code, marker):
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")      # whatever the host has: no device is reachable
    r = subprocess.run([sys.executable, "-c", code % hiplib._name], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and marker in r.stdout, r.stdout + r.stderr[-2000:]


PRELUDE = r"""
import ctypes
L = ctypes.CDLL(%r)
sz, p = ctypes.c_size_t, ctypes.c_void_p
class N(ctypes.Structure):
    _fields_ = [("mode", ctypes.c_int), ("stream", p), ("stream_scalars", sz), ("seed", ctypes.c_ubyte * 32)]
n, d = 2, 4
arr = lambda bufs: (p * len(bufs))(*[ctypes.addressof(b) for b in bufs])
hole = lambda bufs: (p * len(bufs))(ctypes.addressof(bufs[0]), None)
vals = [(ctypes.c_float * d)() for _ in range(n)]; rs = [ctypes.create_string_buffer(32 * d) for _ in range(n)]; r2 = [ctypes.create_string_buffer(32 * d) for _ in range(n)]
ns = (N * n)(); ns[0].mode = ns[1].mode = 1
nostream = (N * n)(); nostream[0].mode = 1; nostream[1].mode = 0; nostream[1].stream_scalars = 100      # a stream announced and not given
rc = (ctypes.c_int * n)(7, 7)
def decodes():
    cnt = ctypes.c_uint64(123)
    assert L.rofl_dbg_point_decodes(ctypes.byref(cnt)) == 0
    return cnt.value
"""


def test_sigma_parameter_checks_need_no_device(hiplib):
    """Each whole-call parameter error is 11 (ROFL_BAD_PARAM), n_clients = 0 is 0 and d = 0 is 0 with every rc_out[i] = 0, all decided
    before the device is touched: run in a child process that sees no GPU."""
    code = PRELUDE + r"""
prf = [ctypes.create_string_buffer(192 * d) for _ in range(n)]; cms = [ctypes.create_string_buffer(96 * d) for _ in range(n)]
V, A, B, P, C = arr(vals), arr(rs), arr(r2), arr(prf), arr(cms)
F = L.rofl_create_sigmaproof_vec_batch
call = lambda kind=1, nc=n, v=V, dd=d, a=A, b=B, e=None, fb=16, ff=7, nn=ns, po=P, co=C, ro=rc: F(kind, sz(nc), v, sz(dd), a, b, e, fb, ff, nn, po, co, ro)
rcs = {
    "kind -1": call(kind=-1), "kind 3": call(kind=3),
    "d far too large": call(dd=1 << 40),
    "null values": call(v=None), "null r1": call(a=None), "null r2, kind 1": call(b=None), "null r2, kind 2": call(kind=2, b=None),
    "null r2, kind 1, d = 0": call(b=None, dd=0),
    "null nonces": call(nn=None), "null proofs_out": call(po=None), "null commits_out": call(co=None), "null rc_out": call(ro=None),
    "null values[1]": call(v=hole(vals)), "null r1[1]": call(a=hole(rs)), "null r2[1]": call(b=hole(r2)),
    "null proofs_out[1]": call(po=hole(prf)), "null commits_out[1]": call(co=hole(cms)), "a stream that is not there": call(nn=nostream),
    "fp_bits 12": call(fb=12), "fp_frac 13": call(ff=13), "fp_frac >= fp_bits": call(fb=8, ff=8),
    "65 536 clients": call(nc=65536), "65 536 clients, d = 0": call(nc=65536, dd=0),
    "d = 0, null nonces": call(dd=0, nn=None), "d = 0, null rc_out": call(dd=0, ro=None),
}
bad = {k: v for k, v in rcs.items() if v != 11}
assert not bad, bad
assert list(rc) == [7, 7] and not any(prf[0].raw) and not any(cms[0].raw)
assert call(nc=0) == 0 and call(nc=0, v=None, a=None, b=None, nn=None, po=None, co=None, ro=None) == 0 and call(nc=0, dd=0) == 0
assert list(rc) == [7, 7]
assert call(kind=0, b=None, dd=0, v=None, a=None, po=None, co=None) == 0 and list(rc) == [0, 0]      # d = 0: nothing to prove, every client 0
assert decodes() == 0
print("sigma create batch params ok", len(rcs))
"""
    _run(hiplib, code, "sigma create batch params ok 25")


def test_l2_parameter_checks_need_no_device(hiplib):
    code = PRELUDE + r"""
prf = [ctypes.create_string_buffer(32 * 23) for _ in range(n)]; com = ctypes.create_string_buffer(32 * n)
V, A, P = arr(vals), arr(rs), arr(prf)
plen = sz(99)
F = L.rofl_create_rangeproof_l2_batch
call = lambda nc=n, v=V, dd=d, a=A, pr=32, npart=1, fb=32, ff=7, nn=ns, po=P, pl=ctypes.byref(plen), co=com, ro=rc: F(sz(nc), v, sz(dd), a, sz(pr), sz(npart), fb, ff, nn, po, pl, co, ro)
rcs = {
    "d = 0": call(dd=0), "d far too large": call(dd=1 << 40), "n_partition = 0": call(npart=0), "prove_range = 0": call(pr=0),
    "null values": call(v=None), "null blindings": call(a=None), "null nonces": call(nn=None), "null proofs_out": call(po=None),
    "null proof_len_out": call(pl=None), "null commits_out": call(co=None), "null rc_out": call(ro=None),
    "null values[1]": call(v=hole(vals)), "null blindings[1]": call(a=hole(rs)), "null proofs_out[1]": call(po=hole(prf)),
    "a stream that is not there": call(nn=nostream),
    "fp_bits 12": call(fb=12), "fp_frac 13": call(ff=13), "fp_frac >= fp_bits": call(fb=8, ff=8),
    "32 768 clients": call(nc=32768),
}
bad = {k: v for k, v in rcs.items() if v != 11}
assert not bad, bad
assert list(rc) == [7, 7] and plen.value == 99 and not any(prf[0].raw) and not any(com.raw)
assert call(nc=0) == 0 and list(rc) == [7, 7]
assert decodes() == 0
print("l2 create batch params ok", len(rcs))
"""
    _run(hiplib, code, "l2 create batch params ok 19")


def test_python_side_has_the_documented_signatures():
    import rofl_project_code_amd as R
    from rofl_project_code_amd import api
    p = inspect.signature(api.rand_proof_vec.create_randproof_vec_batch).parameters
    assert list(p) == ["values_list", "random_list", "nonces", "existing_list", "fp"]
    assert all(p[k].default is None for k in ("nonces", "existing_list", "fp"))
    assert api.rand_proof_vec.create_randproof_vec_batch([], []) == []
    for cls in (api.square_rand_proof_vec, api.square_proof_vec):
        p = inspect.signature(cls.create_l2rangeproof_vec_batch).parameters
        assert list(p) == ["values_list", "random_list", "random2_list", "nonces", "existing_list", "fp"], cls
        assert all(p[k].default is None for k in ("nonces", "existing_list", "fp"))
        assert cls.create_l2rangeproof_vec_batch([], [], []) == []
    p = inspect.signature(api.l2_range_proof_vec.create_rangeproof_l2_batch).parameters
    assert list(p) == ["values_list", "blindings_list", "prove_range", "n_partition", "nonces", "fp"]
    assert p["nonces"].default is None and p["fp"].default is None
    assert api.l2_range_proof_vec.create_rangeproof_l2_batch([], [], 32, 1) == []
    # the containers keep their signatures; the compressed kind keeps its own randomness leg
    q = inspect.signature(R.EncParamsL2.encrypt_batch).parameters
    assert list(q) == ["clients", "prove_range", "n_partition", "l2_range", "nonce_seeds", "fp"]
    assert list(inspect.signature(R.EncParamsL2Compressed.encrypt_batch).parameters) == list(q)
    assert R.EncParamsL2.encrypt_batch([], 8, 2, 32) == [] and R.EncParamsL2Compressed.encrypt_batch([], 8, 2, 32) == []
    assert R.EncParamsRangeCompressed._rand_create_batch is not R.EncParamsRange._rand_create_batch


def test_header_and_ffi_agree():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "check_ffi.py")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
