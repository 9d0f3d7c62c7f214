"""CPU-only checks of the compressed randomness leg of the device-resident round (rofl_round_create_ex, rofl_round_verify_compressed,
api.device_round.verify_compressed, DeviceRound): the symbols are exported and declared, every parameter check answers 11 before a device
is touched, and the Python layer has the documented signatures.  The GPU behaviour is in test_gpu_round_compressed.py."""
import inspect
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_FUNCS = ("rofl_round_create_ex", "rofl_round_verify_compressed")


def test_compressed_round_symbols_are_exported_and_declared(hiplib):
    hdr = open(os.path.join(ROOT, "include", "rofl_zk.h")).read()
    ffi = open(os.path.join(ROOT, "integration", "rofl_crypto_overlay", "src", "ffi.rs")).read()
    for n in NEW_FUNCS:
        assert hasattr(hiplib, n), n
        assert n + "(" in hdr and "fn " + n + "(" in ffi, n
    assert "#define ROFL_ROUND_COMPRESSED 1" in hdr
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "check_ffi.py")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and " 0 differences" in r.stdout, r.stdout + r.stderr


def test_compressed_round_parameter_checks_need_no_device(hiplib):
    """Each bad parameter is 11 (ROFL_BAD_PARAM), answered before the device is touched: run in a child process that sees no GPU."""
    code = r"""
import ctypes
L = ctypes.CDLL(%r)
sz, u64, p, un = ctypes.c_size_t, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint
h = ctypes.c_uint64(0)
ok = (ctypes.c_int * 4)(7, 7, 7, 7)
buf = ctypes.create_string_buffer(128); prf = (p * 1)(ctypes.addressof(buf))
cnt = ctypes.c_uint64(123)
rcs = {
    "create_ex flag 1, record_len 96": L.rofl_round_create_ex(sz(8), sz(96), sz(4), un(1), ctypes.byref(h)),
    "create_ex flag 1, d = 900000": L.rofl_round_create_ex(sz(900000), sz(64), sz(4), un(1), ctypes.byref(h)),
    "create_ex flag 2": L.rofl_round_create_ex(sz(8), sz(64), sz(4), un(2), ctypes.byref(h)),
    "create_ex flag 3": L.rofl_round_create_ex(sz(8), sz(64), sz(4), un(3), ctypes.byref(h)),
    "create_ex flag 1 << 31": L.rofl_round_create_ex(sz(8), sz(64), sz(4), un(1 << 31), ctypes.byref(h)),
    "create_ex null out": L.rofl_round_create_ex(sz(8), sz(64), sz(4), un(1), None),
    "create_ex null out, flag 0": L.rofl_round_create_ex(sz(8), sz(64), sz(4), un(0), None),
    "create_ex d = 0": L.rofl_round_create_ex(sz(0), sz(64), sz(4), un(1), ctypes.byref(h)),
    "create_ex record_len 32": L.rofl_round_create_ex(sz(8), sz(32), sz(4), un(0), ctypes.byref(h)),
    "create_ex max_clients 0": L.rofl_round_create_ex(sz(8), sz(64), sz(0), un(1), ctypes.byref(h)),
    "create_ex too many clients": L.rofl_round_create_ex(sz(8), sz(64), sz(1 << 20), un(1), ctypes.byref(h)),
    "verify_compressed handle 0": L.rofl_round_verify_compressed(u64(0), prf, ok),
    "verify_compressed unknown handle": L.rofl_round_verify_compressed(u64(12345), prf, ok),
    "verify_compressed null proofs": L.rofl_round_verify_compressed(u64(1), None, ok),
    "verify_compressed null ok_out": L.rofl_round_verify_compressed(u64(1), prf, None),
}
bad = {k: v for k, v in rcs.items() if v != 11}
assert not bad, bad
assert h.value == 0 and list(ok) == [7, 7, 7, 7]
assert L.rofl_dbg_point_decodes(ctypes.byref(cnt)) == 0 and cnt.value == 0      # nothing was handed to a device
print("compressed round params ok", len(rcs))
""" % hiplib._name
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")      # whatever the host has: no device is reachable
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "compressed round params ok 15" in r.stdout, r.stdout + r.stderr[-2000:]


def test_python_layer_has_the_documented_signatures():
    import rofl_project_code_amd as R
    from rofl_project_code_amd import api
    p = inspect.signature(api.device_round.create).parameters
    assert list(p) == ["d", "record_len", "max_clients", "flags"] and p["flags"].default == 0
    assert list(inspect.signature(api.device_round.verify_compressed).parameters) == ["h", "proofs"]
    assert api.device_round.COMPRESSED == 1
    D = R.DeviceRound
    assert list(inspect.signature(D.__init__).parameters) == ["self", "cls", "size", "max_clients"]
    assert list(inspect.signature(D.rand).parameters) == ["self", "cls", "us", "idx"]
    doc = " ".join(D.__doc__.split())
    assert "rofl_round_verify_compressed" in doc and "keeps its randomness leg on rofl_verify_compressed_randproof_batch" not in doc
