"""CPU-only checks of the device-resident round's interface (rofl_round_*, rofl_dbg_point_decodes, DeviceRound): the symbols are
exported and declared, every parameter check answers 11 before a device is touched, and the Python class has the documented API.  The GPU
behaviour is in test_gpu_round.py."""
import inspect
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROUND_FUNCS = ("rofl_round_create", "rofl_round_ingest", "rofl_round_verify_sigma", "rofl_round_verify_range", "rofl_round_accumulate",
               "rofl_round_reset", "rofl_round_destroy")


def test_round_symbols_are_exported_and_declared(hiplib):
    hdr = open(os.path.join(ROOT, "include", "rofl_zk.h")).read()
    dbg = open(os.path.join(ROOT, "include", "rofl_zk_debug.h")).read()
    ffi = open(os.path.join(ROOT, "integration", "rofl_crypto_overlay", "src", "ffi.rs")).read()
    for n in ROUND_FUNCS:
        assert hasattr(hiplib, n), n
        assert n + "(" in hdr and "fn " + n + "(" in ffi, n
    assert hasattr(hiplib, "rofl_dbg_point_decodes") and "rofl_dbg_point_decodes(" in dbg


def test_round_parameter_checks_need_no_device(hiplib):
    """Each bad parameter is 11 (ROFL_BAD_PARAM), checked before the device is touched: run in a child process that sees no GPU."""
    code = r"""
import ctypes
L = ctypes.CDLL(%r)
sz, u64, p = ctypes.c_size_t, ctypes.c_uint64, ctypes.c_void_p
h = ctypes.c_uint64(0)
ok = (ctypes.c_int * 4)(7, 7, 7, 7); seed = bytes(32); first = sz(99)
rec = ctypes.create_string_buffer(96 * 8); recs = (p * 1)(ctypes.addressof(rec)); prf = (p * 1)(ctypes.addressof(rec))
acc = (ctypes.c_int * 1)(1)
cnt = ctypes.c_uint64(123)
rcs = {
    "create d = 0": L.rofl_round_create(sz(0), sz(64), sz(4), ctypes.byref(h)),
    "create record_len 32": L.rofl_round_create(sz(8), sz(32), sz(4), ctypes.byref(h)),
    "create record_len 65": L.rofl_round_create(sz(8), sz(65), sz(4), ctypes.byref(h)),
    "create max_clients 0": L.rofl_round_create(sz(8), sz(96), sz(0), ctypes.byref(h)),
    "create null out": L.rofl_round_create(sz(8), sz(64), sz(4), None),
    "create size overflows": L.rofl_round_create(sz(1 << 40), sz(96), sz(1 << 30), ctypes.byref(h)),
    "create too many clients": L.rofl_round_create(sz(8), sz(64), sz(1 << 20), ctypes.byref(h)),
    "ingest unknown handle": L.rofl_round_ingest(u64(12345), sz(1), recs, ctypes.byref(first)),
    "ingest handle 0": L.rofl_round_ingest(u64(0), sz(1), recs, None),
    "ingest null records": L.rofl_round_ingest(u64(1), sz(3), None, None),
    "sigma unknown handle": L.rofl_round_verify_sigma(u64(12345), 0, prf, ok, None),
    "sigma handle 0": L.rofl_round_verify_sigma(u64(0), 1, prf, ok, None),
    "sigma null ok_out": L.rofl_round_verify_sigma(u64(1), 0, prf, None, None),
    "sigma null proofs": L.rofl_round_verify_sigma(u64(1), 0, None, ok, None),
    "sigma kind 3": L.rofl_round_verify_sigma(u64(1), 3, prf, ok, None),
    "range unknown handle": L.rofl_round_verify_range(u64(12345), prf, sz(608), sz(1), sz(8), sz(8), 16, 7, seed, ok),
    "range handle 0": L.rofl_round_verify_range(u64(0), prf, sz(608), sz(1), sz(8), sz(8), 16, 7, seed, ok),
    "range null ok_out": L.rofl_round_verify_range(u64(1), prf, sz(608), sz(1), sz(8), sz(8), 16, 7, seed, None),
    "range null proofs": L.rofl_round_verify_range(u64(1), None, sz(608), sz(1), sz(8), sz(8), 16, 7, seed, ok),
    "range null seed": L.rofl_round_verify_range(u64(1), prf, sz(608), sz(1), sz(8), sz(8), 16, 7, None, ok),
    "accumulate unknown round": L.rofl_round_accumulate(u64(12345), u64(1), acc),
    "accumulate handle 0": L.rofl_round_accumulate(u64(0), u64(0), None),
    "reset unknown": L.rofl_round_reset(u64(5)),
    "reset 0": L.rofl_round_reset(u64(0)),
    "destroy unknown": L.rofl_round_destroy(u64(5)),
    "destroy 0": L.rofl_round_destroy(u64(0)),
    "decode counter null": L.rofl_dbg_point_decodes(None),
}
bad = {k: v for k, v in rcs.items() if v != 11}
assert not bad, bad
assert h.value == 0 and list(ok) == [7, 7, 7, 7] and first.value == 99
assert L.rofl_dbg_point_decodes(ctypes.byref(cnt)) == 0 and cnt.value == 0      # nothing was handed to a device
print("round params ok", len(rcs))
""" % hiplib._name
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")      # whatever the host has: no device is reachable
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "round params ok 27" in r.stdout, r.stdout + r.stderr[-2000:]


def test_device_round_has_the_documented_api():
    import rofl_project_code_amd as R
    from rofl_project_code_amd import api, params
    D = R.DeviceRound
    assert D is params.DeviceRound
    for name in ("ingest", "verify", "accumulate_into", "reset", "close", "__enter__", "__exit__", "__del__", "__len__"):
        assert callable(getattr(D, name, None)), name
    assert list(inspect.signature(D.__init__).parameters) == ["self", "cls", "size", "max_clients"]
    sig = inspect.signature(D.verify).parameters
    assert list(sig) == ["self", "verifier_seed", "fp"] and sig["verifier_seed"].default is None and sig["fp"].default is None
    sig = inspect.signature(D.accumulate_into).parameters
    assert list(sig) == ["self", "acc", "accept"] and sig["accept"].default is None
    for name in ("create", "ingest", "verify_sigma", "verify_range", "accumulate", "reset", "destroy"):
        assert callable(getattr(api.device_round, name, None)), name
    assert callable(api.point_decodes)
    # the batched verification of the containers is unchanged for its callers: the legs' source is a private keyword with the host default
    for cls in (R.EncParamsRange, R.EncParamsRangeCompressed, R.EncParamsL2, R.EncParamsL2Compressed):
        p = inspect.signature(cls.verify_batch).parameters
        assert list(p) == ["updates", "verifier_seed", "fp", "_legs"] and p["_legs"].default is params._HostLegs
    try:
        D(R.EncModelParamsAccumulator, 8, 2)
    except ValueError:
        pass
    else:
        raise AssertionError("a class that is not an update container was accepted")
