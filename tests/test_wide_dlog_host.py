"""CPU-only checks of the wide discrete-log widths (bsgs_bits 24 and 40): which (table_size, bsgs_bits) pairs pass the parameter check, in
a child process that sees no GPU, and the plain-integer reference tests/test_gpu_wide_dlog.py leans on."""
import os
import subprocess
import sys

import bsgs_model as BM


def test_widths_24_and_40_pass_the_parameter_check(hiplib):
    """valid wide calls get past the check and fail at the missing device (>= 100); other widths and tables of 2^bits or more are 11"""
    code = r"""
import ctypes
L = ctypes.CDLL(%r)
sz = ctypes.c_size_t
pts = ctypes.create_string_buffer(64); out = ctypes.create_string_buffer(64)
log = lambda m, bits: L.rofl_discrete_log_vec(pts, sz(2), sz(m), bits, out)
reach = {"24": log(1 << 10, 24), "24 odd": log(3000, 24), "40": log(1 << 20, 40), "24 largest": log((1 << 24) - 1, 24)}
refuse = {"12": log(1 << 10, 12), "48": log(1 << 20, 48), "24 table 2^24": log(1 << 24, 24), "24 table 2^25": log(1 << 25, 24),
          "40 table 2^30": log(1 << 30, 40)}
assert all(v >= 100 for v in reach.values()), reach
assert all(v == 11 for v in refuse.values()), refuse
print("wide params ok", len(reach), len(refuse))
""" % hiplib._name
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "wide params ok 4 5" in r.stdout, r.stdout + r.stderr[-2000:]


def test_the_model_returns_the_plain_logarithm_at_width_24():
    for m in (1 << 10, 3000):
        reach = BM.max_it(m, 24) * m
        for v in (0, 1, m, m + 1, 70000, 115200, reach - 1, reach):
            assert BM.solve(v, m, 24) == v % (1 << 24) and BM.solve(-v, m, 24) == -(v % (1 << 24)) % BM.L, (m, v)
        assert BM.solve(reach + 1, m, 24) is None and BM.solve(-reach - 1, m, 24) is None
    assert BM.solve(70000, 1 << 10, 16) is None and BM.solve(65536, 1 << 10, 16) == 0
