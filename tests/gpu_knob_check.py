"""Helper of test_gpu_knob_matrix.py, run as a fresh process per case (the knobs are read once per process):
    python tests/gpu_knob_check.py <workload> [<workload> ...]
Runs the named workloads of tests/knob_matrix.py on the GPU under whatever ROFL_* environment it was started with (always with
ROFL_TRACE=1) and prints, per workload, the ITEM / RESULT digest lines that knob_matrix.oracle_lines() computes from the CPU oracle,
plus "WITNESS <name> <int>" lines.  It compares nothing itself: the driver holds the oracle's lines."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
os.environ["ROFL_TRACE"] = "1"
import ctypes

import numpy as np

import knob_matrix as KM
import rofl_project_code_amd as R
from rofl_project_code_amd import api


def say(*a):
    print(*a, flush=True)


def mark(text):
    """a line of the helper's own between the library's trace lines (both unbuffered on fd 2)"""
    sys.stderr.write("[knob-check] %s\n" % text); sys.stderr.flush()


def gpu_msm(k, p):
    out = np.zeros(32, np.uint8)
    rc = R.lib().rofl_dbg_msm(k.ctypes.data_as(ctypes.c_void_p), p.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(k.shape[0]), out.ctypes.data_as(ctypes.c_void_p))
    assert rc == 0, rc
    return out


def run_msm(D, workload):
    for n in KM.msm_sizes(workload):
        pts, fam = KM.msm_inputs(n)
        for name, k in fam.items():
            D.add("n%d/%s" % (n, name), gpu_msm(k, pts))


def run_sigma(D):
    api.set_fp(16, 7)
    verify_msms = 0
    for kind in (0, 1, 2):
        vals, r1, r2, seed = KM.sigma_inputs(kind)
        M = (R.rand_proof_vec, R.square_rand_proof_vec, R.square_proof_vec)[kind]
        if kind == 0:
            pr, cm = M.create_randproof_vec(vals, r1, nonce=R.Nonce.seeded(seed)); ver = M.verify_randproof_vec
        else:
            pr, cm = M.create_l2rangeproof_vec(vals, r1, r2, nonce=R.Nonce.seeded(seed)); ver = M.verify_l2rangeproof_vec
        before = api.msm_retries()["done"]
        ok = ver(pr, cm)
        verify_msms += api.msm_retries()["done"] - before
        D.add("kind%d/proofs" % kind, pr); D.add("kind%d/commits" % kind, cm); D.add("kind%d/verdict" % kind, bool(ok))
    say("WITNESS sigma.verify_msms %d" % verify_msms)


def run_range(D, workload):
    for shape in KM._range_shapes(workload):
        d, nb, P, fb, ff = shape
        api.set_fp(fb, ff)
        vals, bl, seed = KM.range_inputs(shape)
        tag = "%dx%dx%d" % (d, nb, P)
        reps = 3 if workload == "lazy" else 1
        for rep in range(reps):
            if rep:
                time.sleep(KM.LAZY_PAUSE_S)      # longer than ROFL_GENS_LAZY_IDLE_MS: the background build of the full fold table gets its quiet moment
            mark("create %s #%d" % (tag, rep))
            pr, cm = R.range_proof_vec.create_rangeproof(vals, bl, nb, P, nonce=R.Nonce.seeded(seed))
            sfx = "#%d" % rep if workload == "lazy" else ""
            D.add(tag + "/proofs" + sfx, pr); D.add(tag + "/commits" + sfx, cm)
        mark("verify %s" % tag)
        D.add(tag + "/verdict", bool(R.range_proof_vec.verify_rangeproof(pr, cm, nb, verifier_seed=b"\x05" * 32)))
        D.add(tag + "/tampered", bool(R.range_proof_vec.verify_rangeproof(KM.tamper(pr), cm, nb, verifier_seed=b"\x05" * 32)))
    api.set_fp(16, 7)


def main(workloads):
    R.set_device(0)
    L = R.lib()
    for name, fn, args in (("horner8", "rofl_dbg_host_horner8_selftest", (ctypes.c_uint(37), ctypes.c_uint(7), 8, None, None)),
                           ("merlin8", "rofl_dbg_host_merlin8_selftest", (8, ctypes.c_uint(4), ctypes.c_uint(1), None, None))):
        say("SELFTEST %s %d" % (name, getattr(L, fn)(*args)))
    for w in workloads:
        assert w in KM.WORKLOADS, w
        t0 = time.time()
        done0 = api.msm_retries()["done"]
        mark("workload %s" % w)
        D = KM.Digest(w)
        if w in ("msm", "msm5000"):
            run_msm(D, w)
        elif w == "sigma":
            run_sigma(D)
        else:
            run_range(D, w)
        for l in D.lines():
            say(l)
        say("WITNESS %s.msms_done %d" % (w, api.msm_retries()["done"] - done0))
        say("SECONDS %s %.2f" % (w, time.time() - t0))
    for key in ("sigma_batch", "blocking_sync", "verify_batch"):
        say("WITNESS option.%s %d" % (key, api.get_option(key)))
    r = api.msm_retries()
    say("WITNESS retries %d" % (r["small_overflow"] + r["bin_overflow_to_slots"] + r["slot_overflow"]))


if __name__ == "__main__":
    main(sys.argv[1:])
