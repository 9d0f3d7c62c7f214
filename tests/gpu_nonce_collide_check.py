"""Helper of test_gpu_nonce_collide.py, run as a fresh process per knob environment (the knobs are read once per process):
    python tests/gpu_nonce_collide_check.py <case id> [<case id> ...]
Proves the named cases of tests/nonce_collide.py on the GPU under whatever ROFL_* environment it was started with and prints, per case,
"PROOF <id> <sha256 of proofs || commitments>", "VERDICT <id> <0 / 1>" (the device verifier on the device's own proof) and
"REPEATS <id> <small> <bin> <slot>" (the deltas of rofl_dbg_msm_retries over the create call).  It compares nothing itself: the driver holds
the oracle's bytes and verdicts."""
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np

import nonce_collide as NC
import rofl_project_code_amd as R
from rofl_project_code_amd import api


def digest(pr, cm):
    return hashlib.sha256(np.ascontiguousarray(pr).tobytes() + np.ascontiguousarray(cm).tobytes()).hexdigest()


def main(ids):
    R.set_device(0)
    api.set_fp(*NC.FP)
    for cid in ids:
        case = NC.case_by_id(cid)
        n, P = case["n"], case["P"]
        vals, bl, stream = NC.case_inputs(case)
        r0 = api.msm_retries()
        pr, cm = R.range_proof_vec.create_rangeproof(vals, bl, n, P, nonce=R.Nonce.stream(stream))
        r1 = api.msm_retries()
        print("PROOF %s %s" % (cid, digest(pr, cm)), flush=True)
        print("VERDICT %s %d" % (cid, int(R.range_proof_vec.verify_rangeproof(pr, cm, n, verifier_seed=b"\x05" * 32))), flush=True)
        print("REPEATS %s %d %d %d" % (cid, r1["small_overflow"] - r0["small_overflow"], r1["bin_overflow_to_slots"] - r0["bin_overflow_to_slots"],
                                        r1["slot_overflow"] - r0["slot_overflow"]), flush=True)


if __name__ == "__main__":
    main(sys.argv[1:])
