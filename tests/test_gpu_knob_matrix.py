"""KNOBS.md promises that a tuning knob "never changes a result".  Every case of tests/knob_matrix.py -- one environment, the few workloads that
reach its path -- runs in a fresh process (tests/gpu_knob_check.py) and must (a) give the CPU oracle's bytes and verdicts, bit for bit, and
(b) show in its ROFL_TRACE=1 lines that the path it names really ran: an unmet witness is a failure, not a skip.  The only skips are the
host-SIMD cases on a CPU without AVX-512 (IFMA), decided by the library's own selftests."""
import functools
import os
import subprocess
import sys
import time

import pytest

import knob_matrix as KM

pytestmark = pytest.mark.gpu
HELPER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "gpu_knob_check.py")


@pytest.fixture(scope="module")
def R():
    import rofl_project_code_amd as R
    from rofl_project_code_amd import build
    build.build()
    R.set_device(0)     # fails loudly when there is no HIP device / library
    return R


@functools.lru_cache(maxsize=None)
def _oracle(workload):
    """the oracle's lines of a workload: computed once per session, shared by every case that runs it"""
    return tuple(KM.oracle_lines(workload))


@pytest.mark.parametrize("case", KM.CASES, ids=[c["id"] for c in KM.CASES])
def test_knob_case_matches_the_oracle_and_takes_its_path(R, case):
    env = {k: v for k, v in os.environ.items() if not k.startswith("ROFL_") or k in ("ROFL_ZK_LIB",)}
    env.update(case["env"])
    t0 = time.time()
    r = subprocess.run([sys.executable, HELPER] + list(case["workloads"]), env=env, capture_output=True, text=True, timeout=300)
    tail = "\n--- stdout\n" + r.stdout[-3000:] + "\n--- stderr (trace)\n" + r.stderr[-6000:]
    assert r.returncode == 0, "helper exited with %d%s" % (r.returncode, tail)
    got = [l for l in r.stdout.splitlines() if l.startswith(("ITEM ", "RESULT "))]
    want = [l for w in case["workloads"] for l in _oracle(w)]
    diff = [(g, w) for g, w in zip(got, want) if g != w]
    assert got == want, "differs from the oracle under %r; first difference (got, oracle): %r%s" % (case["env"], diff[:1] or (len(got), len(want)), tail)
    if case["skip_unless"]:      # (after the comparison: the bytes must equal the oracle's on any CPU; only the witness of a SIMD path can be out of reach)
        st = dict(l.split()[1:3] for l in r.stdout.splitlines() if l.startswith("SELFTEST "))
        if st.get(case["skip_unless"]) == "-1":
            pytest.skip("bytes agree; this CPU has no AVX-512 path for %s (the library's selftest returns -1), so the path cannot be witnessed" % case["skip_unless"])
    unmet = KM.unmet(case["witnesses"], r.stderr, r.stdout)
    assert not unmet, "the bytes agree but the path did not run -- unmet witnesses %r under %r%s" % (unmet, case["env"], tail)
    print("knob case %s: %s in %.1f s" % (case["id"], " ".join(case["workloads"]), time.time() - t0))
