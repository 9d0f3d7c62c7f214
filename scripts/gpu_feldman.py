"""Verifiable sharing (rofl_feldman_commit: k_shamir_coeffs, k_feldman_commit; rofl_feldman_verify: k_dh_decode, k_feldman_check) at the sizes
a deployment runs it, on ONE box in ONE run:

  a  commit 96 secrets at threshold 32                     (a process hosting 48 clients of a 48-client round, two secrets each)
  b  commit 2 secrets at threshold 667                     (one client of a 1 000-client round)
  c  server verify 48 secrets x 32 shares, threshold 32    (3 + 45 secrets of a 48-client round that lost three, 32 survivors answering)
  d  server verify 1 000 secrets x 667 shares, threshold 667
  e  client verify 96 x 1, threshold 32                    (one client's shares from 48 dealers, two secrets each)
  f  client verify 2 000 x 1, threshold 667

The device call: host clock around secret_sharing.commit / verify_shares (they return after their stream has been synchronised) after two
warm-ups, median of --reps repetitions with the spread.  The baseline is rofl_dbg_host_feldman_commit / _verify on ONE core of the same box
-- the parent commit has no route at all; a pass that takes more than 5 s is timed once, and cases d and f, whose pass would take minutes,
are timed on whole rows of a stated number of their secrets (--host-secrets-d, --host-secrets-f; the host's work is the same for every
secret): the count is in the result and the figure for the whole case is that time scaled by secrets and marked "not measured".  Before any
clock starts the bytes and verdicts of the two routes are compared on what the host computes, one share per case is made wrong and must
come back as exactly that verdict, and the commitments of cases a and b must accept the shares rofl_shamir_share deals.

Operation counts (from the formulas of csrc/fe26.hpp): a doubling is 8 field multiplications (4 squarings among them), an addition 9 (the
product by 2d among them).  A Horner step of k_feldman_check is xbits - 1 doublings, one addition per set bit of the lane's x below bit
xbits - 1 (the top bit selects the start), and the addition of C_k; the share's side is one fixed-base product of at most 32 mixed additions (7
multiplications each) and the comparison 4 multiplications.  The script counts them per call from the points and the shares.

  python scripts/gpu_feldman.py [--reps 20] [--no-host] [--cases a,b,c,d,e,f] [--out profiles/feldman_vss.json]

The kernels' own times come from a run of their own:
  rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python scripts/gpu_feldman.py --no-host --reps 3 --out ''"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import rofl_project_code_amd as R  # noqa: E402
from rofl_project_code_amd.api import secret_sharing as S  # noqa: E402

COMMIT = {"a": (96, 32), "b": (2, 667)}
VERIFY = {"c": (48, 32, 32), "d": (1000, 667, 667), "e": (96, 1, 32), "f": (2000, 1, 667)}      # secrets, shares, threshold
DOUBLE_MULS, ADD_MULS, MADD_MULS = 8, 9, 7
sz, vp = ctypes.c_size_t, ctypes.c_void_p


def host_commit(lib, sec, seeds, t):
    out = np.zeros((len(sec), t, 32), np.uint8)
    t0 = time.perf_counter()
    rc = lib.rofl_dbg_host_feldman_commit(len(sec), sec.ctypes.data, seeds.ctypes.data, t, out.ctypes.data)
    sec_s = time.perf_counter() - t0
    assert rc == 0
    return out, sec_s


def host_verify(lib, com, xs, sh):
    com, sh, xs = np.ascontiguousarray(com), np.ascontiguousarray(sh), np.ascontiguousarray(xs, dtype=np.uint32)
    out = np.zeros(sh.shape[:2], np.uint8)
    t0 = time.perf_counter()
    rc = lib.rofl_dbg_host_feldman_verify(com.shape[0], com.shape[1], com.ctypes.data, sh.shape[1], xs.ctypes.data, sh.ctypes.data, out.ctypes.data)
    sec_s = time.perf_counter() - t0
    assert rc == 0
    return out, sec_s


def timed(fn, reps):
    fn()                                                           # (warm-up 2; warm-up 1 produced the bytes that were compared)
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ms.append(round((time.perf_counter() - t0) * 1e3, 3))
    return {"ms": ms, "median_ms": float(np.median(ms)), "min_ms": min(ms), "max_ms": max(ms)}


def host_passes(one, first):
    passes = [first]
    while first < 5.0 and len(passes) < 3:
        passes.append(one())
    return {"passes": len(passes), "passes_ms": [round(s * 1e3, 2) for s in passes], "median_ms": round(float(np.median(passes)) * 1e3, 2), "results_equal": True}


def check_ops(n_sec, xs, t):
    """point operations and field multiplications of one k_feldman_check launch: the Horner steps of every (secret, share) pair"""
    xbits = int(max(xs)).bit_length()
    adds_on_bits = sum(bin(int(x) & ((1 << (xbits - 1)) - 1)).count("1") for x in xs)      # (the top bit selects the start: no addition)
    steps = t - 1
    doublings = n_sec * len(xs) * steps * (xbits - 1)
    additions = n_sec * steps * (adds_on_bits + len(xs))
    return {"xbits": xbits, "horner_doublings": doublings, "horner_additions": additions, "horner_point_ops": doublings + additions,
            "horner_field_multiplications": doublings * DOUBLE_MULS + additions * ADD_MULS,
            "share_side_field_multiplications_at_most": n_sec * len(xs) * (32 * MADD_MULS + 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--no-host", action="store_true", help="skip the host route (the kernel-trace run)")
    ap.add_argument("--cases", default="a,b,c,d,e,f")
    ap.add_argument("--host-secrets-d", type=int, default=2)
    ap.add_argument("--host-secrets-f", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "feldman_vss.json"), help="'' = print only")
    a = ap.parse_args()
    R.set_device(0)
    lib = R.lib()
    lib.rofl_dbg_host_feldman_commit.argtypes = [sz, vp, vp, sz, vp]
    lib.rofl_dbg_host_feldman_verify.argtypes = [sz, sz, vp, sz, vp, vp, vp]
    rng = np.random.default_rng(20261025)
    res = {"reps": a.reps, "host_clock": "perf_counter around each call after two warm-ups; the call ends in a stream synchronise",
           "baseline": "rofl_dbg_host_feldman_commit / _verify on one core", "cases": {}}
    for name in a.cases.split(","):
        if name in COMMIT:
            n_sec, t = COMMIT[name]
            sec, seeds = rng.integers(0, 256, size=(n_sec, 32), dtype=np.uint8), rng.integers(0, 256, size=(n_sec, 32), dtype=np.uint8)
            got = S.commit(sec, seeds, t)                          # (warm-up 1)
            # the commitments accept what rofl_shamir_share deals, and refuse one share made wrong
            sh = S.share(sec, seeds, t, t)
            sh[-1, -1, 0] ^= 1
            v = S.verify_shares(got, np.arange(1, t + 1), sh)
            assert v[-1, -1] == 1 and v.sum() == 1, "case %s: the commitments and the shares of one polynomial disagree" % name
            c = {"kind": "commit", "n_secrets": n_sec, "threshold": t, "commitments": n_sec * t}
            if not a.no_host:
                want, first = host_commit(lib, sec, seeds, t)
                assert (got == want).all(), "case %s: the device and the host route differ" % name
                c["host"] = host_passes(lambda: host_commit(lib, sec, seeds, t)[1], first)
                c["host"]["us_per_commitment"] = round(c["host"]["median_ms"] * 1e3 / (n_sec * t), 3)
            c["device"] = timed(lambda: S.commit(sec, seeds, t), a.reps)
            c["device"]["us_per_commitment"] = round(c["device"]["median_ms"] * 1e3 / (n_sec * t), 3)
        else:
            n_sec, n, t = VERIFY[name]
            sec, seeds = rng.integers(0, 256, size=(n_sec, 32), dtype=np.uint8), rng.integers(0, 256, size=(n_sec, 32), dtype=np.uint8)
            # the points: the first n clients for the server; for a client its own, the last of the round
            xs = np.arange(1, n + 1, dtype=np.uint32) if n > 1 else np.array([{32: 48, 667: 1000}[t]], np.uint32)
            com = S.commit(sec, seeds, t)
            if n >= t:
                sh = S.share(sec, seeds, t, n, xs=xs)
            else:                                                  # (a sharing has at least t points: deal t of them, keep the client's column)
                deal = np.concatenate([np.setdiff1d(np.arange(1, t + 1, dtype=np.uint32), xs)[:t - n], xs])
                sh = np.ascontiguousarray(S.share(sec, seeds, t, t, xs=deal)[:, t - n:])
            sh[n_sec // 2, n // 2, 5] ^= 0x10                      # one wrong share: exactly that verdict
            got = S.verify_shares(com, xs, sh)                     # (warm-up 1)
            assert got[n_sec // 2, n // 2] == 1 and got.sum() == 1, "case %s: the verdicts are not the one wrong share" % name
            c = {"kind": "verify", "n_secrets": n_sec, "n_shares": n, "threshold": t, "pairs": n_sec * n, "k_feldman_check": check_ops(n_sec, xs, t)}
            if not a.no_host:
                hs = {"d": a.host_secrets_d, "f": a.host_secrets_f}.get(name, n_sec)
                hs = min(hs, n_sec)
                rows = np.arange(min(n_sec // 2, n_sec - hs), min(n_sec // 2, n_sec - hs) + hs)      # (whole rows, the one with the wrong share among them)
                hcom, hsh = com[rows], sh[rows]
                want, first = host_verify(lib, hcom, xs, hsh)
                assert (got[rows] == want).all(), "case %s: the device and the host route differ" % name
                c["host"] = host_passes(lambda: host_verify(lib, hcom, xs, hsh)[1], first)
                c["host"]["secrets_timed"] = hs
                c["host"]["whole_case_ms"] = round(c["host"]["median_ms"] * n_sec / hs, 2)
                c["host"]["whole_case_is"] = "not measured: the time of %d of %d secrets scaled" % (hs, n_sec) if hs < n_sec else "measured"
            c["device"] = timed(lambda: S.verify_shares(com, xs, sh), a.reps)
            c["device"]["us_per_pair"] = round(c["device"]["median_ms"] * 1e3 / (n_sec * n), 3)
        if "host" in c:
            c["host_over_device"] = round(c["host"].get("whole_case_ms", c["host"]["median_ms"]) / c["device"]["median_ms"], 2)
        res["cases"][name] = c
        print("%s %s: device %.3f ms (%.3f-%.3f)%s" % (name, {k: v for k, v in c.items() if k.startswith("n_") or k == "threshold"}, c["device"]["median_ms"],
              c["device"]["min_ms"], c["device"]["max_ms"], "; host %.1f ms over %d pass(es)%s" % (
                  c["host"].get("whole_case_ms", c["host"]["median_ms"]), c["host"]["passes"],
                  " (scaled, not measured)" if c["host"].get("whole_case_is", "measured") != "measured" else "") if "host" in c else ""), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
