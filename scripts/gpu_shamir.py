"""Secret sharing of the mask secrets (rofl_shamir_share: k_shamir_coeffs, k_shamir_eval; rofl_shamir_reconstruct: k_shamir_weights,
k_shamir_combine) at the sizes a deployment runs it, on ONE box in ONE run:

  a  share 96 secrets at 48 points, threshold 32          (a process hosting 48 clients of a 48-client round, two secrets each)
  b  share 96 secrets at 1 000 points, threshold 667
  c  share 96 secrets at 10 000 points, threshold 6 667
  d  reconstruct 3 + 45 secrets from 32 shares             (the server of a 48-client round that lost three)
  e  reconstruct 10 000 secrets from 6 667 shares          (four calls of 2 500 secrets: a call holds at most 2^24 shares)

The device call: host clock around secret_sharing.share / reconstruct (they return after their stream has been synchronised) after two
warm-ups, median of --reps repetitions with the spread.  The baseline is rofl_dbg_host_shamir_share / _reconstruct on ONE core of the same
box -- the parent commit has no route at all; a pass that takes more than 5 s is timed once, and case c, whose pass would take minutes,
is timed on its first --host-secrets secrets only (the count is in the result, the figure for all 96 is that time scaled and marked so).
Before any clock starts the bytes of the two routes are compared (case c: the rows of those secrets; every other row is checked by
reconstructing its secret from a threshold of its shares).

  python scripts/gpu_shamir.py [--reps 20] [--no-host] [--cases a,b,c,d,e] [--out profiles/shamir_sharing.json]

The kernels' own times come from a run of their own:
  rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python scripts/gpu_shamir.py --no-host --reps 3 --out ''"""
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

L = 2 ** 252 + 27742317777372353535851937790883648493
SHARE = {"a": (96, 48, 32), "b": (96, 1000, 667), "c": (96, 10000, 6667)}
RECON = {"d": (48, 32, 1), "e": (2500, 6667, 4)}      # secrets per call, shares, calls
sz, vp = ctypes.c_size_t, ctypes.c_void_p


def reduced(a):
    return np.frombuffer(b"".join((int.from_bytes(r.tobytes(), "little") % L).to_bytes(32, "little") for r in a), np.uint8).reshape(-1, 32)


def host_share(lib, sec, seeds, t, n):
    out = np.zeros((len(sec), n, 32), np.uint8)
    t0 = time.perf_counter()
    rc = lib.rofl_dbg_host_shamir_share(len(sec), sec.ctypes.data, seeds.ctypes.data, t, n, None, out.ctypes.data)
    sec_s = time.perf_counter() - t0
    assert rc == 0
    return out, sec_s


def host_reconstruct(lib, xs, sh):
    out = np.zeros((len(sh), 32), np.uint8)
    t0 = time.perf_counter()
    rc = lib.rofl_dbg_host_shamir_reconstruct(len(sh), len(xs), xs.ctypes.data, sh.ctypes.data, out.ctypes.data)
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
    return {"passes": len(passes), "passes_ms": [round(s * 1e3, 2) for s in passes], "median_ms": round(float(np.median(passes)) * 1e3, 2), "bytes_equal": True}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--no-host", action="store_true", help="skip the host route (the kernel-trace run)")
    ap.add_argument("--cases", default="a,b,c,d,e")
    ap.add_argument("--host-secrets", type=int, default=2, help="secrets of case c the host route is timed on")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "shamir_sharing.json"), help="'' = print only")
    a = ap.parse_args()
    R.set_device(0)
    lib = R.lib()
    lib.rofl_dbg_host_shamir_share.argtypes = [sz, vp, vp, sz, sz, vp, vp]
    lib.rofl_dbg_host_shamir_reconstruct.argtypes = [sz, sz, vp, vp, vp]
    rng = np.random.default_rng(20261019)
    res = {"reps": a.reps, "host_clock": "perf_counter around each call after two warm-ups; the call ends in a stream synchronise",
           "baseline": "rofl_dbg_host_shamir_share / _reconstruct on one core", "cases": {}}
    for name in a.cases.split(","):
        if name in SHARE:
            n_sec, n, t = SHARE[name]
            sec, seeds = rng.integers(0, 256, size=(n_sec, 32), dtype=np.uint8), rng.integers(0, 256, size=(n_sec, 32), dtype=np.uint8)
            got = S.share(sec, seeds, t, n)                        # (warm-up 1)
            mults = n_sec * n * (t - 1)
            c = {"kind": "share", "n_secrets": n_sec, "n_shares": n, "threshold": t, "multiplications": mults}
            if not a.no_host:
                hs = min(n_sec, a.host_secrets) if name == "c" else n_sec
                want, first = host_share(lib, sec[:hs], seeds[:hs], t, n)
                assert (got[:hs] == want).all(), "case %s: the device and the host route differ" % name
                if hs < n_sec:                                     # the rows the host did not compute: their secrets come back from t of their shares
                    pick = np.sort(rng.permutation(n)[:t])
                    back = S.reconstruct(pick + 1, np.ascontiguousarray(got[:, pick]))
                    assert (back == reduced(sec)).all(), "case %s: a row does not reconstruct its secret" % name
                c["host"] = host_passes(lambda: host_share(lib, sec[:hs], seeds[:hs], t, n)[1], first)
                c["host"]["secrets_timed"] = hs
                c["host"]["ns_per_multiplication"] = round(c["host"]["median_ms"] * 1e6 / (hs * n * (t - 1)), 2)
                c["host"]["all_secrets_ms"] = round(c["host"]["median_ms"] * n_sec / hs, 2)
                c["host"]["all_secrets_is_scaled"] = hs < n_sec
            c["device"] = timed(lambda: S.share(sec, seeds, t, n), a.reps)
            c["device"]["ns_per_multiplication"] = round(c["device"]["median_ms"] * 1e6 / mults, 4)
        else:
            n_sec, n, calls = RECON[name]
            sec, seeds = rng.integers(0, 256, size=(n_sec, 32), dtype=np.uint8), rng.integers(0, 256, size=(n_sec, 32), dtype=np.uint8)
            xs = np.sort(rng.permutation(10000)[:n] + 1).astype(np.uint32)
            sh = S.share(sec, seeds, 3, n, xs=xs)                  # (any n >= 3 consistent shares give the secret; the work does not depend on the bytes)
            got = S.reconstruct(xs, sh)                            # (warm-up 1)
            assert (got == reduced(sec)).all(), "case %s: the secrets do not come back" % name
            c = {"kind": "reconstruct", "n_secrets": n_sec * calls, "n_shares": n, "calls": calls, "secrets_per_call": n_sec,
                 "note": "every call gets the same %d secrets" % n_sec if calls > 1 else ""}
            if not a.no_host:
                want, first = host_reconstruct(lib, xs, sh)
                assert (got == want).all(), "case %s: the device and the host route differ" % name
                first = first + sum(host_reconstruct(lib, xs, sh)[1] for _ in range(calls - 1))
                c["host"] = host_passes(lambda: sum(host_reconstruct(lib, xs, sh)[1] for _ in range(calls)), first)
            c["device"] = timed(lambda: [S.reconstruct(xs, sh) for _ in range(calls)], a.reps)
        if "host" in c:
            c["host_over_device"] = round(c["host"].get("all_secrets_ms", c["host"]["median_ms"]) / c["device"]["median_ms"], 2)
        res["cases"][name] = c
        print("%s %s: device %.3f ms (%.3f-%.3f)%s" % (name, {k: v for k, v in c.items() if k.startswith("n_") or k == "threshold"}, c["device"]["median_ms"],
              c["device"]["min_ms"], c["device"]["max_ms"], "; host %.1f ms over %d pass(es)%s" % (
                  c["host"].get("all_secrets_ms", c["host"]["median_ms"]), c["host"]["passes"], " (scaled)" if c["host"].get("all_secrets_is_scaled") else "") if "host" in c else ""), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
