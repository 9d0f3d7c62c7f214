"""The wide discrete-log solver (bsgs_bits 24 and 40: k_wdlog_build, k_wdlog_solve, k_wdlog_finish) on ONE box in ONE run.

Per (table_size, bsgs_bits) in (2^16, 24), (2^20, 40), (2^24, 40):
  the first call on one point (it builds and caches the table: "build_ms" is that call minus a warm one-point call);
  pedersen_ops.discrete_log_vec for d = 64, 5 000, 55 000 points with seeded logs below 2^24 of both signs, host clock around the call
  (it ends in a stream synchronise) after a warm-up, median of --reps repetitions;
  "full_walk": d = 64 points whose logs lie beyond the reach, so that no walker stops early -- giant steps per second and the
  share of the field-multiplication ceiling bench_femul measures in the same run (a step is counted as 11 multiplications, a squaring and
  1/7 of an inversion of 254 squarings and 11 multiplications: 50.1 products, squarings counted as one).
"range_equivalent": the same points at (2^20, 32) -- k_bsgs_solve, the route that existed before -- and at (2^20, 40), results compared
before any clock starts.

  python scripts/gpu_wide_dlog.py [--reps 5] [--out profiles/wide_dlog.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import rofl_project_code_amd as R  # noqa: E402
from rofl_project_code_amd import api  # noqa: E402

ELL = 2 ** 252 + 27742317777372353535851937790883648493
STEP_PRODUCTS = 11 + 1 + (254 + 11) / 7.0
DLOG = R.pedersen_ops.discrete_log_vec


def timed(fn, reps):
    fn()
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ms.append(round((time.perf_counter() - t0) * 1e3, 3))
    return {"ms": ms, "median_ms": float(np.median(ms)), "min_ms": min(ms), "max_ms": max(ms)}


def points(vs):
    sc = np.stack([np.frombuffer((int(v) % ELL).to_bytes(32, "little"), np.uint8) for v in vs])
    return R.pedersen_ops.commit_no_blinding_vec(sc), sc


def not_found(p, m, bits):
    try:
        DLOG(p, m, bits)
    except R.RoflError as e:
        assert e.code == 11
    else:
        raise AssertionError("a log beyond the reach was found")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wide_dlog.json"), help="'' = print only")
    a = ap.parse_args()
    R.set_device(0)
    rng = np.random.default_rng(20261126)
    femul = api.bench_femul()
    res = {"box": "one MI355X (gfx950), one process, one run", "reps": a.reps, "host_clock": "perf_counter around each call after a warm-up; the call ends in a stream synchronise",
           "bench_femul_per_s": femul, "products_per_step": round(STEP_PRODUCTS, 1), "cases": {}}
    logs = {d: rng.integers(-(1 << 24) + 1, 1 << 24, size=d) for d in (64, 5000, 55000)}
    pts = {d: points(v) for d, v in logs.items()}
    one = points([12345])[0]
    for m, bits in ((1 << 16, 24), (1 << 20, 40), (1 << 24, 40)):
        t0 = time.perf_counter()
        DLOG(one, m, bits)
        first = (time.perf_counter() - t0) * 1e3
        warm = timed(lambda: DLOG(one, m, bits), a.reps)["median_ms"]
        c = {"first_call_ms": round(first, 3), "one_point_ms": warm, "build_ms": round(first - warm, 3)}
        for d, (p, sc) in pts.items():
            assert DLOG(p, m, bits).tobytes() == sc.tobytes(), (m, bits, d)
            c["d%d" % d] = timed(lambda: DLOG(p, m, bits), a.reps)
        # 64 logs beyond the reach: the call answers 11 after every walker has walked its whole run (the launcher's split, restated)
        nowhere = points([(4 << bits) + k for k in range(64)])[0]
        per_dir = ((1 << bits) // m + 1) // 2 + 1
        half = max(1, min(65536 // 128, -(-per_dir // 56)))
        steps = 64 * 2 * half * (-(-(-(-per_dir // half)) // 7) * 7)
        t = timed(lambda: not_found(nowhere, m, bits), max(3, a.reps // 2))
        c["full_walk_d64"] = dict(t, giant_steps=steps, steps_per_s=round(steps / (t["median_ms"] * 1e-3)),
                                  fraction_of_femul_ceiling=round(steps * STEP_PRODUCTS / (t["median_ms"] * 1e-3) / femul, 4))
        res["cases"]["%d,%d" % (m, bits)] = c
        print(m, bits, json.dumps({k: (v["median_ms"] if isinstance(v, dict) else v) for k, v in c.items()}), flush=True)
    cmp_ = {}
    m = 1 << 20
    DLOG(one, m, 32)
    for d, (p, sc) in pts.items():
        assert DLOG(p, m, 32).tobytes() == sc.tobytes() == DLOG(p, m, 40).tobytes()
        old, new = timed(lambda: DLOG(p, m, 32), 3), timed(lambda: DLOG(p, m, 40), a.reps)
        cmp_["d%d" % d] = {"old_32": old, "new_40": new, "old_over_new": round(old["median_ms"] / new["median_ms"], 2)}
        print("range-equivalent", d, json.dumps({"old_ms": old["median_ms"], "new_ms": new["median_ms"]}), flush=True)
    res["range_equivalent"] = cmp_
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
