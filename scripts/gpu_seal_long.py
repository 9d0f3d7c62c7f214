"""Long sealed records: where the long route (k_aead_long_*) beats the one-lane kernels (k_aead_seal / k_aead_open), on ONE box in ONE
process.  Payload lengths 256 B .. 1 MB in powers of two plus 16 MB; n = 1, n = 64 and the largest n up to 65 536 that --max-total bytes
allow; three ways through the C ABI on the same arrays:

  long      rofl_dbg_aead_seal_long / _open_long, seg_blocks 0: every record down the long route
  one_lane  rofl_aead_seal / _open of a build in which no record is long -- the parent's route.  Build it beside the library with
            ROFL_BUILD_VARIANT=onelane ROFL_BUILD_DEFS=-DROFL_AEAD_LONG_MIN=0xffffffffu python -m rofl_project_code_amd.build
  host      rofl_dbg_host_aead_seal / _open on one core (one pass per case, after the bytes were compared)

Before any clock starts the sealed records of the three are compared byte for byte, and the opened plaintexts with the payloads.  Host
clock around each call (it returns after its stream has been synchronised), two warm-ups, median of --reps with min and max.  AEAD_LONG_MIN
(protocol_calls.hpp) is the smallest power of two from which the long route's median beats the one-lane median by more than the two spreads
at all batch sizes; the JSON carries that figure as "long_min_supported".

  python scripts/gpu_seal_long.py [--reps 20] [--max-total 1073741824] [--sizes ...] [--no-host] [--out profiles/aead_long.json]

The kernels' own times come from a run of their own:
  rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python scripts/gpu_seal_long.py --no-host --reps 3 --sizes 1048576,16777216 --batches 1 --out ''"""
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

sz, vp, u32 = ctypes.c_size_t, ctypes.c_void_p, ctypes.c_uint32
SEAL_ARGS = [sz, vp, vp, sz, vp, vp, vp, vp, vp, vp, vp]


def timed(fn, reps):
    fn(); fn()
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ms.append(round((time.perf_counter() - t0) * 1e3, 3))
    return {"median_ms": float(np.median(ms)), "min_ms": min(ms), "max_ms": max(ms)}


def case(libs, rng, size, n, reps, host):
    keys, nonces = rng.integers(0, 256, (n, 32), np.uint8), rng.integers(0, 256, (n, 12), np.uint8)
    ads, pts = rng.integers(0, 256, (n, 32), np.uint8), rng.integers(0, 256, (n, size), np.uint8)
    ao, po, so = (np.arange(n + 1, dtype=np.uint64) * np.uint64(w) for w in (32, size, size + 16))
    recs = {k: np.zeros((n, size + 16), np.uint8) for k in libs}
    back, v = np.zeros((n, size + 16), np.uint8), np.zeros(n, np.uint8)
    p = lambda a: a.ctypes.data      # noqa: E731

    def seal(k):
        fn, more = libs[k][0]
        assert fn(n, p(keys), None, n, None, p(nonces), p(ads), p(ao), p(pts), p(po), p(recs[k]), *more) == 0

    def open_(k):
        fn, more = libs[k][1]
        assert fn(n, p(keys), None, n, None, p(nonces), p(ads), p(ao), p(recs["long"]), p(so), p(back), p(v), *more) == 0
    res = {"bytes": size, "n": n}
    for k in libs:      # the bytes first
        t0 = time.perf_counter(); seal(k); ts = time.perf_counter() - t0
        assert (recs[k] == recs["long"]).all(), "%s and the long route differ (seal, %d x %d)" % (k, n, size)
        back[...] = 0xaa
        t0 = time.perf_counter(); open_(k); to = time.perf_counter() - t0
        assert not v.any() and (back[:, :size] == pts).all(), "%s: open (%d x %d)" % (k, n, size)
        if k == "host":
            res[k] = {"seal": {"passes": 1, "median_ms": round(ts * 1e3, 3)}, "open": {"passes": 1, "median_ms": round(to * 1e3, 3)}}
    for k in libs:
        if k != "host":
            res[k] = {"seal": timed(lambda: seal(k), reps), "open": timed(lambda: open_(k), reps)}
    if "one_lane" in res:
        for op in ("seal", "open"):
            a, b = res["long"][op], res["one_lane"][op]
            res["long_wins_" + op] = bool(b["median_ms"] - a["median_ms"] > (a["max_ms"] - a["min_ms"]) + (b["max_ms"] - b["min_ms"]))
    print("%8d B x %5d: " % (size, n) + "; ".join("%s %.3f / %.3f ms" % (k, res[k]["seal"]["median_ms"], res[k]["open"]["median_ms"]) for k in libs if k in res), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--max-total", type=int, default=1 << 30, help="payload bytes of the largest batch of a size")
    ap.add_argument("--sizes", default=",".join(str(1 << k) for k in range(8, 21)) + ",%d" % (1 << 24))
    ap.add_argument("--batches", default="1,64,max")
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--one-lane-lib", default=os.path.join(ROOT, "rofl_project_code_amd", "build", "librofl_zk_onelane.so"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "aead_long.json"), help="'' = print only")
    a = ap.parse_args()
    R.set_device(0)
    L = R.lib()
    geo = R.aead.long_geometry()
    for f in (L.rofl_dbg_aead_seal_long, L.rofl_dbg_host_aead_seal):
        f.argtypes = SEAL_ARGS + ([u32] if f is L.rofl_dbg_aead_seal_long else [])
    L.rofl_dbg_aead_open_long.argtypes, L.rofl_dbg_host_aead_open.argtypes = SEAL_ARGS + [vp, u32], SEAL_ARGS + [vp]
    libs = {"long": ((L.rofl_dbg_aead_seal_long, (0,)), (L.rofl_dbg_aead_open_long, (0,)))}
    if os.path.exists(a.one_lane_lib):
        L1 = ctypes.CDLL(a.one_lane_lib)
        assert L1.rofl_set_device(0) == 0
        L1.rofl_aead_seal.argtypes, L1.rofl_aead_open.argtypes = SEAL_ARGS, SEAL_ARGS + [vp]
        libs["one_lane"] = ((L1.rofl_aead_seal, ()), (L1.rofl_aead_open, ()))
    if not a.no_host:
        libs["host"] = ((L.rofl_dbg_host_aead_seal, ()), (L.rofl_dbg_host_aead_open, ()))
    rng = np.random.default_rng(20261305)
    res = {"reps": a.reps, "max_total": a.max_total, "tile_blocks": geo[0], "segment_blocks": geo[1], "long_min_built": geo[2],
           "host_clock": "perf_counter around each C call after two warm-ups; the call ends in a stream synchronise", "ways": sorted(libs), "cases": []}
    sizes = [int(x) for x in a.sizes.split(",")]
    for size in sizes:
        ns = sorted({1 if b == "1" else 64 if b == "64" else max(1, min(65536, a.max_total // size)) for b in a.batches.split(",")})
        for n in ns:
            if n * size <= a.max_total:
                res["cases"].append(case(libs, rng, size, n, a.reps, not a.no_host))
    if "one_lane" in libs:      # the smallest power of two from which the long route wins at every batch size, seal and open, and keeps winning
        good = None
        for size in sorted(sizes, reverse=True):
            if all(c["long_wins_seal"] and c["long_wins_open"] for c in res["cases"] if c["bytes"] == size):
                good = size
            else:
                break
        res["long_min_supported"] = good
        print("long route wins from %s bytes" % good)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
