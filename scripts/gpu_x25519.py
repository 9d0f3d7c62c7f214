"""X25519 (rofl_x25519_shared: k_x25519) in ONE run on one box: its two layouts against each other, the call against the Ristretto agreement
(rofl_dh_shared: k_dh_public, k_dh_decode, k_dh_shared) at the same shapes, and against its host twin on ONE core.

Every shape is n_own keys against n_peer peer keys, all pairs (pairs = NULL): 1 x 1, a client's 1 x 47, a host's 48 x 47, 64 x 64, 128 x 128
(the derived rule's 16 384 pairs), 256 x 256 and 48 x 10 000.  Host clock around each call (every call returns after its stream has been
synchronised) after a warm-up, median of --reps repetitions with the spread.  Before any clock starts the two layouts' bytes are compared with
each other and, at the small shapes, with the host twin's.  The crossover recorded is the smallest shape measured at which the lane layout's
median is below the quad layout's.

  python scripts/gpu_x25519.py [--reps 5] [--out profiles/x25519.json]

The kernels' own times come from a run of their own:
  rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python scripts/gpu_x25519.py --no-host --reps 3 --out ''"""
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

sz, vp = ctypes.c_size_t, ctypes.c_void_p
SHAPES = [(1, 1), (1, 47), (48, 47), (64, 64), (128, 128), (256, 256), (48, 10000)]
HOST_SIZES = [1, 8, 47]


def call(lib, name, *args):
    fn = getattr(lib, name)
    fn.argtypes = [sz if isinstance(a, int) else vp for a in args]
    rc = fn(*[a if isinstance(a, int) or a is None else a.ctypes.data for a in args])
    assert rc == 0, (name, rc)


def timed(fn, reps):
    fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": float(np.median(t)), "min_ms": float(min(t)), "max_ms": float(max(t)), "reps": len(t)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "x25519.json"))
    a = ap.parse_args()
    R.set_device(0)
    lib = R.api.lib()
    rng = np.random.default_rng(20261126)
    rows = []
    for n_own, n_peer in SHAPES:
        n = n_own * n_peer
        sk = rng.integers(0, 256, size=(n_own, 32), dtype=np.uint8)
        peer_x = rng.integers(0, 256, size=(n_peer, 32), dtype=np.uint8)
        peer_r = R.key_agreement.public_keys(rng.integers(0, 256, size=(n_peer, 32), dtype=np.uint8))
        out, st = [np.zeros((n, 32), np.uint8) for _ in range(3)], np.zeros(n, np.uint8)
        route = lambda r, o: call(lib, "rofl_dbg_x25519_shared", r, n_own, sk, None, n_peer, peer_x, n, None, o, st)      # noqa: E731
        route(1, out[1]); route(2, out[2])
        assert out[1].tobytes() == out[2].tobytes() and not st.any()
        row = {"n_own": n_own, "n_peer": n_peer, "n_pairs": n, "lane": timed(lambda: route(1, out[0]), a.reps), "quad": timed(lambda: route(2, out[0]), a.reps),
               "x25519_shared": timed(lambda: call(lib, "rofl_x25519_shared", n_own, sk, None, n_peer, peer_x, n, None, out[0], st), a.reps),
               "dh_shared": timed(lambda: call(lib, "rofl_dh_shared", n_own, sk, None, n_peer, peer_r, n, None, out[0], st), a.reps)}
        rows.append(row)
        print(json.dumps(row), flush=True)
    host = []
    for n in [] if a.no_host else HOST_SIZES:
        sk, u = rng.integers(0, 256, size=(1, 32), dtype=np.uint8), rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
        ho, hs, do, ds = np.zeros((n, 32), np.uint8), np.zeros(n, np.uint8), np.zeros((n, 32), np.uint8), np.zeros(n, np.uint8)
        twin = lambda: call(lib, "rofl_dbg_host_x25519", n, np.ascontiguousarray(np.repeat(sk, n, axis=0)), u, ho, hs)      # noqa: E731
        dev = lambda: call(lib, "rofl_x25519_shared", 1, sk, None, n, u, n, None, do, ds)      # noqa: E731
        twin(); dev()
        assert ho.tobytes() == do.tobytes() and hs.tobytes() == ds.tobytes()
        host.append({"n_pairs": n, "host_one_core": timed(twin, a.reps), "x25519_shared": timed(dev, a.reps)})
        print(json.dumps(host[-1]), flush=True)
    wins = [r["n_pairs"] for r in rows if r["lane"]["median_ms"] < r["quad"]["median_ms"]]
    res = {"what": "rofl_dbg_x25519_shared at route 1 (one ladder per lane) and 2 (per lane quad), rofl_x25519_shared against rofl_dh_shared at the same "
                   "all-pairs shapes, and against rofl_dbg_host_x25519 on one core: same box, same run, host clock, medians",
           "device": "MI355X", "date": time.strftime("%Y-%m-%d"), "derived_rule_pairs": 16384, "lane_first_wins_at_pairs": min(wins) if wins else None,
           "rows": rows, "host": host}
    if a.out:
        json.dump(res, open(a.out, "w"), indent=1)
        print("wrote", a.out)


if __name__ == "__main__":
    main()
