"""The view round through a Merkle tree (rofl_merkle_build: k_mt_leaves, k_mt_tile, k_mt_paths; rofl_merkle_verify: k_mt_leaves, k_mt_climb)
at the sizes a deployment runs it, on ONE box in ONE run: n = 48, 10 000 and 100 000 dealers, one 156-byte view_leaf each.

Per case, host clock around each call (they return after their stream has been synchronised) after two warm-ups, median of --reps
repetitions with the spread:
  view_tree (the leaves made in Python, ONE merkle.build) and merkle.build alone on the leaves already made, with and without all n paths;
  verify_view_roots of n clients' signatures on the 60-byte root message;
  merkle.verify of all n paths, and one client's verify_view_entries of 32 entries;
beside them, in the same run:
  the parent commit's only route: verify_views of the same n signers on the v1 view_message of the same dealers (132 bytes a dealer);
  the host twins rofl_dbg_host_merkle_build / _verify on ONE core of the same box.
Before any clock starts the bytes and verdicts of device and host twin are compared, and one path and one signature per case are made wrong
and must come back as exactly that verdict.

  python scripts/gpu_merkle.py [--reps 20] [--no-host] [--no-v1] [--sizes 48,10000,100000] [--out profiles/merkle.json]

The kernels' own times come from a run of their own:
  rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python scripts/gpu_merkle.py --no-host --no-v1 --reps 3 --sizes 10000 --out ''"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import rofl_project_code_amd as R  # noqa: E402
from rofl_project_code_amd.api import merkle as MT, secret_sharing as SS, signatures as SG  # noqa: E402

ROUND_NO = 7


def timed(fn, reps):
    fn()                                                           # (warm-up 2; warm-up 1 produced the bytes that were compared)
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ms.append(round((time.perf_counter() - t0) * 1e3, 3))
    return {"ms": ms, "median_ms": float(np.median(ms)), "min_ms": min(ms), "max_ms": max(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--no-host", action="store_true", help="skip the host twins (the kernel-trace run)")
    ap.add_argument("--no-v1", action="store_true", help="skip verify_views on the flat view message")
    ap.add_argument("--sizes", default="48,10000,100000")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "merkle.json"), help="'' = print only")
    a = ap.parse_args()
    R.set_device(0)
    lib = R.lib()
    hb, hv = lib.rofl_dbg_host_merkle_build, lib.rofl_dbg_host_merkle_verify
    rng = np.random.default_rng(20270301)
    res = {"reps": a.reps, "host_clock": "perf_counter around each call after two warm-ups; the call ends in a stream synchronise",
           "baseline": "verify_views on the v1 view_message (the parent commit's only route); rofl_dbg_host_merkle_build / _verify on one core",
           "leaf_bytes": 156, "tile_leaves": int(lib.rofl_dbg_merkle_tile_leaves()), "cases": {}}
    for n in [int(x) for x in a.sizes.split(",") if x]:
        reps = a.reps if n <= 10000 else max(3, a.reps // 4)
        shown = dict(enumerate(rng.integers(0, 256, size=(n, 2, 64), dtype=np.uint8)))      # the dealers' signature pairs: any bytes
        leaves = [SS.view_leaf(ROUND_NO, d, shown[d]) for d in range(n)]
        every = list(range(n))
        root, dealers, paths = SS.view_tree(ROUND_NO, shown, paths_for=every)              # (warm-up 1)
        assert dealers == every and MT.build(leaves).tobytes() == root.tobytes()
        bad = paths.copy(); wrong = (n * 5) // 8; bad[wrong, MT.depth(n) - 1, 3] ^= 1
        verdicts = MT.verify(root, [n], bad, messages=leaves)
        assert verdicts[wrong] == 1 and verdicts.sum() == 1, "n = %d: the verdicts are not the one wrong path" % n
        mine = sorted(rng.choice(n, size=min(32, n), replace=False).tolist())
        entries = [(d, shown[d]) for d in mine]
        assert not SS.verify_view_entries(ROUND_NO, root, n, mine, entries, paths[mine]).any()
        sks = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
        view_sigs = SS.sign_view_root(sks, ROUND_NO, n, np.tile(root, (n, 1)))
        pks = SG.public_keys(sks)
        bad_sigs = view_sigs.copy(); bad_sigs[wrong, 40] ^= 1
        sv = SS.verify_view_roots(pks, ROUND_NO, n, root, bad_sigs)
        assert sv[wrong] == 1 and sv.sum() == 1, "n = %d: the verdicts are not the one wrong signature" % n
        c = {"n_dealers": n, "depth": MT.depth(n)}
        if not a.no_host:
            h = MT._build(hb, leaves, None, every, False)
            assert h[0].tobytes() == root.tobytes() and (h[1] == paths).all(), "n = %d: the device and the host twin differ (build)" % n
            assert (MT._verify(hv, root, [n], bad, leaves, None, None) == verdicts).all(), "n = %d: the device and the host twin differ (verify)" % n
            hreps = 3 if n > 10000 else 5
            c["host_build_all_paths"] = timed(lambda: MT._build(hb, leaves, None, every, False), hreps)
            c["host_build_root_only"] = timed(lambda: MT._build(hb, leaves, None, None, False), hreps)
            c["host_verify_all_paths"] = timed(lambda: MT._verify(hv, root, [n], bad, leaves, None, None), hreps)
        c["view_tree"] = timed(lambda: SS.view_tree(ROUND_NO, shown), reps)
        c["build_root_only"] = timed(lambda: MT.build(leaves), reps)
        c["build_all_paths"] = timed(lambda: MT.build(leaves, paths_for=every), reps)
        c["verify_view_roots"] = timed(lambda: SS.verify_view_roots(pks, ROUND_NO, n, root, bad_sigs), reps)
        c["verify_all_paths"] = timed(lambda: MT.verify(root, [n], bad, messages=leaves), reps)
        c["verify_view_entries_32"] = timed(lambda: SS.verify_view_entries(ROUND_NO, root, n, mine, entries, paths[mine]), reps)
        if not a.no_v1:
            view = SS.view_message(ROUND_NO, shown)
            v1_sigs = SG.sign(sks, [view], [(i, 0) for i in range(n)])
            v1_bad = v1_sigs.copy(); v1_bad[wrong, 40] ^= 1
            vv = SS.verify_views(pks, view, v1_bad)
            assert vv[wrong] == 1 and vv.sum() == 1
            c["v1_verify_views"] = dict(timed(lambda: SS.verify_views(pks, view, v1_bad), max(3, reps // 4)), view_bytes=len(view))
            c["v1_over_tree_verify_view_roots"] = round(c["v1_verify_views"]["median_ms"] / c["verify_view_roots"]["median_ms"], 2)
        res["cases"][str(n)] = c
        print("n = %d: " % n + ", ".join("%s %.3f ms" % (k, v["median_ms"]) for k, v in c.items() if isinstance(v, dict)), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
