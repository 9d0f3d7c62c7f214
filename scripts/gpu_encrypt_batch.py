"""The compressed randomness proofs of the clients of one process (CompressedRandProof::helper_prove(_existing), the randomness leg of
EncParamsRangeCompressed.encrypt; rofl_service's client binary hosts its clients as tasks of one process, client.rs:265-266) at the paper's
end-to-end shape and at BASELINE's vector length: 48 clients, fp 16/7, d = 40 000 and d = 55 000.

In ONE process, after a warm-up, five alternations of the chosen ways
  lanes:   helper_prove(_existing) per client through params._concurrently (one call per client on the library's lanes)
  single:  helper_prove(_existing) one client at a time, each call timed: the one-client latency (median per call, max - min over all calls)
  batch:   ONE helper_prove_batch (rofl_create_compressed_randproof_batch)
each timed with a host clock (every way returns host bytes: the device has been synchronised).  Every client's proof and pairs are
asserted byte-equal between the ways in every repetition.  Gates: the median of batch is not above the median of lanes by more than
that run's max - min of lanes; with --parent JSON (this script's output on the parent commit, same box, same job), no way's median is
above the parent's by more than the parent run's own max - min of that way.

  python scripts/gpu_encrypt_batch.py [--clients 48] [--reps 5] [--shapes d40000,d55000,d40000_existing] [--ways lanes,single,batch]
                                      [--parent profiles/r12_compressed_one_creator_parent.json] [--out profiles/r12_compressed_one_creator.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import rofl_project_code_amd as R  # noqa: E402
from rofl_project_code_amd import params  # noqa: E402

SHAPES = {
    "d40000": dict(d=40000, fp=(16, 7), existing=False),
    "d55000": dict(d=55000, fp=(16, 7), existing=False),
    "d40000_existing": dict(d=40000, fp=(16, 7), existing=True),      # check_percentage 1.0: the range proofs' commitments are completed
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clients", type=int, default=48)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shapes", default="d40000,d55000")
    ap.add_argument("--ways", default="lanes,batch")
    ap.add_argument("--parent", default="", help="the JSON this script wrote on the parent commit: gate every way against it")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r12_compressed_one_creator.json"), help="'' = print only")
    a = ap.parse_args()
    names = a.ways.split(",")
    parent = json.load(open(a.parent))["shapes"] if a.parent else {}
    R.set_device(0)
    res = {"clients": a.clients, "reps": a.reps, "host_clock": "perf_counter around each way", "shapes": {}}
    gate_all = True
    for name in a.shapes.split(","):
        sh = SHAPES[name]
        d, fp, n = sh["d"], sh["fp"], a.clients
        xs, bls, exs, seeds = [], [], [], []
        for i in range(n):
            rng = np.random.default_rng(8100 + i)
            x = (rng.integers(-100, 100, size=d) / 128.0).astype(np.float32)      # inside the 8-bit range at frac 7
            bl = rng.integers(0, 256, size=(d, 32), dtype=np.uint8); bl[:, 31] &= 0x0F
            xs.append(x); bls.append(bl); seeds.append(bytes([i % 251 + 1]) * 32)
            exs.append(R.pedersen_ops.commit_vec(R.conversion32.f32_to_scalar_vec(x, fp=fp), bl) if sh["existing"] else None)
        nonces = lambda: [R.Nonce.seeded(s) for s in seeds]
        one = lambda i, nn: R.compressed_rand_proof.helper_prove(xs[i], bls[i], nonce=nn, existing=exs[i], fp=fp)
        calls = []      # the single way's own clock: one entry per call

        def single():
            out = []
            for i, nn in enumerate(nonces()):
                t0 = time.perf_counter()
                out.append(one(i, nn))
                calls.append(round((time.perf_counter() - t0) * 1e3, 3))
            return out
        ways = {"lanes": lambda: params._concurrently(*[lambda i=i, nn=nn: one(i, nn) for i, nn in enumerate(nonces())]),
                "single": single,
                "batch": lambda: R.compressed_rand_proof.helper_prove_batch(xs, bls, nonces=nonces(), existing_list=exs, fp=fp)}
        for w in names:      # warm-up: fixed-base tables, lane workspaces, staging
            ways[w]()
        calls.clear()
        times = {w: [] for w in names}
        same = True
        for _ in range(a.reps):
            outs = {}
            for w in names:
                t0 = time.perf_counter()
                outs[w] = ways[w]()
                times[w].append(round((time.perf_counter() - t0) * 1e3, 3))
            same &= all(not isinstance(g, Exception) and (g[0] == s[0]).all() and (g[1] == s[1]).all() for w in names[1:] for g, s in zip(outs[w], outs[names[0]]))
        if "single" in times:
            times["single"] = list(calls)      # per call, not per sweep of the clients
        med = {w: float(np.median(v)) for w, v in times.items()}
        spread = {w: round(max(v) - min(v), 3) for w, v in times.items()}
        gates = {}
        if "lanes" in med and "batch" in med:
            gates["batch_not_slower_than_lanes"] = bool(med["batch"] <= med["lanes"] + spread["lanes"])
        for w in names:
            if name in parent and w in parent[name]["median_ms"]:
                gates[w + "_not_slower_than_parent"] = bool(med[w] <= parent[name]["median_ms"][w] + parent[name]["max_minus_min_ms"][w])
        gate_all &= all(gates.values()) and same
        res["shapes"][name] = dict(d=d, fp=list(fp), existing=sh["existing"], ms=times, median_ms=med, max_minus_min_ms=spread, bytes_equal=bool(same), gates=gates)
        print("%s: %s, bytes equal: %s, gates: %s" % (name, ", ".join("%s %.2f ms (+-%.2f)" % (w, med[w], spread[w]) for w in names), same, gates), flush=True)
        if not same:
            print(json.dumps(res)); sys.exit(1)
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(json.dumps(res, indent=1) + "\n")
    sys.exit(0 if gate_all else 2)


if __name__ == "__main__":
    main()
