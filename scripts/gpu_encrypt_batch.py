"""The compressed randomness proofs of the clients of one process (CompressedRandProof::helper_prove(_existing), the randomness leg of
EncParamsRangeCompressed.encrypt; rofl_service's client binary hosts its clients as tasks of one process, client.rs:265-266) at the paper's
end-to-end shape and at BASELINE's vector length: 48 clients, fp 16/7, d = 40 000 and d = 55 000.

In ONE process, after a warm-up, five alternations of
  (a) lanes:  helper_prove(_existing) per client through params._concurrently (one call per client on the library's lanes)
  (b) batch:  ONE helper_prove_batch (rofl_create_compressed_randproof_batch)
each timed with a host clock (both ways return host bytes: the device has been synchronised).  Every client's proof and pairs are
asserted byte-equal between the two ways in every repetition.  Gate: the median of (b) is not above the median of (a) by more than
that run's max - min of (a).

  python scripts/gpu_encrypt_batch.py [--clients 48] [--reps 5] [--shapes d40000,d55000,d40000_existing] [--out profiles/r10_compressed_create_batch.json]"""
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r10_compressed_create_batch.json"), help="'' = print only")
    a = ap.parse_args()
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
        ways = {"lanes": lambda: params._concurrently(*[lambda i=i, nn=nn: R.compressed_rand_proof.helper_prove(xs[i], bls[i], nonce=nn, existing=exs[i], fp=fp)
                                                        for i, nn in enumerate(nonces())]),
                "batch": lambda: R.compressed_rand_proof.helper_prove_batch(xs, bls, nonces=nonces(), existing_list=exs, fp=fp)}
        names = ["lanes", "batch"]
        for w in names:      # warm-up: fixed-base tables, lane workspaces, staging
            ways[w]()
        times = {w: [] for w in names}
        same = True
        for _ in range(a.reps):
            outs = {}
            for w in names:
                t0 = time.perf_counter()
                outs[w] = ways[w]()
                times[w].append(round((time.perf_counter() - t0) * 1e3, 3))
            same &= all(not isinstance(g, Exception) and (g[0] == s[0]).all() and (g[1] == s[1]).all() for g, s in zip(outs["batch"], outs["lanes"]))
        med = {w: float(np.median(v)) for w, v in times.items()}
        spread = max(times["lanes"]) - min(times["lanes"])
        gate = med["batch"] <= med["lanes"] + spread
        gate_all &= gate and same
        res["shapes"][name] = dict(d=d, fp=list(fp), existing=sh["existing"], ms=times, median_ms=med, lanes_max_minus_min_ms=round(spread, 3), bytes_equal=bool(same),
                                   batch_over_lanes=round(med["batch"] / med["lanes"], 4), gate_batch_not_slower=bool(gate))
        print("%s: lanes %.1f ms, batch %.1f ms, bytes equal: %s, gate: %s" % (name, med["lanes"], med["batch"], same, gate), flush=True)
        if not same:
            print(json.dumps(res)); sys.exit(1)
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(json.dumps(res, indent=1) + "\n")
    sys.exit(0 if gate_all else 2)


if __name__ == "__main__":
    main()
