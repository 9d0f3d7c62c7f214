"""Extraction of a round that rejected somebody (rofl_acc_extract_opened / _terms, k_acc_open) at the sizes of BASELINE cfg 4 / cfg 5: 48 clients
with pairwise blindings, 3 of them rejected, d = 40 000 and 55 000, fp 32/7, on ONE box in ONE run:

  a  DeviceAccumulator.extract_opened(opening_terms=...)     the opening built on the device from the 45 x 3 shared seeds
  b  DeviceAccumulator.extract_opened(opening=device tensor)  the opening handed in on the device
  c  EncModelParamsAccumulator.extract(opening=...)    the composed route from a host-held opening and host-held sums (commit_vec, add_rp_vec,
                                                       a byte comparison, discrete_log_vec): the only way to the answer on the parent commit
  d  DeviceAccumulator.extract() of the fully cancelling round of the same shape: the floor -- BSGS and the download are common to all four

Host clock around every call after warm-up (every call returns after its stream has been synchronised); median and max - min over --reps
repetitions.  All four give the same bytes where they answer the same question (a, b, c), checked before anything is timed.

The time of k_acc_open itself comes from a profiler run of its own (a kernel trace with statistics around `--kernel-only`, which runs case a
a few times and nothing else); --kernel-stats <csv> merges that run's row into the result file.

  python scripts/gpu_extract_opened.py [--clients 48] [--rejected 5,17,40] [--d 40000,55000] [--reps 20] [--kernel-only] [--kernel-stats CSV]
                                       [--out profiles/r09_extract_opened.json]"""
import argparse
import csv
import json
import os
import sys
import time

import numpy as np
import torch

torch.cuda.init()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import rofl_project_code_amd as R  # noqa: E402
from rofl_project_code_amd.api import conversion32, pedersen_ops as P  # noqa: E402

FP = (32, 7)


def timed(f, reps, warmup=2):
    for _ in range(warmup):
        f()
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        f()
        ms.append(round((time.perf_counter() - t0) * 1e3, 3))
    return {"ms": ms, "median_ms": float(np.median(ms)), "max_minus_min_ms": round(max(ms) - min(ms), 3)}


def make_round(n, d):
    """n clients' records (uint8[d, 64] each) under pairwise blindings, their values, and the pair seeds"""
    seeds = {(i, j): P.pairwise_round_seed(b"pair %d %d" % (i, j), 9) for i in range(n) for j in range(i + 1, n)}
    peers = [[(j, seeds[min(i, j), max(i, j)]) for j in range(n) if j != i] for i in range(n)]
    bl = P.pairwise_blinding_vecs(list(enumerate(peers)), d)
    xs, recs = [], []
    for i in range(n):
        x = (np.random.default_rng(9100 + i).integers(-3, 4, size=d) / 128.0).astype(np.float32)
        L = P.commit_vec(conversion32.f32_to_scalar_vec(x, fp=FP), bl[i])
        recs.append(np.ascontiguousarray(np.concatenate([L, P.commit_no_blinding_vec(bl[i])], axis=1)))
        xs.append(x)
    return xs, recs, seeds


def kernel_row(path):
    for row in csv.DictReader(open(path)):
        if row["Name"].startswith("rofl::k_acc_open("):
            return {"calls": int(row["Calls"]), "average_us": float(row["AverageNs"]) / 1e3, "min_us": float(row["MinNs"]) / 1e3, "max_us": float(row["MaxNs"]) / 1e3}
    return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clients", type=int, default=48)
    ap.add_argument("--rejected", default="5,17,40")
    ap.add_argument("--d", default="40000,55000")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--kernel-only", action="store_true", help="case a three times and nothing else: the run a profiler wraps")
    ap.add_argument("--kernel-stats", default="", help="kernel statistics (csv) of a profiled --kernel-only run at the LAST d of --d: merged into --out")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r09_extract_opened.json"), help="'' = print only")
    a = ap.parse_args()
    n, rej = a.clients, sorted(int(x) for x in a.rejected.split(","))
    acc_ids = [i for i in range(n) if i not in rej]
    ds = [int(x) for x in a.d.split(",")]
    if a.kernel_stats:
        res = json.load(open(a.out))
        res["k_acc_open_d%d" % ds[-1]] = kernel_row(a.kernel_stats)
        open(a.out, "w").write(json.dumps(res, indent=1) + "\n")
        print(json.dumps(res["k_acc_open_d%d" % ds[-1]]))
        return
    R.set_device(0)
    R.api.set_fp(*FP)
    res = {"clients": n, "rejected": rej, "reps": a.reps, "fp": list(FP), "host_clock": "perf_counter around each call after two warm-up calls", "cases": {}}
    for d in (ds[-1:] if a.kernel_only else ds):
        xs, recs, seeds = make_round(n, d)
        terms = P.pairwise_residual_terms(acc_ids, rej, seeds)
        with R.DeviceAccumulator(d) as part, R.DeviceAccumulator(d) as full:
            part._add([recs[i] for i in acc_ids], 64)
            if a.kernel_only:
                for _ in range(3):
                    assert part.extract_opened(opening_terms=terms) is not None
                continue
            full._add(recs, 64)
            s_host = P.blinding_vecs([terms], d)[0]
            s_dev = torch.from_numpy(s_host).to("cuda")
            host = R.EncModelParamsAccumulator(d)
            host.acc = part.export()
            want = np.sum(np.stack([xs[i] for i in acc_ids]).astype(np.float64), axis=0).astype(np.float32).tobytes()
            assert part.extract() is None
            for f in (lambda: part.extract_opened(opening_terms=terms), lambda: part.extract_opened(opening=s_dev), lambda: host.extract(opening=s_host)):
                assert f().tobytes() == want
            assert full.extract() is not None
            c = {
                "a_extract_opening_terms": timed(lambda: part.extract_opened(opening_terms=terms), a.reps),
                "b_extract_opening_device_tensor": timed(lambda: part.extract_opened(opening=s_dev), a.reps),
                "c_composed_host_route": timed(lambda: host.extract(opening=s_host), a.reps),
                "d_plain_extract_cancelling_round": timed(lambda: full.extract(), a.reps),
            }
            c["terms"] = len(terms)
            res["cases"]["d%d" % d] = c
            print("d = %d: %s" % (d, ", ".join("%s %.2f ms (+-%.2f)" % (k[0], v["median_ms"], v["max_minus_min_ms"]) for k, v in c.items() if isinstance(v, dict))), flush=True)
    if a.kernel_only:
        return
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
