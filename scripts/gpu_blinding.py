"""Blinding vectors generated on the GPU from seeds (rofl_blinding_vecs / k_blind_combine) at the sizes of BASELINE cfg 4 / cfg 5, each case
with host output (numpy arrays) and with device output (a torch uint8 tensor on the GPU, written in place), on ONE box in ONE run:

  a  rnd_scalar_vec_seeded for 48 x 55 000 as one blinding_vecs call (one +1 term per vector)
  b  generate_cancelling_scalar_vec_seeded(48, 55 000)
  c  pairwise_blinding_vec for one client with 47 peers at d = 55 000
  d  pairwise_blinding_vecs for 48 hosted clients x 47 peers: 48 * 47 * 27 500 Keccak permutations, reported as permutations per second next
     to the rate of k_nonce_expand in profiles/r06_bench_kernel_stats.csv (cfg 2: 4 chunks x 8 192 x 68 / 2 = 1 114 112 permutations a launch)

beside the code of the parent commit on the same box: pedersen_ops.rnd_scalar_vec(55 000) once and generate_cancelling_scalar_vec(4, 55 000)
once (its scaling to 48 vectors is stated as scaling -- 12 x -- not measured), and EncParamsL2.encrypt_batch at 48 x 55 000 (8-bit, P = 4,
l2_range 32, fp 32/7) with the r2 of all clients generated inside the clock by ONE blinding_vecs call (what a seeded host does: the rows go in as
rand_scalars) against the same call with the same r2 made before the clock started, alternating; the seeded way passes when its median is within
3 % (the spread of this pool's boxes) of the other.  Host clock around every call after one warm-up: every call returns
after its stream has been synchronised.

  python scripts/gpu_blinding.py [--clients 48] [--d 55000] [--reps 7] [--encrypt-reps 5] [--no-parent] [--no-encrypt] [--out profiles/r08_blinding.json]"""
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
from rofl_project_code_amd.api import pedersen_ops as P  # noqa: E402

FP, NB, NPART, L2N = (32, 7), 8, 4, 32


def timed(f, reps):
    f()
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        f()
        ms.append(round((time.perf_counter() - t0) * 1e3, 3))
    return {"ms": ms, "median_ms": float(np.median(ms)), "max_minus_min_ms": round(max(ms) - min(ms), 3)}


def nonce_expand_rate():
    """permutations per second of k_nonce_expand in the cfg 2 benchmark profile (average launch)"""
    path = os.path.join(ROOT, "profiles", "r06_bench_kernel_stats.csv")
    for row in csv.DictReader(open(path)):
        if row["Name"].startswith("rofl::k_nonce_expand("):
            return 4 * 8192 * 68 // 2 / (float(row["AverageNs"]) * 1e-9)
    return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clients", type=int, default=48)
    ap.add_argument("--d", type=int, default=55000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--encrypt-reps", type=int, default=5)
    ap.add_argument("--no-parent", action="store_true")
    ap.add_argument("--no-encrypt", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r08_blinding.json"), help="'' = print only")
    a = ap.parse_args()
    R.set_device(0)
    n, d = a.clients, a.d
    seeds = [bytes([i + 1]) * 32 for i in range(n)]
    pair = {(i, j): P.pairwise_round_seed(b"pair %d %d" % (i, j), 1) for i in range(n) for j in range(i + 1, n)}
    peers = [[(j, pair[min(i, j), max(i, j)]) for j in range(n) if j != i] for i in range(n)]
    dev = torch.empty((n, d, 32), dtype=torch.uint8, device="cuda")
    dealer = [P.cancelling_vec_seed(seeds[0], i) for i in range(n - 1)]
    dealer_terms = [[(s, 1)] for s in dealer] + [[(s, -1) for s in dealer]]
    pair_terms = [P._pairwise_terms(i, peers[i]) for i in range(n)]
    res = {"clients": n, "d": d, "reps": a.reps, "host_clock": "perf_counter around each call after one warm-up", "cases": {}}
    cases = {
        "a_rnd_scalar_vec_seeded_%dx%d" % (n, d): ([[(s, 1)] for s in seeds], lambda: P.blinding_vecs([[(s, 1)] for s in seeds], d)),
        "b_generate_cancelling_seeded_%dx%d" % (n, d): (dealer_terms, lambda: P.generate_cancelling_scalar_vec_seeded(n, d, seeds[0])),
        "c_pairwise_one_client_%d_peers" % (n - 1): (pair_terms[:1], lambda: P.pairwise_blinding_vec(0, peers[0], d)),
        "d_pairwise_%d_hosted_clients" % n: (pair_terms, lambda: P.pairwise_blinding_vecs(list(enumerate(peers)), d)),
    }
    for name, (terms, host_call) in cases.items():
        outs = [dev[v] for v in range(len(terms))]
        c = {"host_output": timed(host_call, a.reps), "device_output": timed(lambda: P.blinding_vecs(terms, d, out=outs), a.reps)}
        got = host_call()
        assert (np.asarray(got).reshape(len(terms), d, 32) == dev[:len(terms)].cpu().numpy()).all(), name      # the two outputs hold the same bytes
        c["keccak_permutations"] = sum(len(t) for t in terms) * ((d + 1) // 2)
        res["cases"][name] = c
        print("%s: host output %.2f ms, device output %.2f ms" % (name, c["host_output"]["median_ms"], c["device_output"]["median_ms"]), flush=True)
    cd = res["cases"]["d_pairwise_%d_hosted_clients" % n]
    rate, ref = cd["keccak_permutations"] / (cd["device_output"]["median_ms"] * 1e-3), nonce_expand_rate()
    res["keccak"] = {"k_blind_combine_permutations_per_s": rate, "k_nonce_expand_permutations_per_s_r06_cfg2": ref, "ratio": rate / ref if ref else None}
    print("k_blind_combine %.3g permutations/s, k_nonce_expand (r06 cfg 2 profile) %.3g" % (rate, ref or 0), flush=True)
    if not a.no_parent:
        t0 = time.perf_counter(); P.rnd_scalar_vec(d); one = (time.perf_counter() - t0) * 1e3
        t0 = time.perf_counter(); P.generate_cancelling_scalar_vec(4, d); four = (time.perf_counter() - t0) * 1e3
        res["parent"] = {"rnd_scalar_vec_%d_ms" % d: round(one, 1), "generate_cancelling_scalar_vec_4x%d_ms" % d: round(four, 1),
                         "generate_cancelling_scalar_vec_%dx%d_ms_by_linear_scaling_not_measured" % (n, d): round(four * n / 4, 1)}
        print("parent: %s" % res["parent"], flush=True)
    if not a.no_encrypt:
        cl = []
        for i in range(n):
            rng = np.random.default_rng(8300 + i)
            x = (rng.integers(-3, 4, size=d) / 128.0).astype(np.float32)
            bl = rng.integers(0, 256, size=(d, 32), dtype=np.uint8); bl[:, 31] &= 0x0F
            cl.append((x, bl))
        ns, rs = [bytes([i % 251 + 1]) * 32 for i in range(n)], [bytes([i + 101]) * 32 for i in range(n)]
        r2 = P.blinding_vecs([[(s, 1)] for s in rs], d)
        with_scalars = lambda: R.EncParamsL2.encrypt_batch([(x, bl, r2[i]) for i, (x, bl) in enumerate(cl)], NB, NPART, L2N, nonce_seeds=ns, fp=FP)
        def with_seeds():
            g = P.blinding_vecs([[(sd, 1)] for sd in rs], d)
            return R.EncParamsL2.encrypt_batch([(x, bl, g[i]) for i, (x, bl) in enumerate(cl)], NB, NPART, L2N, nonce_seeds=ns, fp=FP)
        A, B = with_scalars(), with_seeds()
        same = all(u.serialize() == v.serialize() for u, v in zip(A, B))
        del A, B
        t = {"rand_scalars": [], "seeded_in_the_clock": []}
        for _ in range(a.encrypt_reps):
            for w, f in (("rand_scalars", with_scalars), ("seeded_in_the_clock", with_seeds)):
                t0 = time.perf_counter(); f(); t[w].append(round((time.perf_counter() - t0) * 1e3, 3))
        med = {w: float(np.median(v)) for w, v in t.items()}
        res["encrypt_batch_l2_%dx%d" % (n, d)] = {"ms": t, "median_ms": med, "bytes_equal": bool(same),
                                                   "seeded_within_3_percent_of_rand_scalars": bool(med["seeded_in_the_clock"] <= 1.03 * med["rand_scalars"])}
        print("encrypt_batch: %s" % res["encrypt_batch_l2_%dx%d" % (n, d)], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
