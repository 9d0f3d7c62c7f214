"""The two create legs of a hosted L2 round that used to run client by client -- the per-element Sigma-proof vectors and the L2 sum proofs
-- as per-client calls on the lanes (the way encrypt_batch issued them before rofl_create_sigmaproof_vec_batch and
rofl_create_rangeproof_l2_batch existed) against ONE batched call, and the whole EncParamsL2.encrypt_batch both ways.

In ONE process, after a warm-up of the chosen ways, --reps alternations (seven by default) of
  lanes:   one call per client through params._concurrently (32 host threads, the library's lanes)
  single:  one call per client, one client at a time, each call timed: the one-client latency (median per call, max - min over all calls)
  batch:   ONE batched call
each timed with a host clock (every way returns host bytes: the device has been synchronised).  Every client's bytes are asserted equal
between the ways in every repetition.  Shapes: SquareRandProof vectors (sq: completing the range proofs' commitments, as encrypt does;
sqown: computing their own) and L2 sum proofs at 48 x 5 000, 25 000, 55 000; RandProof vectors at 48 x 40 000; EncParamsL2.encrypt_batch
at 48 x 55 000, 8-bit, P = 4, l2_range 32, fp 32/7 (before the batched create entries: the L-inf batch + 2 x 48 per-client thunks; now:
three batched calls).  With --parent JSON (this script's output on the parent commit, same box, same job) every way of every case is
gated: its median may not exceed the parent's by more than the parent run's own max - min of that way (exit status 2 when one does).

  python scripts/gpu_create_legs_batch.py [--clients 48] [--reps 7] [--cases sq5000,...] [--ways lanes,single,batch] [--parent JSON]
                                          [--out profiles/r08_create_legs_batch.json]"""
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
from rofl_project_code_amd.params import _concurrently, _sub_nonce, witness_digest  # noqa: E402

FP, NB, P, L2N = (32, 7), 8, 4, 32
CASES = ["sq5000", "sq25000", "sq55000", "l2_5000", "l2_25000", "l2_55000", "rand40000", "encrypt_l2_55000"]      # (the default; sqown<d> on request)


def clients(n, d):
    out = []
    for i in range(n):
        rng = np.random.default_rng(8300 + i)
        x = (rng.integers(-3, 4, size=d) / 128.0).astype(np.float32)      # inside the 8-bit range; sum k^2 < 2^24, so the f32 shadow sum is exact
        bl = rng.integers(0, 256, size=(d, 32), dtype=np.uint8); bl[:, 31] &= 0x0F
        r2 = rng.integers(0, 256, size=(d, 32), dtype=np.uint8); r2[:, 31] &= 0x0F
        out.append((x, bl, r2))
    return out


def parent_encrypt_batch_l2(cl, seeds):
    """EncParamsL2.encrypt_batch as it issued its legs before the batched create entries: the L-inf batch and 2 n per-client thunks"""
    cls, fp, n = R.EncParamsL2, FP, len(cl)
    xs, bls, r2s = [c[0] for c in cl], [c[1] for c in cl], [c[2] for c in cl]
    clipped = [R.range_proof_vec.clip_f32_to_range_vec(x, NB, fp=fp) for x in xs]
    d = xs[0].size
    wds = [witness_digest(x, bl, r2) for x, bl, r2 in zip(xs, bls, r2s)]
    enc_all = R.pedersen_ops.commit_vec(np.concatenate([R.conversion32.f32_to_scalar_vec(c, fp=fp) for c in clipped]), np.concatenate(bls))
    enc_com = [enc_all[i * d:(i + 1) * d] for i in range(n)]
    thunks = [lambda: R.range_proof_vec.create_rangeproof_batch(clipped, bls, NB, P, nonces=[_sub_nonce(sd, b"range", wd) for sd, wd in zip(seeds, wds)], fp=fp)]
    for i in range(n):
        thunks.append(lambda i=i: R.l2_range_proof_vec.create_rangeproof_l2(clipped[i], r2s[i], L2N, P, nonce=_sub_nonce(seeds[i], b"l2", wds[i]), fp=fp))
        thunks.append(lambda i=i: R.square_rand_proof_vec.create_l2rangeproof_vec_existing(clipped[i], enc_com[i], bls[i], r2s[i], nonce=_sub_nonce(seeds[i], b"sq", wds[i]), fp=fp))
    res = _concurrently(*thunks)
    return [cls(res[2 + 2 * i][1], res[2 + 2 * i][0], res[0][i][0], res[1 + 2 * i][0], NB, L2N) for i in range(n)]


def ways_of(case, n):
    """(lanes, batch, same, one): two thunks returning one result per client, the comparison of two such results, and one client's call
    one(i, nonce) (None where a way is not a call per client)"""
    kind, d = case.rstrip("0123456789"), int(case[len(case.rstrip("0123456789")):])
    cl = clients(n, d)
    xs, bls, r2s = [c[0] for c in cl], [c[1] for c in cl], [c[2] for c in cl]
    seeds = [bytes([i % 251 + 1]) * 32 for i in range(n)]
    nonces = lambda: [R.Nonce.seeded(s) for s in seeds]
    pair_same = lambda a, b: not isinstance(a, Exception) and (a[0] == b[0]).all() and (np.asarray(a[1]) == np.asarray(b[1])).all()
    lanes_of = lambda one: lambda: _concurrently(*[lambda i=i, nn=nn: one(i, nn) for i, nn in enumerate(nonces())])
    if kind in ("sq", "sqown"):
        com = [R.pedersen_ops.commit_vec(R.conversion32.f32_to_scalar_vec(x, fp=FP), bl) for x, bl in zip(xs, bls)] if kind == "sq" else [None] * n
        one = lambda i, nn: R.square_rand_proof_vec.create_l2rangeproof_vec(xs[i], bls[i], r2s[i], nonce=nn, existing=com[i], fp=FP)
        return (lanes_of(one), lambda: R.square_rand_proof_vec.create_l2rangeproof_vec_batch(xs, bls, r2s, nonces=nonces(), existing_list=com if kind == "sq" else None, fp=FP),
                pair_same, one)
    if kind == "rand":
        one = lambda i, nn: R.rand_proof_vec.create_randproof_vec(xs[i], bls[i], nonce=nn, fp=FP)
        return lanes_of(one), lambda: R.rand_proof_vec.create_randproof_vec_batch(xs, bls, nonces=nonces(), fp=FP), pair_same, one
    if kind == "l2_":
        one = lambda i, nn: R.l2_range_proof_vec.create_rangeproof_l2(xs[i], r2s[i], L2N, P, nonce=nn, fp=FP)
        return lanes_of(one), lambda: R.l2_range_proof_vec.create_rangeproof_l2_batch(xs, r2s, L2N, P, nonces=nonces(), fp=FP), pair_same, one
    if kind == "encrypt_l2_":
        return (lambda: parent_encrypt_batch_l2(cl, seeds), lambda: R.EncParamsL2.encrypt_batch(cl, NB, P, L2N, nonce_seeds=seeds, fp=FP),
                lambda a, b: a.serialize() == b.serialize(), None)
    raise SystemExit("unknown case " + case)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clients", type=int, default=48)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--ways", default="lanes,batch")
    ap.add_argument("--parent", default="", help="the JSON this script wrote on the parent commit: gate every way against it")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r08_create_legs_batch.json"), help="'' = print only")
    a = ap.parse_args()
    R.set_device(0)
    res = {"clients": a.clients, "reps": a.reps, "host_clock": "perf_counter around each way, alternating, after one warm-up of each", "cases": {}}
    if a.out and os.path.exists(a.out):      # cases measured by an earlier invocation stay (the cases may be split over several runs)
        res["cases"] = json.load(open(a.out)).get("cases", {})
    parent = json.load(open(a.parent))["cases"] if a.parent else {}
    ok = gate_all = True
    for case in a.cases.split(","):
        lanes, batch, same_one, one = ways_of(case, a.clients)
        calls = []      # the single way's own clock: one entry per call

        def single():
            out = []
            for i in range(a.clients):
                nn = R.Nonce.seeded(bytes([i % 251 + 1]) * 32)
                t0 = time.perf_counter()
                out.append(one(i, nn))
                calls.append(round((time.perf_counter() - t0) * 1e3, 3))
            return out
        ways = {w: f for w, f in (("lanes", lanes), ("single", single), ("batch", batch)) if w in a.ways.split(",") and (w != "single" or one)}
        names = list(ways)
        for w in names:      # warm-up: generator and fixed-base tables, lane workspaces, staging
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
            same &= all(same_one(g, s) for w in names[1:] for g, s in zip(outs[w], outs[names[0]]))
            del outs
        if "single" in times:
            times["single"] = list(calls)      # per call, not per sweep of the clients
        med = {w: float(np.median(v)) for w, v in times.items()}
        spread = {w: round(max(v) - min(v), 3) for w, v in times.items()}
        gates = {}
        if "lanes" in med and "batch" in med:
            gates["batch_not_slower_than_lanes_by_more_than_its_spread"] = bool(med["batch"] <= med["lanes"] + spread["lanes"])
        for w in names:
            if case in parent and w in parent[case]["median_ms"]:
                gates[w + "_not_slower_than_parent"] = bool(med[w] <= parent[case]["median_ms"][w] + parent[case]["max_minus_min_ms"][w])
        gate_all &= all(v for k, v in gates.items() if k.endswith("_parent"))
        res["cases"][case] = dict(ms=times, median_ms=med, max_minus_min_ms=spread, bytes_equal=bool(same), **gates)
        print("%s: %s, bytes equal: %s, gates: %s" % (case, ", ".join("%s %.2f ms (max-min %.2f)" % (w, med[w], spread[w]) for w in names), same, gates), flush=True)
        ok &= same
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            open(a.out, "w").write(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))
    sys.exit(1 if not ok else 0 if gate_all else 2)


if __name__ == "__main__":
    main()
