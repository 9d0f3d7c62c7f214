"""The two create legs of a hosted L2 round that used to run client by client -- the per-element Sigma-proof vectors and the L2 sum proofs
-- as per-client calls on the lanes (the way encrypt_batch issued them before rofl_create_sigmaproof_vec_batch and
rofl_create_rangeproof_l2_batch existed) against ONE batched call, and the whole EncParamsL2.encrypt_batch both ways.

In ONE process, after a warm-up of both ways, --reps alternations (seven by default) of
  lanes:  one call per client through params._concurrently (32 host threads, the library's lanes)
  batch:  ONE batched call
each timed with a host clock (every way returns host bytes: the device has been synchronised).  Every client's bytes are asserted equal
between the ways in every repetition.  Shapes: SquareRandProof vectors (completing the range proofs' commitments, as encrypt does) and L2
sum proofs at 48 x 5 000, 25 000, 55 000; RandProof vectors at 48 x 40 000; EncParamsL2.encrypt_batch at 48 x 55 000, 8-bit, P = 4,
l2_range 32, fp 32/7 (parent: the L-inf batch + 2 x 48 per-client thunks; now: three batched calls).

  python scripts/gpu_create_legs_batch.py [--clients 48] [--reps 7] [--cases sq5000,...] [--out profiles/r08_create_legs_batch.json]"""
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
CASES = ["sq5000", "sq25000", "sq55000", "l2_5000", "l2_25000", "l2_55000", "rand40000", "encrypt_l2_55000"]


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
    """(lanes, batch, same): two thunks returning one result per client, and the comparison of two such results"""
    kind, d = case.rstrip("0123456789"), int(case[len(case.rstrip("0123456789")):])
    cl = clients(n, d)
    xs, bls, r2s = [c[0] for c in cl], [c[1] for c in cl], [c[2] for c in cl]
    seeds = [bytes([i % 251 + 1]) * 32 for i in range(n)]
    nonces = lambda: [R.Nonce.seeded(s) for s in seeds]
    pair_same = lambda a, b: not isinstance(a, Exception) and (a[0] == b[0]).all() and (np.asarray(a[1]) == np.asarray(b[1])).all()
    if kind == "sq":
        com = [R.pedersen_ops.commit_vec(R.conversion32.f32_to_scalar_vec(x, fp=FP), bl) for x, bl in zip(xs, bls)]
        one = lambda i, nn: R.square_rand_proof_vec.create_l2rangeproof_vec_existing(xs[i], com[i], bls[i], r2s[i], nonce=nn, fp=FP)
        return (lambda: _concurrently(*[lambda i=i, nn=nn: one(i, nn) for i, nn in enumerate(nonces())]),
                lambda: R.square_rand_proof_vec.create_l2rangeproof_vec_batch(xs, bls, r2s, nonces=nonces(), existing_list=com, fp=FP), pair_same)
    if kind == "rand":
        one = lambda i, nn: R.rand_proof_vec.create_randproof_vec(xs[i], bls[i], nonce=nn, fp=FP)
        return (lambda: _concurrently(*[lambda i=i, nn=nn: one(i, nn) for i, nn in enumerate(nonces())]),
                lambda: R.rand_proof_vec.create_randproof_vec_batch(xs, bls, nonces=nonces(), fp=FP), pair_same)
    if kind == "l2_":
        one = lambda i, nn: R.l2_range_proof_vec.create_rangeproof_l2(xs[i], r2s[i], L2N, P, nonce=nn, fp=FP)
        return (lambda: _concurrently(*[lambda i=i, nn=nn: one(i, nn) for i, nn in enumerate(nonces())]),
                lambda: R.l2_range_proof_vec.create_rangeproof_l2_batch(xs, r2s, L2N, P, nonces=nonces(), fp=FP), pair_same)
    if kind == "encrypt_l2_":
        return (lambda: parent_encrypt_batch_l2(cl, seeds), lambda: R.EncParamsL2.encrypt_batch(cl, NB, P, L2N, nonce_seeds=seeds, fp=FP),
                lambda a, b: a.serialize() == b.serialize())
    raise SystemExit("unknown case " + case)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clients", type=int, default=48)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r08_create_legs_batch.json"), help="'' = print only")
    a = ap.parse_args()
    R.set_device(0)
    res = {"clients": a.clients, "reps": a.reps, "host_clock": "perf_counter around each way, alternating, after one warm-up of each", "cases": {}}
    if a.out and os.path.exists(a.out):      # cases measured by an earlier invocation stay (the cases may be split over several runs)
        res["cases"] = json.load(open(a.out)).get("cases", {})
    ok = True
    for case in a.cases.split(","):
        lanes, batch, same_one = ways_of(case, a.clients)
        ways = {"lanes": lanes, "batch": batch}
        for w in ways:      # warm-up: generator and fixed-base tables, lane workspaces, staging
            ways[w]()
        times = {w: [] for w in ways}
        same = True
        for _ in range(a.reps):
            outs = {}
            for w in ways:
                t0 = time.perf_counter()
                outs[w] = ways[w]()
                times[w].append(round((time.perf_counter() - t0) * 1e3, 3))
            same &= all(same_one(g, s) for g, s in zip(outs["batch"], outs["lanes"]))
            del outs
        med = {w: float(np.median(v)) for w, v in times.items()}
        spread = {w: round(max(v) - min(v), 3) for w, v in times.items()}
        res["cases"][case] = dict(ms=times, median_ms=med, max_minus_min_ms=spread, bytes_equal=bool(same),
                                  batch_not_slower_than_lanes_by_more_than_its_spread=bool(med["batch"] <= med["lanes"] + spread["lanes"]))
        print("%s: lanes %.2f ms (max-min %.2f), batch %.2f ms (max-min %.2f), bytes equal: %s" % (case, med["lanes"], spread["lanes"], med["batch"], spread["batch"], same), flush=True)
        ok &= same
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            open(a.out, "w").write(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
