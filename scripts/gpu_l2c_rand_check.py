"""What the opt-in CompressedRandProof check of EncL2Compressed updates costs, and that the reference-faithful path did not get slower:
48 clients of d = 55 000 (BASELINE cfg 5's shape: fp 32/7, 8-bit L-inf legs, 32-bit sum proof, n_partition 4), blindings that cancel.

In ONE process, after a warm-up, five alternations of
  round_loose   DeviceRound(EncParamsL2Compressed): ingest, verify, accumulate_into (+ extract), timed apart and together
  round_strict  DeviceRound(EncParamsL2CompressedStrict): the same -- ingest also hashes the transcripts, verify also runs the randomness leg
  batch_loose   EncParamsL2Compressed.verify_batch on host bytes
  batch_strict  EncParamsL2CompressedStrict.verify_batch on host bytes (the strided call as a fourth leg)
each timed with a host clock (every way returns host values: the device has been synchronised).  The verdict lists of all ways are
compared in every repetition (all True: an honest round), and the aggregates with the values' sum.

The extra leg is new work and has no bound.  The gate is about the reference-faithful ways: run the script with --ways loose on a checkout
of the commit before (which has no strict class), same box, same job, same --rounds directory, and pass its JSON as --parent: the median of
round_loose and of batch_loose here must not exceed the parent's median by more than the parent's max - min.

  python scripts/gpu_l2c_rand_check.py [--clients 48] [--d 55000] [--reps 5] [--ways loose,strict] [--rounds DIR] [--parent FILE] [--out profiles/r11_l2c_rand_check.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import rofl_project_code_amd as R  # noqa: E402

FP, NB, P, L2N = (32, 7), 8, 4, 32
SEED = b"\x5e" * 32


def make_round(n, d, cache=None):
    """(values' f32 sum, the messages); cache: an .npz of the messages (written when absent), so that the other checkout reads the same round"""
    if cache and os.path.exists(cache):
        z = np.load(cache)
        return z["total"], [np.ascontiguousarray(r) for r in z["msgs"]]
    rng = np.random.default_rng(8200)
    xs = [(rng.integers(-3, 4, size=d) / 128.0).astype(np.float32) for _ in range(n)]
    bls = []
    for _ in range(n - 1):
        b = rng.integers(0, 256, size=(d, 32), dtype=np.uint8); b[:, 31] &= 0x0F
        bls.append(b)
    bls.append(R.pedersen_ops.add_scalar_vec(np.zeros((d, 32), np.uint8), R.pedersen_ops.add_scalar_vec_vec(bls), subtract=True))      # the blindings cancel
    bufs = []
    for i0 in range(0, n, 8):      # eight clients per encrypt_batch: the device holds one batch's workspaces at a time
        cl = []
        for i in range(i0, min(n, i0 + 8)):
            r2 = rng.integers(0, 256, size=(d, 32), dtype=np.uint8); r2[:, 31] &= 0x0F
            cl.append((xs[i], bls[i], r2))
        ups = R.EncParamsL2Compressed.encrypt_batch(cl, NB, P, L2N, nonce_seeds=[bytes([i % 251 + 1]) * 32 for i in range(i0, i0 + len(cl))], fp=FP)
        bufs += [u.serialize(as_array=True) for u in ups]
    total = np.sum(np.stack(xs).astype(np.float64), axis=0).astype(np.float32)
    if cache:
        np.savez(cache, msgs=np.stack(bufs), total=total)      # (all messages of the shape have one length)
    return total, bufs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clients", type=int, default=48)
    ap.add_argument("--d", type=int, default=55000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--ways", default="loose,strict", help="'loose' alone runs on a tree without the strict class")
    ap.add_argument("--rounds", default="", help="directory for the round's messages: reused when present, written otherwise")
    ap.add_argument("--parent", default="", help="the JSON of a --ways loose run on the commit before: evaluates the gate")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r11_l2c_rand_check.json"), help="'' = print only")
    a = ap.parse_args()
    kinds = a.ways.split(",")
    R.set_device(0)
    R.api.set_fp(*FP)
    n, d = a.clients, a.d
    cache = os.path.join(a.rounds, "l2c_%d_%d.npz" % (d, n)) if a.rounds else None
    if cache:
        os.makedirs(a.rounds, exist_ok=True)
    t = time.perf_counter()
    total, bufs = make_round(n, d, cache)
    gen_s = time.perf_counter() - t
    classes = {"loose": R.EncParamsL2Compressed}
    if "strict" in kinds:
        classes["strict"] = R.EncParamsL2CompressedStrict
    ups = {k: [c.deserialize(b, copy=False) for b in bufs] for k, c in classes.items() if k in kinds}
    acc = R.DeviceAccumulator(d)
    rounds = {k: R.DeviceRound(classes[k], d, max_clients=n) for k in ups}
    split = {k: {p: [] for p in ("ingest", "verify", "accumulate", "extract")} for k in ups}

    def round_way(k):
        rnd, sp = rounds[k], split[k]
        acc.reset(); rnd.reset()
        t0 = time.perf_counter(); rnd.ingest(ups[k])
        t1 = time.perf_counter(); ok = rnd.verify(verifier_seed=SEED, fp=FP)
        t2 = time.perf_counter(); rnd.accumulate_into(acc, accept=ok)
        t3 = time.perf_counter(); agg = acc.extract(fp=FP)
        t4 = time.perf_counter()
        for p, dt in zip(("ingest", "verify", "accumulate", "extract"), (t1 - t0, t2 - t1, t3 - t2, t4 - t3)):
            sp[p].append(round(dt * 1e3, 3))
        return ok, agg

    ways = {}
    for k in ups:
        ways["round_" + k] = lambda k=k: round_way(k)
        ways["batch_" + k] = lambda k=k: (classes[k].verify_batch(ups[k], verifier_seed=SEED, fp=FP), None)
    names = list(ways)
    for w in names:      # warm-up: generator tables, lane workspaces, staging, the BSGS table
        ways[w]()
    for sp in split.values():
        for v in sp.values():
            v.clear()
    times = {w: [] for w in names}
    good = True
    for _ in range(a.reps):
        for w in names:
            t0 = time.perf_counter()
            ok, agg = ways[w]()
            times[w].append(round((time.perf_counter() - t0) * 1e3, 3))
            good &= ok == [True] * n and (agg is None) == w.startswith("batch_") and (agg is None or agg.tobytes() == total.tobytes())
    med = {w: float(np.median(v)) for w, v in times.items()}
    spread = {w: round(max(v) - min(v), 3) for w, v in times.items()}
    res = dict(clients=n, d=d, fp=list(FP), prove_range=NB, n_partition=P, l2_range=L2N, reps=a.reps, ways=names, host_clock="perf_counter around each way",
               round_creation_s=round(gen_s, 2), ms=times, median_ms=med, max_minus_min_ms=spread,
               round_parts_median_ms={k: {p: float(np.median(v)) for p, v in sp.items()} for k, sp in split.items()},
               round_parts_max_minus_min_ms={k: {p: round(max(v) - min(v), 3) for p, v in sp.items()} for k, sp in split.items()},
               verdicts_and_aggregates_right=bool(good))
    gate = True
    if a.parent:
        par = json.load(open(a.parent))
        res["parent"] = {w: dict(median_ms=par["median_ms"][w], max_minus_min_ms=par["max_minus_min_ms"][w], ms=par["ms"][w]) for w in ("round_loose", "batch_loose")}
        res["parent_round_parts_median_ms"] = par["round_parts_median_ms"]["loose"]
        res["gate_loose_not_slower_than_parent"] = {w: bool(med[w] <= par["median_ms"][w] + par["max_minus_min_ms"][w]) for w in ("round_loose", "batch_loose")}
        gate = all(res["gate_loose_not_slower_than_parent"].values())
    for w in names:
        print("%s: median %.1f ms, max - min %.1f ms" % (w, med[w], spread[w]), flush=True)
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(json.dumps(res, indent=1) + "\n")
    for rnd in rounds.values():
        rnd.close()
    acc.close()
    sys.exit(0 if good and gate else (1 if not good else 2))


if __name__ == "__main__":
    main()
