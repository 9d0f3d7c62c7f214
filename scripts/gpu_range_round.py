"""The server's check of one round of L-inf updates (EncModelParams::verify, params.rs:185-203 / 235-256, for every client of a round,
server.rs:656-687) at the shapes of the paper's e2e runs and of BASELINE cfg 4: 48 clients.

In ONE process, after a warm-up, five alternations of
  (a) loop:   update.verify() for every client, one after the other
  (b) pool16: update.verify() for every client on a 16-thread pool (the reference's num_verif_threads rayon pool)
  (c) batch:  EncParamsRange{,Compressed}.verify_batch(updates)
each timed with a host clock (every way returns host verdicts: the device has been synchronised).  The verdict lists of the three are
asserted equal in every repetition.  Updates are parsed in place from their wire bytes (deserialize(copy=False)), as a server holds them.
Shapes:
  rc_0.013   RangeCompressed, d = 40 000, fp 16/7, range 8, n_partition 64, check_percentage 0.013 (cifar_large.yml's default)
  rc_1.0     the same with check_percentage 1.0
  range_cfg4 Range, d = 55 000, fp 32/7, range 32, n_partition 4, check_percentage 1.0 (BASELINE cfg 4)
rofl_set_option("verify_batch", 2) for all three ways (one random-weighted range-proof equation per batch call).  --legs also times the two
legs of verify_batch alone, one after the other (what the batch runs side by side): _rand_batch and the range-proof batch over k pairs.

  python scripts/gpu_range_round.py [--clients 48] [--reps 5] [--shapes rc_0.013,rc_1.0,range_cfg4] [--ways loop,pool16,batch]
                                    [--out profiles/r07_range_round.json] [--rounds DIR] [--legs]"""
import argparse
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import rofl_project_code_amd as R  # noqa: E402

SHAPES = {
    "rc_0.013": dict(cls="EncParamsRangeCompressed", d=40000, fp=(16, 7), nb=8, P=64, check=0.013),
    "rc_1.0": dict(cls="EncParamsRangeCompressed", d=40000, fp=(16, 7), nb=8, P=64, check=1.0),
    "range_cfg4": dict(cls="EncParamsRange", d=55000, fp=(32, 7), nb=32, P=4, check=1.0),
}
SEED = b"\x5e" * 32


def make_round(cls, n, sh, seed0, cache=None):
    """the round's wire messages, parsed in place; cache: an .npy file of the messages (written when absent), so that a profiled run
    of the batched call does not trace the creation of its inputs"""
    if cache and os.path.exists(cache):
        raw = np.load(cache)
        bufs = [np.ascontiguousarray(r) for r in raw]
        return [cls.deserialize(b, copy=False) for b in bufs], bufs
    bufs = []
    for i in range(n):
        rng = np.random.default_rng(seed0 + i)
        x = (rng.integers(-100, 100, size=sh["d"]) / 128.0).astype(np.float32)      # inside the 8-bit range at frac 7
        bl = rng.integers(0, 256, size=(sh["d"], 32), dtype=np.uint8); bl[:, 31] &= 0x0F
        u = cls.encrypt(x, bl, sh["nb"], sh["P"], sh["check"], nonce_seed=bytes([i % 251 + 1]) * 32, fp=sh["fp"])
        bufs.append(u.serialize(as_array=True))
    if cache:
        np.save(cache, np.stack(bufs))      # (all messages of a shape have one length)
    return [cls.deserialize(b, copy=False) for b in bufs], bufs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clients", type=int, default=48)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--ways", default="loop,pool16,batch")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r07_range_round.json"), help="'' = print only")
    ap.add_argument("--legs", action="store_true", help="also time the two legs of verify_batch alone (randomness proofs; range proofs)")
    ap.add_argument("--rounds", default="", help="directory for the rounds' messages: reused when present, written otherwise")
    a = ap.parse_args()
    R.set_device(0)
    R.set_option("verify_batch", 2)
    pool = ThreadPoolExecutor(max_workers=16)
    res = {"clients": a.clients, "reps": a.reps, "verify_batch_option": 2, "host_clock": "perf_counter around each way", "shapes": {}}
    for name in a.shapes.split(","):
        sh = SHAPES[name]
        cls = getattr(R, sh["cls"])
        t = time.perf_counter()
        cache = os.path.join(a.rounds, "%s_%d.npy" % (name, a.clients)) if a.rounds else None
        if cache:
            os.makedirs(a.rounds, exist_ok=True)
        ups, _keep = make_round(cls, a.clients, sh, 7000, cache)
        gen_s = time.perf_counter() - t
        fp = sh["fp"]
        ways = {"loop": lambda: [u.verify(verifier_seed=SEED, fp=fp) for u in ups],
                "pool16": lambda: list(pool.map(lambda u: u.verify(verifier_seed=SEED, fp=fp), ups)),
                "batch": lambda: cls.verify_batch(ups, verifier_seed=SEED, fp=fp)}
        k = R.params._num_checked(sh["d"], sh["check"])
        legs = {"leg_rand": lambda: cls._rand_batch(ups),
                "leg_range": lambda: R.range_proof_vec.verify_rangeproof_batch([u.range_proofs for u in ups], [u.enc_values[:k] for u in ups], sh["nb"],
                                                                             verifier_seed=SEED, fp=fp, commit_stride=64)} if a.legs else {}
        ways.update(legs)
        names = [w for w in a.ways.split(",") if w in ways] + list(legs)
        for w in names:      # warm-up: generator tables, lane workspaces, staging
            ways[w]()
        times = {w: [] for w in names}
        same = True
        verdicts = None
        for _ in range(a.reps):
            outs = {}
            for w in names:
                t0 = time.perf_counter()
                outs[w] = ways[w]()
                times[w].append(round((time.perf_counter() - t0) * 1e3, 3))
            verdicts = outs[names[0]]
            same &= all(outs[w] == verdicts for w in names if w not in legs)
        med = {w: float(np.median(v)) for w, v in times.items()}
        out = dict(sh, k=k, input_generation_s=round(gen_s, 2), ms=times, median_ms=med, verdicts_equal=bool(same),
                   all_verified=bool(verdicts is not None and all(verdicts)))
        if "batch" in med and "pool16" in med:
            out["batch_over_pool16"] = round(med["batch"] / med["pool16"], 4)
        if "batch" in med and "loop" in med:
            out["batch_over_loop"] = round(med["batch"] / med["loop"], 4)
        res["shapes"][name] = out
        print("%s: %s, verdicts equal: %s" % (name, ", ".join("%s %.1f ms" % (w, med[w]) for w in names), same), flush=True)
        if not same:
            print(json.dumps(res)); sys.exit(1)
        del ups, _keep
    pool.shutdown()
    R.set_option("verify_batch", 1)
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
