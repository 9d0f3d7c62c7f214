"""The server's part of one round -- check every client's proofs, add the accepted updates into the round's sum, extract the aggregate
(server.rs:474-521, 656-714; params.rs:74-147, 181-291) -- at BASELINE's cfg-4 and cfg-5 shapes, 48 clients, two ways:

  (a) cls.verify_batch(updates) -> DeviceAccumulator.accumulate_batch(accepted) -> extract()       every call uploads and decodes on its own
  (b) DeviceRound.ingest(updates) -> verify() -> accumulate_into(acc, accept) -> extract()          one upload, every record point decoded once

In ONE process, after a warm-up of each way, --reps alternations of (a) and (b), a host clock around each way (both end in host-visible
results: verdicts and the f32 aggregate); verdict lists and aggregates are asserted equal in every repetition; ingest / verify /
accumulate / extract of (b) are also timed apart, and the decode counter (rofl_dbg_point_decodes) is read around each way when the
library has it.  Updates are parsed in place from their wire bytes (deserialize(copy=False)); their blindings cancel over the round, so the
round verifies AND extracts.  rofl_set_option("verify_batch", 2).
Shapes:
  range_cfg4  EncParamsRange, d = 55 000, fp 32/7, range 32, n_partition 4, check_percentage 1.0 (BASELINE cfg 4)
  l2_cfg5     EncParamsL2, d = 55 000, fp 32/7, 8-bit L-inf legs, 32-bit sum proof, n_partition 4 (BASELINE cfg 5)
  range_compressed_e2e  EncParamsRangeCompressed, d = 40 000, fp 16/7, range 8, n_partition 64, check_percentage 0.013 (the shape of the
              reference's end-to-end experiments; --check 1.0 for every element range-checked).  Not among the default shapes.
Way (a) uses nothing that the commit before the device-resident round lacks: the same file with --ways a runs on a checkout of that commit
(same box, same job) and gives the figure (b) is compared with.

  python scripts/gpu_round_session.py [--clients 48] [--reps 5] [--shapes range_cfg4,l2_cfg5] [--ways a,b] [--warmup 1] [--check P]
                                      [--out profiles/r08_round_session.json] [--rounds DIR]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import rofl_project_code_amd as R  # noqa: E402

SHAPES = {
    "range_cfg4": dict(cls="EncParamsRange", d=55000, fp=(32, 7), nb=32, P=4, check=1.0),
    "l2_cfg5": dict(cls="EncParamsL2", d=55000, fp=(32, 7), nb=8, P=4, l2n=32),
    "range_compressed_e2e": dict(cls="EncParamsRangeCompressed", d=40000, fp=(16, 7), nb=8, P=64, check=0.013),
}
SEED = b"\x5e" * 32


def make_round(cls, n, sh, seed0, cache=None):
    """(values' f32 sum, updates parsed in place, their buffers); cache: an .npz of the messages (written when absent), so that the other
    checkout and a profiled run read the same round instead of creating it again"""
    d, fp = sh["d"], sh["fp"]
    if cache and os.path.exists(cache):
        z = np.load(cache)
        bufs = [np.ascontiguousarray(r) for r in z["msgs"]]
        return z["total"], [cls.deserialize(b, copy=False) for b in bufs], bufs
    rng = np.random.default_rng(seed0)
    xs = [(rng.integers(-3, 4, size=d) / 128.0).astype(np.float32) for _ in range(n)]
    bls = []
    for _ in range(n - 1):
        b = rng.integers(0, 256, size=(d, 32), dtype=np.uint8); b[:, 31] &= 0x0F
        bls.append(b)
    bls.append(R.pedersen_ops.add_scalar_vec(np.zeros((d, 32), np.uint8), R.pedersen_ops.add_scalar_vec_vec(bls), subtract=True))      # the blindings cancel
    bufs = []
    for i, (x, bl) in enumerate(zip(xs, bls)):
        ns = bytes([i % 251 + 1]) * 32
        if "l2n" in sh:
            r2 = rng.integers(0, 256, size=(d, 32), dtype=np.uint8); r2[:, 31] &= 0x0F
            u = cls.encrypt(x, bl, sh["nb"], sh["P"], sh["l2n"], nonce_seed=ns, rand_scalars=r2, fp=fp)
        else:
            u = cls.encrypt(x, bl, sh["nb"], sh["P"], sh["check"], nonce_seed=ns, fp=fp)
        bufs.append(u.serialize(as_array=True))
    total = np.sum(np.stack(xs).astype(np.float64), axis=0).astype(np.float32)
    if cache:
        np.savez(cache, msgs=np.stack(bufs), total=total)      # (all messages of a shape have one length)
    return total, [cls.deserialize(b, copy=False) for b in bufs], bufs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clients", type=int, default=48)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shapes", default="range_cfg4,l2_cfg5")
    ap.add_argument("--check", type=float, default=None, help="check_percentage of the Range shapes instead of the shape's own")
    ap.add_argument("--ways", default="a,b")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r08_round_session.json"), help="'' = print only")
    ap.add_argument("--rounds", default="", help="directory for the rounds' messages: reused when present, written otherwise")
    a = ap.parse_args()
    ways = a.ways.split(",")
    R.set_device(0)
    R.set_option("verify_batch", 2)
    decodes = getattr(R.api, "point_decodes", None)
    res = {"clients": a.clients, "reps": a.reps, "ways": ways, "verify_batch_option": 2, "host_clock": "perf_counter around each way", "shapes": {}}
    for name in a.shapes.split(","):
        sh = dict(SHAPES[name])
        if a.check is not None and "check" in sh:
            sh["check"] = a.check
            name = "%s_check%g" % (name, a.check)
        cls, d, fp = getattr(R, sh["cls"]), sh["d"], sh["fp"]
        R.api.set_fp(*fp)
        t = time.perf_counter()
        cache = os.path.join(a.rounds, "%s_%d.npz" % (name, a.clients)) if a.rounds else None
        if cache:
            os.makedirs(a.rounds, exist_ok=True)
        total, ups, _keep = make_round(cls, a.clients, sh, 8000, cache)
        gen_s = time.perf_counter() - t
        acc = R.DeviceAccumulator(d)
        rnd = R.DeviceRound(cls, d, max_clients=a.clients) if "b" in ways else None
        split = {k: [] for k in ("ingest", "verify", "accumulate", "extract")}

        def way_a():
            acc.reset()
            ok = cls.verify_batch(ups, verifier_seed=SEED, fp=fp)
            acc.accumulate_batch([u for u, o in zip(ups, ok) if o])
            return ok, acc.extract(fp=fp)

        def way_b(record=True):
            acc.reset(); rnd.reset()
            t0 = time.perf_counter(); rnd.ingest(ups)
            t1 = time.perf_counter(); ok = rnd.verify(verifier_seed=SEED, fp=fp)
            t2 = time.perf_counter(); rnd.accumulate_into(acc, accept=ok)
            t3 = time.perf_counter(); agg = acc.extract(fp=fp)
            t4 = time.perf_counter()
            if record:
                for k, v in zip(("ingest", "verify", "accumulate", "extract"), (t1 - t0, t2 - t1, t3 - t2, t4 - t3)):
                    split[k].append(round(v * 1e3, 3))
            return ok, agg
        run = {"a": way_a, "b": way_b}
        for w in ways:
            for _ in range(a.warmup):      # generator tables, lane workspaces, staging, the baby-step table
                run[w](False) if w == "b" else run[w]()
        times = {w: [] for w in ways}
        counts = {w: [] for w in ways}
        same = True
        for _ in range(a.reps):
            outs = {}
            for w in ways:
                c0 = decodes() if decodes else 0
                t0 = time.perf_counter()
                outs[w] = run[w]()
                times[w].append(round((time.perf_counter() - t0) * 1e3, 3))
                if decodes:
                    counts[w].append(decodes() - c0)
            for w in ways:
                ok, agg = outs[w]
                same &= ok == [True] * a.clients and agg is not None and agg.tobytes() == total.tobytes()
        med = {w: float(np.median(v)) for w, v in times.items()}
        out = dict(sh, input_generation_s=round(gen_s, 2), ms=times, median_ms=med, spread_ms={w: round(max(v) - min(v), 3) for w, v in times.items()},
                   results_equal_and_correct=bool(same))
        if decodes:
            out["point_decodes"] = {w: sorted(set(v)) for w, v in counts.items()}
        if "b" in ways:
            out["b_split_ms"] = split
            out["b_split_median_ms"] = {k: float(np.median(v)) for k, v in split.items() if v}
        if "a" in med and "b" in med:
            out["b_over_a"] = round(med["b"] / med["a"], 4)
        res["shapes"][name] = out
        print("%s: %s, results equal and correct: %s" % (name, ", ".join("%s %.1f ms" % (w, med[w]) for w in ways), same), flush=True)
        if rnd is not None:
            rnd.close()
        acc.close()
        if not same:
            print(json.dumps(res)); sys.exit(1)
        del ups, _keep
    R.set_option("verify_batch", 1)
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
