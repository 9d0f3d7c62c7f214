"""Aggregation of one server round (params.rs:74-147, server.rs:696-714) at the shape of BASELINE cfg 4 / 5: 48 clients, d = 55 000.

In ONE process, after a warm-up, five alternations of
  (a) EncModelParamsAccumulator: one rofl_add_points_vec per client (host accumulator up / down every time) + extract
  (b) DeviceAccumulator: one accumulate_other per client + extract
  (c) DeviceAccumulator: one accumulate_batch + extract
each timed with a host clock around work that ends in a device synchronisation (extract returns host data).  The exports and the f32
aggregates of a, b and c are compared byte for byte.  cfg 4: 64-byte ElGamal pairs (EncParamsRange); cfg 5: 96-byte
SquareRandProofCommitments read in place from serialised EncParamsL2 messages (deserialize(copy=False)).
Updates are (m B + r B~, r B) pairs from commit_vec with cancelling blindings (no proofs: aggregation does not read them).

  python scripts/gpu_aggregate_round.py [--clients 48] [--d 55000] [--reps 5] [--cfg 4,5] [--out file.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import rofl_project_code_amd as R  # noqa: E402

FP = (32, 7)


def make_round(n, d, seed):
    rng = np.random.default_rng(seed)
    xs = [(rng.integers(-300, 300, size=d) / 128.0).astype(np.float32) for _ in range(n)]
    bls = []
    for _ in range(n - 1):
        b = rng.integers(0, 256, size=(d, 32), dtype=np.uint8); b[:, 31] &= 0x0F
        bls.append(b)
    bls.append(R.pedersen_ops.add_scalar_vec(np.zeros((d, 32), np.uint8), R.pedersen_ops.add_scalar_vec_vec(bls), subtract=True))
    pairs = []
    for x, b in zip(xs, bls):
        m = R.conversion32.f32_to_scalar_vec(x, fp=FP)
        pairs.append(np.ascontiguousarray(np.concatenate([R.pedersen_ops.commit_vec(m, b), R.pedersen_ops.commit_no_blinding_vec(b)], axis=1)))
    return xs, pairs


def messages(cfg, pairs):
    if cfg == 4:
        return [R.EncParamsRange(p, np.zeros((p.shape[0], 128), np.uint8), np.zeros((1, 608), np.uint8), 32, 1.0) for p in pairs], []
    bufs, out = [], []
    for p in pairs:
        ev = np.ascontiguousarray(np.concatenate([p, p[:, :32]], axis=1))      # c, then a stand-in c_sq (aggregation does not read it)
        buf = R.EncParamsL2(ev, np.zeros((p.shape[0], 192), np.uint8), np.zeros((1, 672), np.uint8), np.zeros(608, np.uint8), 32, 32).serialize(as_array=True)
        m = R.EncParamsL2.deserialize(buf, copy=False)
        assert np.shares_memory(m.enc_values, buf)
        bufs.append(buf); out.append(m)
    return out, bufs


def run_a(d, msgs):
    t0 = time.perf_counter()
    acc = R.EncModelParamsAccumulator.unity(d)
    for m in msgs:
        acc.accumulate_other(m)
    t1 = time.perf_counter()
    out = acc.extract()
    t2 = time.perf_counter()
    return (t2 - t0) * 1e3, (t1 - t0) * 1e3, acc.acc.copy(), out


def run_b(d, msgs, batch):
    t0 = time.perf_counter()
    acc = R.DeviceAccumulator.unity(d)
    if batch:
        acc.accumulate_batch(msgs)
    else:
        for m in msgs:
            acc.accumulate_other(m)
    t1 = time.perf_counter()
    out = acc.extract()
    t2 = time.perf_counter()
    ex = acc.export()
    acc.close()
    return (t2 - t0) * 1e3, (t1 - t0) * 1e3, ex, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clients", type=int, default=48)
    ap.add_argument("--d", type=int, default=55000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cfg", default="4,5")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    R.set_device(0)
    R.api.set_fp(*FP)
    t = time.perf_counter()
    xs, pairs = make_round(a.clients, a.d, 2024)
    gen_s = time.perf_counter() - t
    want = np.sum(np.stack(xs).astype(np.float64), axis=0).astype(np.float32)
    res = {"clients": a.clients, "d": a.d, "reps": a.reps, "fp": list(FP), "input_generation_s": round(gen_s, 2),
           "decodes_per_round_device": 2 * a.clients * a.d, "point_ops_per_round_host_path": 6 * a.clients * a.d, "cfgs": {}}
    for cfg in [int(c) for c in a.cfg.split(",")]:
        msgs, _keep = messages(cfg, pairs)
        runs = {"a": lambda: run_a(a.d, msgs), "b": lambda: run_b(a.d, msgs, False), "c": lambda: run_b(a.d, msgs, True)}
        for k in "abc":      # warm-up: tables, lane workspaces, staging
            runs[k]()
        times = {k: [] for k in "abc"}
        add_times = {k: [] for k in "abc"}
        same = True
        for _ in range(a.reps):
            outs = {}
            for k in "abc":
                tot, add, ex, out = runs[k]()
                times[k].append(round(tot, 3)); add_times[k].append(round(add, 3))
                outs[k] = (ex, out)
            same &= bool((outs["a"][0] == outs["b"][0]).all() and (outs["a"][0] == outs["c"][0]).all())
            same &= outs["a"][1] is not None and outs["a"][1].tobytes() == outs["b"][1].tobytes() == outs["c"][1].tobytes() == want.tobytes()
        med = {k: float(np.median(v)) for k, v in times.items()}
        res["cfgs"][str(cfg)] = {
            "record_bytes": 64 if cfg == 4 else 96,
            "ms": times, "accumulate_ms": add_times, "median_ms": med,
            "median_accumulate_ms": {k: float(np.median(v)) for k, v in add_times.items()},
            "c_over_a": round(med["c"] / med["a"], 4), "b_over_a": round(med["b"] / med["a"], 4),
            "outputs_equal": same}
        print("cfg %d: median a %.1f ms, b %.1f ms, c %.1f ms (c/a %.3f), outputs equal: %s" % (cfg, med["a"], med["b"], med["c"], med["c"] / med["a"], same), flush=True)
        if not same:
            print(json.dumps(res)); sys.exit(1)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
