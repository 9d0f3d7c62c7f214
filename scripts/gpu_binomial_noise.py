"""Distributed noise on the GPU (rofl_noise_binomial / k_noise_binomial) on ONE box in ONE run.

  rates      Keccak permutations per second of an in-place device call over 48 vectors at W = k / 16 in {1, 32, 512}: at 48 x 55 000 (the
             size of a round; at W = 1 that is 82 500 permutations, a call that is mostly launch and synchronisation), and at W = 1 also
             over 48 x 1 760 000, which has the permutations of W = 32 at 48 x 55 000.  The yardstick is k_quantize_prob in the same
             process over 48 x 1 760 000 in place -- one permutation per lane like this kernel, the same number of permutations as the
             W = 1 long and the W = 32 calls, so launch and synchronisation weigh the same in both.  A ratio well below 1 would mean that
             the segmented sum or the memory pattern costs what it should not.
  crossover  the host-compiled route (rofl_dbg_noise_binomial_route 0, one core) against the kernel for host callers (route 1: staged
             upload, launch, staged download), swept over the permutations of the call at W = 1 and W = 32: what kNoiseHostBelowPerms in
             csrc/rofl_zk.hip is set from.
  encrypt    EncParamsRange.encrypt_batch_private at 48 x 55 000 (8-bit range, P = 4, fp 32/7) with noise seeds at sigma = 64 steps
             (k = 8192) against encrypt_batch_quantized without, alternating.  (At an 8-bit range that noise saturates; the time does
             not depend on it.)

The device route is checked against the host route, byte for byte, at 3 x 5 000 for every W measured.  Host clock around every call after
one warm-up; every call returns after its stream has been synchronised.

  python scripts/gpu_binomial_noise.py [--reps 9] [--encrypt-reps 5] [--no-encrypt] [--out profiles/binomial_noise.json]"""
import argparse
import ctypes
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

FP, NB, NPART = (32, 7), 8, 4
sz = ctypes.c_size_t


def timed(f, reps):
    f()
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        f()
        ms.append(round((time.perf_counter() - t0) * 1e3, 4))
    return {"ms": ms, "median_ms": float(np.median(ms)), "max_minus_min_ms": round(max(ms) - min(ms), 4)}


def _arrs(xs):
    return (ctypes.c_void_p * len(xs))(*[x.data_ptr() if hasattr(x, "data_ptr") else x.ctypes.data for x in xs])


def noise(route, seeds, ins, outs, d, W, first=0, nb=32):
    args = [sz(len(ins)), seeds, _arrs(ins), sz(first), sz(d), ctypes.c_uint32(16 * W), sz(nb), ctypes.c_uint(FP[0]), ctypes.c_uint(FP[1]), _arrs(outs)]
    rc = R.lib().rofl_noise_binomial(*args) if route is None else R.lib().rofl_dbg_noise_binomial_route(ctypes.c_uint(route), *args)
    assert rc == 0, rc


def quant(seeds, ins, outs, d):
    rc = R.lib().rofl_quantize_prob(sz(len(ins)), seeds, _arrs(ins), sz(0), sz(d), sz(32), ctypes.c_uint(FP[0]), ctypes.c_uint(FP[1]), _arrs(outs))
    assert rc == 0, rc


def perms_of(n, d, W):
    return n * ((d * W + 31) // 32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--encrypt-reps", type=int, default=5)
    ap.add_argument("--no-encrypt", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "binomial_noise.json"), help="'' = print only")
    a = ap.parse_args()
    R.set_device(0)
    res = {"fp": FP, "reps": a.reps, "host_clock": "perf_counter around each call after one warm-up"}
    n = 48
    seeds = b"".join(bytes([i + 1]) * 32 for i in range(n))
    # the two routes give the same bytes
    for W in (1, 32, 512):
        xs = [np.random.default_rng(W + i).uniform(-1.2, 1.2, 5000).astype(np.float32) for i in range(3)]
        h, k = [np.empty(5000, np.float32) for _ in xs], [np.empty(5000, np.float32) for _ in xs]
        noise(0, seeds[:96], xs, h, 5000, W, first=11)
        noise(1, seeds[:96], xs, k, 5000, W, first=11)
        assert all(p.tobytes() == q.tobytes() for p, q in zip(h, k)), "the routes differ at W = %d" % W
    res["routes_bytes_equal"] = True
    # the yardstick: k_quantize_prob, one permutation per 32 elements
    d_long = 1760000
    big = [torch.rand(d_long, dtype=torch.float32, device="cuda") for _ in range(n)]
    t = timed(lambda: quant(seeds, big, big, d_long), a.reps)
    q_perms = n * ((d_long + 31) // 32)
    q_rate = q_perms / (t["median_ms"] * 1e-3)
    res["yardstick_k_quantize_prob"] = {"shape": "%dx%d in place, device" % (n, d_long), "call": t, "keccak_permutations": q_perms, "permutations_per_s": q_rate}
    print("k_quantize_prob: %.3g permutations/s" % q_rate, flush=True)
    rates = []
    for W, d in ((1, d_long), (1, 55000), (32, 55000), (512, 55000)):
        xs = big if d == d_long else [torch.rand(d, dtype=torch.float32, device="cuda") for _ in range(n)]
        t = timed(lambda: noise(None, seeds, xs, xs, d, W), a.reps)
        p = perms_of(n, d, W)
        rate = p / (t["median_ms"] * 1e-3)
        rates.append({"W": W, "k": 16 * W, "shape": "%dx%d in place, device" % (n, d), "call": t, "keccak_permutations": p, "permutations_per_s": rate,
                      "ratio_to_k_quantize_prob": rate / q_rate})
        print("k_noise_binomial W=%d d=%d: %.3f ms, %.3g permutations/s, ratio %.3f" % (W, d, t["median_ms"], rate, rate / q_rate), flush=True)
    del big
    res["rates"] = rates
    # host callers at the size of a round: staged upload, launch, staged download
    d = 55000
    xs = [np.random.default_rng(i).uniform(-1.2, 1.2, d).astype(np.float32) for i in range(n)]
    ho = [np.empty(d, np.float32) for _ in range(n)]
    res["host_to_host_48x55000"] = {"W%d" % W: timed(lambda: noise(1, seeds, xs, ho, d, W), a.reps) for W in (1, 32, 512)}
    print("host to host 48x55000: %s" % {k: v["median_ms"] for k, v in res["host_to_host_48x55000"].items()}, flush=True)
    # crossover for host callers, in permutations
    sweep = []
    for W in (1, 32):
        for perms in (16, 32, 64, 128, 256, 512, 1024, 2048, 4096):
            d = perms * 32 // W
            x = [np.random.default_rng(perms).uniform(-1.2, 1.2, d).astype(np.float32)]
            o = [np.empty(d, np.float32)]
            h = timed(lambda: noise(0, seeds[:32], x, o, d, W), 15)["median_ms"]
            k = timed(lambda: noise(1, seeds[:32], x, o, d, W), 15)["median_ms"]
            sweep.append({"W": W, "d": d, "keccak_permutations": perms, "host_compiled_ms": h, "kernel_host_to_host_ms": k})
    res["crossover_sweep"] = sweep
    res["crossover_permutations"] = {"W%d" % W: next((s["keccak_permutations"] for s in sweep if s["W"] == W and s["kernel_host_to_host_ms"] < s["host_compiled_ms"]), None) for W in (1, 32)}
    print("crossover: %s" % res["crossover_permutations"], flush=True)
    if not a.no_encrypt:
        d, k = 55000, R.range_proof_vec.binomial_noise_k(64)
        cl = []
        for i in range(n):
            rng = np.random.default_rng(9300 + i)
            x = (rng.integers(-12, 13, size=d) / 512.0).astype(np.float32)      # quarter steps
            bl = rng.integers(0, 256, size=(d, 32), dtype=np.uint8); bl[:, 31] &= 0x0F
            cl.append((x, bl))
        ns, qs, zs = ([bytes([i % 251 + 1]) * 32 for i in range(n)], [bytes([i + 101]) * 32 for i in range(n)], [bytes([i + 151]) * 32 for i in range(n)])
        plain = lambda: R.EncParamsRange.encrypt_batch_quantized(cl, NB, NPART, 1.0, qs, nonce_seeds=ns, fp=FP)
        noisy = lambda: R.EncParamsRange.encrypt_batch_private(cl, NB, NPART, 1.0, nonce_seeds=ns, fp=FP, quant_seeds=qs, noise_seeds=zs, noise_k=k)
        plain(); noisy()
        t = {"encrypt_batch_quantized": [], "encrypt_batch_private_with_noise": []}
        for _ in range(a.encrypt_reps):
            for w, f in (("encrypt_batch_quantized", plain), ("encrypt_batch_private_with_noise", noisy)):
                t0 = time.perf_counter(); f(); t[w].append(round((time.perf_counter() - t0) * 1e3, 3))
        res["encrypt_batch_range_48x55000"] = {"noise_k": k, "ms": t, "median_ms": {w: float(np.median(v)) for w, v in t.items()}}
        print("encrypt_batch: %s" % res["encrypt_batch_range_48x55000"]["median_ms"], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
