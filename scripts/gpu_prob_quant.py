"""Probabilistic quantization on the GPU (rofl_quantize_prob / k_quantize_prob) at the sizes of a round, 1 x 25 000 and 48 x 55 000, on ONE
box in ONE run.  Four routes per shape:

  device_to_device  inputs and outputs are torch tensors on the GPU (the kernel reads and writes them in place)
  host_to_host      numpy arrays through the kernel (rofl_dbg_quantize_prob_route 1): staged upload, launch, staged download
  host_compiled     numpy arrays through the host copy of the rule (route 0), one core
  numpy_model       a NumPy restatement of the definition (hashlib SHAKE256 per block, vectorised rounding)

all four checked to give the same bytes.  Then the kernel's rate -- Keccak permutations per second of an in-place device call over 48 long
vectors, where launch and synchronisation are a few per cent -- against the rate of k_blind_combine in profiles/r08_blinding.json and against
the HBM bound of 8 bytes per element; the crossover of the host-compiled route and the kernel for host callers (what kQuantProbHostBelow in
csrc/rofl_zk.hip is set from); and EncParamsRange.encrypt_batch at 48 x 55 000 (8-bit, P = 4, fp 32/7) with and without quant seeds,
alternating: with seeds it may cost what it costs without them, plus the measured host-to-host time of the quantize call, plus 10 %.
(Without seeds encrypt_batch runs the parent commit's statements: the clip, then the same legs.)  Host clock around every call after one
warm-up; every call returns after its stream has been synchronised.

  python scripts/gpu_prob_quant.py [--reps 9] [--encrypt-reps 5] [--no-encrypt] [--out profiles/prob_quant.json]"""
import argparse
import ctypes
import hashlib
import json
import os
import struct
import sys
import time

import numpy as np
import torch

torch.cuda.init()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import rofl_project_code_amd as R  # noqa: E402

FP, NB, NPART = (32, 7), 8, 4
HBM_BYTES_PER_S = 8.0e12      # MI355X peak
sz = ctypes.c_size_t


def timed(f, reps):
    f()
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        f()
        ms.append(round((time.perf_counter() - t0) * 1e3, 4))
    return {"ms": ms, "median_ms": float(np.median(ms)), "max_minus_min_ms": round(max(ms) - min(ms), 4)}


def call(route, seeds, ins, outs, d, first=0):
    n = len(ins)
    addr = lambda x: x.data_ptr() if hasattr(x, "data_ptr") else x.ctypes.data
    arr = lambda xs: (ctypes.c_void_p * n)(*[addr(x) for x in xs])
    args = [sz(n), seeds, arr(ins), sz(first), sz(d), sz(NB), ctypes.c_uint(FP[0]), ctypes.c_uint(FP[1]), arr(outs)]
    rc = R.lib().rofl_quantize_prob(*args) if route is None else R.lib().rofl_dbg_quantize_prob_route(ctypes.c_uint(route), *args)
    assert rc == 0, rc


def numpy_model(seeds, xs):
    """the definition restated with NumPy: clip, floor, the threshold t = floor(r 2^32), one SHAKE256 call per 32 elements"""
    mx = np.float32(((1 << (NB - 1)) - 1) / float(1 << FP[1]))
    out = []
    for v, x in enumerate(xs):
        seed = seeds[32 * v:32 * v + 32]
        nblk = (x.size + 31) // 32
        w = np.frombuffer(b"".join(hashlib.shake_256(b"rofl-zk/quant/v1" + seed + struct.pack("<Q", b)).digest(128) for b in range(nblk)), "<u4")[:x.size]
        c = np.minimum(mx, np.maximum(-mx, np.where(np.isnan(x), -mx, x))).astype(np.float32)
        s = np.abs(c).astype(np.float64) * (1 << FP[1])
        f = np.floor(s)
        t = np.floor((s - f) * 4294967296.0)
        out.append(np.copysign(((f + (w < t)) / (1 << FP[1])).astype(np.float32), c))
    return out


def blind_combine_rate():
    """Keccak permutations per second of k_blind_combine with 48 vectors (profiles/r08_blinding.json, case d, device output)"""
    try:
        c = json.load(open(os.path.join(ROOT, "profiles", "r08_blinding.json")))["cases"]["d_pairwise_48_hosted_clients"]
        return c["keccak_permutations"] / (c["device_output"]["median_ms"] * 1e-3)
    except (OSError, KeyError):
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--encrypt-reps", type=int, default=5)
    ap.add_argument("--no-encrypt", action="store_true")
    ap.add_argument("--rate-d", type=int, default=1760000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "prob_quant.json"), help="'' = print only")
    a = ap.parse_args()
    R.set_device(0)
    res = {"fp": FP, "prove_range": NB, "reps": a.reps, "host_clock": "perf_counter around each call after one warm-up", "shapes": {}}
    for n, d in ((1, 25000), (48, 55000)):
        rng = np.random.default_rng(n * 1000 + 7)
        seeds = b"".join(bytes([i + 1]) * 32 for i in range(n))
        xs = [rng.uniform(-1.2, 1.2, d).astype(np.float32) for _ in range(n)]
        dx = [torch.from_numpy(x).cuda() for x in xs]
        dout = [torch.empty(d, dtype=torch.float32, device="cuda") for _ in range(n)]
        h1, h0 = [np.empty(d, np.float32) for _ in range(n)], [np.empty(d, np.float32) for _ in range(n)]
        c = {"device_to_device": timed(lambda: call(None, seeds, dx, dout, d), a.reps),
             "host_to_host": timed(lambda: call(1, seeds, xs, h1, d), a.reps),
             "host_compiled": timed(lambda: call(0, seeds, xs, h0, d), max(3, a.reps // 3)),
             "numpy_model": timed(lambda: numpy_model(seeds, xs), 2)}
        model = numpy_model(seeds, xs)
        same = all(o.cpu().numpy().tobytes() == p.tobytes() == q.tobytes() == m.tobytes() for o, p, q, m in zip(dout, h1, h0, model))
        assert same, "the four routes differ"
        c["bytes_equal"], c["elements"], c["keccak_permutations"] = True, n * d, n * ((d + 31) // 32)
        res["shapes"]["%dx%d" % (n, d)] = c
        print("%dx%d: %s" % (n, d, {k: v["median_ms"] for k, v in c.items() if isinstance(v, dict)}), flush=True)
    # the kernel's rate where the call is the kernel: 48 long vectors, in place on the device
    n, d = 48, a.rate_d
    seeds = b"".join(bytes([i + 1]) * 32 for i in range(n))
    big = [torch.rand(d, dtype=torch.float32, device="cuda") for _ in range(n)]
    t = timed(lambda: call(None, seeds, big, big, d), a.reps)
    perms, ref = n * ((d + 31) // 32), blind_combine_rate()
    rate = perms / (t["median_ms"] * 1e-3)
    res["kernel_rate"] = {"shape": "%dx%d in place, device" % (n, d), "call": t, "keccak_permutations": perms, "permutations_per_s": rate,
                          "k_blind_combine_permutations_per_s_r08": ref, "ratio_to_k_blind_combine": rate / ref if ref else None,
                          "bytes_per_s": 8.0 * n * d / (t["median_ms"] * 1e-3), "hbm_bound_ms_at_8_bytes_per_element": 8.0 * n * d / HBM_BYTES_PER_S * 1e3,
                          "share_of_hbm_bound": (8.0 * n * d / HBM_BYTES_PER_S * 1e3) / t["median_ms"]}
    del big
    print("kernel rate: %.3g permutations/s (k_blind_combine %.3g), %.3g B/s" % (rate, ref or 0, res["kernel_rate"]["bytes_per_s"]), flush=True)
    # crossover for host callers: the host copy against the kernel, one vector and eight
    sweep = []
    for n in (1, 8):
        for total in (256, 512, 1024, 2048, 4096, 8192, 16384, 32768, 65536):
            d = total // n
            seeds = b"".join(bytes([i + 1]) * 32 for i in range(n))
            xs = [np.random.default_rng(total + i).uniform(-1.2, 1.2, d).astype(np.float32) for i in range(n)]
            o = [np.empty(d, np.float32) for _ in range(n)]
            h = timed(lambda: call(0, seeds, xs, o, d), 15)["median_ms"]
            k = timed(lambda: call(1, seeds, xs, o, d), 15)["median_ms"]
            sweep.append({"n_vec": n, "elements": n * d, "host_compiled_ms": h, "kernel_host_to_host_ms": k})
    res["crossover_sweep"] = sweep
    res["crossover_elements"] = {str(n): next((s["elements"] for s in sweep if s["n_vec"] == n and s["kernel_host_to_host_ms"] < s["host_compiled_ms"]), None) for n in (1, 8)}
    print("crossover: %s" % res["crossover_elements"], flush=True)
    if not a.no_encrypt:
        n, d = 48, 55000
        cl = []
        for i in range(n):
            rng = np.random.default_rng(9300 + i)
            x = (rng.integers(-12, 13, size=d) / 512.0).astype(np.float32)      # quarter steps
            bl = rng.integers(0, 256, size=(d, 32), dtype=np.uint8); bl[:, 31] &= 0x0F
            cl.append((x, bl))
        ns, qs = [bytes([i % 251 + 1]) * 32 for i in range(n)], [bytes([i + 101]) * 32 for i in range(n)]
        plain = lambda: R.EncParamsRange.encrypt_batch(cl, NB, NPART, 1.0, nonce_seeds=ns, fp=FP)
        seeded = lambda: R.EncParamsRange.encrypt_batch_quantized(cl, NB, NPART, 1.0, qs, nonce_seeds=ns, fp=FP)
        plain(); seeded()
        t = {"without_seeds": [], "with_quant_seeds": []}
        for _ in range(a.encrypt_reps):
            for w, f in (("without_seeds", plain), ("with_quant_seeds", seeded)):
                t0 = time.perf_counter(); f(); t[w].append(round((time.perf_counter() - t0) * 1e3, 3))
        med = {w: float(np.median(v)) for w, v in t.items()}
        q_ms = res["shapes"]["48x55000"]["host_to_host"]["median_ms"]
        res["encrypt_batch_range_48x55000"] = {"ms": t, "median_ms": med, "quantize_host_to_host_ms": q_ms,
                                               "allowed_ms": 1.10 * (med["without_seeds"] + q_ms),
                                               "within_plain_plus_quantize_plus_10_percent": bool(med["with_quant_seeds"] <= 1.10 * (med["without_seeds"] + q_ms))}
        print("encrypt_batch: %s" % res["encrypt_batch_range_48x55000"], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
