"""Discrete Gaussian noise on the GPU (rofl_noise_dgauss / k_noise_dgauss) on ONE box in ONE run.

  rates      an in-place device call over 48 vectors at sigma2 in {1, 4096, 2^24}, at 48 x 55 000 (the size of a round) and at
             48 x 1 760 000: time, Keccak permutations and permutations per second.  The permutations are the model's count
             (tests/dgauss_model.py: the blocks each element needs, the mean over the first 20 000 elements of seed 00 01 .. 1f times the
             elements of the call; the kernel squeezes exactly the blocks an element needs).  The yardstick is k_quantize_prob in the same
             process over 48 x 1 760 000 in place, one permutation per lane like this kernel.
  binomial   the call at sigma2 = 4096 against rofl_noise_binomial at k = 8 192 (sigma = 64 steps as well), 48 x 55 000 in place on the
             device, alternating in this process.
  divergence from the model, for one vector of 55 000 elements of a call of 48 at each sigma2 on the grid the library launches: the blocks
             a lane squeezes (the sum over its elements), their mean, and the mean over the waves of the largest of a wave's 64 lanes
             -- a wave runs as long as its slowest lane, so mean / that is the share of the lanes' trips that do work; the same
             share at 1 760 000 elements a vector, by resampling those blocks; and the attempts (passes of the rejection loop) and
             words per element.
  crossover  the host-compiled route (rofl_dbg_noise_dgauss_route 0, one core) against the kernel for host callers (route 1: staged
             upload, launch, staged download), swept over the elements of the call at sigma2 = 1 and 4096: what kDgaussHostBelow in
             csrc/prepare_calls.hpp is set from.
  encrypt    EncParamsRange.encrypt_batch_private at 48 x 55 000 (8-bit range, P = 4, fp 32/7) with noise_k = DiscreteGaussian(4096)
             against encrypt_batch_quantized without, alternating.  (At an 8-bit range that noise saturates; the time does not depend
             on it.)

The device route is checked against the host route, byte for byte, at 3 x 5 000 for every sigma2 measured, before any clock starts.  Host
clock around every call after one warm-up; every call returns after its stream has been synchronised.

  python scripts/gpu_dgauss_noise.py [--reps 9] [--encrypt-reps 5] [--no-encrypt] [--out profiles/dgauss_noise.json]"""
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
import rofl_project_code_amd as R  # noqa: E402
import dgauss_model as M  # noqa: E402

FP, NB, NPART = (32, 7), 8, 4
SIGMA2S = (1, 4096, 1 << 24)
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


def dgauss(route, seeds, ins, outs, d, s2, first=0, nb=32):
    args = [sz(len(ins)), seeds, _arrs(ins), sz(first), sz(d), ctypes.c_uint32(s2), sz(nb), ctypes.c_uint(FP[0]), ctypes.c_uint(FP[1]), _arrs(outs)]
    rc = R.lib().rofl_noise_dgauss(*args) if route is None else R.lib().rofl_dbg_noise_dgauss_route(ctypes.c_uint(route), *args)
    assert rc == 0, rc


def binomial(seeds, ins, outs, d, k):
    rc = R.lib().rofl_noise_binomial(sz(len(ins)), seeds, _arrs(ins), sz(0), sz(d), ctypes.c_uint32(k), sz(32), ctypes.c_uint(FP[0]), ctypes.c_uint(FP[1]), _arrs(outs))
    assert rc == 0, rc


def quant(seeds, ins, outs, d):
    rc = R.lib().rofl_quantize_prob(sz(len(ins)), seeds, _arrs(ins), sz(0), sz(d), sz(32), ctypes.c_uint(FP[0]), ctypes.c_uint(FP[1]), _arrs(outs))
    assert rc == 0, rc


def divergence(d, n_vec, s2):
    """the model's blocks per lane and per wave on the grid of a call of n_vec vectors of d elements (as dgauss_grid in prepare_calls.hpp)"""
    blocks = M.blocks_used(bytes(range(32)), 0, d, s2)
    gx = max(1, min((d + 127) // 128, 2048 // min(n_vec, 2048)))
    lanes = gx * 64
    per_lane = np.zeros(lanes, np.int64)
    np.add.at(per_lane, np.arange(d) % lanes, blocks)
    per_wave_max = per_lane.reshape(gx, 64).max(axis=1)
    # the same at 1 760 000 elements a vector, which the model is too slow for: a lane's elements drawn from the blocks of these d elements
    long_lane = -(-1760000 // lanes)
    res_lane = np.random.default_rng(s2).choice(blocks, size=(gx * 64, long_lane)).sum(axis=1)
    res_share = float(res_lane.mean() / res_lane.reshape(gx, 64).max(axis=1).mean())
    return {"d": d, "n_vec": n_vec, "sigma2": s2, "workgroups_per_vector": gx, "resampled_at_1760000": {"elements_per_lane": long_lane, "share_of_lane_trips_that_work": res_share}, "elements_per_lane": -(-d // lanes), "blocks_per_element_mean": float(blocks.mean()),
            "blocks_per_element_max": int(blocks.max()), "blocks_per_lane_mean": float(per_lane.mean()), "blocks_of_a_waves_slowest_lane_mean": float(per_wave_max.mean()),
            "blocks_of_a_waves_slowest_lane_max": int(per_wave_max.max()), "share_of_lane_trips_that_work": float(per_lane.mean() / per_wave_max.mean())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--encrypt-reps", type=int, default=5)
    ap.add_argument("--no-encrypt", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dgauss_noise.json"), help="'' = print only")
    a = ap.parse_args()
    R.set_device(0)
    res = {"fp": FP, "reps": a.reps, "host_clock": "perf_counter around each call after one warm-up"}
    n = 48
    seeds = b"".join(bytes([i + 1]) * 32 for i in range(n))
    # the two routes give the same bytes
    for s2 in SIGMA2S:
        xs = [np.random.default_rng(s2 % 1000 + i).uniform(-1.2, 1.2, 5000).astype(np.float32) for i in range(3)]
        h, k = [np.empty(5000, np.float32) for _ in xs], [np.empty(5000, np.float32) for _ in xs]
        dgauss(0, seeds[:96], xs, h, 5000, s2, first=11)
        dgauss(1, seeds[:96], xs, k, 5000, s2, first=11)
        assert all(p.tobytes() == q.tobytes() for p, q in zip(h, k)), "the routes differ at sigma2 = %d" % s2
    res["routes_bytes_equal"] = True
    mean_blocks = {s2: float(M.blocks_used(bytes(range(32)), 0, 20000, s2).mean()) for s2 in SIGMA2S}
    res["model_blocks_per_element_mean_of_20000"] = {str(s2): v for s2, v in mean_blocks.items()}
    aw = {s2: M.attempts_and_words(bytes(range(32)), 0, 20000, s2) for s2 in SIGMA2S}
    res["model_attempts_per_element_mean_of_20000"] = {str(s2): float(v[0].mean()) for s2, v in aw.items()}
    res["model_words_per_element_mean_of_20000"] = {str(s2): float(v[1].mean()) for s2, v in aw.items()}
    # the yardstick: k_quantize_prob, one permutation per 32 elements
    d_long = 1760000
    big = [torch.rand(d_long, dtype=torch.float32, device="cuda") for _ in range(n)]
    t = timed(lambda: quant(seeds, big, big, d_long), a.reps)
    q_perms = n * ((d_long + 31) // 32)
    q_rate = q_perms / (t["median_ms"] * 1e-3)
    res["yardstick_k_quantize_prob"] = {"shape": "%dx%d in place, device" % (n, d_long), "call": t, "keccak_permutations": q_perms, "permutations_per_s": q_rate}
    print("k_quantize_prob: %.3g permutations/s" % q_rate, flush=True)
    small = [torch.rand(55000, dtype=torch.float32, device="cuda") for _ in range(n)]
    rates = []
    for d in (55000, d_long):
        xs = big if d == d_long else small
        for s2 in SIGMA2S:
            t = timed(lambda: dgauss(None, seeds, xs, xs, d, s2), a.reps)
            p = n * d * mean_blocks[s2]
            rate = p / (t["median_ms"] * 1e-3)
            rates.append({"sigma2": s2, "shape": "%dx%d in place, device" % (n, d), "call": t, "keccak_permutations_model": p, "permutations_per_s": rate,
                          "elements_per_s": n * d / (t["median_ms"] * 1e-3), "ratio_to_k_quantize_prob": rate / q_rate})
            print("k_noise_dgauss sigma2=%d d=%d: %.3f ms, %.3g permutations/s, ratio %.3f" % (s2, d, t["median_ms"], rate, rate / q_rate), flush=True)
    del big
    res["rates"] = rates
    # against the binomial noise of the same sigma, alternating
    tb, tg = [], []
    binomial(seeds, small, small, 55000, 8192); dgauss(None, seeds, small, small, 55000, 4096)
    for _ in range(a.reps):
        t0 = time.perf_counter(); binomial(seeds, small, small, 55000, 8192); tb.append(round((time.perf_counter() - t0) * 1e3, 4))
        t0 = time.perf_counter(); dgauss(None, seeds, small, small, 55000, 4096); tg.append(round((time.perf_counter() - t0) * 1e3, 4))
    res["against_binomial_48x55000_sigma_64"] = {"rofl_noise_binomial_k8192_ms": tb, "rofl_noise_dgauss_sigma2_4096_ms": tg, "median_ms": [float(np.median(tb)), float(np.median(tg))],
                                                 "binomial_over_dgauss": float(np.median(tb) / np.median(tg))}
    print("binomial k=8192 %.3f ms, dgauss 4096 %.3f ms" % (np.median(tb), np.median(tg)), flush=True)
    del small
    res["divergence_model"] = {str(s2): divergence(55000, n, s2) for s2 in SIGMA2S}
    print("divergence: %s" % res["divergence_model"], flush=True)
    # host callers at the size of a round: staged upload, launch, staged download
    d = 55000
    xs = [np.random.default_rng(i).uniform(-1.2, 1.2, d).astype(np.float32) for i in range(n)]
    ho = [np.empty(d, np.float32) for _ in range(n)]
    res["host_to_host_48x55000"] = {"sigma2_%d" % s2: timed(lambda: dgauss(1, seeds, xs, ho, d, s2), a.reps) for s2 in SIGMA2S}
    print("host to host 48x55000: %s" % {k: v["median_ms"] for k, v in res["host_to_host_48x55000"].items()}, flush=True)
    # crossover for host callers, in elements
    sweep = []
    for s2 in (1, 4096):
        for d in (16, 32, 64, 128, 256, 384, 512, 576, 640, 704, 768, 832, 896, 960, 1024, 2048, 4096):
            x = [np.random.default_rng(d).uniform(-1.2, 1.2, d).astype(np.float32)]
            o = [np.empty(d, np.float32)]
            h = timed(lambda: dgauss(0, seeds[:32], x, o, d, s2), 15)["median_ms"]
            k = timed(lambda: dgauss(1, seeds[:32], x, o, d, s2), 15)["median_ms"]
            sweep.append({"sigma2": s2, "elements": d, "host_compiled_ms": h, "kernel_host_to_host_ms": k})
    res["crossover_sweep"] = sweep
    res["crossover_elements"] = {"sigma2_%d" % s2: next((s["elements"] for s in sweep if s["sigma2"] == s2 and s["kernel_host_to_host_ms"] < s["host_compiled_ms"]), None) for s2 in (1, 4096)}
    print("crossover: %s" % res["crossover_elements"], flush=True)
    if not a.no_encrypt:
        d, g = 55000, R.DiscreteGaussian(4096)
        cl = []
        for i in range(n):
            rng = np.random.default_rng(9300 + i)
            x = (rng.integers(-12, 13, size=d) / 512.0).astype(np.float32)      # quarter steps
            bl = rng.integers(0, 256, size=(d, 32), dtype=np.uint8); bl[:, 31] &= 0x0F
            cl.append((x, bl))
        ns, qs, zs = ([bytes([i % 251 + 1]) * 32 for i in range(n)], [bytes([i + 101]) * 32 for i in range(n)], [bytes([i + 151]) * 32 for i in range(n)])
        plain = lambda: R.EncParamsRange.encrypt_batch_quantized(cl, NB, NPART, 1.0, qs, nonce_seeds=ns, fp=FP)
        noisy = lambda: R.EncParamsRange.encrypt_batch_private(cl, NB, NPART, 1.0, nonce_seeds=ns, fp=FP, quant_seeds=qs, noise_seeds=zs, noise_k=g)
        plain(); noisy()
        t = {"encrypt_batch_quantized": [], "encrypt_batch_private_with_dgauss_noise": []}
        for _ in range(a.encrypt_reps):
            for w, f in (("encrypt_batch_quantized", plain), ("encrypt_batch_private_with_dgauss_noise", noisy)):
                t0 = time.perf_counter(); f(); t[w].append(round((time.perf_counter() - t0) * 1e3, 3))
        med = {w: float(np.median(v)) for w, v in t.items()}
        bound = 1.10 * (med["encrypt_batch_quantized"] + res["host_to_host_48x55000"]["sigma2_4096"]["median_ms"])
        res["encrypt_batch_range_48x55000"] = {"noise_k": repr(g), "ms": t, "median_ms": med, "bound_1.10x_quantized_plus_host_caller_ms": bound,
                                               "within_bound": med["encrypt_batch_private_with_dgauss_noise"] <= bound}
        print("encrypt_batch: %s bound %.1f" % (med, bound), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
