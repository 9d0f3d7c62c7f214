"""Norm clipping on the GPU (rofl_clip_l2: k_clip_l2_sumsq + k_clip_l2_apply / _seeded) on ONE box in ONE run.

  call       clip_l2_vecs at 48 x 55 000, fp 32/7, in the four combinations device-resident in place / host to host x seeded / unseeded,
             every vector scaled (max_sq = half its sum of squares: the seeded form then permutes every block), and the device-resident
             forms again with every vector fitting (no permutation, no search).  Launches per call: two kernels (one reduction, one
             scaling), one copy of the descriptors, the copy of the scales, and for a seeded call the wipe of the descriptors.
             Bytes of the unseeded form: each value is read twice and written once, 12 bytes per element, against the 8.0 TB/s of the
             HBM's data sheet.  Keccak rate of the seeded form: one permutation per 32 elements, against rofl_quantize_prob
             (k_quantize_prob) at the same shape in the same process.  At 10 MB of data both are at the launch floor; the same ratio at
             48 x 1 760 000 shows what the kernels sustain.
  baseline   a single-core NumPy float64 clip of the same 48 x 55 000 values (norm, scale, round to the grid).
  crossover  the host-compiled route (rofl_dbg_clip_l2_route 0, one core) against the kernels for host callers (route 1: staged upload,
             two launches, staged download), swept over n_vec d, seeded and unseeded: what kClipL2HostBelow in csrc/rofl_zk.hip is set
             from.
  encrypt    EncParamsL2.encrypt_batch_clipped at 48 x 55 000 (8-bit range, P = 4, l2_range 32, fp 32/7) with l2_clip (every update
             scaled, seeded) and without it, against encrypt_batch_private, alternating.

The device route is checked against the host route, byte for byte, at 3 x 5 000.  Host clock around every call after one warm-up; every
call returns after its stream has been synchronised.

  python scripts/gpu_l2_clip.py [--reps 9] [--encrypt-reps 3] [--no-encrypt] [--out profiles/l2_clip.json]"""
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

FP, NB, NPART, L2N = (32, 7), 8, 4, 32
HBM_PEAK = 8.0e12
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


def clip(route, seeds, ins, outs, d, T, scale=None):
    ts = (ctypes.c_uint64 * len(T))(*T)
    args = [sz(len(ins)), seeds, _arrs(ins), sz(d), ts, sz(NB), ctypes.c_uint(FP[0]), ctypes.c_uint(FP[1]), _arrs(outs), scale]
    rc = R.lib().rofl_clip_l2(*args) if route is None else R.lib().rofl_dbg_clip_l2_route(ctypes.c_uint(route), *args)
    assert rc == 0, rc


def quant(seeds, ins, outs, d):
    rc = R.lib().rofl_quantize_prob(sz(len(ins)), seeds, _arrs(ins), sz(0), sz(d), sz(NB), ctypes.c_uint(FP[0]), ctypes.c_uint(FP[1]), _arrs(outs))
    assert rc == 0, rc


def values(i, d):
    """values of up to 100 grid steps, on the grid (inside the clip range of an 8-bit proof)"""
    return (np.random.default_rng(i).integers(-100, 101, d) / 128.0).astype(np.float32)


def sum_sq(x):
    return int((np.round(x.astype(np.float64) * 128) ** 2).sum())


def numpy_clip(xs, T):
    out = []
    for x, t in zip(xs, T):
        q = np.rint(x.astype(np.float64) * 128)
        n2 = float((q * q).sum())
        out.append((np.trunc(q * min(1.0, np.sqrt(t / n2))) / 128).astype(np.float32))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--encrypt-reps", type=int, default=3)
    ap.add_argument("--no-encrypt", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "l2_clip.json"), help="'' = print only")
    a = ap.parse_args()
    R.set_device(0)
    res = {"fp": FP, "prove_range": NB, "reps": a.reps, "host_clock": "perf_counter around each call after one warm-up",
           "launches_per_call": {"kernels": 2, "copies": "descriptors up, scales down (+ one staged copy per host vector each way)", "seeded_extra": "one memset of the descriptors"}}
    n, d = 48, 55000
    seeds = b"".join(bytes([i + 1]) * 32 for i in range(n))
    # the two routes give the same bytes
    xs = [values(i, 5000) for i in range(3)]
    T3 = [sum_sq(xs[0]), sum_sq(xs[1]) // 2, 71 ** 2]
    for sd in (None, seeds[:96]):
        h, k = [np.empty(5000, np.float32) for _ in xs], [np.empty(5000, np.float32) for _ in xs]
        sh, sk = (ctypes.c_uint64 * 3)(), (ctypes.c_uint64 * 3)()
        clip(0, sd, xs, h, 5000, T3, sh)
        clip(1, sd, xs, k, 5000, T3, sk)
        assert all(p.tobytes() == q.tobytes() for p, q in zip(h, k)) and list(sh) == list(sk), "the routes differ"
    res["routes_bytes_equal"] = True
    hx = [values(100 + i, d) for i in range(n)]
    S = [sum_sq(x) for x in hx]
    half, fits = [s // 2 for s in S], S
    # the yardstick: k_quantize_prob at the same shape, device-resident in place
    dev = [torch.from_numpy(x).cuda() for x in hx]
    t = timed(lambda: quant(seeds, dev, dev, d), a.reps)
    q_perms = n * ((d + 31) // 32)
    res["yardstick_k_quantize_prob_48x55000"] = {"call": t, "keccak_permutations": q_perms, "permutations_per_s": q_perms / (t["median_ms"] * 1e-3)}
    print("k_quantize_prob 48x55000: %.3f ms" % t["median_ms"], flush=True)
    calls = {}
    for name, sd, T in (("device_unseeded_scaled", None, half), ("device_seeded_scaled", seeds, half), ("device_unseeded_fits", None, fits), ("device_seeded_fits", seeds, fits)):
        src = [torch.from_numpy(x).cuda() for x in hx]
        out = [torch.empty(d, dtype=torch.float32, device="cuda") for _ in range(n)]
        t = timed(lambda: clip(None, sd, src, out, d, T), a.reps)
        e = {"call": t, "bytes": 12 * n * d, "bytes_per_s": 12 * n * d / (t["median_ms"] * 1e-3)}
        e["fraction_of_hbm_peak"] = e["bytes_per_s"] / HBM_PEAK
        if sd is not None and T is half:
            e["keccak_permutations"] = q_perms
            e["permutations_per_s"] = q_perms / (t["median_ms"] * 1e-3)
            e["ratio_to_k_quantize_prob"] = e["permutations_per_s"] / res["yardstick_k_quantize_prob_48x55000"]["permutations_per_s"]
        calls[name] = e
        print("%s: %.3f ms" % (name, t["median_ms"]), flush=True)
    ho = [np.empty(d, np.float32) for _ in range(n)]
    for name, sd in (("host_to_host_unseeded_scaled", None), ("host_to_host_seeded_scaled", seeds)):
        calls[name] = {"call": timed(lambda: clip(1, sd, hx, ho, d, half), a.reps)}
        print("%s: %.3f ms" % (name, calls[name]["call"]["median_ms"]), flush=True)
    calls["host_compiled_one_core_unseeded_scaled"] = {"call": timed(lambda: clip(0, None, hx, ho, d, half), 3)}
    calls["host_compiled_one_core_seeded_scaled"] = {"call": timed(lambda: clip(0, seeds, hx, ho, d, half), 3)}
    res["clip_48x55000"] = calls
    torch.set_num_threads(1)
    res["numpy_float64_one_core_48x55000"] = timed(lambda: numpy_clip(hx, half), 5)
    print("numpy float64 clip: %.3f ms" % res["numpy_float64_one_core_48x55000"]["median_ms"], flush=True)
    # what the kernels sustain: 48 x 1 760 000 (338 MB), device-resident in place
    d_long = 1760000
    big = [torch.from_numpy(values(200 + i % 4, d_long)).cuda() for i in range(n)]
    Sb = [sum_sq(b.cpu().numpy()) for b in big[:4]]
    Tb = [Sb[i % 4] // 2 for i in range(n)]
    out = [torch.empty(d_long, dtype=torch.float32, device="cuda") for _ in range(n)]
    long_res = {}
    t = timed(lambda: quant(seeds, big, out, d_long), a.reps)
    lp = n * ((d_long + 31) // 32)
    long_res["k_quantize_prob"] = {"call": t, "permutations_per_s": lp / (t["median_ms"] * 1e-3)}
    for name, sd in (("unseeded_scaled", None), ("seeded_scaled", seeds)):
        t = timed(lambda: clip(None, sd, big, out, d_long, Tb), a.reps)
        e = {"call": t, "bytes_per_s": 12 * n * d_long / (t["median_ms"] * 1e-3)}
        e["fraction_of_hbm_peak"] = e["bytes_per_s"] / HBM_PEAK
        if sd is not None:
            e["permutations_per_s"] = lp / (t["median_ms"] * 1e-3)
            e["ratio_to_k_quantize_prob"] = e["permutations_per_s"] / long_res["k_quantize_prob"]["permutations_per_s"]
        long_res[name] = e
        print("48x1760000 %s: %.3f ms, %.3g B/s" % (name, t["median_ms"], e["bytes_per_s"]), flush=True)
    res["clip_48x1760000_device"] = long_res
    del big, out
    # crossover for host callers, in elements
    sweep = []
    for sd_name, sd in (("unseeded", None), ("seeded", seeds[:32])):
        for el in (256, 512, 1024, 2048, 4096, 8192, 16384, 32768, 65536, 131072):
            x = [values(el, el)]
            o = [np.empty(el, np.float32)]
            T = [sum_sq(x[0]) // 2]
            h = timed(lambda: clip(0, sd, x, o, el, T), 15)["median_ms"]
            k = timed(lambda: clip(1, sd, x, o, el, T), 15)["median_ms"]
            sweep.append({"form": sd_name, "elements": el, "host_compiled_ms": h, "kernels_host_to_host_ms": k})
    res["crossover_sweep"] = sweep
    res["crossover_elements"] = {f: next((s["elements"] for s in sweep if s["form"] == f and s["kernels_host_to_host_ms"] < s["host_compiled_ms"]), None) for f in ("unseeded", "seeded")}
    print("crossover: %s" % res["crossover_elements"], flush=True)
    if not a.no_encrypt:
        cl = []
        for i in range(n):
            rng = np.random.default_rng(9300 + i)
            x = (rng.integers(-3, 4, size=d) / 128.0).astype(np.float32)
            bl = rng.integers(0, 256, size=(d, 32), dtype=np.uint8); bl[:, 31] &= 0x0F
            r2 = rng.integers(0, 256, size=(d, 32), dtype=np.uint8); r2[:, 31] &= 0x0F
            cl.append((x, bl, r2))
        budget = min(sum_sq(c[0]) for c in cl) // 2      # every update is scaled
        ns, qs, cs = ([bytes([i % 251 + 1]) * 32 for i in range(n)], [bytes([i + 101]) * 32 for i in range(n)], [bytes([i + 151]) * 32 for i in range(n)])
        runs = (("encrypt_batch_private", lambda: R.EncParamsL2.encrypt_batch_private(cl, NB, NPART, L2N, nonce_seeds=ns, fp=FP, quant_seeds=qs)),
                ("encrypt_batch_clipped_without_l2_clip", lambda: R.EncParamsL2.encrypt_batch_clipped(cl, NB, NPART, L2N, nonce_seeds=ns, fp=FP, quant_seeds=qs)),
                ("encrypt_batch_clipped_with_l2_clip", lambda: R.EncParamsL2.encrypt_batch_clipped(cl, NB, NPART, L2N, nonce_seeds=ns, fp=FP, quant_seeds=qs, l2_clip=budget, clip_seeds=cs)))
        for _, f in runs:
            f()
        t = {w: [] for w, _ in runs}
        for _ in range(a.encrypt_reps):
            for w, f in runs:
                t0 = time.perf_counter(); f(); t[w].append(round((time.perf_counter() - t0) * 1e3, 3))
        res["encrypt_batch_l2_48x55000"] = {"l2_clip": budget, "ms": t, "median_ms": {w: float(np.median(v)) for w, v in t.items()}}
        print("encrypt_batch: %s" % res["encrypt_batch_l2_48x55000"]["median_ms"], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
