"""Signatures (rofl_sig_sign: k_sig_digest, k_dh_public, k_sig_sign; rofl_sig_verify: k_sig_digest, k_dh_decode, k_sig_verify) at the sizes a
deployment runs them, on ONE box in ONE run:

  a  sign 96 messages of a threshold-32 round              (a process hosting 48 clients: two commitment messages of 1 057 bytes each)
  b  server verify those 96
  c  server verify 20 000 signatures of 10 000 dealers at threshold 667   (21 377 bytes a message; the total is checked against the 2^30 cap)
  d  client verify_views: 10 000 signatures over ONE view message         (1 320 028 bytes: one serial digest chain, then 10 000 equations)
  e  sign one 213 377-byte message alone                   (the commitments of a 6 667-threshold sharing: the serial digest chain by itself)

The device call: host clock around signatures.sign / verify (they return after their stream has been synchronised) after two warm-ups,
median of --reps repetitions with the spread.  The baseline is rofl_dbg_host_sig_sign / _verify on ONE core of the same box -- the parent
commit has no route at all; a pass that takes more than 5 s is timed once, and case c, whose pass would take minutes, is timed on a stated
number of its signatures (--host-sigs-c, whole dealers: the host's work is the same for every signature): the count is in the result and
the figure for the whole case is that time scaled and marked "not measured".  Before any clock starts the bytes and verdicts of the two
routes are compared on what the host computes, and one signature per case is made wrong and must come back as exactly that verdict.

Operation counts per verified signature (from the formulas of csrc/fe26.hpp: a doubling is 8 field multiplications, an addition 9, a mixed
addition 7): the fixed-base product is at most 32 mixed additions; the variable-base one builds 8 multiples (7 additions), then 64 windows
of 4 doublings and at most 65 additions; one addition joins the two; the encoding is one inverse square root (252 squarings and 11
products in the standard chain, 8 more around it) and 12 products.  bench_femul's figure of the same process is recorded beside them.

  python scripts/gpu_sig.py [--reps 20] [--no-host] [--cases a,b,c,d,e] [--out profiles/signatures.json]

The kernels' own times come from a run of their own:
  rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python scripts/gpu_sig.py --no-host --reps 3 --out ''"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import rofl_project_code_amd as R  # noqa: E402
from rofl_project_code_amd.api import secret_sharing as SS, signatures as G  # noqa: E402

DOUBLE_MULS, ADD_MULS, MADD_MULS, ENCODE_MULS = 8, 9, 7, 252 + 11 + 8 + 12
VERIFY_MULS_AT_MOST = 32 * MADD_MULS + 7 * ADD_MULS + 256 * DOUBLE_MULS + 65 * ADD_MULS + ADD_MULS + ENCODE_MULS
SIGN_MULS_AT_MOST = 32 * MADD_MULS + ENCODE_MULS
CAP = 1 << 30
sz, vp = ctypes.c_size_t, ctypes.c_void_p


def pack(msgs):
    off = np.zeros(len(msgs) + 1, np.uint64)
    off[1:] = np.cumsum([len(m) for m in msgs], dtype=np.uint64)
    return np.frombuffer(b"".join(msgs), np.uint8), off


def refs_arr(refs):
    return np.ascontiguousarray(np.asarray(refs, np.uint32).reshape(-1, 2))


def host_sign(lib, sks, msgs, refs):
    data, off = pack(msgs)
    r = refs_arr(refs)
    out = np.zeros((len(r), 64), np.uint8)
    t0 = time.perf_counter()
    rc = lib.rofl_dbg_host_sig_sign(len(sks), sks.ctypes.data, None, len(msgs), data.ctypes.data, off.ctypes.data, len(r), r.ctypes.data, out.ctypes.data)
    sec_s = time.perf_counter() - t0
    assert rc == 0
    return out, sec_s


def host_verify(lib, pks, msgs, sigs, refs):
    data, off = pack(msgs)
    r, sigs, pks = refs_arr(refs), np.ascontiguousarray(sigs), np.ascontiguousarray(pks)
    out = np.zeros(len(r), np.uint8)
    t0 = time.perf_counter()
    rc = lib.rofl_dbg_host_sig_verify(len(pks), pks.ctypes.data, len(msgs), data.ctypes.data, off.ctypes.data, len(r), r.ctypes.data, sigs.ctypes.data, out.ctypes.data)
    sec_s = time.perf_counter() - t0
    assert rc == 0
    return out, sec_s


def timed(fn, reps):
    fn()                                                           # (warm-up 2; warm-up 1 produced the bytes that were compared)
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ms.append(round((time.perf_counter() - t0) * 1e3, 3))
    return {"ms": ms, "median_ms": float(np.median(ms)), "min_ms": min(ms), "max_ms": max(ms)}


def host_passes(one, first):
    passes = [first]
    while first < 5.0 and len(passes) < 3:
        passes.append(one())
    return {"passes": len(passes), "passes_ms": [round(s * 1e3, 2) for s in passes], "median_ms": round(float(np.median(passes)) * 1e3, 2), "results_equal": True}


def commitment_round(rng, n_dealers, t, round_no=7):
    """(messages, refs): two commitment messages per dealer -- the commitments are random bytes, which is all a signature sees of them"""
    msgs = []
    for d in range(n_dealers):
        com = rng.integers(0, 256, size=(2, t, 32), dtype=np.uint8)
        msgs.append(SS.commitment_message(round_no, d, 0, com[0]))
        msgs.append(SS.commitment_message(round_no, d, 1, com[1]))
    return msgs, [(d, 2 * d + k) for d in range(n_dealers) for k in (0, 1)]


def finish(c, n_sigs, muls):
    c["device"]["us_per_signature"] = round(c["device"]["median_ms"] * 1e3 / n_sigs, 3)
    c["field_multiplications_at_most"] = n_sigs * muls
    if "host" in c:
        c["host_over_device"] = round(c["host"].get("whole_case_ms", c["host"]["median_ms"]) / c["device"]["median_ms"], 2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--no-host", action="store_true", help="skip the host route (the kernel-trace run)")
    ap.add_argument("--cases", default="a,b,c,d,e")
    ap.add_argument("--host-sigs-c", type=int, default=200)
    ap.add_argument("--dealers-c", type=int, default=10000, help="dealers of case c (the case as stated: 10 000)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "signatures.json"), help="'' = print only")
    a = ap.parse_args()
    R.set_device(0)
    lib = R.lib()
    lib.rofl_dbg_host_sig_sign.argtypes = [sz, vp, vp, sz, vp, vp, sz, vp, vp]
    lib.rofl_dbg_host_sig_verify.argtypes = [sz, vp, sz, vp, vp, sz, vp, vp, vp]
    rng = np.random.default_rng(20261120)
    cases = a.cases.split(",")
    res = {"reps": a.reps, "host_clock": "perf_counter around each call after two warm-ups; the call ends in a stream synchronise",
           "baseline": "rofl_dbg_host_sig_sign / _verify on one core", "bench_femul_per_s": R.bench_femul(),
           "field_multiplications_per_signature_at_most": {"verify": VERIFY_MULS_AT_MOST, "sign": SIGN_MULS_AT_MOST}, "cases": {}}

    def say(name, c):
        res["cases"][name] = c
        h = c.get("host")
        print("%s %s: device %.3f ms (%.3f-%.3f)%s" % (name, c["what"], c["device"]["median_ms"], c["device"]["min_ms"], c["device"]["max_ms"],
              "; host %.1f ms over %d pass(es)%s" % (h.get("whole_case_ms", h["median_ms"]), h["passes"],
                                                     " (scaled, not measured)" if h.get("whole_case_is", "measured") != "measured" else "") if h else ""), flush=True)

    if "a" in cases or "b" in cases:
        sks = rng.integers(0, 256, size=(48, 32), dtype=np.uint8)
        msgs, refs = commitment_round(rng, 48, 32)
        sigs, pks = G.sign(sks, msgs, refs, with_public=True)      # (warm-up 1)
        if "a" in cases:
            c = {"what": "sign 96 messages of 48 dealers, t = 32", "kind": "sign", "n_keys": 48, "n_msgs": 96, "n": 96, "message_bytes": len(msgs[0]), "total_bytes": sum(map(len, msgs))}
            if not a.no_host:
                want, first = host_sign(lib, sks, msgs, refs)
                assert (sigs == want).all(), "case a: the device and the host route differ"
                c["host"] = host_passes(lambda: host_sign(lib, sks, msgs, refs)[1], first)
            c["device"] = timed(lambda: G.sign(sks, msgs, refs), a.reps)
            finish(c, 96, SIGN_MULS_AT_MOST)
            say("a", c)
        if "b" in cases:
            bad = sigs.copy(); bad[50, 7] ^= 0x10
            got = G.verify(pks, msgs, bad, refs)                   # (warm-up 1)
            assert got[50] == 1 and got.sum() == 1, "case b: the verdicts are not the one wrong signature"
            c = {"what": "server verify 96 signatures of 48 dealers, t = 32", "kind": "verify", "n_keys": 48, "n_msgs": 96, "n": 96, "message_bytes": len(msgs[0]),
                 "total_bytes": sum(map(len, msgs))}
            if not a.no_host:
                want, first = host_verify(lib, pks, msgs, bad, refs)
                assert (got == want).all(), "case b: the device and the host route differ"
                c["host"] = host_passes(lambda: host_verify(lib, pks, msgs, bad, refs)[1], first)
            c["device"] = timed(lambda: G.verify(pks, msgs, bad, refs), a.reps)
            finish(c, 96, VERIFY_MULS_AT_MOST)
            say("b", c)
    if "c" in cases:
        n_d, t = a.dealers_c, 667
        wrong = (2 * n_d * 5) // 8 | 1
        sks = rng.integers(0, 256, size=(n_d, 32), dtype=np.uint8)
        msgs, refs = commitment_round(rng, n_d, t)
        total = sum(map(len, msgs))
        assert total <= CAP, "case c: %d message bytes are above the cap of 2^30" % total
        sigs, pks = G.sign(sks, msgs, refs, with_public=True)
        bad = sigs.copy(); bad[wrong, 40] ^= 1
        got = G.verify(pks, msgs, bad, refs)                       # (warm-up 1)
        assert got[wrong] == 1 and got.sum() == 1, "case c: the verdicts are not the one wrong signature"
        c = {"what": "server verify %d signatures of %d dealers, t = 667" % (2 * n_d, n_d), "kind": "verify", "n_keys": n_d, "n_msgs": 2 * n_d, "n": 2 * n_d, "message_bytes": len(msgs[0]),
             "total_bytes": total, "cap_bytes": CAP, "total_over_cap": round(total / CAP, 4)}
        if not a.no_host:
            hs = min(a.host_sigs_c, 2 * n_d) // 2 * 2
            lo = max(0, min(wrong // 2 * 2 - hs // 2 // 2 * 2, 2 * n_d - hs))      # (whole dealers, the wrong signature among them)
            d0, nd = lo // 2, hs // 2
            hm, hr = msgs[lo:lo + hs], [(d, 2 * d + k) for d in range(nd) for k in (0, 1)]
            hsig, first_s = host_sign(lib, sks[d0:d0 + nd], hm, hr)
            assert (hsig == sigs[lo:lo + hs]).all(), "case c: the device and the host route differ (sign)"
            want, first = host_verify(lib, pks[d0:d0 + nd], hm, bad[lo:lo + hs], hr)
            assert (got[lo:lo + hs] == want).all() and want.sum() == 1, "case c: the device and the host route differ"
            c["host"] = host_passes(lambda: host_verify(lib, pks[d0:d0 + nd], hm, bad[lo:lo + hs], hr)[1], first)
            c["host"]["signatures_timed"] = hs
            c["host"]["whole_case_ms"] = round(c["host"]["median_ms"] * 2 * n_d / hs, 2)
            c["host"]["whole_case_is"] = "not measured: the time of %d of %d signatures scaled" % (hs, 2 * n_d)
            c["host_sign_ms_of_the_same_signatures"] = round(first_s * 1e3, 2)
        c["device"] = timed(lambda: G.verify(pks, msgs, bad, refs), max(3, a.reps // 4))
        c["python_packing_inside_the_call"] = timed(lambda: R.api._pack_messages(msgs), 3)      # (the wrapper joins the list into one buffer on every call)
        c["device_sign"] = timed(lambda: G.sign(sks, msgs, refs), 3)
        finish(c, 2 * n_d, VERIFY_MULS_AT_MOST)
        say("c", c)
        del msgs, sigs, bad
    if "d" in cases:
        n = 10000
        sks = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
        view = SS.view_message(7, {d: s for d, s in enumerate(rng.integers(0, 256, size=(n, 2, 64), dtype=np.uint8))})
        refs = [(i, 0) for i in range(n)]
        sigs, pks = G.sign(sks, [view], refs, with_public=True)
        bad = sigs.copy(); bad[6789, 33] ^= 2
        got = SS.verify_views(pks, view, bad)                      # (warm-up 1)
        assert got[6789] == 1 and got.sum() == 1, "case d: the verdicts are not the one wrong signature"
        c = {"what": "client verify_views: 10 000 signatures over one message", "kind": "verify", "n_keys": n, "n_msgs": 1, "n": n, "message_bytes": len(view), "total_bytes": len(view)}
        if not a.no_host:
            want, first = host_verify(lib, pks, [view], bad, refs)
            assert (got == want).all(), "case d: the device and the host route differ"
            c["host"] = host_passes(lambda: host_verify(lib, pks, [view], bad, refs)[1], first)
        c["device"] = timed(lambda: SS.verify_views(pks, view, bad), a.reps)
        finish(c, n, VERIFY_MULS_AT_MOST)
        say("d", c)
    if "e" in cases:
        sk = rng.integers(0, 256, size=(1, 32), dtype=np.uint8)
        msg = SS.commitment_message(7, 0, 0, rng.integers(0, 256, size=(6667, 32), dtype=np.uint8))
        sig = G.sign(sk, [msg])                                    # (warm-up 1)
        c = {"what": "sign one message of 213 377 bytes", "kind": "sign", "n_keys": 1, "n_msgs": 1, "n": 1, "message_bytes": len(msg), "total_bytes": len(msg),
             "keccak_permutations": (24 + len(msg)) // 136 + 1}
        if not a.no_host:
            want, first = host_sign(lib, sk, [msg], [(0, 0)])
            assert (sig == want).all(), "case e: the device and the host route differ"
            c["host"] = host_passes(lambda: host_sign(lib, sk, [msg], [(0, 0)])[1], first)
        c["device"] = timed(lambda: G.sign(sk, [msg]), a.reps)
        finish(c, 1, SIGN_MULS_AT_MOST)
        say("e", c)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
