"""Nonce streams and witnesses that make the scalars of the inner-product rounds' L/R-merged MSMs collide -- test infrastructure only.

Nonce.stream hands the prover its nonces byte for byte (mode 0 of k_nonce_expand).  With ONE 64-byte block repeated, every nonce is the
same scalar s, a[k] = bit_k - z + s x takes two values over a chunk (one when all bits of the shifted values are equal), the fold
a' = a_lo u + a_hi / u keeps that, and the G-side MSM scalars of a round, a' tG[h], have at most 2^r times as many distinct values as a'.
Hundreds or thousands of terms of one side then share a bucket in every window, which pseudo-random nonces never do.  The H side stays
spread: b carries y^k and z^(2+j) 2^i.

Three layers, all in Python integers:
  * stream and witness builders (the corpus);
  * a STRUCTURAL model of the merged mode: which side a term of the merged array [Gc | Hc] belongs to (kernels.hpp msm_item /
    msm_side_term) and which G-side terms of a round must carry equal scalars, from the witness bits, the stream's pattern and the prover's
    fold schedule alone (host_prover.hpp: fold_t1, fold_t, fold_min, use_new, the re-materialisation that resets n_g) -- no challenge
    enters it;
  * a REPLAY of a finished proof: the challenges are re-derived from the proof's own bytes with the Merlin transcript of
    tests/golden/pyref.py, l(x), r(x) and every round's merged scalar array are computed exactly as k_lr_first / k_ipp_round define them, and
    the final a, b must equal the proof's last 64 bytes (the replay checks itself).  From the exact scalars tests/msm_model.py gives the
    bucket loads of each side and the chain of attempts each round's msm_run must make (predict_merged).

Scalars are Python integers mod l; arrays for msm_model are uint8 [n][32] little-endian."""
import os
import sys

import numpy as np

import msm_model as M

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import pyref  # noqa: E402

L = M.L
FP = (16, 7)              # fixed-point format of every case: prove_range 8 and 16 fit fp_bits = 16
FOLD_T1, FOLD_T, FOLD_MIN, FB_MIN = 3, 2, 1024, 4096      # Ctx defaults: ROFL_FOLD_T1, ROFL_FOLD_T, ROFL_FOLD_MIN, ROFL_MSM_FB_MIN


# ---------------------------------------------------------------- geometry
def next_pow2(x):
    p = 1
    while p < x:
        p *= 2
    return p


def chunk_m(d, P):
    """values per chunk: the client's d values in P chunks, each padded to a power of two (range_proof_vec/mod.rs)"""
    return next_pow2((d + P - 1) // P)


def nonces_per_chunk(n, m):
    return m * (2 * n + 4)


# ---------------------------------------------------------------- streams (bytes: 64 per nonce, reference draw order)
def block(tag):
    """a fixed 64-byte block that is no special value: SHAKE256 of the tag"""
    import hashlib
    return hashlib.shake_256(b"nonce_collide/" + tag).digest(64)


def stream_zero(count):
    return bytes(64 * count)


def stream_repeat(count, blk=None):
    return (blk or block(b"one")) * count


def stream_alternating(n, m, P, blk_a=None, blk_b=None):
    """two blocks alternating in runs of n, in step with the draw order (per party: a_bl, s_bl, s_L[0..n), s_R[0..n)): s_L is block A
    throughout and s_R block B, so the two differ; the blinding nonces take A"""
    a, b = blk_a or block(b"A"), blk_b or block(b"B")
    party = a + a + a * n + b * n
    return (party * m + a * (2 * m)) * P


def stream_random(count, seed):
    return np.random.default_rng(seed).integers(0, 256, 64 * count, dtype=np.uint8).tobytes()


def stream_chunk_only(n, m, P, chunk, seed, blk=None):
    """random everywhere but in `chunk`, whose share is one block repeated"""
    per = nonces_per_chunk(n, m)
    s = bytearray(stream_random(per * P, seed))
    s[64 * per * chunk:64 * per * (chunk + 1)] = stream_repeat(per, blk)
    return bytes(s)


def stream_partial(n, m, positions, seed, blk=None):
    """one chunk, random but for s_L at the slots `positions` (k = party * n + bit), which all take one block: a class of len(positions)
    equal values of a, of a size the caller chooses (what puts an overflow list BELOW its capacity)"""
    s = bytearray(stream_random(nonces_per_chunk(n, m), seed))
    b = blk or block(b"one")
    for k in positions:
        idx = (k // n) * (2 * n + 2) + 2 + k % n
        s[64 * idx:64 * idx + 64] = b
    return bytes(s)


def stream_scalars(stream, n, m, chunk=0):
    """(s_L[N], s_R[N]) of a chunk as integers mod l, wide-reduced as Scalar::from_bytes_mod_order_wide does"""
    per = nonces_per_chunk(n, m)
    raw = np.frombuffer(stream, np.uint8)[64 * per * chunk:64 * per * (chunk + 1)].reshape(per, 64)
    val = [int.from_bytes(r.tobytes(), "little") % L for r in raw[:m * (2 * n + 2)]]
    sL, sR = [], []
    for j in range(m):
        base = j * (2 * n + 2) + 2
        sL += val[base:base + n]
        sR += val[base + n:base + 2 * n]
    return sL, sR


def stream_classes(stream, n, m, chunk=0):
    """equality classes of s_L over the chunk's N slots, as small integers (equal blocks <=> equal id)"""
    per = nonces_per_chunk(n, m)
    raw = np.frombuffer(stream, np.uint8)[64 * per * chunk:64 * per * (chunk + 1)].reshape(per, 64)
    ids, out = {}, []
    for j in range(m):
        base = j * (2 * n + 2) + 2
        for i in range(n):
            out.append(ids.setdefault(raw[base + i].tobytes(), len(ids)))
    return out


# ---------------------------------------------------------------- witnesses (float32 values at fixed-point FP; the shifted value is k + 2^(n-1))
def vmax(n):
    """the closed upper clip bound of prove_range n: (2^(n-1) - 1) / 2^frac, exact in f32 for n <= 16"""
    return np.float32(((1 << (n - 1)) - 1) / float(1 << FP[1]))


def witness(kind, n, d, seed=0):
    mx = vmax(n)
    if kind == "+max":            # shifted 2^n - 1: every bit set
        return np.full(d, mx, np.float32)
    if kind == "-max":            # shifted 1: one-hot
        return np.full(d, -mx, np.float32)
    if kind == "alternating":
        return np.where(np.arange(d) % 2 == 0, mx, -mx).astype(np.float32)
    if kind == "random":
        rng = np.random.default_rng(seed)
        return np.clip(rng.uniform(-mx, mx, size=d).astype(np.float32), -mx, mx)
    raise ValueError(kind)


def blindings(d, seed):
    bl = np.random.default_rng(seed).integers(0, 256, size=(d, 32), dtype=np.uint8)
    bl[:, 31] &= 0x0F
    return bl


def shifted(values, n, m, P):
    """the shifted integers the proof is about, [P][m]: round-to-nearest-even of |v| 2^frac, signed, + 2^(n-1); padded slots are 0"""
    v = np.asarray(values, np.float32).astype(np.float64)
    k = np.rint(np.abs(v) * float(1 << FP[1])).astype(np.int64)
    s = np.where(v < 0, -k, k) + (1 << (n - 1))
    out = np.zeros(P * m, np.int64)
    out[:len(s)] = s
    return out.reshape(P, m)


def bits_of(shift_row, n):
    """bit k = party * n + i of a chunk"""
    return [(int(v) >> i) & 1 for v in shift_row for i in range(n)]


# ---------------------------------------------------------------- the merged layout, in integers
def is_left(i, lr_nh, lr_ng):
    """msm_item: term i of the merged array [Gc (lr_ng) | Hc (lr_ng)] belongs to L (problem 2q) or to R (2q + 1)"""
    return (i & lr_nh) != 0 if i < lr_ng else (i & lr_nh) == 0


def side_term(side, k, lr_nh, lr_ng):
    """msm_side_term: the k-th term of `side` (0 = L, 1 = R) in the merged array; lr_nh is a power of two"""
    half = lr_ng // 2
    hside = 1 if k >= half else 0
    kk = k - hside * half
    low = lr_nh - 1
    j = ((kk & ~low) << 1) | (kk & low)
    if (side == 1) if hside else (side == 0):
        j |= lr_nh
    return hside * lr_ng + j


def side_indices(side, lr_nh, lr_ng):
    return [side_term(side, k, lr_nh, lr_ng) for k in range(lr_ng)]


def schedule(n, m, P):
    """The prover's rounds at default knobs: [(n_g, r, fixed_base)] -- n_g materialised generators a side, r pending challenges (the logical
    length is n_k = n_g >> r), and whether the round's MSM runs over the window table (first fold level of a shape with 2N >= FB_MIN).
    After a round r grows by one; the generators are re-materialised (n_g >>= r, r = 0) when r has reached fold_t1 (first level) / fold_t and
    the fold pays: n_after >= fold_min, or n_after >= 64 with 2 P n_after >= 8 fold_min."""
    N = n * m
    lg = N.bit_length() - 1
    n_g, r, first, out = N, 0, True, []
    for rnd in range(lg):
        out.append((n_g, r, first and 2 * N >= FB_MIN))
        r += 1
        n_after = n_g >> r
        pays = n_after >= FOLD_MIN or (n_after >= 64 and 2 * P * n_after >= 8 * FOLD_MIN)
        if rnd + 1 < lg and r >= (FOLD_T1 if first else FOLD_T) and pays:
            n_g, r, first = n_after, 0, False
    return out


def g_classes(bits, s_ids, n, m, P):
    """STRUCTURE ONLY.  Per round: (n_g, nh, cls) with cls[j] the equality class of the G-side scalar of merged term j < n_g.  Term j = h n_k + i
    carries a'[ii] tG[h], ii = i +- nh; after R rounds a'[ii] is a fixed combination (the challenges' products) of a[ii + t n_k], t < 2^R,
    and a[k] = bit_k - z + s_L[k] x depends on (bit_k, the block of s_L[k]) alone.  So the class is (h, that tuple of pairs): equal classes
    carry equal scalars for every challenge, distinct ones differ but for coincidences of probability ~2^-252."""
    N = n * m
    ids = {}
    acls = [ids.setdefault((bits[k], s_ids[k]), len(ids)) for k in range(N)]      # class of a[k]
    out = []
    for R, (n_g, r, _) in enumerate(schedule(n, m, P)):
        n_k = n_g >> r
        nh = n_k // 2
        assert n_k == N >> R
        if R:                     # one fold: a'[i] is the same combination of (a[i], a[n_k + i]) for every i -- the tuple above, built pair by pair
            ids = {}
            acls = [ids.setdefault((acls[i], acls[n_k + i]), len(ids)) for i in range(n_k)]
        ids, cls = {}, []
        for j in range(n_g):
            h, i = divmod(j, n_k)
            ii = nh + i if i < nh else i - nh
            cls.append(ids.setdefault((h, acls[ii]), len(ids)))
        out.append((n_g, nh, cls))
    return out


def largest_g_class(bits, s_ids, n, m, P):
    """per round: the most G-side terms of ONE side that must share a scalar (a lower bound of that side's fullest bucket in every window
    whose digit is not zero)"""
    out = []
    for n_g, nh, cls in g_classes(bits, s_ids, n, m, P):
        best = 0
        for side in (0, 1):
            cnt = {}
            for j in range(n_g):
                if is_left(j, nh, n_g) == (side == 0):
                    cnt[cls[j]] = cnt.get(cls[j], 0) + 1
            best = max(best, max(cnt.values()))
        out.append(best)
    return out


# ---------------------------------------------------------------- replay of a finished proof
def transcript_commitments(commits, n, m, P):
    """[P m][32]: what the transcript absorbs as V.  The call returns commitments to the un-shifted values; the proof is about value + 2^(n-1),
    so 2^(n-1) B is added back (range_proof_vec/mod.rs:156-158), and a padded slot is the identity: 32 zero bytes (:163-167)."""
    import orc
    cm = np.ascontiguousarray(commits, np.uint8).reshape(-1, 32)
    off = orc.commit_vec(M.from_int(1 << (n - 1))[None], None)
    rc, V = orc.add_points_vec(cm, np.tile(off, (cm.shape[0], 1)))
    assert rc == 0
    out = np.zeros((P * m, 32), np.uint8)
    out[:cm.shape[0]] = V
    return out


def _inv(x):
    return pow(x, L - 2, L)


def replay(proof, V, shift_row, sL, sR, n, m, P, label=b"RangeProof"):
    """One chunk.  proof: its bytes; V: the chunk's m commitments as the transcript saw them [m][32]; shift_row: its m shifted integers;
    sL, sR: its nonces (stream_scalars); P: the chunks of the call (the fold schedule depends on it).
    -> list per round of dict(n_g, nh, fixed_base, merged = the 2 n_g scalars of the merged array as integers).  Raises AssertionError when the
    replayed a, b are not the proof's: then the transcript or the arithmetic here is not the prover's, and no prediction may be drawn."""
    proof = bytes(np.asarray(proof, np.uint8).tobytes())
    N = n * m
    lg = N.bit_length() - 1
    assert len(proof) == 32 * (9 + 2 * lg)
    T = pyref.Transcript(label)
    T.append_message(b"dom-sep", b"rangeproof v1")
    T.append_u64(b"n", n)
    T.append_u64(b"m", m)
    for j in range(m):
        T.append_message(b"V", bytes(np.asarray(V[j], np.uint8).tobytes()))
    T.append_message(b"A", proof[0:32])
    T.append_message(b"S", proof[32:64])
    y, z = T.challenge_scalar(b"y"), T.challenge_scalar(b"z")
    T.append_message(b"T_1", proof[64:96])
    T.append_message(b"T_2", proof[96:128])
    x = T.challenge_scalar(b"x")
    T.append_message(b"t_x", proof[128:160])
    T.append_message(b"t_x_blinding", proof[160:192])
    T.append_message(b"e_blinding", proof[192:224])
    T.challenge_scalar(b"w")
    T.append_message(b"dom-sep", b"ipp v1")
    T.append_u64(b"n", N)
    us = []
    for rnd in range(lg):
        o = 224 + 64 * rnd
        T.append_message(b"L", proof[o:o + 32])
        T.append_message(b"R", proof[o + 32:o + 64])
        us.append(T.challenge_scalar(b"u"))
    bits = bits_of(shift_row, n)
    zz, yinv = z * z % L, _inv(y)
    a, b, yinvpow = [], [], []
    yk, yik = 1, 1
    zj = [zz * pow(z, j, L) % L for j in range(m)]
    for k in range(N):
        j, i = divmod(k, n)
        a.append((bits[k] - z + sL[k] * x) % L)
        b.append((yk * (bits[k] - 1 + z) + zj[j] * (1 << i) + yk * sR[k] % L * x) % L)
        yinvpow.append(yik)
        yk, yik = yk * y % L, yik * yinv % L
    assert sum(p * q for p, q in zip(a, b)) % L == int.from_bytes(proof[128:160], "little"), "t_x of the proof is not <l(x), r(x)> of the replay"
    rounds = []
    gscale = hscale = 1
    pend = []                     # pending challenges, oldest first: challenge q <-> bit r - 1 - q of h
    for rnd, (n_g, r, fb) in enumerate(schedule(n, m, P)):
        assert r == len(pend)
        n_k = n_g >> r
        nh = n_k // 2
        if rnd:
            u = us[rnd - 1]
            ui = _inv(u)
            a = [(a[i] * u + a[n_k + i] * ui) % L for i in range(n_k)]
            b = [(b[i] * ui + b[n_k + i] * u) % L for i in range(n_k)]
        tG, tH = [gscale], [hscale]
        for u in pend:            # table over h: the newest challenge is bit 0
            ui = _inv(u)
            tG = [t * f % L for t in tG for f in (ui, u)]
            tH = [t * f % L for t in tH for f in (u, ui)]
        merged = [0] * (2 * n_g)
        for j in range(n_g):
            h, i = divmod(j, n_k)
            ii = nh + i if i < nh else i - nh
            merged[j] = a[ii] * tG[h] % L
            merged[n_g + j] = b[ii] * tH[h] % L * yinvpow[j] % L
        rounds.append({"n_g": n_g, "nh": nh, "fixed_base": fb, "merged": merged})
        pend.append(us[rnd])
        nxt = schedule(n, m, P)[rnd + 1] if rnd + 1 < lg else None
        if nxt is not None and nxt[1] == 0:      # re-materialised: s_G(0) = prod u^-1 and s_H(0) = prod u move into the scales
            for u in pend:
                gscale, hscale = gscale * _inv(u) % L, hscale * u % L
            pend = []
    u = us[-1]
    ui = _inv(u)
    a_fin, b_fin = (a[0] * u + a[1] * ui) % L, (b[0] * ui + b[1] * u) % L
    o = 224 + 64 * lg
    assert (a_fin, b_fin) == (int.from_bytes(proof[o:o + 32], "little"), int.from_bytes(proof[o + 32:o + 64], "little")), "replayed a, b differ from the proof's"
    return rounds


def side_scalars(rnd):
    """(L terms, R terms) of a replayed round as uint8 [n_g][32], in the order msm_side_term enumerates them"""
    out = []
    for side in (0, 1):
        idx = side_indices(side, rnd["nh"], rnd["n_g"])
        assert all(is_left(i, rnd["nh"], rnd["n_g"]) == (side == 0) for i in idx) and len(set(idx)) == rnd["n_g"]
        out.append(M.from_ints([rnd["merged"][i] for i in idx]))
    return out


def predict(chunks, n, m):
    """chunks: the replayed rounds of every chunk of ONE call.  -> per round the attempts of its merged launch (msm_model.predict_merged)"""
    out = []
    for rnd in range(len(chunks[0])):
        sides = [s for ch in chunks for s in side_scalars(ch[rnd])]
        out.append(M.predict_merged(sides, chunks[0][rnd]["n_g"], 2 * n * m, chunks[0][rnd]["fixed_base"]))
    return out


def retries_of(chains):
    """how often each repeat class must occur over predicted chains -> (small_overflow, bin_overflow_to_slots, slot_overflow); attempts whose
    repeat the model cannot tell (repeated None) are left to the caller"""
    small = sum(1 for ch in chains for a in ch if a["kind"] == "small" and a["repeated"])
    two = sum(1 for ch in chains for a in ch if a["two"] and a["repeated"])
    slot = sum(1 for ch in chains for a in ch if not a["two"] and a["kind"] in ("fixed_base", "slots") and a["repeated"])
    return small, two, slot


# ---------------------------------------------------------------- the corpus
# must: (round, structure) pairs the case is built to run over -- structure_loads() must show load > capacity there.  Structures:
#   small     a bucket list of the fused small launch (64 / 72 entries)
#   slots     a bucket's slots in the generic slot sort;   ovf_list   that sort's overflow list (4096 entries)
#   fb_slots  a bucket's slots in the fixed-base slot sort; fb_ovf_list its overflow list
#   bin       a coarse bin of the two-level sort, main region and tail together
# in_place: rounds whose slot sort must leave 1 .. 4096 entries to the overflow list (handled by k_msm_overflow, no repeat)
def _case(id, n, m, P, wit, stream, d=None, verdict=True, must=(), in_place=(), control=False, collide_chunk=0):
    return {"id": id, "n": n, "m": m, "P": P, "d": P * m if d is None else d, "witness": wit, "stream": stream, "verdict": verdict, "must": tuple(must),
            "in_place": tuple(in_place), "control": control, "collide_chunk": collide_chunk}


def _per(n, m, P=1):
    return nonces_per_chunk(n, m) * P


PARTIAL_80 = list(range(0, 80)) + list(range(256, 336))      # 80 slots of the low half and 80 of the high half of a 512-slot chunk

CASES = [
    # (8, 64, 1): N = 512, no window table (2N < FB_MIN): every round is a generic merged launch through the fused small launch
    _case("512-repeat-max", 8, 64, 1, "+max", lambda: stream_repeat(_per(8, 64)), must=[(0, "small"), (0, "slots"), (0, "ovf_list"), (1, "small"), (1, "ovf_list")]),
    _case("512-repeat-minus-max", 8, 64, 1, "-max", lambda: stream_repeat(_per(8, 64)), must=[(0, "small"), (0, "ovf_list")]),
    _case("512-repeat-alternating", 8, 64, 1, "alternating", lambda: stream_repeat(_per(8, 64)), must=[(0, "small"), (0, "ovf_list")]),
    _case("512-repeat-one-short", 8, 64, 1, "+max", lambda: stream_repeat(_per(8, 64)), d=63, must=[(0, "small"), (0, "ovf_list")]),
    _case("512-repeat-random-witness", 8, 64, 1, "random", lambda: stream_repeat(_per(8, 64)), must=[(0, "small")]),
    _case("512-zero-max", 8, 64, 1, "+max", lambda: stream_zero(_per(8, 64)), verdict=False, must=[(0, "small"), (0, "ovf_list")]),
    _case("512-alternating-minus-max", 8, 64, 1, "-max", lambda: stream_alternating(8, 64, 1), must=[(0, "small"), (0, "ovf_list")]),
    _case("512-partial80-max", 8, 64, 1, "+max", lambda: stream_partial(8, 64, PARTIAL_80, 4), must=[(0, "small"), (0, "slots")], in_place=[0, 1]),
    _case("512-random", 8, 64, 1, "random", lambda: stream_random(_per(8, 64), 3), control=True),
    # (16, 128, 1): N = 2048, window table; the prover never re-materialises at P = 1 (n_after = 256 < fold_min), so every round is a fixed-base
    # launch below 8192 terms a side: the fixed-base slot sort, then -- repeated -- the generic variants over the same generators
    _case("2048-repeat-max", 16, 128, 1, "+max", lambda: stream_repeat(_per(16, 128)), must=[(0, "fb_slots"), (0, "fb_ovf_list"), (0, "small"), (0, "ovf_list")], in_place=[6]),
    _case("2048-random", 16, 128, 1, "random", lambda: stream_random(_per(16, 128), 3), control=True),
    # (16, 1024, 1): N = 16 384: 8192 terms a side and more -> coarse bins; rounds 0 .. 2 over the window table, one re-materialisation, generic after it
    _case("16384-repeat-max", 16, 1024, 1, "+max", lambda: stream_repeat(_per(16, 1024)), must=[(0, "bin"), (0, "fb_ovf_list"), (0, "ovf_list"), (1, "bin"), (3, "small"), (3, "ovf_list")]),
    # (8, 64, 4): the collisions sit in chunk 2 alone
    _case("4x512-chunk2", 8, 64, 4, "+max", lambda: stream_chunk_only(8, 64, 4, 2, 11), must=[(0, "small"), (0, "ovf_list")], collide_chunk=2),
]
CASE_IDS = [c["id"] for c in CASES]
_DATA = {}


def case_by_id(cid):
    return CASES[CASE_IDS.index(cid)]


def case_inputs(case):
    """(values, blindings, stream) of a case: functions of the case alone"""
    return witness(case["witness"], case["n"], case["d"], seed=5), blindings(case["d"], 9), case["stream"]()


def case_data(case):
    """Everything a test needs of a case, computed once per process: inputs, the oracle's proof and verdict, the replayed rounds of every
    chunk and the predicted attempt chain of every round."""
    import orc
    if case["id"] in _DATA:
        return _DATA[case["id"]]
    n, m, P, d = case["n"], case["m"], case["P"], case["d"]
    assert chunk_m(d, P) == m
    vals, bl, stream = case_inputs(case)
    assert len(stream) == 64 * _per(n, m, P)
    rc, opr, ocm = orc.create_rangeproof(vals, bl, n, P, FP[0], FP[1], stream=stream)
    out = {"vals": vals, "bl": bl, "stream": stream, "rc": rc, "opr": opr, "ocm": ocm}
    if rc == 0:
        out["verdict"] = orc.verify_rangeproof(opr, ocm, n, FP[0], FP[1])
        sh, V = shifted(vals, n, m, P), transcript_commitments(ocm, n, m, P)
        out["shifted"] = sh
        out["chunks"] = [replay(opr[c], V[c * m:(c + 1) * m], sh[c], *stream_scalars(stream, n, m, c), n, m, P) for c in range(P)]
        out["chains"] = predict(out["chunks"], n, m)
    _DATA[case["id"]] = out
    return out


def structure_loads(case, data, rnd):
    """{structure: (load, capacity)} of round `rnd`, for the structures the round's launch could reach (whether it does is the chain's business):
    the fullest bucket against a list / the slots, the overflow word against the overflow list, the fullest bin against all its room"""
    n, m = case["n"], case["m"]
    sides = [s for ch in data["chunks"] for s in side_scalars(ch[rnd])]
    n_g, nq = data["chunks"][0][rnd]["n_g"], len(data["chunks"])
    out = {}
    if data["chunks"][0][rnd]["fixed_base"]:
        f = M.merged_fixed_plan(n_g, nq, 2 * n * m)
        sl = [M.merge_sets(M.loads(s, f["c"]), f["sets"]) for s in sides]
        out["fb_slots"] = (max(int(x.max()) for x in sl), f["cap"])
        out["fb_ovf_list"] = (sum(M.overflow(x, f["cap"]) for x in sl), M.OVF_MAX)
        if f["two"]:
            out["bin"] = (max(int(M.bin_loads(x, f["fbits"]).max()) for x in sl), f["cap_bin"] + M.BIN_TAIL)
    g = M.merged_generic_plan(2 * n_g, nq)
    if g["small"]:
        out["small"] = (max(int(M.loads(s, g["c_small"]).max()) for s in sides), g["small_cap"])
    ld = [M.loads(s, g["c"]) for s in sides]
    out["slots"] = (max(int(x.max()) for x in ld), g["cap"])
    out["ovf_list"] = (sum(M.overflow(x, g["cap"]) for x in ld), M.OVF_MAX)
    return out
