"""The window layout, the digits and the retry policy of the Pippenger driver (csrc/kernels.hpp msm_window / msm_digit, csrc/host_msm.hpp
msm_plan_job / msm_retry) in plain Python integers -- test infrastructure only.

A scalar k < 2^253 is cut into W windows (plan(c)); window w gives the signed Booth digit d_w with sum_w d_w 2^pos_w == k, and the term
goes into bucket |d_w| - 1 of window w (two entries, buckets B - 1 and |d_w| - B - 1, when |d_w| > B: only the top window of a scalar
>= 2^252 + 2^(252 - c) can do that, and no scalar below l is that large for c <= 16 -- the top digit of every k in [2^252, l) is exactly B).
loads() counts the entries per (window, bucket); the builders return canonical scalars whose loads at chosen buckets are exact, so that a
test can put a fixed-size structure of the driver at its capacity, one over, and far over, and say which overflow word must come back.

Scalars travel as numpy uint8 arrays [n][32], little-endian, as the C ABI takes them."""
import numpy as np

L = 2 ** 252 + 27742317777372353535851937790883648493
OVF_MAX = 4096            # MSM_OVF_MAX: entries of the slot sort's overflow list
SIZEOF_GE = 128
TOP_RANGE = -1            # build(): a group (TOP_RANGE, 0, count) replaces `count` terms by scalars of [2^252, l): top-window digit exactly B


def plan(c):
    """msm_plan_c: W windows; `wide` windows of c bits, then windows of c - 1 bits, the top window [253 - c, 254) of c + 1 bits."""
    W = (253 - c + c - 1) // c + 1
    wide = (253 - c) - (c - 1) * (W - 1)
    win = []
    for w in range(W):
        if w + 1 == W:
            win.append((253 - c, c + 1))
        elif w < wide:
            win.append((w * c, c))
        else:
            win.append((wide * c + (w - wide) * (c - 1), c - 1))
    return {"c": c, "W": W, "wide": wide, "B": 1 << (c - 1), "windows": win}


def digit(k, pos, width):
    """msm_digit: the Booth digit of the window [pos, pos + width) of k, in [-2^(width-1), 2^(width-1)] (it borrows bit pos - 1)."""
    x = ((k << 1) >> pos) & ((1 << (width + 1)) - 1)
    V, bm1 = x >> 1, x & 1
    top = (V >> (width - 1)) & 1
    return (V & ((1 << (width - 1)) - 1)) + bm1 - (top << (width - 1))


def digits(k, c):
    return [digit(k, pos, width) for pos, width in plan(c)["windows"]]


def entries(d, B):
    """bucket indices (0-based) that a digit occupies: none for 0, two when |d| > B"""
    a = abs(d)
    if a > B:
        return [B - 1, a - B - 1]
    return [a - 1] if a else []


def to_int(row):
    return int.from_bytes(bytes(row), "little")


def from_int(k):
    return np.frombuffer(int(k).to_bytes(32, "little"), np.uint8)


def from_ints(ks):
    return np.stack([from_int(k) for k in ks])


def digits_np(scal, c, only=None):
    """digits() of every scalar of scal [n][32] at once: int64 [n][W] (only = w: that window alone, int64 [n])"""
    scal = np.ascontiguousarray(scal, dtype=np.uint8).reshape(-1, 32)
    bits = np.unpackbits(scal, axis=1, bitorder="little")
    bits = np.concatenate([np.zeros((bits.shape[0], 1), np.uint8), bits], axis=1)      # column j + 1 = bit j, column 0 = "bit -1"
    P = plan(c)
    out = np.zeros((scal.shape[0], P["W"]), np.int64)
    for w, (pos, width) in enumerate(P["windows"]):
        if only is not None and w != only:
            continue
        x = bits[:, pos:pos + width + 1].astype(np.int64) @ (np.int64(1) << np.arange(width + 1, dtype=np.int64))
        V, bm1 = x >> 1, x & 1
        top = (V >> (width - 1)) & 1
        out[:, w] = (V & ((1 << (width - 1)) - 1)) + bm1 - (top << (width - 1))
    return out if only is None else out[:, only]


def loads(scal, c):
    """entries per (window, bucket) of one problem: int64 [W][B]"""
    P = plan(c)
    B = P["B"]
    a = np.abs(digits_np(scal, c))
    out = np.zeros((P["W"], B), np.int64)
    for w in range(P["W"]):
        col = a[:, w]
        big = col > B
        first = np.where(big, B, col)
        out[w] += np.bincount(first[first > 0] - 1, minlength=B)
        if big.any():
            out[w] += np.bincount(col[big] - B - 1, minlength=B)
    return out


def merge_sets(ld, sets):
    """fixed-base: windows s, s + sets, s + 2 sets, ... of a problem share bucket set s: [W][B] -> [sets][B]"""
    return np.stack([ld[s::sets].sum(axis=0) for s in range(sets)])


def overflow(ld, cap):
    """what the slot sort's overflow word must show: the entries that find the `cap` slots of their bucket taken"""
    return int(np.maximum(np.asarray(ld) - cap, 0).sum())


def random_scalars(rng, n):
    """n scalars uniform below 2^252 (all canonical, every bit below 252 uniform)"""
    s = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    s[:, 31] &= 0x0F
    return s


def top_range_scalars(rng, n):
    """n scalars in [2^252, l): 2^252 + r with r < 2^124.  Their top-window digit is exactly B for every c <= 16."""
    s = np.zeros((n, 32), np.uint8)
    s[:, :15] = rng.integers(0, 256, size=(n, 15), dtype=np.uint8)
    s[:, 15] = rng.integers(0, 16, size=n, dtype=np.uint8)
    s[:, 31] = 0x10
    return s


def _encode(d, width, bm1, top_window, B):
    """the `width` window bits V that give digit d next to the borrowed bit bm1"""
    half = 1 << (width - 1)
    v = d - bm1
    if top_window:
        if not 0 <= v < B:
            raise ValueError("the top window of a scalar below 2^252 holds digits 0 .. B")
    elif not -half <= v < half:
        raise ValueError("digit %d does not fit a window of %d bits with borrowed bit %d" % (d, width, bm1))
    return v & ((1 << width) - 1)


def force(scal, idx, window, d, c):
    """Rewrites bits [pos - 1, pos + width) of the terms `idx` in place so that their digit in `window` is d.  The borrowed bit alternates
    over the terms where d leaves the choice (it is the top bit of window - 1: that window's digit changes sign with it, and the top bit
    of this window is borrowed by window + 1)."""
    P = plan(c)
    pos, width = P["windows"][window]
    half = 1 << (width - 1)
    top_window = window + 1 == P["W"]
    for j, i in enumerate(idx):
        bm1 = j & 1
        if pos == 0 or d == -half or (top_window and d == 0):
            bm1 = 0
        if d == half or (top_window and d == P["B"]):
            bm1 = 1
        if pos == 0 and bm1:
            raise ValueError("window 0 has no borrowed bit: its digits end at 2^(width-1) - 1")
        V = _encode(d, width, bm1, top_window, P["B"])
        k = to_int(scal[i])
        if pos == 0:
            k = (k & ~((1 << width) - 1)) | V
        else:
            k = (k & ~(((1 << (width + 1)) - 1) << (pos - 1))) | (((V << 1) | bm1) << (pos - 1))
        scal[i] = from_int(k)
    return scal


def build(n, c, groups, seed, base=None):
    """n canonical scalars, seeded, in which every group (window, digit, count) of `groups` has exactly `count` terms with that digit in that
    window and NO other term touches that bucket.  Groups of one window and of neighbouring windows get disjoint terms (forcing a window
    rewrites one bit of each neighbour); other groups share terms, so the total may exceed n.  A group (TOP_RANGE, 0, count) makes `count`
    terms scalars of [2^252, l) instead.  Returns (scalars, {(window, bucket): load})."""
    rng = np.random.default_rng(seed)
    scal = random_scalars(rng, n) if base is None else np.array(base, dtype=np.uint8, copy=True).reshape(n, 32)
    P = plan(c)
    B, W = P["B"], P["W"]
    order = [int(i) for i in rng.permutation(n)]
    used = {}
    claims = {}
    frozen = set()      # the terms of TOP_RANGE groups: whole scalars, taken from the far end of the order, never forced afterwards
    for w, d, cnt in sorted(groups, key=lambda g: g[0] != TOP_RANGE):
        top_range = w == TOP_RANGE
        if top_range:
            w, d = W - 1, B
        busy = used.get(w - 1, set()) | used.get(w, set()) | used.get(w + 1, set()) | frozen
        idx = []
        for i in (reversed(order) if top_range else order):
            if len(idx) == cnt:
                break
            if i not in busy:
                idx.append(i)
        if len(idx) < cnt:
            raise ValueError("not enough free terms for group (%d, %d, %d)" % (w, d, cnt))
        if top_range:
            scal[idx] = top_range_scalars(rng, cnt)
            frozen.update(idx)
        else:
            force(scal, idx, w, d, c)
        used.setdefault(w, set()).update(idx)
        for b in entries(d, B):
            claims[(w, b)] = claims.get((w, b), 0) + cnt
    # every other term leaves the claimed buckets: new low bits of that window only (neither its top bit, which the next window borrows,
    # nor its borrowed bit change; in the top window bit 252 stays clear, and a scalar above 2^252 keeps its bits from 124 up clear),
    # until its digit points elsewhere
    for w in sorted(used):
        pos, width = P["windows"][w]
        free = width - 1 if w + 1 < W else width - 2
        taken = np.array(sorted({b for (ww, b) in claims if ww == w}), np.int64)
        mine = np.zeros(n, bool)
        mine[list(used[w])] = True
        for _ in range(64):
            a = np.abs(digits_np(scal, c, only=w))
            hit = np.isin(np.minimum(a, B) - 1, taken) | ((a > B) & np.isin(a - B - 1, taken))
            bad = np.nonzero(hit & ~mine)[0]
            if not len(bad):
                break
            for i in bad:
                k = to_int(scal[i])
                f = free if k < 1 << 252 else min(free, max(0, 124 - pos))
                if f == 0:
                    raise ValueError("term %d cannot leave window %d" % (i, w))
                k = (k & ~(((1 << f) - 1) << pos)) | (int(rng.integers(0, 1 << f)) << pos)
                scal[i] = from_int(k)
        else:
            raise ValueError("window %d does not settle" % w)
    if any(to_int(scal[i]) >= L for i in np.nonzero(scal[:, 31] >= 0x10)[0]):
        raise ValueError("a scalar left the canonical range")
    return scal, claims


def sites(c):
    """The (window, digit) sites of the spread family, in the order the excess is handed out: a bucket and its twin in another bucket array
    (equal bucket index, hence equal index mod 64: k_msm_overflow gives an entry to lane `index & 63`), a negative digit, +B and -B in windows
    of c bits, a small digit in the top window, one more plain bucket, and the scalars of [2^252, l) (top-window digit exactly B)."""
    P = plan(c)
    B, W = P["B"], P["W"]
    assert P["wide"] >= 10 and B >= 16
    return [(1, 5), (3, 5), (2, -7), (5, B), (7, -B), (W - 1, 3), (9, 11), (TOP_RANGE, 0)]


def spread(c, cap, excess):
    """groups that load site i of sites(c) with cap + excess[i] entries"""
    return [(w, d, cap + e) for (w, d), e in zip(sites(c), excess)]


def split(total):
    """`total` over the eight sites: at most 4 to the scalars of [2^252, l) (their zero bits 125 .. 251 put them all into a handful of buckets
    of the window that straddles bit 124, which a large group would overflow as well), the rest as evenly as it goes"""
    last = min(4, total // 8)
    rest = total - last
    return [rest // 7 + (1 if i < rest % 7 else 0) for i in range(7)] + [last]


# ---- the driver's policy at default knobs (msm_plan, msm_plan_job, msm_retry_inner), for generic problems
def generic_plan(n, np_=1):
    """what msm_plan_job decides for np_ generic problems of n terms: the window width of the slot / count-sort variants (c), whether the fused
    small launch takes the shape first and with which width and list capacity, the slots per bucket, and how the problems are finished"""
    t10 = 2048 if np_ >= 32 else 512
    c = 16 if n >= 1 << 17 else 13 if n >= 8192 else 10 if n >= t10 else 7 if n >= 64 else 4
    c_small = 10 if (n <= 8192 and c > 10 and np_ * 26 <= 512) else c
    Ps = plan(c_small)
    Bs = Ps["B"]
    small_cap = 64 if n <= 8 * Bs else 72
    small_lds = max(Bs * 4 * (1 + small_cap), ((Bs // 8) * 4 + (Bs // 16) * 5 + 1) * SIZEOF_GE, (Bs + Bs * 3 // 4 + 1) * SIZEOF_GE)
    small = n <= 8192 and c_small <= 10 and n <= 16 * Bs and (np_ * Ps["W"] <= 512 or small_lds <= 24 * 1024)
    cap = 16
    while cap < 256 and cap * plan(c)["B"] < 4 * n:
        cap *= 2
    return {"c": c, "small": small, "c_small": c_small, "small_cap": small_cap, "small_group": 4 if (small and Bs == 64 and np_ * Ps["W"] > 512) else 1,
            "cap": cap}


def predict_generic(problems):
    """The attempts msm_run makes for the generic problems `problems` [np][n][32]: a list of (kind, c, overflow word or None, repeated).  The word
    of the small launch is a flag (None = any non-zero value), that of the slot sort a count."""
    np_, n = problems.shape[0], problems.shape[1]
    g = generic_plan(n, np_)
    out = []
    if g["small"]:
        over = any(int(loads(p, g["c_small"]).max()) > g["small_cap"] for p in problems)
        out.append(("small", g["c_small"], None if over else 0, over))
        if not over:
            return out
    word = sum(overflow(loads(p, g["c"]), g["cap"]) for p in problems)
    out.append(("slots", g["c"], word, word > OVF_MAX))
    if word > OVF_MAX:
        out.append(("count_sort", g["c"], 0, False))
    return out


# ---- the same policy for the L/R-merged launches of the inner-product rounds (MsmOpt::lr_nh != 0): ONE scalar array of n = 2 n_g terms over
# [Gc | Hc] per chunk serves problems 2q (L) and 2q + 1 (R); every term belongs to one side, so a problem has per_side = n / 2 terms
BIN_TAIL = 2048           # MSM_BIN_TAIL: entries of a coarse bin's tail region
FB_THREADS = 1 << 19      # Ctx::msm_fb_threads: accumulate threads a fixed-base launch asks for when it is alone on the device


def bin_cap(avg):
    """msm_bin_cap at the default ROFL_MSM_BIN_SIGMA = 8: twice the mean load of a bin, eight standard deviations, 64, rounded up to 64"""
    hot, dev = 2 * avg, 1
    while dev * dev < hot:
        dev += 1
    return (hot + 8 * dev + 64 + 63) // 64 * 64


def _slot_cap(B, n):
    cap = 16
    while cap < 256 and cap * B < 4 * n:
        cap *= 2
    return cap


def merged_generic_plan(n, nq):
    """msm_plan_job for a generic merged launch of nq chunks (np = 2 nq problems) with n = 2 n_g merged terms: the window width follows n and
    np, everything that is sized per problem follows per_side = n / 2; `cap` from 4 n / B for the layout of each variant"""
    np_, per_side = 2 * nq, n // 2
    t10 = 2048 if np_ >= 32 else 512
    c = 16 if n >= 1 << 17 else 13 if n >= 8192 else 10 if n >= t10 else 7 if n >= 64 else 4
    c_small = 10 if (per_side <= 8192 and c > 10 and np_ * 26 <= 512) else c
    Ps = plan(c_small)
    Bs = Ps["B"]
    small_cap = 64 if per_side <= 8 * Bs else 72
    small_lds = max(Bs * 4 * (1 + small_cap), ((Bs // 8) * 4 + (Bs // 16) * 5 + 1) * SIZEOF_GE, (Bs + Bs * 3 // 4 + 1) * SIZEOF_GE)
    small = per_side <= 8192 and c_small <= 10 and per_side <= 16 * Bs and (np_ * Ps["W"] <= 512 or small_lds <= 24 * 1024)
    return {"c": c, "per_side": per_side, "small": small, "c_small": c_small, "small_cap": small_cap, "cap_small": _slot_cap(Bs, n),
            "small_group": 4 if (small and Bs == 64 and np_ * Ps["W"] > 512) else 1, "cap": _slot_cap(plan(c)["B"], n)}


def merged_fixed_plan(n_g, nq, stride, c=16, want=FB_THREADS):
    """the fixed-base branch of msm_plan_job for a merged launch over the window table of a shape with `stride` = 2 N generators: bucket sets
    per problem, windows per set, slots per bucket, and -- from 8192 terms a side on, at 2^14 or 2^15 buckets -- the two-level sort with the
    capacity of its coarse bins.  per_side = n_g."""
    P = plan(c)
    W, B, per_side = P["W"], P["B"], n_g
    sets = W
    for sdiv in range(1, W + 1):
        if W % sdiv == 0 and nq * 2 * sdiv * B >= want:
            sets = sdiv
            break
    wide_b = B in (32768, 16384)
    if wide_b and per_side >= 8192:
        while sets < W and bin_cap(per_side * (W // sets) // 512) * 4 + 1024 > 96 * 1024:
            sets += 1
            while sets < W and W % sets:
                sets += 1
    wps = W // sets
    cap = 16
    while cap < 2048 and cap * B < 3 * per_side * (wps + 1):
        cap *= 2
    if wps == 1:
        cap *= 2
    two = wide_b and W * stride <= 1 << 24
    nbins, fbits, cap_bin = 256, 7 if B == 32768 else 6, 0
    if two:
        cap_bin = bin_cap(per_side * wps // nbins)
        if cap_bin * 4 + 1024 > 96 * 1024:
            nbins, fbits = 512, fbits - 1
            cap_bin = bin_cap(per_side * wps // nbins)
        if cap_bin * 4 + 1024 > 96 * 1024 or per_side < 8192:
            two = False
    return {"c": c, "W": W, "B": B, "per_side": per_side, "sets": sets, "wps": wps, "cap": cap, "two": two, "cap_bin": cap_bin if two else 0,
            "nbins": nbins, "fbits": fbits}


def bin_loads(set_loads, fbits):
    """[sets][B] bucket loads -> [sets][bins]: the entries of each coarse bin (bucket >> fbits) of the two-level sort"""
    ld = np.asarray(set_loads)
    return ld.reshape(ld.shape[0], -1, 1 << fbits).sum(axis=2)


def bin_verdict(max_bin_load, cap_bin):
    """Does a coarse bin with this many entries overflow?  True above cap_bin + BIN_TAIL (a bin's main region and its tail are all the room
    it has), False up to cap_bin - 64 (what msm_bin_cap sizes the main region for; the 64 on top are its allowance for the left-overs),
    None in between: level 1 reserves main-region space in multiples of 32 per tile, so the exact capacity is not a function of the loads."""
    if max_bin_load > cap_bin + BIN_TAIL:
        return True
    return False if max_bin_load <= cap_bin - 64 else None


def predict_merged(sides, n_g, stride, fixed_base):
    """The attempts msm_run makes for ONE merged launch.  sides: [np][per_side][32], problem 2q = the L terms of chunk q, 2q + 1 its R terms.
    -> list of dicts kind, two, c, W, cap, cap_bin, overflow, repeated; overflow is None where the word is only a flag (small launch, two-level
    sort: non-zero exactly when repeated) and repeated is None where bin_verdict cannot tell (the list then goes on as if it were repeated)."""
    sides = [np.ascontiguousarray(s, dtype=np.uint8).reshape(-1, 32) for s in sides]
    nq, n = len(sides) // 2, 2 * n_g
    out = []

    def att(kind, two, c, cap, cap_bin, overflow, repeated):
        out.append({"kind": kind, "two": two, "c": c, "W": plan(c)["W"], "cap": cap, "cap_bin": cap_bin, "overflow": overflow, "repeated": repeated})

    if fixed_base:
        f = merged_fixed_plan(n_g, nq, stride)
        set_loads = [merge_sets(loads(s, f["c"]), f["sets"]) for s in sides]
        if f["two"]:
            verdict = bin_verdict(max(int(bin_loads(sl, f["fbits"]).max()) for sl in set_loads), f["cap_bin"])
            att("fixed_base", True, f["c"], f["cap"], f["cap_bin"], None, verdict)
            if verdict is False:
                return out
        word = sum(overflow(sl, f["cap"]) for sl in set_loads)
        att("fixed_base", False, f["c"], f["cap"], 0, word, word > OVF_MAX)
        if word <= OVF_MAX:
            return out
    g = merged_generic_plan(n, nq)
    if g["small"]:
        over = any(int(loads(s, g["c_small"]).max()) > g["small_cap"] for s in sides)
        att("small", False, g["c_small"], g["cap_small"], 0, None, over)
        if not over:
            return out
    word = sum(overflow(loads(s, g["c"]), g["cap"]) for s in sides)
    att("slots", False, g["c"], g["cap"], 0, word, word > OVF_MAX)
    if word > OVF_MAX:
        att("count_sort", False, g["c"], g["cap"], 0, 0, False)
    return out


def finisher(np_, fixed_base, host8):
    """who combines the windows: the host's chains; from eight generic problems on the eight-lane host chains where the CPU has them, else
    from 32 problems on the device"""
    if fixed_base or np_ < 8:
        return "host"
    if host8:
        return "host8"
    return "device" if np_ >= 32 else "host"
