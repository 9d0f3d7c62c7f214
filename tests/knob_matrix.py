"""The knob matrix: every ROFL_* variable of the registry (csrc/host_rt.hpp, KNOBS.md) classified, and the cases that hold the
path-selecting ones to KNOBS.md's promise -- "proofs, commitments and verdicts are the same for every setting".

Plain data and helpers, no fixtures.  tests/test_knob_matrix_host.py checks that no knob escapes the classification and that every
path / resource knob (every accepted value of an enumeration) has a case; tests/test_gpu_knob_matrix.py runs each case in a fresh
process (tests/gpu_knob_check.py: knobs are read once per process) and compares every workload bit for bit with the CPU oracle.

A case is (id, environment, workloads, witnesses).  A witness shows that the case's path RAN -- a knob that is clamped, ignored or not
reached at these sizes must fail, not pass vacuously.  Witness forms, all over the child's ROFL_TRACE=1 lines ("[rofl] <kind> k=v ..."):
    ("some", kind, {field: want, ...})    at least one line of that kind matches every field
    ("none", kind, {field: want, ...})    no line of that kind matches every field ({} = no such line at all)
    ("count", name, want)                 a "WITNESS <name> <int>" line of the helper
A fourth element of a "some" / "none" witness names a section: only the lines after the helper's own "[knob-check] <section>" mark and before
its next mark count (which call of the process the line belongs to).
`want` is a literal, ">N" / "<N" against the field's integer value, or "!=X" (as integers when X is one, as strings otherwise).  A want that
starts with another operator sign raises: a misspelt comparison must not turn into a literal that never matches."""
import hashlib
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rofl_project_code_amd", "csrc")

# ---------------------------------------------------------------- classification
# path: selects a kernel, launch geometry, table layout or host SIMD path -> a matrix case at a non-default value (enumerations: every value)
PATH = [
    "ROFL_HOST_THREADS", "ROFL_POOL_SPIN_US", "ROFL_GENS_LAZY", "ROFL_GENS_LAZY_IDLE_MS", "ROFL_GENS_LAZY_MAX_WAIT_MS",
    "ROFL_FOLD_T1", "ROFL_FOLD_T", "ROFL_FOLD_MIN", "ROFL_MSM_BIN_SIGMA", "ROFL_FOLD_TAB", "ROFL_FOLD_PB", "ROFL_FOLD_W", "ROFL_FOLD_TAB_MB",
    "ROFL_FOLD_K", "ROFL_FOLD_THREADS", "ROFL_MSM_FB", "ROFL_MSM_FB_MIN", "ROFL_MSM_FB_C", "ROFL_MSM_FB_THREADS", "ROFL_MSM_TWO_LEVEL",
    "ROFL_MSM_SLOTS", "ROFL_MSM_LDS", "ROFL_MSM_LDS_MIN", "ROFL_MSM_LDS_TILE", "ROFL_MSM_SMALL_MAX", "ROFL_MSM_SMALL_GROUP", "ROFL_MERLIN_X8",
    "ROFL_MSM_HOST8", "ROFL_MSM_HOST8_MIN", "ROFL_MSM_FB_HOST8_MIN", "ROFL_KECCAK_ZMM", "ROFL_MSM_DEV_HORNER_MIN", "ROFL_MSM_T13", "ROFL_MSM_T10",
    "ROFL_MSM_C", "ROFL_RED_FUSED_T", "ROFL_ACC_BALANCE",
]
# option: the environment default of an ABI behaviour option (rofl_set_option) -> the existing test that covers the option
OPTION = {
    "ROFL_DEVICES": "tests/test_gpu_multidevice.py::test_batch_calls_shard_over_the_listed_devices",
    "ROFL_BLOCKING_SYNC": "tests/test_host_lib.py::test_options_are_process_wide_and_checked",
    "ROFL_VERIFY_ZIP_TRUNCATE": "tests/test_gpu_hardening.py::test_behaviour_options_are_abi_calls",
    "ROFL_VERIFY_BATCH": "tests/test_gpu_hardening.py::test_behaviour_options_are_abi_calls",
    "ROFL_SIGMA_BATCH": "tests/test_gpu_l2_batch.py::test_sigma_batches_of_the_other_kinds_and_options",
}
# resource: memory or scheduling only -> still one case at a small value (it can change which table serves a call)
RESOURCE = ["ROFL_LANES", "ROFL_STAGE_KEEP_MB", "ROFL_GENS_RESERVE_MB", "ROFL_GENS_BUDGET_MB"]
# inert: cannot reach a result
INERT = {
    "ROFL_DEVICE_MAP": "which physical GPU a logical device is; tests/test_gpu_multidevice.py runs under it",
    "ROFL_RCCL_LIB": "the file name rofl_comm_* hands to dlopen",
    "ROFL_TRACE": "stderr lines only; every matrix case runs under ROFL_TRACE=1 and reads them",
    "ROFL_DBG_SMALL_TIMELINE": "debugging: clock stamps of the fused small launch on stderr (synchronises)",
    "ROFL_DBG_ACC_TIMELINE": "debugging: per-wave records of the accumulate launch appended to a file",
    "ROFL_FEMUL_LDS": "rofl_bench_femul micro-benchmark only",
    "ROFL_FEMUL_MODE": "rofl_bench_femul micro-benchmark only",
    "ROFL_FEMUL_TABLE": "rofl_bench_femul micro-benchmark only",
}


def classification():
    """{knob: class}; a name listed twice raises"""
    out = {}
    for cls, names in (("path", PATH), ("option", OPTION), ("resource", RESOURCE), ("inert", INERT)):
        for n in names:
            if n in out:
                raise ValueError("%s is classified twice" % n)
            out[n] = cls
    return out


# enumeration knobs: the non-default values the source accepts (test_knob_matrix_host.py reads them back from the `if (v == ...)` lines)
ENUMS = {
    "ROFL_MSM_C": ("host_msm.hpp", [4, 7, 10, 13, 16]),
    "ROFL_MSM_FB_C": ("host_rt.hpp", [13, 15, 16]),
    "ROFL_FOLD_K": ("host_rt.hpp", [1, 2, 4]),
    "ROFL_FOLD_PB": ("host_rt.hpp", [16, 64]),              # (32 is the default)
    "ROFL_MSM_SMALL_GROUP": ("host_msm.hpp", [1, 2]),       # (clamped to 1..4, 3 runs as 2; 4 is the default and has a case of its own)
}
ENUM_DEFAULTS = {"ROFL_FOLD_PB": 32, "ROFL_MSM_SMALL_GROUP": 4}


def accepted_in_source(knob):
    """the values the source accepts for an enumeration knob: the `v == a || v == b ...` (or `force == ...`) chain next to its knob() read;
    ROFL_MSM_SMALL_GROUP is a clamp: the bounds of its std::max / std::min pair"""
    src = open(os.path.join(CSRC, ENUMS[knob][0])).read()
    line = [l for l in src.splitlines() if 'knob("%s")' % knob in l]
    assert len(line) == 1, (knob, len(line))
    line = line[0]
    if knob == "ROFL_MSM_SMALL_GROUP":
        m = re.search(r"std::max\((\d+), std::min\((\d+), atoi", line)
        lo, hi = int(m.group(1)), int(m.group(2))
        return list(range(lo, hi + 1))
    if knob == "ROFL_MSM_FB_C":      # the knob is read into `force`; the accepted values are in the return below it
        line = src[src.index(line):].split("return", 1)[1].split(";", 1)[0]
    vals = [int(x) for x in re.findall(r"(?:v|force) == (\d+)", line)]
    assert vals, (knob, line)
    return vals


# ---------------------------------------------------------------- workloads (inputs are functions of the workload alone; the oracle's bytes are computed once per session)
MSM_SIZES = (1, 63, 64, 300, 2000)
RANGE_SHAPES = ((3, 8, 2, 16, 7), (64, 8, 1, 16, 7), (500, 32, 4, 32, 7))            # (d, n_bits, P, fp_bits, fp_frac)
RANGE_WIDE = (256, 32, 1, 32, 7)       # one chunk of 8 192 generators a side: the smallest at which msm_plan_job allows the two-level sort
# The smallest (d, 8, P) whose IPP-tail launches have 64 buckets a window (c = 7) and more than 512 bucket arrays, found with the witness
# `kind=small c=7 group=4`: P = 8 gives 16 L / R problems of 37 windows = 592 arrays (P = 4: 296), and d = 64 makes them 64 generators a side
# = 128 terms, six launches of it (probed on the MI355X: (64, 8, 8), (128, 8, 8) and (64 / 128 / 256, 8, 16) all reach it; this is the least)
RANGE_MANY = (64, 8, 8, 16, 7)
RANGE_CHUNKS32 = (64, 8, 32, 16, 7)    # 32 chunks: where the verifier's SIMD transcript prefixes (eight chunks per stream) start
SIGMA_D = 70
# The fast start (compact fold table first, full table from a background thread) only exists for fold tables of 4 GB and more: 16 384
# generators a side at the default layout is the smallest shape that has it.  At (500, 32, 4) -- 4 096 a side, 1.6 GB -- neither
# ROFL_GENS_LAZY nor its two timers is ever read, so that shape is created three times as well, and this one carries the witness.
LAZY_SHAPES = ((500, 32, 4, 32, 7), (512, 32, 1, 32, 7))
LAZY_PAUSE_S = 0.75

RANGE_4GB = (512, 32, 1, 32, 7)        # the second lazy shape, created once
MSM_TILE_SIZE = 5000                   # with 64 windows (c = 4): the least round size at which ROFL_MSM_LDS_TILE=1024 decides the tile of the LDS slot sort
WORKLOADS = ("msm", "msm5000", "range", "range_wide", "range_many", "range_chunks32", "range_4gb", "sigma", "lazy")


def range_inputs(shape, salt=0):
    d, nb, P, fb, ff = shape
    rng = np.random.default_rng(1000003 * d + 1009 * nb + 31 * P + salt)
    mx = np.float32(((1 << (nb - 1)) - 1) / float(1 << ff))      # get_clip_bounds(nb), drawn from the half-open interval
    vals = np.clip(rng.uniform(-mx, mx, size=d).astype(np.float32), -mx, np.nextafter(mx, np.float32(0)))
    bl = rng.integers(0, 256, size=(d, 32), dtype=np.uint8); bl[:, 31] &= 0x0F
    seed = bytes(rng.integers(0, 256, 32, dtype=np.uint8))
    return vals, bl, seed


def msm_sizes(workload):
    return MSM_SIZES if workload == "msm" else (MSM_TILE_SIZE,)


def msm_inputs(n):
    """(points, {family: scalars}): the six scalar families of test_msm_extreme_scalars on n random points"""
    import orc
    rng = np.random.default_rng(n)
    pts = orc.commit_vec(orc.rand_scalars(rng, n), None)
    return pts, {k: np.ascontiguousarray(v) for k, v in orc.extreme_scalar_cases(rng, n).items()}


def sigma_inputs(kind):
    import orc
    rng = np.random.default_rng(4200 + kind)
    vals = rng.uniform(-100, 100, SIGMA_D).astype(np.float32)
    return vals, orc.rand_scalars(rng, SIGMA_D), orc.rand_scalars(rng, SIGMA_D), bytes(rng.integers(0, 256, 32, dtype=np.uint8))


def tamper(proofs):
    t = proofs.copy(); t[0, 40] ^= 1
    return t


class Digest:
    """RESULT <workload> <sha256> over the items in order; ITEM lines say which one differs"""
    def __init__(self, workload):
        self.workload, self.h, self.items = workload, hashlib.sha256(), []

    def add(self, name, *arrays):
        b = b"".join(bytes([int(a)]) if isinstance(a, (bool, int)) else np.ascontiguousarray(a).tobytes() for a in arrays)      # (a verdict is one byte)
        self.h.update(b)
        self.items.append((name, hashlib.sha256(b).hexdigest()[:16]))

    def lines(self):
        return ["ITEM %s/%s %s" % (self.workload, n, h) for n, h in self.items] + ["RESULT %s %s" % (self.workload, self.h.hexdigest())]


def _range_shapes(workload):
    return {"range": RANGE_SHAPES, "range_wide": (RANGE_WIDE,), "range_many": (RANGE_MANY,), "range_chunks32": (RANGE_CHUNKS32,), "range_4gb": (RANGE_4GB,), "lazy": LAZY_SHAPES}[workload]


def oracle_lines(workload):
    """what tests/gpu_knob_check.py must print for `workload`, from the CPU oracle alone"""
    import orc
    D = Digest(workload)
    if workload in ("msm", "msm5000"):
        for n in msm_sizes(workload):
            pts, fam = msm_inputs(n)
            for name, k in fam.items():
                D.add("n%d/%s" % (n, name), orc.msm(k, pts))
    elif workload == "sigma":
        for kind in (0, 1, 2):
            vals, r1, r2, seed = sigma_inputs(kind)
            rc, pr, cm = orc.sigma_create(kind, vals, r1, r2 if kind else None, 16, 7, seed=seed)
            assert rc == 0 and orc.sigma_verify(kind, pr, cm) == (0, True)
            D.add("kind%d/proofs" % kind, pr); D.add("kind%d/commits" % kind, cm); D.add("kind%d/verdict" % kind, True)
    else:
        for shape in _range_shapes(workload):
            d, nb, P, fb, ff = shape
            vals, bl, seed = range_inputs(shape)
            rc, pr, cm = orc.create_rangeproof(vals, bl, nb, P, fb, ff, seed=seed)
            assert rc == 0 and orc.verify_rangeproof(pr, cm, nb, fb, ff) == (0, True) and orc.verify_rangeproof(tamper(pr), cm, nb, fb, ff) == (0, False)
            tag = "%dx%dx%d" % (d, nb, P)
            for rep in range(3 if workload == "lazy" else 1):
                sfx = "#%d" % rep if workload == "lazy" else ""
                D.add(tag + "/proofs" + sfx, pr); D.add(tag + "/commits" + sfx, cm)
            D.add(tag + "/verdict", True); D.add(tag + "/tampered", False)
    return D.lines()


# ---------------------------------------------------------------- witnesses
def parse_trace(stderr):
    """[(kind, {field: value}, section)] of the "[rofl] <kind> k=v ..." lines; section = the helper's last "[knob-check] ..." mark before the line"""
    out, section = [], ""
    for l in stderr.splitlines():
        if l.startswith("[knob-check] "):
            section = l[len("[knob-check] "):].strip()
            continue
        m = re.match(r"\[rofl\] ([a-z0-9-]+) (.*)$", l)
        if m:
            out.append((m.group(1), dict(kv.split("=", 1) for kv in m.group(2).split() if "=" in kv), section))
    return out


def _holds(got, want):
    want = str(want)
    m = re.match(r"(>|<|!=)(.+)$", want)
    if not m:
        if re.match(r"[<>=!~]", want):
            raise ValueError("witness value %r: not a literal, >N, <N or !=X" % want)
        return got == want
    op, arg = m.groups()
    if re.fullmatch(r"-?\d+", arg):
        try:
            g = int(got)
        except (TypeError, ValueError):
            return op == "!="      # (a field that is no integer differs from every integer)
        return {">": g > int(arg), "<": g < int(arg), "!=": g != int(arg)}[op]
    if op != "!=":
        raise ValueError("witness value %r: %s needs an integer" % (want, op))
    return got != arg


def unmet(witnesses, stderr, stdout):
    """the witnesses of a case that the child's output does not bear out ([] = the case's paths ran)"""
    lines = parse_trace(stderr)
    counts = dict(l.split()[1:3] for l in stdout.splitlines() if l.startswith("WITNESS ") and len(l.split()) == 3)
    bad = []
    for w in witnesses:
        if w[0] == "count":
            ok = w[1] in counts and _holds(counts[w[1]], w[2])
        else:
            hit = any(k == w[1] and (len(w) < 4 or sec == w[3]) and all(f in fl and _holds(fl[f], v) for f, v in w[2].items()) for k, fl, sec in lines)
            ok = hit if w[0] == "some" else not hit
        if not ok:
            bad.append(w)
    return bad


# ---------------------------------------------------------------- the cases
# skip_unless: the library's own selftest that returns -1 on a CPU without the instruction set (the only permitted skips)
F16 = {"ROFL_FOLD_MIN": "16"}      # folds happen at these sizes
COMPACT = {"tab": "1", "pb": "64", "w": "4"}      # a first fold served by the compact fold table of the fast start
LAZY_FIRST, LAZY_LAST = "create 512x32x1 #0", "create 512x32x1 #2"


# unproved: knobs of the environment that the case's witnesses do NOT speak for (presence in an environment is not coverage:
# test_knob_matrix_host.py wants every path / resource knob among some case's proved ones, or in UNWITNESSED with its reason)
def _c(id, env, workloads, witnesses, skip_unless=None, unproved=()):
    assert not set(unproved) - set(env), id
    return {"id": id, "env": env, "workloads": tuple(workloads), "witnesses": witnesses, "skip_unless": skip_unless, "proves": tuple(k for k in env if k not in unproved)}


UNWITNESSED = {
    "ROFL_STAGE_KEEP_MB": "whether a lane's pinned arena was trimmed after a call leaves no mark in the trace; the case still runs under 1 MB",
}


CASES = [
    # -- generic window width (chosen scalars reach every width: c = 4 has 64 windows, c = 16 the split top window at 2^252 and above) x fold segments
    _c("c4-foldk1", dict(F16, ROFL_MSM_C="4", ROFL_FOLD_K="1"), ("msm", "range"),
       [("some", "msm", {"n": "2000", "c": "4", "kind": "slots"}), ("some", "msm", {"c": "4", "kind": "small"}), ("some", "fold", {"K": "1"}), ("none", "fold", {"K": "!=1"})]),
    _c("c7-foldk2", dict(F16, ROFL_MSM_C="7", ROFL_FOLD_K="2"), ("msm", "range"),
       [("some", "msm", {"n": "2000", "c": "7"}), ("some", "msm", {"n": "1", "c": "7"}), ("none", "msm", {"kind": "!=fb", "c": "!=7"}), ("some", "fold", {"K": "2"}), ("none", "fold", {"K": "!=2"})]),
    _c("c10-foldk4", dict(F16, ROFL_MSM_C="10", ROFL_FOLD_K="4", ROFL_FOLD_THREADS="1"), ("msm", "range"),
       [("some", "msm", {"n": "63", "c": "10"}), ("some", "fold", {"K": "4"}), ("none", "fold", {"K": "!=4"})]),
    _c("c13-fold-threads1", dict(F16, ROFL_MSM_C="13", ROFL_MSM_SMALL_MAX="0", ROFL_FOLD_THREADS="1"), ("msm", "range"),
       [("some", "msm", {"n": "2000", "c": "13", "kind": "slots"}), ("some", "msm", {"n": "1", "c": "13"}), ("some", "fold", {"K": "1"}), ("none", "fold", {"K": "!=1"})]),
    _c("c16-fold-threads-huge", dict(F16, ROFL_MSM_C="16", ROFL_MSM_SMALL_MAX="0", ROFL_FOLD_THREADS="1000000000"), ("msm", "range"),
       [("some", "msm", {"n": "2000", "c": "16", "kind": "slots"}), ("some", "msm", {"n": "1", "c": "16"}), ("some", "fold", {"K": "4"}), ("none", "fold", {"K": "!=4"})]),
    # -- size thresholds of the window width x fold table layouts
    _c("t10-foldtab0", dict(F16, ROFL_MSM_T10="64", ROFL_FOLD_TAB="0"), ("msm", "range"),
       [("some", "msm", {"n": "64", "c": "10", "kind": "small"}), ("some", "msm", {"n": "63", "c": "4"}), ("some", "fold", {"tab": "0"}), ("none", "fold", {"tab": "1"})]),
    _c("t13-foldpb64", dict(F16, ROFL_MSM_T13="256", ROFL_MSM_SMALL_MAX="0", ROFL_FOLD_PB="64"), ("msm", "range"),
       [("some", "msm", {"n": "300", "c": "13"}), ("some", "msm", {"n": "64", "c": "7"}), ("some", "fold", {"tab": "1", "pb": "64"})]),
    # (the LDS slot sort first halves its tile until the launch has 256 blocks; only then is the knob looked at.  5 000 terms at c = 4 -- 64 windows --
    #  stop at 1 250 a tile without the knob and at 625 with ROFL_MSM_LDS_TILE=1024; at n = 2 000 and below that rule alone decides)
    _c("lds-tile-foldpb16", dict(F16, ROFL_MSM_LDS_TILE="1024", ROFL_MSM_LDS_MIN="32", ROFL_MSM_SMALL_MAX="0", ROFL_MSM_C="4", ROFL_FOLD_PB="16", ROFL_FOLD_W="5"), ("msm5000", "msm", "range"),
       [("some", "msm", {"n": "5000", "c": "4", "kind": "slots", "tile": "625"}), ("none", "msm", {"n": "5000", "tile": "!=625"}), ("some", "msm", {"n": "64", "tile": "64"}),
        ("some", "fold", {"tab": "1", "pb": "16", "w": "5"})]),
    _c("redfused64-foldtabmb1", dict(F16, ROFL_RED_FUSED_T="64", ROFL_MSM_SMALL_MAX="0", ROFL_FOLD_TAB_MB="1"), ("msm", "range"),
       [("some", "msm", {"n": "2000", "c": "10", "fused_t": "64"}), ("none", "msm", {"fused_t": ">64"}), ("some", "fold", {"tab": "1", "w": "6"}), ("none", "fold", {"tab": "1", "w": ">6"})]),
    _c("redfused0-clamped", {"ROFL_RED_FUSED_T": "0", "ROFL_MSM_SMALL_MAX": "0"}, ("msm",),      # (raised to one wave where the knob is read: a launch without threads otherwise)
       [("some", "msm", {"n": "2000", "kind": "slots", "fused_t": "64"}), ("none", "msm", {"kind": "slots", "fused_t": "!=64"})]),
    _c("redfused256-foldt", dict(F16, ROFL_RED_FUSED_T="256", ROFL_MSM_SMALL_MAX="0", ROFL_MSM_FB_MIN="64", ROFL_FOLD_T="1", ROFL_FOLD_T1="2"), ("msm", "range"),
       [("some", "msm", {"kind": "fb", "fused_t": "256"}), ("none", "msm", {"fused_t": ">256"}), ("some", "fold", {"nsrc": "4", "tab": "1"}), ("some", "fold", {"nsrc": "2", "tab": "0"})]),
    # -- fixed-base window tables
    _c("fbc13", {"ROFL_MSM_FB_C": "13", "ROFL_MSM_FB_MIN": "64"}, ("range",),
       [("some", "msm", {"kind": "fb", "c": "13", "fb": ">0"}), ("none", "msm", {"kind": "fb", "c": "!=13"})]),
    _c("fbc15-two-level", {"ROFL_MSM_FB_C": "15", "ROFL_MSM_FB_MIN": "64"}, ("range", "range_wide"),
       [("some", "msm", {"kind": "fb", "c": "15", "fb": ">0", "two": "1"}), ("some", "msm", {"kind": "fb", "c": "15", "two": "0"}), ("none", "msm", {"kind": "fb", "c": "!=15"})]),
    _c("fbc16-two-level", {"ROFL_MSM_FB_C": "16", "ROFL_MSM_FB_MIN": "64"}, ("range", "range_wide"),
       [("some", "msm", {"kind": "fb", "c": "16", "fb": ">0", "two": "1"}), ("some", "msm", {"kind": "fb", "c": "16", "two": "0"}), ("none", "msm", {"kind": "fb", "c": "!=16"})]),
    _c("fb-threads-one-set", {"ROFL_MSM_FB_THREADS": "32768"}, ("range_wide",),
       [("some", "msm", {"kind": "fb", "c": "16", "fb": "1", "two": "1"}), ("none", "msm", {"kind": "fb", "c": "16", "fb": ">1"})]),      # (the verifier's 15-bit table has 17 windows: one set or seventeen)
    # (the L / R launches of the first rounds: 8 192 terms a side, eight sets of two windows over 256 bins = 64 a bin, twice that in the hot half:
    #  msm_bin_cap gives 128 + 256 -> 384 entries with the fixed margin, 128 + 8 x 12 + 64 -> 320 with eight standard deviations)
    _c("bin-sigma0", {"ROFL_MSM_BIN_SIGMA": "0"}, ("range_wide",),
       [("some", "msm", {"kind": "fb", "two": "1", "np": "2", "fb": "8", "bin": "BIN_SIGMA0"}), ("none", "msm", {"two": "1", "np": "2", "fb": "8", "bin": "BIN_DEFAULT"})]),
    _c("two-level0-accbalance0", {"ROFL_MSM_TWO_LEVEL": "0", "ROFL_ACC_BALANCE": "0"}, ("range_wide",),
       [("some", "msm", {"kind": "fb", "two": "0", "tile": ">0", "n": "16384", "bal": "0"}), ("none", "msm", {"two": "1"}), ("none", "msm", {"bal": "!=0"})]),
    _c("fb0-lds0-small0", {"ROFL_MSM_FB": "0", "ROFL_MSM_LDS": "0", "ROFL_MSM_SMALL_MAX": "0"}, ("range", "range_wide"),
       [("some", "msm", {"kind": "slots", "n": "16384"}), ("none", "msm", {"kind": "!=slots"}), ("none", "msm", {"tile": ">0"})]),
    _c("slots0", {"ROFL_MSM_SLOTS": "0"}, ("msm", "range"),
       [("none", "msm", {}), ("count", "msm.msms_done", ">0"), ("count", "range.msms_done", ">0")]),
    # -- the fused small launch with more than 512 bucket arrays of 64 buckets
    _c("small-group1", {"ROFL_MSM_SMALL_GROUP": "1"}, ("range_many",), [("some", "msm", {"kind": "small", "c": "7", "group": "1", "np": "16"}), ("none", "msm", {"group": ">1"})]),
    _c("small-group2", {"ROFL_MSM_SMALL_GROUP": "2"}, ("range_many",), [("some", "msm", {"kind": "small", "c": "7", "group": "2", "np": "16"}), ("none", "msm", {"group": ">2"})]),
    _c("small-group4", {"ROFL_MSM_SMALL_GROUP": "4"}, ("range_many",), [("some", "msm", {"kind": "small", "c": "7", "group": "4", "np": "16"})]),
    # -- where the window chains of a launch with many problems run
    _c("host8-off-dev-horner", {"ROFL_MSM_HOST8": "0", "ROFL_MSM_DEV_HORNER_MIN": "1"}, ("range", "range_many"),
       [("some", "msm", {"horner": "dev", "kind": "small"}), ("none", "msm", {"horner": "host8"}), ("some", "msm-finish", {"finish": "dev"})], "horner8"),
    _c("host8-min2", {"ROFL_MSM_HOST8_MIN": "2"}, ("range",),
       [("some", "msm", {"horner": "host8", "np": "4"}), ("some", "msm-finish", {"finish": "host8", "np": "4"})], "horner8"),
    _c("host8-min-high", {"ROFL_MSM_HOST8_MIN": "1000"}, ("range", "range_many"),
       [("some", "msm", {"horner": "host", "np": "16", "kind": "small"}), ("none", "msm", {"horner": "host8"}), ("none", "msm-finish", {"finish": "host8"})], "horner8"),
    # (a lower ROFL_MSM_FB_HOST8_MIN changes nothing at these shapes: the fixed-base launches below eight problems carry no eight-wide finisher, or
    #  eight sets of sixteen bit-sums -- more than the 64 a stream takes; the higher value sends the eight L / R problems of four chunks down the scalar chains)
    _c("fb-host8-min-high", {"ROFL_MSM_FB_HOST8_MIN": "1000", "ROFL_MSM_FB_MIN": "64"}, ("range", "range_many"),
       [("some", "msm-finish", {"finish": "fb", "np": "8"}), ("some", "msm-finish", {"finish": "fb", "np": "16"}), ("none", "msm-finish", {"finish": "fb8"})], "horner8"),
    _c("merlin-x8-off", {"ROFL_MERLIN_X8": "0"}, ("range_chunks32",),
       [("some", "verify-hash", {"chunks": "32", "per": "1"}), ("none", "verify-hash", {"per": "8"})], "merlin8"),
    # -- host side of the Sigma-proofs and of every transcript
    _c("sigma-batch0", {"ROFL_SIGMA_BATCH": "0"}, ("sigma",), [("count", "option.sigma_batch", "0"), ("count", "sigma.verify_msms", "0")]),
    _c("keccak-scalar-one-thread", {"ROFL_KECCAK_ZMM": "0", "ROFL_HOST_THREADS": "1", "ROFL_POOL_SPIN_US": "0", "ROFL_BLOCKING_SYNC": "1"}, ("sigma", "range"),
       [("some", "host", {"threads": "1", "spin_us": "0", "keccak_zmm": "0"}), ("count", "option.blocking_sync", "1"), ("count", "sigma.verify_msms", ">0")]),
    _c("keccak-zmm", {"ROFL_KECCAK_ZMM": "1"}, ("sigma", "range"), [("some", "host", {"keccak_zmm": "1"})], "merlin8"),
    # -- fast start of the fold table
    _c("lazy-off", {"ROFL_GENS_LAZY": "0"}, ("lazy",),
       [("some", "fold", {"tab": "1"}, LAZY_FIRST), ("none", "fold", COMPACT, LAZY_FIRST), ("some", "fold", {"tab": "1"}, LAZY_LAST), ("none", "fold", COMPACT, LAZY_LAST)]),
    _c("lazy-quick-upgrade", {"ROFL_GENS_LAZY_IDLE_MS": "1", "ROFL_GENS_LAZY_MAX_WAIT_MS": "50"}, ("lazy",),
       [("some", "fold", COMPACT, LAZY_FIRST), ("some", "fold", {"tab": "1"}, LAZY_LAST), ("none", "fold", COMPACT, LAZY_LAST)]),
    # -- resources at small values: one lane, staging freed after every call, every new (n, m) evicts the previous tables, no big table may be allocated
    # (the reserve is more than the device has: the 6.4 GB fold table of 16 384 generators a side may not be allocated and is narrowed to width 9, 3.2 GB,
    #  which is below the size the reserve guards; ROFL_GENS_LAZY=0 so that the first create is not served by the compact table anyway)
    _c("resources-small", {"ROFL_LANES": "1", "ROFL_STAGE_KEEP_MB": "1", "ROFL_GENS_BUDGET_MB": "1", "ROFL_GENS_RESERVE_MB": "400000", "ROFL_GENS_LAZY": "0"}, ("range", "sigma", "range_4gb"),
       [("some", "host", {"lanes": "1"}), ("some", "gens-evict", {"keep_mb": "<2"}), ("some", "fold", {"tab": "1", "pb": "32", "w": "9"}, "create 512x32x1 #0"),
        ("none", "fold", {"tab": "1", "w": "10"}, "create 512x32x1 #0")], unproved=("ROFL_STAGE_KEEP_MB", "ROFL_GENS_LAZY")),
]
BIN_LITERALS = {"BIN_SIGMA0": "384", "BIN_DEFAULT": "320"}
for _case in CASES:
    _case["witnesses"] = [(w[0], w[1], {f: BIN_LITERALS.get(v, v) for f, v in w[2].items()}) + tuple(w[3:]) if w[0] != "count" else w for w in _case["witnesses"]]


def cases_by_id():
    ids = [c["id"] for c in CASES]
    assert len(set(ids)) == len(ids)
    return {c["id"]: c for c in CASES}


def covered_values():
    """{knob: set of the values it takes in some case}"""
    out = {}
    for c in CASES:
        for k, v in c["env"].items():
            out.setdefault(k, set()).add(v)
    return out
