"""ctypes binding of librofl_zk.so, shaped like the reference's Rust modules.

Reference signatures mirrored here (rofl_crypto/src/...):
  range_proof_vec/mod.rs:16-21   create_rangeproof(values, blindings, prove_range, n_partition)
  range_proof_vec/mod.rs:149-153 verify_rangeproof(proofs, commits, prove_range)
  l2_range_proof_vec/mod.rs:15-20, :185-189
  pedersen_ops.rs:9-127, conversion32.rs:11-66
Scalars / points are numpy uint8 arrays of shape (d, 32); proofs are (n_proofs, proof_len).
Errors that the reference reports as Err(..) (or panics) raise RoflError(code).
"""
import contextlib
import ctypes
import hashlib
import math
import os
import struct
import threading
from fractions import Fraction

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB_PATH = os.environ.get("ROFL_ZK_LIB") or os.path.join(_HERE, "librofl_zk.so")      # ROFL_ZK_LIB: another build of the same library (same-box A/B runs)

ERROR_NAMES = {
    1: "WrongNumBlindingFactors", 2: "ValueOutOfRangeError", 3: "InvalidBitsize", 4: "InvalidAggregation",
    5: "FormatError", 6: "InvalidGeneratorsLength", 7: "NormOutOfRangeError", 8: "OverflowError", 9: "SumError",
    10: "NonFiniteValue", 11: "BadParameter", 12: "NonceStreamTooShort",
}


class RoflError(Exception):
    def __init__(self, code, msg=""):
        self.code = code
        self.name = ERROR_NAMES.get(code, "HipError" if code >= 100 else "Unknown")
        super().__init__(f"{self.name} ({code}): {msg}")


class _NonceStruct(ctypes.Structure):
    _fields_ = [("mode", ctypes.c_int), ("stream", ctypes.c_void_p), ("stream_scalars", ctypes.c_size_t),
                ("seed", ctypes.c_ubyte * 32)]


class _BlindTerm(ctypes.Structure):
    """rofl_blind_term_t"""
    _fields_ = [("seed", ctypes.c_ubyte * 32), ("sign", ctypes.c_int32)]


class _DhPair(ctypes.Structure):
    """rofl_dh_pair_t"""
    _fields_ = [("own", ctypes.c_uint32), ("peer", ctypes.c_uint32)]


class _SigRef(ctypes.Structure):
    """rofl_sig_ref_t"""
    _fields_ = [("key", ctypes.c_uint32), ("msg", ctypes.c_uint32)]


class _MerkleRef(ctypes.Structure):
    """rofl_merkle_ref_t"""
    _fields_ = [("root", ctypes.c_uint32), ("index", ctypes.c_uint32)]


class _Timing(ctypes.Structure):
    _fields_ = [("total_ms", ctypes.c_double), ("msm_accumulate_ms", ctypes.c_double),
                ("msm_accumulate_launches", ctypes.c_uint64), ("msm_terms", ctypes.c_uint64),
                ("fold_ms", ctypes.c_double), ("fold_launches", ctypes.c_uint64),
                ("fold_point_reads", ctypes.c_uint64), ("host_ms", ctypes.c_double), ("msm_additions", ctypes.c_uint64)]


class Nonce:
    """Prover randomness (the reference uses rand::thread_rng inside bulletproofs).

    Nonce.seeded(seed32): deterministic SHAKE256 stream; Nonce.stream(bytes): explicit 64-byte wide scalars
    in the reference draw order; Nonce.random(): fresh OS randomness (what a deployment uses).  A stream with repeated blocks
    (equal nonces) is accepted and proved bit for bit like any other, only slower: the rounds' MSMs are repeated on slower variants."""

    def __init__(self, mode, seed=None, stream=None):
        self.mode, self.seed, self._stream = mode, seed, stream

    @staticmethod
    def seeded(seed32):
        seed32 = bytes(seed32)
        assert len(seed32) == 32
        return Nonce(1, seed=seed32)

    @staticmethod
    def random():
        return Nonce(1, seed=os.urandom(32))

    @staticmethod
    def stream(data):
        arr = np.ascontiguousarray(np.frombuffer(bytes(data), dtype=np.uint8))
        assert arr.size % 64 == 0
        return Nonce(0, stream=arr)

    def _struct(self):
        s = _NonceStruct()
        s.mode = self.mode
        if self.mode == 1:
            s.seed = (ctypes.c_ubyte * 32)(*self.seed)
        else:
            s.stream = self._stream.ctypes.data
            s.stream_scalars = self._stream.size // 64
        return s


_lib = None


def lib():
    """Load librofl_zk.so (no fallback: a missing library is a hard error)."""
    global _lib
    if _lib is None:
        if not os.path.exists(_LIB_PATH):
            raise RuntimeError(f"{_LIB_PATH} not found: build it with `python -m rofl_project_code_amd.build` "
                               "(hipcc --offload-arch=gfx950); there is no CPU fallback")
        _lib = ctypes.CDLL(_LIB_PATH)
        for name in ("rofl_next_pow2", "rofl_rangeproof_chunks", "rofl_rangeproof_size", "rofl_nonces_per_chunk", "rofl_wire_encoded_size", "rofl_dbg_merkle_tile_leaves"):
            getattr(_lib, name).restype = ctypes.c_size_t
    return _lib


def _check(rc):
    if rc != 0:
        buf = ctypes.create_string_buffer(512)
        lib().rofl_last_error(buf, ctypes.c_size_t(512))
        raise RoflError(rc, buf.value.decode(errors="replace"))


_sz = ctypes.c_size_t


def _u8(a, last=32):
    a = np.ascontiguousarray(np.asarray(a, dtype=np.uint8))
    if a.ndim == 1 and last and a.size % last == 0:
        a = a.reshape(-1, last)
    return a


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _is_dev(x):
    """a torch tensor living on the GPU (anything with data_ptr() and is_cuda): handed to the library as a device pointer"""
    return hasattr(x, "data_ptr") and getattr(x, "is_cuda", False)


def _dev_arg(x, elem_bytes, row=1):
    """(pointer, rows) of a contiguous device tensor holding rows of `row` elements of `elem_bytes` bytes"""
    if not x.is_contiguous() or x.element_size() != elem_bytes:
        raise ValueError("device inputs must be contiguous tensors of the expected element type")
    return ctypes.c_void_p(x.data_ptr()), x.numel() // row


def set_device(dev):
    """rofl_set_device: bind the CALLING THREAD to logical device `dev` and bring that device up.  Only the FIRST successful call of the
    process also makes `dev` the default of threads that never bind (set_option("default_device", d) moves it later); the containers of
    params.py run their legs on pool threads bound to the device of the thread that called them."""
    _check(lib().rofl_set_device(int(dev)))


def get_device():
    out = ctypes.c_int()
    _check(lib().rofl_get_device(ctypes.byref(out)))
    return out.value


def map_device(logical, physical):
    """test hook (include/rofl_zk_debug.h): logical device -> HIP device, before the logical device is first used"""
    _check(lib().rofl_dbg_map_device(int(logical), int(physical)))


def bind_device(dev):
    """rofl_bind_device: the thread-binding half of set_device without touching HIP (-1 = back to the process default) -- for pool workers
    that run calls on behalf of a thread whose device is already up"""
    _check(lib().rofl_bind_device(int(dev)))


def bp_gens_table_bytes(n_bits, m):
    """HBM bytes of the cached tables of (n_bits, m) (0 if not built)."""
    out = _sz()
    _check(lib().rofl_bp_gens_table_bytes(_sz(n_bits), _sz(m), ctypes.byref(out)))
    return out.value


def bp_gens_prepare(n_bits, m):
    """Build (or touch) the cached BulletproofGens::new(n, m) tables on the device -- the reference recomputes them in every
    create / verify call (range_proof_vec/mod.rs:126,201)."""
    _check(lib().rofl_bp_gens_prepare(_sz(n_bits), _sz(m)))


def bp_gens_prepare_verify(n_bits, m):
    """rofl_bp_gens_prepare_verify: the tables a VERIFIER of (n_bits, m) reads -- generators and window slices, no fold table (a server's
    start-up call; the verify entry points build the same on first use)."""
    _check(lib().rofl_bp_gens_prepare_verify(_sz(n_bits), _sz(m)))


def set_option(key, value):
    """rofl_set_option: process-wide behaviour switches of the library (include/rofl_zk.h): "verify_zip_truncate", "verify_batch"
    (0 per proof, 1 per client, 2 per batch with a closer look on failure), "sigma_batch", "blocking_sync", "devices" (bit mask of the
    logical devices the batch entry points spread their clients over).  The ROFL_* environment variables of the same names only
    provide the defaults."""
    _check(lib().rofl_set_option(str(key).encode(), ctypes.c_long(int(value))))


def get_option(key):
    out = ctypes.c_long()
    _check(lib().rofl_get_option(str(key).encode(), ctypes.byref(out)))
    return out.value


class comm:
    """rofl_comm_*: the exchange steps of a round between the ranks of a node (one process per GPU) through the library's own RCCL
    communicator -- on the HIP runtime the library is bound to, no torch in the data path.  Payloads are host memory."""

    @staticmethod
    def unique_id():
        out = (ctypes.c_uint8 * 128)()
        _check(lib().rofl_comm_unique_id(out))
        return bytes(out)

    @staticmethod
    def init(uid, rank, world):
        uid = bytes(uid)
        assert len(uid) == 128
        _check(lib().rofl_comm_init((ctypes.c_uint8 * 128).from_buffer_copy(uid), int(rank), int(world)))

    @staticmethod
    def info():
        r, w, v = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        buf = ctypes.create_string_buffer(1024)
        _check(lib().rofl_comm_info(ctypes.byref(r), ctypes.byref(w), ctypes.byref(v), buf, _sz(1024)))
        return {"rank": r.value, "world": w.value, "rccl_version": v.value, "library": buf.value.decode(errors="replace")}

    @staticmethod
    def allgather(local_u8, world):
        a = np.ascontiguousarray(local_u8, dtype=np.uint8).reshape(-1)
        out = np.empty((int(world), a.size), dtype=np.uint8)
        _check(lib().rofl_comm_allgather(_ptr(a), _sz(a.size), _ptr(out)))
        return out

    @staticmethod
    def allreduce(values, op="sum"):
        a = np.ascontiguousarray(values, dtype=np.float64).reshape(-1).copy()
        _check(lib().rofl_comm_allreduce_f64(_ptr(a), _sz(a.size), {"sum": 0, "min": 1, "max": 2}[op]))
        return a

    @staticmethod
    def barrier():
        _check(lib().rofl_comm_barrier())

    @staticmethod
    def destroy():
        _check(lib().rofl_comm_destroy())


def msm_retries():
    """test hook (include/rofl_zk_debug.h): process-wide counters of the MSM driver --
    {"done", "small_overflow", "bin_overflow_to_slots", "slot_overflow"}"""
    out = (ctypes.c_uint64 * 4)()
    _check(lib().rofl_dbg_msm_retries(out))
    return dict(zip(("done", "small_overflow", "bin_overflow_to_slots", "slot_overflow"), (int(x) for x in out)))


class _MsmAttempt(ctypes.Structure):
    _fields_ = [(f, ctypes.c_uint32) for f in ("kind", "two", "c", "W", "cap", "cap_bin", "sets", "small_group", "finisher", "overflow", "repeated")]


MSM_KINDS = ("fixed_base", "small", "slots", "count_sort")
MSM_FINISHERS = ("host", "device", "host8")


def _attempt_dict(a):
    d = {f[0]: int(getattr(a, f[0])) for f in _MsmAttempt._fields_}
    d["kind"], d["finisher"], d["two"], d["repeated"] = MSM_KINDS[d["kind"]], MSM_FINISHERS[d["finisher"]], bool(d["two"]), bool(d["repeated"])
    return d


def msm_trace():
    """test hook (include/rofl_zk_debug.h): the attempts of the calling thread's last MSM, first to last, one dict per attempt --
    kind (MSM_KINDS), two, c, W, cap, cap_bin, sets, small_group, finisher (MSM_FINISHERS), overflow (the raw word), repeated"""
    buf = (_MsmAttempt * 8)()
    cnt = ctypes.c_size_t()
    _check(lib().rofl_dbg_msm_trace(buf, _sz(8), ctypes.byref(cnt)))
    return [_attempt_dict(a) for a in buf[:min(cnt.value, 8)]]


class _MsmRun(ctypes.Structure):
    """rofl_msm_run_t"""
    _fields_ = [(f, ctypes.c_uint32) for f in ("tag", "np", "n", "lr", "n_attempts")] + [("attempts", _MsmAttempt * 8)]


def msm_trace_begin():
    """test hook (include/rofl_zk_debug.h): empty the calling thread's store of MSM runs and switch it on"""
    _check(lib().rofl_dbg_msm_trace_begin())


def msm_trace_all(max_runs=1024):
    """test hook (include/rofl_zk_debug.h): every msm_run of the calling thread since msm_trace_begin(), oldest first, one dict per run --
    tag (99 = the S commitment, 100 + r = inner-product round r), np, n, lr (the L/R-merged mode), attempts (as msm_trace gives them)"""
    buf = (_MsmRun * max_runs)()
    cnt = ctypes.c_size_t()
    _check(lib().rofl_dbg_msm_trace_all(buf, _sz(max_runs), ctypes.byref(cnt)))
    return [{"tag": int(r.tag), "np": int(r.np), "n": int(r.n), "lr": bool(r.lr), "attempts": [_attempt_dict(a) for a in r.attempts[:min(int(r.n_attempts), 8)]]}
            for r in buf[:min(cnt.value, max_runs, 1024)]]


def dbg_msm_many(scalars32, points32):
    """test hook: out[p] = sum_i scalars32[p][i] * points32[i] for the np problems of scalars32 [np][n][32], in ONE launch chain"""
    k = np.ascontiguousarray(scalars32, dtype=np.uint8)
    p = np.ascontiguousarray(points32, dtype=np.uint8).reshape(-1, 32)
    if k.ndim != 3 or k.shape[2] != 32 or k.shape[1] != p.shape[0]:
        raise ValueError("scalars32 must be [np][n][32] over n points")
    out = np.zeros((k.shape[0], 32), dtype=np.uint8)
    _check(lib().rofl_dbg_msm_many(_sz(k.shape[0]), _sz(k.shape[1]), _ptr(k), _ptr(p), _ptr(out)))
    return out


def dbg_msm_fixed(n_bits, m, scalars32):
    """test hook: out[p] = sum_k s[p][k] G_k + sum_k s[p][N + k] H_k over the Bulletproofs generators of (n_bits, m), scalars32 [np][2 N][32],
    through the fixed-base variants of the MSM driver (the shape's window table)"""
    k = np.ascontiguousarray(scalars32, dtype=np.uint8)
    if k.ndim != 3 or k.shape[2] != 32 or k.shape[1] != 2 * n_bits * m:
        raise ValueError("scalars32 must be [np][2 n_bits m][32]")
    out = np.zeros((k.shape[0], 32), dtype=np.uint8)
    _check(lib().rofl_dbg_msm_fixed(_sz(n_bits), _sz(m), _sz(k.shape[0]), _ptr(k), _ptr(out)))
    return out


def dbg_encode_reps(site, xyzt):
    """test hook (include/rofl_zk_debug.h): the encoder and the identity predicate of `site` (0 device, 1 fe26 on the host, 2 fe32, 3 h51,
    4 h8::encode8 in batches of eight) on the n representatives xyzt [n][4][32] (X, Y, Z, T canonical) -> (encodings u8[n, 32],
    is_identity u8[n]), or None where site 4 has no AVX-512 IFMA to run on"""
    p = np.ascontiguousarray(xyzt, dtype=np.uint8).reshape(-1, 128)
    out = np.zeros((p.shape[0], 32), dtype=np.uint8)
    ident = np.full(p.shape[0], 0xFF, dtype=np.uint8)
    rc = lib().rofl_dbg_encode_reps(ctypes.c_uint(int(site)), _sz(p.shape[0]), _ptr(p), _ptr(out), _ptr(ident))
    if rc == -1:
        return None
    _check(rc)
    return out, ident


def set_timing(on):
    """0 / False = off, 1 / True = every instrumented launch, 2 = only the fixed-base accumulation (cheap enough for timed steps)"""
    _check(lib().rofl_set_timing(int(on)))


def last_timing():
    t = _Timing()
    _check(lib().rofl_last_timing(ctypes.byref(t)))
    return {f[0]: getattr(t, f[0]) for f in _Timing._fields_}


class _KernelTime(ctypes.Structure):
    _fields_ = [("ms", ctypes.c_double), ("launches", ctypes.c_uint64), ("fe_muls", ctypes.c_uint64), ("bytes", ctypes.c_uint64)]


KERNEL_KINDS = ("k_msm_accumulate_fb", "k_msm_accumulate_gen", "k_msm_bin_l1+l2 / k_msm_scatter_lds", "k_msm_reduce_level+fused", "k_msm_small",
                "k_fold_gens_tab", "k_fold_gens", "other", "k_sigma_prove / k_sigma_vprep / k_sigma_verify", "k_verify_scalars", "k_decode / k_commit")


def last_kernel_times():
    """{kernel kind: {ms, launches, fe_muls, bytes}} of the calling thread's last instrumented call (rofl_last_kernel_times)."""
    arr = (_KernelTime * len(KERNEL_KINDS))()
    _check(lib().rofl_last_kernel_times(arr))
    return {k: {"ms": arr[i].ms, "launches": arr[i].launches, "fe_muls": arr[i].fe_muls, "bytes": arr[i].bytes} for i, k in enumerate(KERNEL_KINDS)}


def bench_femul(iters=2000):
    out = ctypes.c_double()
    _check(lib().rofl_bench_femul(ctypes.c_uint(iters), ctypes.byref(out)))
    return out.value


class _FpDefault(threading.local):
    """Per-thread default of the reference's cargo features (N_BITS, frac) (fp.rs:8-139).  Every function that depends on
    them takes an explicit `fp=(fp_bits, fp_frac)` argument; `set_fp` only sets the calling thread's default for calls that
    omit it (threads start at the reference's default feature set fp16 / frac7), so concurrent callers never share state."""
    fp_bits = 16
    fp_frac = 7


_fp_default = _FpDefault()


def set_fp(fp_bits, fp_frac):
    """Default (fp_bits, fp_frac) of the CALLING THREAD for calls without an explicit fp= argument."""
    _fp_default.fp_bits, _fp_default.fp_frac = int(fp_bits), int(fp_frac)


def get_fp():
    return _fp_default.fp_bits, _fp_default.fp_frac


def _fp(fp):
    if fp is None:
        return _fp_default.fp_bits, _fp_default.fp_frac
    b, f = fp
    return int(b), int(f)


def _float_vecs(list_of_values, out, call, out_len=None):
    """what rofl_quantize_prob, rofl_noise_binomial, rofl_clip_l2 and rofl_rotate share: n float32 vectors of one length d in, n float32
    destinations out, each in host or device memory, checked and marshalled; call(n, values, d, out) -> return code.  out_len(d) -> the
    length of a destination where it is not d (rofl_rotate).  -> one (n, out_len) array for out=None, else the list of the destinations."""
    n = len(list_of_values)
    keep, vp, d = [], (ctypes.c_void_p * max(n, 1))(), None
    for v, x in enumerate(list_of_values):
        if _is_dev(x):
            p, dv = _dev_arg(x, 4)
            p = p.value
        else:
            x = np.ascontiguousarray(x, dtype=np.float32).reshape(-1)
            p, dv = x.ctypes.data, x.size
        keep.append(x)
        if d is not None and dv != d:
            raise ValueError("the vectors of one call have one length")
        d, vp[v] = dv, p
    d = d or 0
    do = d if out_len is None else out_len(d)
    if out is None:
        res = np.empty((n, do), dtype=np.float32)
        dst = [res[v] for v in range(n)]
    else:
        res = dst = list(out)
        if len(dst) != n:
            raise ValueError("one destination per vector")
    op = (ctypes.c_void_p * max(n, 1))()
    for v, o in enumerate(dst):
        if _is_dev(o):
            if not o.is_contiguous() or o.element_size() != 4 or o.numel() != do:
                raise ValueError("a device destination is a contiguous float32 tensor of %d elements" % do)
            op[v] = o.data_ptr()
        else:
            if not (isinstance(o, np.ndarray) and o.dtype == np.float32 and o.flags.c_contiguous and o.flags.writeable and o.size == do):
                raise ValueError("a host destination is a writable contiguous float32 array of %d elements" % do)
            op[v] = o.ctypes.data
    _check(call(_sz(n), vp, _sz(d), op))
    return res


@contextlib.contextmanager
def _seed_buffer(seeds, n):
    """one 32-byte seed per vector as the buffer a call reads them from, zeroed when the block is left; seeds=None -> None (a null pointer)"""
    if seeds is None:
        yield None
        return
    seeds = [bytes(s) for s in seeds]
    if len(seeds) != n:
        raise ValueError("one seed per vector")
    if any(len(s) != 32 for s in seeds):
        raise ValueError("a seed is 32 bytes")
    sb = ctypes.create_string_buffer(b"".join(seeds), max(32 * n, 1))
    try:
        yield sb
    finally:
        ctypes.memset(sb, 0, ctypes.sizeof(sb))


class DiscreteGaussian:
    """noise_k=DiscreteGaussian(sigma2) of the containers' encrypt calls: discrete Gaussian noise of variance parameter sigma2 (an integer
    from 1 to 2^24, range_proof_vec.dgauss_sigma2) in place of the binomial noise an int noise_k asks for.  Immutable."""
    __slots__ = ("_sigma2",)

    def __init__(self, sigma2):
        object.__setattr__(self, "_sigma2", _dgauss_sigma2_arg(sigma2))

    sigma2 = property(lambda self: self._sigma2)

    def __setattr__(self, name, value):
        raise AttributeError("DiscreteGaussian is immutable")

    def __eq__(self, other):
        return isinstance(other, DiscreteGaussian) and other._sigma2 == self._sigma2

    def __hash__(self):
        return hash(("DiscreteGaussian", self._sigma2))

    def __repr__(self):
        return "DiscreteGaussian(%d)" % self._sigma2


def _dgauss_sigma2_arg(sigma2):
    if isinstance(sigma2, DiscreteGaussian):
        return sigma2.sigma2
    if isinstance(sigma2, bool) or int(sigma2) != sigma2 or not 1 <= int(sigma2) <= 1 << 24:
        raise ValueError("sigma2 is an integer from 1 to 2^24")
    return int(sigma2)


def _check_range_args(first, prove_range):
    if int(first) < 0 or int(prove_range) < 1:
        raise ValueError("first is not negative and prove_range is at least 1")


class range_proof_vec:
    @staticmethod
    def next_pow2(v):
        return lib().rofl_next_pow2(_sz(v))

    @staticmethod
    def clip_f32_to_range_vec(values, prove_range, fp=None):
        v = np.ascontiguousarray(values, dtype=np.float32)
        out = np.empty_like(v)
        _check(lib().rofl_clip_f32(_ptr(v), _sz(v.size), _sz(prove_range), *_fp(fp), _ptr(out)))
        return out

    # ---- probabilistic quantization (rofl_quantize_prob): seeded stochastic rounding onto the fixed-point grid, one launch per call ----
    @staticmethod
    def quantize_probabilistic_vecs(list_of_values, prove_range, seeds, first=0, fp=None, out=None):
        """rofl_quantize_prob for several vectors of one length (the clients a process hosts) in ONE call: vector v is clipped like
        clip_f32_to_range_vec and each element is rounded to one of its two neighbours on the grid of 2^-fp_frac, up with the probability of
        its fractional part, by word `first + k` of the rounding stream of seeds[v] (include/rofl_zk.h has the definition).  The results are
        f32 values ON the grid: the create calls convert them exactly, and a round aggregates to exactly their sum.
        A vector is a float32 numpy array (anything np.asarray takes) or a contiguous float32 torch tensor on the library's GPU.  out=None
        returns one float32 (n, d) numpy array; otherwise `out` lists one destination per vector -- a writable contiguous float32 numpy array
        or a float32 tensor on the GPU of d elements, which may be the input itself -- and the list is returned.
        A seed is a per-round SECRET of its client (pedersen_ops.quant_round_seed): whoever knows it knows which way every coordinate went."""
        fp = _fp(fp)
        _check_range_args(first, prove_range)
        with _seed_buffer(seeds, len(list_of_values)) as sb:
            return _float_vecs(list_of_values, out, lambda n, vp, d, op:
                               lib().rofl_quantize_prob(n, sb, vp, _sz(int(first)), d, _sz(prove_range), *fp, op))

    @staticmethod
    def quantize_probabilistic(values, prove_range, seed, first=0, fp=None):
        """bindings32.rs quantize_probabilistic(values, len, range) with the rounding the reference's stub leaves out, the randomness an
        explicit 32-byte seed: quantize_probabilistic_vecs for one vector.  -> float32[d] on the fixed-point grid, within the clip range."""
        return range_proof_vec.quantize_probabilistic_vecs([values], prove_range, [seed], first, fp)[0]

    # ---- distributed noise (rofl_noise_binomial): seeded centered-binomial noise on the fixed-point grid, one launch per call ----
    @staticmethod
    def add_binomial_noise_vecs(list_of_values, prove_range, seeds, k, first=0, fp=None, out=None):
        """rofl_noise_binomial for several vectors of one length (the clients a process hosts) in ONE call: vector v is clipped like
        clip_f32_to_range_vec, rounded onto the grid of 2^-fp_frac (the identity after quantize_probabilistic), and element `first + i` gets
        popcount(2k bits of the noise stream of seeds[v]) - k grid steps added: mean 0, variance k / 2 steps^2, and the noise of n clients
        adds up to Binomial(2nk, 1/2) - nk (include/rofl_zk.h has the definition).  k is a multiple of 16 from 16 to 2^20
        (binomial_noise_k).  The results are f32 values ON the grid, inside the clip range: a value within k steps of a bound can saturate
        there, which truncates its noise -- clip_f32_for_noise first where the exact distribution matters.
        Vectors, `out` and the return value are as in quantize_probabilistic_vecs: numpy arrays or float32 tensors on the library's GPU.
        A seed is a per-round SECRET of its client (pedersen_ops.noise_round_seed): whoever knows it removes the client's noise."""
        k, fp = int(k), _fp(fp)
        if k < 16 or k > 1 << 20 or k % 16:
            raise ValueError("k is a multiple of 16 from 16 to 2^20")
        _check_range_args(first, prove_range)
        with _seed_buffer(seeds, len(list_of_values)) as sb:
            return _float_vecs(list_of_values, out, lambda n, vp, d, op:
                               lib().rofl_noise_binomial(n, sb, vp, _sz(int(first)), d, ctypes.c_uint32(k), _sz(prove_range), *fp, op))

    @staticmethod
    def add_binomial_noise(values, prove_range, seed, k, first=0, fp=None):
        """add_binomial_noise_vecs for one vector -> float32[d] on the fixed-point grid, within the clip range."""
        return range_proof_vec.add_binomial_noise_vecs([values], prove_range, [seed], k, first, fp)[0]

    @staticmethod
    def binomial_noise_k(sigma_steps):
        """the smallest k add_binomial_noise accepts whose noise has a standard deviation of at least `sigma_steps` grid steps
        (variance k / 2 >= sigma^2).  What (n clients, k, sensitivity) mean as an (epsilon, delta) is the deployment's accounting."""
        s = Fraction(sigma_steps)
        if s < 0:
            raise ValueError("sigma is not negative")
        k = max(16, 16 * int(math.ceil(2 * s * s / 16)))
        if k > 1 << 20:
            raise ValueError("sigma^2 above 2^19 grid steps^2 needs a k above 2^20")
        return k

    @staticmethod
    def clip_f32_for_noise(values, prove_range, k, fp=None):
        """clip into [min + k steps, max - k steps] of the clip range of (prove_range, fp): after it, add_binomial_noise with this k never
        saturates, so the added noise has exactly the binomial distribution.  NaN goes to the lower bound, as in clip_f32_to_range_vec.
        Raises ValueError when that interval is empty (k steps reach past the middle of the range)."""
        fp, k = _fp(fp), int(k)
        mx = Fraction(conversion32.get_clip_bounds(prove_range, fp=fp)[1])      # (the lower bound is its negative)
        top = mx - Fraction(k, 1 << fp[1])
        if k < 0 or top < 0:
            raise ValueError("no room for k steps of noise inside the clip range")
        hi = np.float32(float(top))                                             # the largest f32 <= max - k steps: on the grid, as every
        if Fraction(float(hi)) > top:                                           # f32 of 2^24 steps or more is
            hi = np.nextafter(hi, np.float32(0))
        v = np.ascontiguousarray(values, dtype=np.float32)
        return np.minimum(hi, np.maximum(-hi, np.where(np.isnan(v), -hi, v))).astype(np.float32)

    # ---- discrete Gaussian noise (rofl_noise_dgauss): the exact seeded sampler, any integer sigma^2 up to 2^24, one launch per call ----
    @staticmethod
    def add_dgauss_noise_vecs(list_of_values, prove_range, seeds, sigma2, first=0, fp=None, out=None):
        """rofl_noise_dgauss for several vectors of one length (the clients a process hosts) in ONE call: vector v is clipped like
        clip_f32_to_range_vec, rounded onto the grid of 2^-fp_frac (the identity after quantize_probabilistic), and element `first + i` gets
        a discrete Gaussian number of grid steps added, P(x) ~ exp(-x^2 / (2 sigma2)), drawn by the exact integer sampler of Canonne,
        Kamath and Steinke from that element's own stream under seeds[v] (include/rofl_zk.h has the definition).  sigma2 is an integer
        from 1 to 2^24 (dgauss_sigma2); the cost does not depend on it.  The results are f32 values ON the grid, inside the clip range: a
        value near a bound can saturate there, which truncates its noise.
        Vectors, `out` and the return value are as in quantize_probabilistic_vecs: numpy arrays or float32 tensors on the library's GPU.
        A seed is a per-round SECRET of its client (pedersen_ops.noise_round_seed): whoever knows it removes the client's noise.  The
        call is not constant time: how long an element takes depends on its noise."""
        sigma2, fp = _dgauss_sigma2_arg(sigma2), _fp(fp)
        _check_range_args(first, prove_range)
        with _seed_buffer(seeds, len(list_of_values)) as sb:
            return _float_vecs(list_of_values, out, lambda n, vp, d, op:
                               lib().rofl_noise_dgauss(n, sb, vp, _sz(int(first)), d, ctypes.c_uint32(sigma2), _sz(prove_range), *fp, op))

    @staticmethod
    def add_dgauss_noise(values, prove_range, seed, sigma2, first=0, fp=None):
        """add_dgauss_noise_vecs for one vector -> float32[d] on the fixed-point grid, within the clip range."""
        return range_proof_vec.add_dgauss_noise_vecs([values], prove_range, [seed], sigma2, first, fp)[0]

    @staticmethod
    def dgauss_sigma2(sigma_steps):
        """the smallest sigma2 add_dgauss_noise accepts that is at least `sigma_steps`^2: an integer from 1 to 2^24.  What (n clients,
        sigma2, sensitivity) mean as an (epsilon, delta) is the deployment's accounting."""
        s = Fraction(sigma_steps)
        if s < 0:
            raise ValueError("sigma is not negative")
        s2 = max(1, int(math.ceil(s * s)))
        if s2 > 1 << 24:
            raise ValueError("sigma above 4096 grid steps needs a sigma2 above 2^24")
        return s2

    # ---- Hadamard rotation (rofl_rotate): y = (1 / sqrt(B)) H_B D x per block of B = 2^block_log2 elements, seeded signs ----
    @staticmethod
    def rotated_len(d, block_log2):
        """ceil(d / B) B with B = 2^block_log2: the length of a rotated vector of d elements -- what the containers and the blinding
        vectors of a rotated round are sized by."""
        d, k = int(d), int(block_log2)
        if d < 0 or not 0 <= k <= 22:
            raise ValueError("d is not negative and block_log2 is 0 .. 22")
        return -(-d >> k) << k

    @staticmethod
    def rotate_vecs(list_of_values, seed_or_seeds, block_log2, inverse=False, out=None):
        """rofl_rotate for several vectors of one length (the clients a process hosts) in ONE call: every block of B = 2^block_log2
        elements of vector v is clamped to +-2^100, multiplied by the signs of the stream of its seed, sent through the Walsh-Hadamard
        butterflies and scaled by 1 / sqrt(B) (include/rofl_zk.h has the definition: bit-defined, the same bytes on the host and on the
        GPU).  A single 32-byte seed is repeated for every vector; it is PUBLIC, every client and the server of a round use the same one
        (pedersen_ops.rotate_round_seed).  A vector of d elements comes back with rotated_len(d, block_log2) elements, the padding
        counting as zeros; inverse=True takes whole blocks and returns as many elements.  Vectors, `out` and the return value are as in
        quantize_probabilistic_vecs: numpy arrays or float32 tensors on the library's GPU, also in place where the buffer holds the
        output length.  The rotation stands in FRONT of the containers: they take the rotated vector and blindings of its length."""
        n, k = len(list_of_values), int(block_log2)
        if not 0 <= k <= 22:
            raise ValueError("block_log2 is 0 .. 22")
        seeds = [bytes(seed_or_seeds)] * n if isinstance(seed_or_seeds, (bytes, bytearray, memoryview)) else list(seed_or_seeds)
        with _seed_buffer(seeds, n) as sb:
            return _float_vecs(list_of_values, out, lambda n_, vp, d, op:
                               lib().rofl_rotate(n_, sb, vp, d, ctypes.c_uint(k), ctypes.c_int(1 if inverse else 0), op),
                               out_len=lambda d: range_proof_vec.rotated_len(d, k))

    @staticmethod
    def rotate(x, seed, block_log2):
        """rotate_vecs for one vector -> float32[rotated_len(d, block_log2)] (a GPU tensor in: pass out= to rotate_vecs to keep it there)."""
        return range_proof_vec.rotate_vecs([x], seed, block_log2)[0]

    @staticmethod
    def unrotate(y, seed, block_log2, d=None):
        """the inverse of rotate on a vector of whole blocks -- what the server applies ONCE to the aggregate DeviceAccumulator.extract
        returns -- truncated to its first d elements (d=None: all of them).  -> float32[d]"""
        x = range_proof_vec.rotate_vecs([y], seed, block_log2, inverse=True)[0]
        if d is not None:
            if not 0 <= int(d) <= x.size:
                raise ValueError("d is 0 .. len(y)")
            x = x[:int(d)]
        return x

    @staticmethod
    def create_rangeproof(values, blindings, prove_range, n_partition, nonce=None, fp=None):
        """-> (proofs uint8[n_proofs, proof_len], commitments uint8[d, 32]).  `values` (f32[d]) and `blindings` (u8[d,32]) may be
        numpy arrays or torch tensors on the library's GPU (no host round trip on the way in)."""
        if _is_dev(values) and _is_dev(blindings):
            (vp, d), (bp, db) = _dev_arg(values, 4), _dev_arg(blindings, 1, 32)
        else:
            v = np.ascontiguousarray(values, dtype=np.float32)
            b = _u8(blindings)
            vp, d, bp, db = _ptr(v), v.size, _ptr(b), (b.shape[0] if b.size else 0)
        nonce = nonce or Nonce.random()
        ns = nonce._struct()
        npr = lib().rofl_rangeproof_chunks(_sz(max(d, 1)), _sz(max(n_partition, 1)))
        plen = lib().rofl_rangeproof_size(_sz(max(prove_range, 1)), _sz(max(d, 1)), _sz(max(n_partition, 1)))
        proofs = np.zeros((max(npr, 1), max(plen, 32)), dtype=np.uint8)
        commits = np.zeros((max(d, 1), 32), dtype=np.uint8)
        plen_o, npr_o = _sz(), _sz()
        _check(lib().rofl_create_rangeproof(vp, _sz(d), bp, _sz(db), _sz(prove_range),
                                            _sz(n_partition), *_fp(fp), ctypes.byref(ns),
                                            _ptr(proofs), ctypes.byref(plen_o), ctypes.byref(npr_o), _ptr(commits)))
        assert plen_o.value == plen and npr_o.value == npr
        return proofs, commits[:d]

    @staticmethod
    def chunk_geometry(d, n_partition):
        """(n_chunks, m): the proofs create_rangeproof produces for d values and the values per chunk (range_proof_vec/mod.rs:54-70)."""
        P = lib().rofl_rangeproof_chunks(_sz(d), _sz(n_partition))
        return P, (lib().rofl_next_pow2(_sz(d)) // P if P else 0)

    @staticmethod
    def create_rangeproof_chunks(values, blindings, prove_range, n_partition, chunk_first, chunk_count, nonce=None, fp=None):
        """rofl_create_rangeproof_chunks: the proofs of chunks [chunk_first, chunk_first + chunk_count) of ONE client -- the unit a rank
        (or a device) takes when a single client's update is split (the reference proves the chunks independently on its rayon pool,
        range_proof_vec/mod.rs:54-78).  `values` / `blindings` are the client's whole vectors.  -> (proofs u8[chunk_count, proof_len],
        commitments u8[k, 32] of the run's own k elements).  Concatenated over the runs in chunk order = create_rangeproof's result."""
        v = np.ascontiguousarray(values, dtype=np.float32)
        b = _u8(blindings)
        d = v.size
        nonce = nonce or Nonce.random()
        ns = nonce._struct()
        P, m = range_proof_vec.chunk_geometry(max(d, 1), max(n_partition, 1))
        plen = lib().rofl_rangeproof_size(_sz(max(prove_range, 1)), _sz(max(d, 1)), _sz(max(n_partition, 1)))
        proofs = np.zeros((max(chunk_count, 1), max(plen, 32)), dtype=np.uint8)
        commits = np.zeros((max(chunk_count * m, 1), 32), dtype=np.uint8)
        plen_o, nc_o = _sz(), _sz()
        _check(lib().rofl_create_rangeproof_chunks(_ptr(v), _sz(d), _ptr(b), _sz(b.shape[0] if b.size else 0), _sz(prove_range), _sz(n_partition), *_fp(fp),
                                                   ctypes.byref(ns), _sz(chunk_first), _sz(chunk_count), _ptr(proofs), ctypes.byref(plen_o), _ptr(commits),
                                                   ctypes.byref(nc_o)))
        assert plen_o.value == plen
        return proofs, commits[:nc_o.value]

    @staticmethod
    def verify_rangeproof_chunks(proofs_run, n_proofs, chunk_first, commits_run, d, prove_range, verifier_seed=None, fp=None):
        """rofl_verify_rangeproof_chunks: the verdict of a run of ONE client's proofs (the AND over the runs is verify_rangeproof's
        bit, range_proof_vec/mod.rs:168-181).  proofs_run u8[count, proof_len] and commits_run (the run's own commitments) are what
        create_rangeproof_chunks returned for the run; n_proofs and d are the client's."""
        p = np.ascontiguousarray(proofs_run, dtype=np.uint8)
        c = _u8(commits_run)
        if c.size == 0:
            c = np.zeros((1, 32), dtype=np.uint8)      # a run of padding chunks has no commitments of its own (nothing is read)
        seed = bytes(verifier_seed) if verifier_seed is not None else os.urandom(32)
        ok = ctypes.c_int()
        _check(lib().rofl_verify_rangeproof_chunks(_ptr(p), _sz(p.shape[1]), _sz(n_proofs), _sz(chunk_first), _sz(p.shape[0]), _ptr(c), _sz(d),
                                                   _sz(prove_range), *_fp(fp), seed, ctypes.byref(ok)))
        return bool(ok.value)

    @staticmethod
    def create_rangeproof_batch(values_list, blindings_list, prove_range, n_partition, nonces=None, fp=None):
        """rofl_create_rangeproof_batch: the updates of several clients (same d) proved as one launch sequence.
        -> list of (proofs, commitments) per client; a client whose own inputs are rejected (out of range, NaN, short nonce
        stream) gets a RoflError instance in its place, the others are proved.  Bit-identical to per-client create_rangeproof."""
        nc = len(values_list)
        if nc == 0:
            return []
        if len(blindings_list) != nc or (nonces is not None and len(nonces) != nc):
            raise ValueError("values_list, blindings_list and nonces must have one entry per client")
        keep, vptrs, bptrs = [], [], []
        d = None
        for v, b in zip(values_list, blindings_list):
            if _is_dev(v) and _is_dev(b):
                (vp, dv), (bp, db) = _dev_arg(v, 4), _dev_arg(b, 1, 32)
                vptrs.append(vp.value); bptrs.append(bp.value)
            else:
                va = np.ascontiguousarray(v, dtype=np.float32); ba = _u8(b)
                keep += [va, ba]
                dv, db = va.size, (ba.shape[0] if ba.size else 0)
                vptrs.append(va.ctypes.data); bptrs.append(ba.ctypes.data)
            if dv != db:
                raise RoflError(1, "WrongNumBlindingFactors")
            if d is not None and dv != d:
                raise ValueError("the clients of a batch have the same number of values")
            d = dv
        nonces = nonces or [Nonce.random() for _ in range(nc)]
        ns = (_NonceStruct * nc)(*[n._struct() for n in nonces])
        npr = lib().rofl_rangeproof_chunks(_sz(max(d, 1)), _sz(max(n_partition, 1)))
        plen = lib().rofl_rangeproof_size(_sz(max(prove_range, 1)), _sz(max(d, 1)), _sz(max(n_partition, 1)))
        proofs = [np.zeros((max(npr, 1), max(plen, 32)), dtype=np.uint8) for _ in range(nc)]
        commits = [np.zeros((max(d, 1), 32), dtype=np.uint8) for _ in range(nc)]
        vp = (ctypes.c_void_p * nc)(*vptrs); bp = (ctypes.c_void_p * nc)(*bptrs)
        pp = (ctypes.c_void_p * nc)(*[p.ctypes.data for p in proofs]); cp = (ctypes.c_void_p * nc)(*[c.ctypes.data for c in commits])
        rcs = (ctypes.c_int * nc)()
        plen_o, npr_o = _sz(), _sz()
        _check(lib().rofl_create_rangeproof_batch(_sz(nc), vp, _sz(d), bp, _sz(prove_range), _sz(n_partition), *_fp(fp), ns, pp,
                                                  ctypes.byref(plen_o), ctypes.byref(npr_o), cp, rcs))
        assert plen_o.value == plen and npr_o.value == npr
        return [(proofs[i], commits[i][:d]) if rcs[i] == 0 else RoflError(rcs[i], "client %d of the batch" % i) for i in range(nc)]

    @staticmethod
    def verify_rangeproof(proofs, commits, prove_range, verifier_seed=None, fp=None):
        p = np.ascontiguousarray(proofs, dtype=np.uint8)
        if _is_dev(commits):
            cptr, dc = _dev_arg(commits, 1, 32)
        else:
            c = _u8(commits)
            cptr, dc = _ptr(c), c.shape[0]
        seed = bytes(verifier_seed) if verifier_seed is not None else os.urandom(32)
        ok = ctypes.c_int()
        _check(lib().rofl_verify_rangeproof(_ptr(p), _sz(p.shape[1]), _sz(p.shape[0]), cptr, _sz(dc),
                                            _sz(prove_range), *_fp(fp), seed, ctypes.byref(ok)))
        return bool(ok.value)

    @staticmethod
    def verify_rangeproof_batch(proofs_list, commits_list, prove_range, verifier_seed=None, fp=None, commit_stride=32):
        """One verdict per client (server.rs:656-687 verifies one client per pool task).  The C entry point takes ONE
        (n_proofs, proof_len, d) for the whole batch and reads that many bytes from every client's pointers, and all three are
        attacker-chosen on the wire: clients whose shapes differ from the majority shape are verified on their own (a malformed
        set counts as not verified), never handed to the batch call with somebody else's lengths.
        commit_stride = 64 / 96: commits_list[i] is the client's (d, stride) array of ElGamal pairs / SquareRandProofCommitments as it came
        off the wire and the commitments are its first 32 bytes per row (params.rs:197, 215) -- no packing pass on the host."""
        if len(proofs_list) != len(commits_list):
            raise ValueError("one commitment vector per proof set")
        ps = [np.ascontiguousarray(p, dtype=np.uint8) for p in proofs_list]
        cs = [_u8(c, last=commit_stride) for c in commits_list]
        n = len(ps)
        if n == 0:
            return []
        seed = bytes(verifier_seed) if verifier_seed is not None else os.urandom(32)
        shapes = [(p.shape if p.ndim == 2 else None, c.shape if c.ndim == 2 and c.shape[1:] == (commit_stride,) else None) for p, c in zip(ps, cs)]
        valid = [sh for sh in shapes if sh[0] is not None and sh[1] is not None and sh[0][0] > 0 and sh[1][0] > 0]
        res = [False] * n
        if not valid:
            return res
        major = max(set(valid), key=valid.count)
        idx = [i for i, sh in enumerate(shapes) if sh == major]
        for i, sh in enumerate(shapes):
            if sh != major and sh in valid:          # a different but well-formed shape: its own call
                try:
                    res[i] = range_proof_vec.verify_rangeproof(ps[i], cs[i][:, :32], prove_range, verifier_seed=seed, fp=fp)
                except RoflError:
                    res[i] = False
        pp = (ctypes.c_void_p * len(idx))(*[ps[i].ctypes.data for i in idx])
        cp = (ctypes.c_void_p * len(idx))(*[cs[i].ctypes.data for i in idx])
        ok = (ctypes.c_int * len(idx))()
        _check(lib().rofl_verify_rangeproof_batch_strided(_sz(len(idx)), pp, _sz(major[0][1]), _sz(major[0][0]), cp, _sz(commit_stride), _sz(major[1][0]),
                                                          _sz(prove_range), *_fp(fp), seed, ok))
        for k, i in enumerate(idx):
            res[i] = bool(ok[k])
        return res


class l2_range_proof_vec:
    # ---- norm clipping (rofl_clip_l2): projection onto the L2 ball on the fixed-point grid, two launches per call ----
    @staticmethod
    def clip_l2_vecs(list_of_values, prove_range, max_sq, seeds=None, fp=None, out=None, with_scale=False):
        """rofl_clip_l2 for several vectors of one length (the clients a process hosts) in ONE call: vector v is clipped like
        clip_f32_to_range_vec and converted to grid steps q; if sum q^2 <= max_sq[v] it comes back on the grid unchanged, otherwise it is
        scaled by m / 2^32, m the largest integer with m^2 sum q^2 <= 2^64 Te, so that the exact integer sum of squares of the RESULT -- what
        the L2 sum proof computes -- is at most max_sq[v] (include/rofl_zk.h has the definition and the proof).  max_sq is an int (steps^2,
        norm_budget) or one int per vector.  seeds=None: the scaled steps are truncated (Te = max_sq); seeds = one 32-byte seed per
        vector: they are rounded up or down by the words of the seed's stream, unbiased given the scale, inside the smaller budget
        Te = (isqrt(max_sq) - ceil(sqrt(d)))^2 that holds the bound for every stream; a seeds list with None entries makes one seeded and
        one unseeded call.  Vectors, `out` and the return value are as in range_proof_vec.quantize_probabilistic_vecs: numpy arrays or
        float32 tensors on the library's GPU, also in place.  with_scale=True: -> (vectors, [scale per vector]), 2^32 for a vector that
        fitted, else m.  A seed is a per-round SECRET of its client (pedersen_ops.clip_round_seed)."""
        n, fp = len(list_of_values), _fp(fp)
        ts = [int(max_sq)] * n if isinstance(max_sq, (int, np.integer)) else [int(t) for t in max_sq]
        if len(ts) != n:
            raise ValueError("one max_sq per vector")
        if any(t < 0 or t >> 64 for t in ts):
            raise ValueError("max_sq is an unsigned 64-bit number of steps^2")
        seeds = [None] * n if seeds is None else list(seeds)
        if len(seeds) != n:
            raise ValueError("one seed (or None) per vector")
        dst = None if out is None else list(out)
        if dst is not None and len(dst) != n:
            raise ValueError("one destination per vector")
        _check_range_args(0, prove_range)
        has = [s is not None for s in seeds]
        # all seeded or none: ONE call; else a seeded and an unseeded call, each into the destinations of its own vectors
        groups = [[i for i in range(n) if has[i]], [i for i in range(n) if not has[i]]] if any(has) and not all(has) else [list(range(n))]
        rows, scales = [None] * n, [None] * n
        for idx in groups:
            tb = (ctypes.c_uint64 * max(len(idx), 1))(*[ts[i] for i in idx])
            sc = (ctypes.c_uint64 * max(len(idx), 1))()
            with _seed_buffer([seeds[i] for i in idx] if idx and has[idx[0]] else None, len(idx)) as sb:
                res = _float_vecs([list_of_values[i] for i in idx], None if dst is None else [dst[i] for i in idx], lambda n_, vp, d, op:
                                  lib().rofl_clip_l2(n_, sb, vp, d, tb, _sz(prove_range), *fp, op, sc))
            for row, i in enumerate(idx):
                rows[i], scales[i] = res[row], int(sc[row])
        if len(groups) > 1:
            res = rows if dst is not None else np.stack(rows)
        return (res, scales) if with_scale else res

    @staticmethod
    def clip_l2(values, prove_range, max_sq, seed=None, fp=None, with_scale=False):
        """clip_l2_vecs for one vector -> float32[d] on the fixed-point grid with sum of squared steps <= max_sq (with_scale: and its scale)."""
        r = l2_range_proof_vec.clip_l2_vecs([values], prove_range, [int(max_sq)], None if seed is None else [seed], fp, None, with_scale)
        return (r[0][0], r[1][0]) if with_scale else r[0]

    @staticmethod
    def norm_budget(l2_range, fp=None, reserve_steps=0):
        """(isqrt(B) - reserve_steps)^2 with B = (2^l2_range - 1) & (2^fp_bits - 1): the max_sq of clip_l2 for an update that is proved with
        `l2_range`.  B is the integer behind the bound of the norm check (conversion32.get_l2_clip_bounds): every sum of squares S <= B
        passes it.  reserve_steps keeps room for what is added AFTER the clip: the noise of noise_k (range_proof_vec.add_binomial_noise) adds
        an L2 length of about sqrt(d noise_k / 2) steps, and since the length of a sum is at most the sum of the lengths, an update clipped
        to isqrt(B) - reserve stays inside B as long as the noise is no longer than the reserve.  How many steps to reserve is the
        deployment's choice: no tail bound is built in, and a draw longer than the reserve fails with NormOutOfRangeError (7) as before.
        S must also stay where the f32 shadow sum of the sum proof is exact (the OverflowError rule, 5); this call does not change that.
        Raises ValueError when the reserve exceeds isqrt(B)."""
        fp, l2_range, reserve_steps = _fp(fp), int(l2_range), int(reserve_steps)
        if l2_range < 1 or reserve_steps < 0:
            raise ValueError("l2_range is at least 1 and the reserve is not negative")
        r = math.isqrt(((1 << l2_range) - 1) & ((1 << fp[0]) - 1)) - reserve_steps
        if r < 0:
            raise ValueError("the reserve exceeds the whole budget of isqrt(B) steps")
        return r * r

    @staticmethod
    def create_rangeproof_l2(values, blindings, prove_range, n_partition, nonce=None, fp=None):
        v = np.ascontiguousarray(values, dtype=np.float32)
        b = _u8(blindings)
        nonce = nonce or Nonce.random()
        ns = nonce._struct()
        proof = np.zeros(32 * (9 + 2 * 6), dtype=np.uint8)
        commit = np.zeros(32, dtype=np.uint8)
        plen = _sz()
        _check(lib().rofl_create_rangeproof_l2(_ptr(v), _sz(v.size), _ptr(b), _sz(b.shape[0] if b.size else 0), _sz(prove_range),
                                               _sz(n_partition), *_fp(fp), ctypes.byref(ns),
                                               _ptr(proof), ctypes.byref(plen), _ptr(commit)))
        return proof[:plen.value].copy(), commit

    @staticmethod
    def create_rangeproof_l2_batch(values_list, blindings_list, prove_range, n_partition, nonces=None, fp=None):
        """rofl_create_rangeproof_l2_batch: create_rangeproof_l2 for several clients (same d) of one process as one launch sequence.
        -> list of (proof, commit) per client, byte-identical to the per-client call with the same nonce; a client whose own inputs are
        rejected gets a RoflError instance with the per-client call's code in its place, the others are proved.  values / blindings of a
        client may be numpy arrays or torch tensors on the library's GPU."""
        nc = len(values_list)
        if nc == 0:
            return []
        if len(blindings_list) != nc or (nonces is not None and len(nonces) != nc):
            raise ValueError("values_list, blindings_list and nonces must have one entry per client")
        keep, vptrs, bptrs = [], [], []
        d = None
        for v, b in zip(values_list, blindings_list):
            (vp, dv), (bp, db) = _client_arg(v, np.float32, 1, keep), _client_arg(b, np.uint8, 32, keep)
            if dv != db:
                raise RoflError(1, "WrongNumBlindingFactors")
            if d is not None and dv != d:
                raise ValueError("the clients of a batch have the same number of values")
            d = dv
            vptrs.append(vp); bptrs.append(bp)
        nonces = nonces or [Nonce.random() for _ in range(nc)]
        ns = (_NonceStruct * nc)(*[n._struct() for n in nonces])
        proofs = [np.zeros(32 * (9 + 2 * 7), dtype=np.uint8) for _ in range(nc)]
        commits = np.zeros((nc, 32), dtype=np.uint8)
        vp = (ctypes.c_void_p * nc)(*vptrs); bp = (ctypes.c_void_p * nc)(*bptrs)
        pp = (ctypes.c_void_p * nc)(*[p.ctypes.data for p in proofs])
        rcs = (ctypes.c_int * nc)()
        plen = _sz()
        _check(lib().rofl_create_rangeproof_l2_batch(_sz(nc), vp, _sz(d), bp, _sz(prove_range), _sz(n_partition), *_fp(fp), ns, pp, ctypes.byref(plen),
                                                     _ptr(commits), rcs))
        return [(proofs[i][:plen.value].copy(), commits[i].copy()) if rcs[i] == 0 else RoflError(rcs[i], "client %d of the batch" % i) for i in range(nc)]

    @staticmethod
    def verify_rangeproof_l2(proof, commit, prove_range, verifier_seed=None, fp=None):
        p = np.ascontiguousarray(proof, dtype=np.uint8)
        c = np.ascontiguousarray(commit, dtype=np.uint8)
        seed = bytes(verifier_seed) if verifier_seed is not None else os.urandom(32)
        ok = ctypes.c_int()
        _check(lib().rofl_verify_rangeproof_l2(_ptr(p), _sz(p.size), _ptr(c), _sz(prove_range), *_fp(fp), seed, ctypes.byref(ok)))
        return bool(ok.value)


    @staticmethod
    def verify_rangeproof_l2_batch(proofs, commits, prove_range, verifier_seed=None, fp=None):
        """rofl_verify_rangeproof_l2_batch: the L2 sum proofs of a round's clients (one length), commits[i] = client i's sum of c_sq.
        One verdict per client."""
        ps = [np.ascontiguousarray(p, dtype=np.uint8).reshape(-1) for p in proofs]
        n = len(ps)
        if n == 0:
            return []
        c = np.ascontiguousarray(commits, dtype=np.uint8).reshape(n, 32)
        if len({p.size for p in ps}) != 1:
            raise RoflError(5, "FormatError: the proofs of a batch have one length")
        seed = bytes(verifier_seed) if verifier_seed is not None else os.urandom(32)
        pp = (ctypes.c_void_p * n)(*[p.ctypes.data for p in ps])
        ok = (ctypes.c_int * n)()
        _check(lib().rofl_verify_rangeproof_l2_batch(_sz(n), pp, _sz(ps[0].size), _ptr(c), _sz(prove_range), *_fp(fp), seed, ok))
        return [bool(x) for x in ok]


def _sigma_verify_batch(fn, plen, clen, proofs_list, commits_list, want_csq):
    """shared body of the three rofl_verify_*_vec_batch bindings: vectors of one length d; returns (verdicts, csq sums or None)"""
    ps = [np.ascontiguousarray(p, dtype=np.uint8).reshape(-1, plen) for p in proofs_list]
    cs = [np.ascontiguousarray(c, dtype=np.uint8).reshape(-1, clen) for c in commits_list]
    n = len(ps)
    if n != len(cs):
        raise ValueError("one commitment vector per proof vector")
    if n == 0:
        return [], (np.zeros((0, 32), np.uint8) if want_csq else None)
    d = ps[0].shape[0]
    if any(p.shape[0] != d for p in ps) or any(c.shape[0] != d for c in cs):
        raise RoflError(1, "WrongNumberOfElGamalPairs: the vectors of a batch have one length")
    pp = (ctypes.c_void_p * n)(*[p.ctypes.data for p in ps])
    cp = (ctypes.c_void_p * n)(*[c.ctypes.data for c in cs])
    ok = (ctypes.c_int * n)()
    if want_csq is None:
        _check(fn(_sz(n), pp, cp, _sz(d), ok))
        return [bool(x) for x in ok], None
    sums = np.zeros((n, 32), dtype=np.uint8)
    _check(fn(_sz(n), pp, cp, _sz(d), ok, _ptr(sums) if want_csq else None))
    return [bool(x) for x in ok], (sums if want_csq else None)


SIGMA_KINDS = {0: (128, 64), 1: (192, 96), 2: (160, 64)}      # kind -> (proof bytes, commitment bytes) per element: RandProof, SquareRandProof, SquareProof


def _client_arg(x, dtype, row, keep):
    """(pointer, rows) of one array of a batch's client, wherever it lives: a numpy array (kept alive in `keep`) or a torch tensor on the library's GPU"""
    if _is_dev(x):
        p, n = _dev_arg(x, np.dtype(dtype).itemsize, row)
        return p.value, n
    a = np.ascontiguousarray(x, dtype=np.float32) if dtype == np.float32 else _u8(x)
    keep.append(a)
    return a.ctypes.data, (a.size if dtype == np.float32 else (a.shape[0] if a.size else 0))


def _sigma_create_batch(kind, values_list, r1_list, r2_list, nonces, existing_list, fp):
    """rofl_create_sigmaproof_vec_batch: the per-element Sigma-proof vectors (kind 0 RandProof, 1 SquareRandProof, 2 SquareProof) of several
    clients (same d) of one process as one launch sequence.  -> list of (proofs, commitments) per client, byte-identical to the per-client
    create_*_vec call with the same nonce; a client whose own inputs are rejected (NaN, an undecodable commitment, a short nonce stream)
    gets a RoflError instance in its place, the others are proved.  The arrays of a client may be numpy arrays or torch tensors on the
    library's GPU."""
    plen, clen = SIGMA_KINDS[int(kind)]
    nc = len(values_list)
    if nc == 0:
        return []
    if existing_list is None:
        existing_list = [None] * nc
    if r2_list is None:
        r2_list = [None] * nc
    if len(r1_list) != nc or len(r2_list) != nc or len(existing_list) != nc or (nonces is not None and len(nonces) != nc):
        raise ValueError("every list of a batch must have one entry per client")
    keep, vptrs, aptrs, bptrs, eptrs = [], [], [], [], []
    d = None
    for v, r1, r2, ex in zip(values_list, r1_list, r2_list, existing_list):
        (vp, dv), (ap, da) = _client_arg(v, np.float32, 1, keep), _client_arg(r1, np.uint8, 32, keep)
        bp, db = (None, dv) if kind == 0 else _client_arg(r2, np.uint8, 32, keep)
        ep, de = (None, dv) if ex is None else _client_arg(ex, np.uint8, 32, keep)
        if dv != da or db != dv or de != dv:
            raise RoflError(1, "WrongNumBlindingFactors")
        if d is not None and dv != d:
            raise ValueError("the clients of a batch have the same number of values")
        d = dv
        vptrs.append(vp); aptrs.append(ap); bptrs.append(bp); eptrs.append(ep)
    nonces = nonces or [Nonce.random() for _ in range(nc)]
    ns = (_NonceStruct * nc)(*[n._struct() for n in nonces])
    proofs = [np.zeros((max(d, 1), plen), dtype=np.uint8) for _ in range(nc)]
    commits = [np.zeros((max(d, 1), clen), dtype=np.uint8) for _ in range(nc)]
    vp = (ctypes.c_void_p * nc)(*vptrs); ap = (ctypes.c_void_p * nc)(*aptrs); ep = (ctypes.c_void_p * nc)(*eptrs)
    bp = None if kind == 0 else (ctypes.c_void_p * nc)(*bptrs)
    pp = (ctypes.c_void_p * nc)(*[p.ctypes.data for p in proofs]); cp = (ctypes.c_void_p * nc)(*[c.ctypes.data for c in commits])
    rcs = (ctypes.c_int * nc)()
    _check(lib().rofl_create_sigmaproof_vec_batch(int(kind), _sz(nc), vp, _sz(d), ap, bp, ep, *_fp(fp), ns, pp, cp, rcs))
    return [(proofs[i][:d], commits[i][:d]) if rcs[i] == 0 else RoflError(rcs[i], "client %d of the batch" % i) for i in range(nc)]


def create_sigmaproof_vec_range(kind, values, random_vec, random_vec_2, elem_first, elem_count, nonce=None, existing=None, fp=None):
    """rofl_create_sigmaproof_vec_range: the proofs of elements [elem_first, elem_first + elem_count) of ONE vector -- the unit a rank takes when a
    client's per-element Sigma-proofs are split over GPUs (the reference proves the elements independently on its rayon pool,
    rand_proof_vec/mod.rs:45-58, square_rand_proof_vec/mod.rs:45-58).  The arrays are the whole vector's; the runs, concatenated in element
    order, are byte for byte what the unsplit create_*_vec call returns.  -> (proofs u8[count, P], commitments u8[count, C])"""
    plen, clen = SIGMA_KINDS[int(kind)]
    v = np.ascontiguousarray(values, dtype=np.float32)
    r1 = _u8(random_vec)
    r2 = None if random_vec_2 is None else _u8(random_vec_2)
    ex = None if existing is None else _u8(existing)
    if r1.shape[0] != v.size or (r2 is not None and r2.shape[0] != v.size) or (ex is not None and ex.shape[0] != v.size):
        raise RoflError(1, "WrongNumBlindingFactors")
    nonce = nonce or Nonce.random()
    ns = nonce._struct()
    proofs = np.zeros((max(elem_count, 1), plen), dtype=np.uint8)
    commits = np.zeros((max(elem_count, 1), clen), dtype=np.uint8)
    _check(lib().rofl_create_sigmaproof_vec_range(int(kind), _ptr(v), _sz(v.size), _ptr(r1), None if r2 is None else _ptr(r2), None if ex is None else _ptr(ex), *_fp(fp),
                                                  ctypes.byref(ns), _sz(elem_first), _sz(elem_count), _ptr(proofs), _ptr(commits)))
    return proofs[:elem_count], commits[:elem_count]


class rand_proof_vec:
    """rand_proof_vec/mod.rs:14-118.  proofs uint8[d,128], ElGamal pairs uint8[d,64]."""

    @staticmethod
    def verify_randproof_vec_batch(proofs_list, pairs_list):
        """rofl_verify_randproof_vec_batch: the vectors of a round's clients in one launch sequence; one verdict per client"""
        return _sigma_verify_batch(lib().rofl_verify_randproof_vec_batch, 128, 64, proofs_list, pairs_list, None)[0]

    @staticmethod
    def create_randproof_vec(values, random_vec, nonce=None, existing=None, fp=None):
        v = np.ascontiguousarray(values, dtype=np.float32)
        r = _u8(random_vec)
        nonce = nonce or Nonce.random()
        ns = nonce._struct()
        d = v.size
        proofs = np.zeros((max(d, 1), 128), dtype=np.uint8)
        pairs = np.zeros((max(d, 1), 64), dtype=np.uint8)
        ex = None if existing is None else _u8(existing)
        _check(lib().rofl_create_randproof_vec(_ptr(v), _sz(d), _ptr(r), _sz(r.shape[0] if r.size else 0), None if ex is None else _ptr(ex),
                                               *_fp(fp), ctypes.byref(ns), _ptr(proofs), _ptr(pairs)))
        return proofs[:d], pairs[:d]

    @staticmethod
    def create_randproof_vec_batch(values_list, random_list, nonces=None, existing_list=None, fp=None):
        """create_randproof_vec(_existing) for several clients (same d) of one process as one call; see _sigma_create_batch"""
        return _sigma_create_batch(0, values_list, random_list, None, nonces, existing_list, fp)

    @staticmethod
    def create_randproof_vec_existing(values, existing, random_vec, nonce=None, fp=None):
        return rand_proof_vec.create_randproof_vec(values, random_vec, nonce=nonce, existing=existing, fp=fp)

    @staticmethod
    def verify_randproof_vec(proofs, pairs):
        p = np.ascontiguousarray(proofs, dtype=np.uint8).reshape(-1, 128)
        c = np.ascontiguousarray(pairs, dtype=np.uint8).reshape(-1, 64)
        if p.shape[0] != c.shape[0]:
            raise RoflError(1, "WrongNumberOfElGamalPairs")
        ok = ctypes.c_int()
        _check(lib().rofl_verify_randproof_vec(_ptr(p), _ptr(c), _sz(p.shape[0]), ctypes.byref(ok)))
        return bool(ok.value)


class square_rand_proof_vec:
    """square_rand_proof_vec/mod.rs:18-159.  proofs uint8[d,192], commitments uint8[d,96] (L | R | c_sq)."""

    @staticmethod
    def create_l2rangeproof_vec(values, random_vec, random_vec_2, nonce=None, existing=None, fp=None):
        v = np.ascontiguousarray(values, dtype=np.float32)
        r1, r2 = _u8(random_vec), _u8(random_vec_2)
        nonce = nonce or Nonce.random()
        ns = nonce._struct()
        d = v.size
        proofs = np.zeros((max(d, 1), 192), dtype=np.uint8)
        commits = np.zeros((max(d, 1), 96), dtype=np.uint8)
        ex = None if existing is None else _u8(existing)
        _check(lib().rofl_create_squarerandproof_vec(_ptr(v), _sz(d), _ptr(r1), _sz(r1.shape[0] if r1.size else 0), _ptr(r2),
                                                     None if ex is None else _ptr(ex), *_fp(fp),
                                                     ctypes.byref(ns), _ptr(proofs), _ptr(commits)))
        return proofs[:d], commits[:d]

    @staticmethod
    def create_l2rangeproof_vec_batch(values_list, random_list, random2_list, nonces=None, existing_list=None, fp=None):
        """create_l2rangeproof_vec(_existing) for several clients (same d) of one process as one call; see _sigma_create_batch"""
        return _sigma_create_batch(1, values_list, random_list, random2_list, nonces, existing_list, fp)

    @staticmethod
    def create_l2rangeproof_vec_existing(values, existing, random_vec, random_vec_2, nonce=None, fp=None):
        return square_rand_proof_vec.create_l2rangeproof_vec(values, random_vec, random_vec_2, nonce=nonce, existing=existing, fp=fp)

    @staticmethod
    def verify_l2rangeproof_vec(proofs, commits):
        p = np.ascontiguousarray(proofs, dtype=np.uint8).reshape(-1, 192)
        c = np.ascontiguousarray(commits, dtype=np.uint8).reshape(-1, 96)
        if p.shape[0] != c.shape[0]:
            raise RoflError(1, "WrongNumberOfElGamalPairs")
        ok = ctypes.c_int()
        _check(lib().rofl_verify_squarerandproof_vec(_ptr(p), _ptr(c), _sz(p.shape[0]), ctypes.byref(ok)))
        return bool(ok.value)


    @staticmethod
    def verify_l2rangeproof_vec_batch(proofs_list, commits_list, with_csq_sums=False):
        """rofl_verify_squarerandproof_vec_batch: one verdict per client; with_csq_sums: also every client's sum of c_sq (params.rs:220)"""
        ok, sums = _sigma_verify_batch(lib().rofl_verify_squarerandproof_vec_batch, 192, 96, proofs_list, commits_list, bool(with_csq_sums))
        return (ok, sums) if with_csq_sums else ok


class square_proof_vec:
    """square_proof_vec/mod.rs:18-159.  proofs uint8[d,160], commitments uint8[d,64] (c_l | c_sq)."""

    @staticmethod
    def verify_l2rangeproof_vec_batch(proofs_list, commits_list, with_csq_sums=False):
        ok, sums = _sigma_verify_batch(lib().rofl_verify_squareproof_vec_batch, 160, 64, proofs_list, commits_list, bool(with_csq_sums))
        return (ok, sums) if with_csq_sums else ok

    @staticmethod
    def create_l2rangeproof_vec(values, random_vec, random_vec_2, nonce=None, existing=None, fp=None):
        v = np.ascontiguousarray(values, dtype=np.float32)
        r1, r2 = _u8(random_vec), _u8(random_vec_2)
        nonce = nonce or Nonce.random()
        ns = nonce._struct()
        d = v.size
        proofs = np.zeros((max(d, 1), 160), dtype=np.uint8)
        commits = np.zeros((max(d, 1), 64), dtype=np.uint8)
        ex = None if existing is None else _u8(existing)
        _check(lib().rofl_create_squareproof_vec(_ptr(v), _sz(d), _ptr(r1), _sz(r1.shape[0] if r1.size else 0), _ptr(r2),
                                                 None if ex is None else _ptr(ex), *_fp(fp),
                                                 ctypes.byref(ns), _ptr(proofs), _ptr(commits)))
        return proofs[:d], commits[:d]

    @staticmethod
    def create_l2rangeproof_vec_batch(values_list, random_list, random2_list, nonces=None, existing_list=None, fp=None):
        """create_l2rangeproof_vec(_existing) for several clients (same d) of one process as one call; see _sigma_create_batch"""
        return _sigma_create_batch(2, values_list, random_list, random2_list, nonces, existing_list, fp)

    @staticmethod
    def create_l2rangeproof_vec_existing(values, existing, random_vec, random_vec_2, nonce=None, fp=None):
        return square_proof_vec.create_l2rangeproof_vec(values, random_vec, random_vec_2, nonce=nonce, existing=existing, fp=fp)

    @staticmethod
    def verify_l2rangeproof_vec(proofs, commits):
        p = np.ascontiguousarray(proofs, dtype=np.uint8).reshape(-1, 160)
        c = np.ascontiguousarray(commits, dtype=np.uint8).reshape(-1, 64)
        if p.shape[0] != c.shape[0]:
            raise RoflError(1, "WrongNumberOfElGamalPairs")
        ok = ctypes.c_int()
        _check(lib().rofl_verify_squareproof_vec(_ptr(p), _ptr(c), _sz(p.shape[0]), ctypes.byref(ok)))
        return bool(ok.value)


class compressed_rand_proof:
    """compressed_rand_proof/mod.rs:134-160 (CompressedRandProof::helper_prove / helper_prove_existing / helper_verify).
    proof uint8[128], ElGamal pairs uint8[d,64]."""

    @staticmethod
    def helper_prove(values, r_vec, nonce=None, existing=None, fp=None):
        v = np.ascontiguousarray(values, dtype=np.float32)
        r = _u8(r_vec)
        nonce = nonce or Nonce.random()
        ns = nonce._struct()
        d = v.size
        proof = np.zeros(128, dtype=np.uint8)
        pairs = np.zeros((max(d, 1), 64), dtype=np.uint8)
        ex = None if existing is None else _u8(existing)
        _check(lib().rofl_create_compressed_randproof(_ptr(v), _sz(d), _ptr(r), _sz(r.shape[0] if r.size else 0), None if ex is None else _ptr(ex),
                                                      *_fp(fp), ctypes.byref(ns), _ptr(proof), _ptr(pairs)))
        return proof, pairs[:d]

    @staticmethod
    def helper_prove_existing(values, m_com, r_vec, nonce=None, fp=None):
        return compressed_rand_proof.helper_prove(values, r_vec, nonce=nonce, existing=m_com, fp=fp)

    @staticmethod
    def helper_prove_batch(values_list, r_list, nonces=None, existing_list=None, fp=None):
        """rofl_create_compressed_randproof_batch: helper_prove / helper_prove_existing for several clients (same d) of one process as one
        launch sequence.  existing_list (optional) holds per client the commitments to complete, or None.  -> list of (proof, pairs) per
        client, byte-identical to the per-client call with the same nonce; a client whose own inputs are rejected (NaN, an undecodable
        commitment, a short nonce stream) gets a RoflError instance in its place, the others are proved.  values / r / existing of a
        client may be numpy arrays or torch tensors on the library's GPU."""
        nc = len(values_list)
        if nc == 0:
            return []
        if existing_list is None:
            existing_list = [None] * nc
        if len(r_list) != nc or len(existing_list) != nc or (nonces is not None and len(nonces) != nc):
            raise ValueError("values_list, r_list, existing_list and nonces must have one entry per client")
        keep, vptrs, rptrs, eptrs = [], [], [], []
        d = None

        def arg(x, dtype, row):      # (pointer, rows) of one array of a client, wherever it lives
            if _is_dev(x):
                p, n = _dev_arg(x, np.dtype(dtype).itemsize, row)
                return p.value, n
            a = np.ascontiguousarray(x, dtype=np.float32) if dtype == np.float32 else _u8(x)
            keep.append(a)
            return a.ctypes.data, (a.size if dtype == np.float32 else (a.shape[0] if a.size else 0))
        for v, r, ex in zip(values_list, r_list, existing_list):
            (vp, dv), (rp, dr) = arg(v, np.float32, 1), arg(r, np.uint8, 32)
            ep, de = (None, dv) if ex is None else arg(ex, np.uint8, 32)
            if dv != dr or de != dv:
                raise RoflError(1, "WrongNumBlindingFactors")
            if d is not None and dv != d:
                raise ValueError("the clients of a batch have the same number of values")
            d = dv
            vptrs.append(vp); rptrs.append(rp); eptrs.append(ep)
        nonces = nonces or [Nonce.random() for _ in range(nc)]
        ns = (_NonceStruct * nc)(*[n._struct() for n in nonces])
        proofs = [np.zeros(128, dtype=np.uint8) for _ in range(nc)]
        pairs = [np.zeros((max(d, 1), 64), dtype=np.uint8) for _ in range(nc)]
        vp = (ctypes.c_void_p * nc)(*vptrs); rp = (ctypes.c_void_p * nc)(*rptrs); ep = (ctypes.c_void_p * nc)(*eptrs)
        pp = (ctypes.c_void_p * nc)(*[p.ctypes.data for p in proofs]); cp = (ctypes.c_void_p * nc)(*[c.ctypes.data for c in pairs])
        rcs = (ctypes.c_int * nc)()
        _check(lib().rofl_create_compressed_randproof_batch(_sz(nc), vp, _sz(d), rp, ep, *_fp(fp), ns, pp, cp, rcs))
        return [(proofs[i], pairs[i][:d]) if rcs[i] == 0 else RoflError(rcs[i], "client %d of the batch" % i) for i in range(nc)]

    @staticmethod
    def helper_verify(proof, pairs):
        p = np.ascontiguousarray(proof, dtype=np.uint8).reshape(128)
        c = np.ascontiguousarray(pairs, dtype=np.uint8).reshape(-1, 64)
        ok = ctypes.c_int()
        _check(lib().rofl_verify_compressed_randproof(_ptr(p), _ptr(c), _sz(c.shape[0]), ctypes.byref(ok)))
        return bool(ok.value)

    @staticmethod
    def helper_verify_batch(proofs, pairs_list):
        """rofl_verify_compressed_randproof_batch: the proofs of a round's clients, one call per vector length d.  One verdict per client,
        what helper_verify gives it -- a member that helper_verify rejects with FormatError is False.  A member whose arrays are malformed
        (a proof that is not 128 bytes, pairs that are not a (d, 64) array) is False without reaching the library."""
        n = len(proofs)
        if n != len(pairs_list):
            raise ValueError("one pair vector per proof")
        ps, cs, by_d = [None] * n, [None] * n, {}
        for i, (p, c) in enumerate(zip(proofs, pairs_list)):
            p = np.ascontiguousarray(p, dtype=np.uint8).reshape(-1)
            c = np.ascontiguousarray(c, dtype=np.uint8)
            if p.size == 128 and c.ndim == 2 and c.shape[1] == 64:
                ps[i], cs[i] = p, c
                by_d.setdefault(c.shape[0], []).append(i)
        res = [False] * n
        for d, idx in by_d.items():
            pp = (ctypes.c_void_p * len(idx))(*[ps[i].ctypes.data for i in idx])
            cp = (ctypes.c_void_p * len(idx))(*[cs[i].ctypes.data for i in idx])
            ok = (ctypes.c_int * len(idx))()
            _check(lib().rofl_verify_compressed_randproof_batch(_sz(len(idx)), pp, cp, _sz(d), ok))
            for k, i in enumerate(idx):
                res[i] = bool(ok[k])
        return res

    @staticmethod
    def helper_verify_batch_strided(proofs_list, records_list, stride):
        """rofl_verify_compressed_randproof_batch_strided: helper_verify_batch over records read in place -- records_list[i] is a (d, stride)
        array, stride 64 (ElGamal pairs) or 96 (SquareRandProofCommitments: the pair is the first 64 bytes, c_sq is never read).  One
        verdict per client, what helper_verify_batch gives it on the packed pairs; a member whose arrays are malformed (a proof that is
        not 128 bytes, records that are not a contiguous (d, stride) array) is False without reaching the library."""
        stride = int(stride)
        if stride not in (64, 96):
            raise RoflError(11, "stride must be 64 or 96")
        n = len(proofs_list)
        if n != len(records_list):
            raise ValueError("one record vector per proof")
        ps, cs, by_d = [None] * n, [None] * n, {}
        for i, (p, c) in enumerate(zip(proofs_list, records_list)):
            p = np.ascontiguousarray(p, dtype=np.uint8).reshape(-1)
            c = np.ascontiguousarray(c, dtype=np.uint8)
            if p.size == 128 and c.ndim == 2 and c.shape[1] == stride:
                ps[i], cs[i] = p, c
                by_d.setdefault(c.shape[0], []).append(i)
        res = [False] * n
        for d, idx in by_d.items():
            pp = (ctypes.c_void_p * len(idx))(*[ps[i].ctypes.data for i in idx])
            cp = (ctypes.c_void_p * len(idx))(*[cs[i].ctypes.data for i in idx])
            ok = (ctypes.c_int * len(idx))()
            _check(lib().rofl_verify_compressed_randproof_batch_strided(_sz(len(idx)), pp, cp, _sz(stride), _sz(d), ok))
            for k, i in enumerate(idx):
                res[i] = bool(ok[k])
        return res


def _keys32(a, what):
    """keys as uint8[n, 32]: an (n, 32) / flat array, or a list of 32-byte strings"""
    if isinstance(a, (list, tuple)):
        a = [np.frombuffer(bytes(k), dtype=np.uint8) if isinstance(k, (bytes, bytearray, memoryview)) else np.asarray(k, dtype=np.uint8).reshape(-1) for k in a]
        if any(k.size != 32 for k in a):
            raise ValueError("%s is 32 bytes" % what)
        a = np.stack(a) if a else np.zeros((0, 32), dtype=np.uint8)
    elif isinstance(a, (bytes, bytearray, memoryview)):
        a = np.frombuffer(bytes(a), dtype=np.uint8)
    a = np.asarray(a, dtype=np.uint8)
    if a.size % 32 or (a.ndim > 1 and a.shape[-1] != 32):
        raise ValueError("%s is 32 bytes" % what)
    return np.ascontiguousarray(a).reshape(-1, 32)


class key_agreement:
    """Batched Ristretto255 Diffie-Hellman (rofl_dh_public_keys / rofl_dh_shared): where the shared secrets of the pairwise masks come from.
    A secret key is 32 bytes, reduced mod l (0 mod l is refused); the public key is encode(sk * B); the shared secret of own key a and peer key
    P_b is SHAKE256("rofl-zk/dh/v1" || 000000 || encode(a * P_b) || lo || hi)[0 .. 32), lo <= hi the two public keys as byte strings -- the
    same 32 bytes on both sides.  Not constant-time.  A key serves one epoch: revealing it (a round that rejects its owner) reveals every
    secret it agreed on."""

    @staticmethod
    def public_keys(sk):
        """-> uint8[n, 32]"""
        sk = _keys32(sk, "a secret key")
        n = sk.shape[0]
        out = np.zeros((n, 32), dtype=np.uint8)
        buf = (ctypes.c_ubyte * max(n * 32, 1))()
        try:
            ctypes.memmove(buf, sk.ctypes.data, n * 32)
            _check(lib().rofl_dh_public_keys(_sz(n), buf, _ptr(out)))
        finally:
            ctypes.memset(buf, 0, ctypes.sizeof(buf))
        return out

    @staticmethod
    def shared_secrets(sk, peer_pks, pairs=None, with_public=False):
        """Shared secrets of own keys sk (n_own) and peer public keys peer_pks (n_peer), ONE call: pairs = [(own, peer), ...] indexes the two
        arrays, None = all n_own x n_peer pairs, own-major.  -> (uint8[n_pairs, 32], uint8[n_pairs]); status 1 = the peer key is not a
        canonical Ristretto encoding, 2 = it is the identity, and the 32 bytes of such a pair are zero.  with_public=True appends the own
        public keys uint8[n_own, 32]."""
        sk, pk = _keys32(sk, "a secret key"), _keys32(peer_pks, "a public key")
        n_own, n_peer = sk.shape[0], pk.shape[0]
        if pairs is None:
            n_pairs, parr = n_own * n_peer, None
        else:
            pl = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
            n_pairs = pl.shape[0]
            if n_pairs and (pl.min() < 0 or pl[:, 0].max() >= n_own or pl[:, 1].max() >= n_peer):
                raise ValueError("a pair names a key that is not in the call")
            parr = (_DhPair * max(n_pairs, 1))()
            np.frombuffer(parr, dtype=np.uint32)[:2 * n_pairs] = pl.astype(np.uint32).reshape(-1)
        out, status = np.zeros((n_pairs, 32), dtype=np.uint8), np.zeros(n_pairs, dtype=np.uint8)
        own_pk = np.zeros((n_own, 32), dtype=np.uint8) if with_public else None
        buf = (ctypes.c_ubyte * max(n_own * 32, 1))()
        try:
            ctypes.memmove(buf, sk.ctypes.data, n_own * 32)
            _check(lib().rofl_dh_shared(_sz(n_own), buf, _ptr(own_pk) if with_public else None, _sz(n_peer), _ptr(pk), _sz(n_pairs), parr,
                                        _ptr(out), _ptr(status)))
        finally:
            ctypes.memset(buf, 0, ctypes.sizeof(buf))
        if with_public and n_pairs == 0 and n_own:      # (an empty call computes nothing: the keys come from their own entry)
            own_pk = key_agreement.public_keys(sk)
        return (out, status, own_pk) if with_public else (out, status)


def _pack_messages(messages):
    """a list of bytes-likes as the C ABI takes it: (uint8[total] packed back to back, uint64[n + 1] offsets)"""
    msgs = [bytes(m) for m in messages]
    off = np.zeros(len(msgs) + 1, dtype=np.uint64)
    if msgs:
        off[1:] = np.cumsum([len(m) for m in msgs], dtype=np.uint64)
    return np.frombuffer(b"".join(msgs), dtype=np.uint8), off


def _sig_refs(refs, n_keys, n_msgs):
    """(n, ctypes array or None) of a ref list [(key, msg), ...]; None = signature i uses key i and message i"""
    if refs is None:
        if n_keys != n_msgs:
            raise ValueError("without refs there is one message per key")
        return n_keys, None
    rl = np.asarray(refs, dtype=np.int64).reshape(-1, 2)
    n = rl.shape[0]
    if n and (rl.min() < 0 or rl[:, 0].max() >= n_keys or rl[:, 1].max() >= n_msgs):
        raise ValueError("a ref names a key or a message that is not in the call")
    arr = (_SigRef * max(n, 1))()
    np.frombuffer(arr, dtype=np.uint32)[:2 * n] = rl.astype(np.uint32).reshape(-1)
    return n, arr


class signatures:
    """Batched deterministic Schnorr signatures over Ristretto255 (rofl_sig_sign / rofl_sig_verify): what authenticates the public keys and
    the Feldman commitments of a round.  A key is 32 bytes, reduced mod l (0 mod l is refused); its public key is encode(key * B), the bytes
    of key_agreement.public_keys.  With h = SHAKE256("rofl-zk/sig/v1/m" || u64le(len m) || m)[0 .. 32): nonce k from
    SHAKE256("rofl-zk/sig/v1/k" || canonical32(key) || h), R = encode(k B), c from SHAKE256("rofl-zk/sig/v1/c" || R || A || h), s = k + c key;
    the signature is R || s, 64 bytes, the same for the same key and message.  Not constant-time; deterministic nonces.  Use a signing key of
    its own, NEVER the key-agreement key: that one is revealed when its owner drops out."""

    @staticmethod
    def public_keys(sk):
        """-> uint8[n, 32], the bytes of key_agreement.public_keys"""
        return key_agreement.public_keys(sk)

    @staticmethod
    def sign(sks, messages, refs=None, with_public=False):
        """Signatures of the keys sks on the messages (a list of bytes-likes), ONE call: refs = [(key, message), ...] indexes the two, None =
        key i signs message i.  -> uint8[n, 64]; with_public=True appends the public keys uint8[n_keys, 32]."""
        sk = _keys32(sks, "a secret key")
        data, off = _pack_messages(messages)
        n_keys, n_msgs = sk.shape[0], off.shape[0] - 1
        n, rarr = _sig_refs(refs, n_keys, n_msgs)
        out = np.zeros((n, 64), dtype=np.uint8)
        pk = np.zeros((n_keys, 32), dtype=np.uint8) if with_public else None
        buf = (ctypes.c_ubyte * max(n_keys * 32, 1))()
        try:
            ctypes.memmove(buf, sk.ctypes.data, n_keys * 32)
            _check(lib().rofl_sig_sign(_sz(n_keys), buf, _ptr(pk) if with_public else None, _sz(n_msgs), _ptr(data) if data.size else None, _ptr(off),
                                       _sz(n), rarr, _ptr(out)))
        finally:
            ctypes.memset(buf, 0, ctypes.sizeof(buf))
        if with_public and n == 0 and n_keys:      # (an empty call computes nothing: the keys come from their own entry)
            pk = key_agreement.public_keys(sk)
        return (out, pk) if with_public else out

    @staticmethod
    def verify(pks, messages, sigs, refs=None):
        """-> uint8[n] verdicts of the signatures sigs uint8[n, 64], ONE call: 0 = valid, 1 = not, 2 = the key is not a canonical Ristretto
        encoding or is the identity, or s >= l.  refs as in sign()."""
        pk = _keys32(pks, "a public key")
        data, off = _pack_messages(messages)
        n_keys, n_msgs = pk.shape[0], off.shape[0] - 1
        n, rarr = _sig_refs(refs, n_keys, n_msgs)
        sg = np.ascontiguousarray(np.asarray(sigs, dtype=np.uint8))
        if sg.size != n * 64 or (sg.ndim > 1 and sg.shape[-1] != 64):
            raise ValueError("sigs are uint8[n, 64], one per ref")
        out = np.zeros(n, dtype=np.uint8)
        _check(lib().rofl_sig_verify(_sz(n_keys), _ptr(pk), _sz(n_msgs), _ptr(data) if data.size else None, _ptr(off), _sz(n), rarr, _ptr(sg), _ptr(out)))
        return out


def _leaf_input(messages, digests):
    """(n, bytes pointer or None, offsets pointer or None, the arrays kept alive) of a call's leaves: messages packed, or digests uint8[n, 32]"""
    if (messages is None) == (digests is None):
        raise ValueError("either messages or digests")
    if digests is not None:
        dg = _keys32(digests, "a leaf digest")
        return dg.shape[0], _ptr(dg), None, (dg,)
    data, off = _pack_messages(messages)
    return off.shape[0] - 1, _ptr(data) if data.size else None, _ptr(off), (data, off)


class merkle:
    """Batched Merkle trees (rofl_merkle_build / rofl_merkle_verify): a list of byte strings behind one 32-byte root, single entries proved and
    checked by a path of depth(n) hashes.  leaf(m) = SHAKE256("rofl-zk/mtr/v1/l" || u64le(len m) || m)[0 .. 32), node(a, b) =
    SHAKE256("rofl-zk/mtr/v1/n" || a || b)[0 .. 32); a level of odd width moves its last node up unchanged (the shape of RFC 6962);
    root = SHAKE256("rofl-zk/mtr/v1/r" || u64le(n) || top)[0 .. 32).  The path of leaf j has depth(n) slots bottom up: the sibling
    level_l[(j >> l) ^ 1], or 32 zero bytes where the node moved up alone.  Nothing is secret.  No consistency or append proofs, no proof
    of absence, one tree per call."""
    MAX_STRIDE = 20

    @staticmethod
    def depth(n):
        """slots in a path of a tree of n >= 1 leaves: bit_length(n - 1)"""
        n = int(n)
        if n < 1:
            raise ValueError("a tree has at least one leaf")
        return (n - 1).bit_length()

    @staticmethod
    def _build(fn, messages, digests, paths_for, with_leaves):
        n, bytes_p, off_p, keep = _leaf_input(messages, digests)
        if n == 0:
            raise ValueError("a tree has at least one leaf")
        idx = np.ascontiguousarray(np.asarray([] if paths_for is None else paths_for, dtype=np.int64).reshape(-1))
        if idx.size and (idx.min() < 0 or idx.max() >= n):
            raise ValueError("a path names a leaf that is not in the tree")
        idx = idx.astype(np.uint32)
        d = merkle.depth(n)
        root = np.zeros(32, dtype=np.uint8)
        leaves = np.zeros((n, 32), dtype=np.uint8) if with_leaves else None
        paths = np.zeros((idx.size, d, 32), dtype=np.uint8)
        _check(fn(_sz(n), bytes_p, off_p, _ptr(root), _ptr(leaves) if with_leaves else None, _sz(idx.size), _ptr(idx) if idx.size else None,
                  _ptr(paths) if paths.size else None))
        del keep
        out = (root,) + ((paths,) if paths_for is not None else ()) + ((leaves,) if with_leaves else ())
        return out if len(out) > 1 else root

    @staticmethod
    def build(messages=None, digests=None, paths_for=None, with_leaves=False):
        """The tree over the messages (a list of bytes-likes) or over leaf digests uint8[n, 32], ONE call -> root uint8[32]; with paths_for
        (leaf indices, any order, repeats allowed) also paths uint8[k, depth(n), 32]; with_leaves=True appends the leaf digests uint8[n, 32]."""
        return merkle._build(lib().rofl_merkle_build, messages, digests, paths_for, with_leaves)

    @staticmethod
    def _verify(fn, roots, counts, paths, messages, digests, refs):
        rt = _keys32(roots, "a root")
        cnt = np.ascontiguousarray(np.asarray(counts, dtype=np.int64).reshape(-1))
        if cnt.size != rt.shape[0]:
            raise ValueError("one leaf count per root")
        if cnt.size and (cnt.min() < 1 or cnt.max() > 1 << 20):
            raise ValueError("a leaf count is in [1, 2^20]")
        cnt = cnt.astype(np.uint32)
        n, bytes_p, off_p, keep = _leaf_input(messages, digests)
        pt = np.ascontiguousarray(np.asarray(paths, dtype=np.uint8))
        if pt.ndim != 3 or pt.shape[0] != n or pt.shape[2] != 32:
            raise ValueError("paths are uint8[n, stride, 32], one row per leaf")
        stride = pt.shape[1]
        rarr = None
        if refs is not None:
            rl = np.asarray(refs, dtype=np.int64).reshape(-1, 2)
            if rl.shape[0] != n:
                raise ValueError("one ref per path")
            if n and (rl.min() < 0 or rl[:, 0].max() >= rt.shape[0] or rl[:, 1].max() >= 1 << 32):
                raise ValueError("a ref names a root that is not in the call")
            rarr = (_MerkleRef * max(n, 1))()
            np.frombuffer(rarr, dtype=np.uint32)[:2 * n] = rl.astype(np.uint32).reshape(-1)
        out = np.zeros(n, dtype=np.uint8)
        _check(fn(_sz(rt.shape[0]), _ptr(rt), _ptr(cnt), _sz(n), rarr, bytes_p, off_p, _ptr(pt) if pt.size else None, _sz(stride), _ptr(out)))
        del keep
        return out

    @staticmethod
    def verify(roots, counts, paths, messages=None, digests=None, refs=None):
        """-> uint8[n] verdicts of the paths uint8[n, stride, 32] (the rows of build(), or wider rows whose further slots are zero), ONE call:
        path i is the leaf messages[i] (or digests[i]) at index refs[i][1] under root refs[i][0] of roots uint8[n_roots, 32] with counts[root]
        leaves; refs=None: one root, leaf i at index i.  0 = the climb gives the root, 1 = it does not, 2 = the index is not below the leaf
        count or a slot the shape leaves empty holds a nonzero byte."""
        return merkle._verify(lib().rofl_merkle_verify, roots, counts, paths, messages, digests, refs)


def _dh_pairs(pairs, n_own, n_peer):
    """(n_pairs, ctypes array or None) of a pair list [(own, peer), ...]; None = all n_own x n_peer pairs, own-major"""
    if pairs is None:
        return n_own * n_peer, None
    pl = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    n_pairs = pl.shape[0]
    if n_pairs and (pl.min() < 0 or pl[:, 0].max() >= n_own or pl[:, 1].max() >= n_peer):
        raise ValueError("a pair names a key that is not in the call")
    parr = (_DhPair * max(n_pairs, 1))()
    np.frombuffer(parr, dtype=np.uint32)[:2 * n_pairs] = pl.astype(np.uint32).reshape(-1)
    return n_pairs, parr


class dleq:
    """Batched Chaum-Pedersen proofs of discrete-log equality over Ristretto255 (rofl_dleq_prove / rofl_dleq_verify): what lets a third
    party judge a complaint about a sealed share.  The holder of x behind A = encode(x B) reveals S = encode(x decode(P)), the raw DH point
    of its pair with the peer key P, and proves that S was made with that x: k from SHAKE256("rofl-zk/dleq/v1k" || canonical32(x) || P ||
    ctx), T1 = encode(k B), T2 = encode(k decode(P)), c from SHAKE256("rofl-zk/dleq/v1c" || A || P || S || T1 || T2 || ctx), s = k + c x;
    the proof is c || s, 64 bytes, the same for the same inputs.  ctx is 32 bytes that bind a proof to its use.  Not constant-time;
    deterministic nonces.  A reveal opens the pair's channel in both directions for the whole epoch of the two keys: re-key afterwards."""

    @staticmethod
    def prove(sks, peer_pks, ctxs, pairs=None, with_public=False):
        """Reveals and proofs of own keys sks (n_own) against peer public keys peer_pks (n_peer), ONE call: pairs as in
        key_agreement.shared_secrets, ctxs uint8[n_pairs, 32].  -> (reveals uint8[n_pairs, 32], proofs uint8[n_pairs, 64], status
        uint8[n_pairs]); status 1 = the peer key is not a canonical Ristretto encoding, 2 = it is the identity, and reveal and proof of such a
        pair are zero.  with_public=True appends the own public keys uint8[n_own, 32]."""
        sk, pk, cx = _keys32(sks, "a secret key"), _keys32(peer_pks, "a public key"), _keys32(ctxs, "a context")
        n_own, n_peer = sk.shape[0], pk.shape[0]
        n_pairs, parr = _dh_pairs(pairs, n_own, n_peer)
        if cx.shape[0] != n_pairs:
            raise ValueError("one context per pair")
        reveal, proof, status = np.zeros((n_pairs, 32), dtype=np.uint8), np.zeros((n_pairs, 64), dtype=np.uint8), np.zeros(n_pairs, dtype=np.uint8)
        own_pk = np.zeros((n_own, 32), dtype=np.uint8) if with_public else None
        buf = (ctypes.c_ubyte * max(n_own * 32, 1))()
        try:
            ctypes.memmove(buf, sk.ctypes.data, n_own * 32)
            _check(lib().rofl_dleq_prove(_sz(n_own), buf, _ptr(own_pk) if with_public else None, _sz(n_peer), _ptr(pk), _sz(n_pairs), parr, _ptr(cx),
                                         _ptr(reveal), _ptr(proof), _ptr(status)))
        finally:
            ctypes.memset(buf, 0, ctypes.sizeof(buf))
        if with_public and n_pairs == 0 and n_own:      # (an empty call computes nothing: the keys come from their own entry)
            own_pk = key_agreement.public_keys(sk)
        return (reveal, proof, status, own_pk) if with_public else (reveal, proof, status)

    @staticmethod
    def verify(own_pks, peer_pks, ctxs, reveals, proofs, pairs=None):
        """-> (verdicts uint8[n_pairs], shared uint8[n_pairs, 32]), ONE call: verdict 0 = the proof holds, 1 = it does not, 2 = a key or the
        reveal is not a canonical Ristretto encoding or is the identity, or c or s >= l.  shared is the key_agreement.shared_secrets output of
        the pair for verdict 0 and zeros otherwise: it opens what the pair sealed, so zero it when done."""
        a, pk, cx = _keys32(own_pks, "a public key"), _keys32(peer_pks, "a public key"), _keys32(ctxs, "a context")
        n_own, n_peer = a.shape[0], pk.shape[0]
        n_pairs, parr = _dh_pairs(pairs, n_own, n_peer)
        rv = _keys32(reveals, "a reveal")
        pf = np.ascontiguousarray(np.asarray(proofs, dtype=np.uint8))
        if pf.size != n_pairs * 64 or (pf.ndim > 1 and pf.shape[-1] != 64):
            raise ValueError("proofs are uint8[n_pairs, 64]")
        if cx.shape[0] != n_pairs or rv.shape[0] != n_pairs:
            raise ValueError("one context and one reveal per pair")
        verdict, shared = np.zeros(n_pairs, dtype=np.uint8), np.zeros((n_pairs, 32), dtype=np.uint8)
        _check(lib().rofl_dleq_verify(_sz(n_own), _ptr(a), _sz(n_peer), _ptr(pk), _sz(n_pairs), parr, _ptr(cx), _ptr(rv), _ptr(pf), _ptr(shared), _ptr(verdict)))
        return verdict, shared


def _packed(x, what):
    """Byte strings as the C ABI takes them -> (uint8[total], uint64[n + 1], form).  Three forms are accepted: a pre-packed
    (uint8[total], uint64[n + 1]) pair (form "packed"); a 2-D uint8 array of equal-length rows (form = the row length; no Python-level
    join); a list of bytes-likes (form None)."""
    if isinstance(x, tuple) and len(x) == 2 and isinstance(x[1], np.ndarray) and x[1].dtype == np.uint64:
        data, off = np.ascontiguousarray(np.asarray(x[0], dtype=np.uint8)).reshape(-1), np.ascontiguousarray(x[1]).reshape(-1)
        if off.size < 1 or off[0] != 0 or (off[1:] < off[:-1]).any() or int(off[-1]) > data.size:
            raise ValueError("%s: offsets start at 0, do not decrease and end inside the bytes" % what)
        return data, off, "packed"
    if isinstance(x, np.ndarray) and x.ndim == 2:
        if x.dtype != np.uint8:
            raise ValueError("%s: a 2-D array is uint8[n, length]" % what)
        return np.ascontiguousarray(x).reshape(-1), np.arange(x.shape[0] + 1, dtype=np.uint64) * np.uint64(x.shape[1]), int(x.shape[1])
    data, off = _pack_messages(x)
    return data, off, None


class aead:
    """Batched RFC 8439 ChaCha20-Poly1305 (rofl_aead_seal / rofl_aead_open): what encrypts the share bundles a server relays between
    clients.  A record is CT || tag, 16 bytes longer than its payload: libsodium's crypto_aead_chacha20poly1305_ietf combined form, which any
    standard library opens.  keys: uint8[n_keys, 32]; record i uses keys[key_idx[i]] (key_idx None: keys[i]).  With derive_round=None a key
    is the RFC 8439 key itself; with derive_round=r a row is a key_agreement.shared_secrets output and the key is
    SHAKE256("rofl-zk/seal/v1\\0" || row || u64le(r))[0 .. 32), derived once per key on the device.  nonces: uint8[n, 12].  ads, plaintexts and
    sealed each come as a list of bytes-likes, as a 2-D uint8 array of equal-length rows, or as a pre-packed (uint8[total], uint64[n + 1])
    pair; the array forms do not go through a Python-level join.  Not constant-time.  A (key, nonce) pair that seals two different payloads
    gives away both and the authenticator: the caller owns nonce uniqueness."""

    @staticmethod
    def _args(keys, nonces, ads, key_idx, derive_round):
        k = _keys32(keys, "a key")
        nc = np.ascontiguousarray(np.asarray(nonces, dtype=np.uint8) if not isinstance(nonces, (list, tuple))
                                  else np.array([np.frombuffer(bytes(v), dtype=np.uint8) for v in nonces], dtype=np.uint8).reshape(-1, 12))
        if nc.size % 12 or (nc.ndim > 1 and nc.shape[-1] != 12):
            raise ValueError("nonces are uint8[n, 12]")
        nc = nc.reshape(-1, 12)
        n = nc.shape[0]
        ad, ad_off, _ = _packed(ads, "ads")
        if ad_off.size != n + 1:
            raise ValueError("one AD per nonce")
        idx = None
        if key_idx is None:
            if k.shape[0] != n:
                raise ValueError("without key_idx there is one key per record")
        else:
            ki = np.asarray(key_idx, dtype=np.int64).reshape(-1)
            if ki.size != n or (n and (ki.min() < 0 or ki.max() >= k.shape[0])):
                raise ValueError("key_idx names one key of the call per record")
            idx = np.ascontiguousarray(ki.astype(np.uint32))
        rnd = None if derive_round is None else np.array([int(derive_round)], dtype=np.uint64)
        return k, nc, n, ad, ad_off, idx, rnd

    @staticmethod
    def seal(keys, nonces, ads, plaintexts, key_idx=None, derive_round=None):
        """-> the sealed records in the form of `plaintexts`: a list of bytes, uint8[n, length + 16], or the packed pair
        (uint8[total + 16 n], uint64[n + 1]).  ONE call."""
        k, nc, n, ad, ad_off, idx, rnd = aead._args(keys, nonces, ads, key_idx, derive_round)
        pt, pt_off, form = _packed(plaintexts, "plaintexts")
        if pt_off.size != n + 1:
            raise ValueError("one plaintext per nonce")
        total = int(pt_off[-1])
        out = np.zeros(total + 16 * n, dtype=np.uint8)
        out_off = pt_off + np.arange(n + 1, dtype=np.uint64) * np.uint64(16)
        bk, bp = (ctypes.c_ubyte * max(k.size, 1))(), (ctypes.c_ubyte * max(total, 1))()
        try:
            ctypes.memmove(bk, k.ctypes.data, k.size)
            ctypes.memmove(bp, pt.ctypes.data, total)
            _check(lib().rofl_aead_seal(_sz(k.shape[0]), bk, None if rnd is None else _ptr(rnd), _sz(n), None if idx is None else _ptr(idx), _ptr(nc),
                                        _ptr(ad) if ad.size else None, _ptr(ad_off), bp if total else None, _ptr(pt_off), _ptr(out)))
        finally:
            ctypes.memset(bk, 0, ctypes.sizeof(bk))
            ctypes.memset(bp, 0, ctypes.sizeof(bp))
        if form == "packed":
            return out, out_off
        if form is None:
            raw = out.tobytes()
            return [raw[int(out_off[i]):int(out_off[i + 1])] for i in range(n)]
        return out.reshape(n, form + 16)

    @staticmethod
    def open(keys, nonces, ads, sealed, key_idx=None, derive_round=None):
        """-> (plaintexts, verdicts uint8[n]), ONE call.  Verdict 0: the tag matches; 1: it does not, and the plaintext is zeros; 2: the record
        is shorter than 16 bytes, and its plaintext is empty.  The tag is checked before anything is decrypted.  The plaintexts come in the
        form of `sealed`: a list of bytes; uint8[n, length - 16]; or, for a packed pair, (uint8[total], the same offsets) with plaintext i at
        offset[i], 16 bytes shorter than its record (the layout of the C ABI)."""
        k, nc, n, ad, ad_off, idx, rnd = aead._args(keys, nonces, ads, key_idx, derive_round)
        ct, ct_off, form = _packed(sealed, "sealed")
        if ct_off.size != n + 1:
            raise ValueError("one sealed record per nonce")
        total = int(ct_off[-1])
        pt, verdict = np.zeros(max(total, 1), dtype=np.uint8), np.zeros(n, dtype=np.uint8)
        bk = (ctypes.c_ubyte * max(k.size, 1))()
        try:
            ctypes.memmove(bk, k.ctypes.data, k.size)
            _check(lib().rofl_aead_open(_sz(k.shape[0]), bk, None if rnd is None else _ptr(rnd), _sz(n), None if idx is None else _ptr(idx), _ptr(nc),
                                        _ptr(ad) if ad.size else None, _ptr(ad_off), _ptr(ct) if total else None, _ptr(ct_off), _ptr(pt), _ptr(verdict)))
        finally:
            ctypes.memset(bk, 0, ctypes.sizeof(bk))
        if form == "packed":
            return (pt[:total], ct_off), verdict
        if form is None:
            raw = pt.tobytes()
            return [raw[int(ct_off[i]):max(int(ct_off[i + 1]) - 16, int(ct_off[i]))] for i in range(n)], verdict
        return np.ascontiguousarray(pt[:total].reshape(n, form)[:, :max(form - 16, 0)]), verdict


def _xs32(xs, n_shares):
    """evaluation points as uint32[n_shares]: nonzero, distinct, each below 2^32"""
    x = np.asarray(xs)
    if x.ndim != 1 or x.shape[0] != n_shares or x.dtype.kind not in "iu":
        raise ValueError("xs is one integer point per share")
    if n_shares and (int(x.min()) < 1 or int(x.max()) >= 2 ** 32):
        raise ValueError("an evaluation point is in [1, 2^32)")
    x = np.ascontiguousarray(x.astype(np.uint32))
    if np.unique(x).size != n_shares:
        raise ValueError("the evaluation points are distinct")
    return x


class secret_sharing:
    """Shamir sharing over the scalar field mod l (rofl_shamir_share / rofl_shamir_reconstruct), for the secrets behind a client's masks: its
    key-agreement key and its per-round self-mask secret.  A secret is 32 bytes, reduced mod l (zero is allowed); with the 32-byte coefficient
    seed c and threshold t it defines f(X) = s + sum_{k=1..t-1} a_k X^k, a_k = scalar k - 1 of the stream of c under the label
    "rofl-zk/share/v1"; the share for the point x (a nonzero uint32; client i holds x = i + 1) is f(x), canonical.  Any t shares determine
    the secret, t - 1 determine nothing.  A coefficient seed is as secret as the secret it shares.  reconstruct() checks nothing: a wrong
    share reconstructs another scalar without an error.  commit() publishes Feldman commitments of the polynomial and verify_shares() checks
    every share against them, one exact equation per share, so a wrong share is named before it is interpolated
    (rofl_feldman_commit / rofl_feldman_verify).  sign_commitments / verify_views authenticate the broadcast of the commitments, and
    seal_shares / open_shares encrypt the shares on their way under a CHANNEL key pair of their own (aead).  sign_bundles makes every
    sealed record attributable, file_complaints opens one pair's channel to a judge with a DLEQ proof (dleq), and judge_complaints rules
    who of complainant and dealer is at fault.  The transport, the round's state machine, what a round does with a convicted party and a
    dealer that sends nothing are the deployment's.  Not constant-time."""

    @staticmethod
    def share(secrets, coef_seeds, threshold, n_shares, xs=None):
        """-> uint8[n_secrets, n_shares, 32], share [s, i] = f_s(xs[i]); xs=None means the points 1 .. n_shares.  A call with a subset of the
        points returns exactly those columns of the whole call."""
        sec, seeds = _keys32(secrets, "a secret"), _keys32(coef_seeds, "a coefficient seed")
        n, threshold, n_shares = sec.shape[0], int(threshold), int(n_shares)
        if seeds.shape[0] != n:
            raise ValueError("one coefficient seed per secret")
        if n_shares < 0 or (n and not 1 <= threshold <= n_shares):
            raise ValueError("the threshold is in [1, n_shares]")
        x = None if xs is None else _xs32(xs, n_shares)
        out = np.zeros((n, n_shares, 32), dtype=np.uint8)
        bs, bc = (ctypes.c_ubyte * max(n * 32, 1))(), (ctypes.c_ubyte * max(n * 32, 1))()
        try:
            ctypes.memmove(bs, sec.ctypes.data, n * 32)
            ctypes.memmove(bc, seeds.ctypes.data, n * 32)
            _check(lib().rofl_shamir_share(_sz(n), bs, bc, _sz(threshold), _sz(n_shares), None if x is None else _ptr(x), _ptr(out)))
        finally:
            ctypes.memset(bs, 0, ctypes.sizeof(bs))
            ctypes.memset(bc, 0, ctypes.sizeof(bc))
        return out

    @staticmethod
    def reconstruct(xs, shares):
        """The secrets from shares uint8[n_secrets, len(xs), 32] at the points xs (one set for all secrets) -> uint8[n_secrets, 32].  ALL
        shares handed in are interpolated; shares that are not canonical are reduced."""
        n_shares = int(np.asarray(xs).shape[0]) if np.asarray(xs).ndim == 1 else -1
        x = _xs32(xs, n_shares)
        sh = np.asarray(shares, dtype=np.uint8)
        if sh.ndim != 3 or sh.shape[1:] != (n_shares, 32):
            raise ValueError("shares are uint8[n_secrets, len(xs), 32]")
        n = sh.shape[0]
        if n and n_shares == 0:
            raise ValueError("secrets without shares")
        out = np.zeros((n, 32), dtype=np.uint8)
        buf = (ctypes.c_ubyte * max(n * n_shares * 32, 1))()
        try:
            ctypes.memmove(buf, np.ascontiguousarray(sh).ctypes.data, n * n_shares * 32)
            _check(lib().rofl_shamir_reconstruct(_sz(n), _sz(n_shares), _ptr(x), buf, _ptr(out)))
        finally:
            ctypes.memset(buf, 0, ctypes.sizeof(buf))
        return out

    @staticmethod
    def commit(secrets, coef_seeds, threshold):
        """Feldman commitments of the polynomials share() evaluates (rofl_feldman_commit) -> uint8[n_secrets, threshold, 32]:
        [s, 0] = encode((secret mod l) B), [s, k] = encode(a_k B).  For a DH key, [s, 0] is its key_agreement.public_keys output.  The
        commitments reveal secret * B: commit only to keys and to fresh uniform secrets."""
        sec, seeds = _keys32(secrets, "a secret"), _keys32(coef_seeds, "a coefficient seed")
        n, threshold = sec.shape[0], int(threshold)
        if seeds.shape[0] != n:
            raise ValueError("one coefficient seed per secret")
        if n and threshold < 1:
            raise ValueError("the threshold is at least 1")
        out = np.zeros((n, max(threshold, 0), 32), dtype=np.uint8)
        bs, bc = (ctypes.c_ubyte * max(n * 32, 1))(), (ctypes.c_ubyte * max(n * 32, 1))()
        try:
            ctypes.memmove(bs, sec.ctypes.data, n * 32)
            ctypes.memmove(bc, seeds.ctypes.data, n * 32)
            _check(lib().rofl_feldman_commit(_sz(n), bs, bc, _sz(threshold), _ptr(out)))
        finally:
            ctypes.memset(bs, 0, ctypes.sizeof(bs))
            ctypes.memset(bc, 0, ctypes.sizeof(bc))
        return out

    @staticmethod
    def verify_shares(commitments, xs, shares):
        """Every share uint8[n_secrets, len(xs), 32] at the points xs (one set for all secrets) against the commitments
        uint8[n_secrets, t, 32] of its secret (rofl_feldman_verify) -> uint8[n_secrets, len(xs)] verdicts: 0 = consistent, 1 = not, 2 = a
        commitment of that secret is not a canonical Ristretto encoding (the whole row).  len(xs) may be below t: a client checks the one
        share it received.  A call on a subset of the secrets or of the points returns those rows or columns of the whole call."""
        n_shares = int(np.asarray(xs).shape[0]) if np.asarray(xs).ndim == 1 else -1
        x = _xs32(xs, n_shares)
        cm, sh = np.asarray(commitments, dtype=np.uint8), np.asarray(shares, dtype=np.uint8)
        if cm.ndim != 3 or cm.shape[2] != 32:
            raise ValueError("commitments are uint8[n_secrets, threshold, 32]")
        n, t = cm.shape[0], cm.shape[1]
        if sh.ndim != 3 or sh.shape != (n, n_shares, 32):
            raise ValueError("shares are uint8[n_secrets, len(xs), 32]")
        if n and n_shares == 0:
            raise ValueError("secrets without shares")
        if n and t < 1:
            raise ValueError("the threshold is at least 1")
        out = np.zeros((n, n_shares), dtype=np.uint8)
        cm, src = np.ascontiguousarray(cm), np.ascontiguousarray(sh)      # (held by name: a temporary copy would be gone before it is read)
        buf = (ctypes.c_ubyte * max(n * n_shares * 32, 1))()
        try:
            ctypes.memmove(buf, src.ctypes.data, n * n_shares * 32)
            _check(lib().rofl_feldman_verify(_sz(n), _sz(t), _ptr(cm), _sz(n_shares), _ptr(x), buf, _ptr(out)))
        finally:
            ctypes.memset(buf, 0, ctypes.sizeof(buf))
            if src is not sh:
                src[...] = 0
        return out

    # ---- the authenticated broadcast of the commitments: what a round signs (signatures.sign / verify) ----
    @staticmethod
    def commitment_message(round_no, dealer, kind, commitments):
        """The bytes a dealer signs for one of its two commitment rows (kind 0 = its key's, 1 = its self-mask secret's):
        b"rofl-zk/vss/v1\\0\\0" || u64le(round_no) || u32le(dealer) || u8(kind) || u32le(t) || commitments (t x 32)."""
        cm = np.ascontiguousarray(np.asarray(commitments, dtype=np.uint8))
        if cm.ndim != 2 or cm.shape[1] != 32 or cm.shape[0] < 1:
            raise ValueError("the commitments of dealer %d are uint8[t, 32]" % int(dealer))
        if int(kind) not in (0, 1):
            raise ValueError("kind is 0 (key) or 1 (self)")
        return b"rofl-zk/vss/v1\0\0" + struct.pack("<QIBI", int(round_no), int(dealer), int(kind), cm.shape[0]) + cm.tobytes()

    @staticmethod
    def view_message(round_no, sigs_by_dealer):
        """The bytes a client signs for everything it was shown: sigs_by_dealer = {dealer: uint8[2, 64]}, the dealer's key and self signatures.
        b"rofl-zk/view/v1\\0" || u64le(round_no) || u32le(count), then for each dealer ascending u32le(dealer) || key sig || self sig.
        Signatures are deterministic and bind their message: two clients who saw the same commitments build the same bytes."""
        parts = [b"rofl-zk/view/v1\0" + struct.pack("<QI", int(round_no), len(sigs_by_dealer))]
        for d in sorted(int(k) for k in sigs_by_dealer):
            s = np.asarray(sigs_by_dealer[d], dtype=np.uint8)
            if s.shape != (2, 64):
                raise ValueError("the signatures of dealer %d are uint8[2, 64]" % d)
            parts.append(struct.pack("<I", d) + s.tobytes())
        return b"".join(parts)

    @staticmethod
    def _commitment_messages(round_no, dealers, key_commitments, self_commitments):
        dealers = [int(d) for d in dealers]
        if len(key_commitments) != len(dealers) or len(self_commitments) != len(dealers):
            raise ValueError("one row of key commitments and one of self commitments per dealer")
        msgs = []
        for r, d in enumerate(dealers):
            msgs.append(secret_sharing.commitment_message(round_no, d, 0, key_commitments[r]))
            msgs.append(secret_sharing.commitment_message(round_no, d, 1, self_commitments[r]))
        return msgs, [(r, 2 * r + k) for r in range(len(dealers)) for k in (0, 1)]

    @staticmethod
    def sign_commitments(sig_sks, round_no, dealers, key_commitments, self_commitments):
        """Every hosted dealer signs its two commitment messages, ONE signatures.sign call: sig_sks[r] is the signing key of dealers[r],
        key_commitments[r] / self_commitments[r] its rows uint8[t, 32].  -> uint8[n, 2, 64], [r, 0] on the key row, [r, 1] on the self row."""
        msgs, refs = secret_sharing._commitment_messages(round_no, dealers, key_commitments, self_commitments)
        if _keys32(sig_sks, "a secret key").shape[0] != len(msgs) // 2:
            raise ValueError("one signing key per dealer")
        return signatures.sign(sig_sks, msgs, refs).reshape(-1, 2, 64)

    @staticmethod
    def verify_commitment_signatures(sig_pks, round_no, dealers, key_commitments, self_commitments, sigs):
        """The signatures sigs uint8[n, 2, 64] of sign_commitments under the dealers' public signing keys sig_pks[r], ONE signatures.verify
        call -> uint8[n, 2] verdicts."""
        msgs, refs = secret_sharing._commitment_messages(round_no, dealers, key_commitments, self_commitments)
        if _keys32(sig_pks, "a public key").shape[0] != len(msgs) // 2:
            raise ValueError("one public signing key per dealer")
        sg = np.asarray(sigs, dtype=np.uint8)
        if sg.shape != (len(msgs) // 2, 2, 64):
            raise ValueError("sigs are uint8[n, 2, 64]")
        return signatures.verify(sig_pks, msgs, sg.reshape(-1, 64), refs).reshape(-1, 2)

    @staticmethod
    def verify_views(sig_pks, view, view_sigs):
        """n clients' signatures view_sigs uint8[n, 64] on ONE view message (view_message) under their public signing keys, ONE
        signatures.verify call with refs (i, 0) -> uint8[n].  A client whose verdict is nonzero saw something else than `view`, or its
        dealer equivocated: the verdict names it."""
        n = _keys32(sig_pks, "a public key").shape[0]
        return signatures.verify(sig_pks, [bytes(view)], view_sigs, [(i, 0) for i in range(n)])

    # ---- the second view round: the same broadcast behind a Merkle root (merkle.build / verify), so that 60 bytes are signed whatever the number
    # of dealers, a client that holds only some dealers' entries checks them against what everybody signed, and two views that differ are
    # settled with one entry and its path ----
    @staticmethod
    def view_leaf(round_no, dealer, sigs2x64):
        """The leaf of one dealer in the view tree, 156 bytes: b"rofl-zk/view/v2\\0" || u64le(round_no) || u32le(dealer) || key sig || self sig."""
        s = np.asarray(sigs2x64, dtype=np.uint8)
        if s.shape != (2, 64):
            raise ValueError("the signatures of dealer %d are uint8[2, 64]" % int(dealer))
        return b"rofl-zk/view/v2\0" + struct.pack("<QI", int(round_no), int(dealer)) + s.tobytes()

    @staticmethod
    def view_tree(round_no, sigs_by_dealer, paths_for=None):
        """The view of sigs_by_dealer = {dealer: uint8[2, 64]} as a tree, ONE merkle.build call: the leaves are the dealers' view_leaf in
        ascending dealer order.  -> (root uint8[32], dealers_sorted); with paths_for (a list of DEALERS) also their paths
        uint8[k, depth(count), 32].  The leaf index of a dealer is its position in dealers_sorted."""
        dealers = sorted(int(k) for k in sigs_by_dealer)
        leaves = [secret_sharing.view_leaf(round_no, d, sigs_by_dealer[d]) for d in dealers]
        if paths_for is None:
            return merkle.build(leaves), dealers
        pos = {d: i for i, d in enumerate(dealers)}
        if any(int(d) not in pos for d in paths_for):
            raise ValueError("a path is asked for a dealer that is not in the view")
        root, paths = merkle.build(leaves, paths_for=[pos[int(d)] for d in paths_for])
        return root, dealers, paths

    @staticmethod
    def view_root_message(round_no, count, root):
        """The bytes a client signs for the tree of everything it was shown, 60 bytes:
        b"rofl-zk/view/v2r" || u64le(round_no) || u32le(count) || root."""
        r = bytes(root) if isinstance(root, (bytes, bytearray, memoryview)) else np.asarray(root, dtype=np.uint8).tobytes()
        if len(r) != 32:
            raise ValueError("a root is 32 bytes")
        return b"rofl-zk/view/v2r" + struct.pack("<QI", int(round_no), int(count)) + r

    @staticmethod
    def sign_view_root(sig_sks, round_no, count, roots):
        """Every hosted client signs the view_root_message of ITS root (roots uint8[n, 32]; clients may have been shown different things), ONE
        signatures.sign call -> uint8[n, 64]."""
        rt = _keys32(roots, "a root")
        if _keys32(sig_sks, "a secret key").shape[0] != rt.shape[0]:
            raise ValueError("one root per signing key")
        return signatures.sign(sig_sks, [secret_sharing.view_root_message(round_no, count, r) for r in rt])

    @staticmethod
    def verify_view_roots(sig_pks, round_no, count, root, view_sigs):
        """n clients' signatures view_sigs uint8[n, 64] on the view_root_message of ONE root under their public signing keys, ONE
        signatures.verify call with refs (i, 0) -> uint8[n].  A client whose verdict is nonzero signed another root: it was shown something
        else, or its dealer equivocated; the verdict names it, as verify_views does."""
        n = _keys32(sig_pks, "a public key").shape[0]
        return signatures.verify(sig_pks, [secret_sharing.view_root_message(round_no, count, root)], view_sigs, [(i, 0) for i in range(n)])

    @staticmethod
    def verify_view_entries(round_no, root, count, positions, entries, paths):
        """What a client that holds only some dealers' signature pairs checks against the root everybody signed, ONE merkle.verify call:
        entries = [(dealer, uint8[2, 64]), ...], positions[i] the leaf index of entry i (the dealer's position among the round's dealers in
        ascending order), paths uint8[k, stride, 32] -> uint8[k] verdicts, 0 = the entry is in the tree of `root` with `count` leaves."""
        leaves = [secret_sharing.view_leaf(round_no, d, s) for d, s in entries]
        pos = [int(p) for p in positions]
        if len(pos) != len(leaves):
            raise ValueError("one position per entry")
        return merkle.verify([root], [int(count)], paths, messages=leaves, refs=[(0, p) for p in pos])

    @staticmethod
    def differing_view_entries(round_no, sigs_a, sigs_b):
        """The dealers whose leaves differ between two views {dealer: uint8[2, 64]}, ascending: a dealer in only one of them, or with other
        signatures -- what to ask paths for when two signed roots differ.  Plain Python."""
        out = []
        for d in sorted(set(int(k) for k in sigs_a) | set(int(k) for k in sigs_b)):
            if d not in sigs_a or d not in sigs_b or secret_sharing.view_leaf(round_no, d, sigs_a[d]) != secret_sharing.view_leaf(round_no, d, sigs_b[d]):
                out.append(d)
        return out

    # ---- the shares on their way: every bundle sealed under the pair's channel key of the round (aead.seal / open) ----
    # A client has THREE key pairs: the mask key (key_agreement; Shamir-shared, and RECONSTRUCTED by the server when its owner drops out), the
    # signing key (signatures) and the CHANNEL key used here, which is never shared and never revealed.  Were the bundles sealed under a key
    # derived from the mask keys' shared secret, reconstructing a dropped client's mask key would open every bundle ever sealed to or from it.
    @staticmethod
    def bundle_nonce(sender, recipient):
        """u32le(sender) || u32le(recipient) || u32le(0), 12 bytes: unique per direction under a pair's key of ONE round (the key is derived
        per round, aead's derive_round), and one bundle goes each way per round."""
        return struct.pack("<III", int(sender), int(recipient), 0)

    @staticmethod
    def bundle_ad(round_no, sender, recipient):
        """b"rofl-zk/shares/1" || u64le(round_no) || u32le(sender) || u32le(recipient), 32 bytes: what a bundle is bound to"""
        return b"rofl-zk/shares/1" + struct.pack("<QII", int(round_no), int(sender), int(recipient))

    @staticmethod
    def _bundle_keys(channel_sks, own_ids, peer_ids, peer_channel_pks, round_no, own_sends):
        """The pairs of a seal_shares / open_shares call, own-major: (shared secrets uint8[n, 32], nonces uint8[n, 12], ADs uint8[n, 32], the
        flat indices of the pairs with own id != peer id, n_own, n_peer); ONE rofl_dh_shared call.  own_sends: the own client is the sender."""
        own, peer = np.asarray(own_ids, dtype=np.uint32).reshape(-1), np.asarray(peer_ids, dtype=np.uint32).reshape(-1)
        sk, pk = _keys32(channel_sks, "a channel secret key"), _keys32(peer_channel_pks, "a channel public key")
        if sk.shape[0] != own.size or pk.shape[0] != peer.size:
            raise ValueError("one channel secret key per own id and one channel public key per peer id")
        n_own, n_peer = own.size, peer.size
        o, p = np.repeat(own, n_peer), np.tile(peer, n_own)
        keep = np.flatnonzero(o != p)
        secrets, status = key_agreement.shared_secrets(sk, pk)
        bad = keep[status[keep] != 0]
        if bad.size:
            secrets[...] = 0
            raise ValueError("peer %d: its channel public key is refused (status %d): no key is derived from it" % (int(p[bad[0]]), int(status[bad[0]])))
        snd, rcp = (o, p) if own_sends else (p, o)
        nonces = np.zeros((o.size, 3), dtype="<u4")
        nonces[:, 0], nonces[:, 1] = snd, rcp
        ads = np.zeros((o.size, 32), dtype=np.uint8)
        ads[:, :16] = np.frombuffer(b"rofl-zk/shares/1", dtype=np.uint8)
        ads[:, 16:24] = np.frombuffer(struct.pack("<Q", int(round_no)), dtype=np.uint8)
        ads[:, 24:28], ads[:, 28:32] = snd.astype("<u4").view(np.uint8).reshape(-1, 4), rcp.astype("<u4").view(np.uint8).reshape(-1, 4)
        return secrets, nonces.view(np.uint8).reshape(-1, 12), ads, keep, n_own, n_peer

    @staticmethod
    def seal_shares(channel_sks, own_ids, peer_ids, peer_channel_pks, round_no, key_shares, self_shares):
        """Every hosted dealer seals its share bundles for all peers: ONE key_agreement.shared_secrets call and ONE aead.seal call.
        channel_sks[a] is the CHANNEL secret key of dealer own_ids[a] (not its mask key, not its signing key), peer_channel_pks[b] the channel
        public key of peer_ids[b]; key_shares / self_shares are uint8[n_own, n_peer, 32], [a, b] dealer own_ids[a]'s share for peer_ids[b].
        The payload is key share || self share (64 bytes), the key the pair's shared secret under derive_round = round_no, the nonce
        bundle_nonce(sender, recipient), the AD bundle_ad(round_no, sender, recipient).  -> uint8[n_own, n_peer, 80]; the record of a pair
        with own id == peer id is zeros.  A peer whose channel key is not a canonical encoding or is the identity raises ValueError naming
        it.  The shared secrets held here are zeroed before the call returns."""
        secrets, nonces, ads, keep, n_own, n_peer = secret_sharing._bundle_keys(channel_sks, own_ids, peer_ids, peer_channel_pks, round_no, True)
        ks, payload = secrets[keep], None
        try:
            k, s = np.asarray(key_shares, dtype=np.uint8), np.asarray(self_shares, dtype=np.uint8)
            if k.shape != (n_own, n_peer, 32) or s.shape != (n_own, n_peer, 32):
                raise ValueError("key_shares and self_shares are uint8[n_own, n_peer, 32]")
            payload = np.concatenate([k, s], axis=2).reshape(-1, 64)[keep]
            out = np.zeros((n_own * n_peer, 80), dtype=np.uint8)
            out[keep] = aead.seal(ks, nonces[keep], ads[keep], payload, derive_round=round_no)
        finally:
            secrets[...] = 0
            ks[...] = 0
            if payload is not None:
                payload[...] = 0
        return out.reshape(n_own, n_peer, 80)

    @staticmethod
    def open_shares(channel_sks, own_ids, peer_ids, peer_channel_pks, round_no, records):
        """Every hosted client opens what it was sent: records uint8[n_own, n_peer, 80], [a, b] what peer_ids[b] sealed for own_ids[a]; ONE
        key_agreement.shared_secrets call and ONE aead.open call.  -> (key_shares, self_shares uint8[n_own, n_peer, 32], verdicts
        uint8[n_own, n_peer]): verdict 1 names a bundle that was changed on the way, sealed for somebody else, by somebody else or for another
        round; its shares are zeros.  The pair with own id == peer id is skipped: verdict 0 and zero shares.  A refused channel key raises
        ValueError naming the peer.  The shared secrets held here are zeroed before the call returns."""
        secrets, nonces, ads, keep, n_own, n_peer = secret_sharing._bundle_keys(channel_sks, own_ids, peer_ids, peer_channel_pks, round_no, False)
        ks = secrets[keep]
        try:
            rec = np.asarray(records, dtype=np.uint8)
            if rec.shape != (n_own, n_peer, 80):
                raise ValueError("records are uint8[n_own, n_peer, 80]")
            pt, v = aead.open(ks, nonces[keep], ads[keep], np.ascontiguousarray(rec.reshape(-1, 80)[keep]), derive_round=round_no)
        finally:
            secrets[...] = 0
            ks[...] = 0
        shares, verdict = np.zeros((n_own * n_peer, 64), dtype=np.uint8), np.zeros(n_own * n_peer, dtype=np.uint8)
        shares[keep], verdict[keep] = pt, v
        shares = shares.reshape(n_own, n_peer, 64)
        return np.ascontiguousarray(shares[:, :, :32]), np.ascontiguousarray(shares[:, :, 32:]), verdict.reshape(n_own, n_peer)

    # ---- a complaint against a dealer: the dealer SIGNS every sealed record, the complainant opens the pair's channel to a judge (dleq) ----
    # A client whose opened share fails verify_shares can name the dealer, but nobody else can check the claim: the record is sealed under a
    # key only the two hold.  With the dealer's signature on the record the complainant can reveal the pair's DH point with a proof that it
    # is the right one (file_complaints), and anyone re-derives the key, opens the signed record and runs the Feldman check
    # (judge_complaints).  The reveal opens that pair's channel in BOTH directions for the whole epoch of the channel keys: the judge learns
    # one share of each of the two clients' secrets per round, and the pair re-keys afterwards.
    @staticmethod
    def bundle_message(round_no, sender, recipient, record):
        """The bytes a dealer signs for one sealed record: b"rofl-zk/sealed/1" || u64le(round_no) || u32le(sender) || u32le(recipient) ||
        record (80 bytes), 112 bytes"""
        rec = np.ascontiguousarray(np.asarray(record, dtype=np.uint8)).reshape(-1)
        if rec.size != 80:
            raise ValueError("a sealed record is 80 bytes")
        return b"rofl-zk/sealed/1" + struct.pack("<QII", int(round_no), int(sender), int(recipient)) + rec.tobytes()

    @staticmethod
    def _bundle_messages(round_no, own_ids, peer_ids, records):
        own, peer = [int(i) for i in own_ids], [int(i) for i in peer_ids]
        rec = np.asarray(records, dtype=np.uint8)
        if rec.shape != (len(own), len(peer), 80):
            raise ValueError("records are uint8[n_own, n_peer, 80]")
        msgs = [secret_sharing.bundle_message(round_no, o, p, rec[a, b]) for a, o in enumerate(own) for b, p in enumerate(peer)]
        return msgs, [(a, a * len(peer) + b) for a in range(len(own)) for b in range(len(peer))]

    @staticmethod
    def sign_bundles(sig_sks, round_no, own_ids, peer_ids, records):
        """Every hosted dealer signs the records it sealed (seal_shares' output uint8[n_own, n_peer, 80]), ONE signatures.sign call:
        sig_sks[a] is the SIGNING key of dealer own_ids[a].  -> uint8[n_own, n_peer, 64].  The signature is what makes a record
        attributable: a record without a valid one is a missing record, not grounds for a complaint."""
        msgs, refs = secret_sharing._bundle_messages(round_no, own_ids, peer_ids, records)
        if _keys32(sig_sks, "a secret key").shape[0] != len(own_ids):
            raise ValueError("one signing key per own id")
        return signatures.sign(sig_sks, msgs, refs).reshape(len(own_ids), len(peer_ids), 64)

    @staticmethod
    def verify_bundle_signatures(sig_pks, round_no, own_ids, peer_ids, records, sigs):
        """The signatures sigs uint8[n_own, n_peer, 64] of sign_bundles under the senders' public signing keys sig_pks[a] (sender own_ids[a],
        recipient peer_ids[b]), ONE signatures.verify call -> uint8[n_own, n_peer] verdicts.  A recipient checks these on receipt."""
        msgs, refs = secret_sharing._bundle_messages(round_no, own_ids, peer_ids, records)
        if _keys32(sig_pks, "a public key").shape[0] != len(own_ids):
            raise ValueError("one public signing key per own id")
        sg = np.asarray(sigs, dtype=np.uint8)
        if sg.shape != (len(own_ids), len(peer_ids), 64):
            raise ValueError("sigs are uint8[n_own, n_peer, 64]")
        return signatures.verify(sig_pks, msgs, sg.reshape(-1, 64), refs).reshape(len(own_ids), len(peer_ids))

    @staticmethod
    def complaint_context(round_no, complainant, dealer):
        """SHA3-256(b"rofl-zk/complain" || u64le(round_no) || u32le(complainant) || u32le(dealer)), 32 bytes: what binds a complaint's proof
        to its round and its two parties (computed on the host, like the self-mask seed)"""
        return hashlib.sha3_256(b"rofl-zk/complain" + struct.pack("<QII", int(round_no), int(complainant), int(dealer))).digest()

    @staticmethod
    def file_complaints(channel_sks, own_ids, dealer_ids, dealer_channel_pks, round_no, which):
        """The hosted clients' complaints which = [(own id, dealer id), ...], ONE dleq.prove call: channel_sks[a] is the CHANNEL secret key of
        own_ids[a], dealer_channel_pks[b] the channel public key of dealer_ids[b].  -> (reveals uint8[n, 32], proofs uint8[n, 64]), one per
        entry of `which`, bound to complaint_context(round_no, own id, dealer id).  A refused dealer key raises ValueError naming the dealer."""
        own, dealers = [int(i) for i in own_ids], [int(i) for i in dealer_ids]
        which = [(int(o), int(d)) for o, d in which]
        for o, d in which:
            if o not in own or d not in dealers:
                raise ValueError("complaint (%d, %d) names a client that is not in the call" % (o, d))
        pairs = [(own.index(o), dealers.index(d)) for o, d in which]
        ctxs = np.frombuffer(b"".join(secret_sharing.complaint_context(round_no, o, d) for o, d in which), dtype=np.uint8).reshape(-1, 32)
        reveals, proofs, status = dleq.prove(channel_sks, dealer_channel_pks, ctxs, pairs)
        if status.any():
            i = int(np.flatnonzero(status)[0])
            raise ValueError("dealer %d: its channel public key is refused (status %d): nothing is revealed against it" % (which[i][1], int(status[i])))
        return reveals, proofs

    @staticmethod
    def judge_complaints(round_no, complaints, channel_pks, sig_pks, key_commitments, self_commitments):
        """Rule on complaints = [(complainant, dealer, record, record_sig, reveal, proof), ...]: the 80-byte record the dealer sent, the
        dealer's signature on it (sign_bundles), and the complainant's reveal and proof (file_complaints).  channel_pks, sig_pks,
        key_commitments and self_commitments are indexed by client id (arrays or dicts); the commitments were signature-checked earlier.
        Exactly ONE call each of signatures.verify, dleq.verify, aead.open (on the shared secrets that came back, derive_round = round_no)
        and verify_shares (the dealers and the points complainant + 1 that occur; grid entries no complaint names are ignored).
        -> [(at_fault, reason), ...] per complaint, the first that applies:
          4  the record's signature does not verify under the dealer's signing key        -> the complainant
          3  the DLEQ verdict is 1 or 2                                                   -> the complainant
          1  the record does not open under the proven key                                -> the dealer
          0  a share of the opened bundle is inconsistent with the dealer's commitments   -> the dealer
          2  the record opens and both shares are consistent                              -> the complainant
        A commitment row with verdict 2 raises ValueError naming the dealer.  The shared secrets and opened shares held here are zeroed
        before the call returns."""
        cs = [(int(c[0]), int(c[1])) for c in complaints]
        n = len(cs)
        if n == 0:
            return []
        if len(set(cs)) != n:
            raise ValueError("two complaints name the same (complainant, dealer): one record per pair and round")
        rec = np.stack([np.asarray(c[2], dtype=np.uint8).reshape(-1) for c in complaints])
        if rec.shape != (n, 80):
            raise ValueError("a sealed record is 80 bytes")
        row = lambda table, i: np.asarray(table[i], dtype=np.uint8)      # noqa: E731
        sig_v = signatures.verify(np.stack([row(sig_pks, d) for _, d in cs]), [secret_sharing.bundle_message(round_no, d, c, rec[i]) for i, (c, d) in enumerate(cs)],
                                  np.stack([np.asarray(c[3], dtype=np.uint8).reshape(-1) for c in complaints]))
        ctxs = np.frombuffer(b"".join(secret_sharing.complaint_context(round_no, c, d) for c, d in cs), dtype=np.uint8).reshape(-1, 32)
        proof_v, shared = dleq.verify(np.stack([row(channel_pks, c) for c, _ in cs]), np.stack([row(channel_pks, d) for _, d in cs]), ctxs,
                                      np.stack([np.asarray(c[4], dtype=np.uint8).reshape(-1) for c in complaints]),
                                      np.stack([np.asarray(c[5], dtype=np.uint8).reshape(-1) for c in complaints]), [(i, i) for i in range(n)])
        opened = shares = None
        try:
            nonces = np.frombuffer(b"".join(secret_sharing.bundle_nonce(d, c) for c, d in cs), dtype=np.uint8).reshape(-1, 12)
            ads = np.frombuffer(b"".join(secret_sharing.bundle_ad(round_no, d, c) for c, d in cs), dtype=np.uint8).reshape(-1, 32)
            opened, open_v = aead.open(shared, nonces, ads, rec, derive_round=round_no)
            dealers, points = sorted({d for _, d in cs}), sorted({c + 1 for c, _ in cs})
            com = np.stack([row(key_commitments, d) for d in dealers] + [row(self_commitments, d) for d in dealers])
            shares = np.zeros((2 * len(dealers), len(points), 32), dtype=np.uint8)
            at = [(dealers.index(d), points.index(c + 1)) for c, d in cs]
            for i, (r, x) in enumerate(at):
                shares[r, x], shares[len(dealers) + r, x] = opened[i, :32], opened[i, 32:]
            share_v = secret_sharing.verify_shares(com, points, shares)
            refused = np.flatnonzero((share_v == 2).any(axis=1))
            if refused.size:
                raise ValueError("dealer %d: a commitment of its %s row is not a canonical encoding" % (dealers[int(refused[0]) % len(dealers)],
                                                                                                      "key" if refused[0] < len(dealers) else "self"))
            out = []
            for i, (c, d) in enumerate(cs):
                r, x = at[i]
                if sig_v[i]:
                    out.append((c, 4))
                elif proof_v[i]:
                    out.append((c, 3))
                elif open_v[i]:
                    out.append((d, 1))
                elif share_v[r, x] or share_v[len(dealers) + r, x]:
                    out.append((d, 0))
                else:
                    out.append((c, 2))
            return out
        finally:
            shared[...] = 0
            for a in (opened, shares):
                if a is not None:
                    a[...] = 0


class pedersen_ops:
    @staticmethod
    def commit_vec(scalars, blindings):
        s, b = _u8(scalars), _u8(blindings)
        assert s.shape == b.shape
        out = np.zeros_like(s)
        _check(lib().rofl_commit_vec(_ptr(s), _ptr(b), _sz(s.shape[0]), _ptr(out)))
        return out

    @staticmethod
    def commit_no_blinding_vec(scalars):
        s = _u8(scalars)
        out = np.zeros_like(s)
        _check(lib().rofl_commit_vec(_ptr(s), None, _sz(s.shape[0]), _ptr(out)))
        return out

    @staticmethod
    def add_rp_vec(a, b):
        a, b = _u8(a), _u8(b)
        assert a.shape == b.shape
        out = np.zeros_like(a)
        _check(lib().rofl_add_points_vec(_ptr(a), _ptr(b), _sz(a.shape[0]), _ptr(out)))
        return out

    @staticmethod
    def add_rp_vec_vec(vecs):
        acc = pedersen_ops.zero_rp_vec(_u8(vecs[0]).shape[0])
        for v in vecs:
            acc = pedersen_ops.add_rp_vec(acc, v)
        return acc

    @staticmethod
    def sum_rp_vec(points):
        """Iterator::sum over RistrettoPoints (params.rs:220, 277)."""
        p = _u8(points)
        out = np.zeros(32, dtype=np.uint8)
        _check(lib().rofl_sum_points(_ptr(p), _sz(p.shape[0]), _sz(32), _ptr(out)))
        return out

    @staticmethod
    def rnd_scalar_vec(length):
        """pedersen_ops.rs:124-127: Scalar::random = 64 uniform bytes reduced mod l (host RNG, as the reference's thread_rng)."""
        L = 2 ** 252 + 27742317777372353535851937790883648493
        raw = os.urandom(64 * length)
        out = np.zeros((length, 32), dtype=np.uint8)
        for i in range(length):
            out[i] = np.frombuffer((int.from_bytes(raw[64 * i:64 * i + 64], "little") % L).to_bytes(32, "little"), dtype=np.uint8)
        return out

    @staticmethod
    def add_scalar_vec(a, b, subtract=False):
        """pedersen_ops.rs:78-81 (out of place)."""
        a, b = _u8(a), _u8(b)
        assert a.shape == b.shape
        out = np.zeros_like(a)
        _check(lib().rofl_scalar_add_vec(_ptr(a), _ptr(b), _sz(a.shape[0]), int(bool(subtract)), _ptr(out)))
        return out

    @staticmethod
    def add_scalar_vec_vec(vecs):
        """pedersen_ops.rs:83-91."""
        acc = pedersen_ops.zero_scalar_vec(_u8(vecs[0]).shape[0])
        for v in vecs:
            acc = pedersen_ops.add_scalar_vec(acc, v)
        return acc

    @staticmethod
    def generate_cancelling_scalar_vec(n_vec, n_dim):
        """pedersen_ops.rs:110-122: n_vec random scalar vectors whose element-wise sum is zero."""
        vecs = [pedersen_ops.rnd_scalar_vec(n_dim) for _ in range(n_vec)]
        vecs[-1] = pedersen_ops.add_scalar_vec(pedersen_ops.zero_scalar_vec(n_dim), pedersen_ops.add_scalar_vec_vec(vecs[:-1]), subtract=True)
        return vecs

    # ---- blinding vectors from seeds (rofl_blinding_vecs): one kernel launch per call, whatever the number of vectors and terms ----
    @staticmethod
    def blinding_vecs(term_lists, d, first=0, out=None):
        """rofl_blinding_vecs: vector v = sum over term_lists[v] = [(seed32, sign), ...] of sign * stream(seed)[first .. first + d) mod l, where
        scalar k of a seed's stream is SHAKE256("rofl-zk/blind/v1" || seed || u64le(k >> 1))[64 (k & 1) .. + 64] reduced mod l.  All vectors
        are ONE launch.  out=None returns one (n_vec, d, 32) uint8 array; otherwise `out` lists one destination per vector, written in
        place: a contiguous uint8 numpy array of d * 32 bytes, or a torch uint8 tensor / a pointer (int) on the library's GPU (16-byte
        aligned; nothing crosses PCIe), and the list is returned.  A sign other than +1 / -1 raises ValueError."""
        n, d, first = len(term_lists), int(d), int(first)
        if d < 0 or first < 0:
            raise ValueError("d and first are not negative")
        counts = (_sz * max(n, 1))()
        keep, tp = [], (ctypes.c_void_p * max(n, 1))()
        for v, terms in enumerate(term_lists):
            arr = (_BlindTerm * max(len(terms), 1))()
            for t, (seed, sign) in enumerate(terms):
                seed = bytes(seed)
                if len(seed) != 32:
                    raise ValueError("a seed is 32 bytes")
                if sign not in (1, -1):
                    raise ValueError("a term's sign is +1 or -1")
                ctypes.memmove(arr[t].seed, seed, 32)
                arr[t].sign = int(sign)
            counts[v] = len(terms)
            keep.append(arr)
            tp[v] = ctypes.addressof(arr)
        if out is None:
            res = np.empty((n, d, 32), dtype=np.uint8)      # every byte is written by the call (n * d * 32 of them: no zeroing pass in front)
            dst = [res[v] for v in range(n)]
        else:
            res = dst = list(out)
            if len(dst) != n:
                raise ValueError("one destination per vector")
        op = (ctypes.c_void_p * max(n, 1))()
        for v, o in enumerate(dst):
            if _is_dev(o):
                if not o.is_contiguous() or o.element_size() != 1 or o.numel() < d * 32:
                    raise ValueError("a device destination is a contiguous uint8 tensor of d * 32 bytes")
                op[v] = o.data_ptr()
            elif isinstance(o, int):
                op[v] = o
            else:
                if not (isinstance(o, np.ndarray) and o.dtype == np.uint8 and o.flags.c_contiguous and o.flags.writeable and o.size >= d * 32):
                    raise ValueError("a host destination is a writable contiguous uint8 array of d * 32 bytes")
                op[v] = o.ctypes.data
        try:
            _check(lib().rofl_blinding_vecs(_sz(n), counts, tp, _sz(first), _sz(d), op))
        finally:
            for arr in keep:
                ctypes.memset(arr, 0, ctypes.sizeof(arr))
        return res

    @staticmethod
    def rnd_scalar_vec_seeded(length, seed, first=0, out=None):
        """pedersen_ops.rs:124-127 with the randomness an explicit input: scalars [first, first + length) of the blinding stream of `seed`
        (blinding_vecs with one +1 term).  -> uint8[length, 32], or `out` (host array / device tensor) written in place."""
        if out is None:
            return pedersen_ops.blinding_vecs([[(seed, 1)]], length, first)[0]
        pedersen_ops.blinding_vecs([[(seed, 1)]], length, first, out=[out])
        return out

    @staticmethod
    def cancelling_vec_seed(seed, i):
        """seed of vector i of generate_cancelling_scalar_vec_seeded: SHA3-256("rofl-zk/blind/v1/vec" || seed || u32le(i))"""
        return hashlib.sha3_256(b"rofl-zk/blind/v1/vec" + bytes(seed) + struct.pack("<I", int(i))).digest()

    @staticmethod
    def generate_cancelling_scalar_vec_seeded(n_vec, n_dim, seed):
        """pedersen_ops.rs:110-122 from one seed, as ONE rofl_blinding_vecs call: vector i < n_vec - 1 is the stream of
        seed_i = SHA3-256("rofl-zk/blind/v1/vec" || seed || u32le(i)), the last vector is minus their sum (n_vec = 1: the zero vector).
        -> list of n_vec uint8[n_dim, 32] arrays whose element-wise sum is zero mod l."""
        n_vec = int(n_vec)
        if n_vec < 1 or len(bytes(seed)) != 32:
            raise ValueError("n_vec >= 1 and a 32-byte seed")
        seeds = [pedersen_ops.cancelling_vec_seed(seed, i) for i in range(n_vec - 1)]
        res = pedersen_ops.blinding_vecs([[(s, 1)] for s in seeds] + [[(s, -1) for s in seeds]], n_dim)
        return [res[v] for v in range(n_vec)]

    @staticmethod
    def _pairwise_terms(index, peers):
        terms = []
        for peer_index, shared_seed in peers:
            if int(peer_index) == int(index):
                raise ValueError("a client is not its own peer")
            terms.append((shared_seed, 1 if int(index) < int(peer_index) else -1))
        return terms

    @staticmethod
    def pairwise_blinding_vec(index, peers, d, first=0, out=None):
        """Dealer-free cancelling blindings: client `index` shares a seed with every peer, peers = [(peer_index, shared_seed32), ...], and its
        vector is sum_j +-stream(s_ij)[first .. first + d) with + where index < peer_index, - otherwise -- the vectors of all clients of a
        round sum to zero, and the sum of the remaining ones after a dropout is minus the vector of the client that left.  A seed serves ONE
        round (pairwise_round_seed derives per-round seeds from a long-lived shared secret)."""
        terms = pedersen_ops._pairwise_terms(index, peers)
        if out is None:
            return pedersen_ops.blinding_vecs([terms], d, first)[0]
        pedersen_ops.blinding_vecs([terms], d, first, out=[out])
        return out

    @staticmethod
    def pairwise_blinding_vecs(clients, d):
        """pairwise_blinding_vec for a process that hosts several clients, clients = [(index, peers), ...]: ONE call -> uint8[n, d, 32]"""
        return pedersen_ops.blinding_vecs([pedersen_ops._pairwise_terms(i, peers) for i, peers in clients], d)

    # ---- double masking: the pairwise vector plus the stream of a per-round self-mask, so that a revealed key does not open a late update ----
    @staticmethod
    def self_mask_seed(b, round_no):
        """SHA3-256("rofl-zk/blind/v1/self" || canonical32(b mod l) || u64le(round_no)): the seed of a client's self-mask from its self-mask
        secret b (32 bytes, read little-endian and reduced mod l as the sharing reduces it).  b is revealed for every SURVIVOR of a round
        (dropout_residual_terms), so a secret serves ONE round whatever round_no says: draw a fresh one each round."""
        b = bytes(b)
        if len(b) != 32:
            raise ValueError("a self-mask secret is 32 bytes")
        canon = (int.from_bytes(b, "little") % (2 ** 252 + 27742317777372353535851937790883648493)).to_bytes(32, "little")
        return hashlib.sha3_256(b"rofl-zk/blind/v1/self" + canon + struct.pack("<Q", int(round_no))).digest()

    @staticmethod
    def double_masked_blinding_vec(index, peers, self_secret, round_no, d, first=0, out=None):
        """pairwise_blinding_vec plus +stream(self_mask_seed(self_secret, round_no)): the pairwise masks still cancel over a whole round, the
        self-masks never do -- every round ends with dropout_residual_terms, which needs the self secrets of the clients in the sum."""
        terms = pedersen_ops._pairwise_terms(index, peers) + [(pedersen_ops.self_mask_seed(self_secret, round_no), 1)]
        if out is None:
            return pedersen_ops.blinding_vecs([terms], d, first)[0]
        pedersen_ops.blinding_vecs([terms], d, first, out=[out])
        return out

    @staticmethod
    def double_masked_blinding_vecs(clients, round_no, d):
        """double_masked_blinding_vec for a process that hosts several clients, clients = [(index, peers, self_secret), ...]: ONE call
        -> uint8[n, d, 32]"""
        return pedersen_ops.blinding_vecs([pedersen_ops._pairwise_terms(i, peers) + [(pedersen_ops.self_mask_seed(b, round_no), 1)]
                                           for i, peers, b in clients], d)

    # ---- the seeds from key agreement (key_agreement.shared_secrets): one Diffie-Hellman call for every hosted client ----
    @staticmethod
    def pairwise_peers_from_keys(index=None, sk=None, public_keys=None, round_no=None, clients=None):
        """The `peers` list [(j, seed_ij), ...] pairwise_blinding_vec takes, for every j != index of the round, from client `index`'s secret key
        and the round's public keys (uint8[n, 32], row j = client j): seed_ij = pairwise_round_seed(shared secret of the pair, round_no).
        A process that hosts several clients passes clients=[(index, sk), ...] instead of index and sk and gets one peers list per client,
        all from ONE rofl_dh_shared call (the form pairwise_blinding_vecs takes once zipped with the indices).  A refused public key raises
        ValueError naming j and the status."""
        several = clients is not None
        if several == (index is not None or sk is not None) or (not several and (index is None or sk is None)):
            raise ValueError("either index and sk, or clients=[(index, sk), ...]")
        if public_keys is None or round_no is None:
            raise ValueError("the round's public keys and its number are needed")
        clients = [(int(i), k) for i, k in clients] if several else [(int(index), sk)]
        pks = _keys32(public_keys, "a public key")
        n = pks.shape[0]
        pairs = []
        for c, (i, _) in enumerate(clients):
            if not 0 <= i < n:
                raise ValueError("client %d has no public key in the round" % i)
            pairs += [(c, j) for j in range(n) if j != i]
        sks = _keys32([k for _, k in clients], "a secret key")
        try:
            secrets, status = key_agreement.shared_secrets(sks, pks, pairs)
        finally:
            sks[...] = 0
        res, at = [], 0
        for i, _ in clients:
            peers = []
            for j in range(n):
                if j == i:
                    continue
                if status[at]:
                    secrets[...] = 0
                    raise ValueError("the public key of client %d is refused (status %d)" % (j, int(status[at])))
                peers.append((j, pedersen_ops.pairwise_round_seed(secrets[at].tobytes(), round_no)))
                at += 1
            res.append(peers)
        secrets[...] = 0
        return res if several else res[0]

    @staticmethod
    def pairwise_residual_terms_from_keys(accepted, revealed, public_keys, round_no):
        """pairwise_residual_terms from ONE revealed secret key per rejected client instead of one seed per (accepted, rejected) pair:
        revealed = {j: sk_j}.  Each key is first checked against the round's public keys -- public_keys([sk_j]) != public_keys[j] raises
        ValueError naming j -- then every (rejected, accepted) secret comes from one rofl_dh_shared call, and the list returned is exactly
        pairwise_residual_terms(accepted, rejected, seeds) for the seeds those keys imply: same order, same signs.  A revealed key gives away
        every mask its owner ever shared under it: keys are per epoch."""
        accepted, rejected = [int(i) for i in accepted], sorted(int(j) for j in revealed)
        both = set(accepted) & set(rejected)
        if both:
            raise ValueError("client %d is both accepted and rejected" % min(both))
        pks = _keys32(public_keys, "a public key")
        for i in accepted + rejected:
            if not 0 <= i < pks.shape[0]:
                raise ValueError("client %d has no public key in the round" % i)
        if not accepted or not rejected:
            return []
        sks = _keys32([revealed[j] for j in rejected], "a secret key")
        try:
            own = key_agreement.public_keys(sks)
            for r, j in enumerate(rejected):
                if own[r].tobytes() != pks[j].tobytes():
                    raise ValueError("the revealed key of client %d does not belong to its public key" % j)
            secrets, status = key_agreement.shared_secrets(sks, pks[accepted], None)
        finally:
            sks[...] = 0
        seeds = {}
        for r, j in enumerate(rejected):
            for a, i in enumerate(accepted):
                at = r * len(accepted) + a
                if status[at]:
                    secrets[...] = 0
                    raise ValueError("the public key of client %d is refused (status %d)" % (i, int(status[at])))
                seeds[(i, j) if i < j else (j, i)] = pedersen_ops.pairwise_round_seed(secrets[at].tobytes(), round_no)
        secrets[...] = 0
        return pedersen_ops.pairwise_residual_terms(accepted, rejected, seeds)

    # ---- a round that loses an honest client: double masks, the secrets from the survivors' shares (secret_sharing) ----
    @staticmethod
    def dropout_residual_terms(survivors, dropped_keys, self_secrets, public_keys, round_no):
        """The terms of the residual blinding of the survivors' sum in a double-masked round (double_masked_blinding_vec):
        pairwise_residual_terms_from_keys(survivors, dropped_keys, public_keys, round_no) -- with its check of every key against the round's
        public keys -- followed by (self_mask_seed(self_secrets[i], round_no), +1) for i in sorted survivors.  dropped_keys = {j: sk_j} for
        the clients that left, self_secrets = {i: b_i} for the survivors.  The server must never hold BOTH secrets of one client (the key
        opens its pairwise masks, the self secret its self-mask: together they open its update), so an index in both dicts raises
        ValueError naming the client; so do a survivor without a self secret and a survivor in dropped_keys."""
        surv = [int(i) for i in survivors]
        dropped = {int(j): k for j, k in dropped_keys.items()}
        selfs = {int(i): b for i, b in self_secrets.items()}
        both = set(dropped) & set(selfs)
        if both:
            raise ValueError("client %d: its key and its self-mask secret are never opened together" % min(both))
        for i in surv:
            if i in dropped:
                raise ValueError("client %d is a survivor and has a revealed key" % i)
            if i not in selfs:
                raise ValueError("survivor %d has no self-mask secret" % i)
        terms = pedersen_ops.pairwise_residual_terms_from_keys(surv, dropped, public_keys, round_no)
        return terms + [(pedersen_ops.self_mask_seed(selfs[i], round_no), 1) for i in sorted(surv)]

    @staticmethod
    def dropout_residual_terms_from_shares(survivors, dropped, xs, key_shares, self_shares, public_keys, round_no):
        """dropout_residual_terms with the secrets reconstructed from the shares the answering survivors hold: xs = their evaluation points
        (client i holds i + 1), key_shares = {j: uint8[len(xs), 32]} the shares of sk_j for every dropped j, self_shares = {i: ...} the
        shares of b_i for every survivor i.  ALL secrets come from ONE rofl_shamir_reconstruct call (dropped keys first, then the survivors'
        self secrets, the same xs).  A wrong key share raises ValueError naming the dropped client (the public-key check); a wrong self share
        gives terms whose opening extract_opened refuses (ok = 0).  Neither names the survivor who lied:
        dropout_residual_terms_from_verified_shares does, and goes on without that survivor."""
        surv, drop = [int(i) for i in survivors], sorted(int(j) for j in dropped)
        key_shares = {int(j): v for j, v in key_shares.items()}
        self_shares = {int(i): v for i, v in self_shares.items()}
        both = (set(key_shares) & set(self_shares)) | (set(surv) & set(drop))
        if both:
            raise ValueError("client %d: its key and its self-mask secret are never opened together" % min(both))
        for j in drop:
            if j not in key_shares:
                raise ValueError("dropped client %d has no key shares" % j)
        for i in surv:
            if i not in self_shares:
                raise ValueError("survivor %d has no self-mask shares" % i)
        order = [(key_shares, j) for j in drop] + [(self_shares, i) for i in sorted(surv)]
        n_sh = int(np.asarray(xs).shape[0])
        stack = np.zeros((len(order), n_sh, 32), dtype=np.uint8)
        for r, (src, c) in enumerate(order):
            a = np.asarray(src[c], dtype=np.uint8)
            if a.shape != (n_sh, 32):
                raise ValueError("the shares of client %d are uint8[len(xs), 32]" % c)
            stack[r] = a
        try:
            sec = secret_sharing.reconstruct(xs, stack) if len(order) else np.zeros((0, 32), dtype=np.uint8)
        finally:
            stack[...] = 0
        try:
            return pedersen_ops.dropout_residual_terms(surv, {j: sec[r].tobytes() for r, j in enumerate(drop)},
                                                       {i: sec[len(drop) + r].tobytes() for r, i in enumerate(sorted(surv))}, public_keys, round_no)
        finally:
            sec[...] = 0

    @staticmethod
    def dropout_residual_terms_from_verified_shares(survivors, dropped, xs, key_shares, self_shares, key_commitments, self_commitments, public_keys,
                                                    round_no):
        """dropout_residual_terms_from_shares behind a check of every share against its dealer's Feldman commitments
        (secret_sharing.commit): key_commitments = {j: uint8[t, 32]} for every dropped j, self_commitments = {i: uint8[t, 32]} for every
        survivor i, the rest as there.  -> (terms, liars).  First key_commitments[j][0] must BE public_keys[j] (the constant-term commitment
        of a key is its public key; ValueError naming j otherwise).  Then ALL shares of all secrets go through ONE verify_shares call, in
        the order ..._from_shares stacks them (dropped keys first, then the survivors' self secrets).  An answering survivor with any
        verdict other than 0 in its column is a liar: its column is removed for every secret, and the remaining columns go to
        dropout_residual_terms_from_shares; liars = the sorted client indices (x - 1) of the removed columns.  Fewer than t columns left
        raises ValueError naming the liars; commitments that are no canonical encodings (verdict 2) raise ValueError naming the dealer."""
        surv, drop = [int(i) for i in survivors], sorted(int(j) for j in dropped)
        key_shares = {int(j): v for j, v in key_shares.items()}
        self_shares = {int(i): v for i, v in self_shares.items()}
        key_commitments = {int(j): np.asarray(v, dtype=np.uint8) for j, v in key_commitments.items()}
        self_commitments = {int(i): np.asarray(v, dtype=np.uint8) for i, v in self_commitments.items()}
        both = (set(key_shares) & set(self_shares)) | (set(surv) & set(drop))
        if both:
            raise ValueError("client %d: its key and its self-mask secret are never opened together" % min(both))
        for j in drop:
            if j not in key_shares:
                raise ValueError("dropped client %d has no key shares" % j)
            if j not in key_commitments:
                raise ValueError("dropped client %d has no key commitments" % j)
        for i in surv:
            if i not in self_shares:
                raise ValueError("survivor %d has no self-mask shares" % i)
            if i not in self_commitments:
                raise ValueError("survivor %d has no self-mask commitments" % i)
        order = [(key_shares, key_commitments, j) for j in drop] + [(self_shares, self_commitments, i) for i in sorted(surv)]
        x = np.asarray(xs)
        n_sh = int(x.shape[0])
        if not order:
            return pedersen_ops.dropout_residual_terms_from_shares(surv, drop, xs, key_shares, self_shares, public_keys, round_no), []
        t = int(order[0][1][order[0][2]].shape[0])
        pk = _keys32(public_keys, "a public key")
        for _, com, c in order:
            if com[c].ndim != 2 or com[c].shape != (t, 32) or t < 1:
                raise ValueError("the commitments of client %d are uint8[t, 32], one t for the round" % c)
        for j in drop:
            if not 0 <= j < pk.shape[0] or key_commitments[j][0].tobytes() != pk[j].tobytes():
                raise ValueError("client %d: the constant-term commitment of its key is not its public key" % j)
        stack = np.zeros((len(order), n_sh, 32), dtype=np.uint8)
        try:
            for r, (src, _, c) in enumerate(order):
                a = np.asarray(src[c], dtype=np.uint8)
                if a.shape != (n_sh, 32):
                    raise ValueError("the shares of client %d are uint8[len(xs), 32]" % c)
                stack[r] = a
            verdict = secret_sharing.verify_shares(np.stack([com[c] for _, com, c in order]), xs, stack)
        finally:
            stack[...] = 0
        for r, (_, _, c) in enumerate(order):
            if (verdict[r] == 2).any():
                raise ValueError("client %d: a commitment of its dealing is not a canonical Ristretto encoding" % c)
        bad = (verdict != 0).any(axis=0)
        liars = sorted(int(x[c]) - 1 for c in np.flatnonzero(bad))
        keep = np.flatnonzero(~bad)
        if keep.size < t:
            raise ValueError("survivors %r handed in shares that fail their commitments: %d consistent columns left, the threshold is %d"
                             % (liars, keep.size, t))
        terms = pedersen_ops.dropout_residual_terms_from_shares(
            surv, drop, x[keep], {j: np.asarray(key_shares[j], dtype=np.uint8)[keep] for j in drop},
            {i: np.asarray(self_shares[i], dtype=np.uint8)[keep] for i in surv}, public_keys, round_no)
        return terms, liars

    @staticmethod
    def dropout_residual_terms_from_signed_shares(survivors, dropped, xs, key_shares, self_shares, key_commitments, self_commitments, public_keys,
                                                  round_no, sig_public_keys, commitment_sigs):
        """dropout_residual_terms_from_verified_shares behind a check of the dealers' signatures on the commitments it uses:
        sig_public_keys = the clients' public SIGNING keys, indexed like public_keys; commitment_sigs = {client: uint8[64]}, the signature
        on secret_sharing.commitment_message(round_no, client, kind, commitments) of the row actually used -- kind 0 (key) for every dropped
        j, kind 1 (self) for every survivor i.  All of them go through ONE signatures.verify call, dropped first, then the survivors
        ascending.  A missing signature or a verdict other than 0 raises ValueError naming the dealer; then the call is
        dropout_residual_terms_from_verified_shares, unchanged.  -> (terms, liars)."""
        surv, drop = sorted(int(i) for i in survivors), sorted(int(j) for j in dropped)
        key_commitments = {int(j): v for j, v in key_commitments.items()}
        self_commitments = {int(i): v for i, v in self_commitments.items()}
        commitment_sigs = {int(c): np.asarray(v, dtype=np.uint8) for c, v in commitment_sigs.items()}
        spk = _keys32(sig_public_keys, "a public key")
        used = [(j, 0, key_commitments) for j in drop] + [(i, 1, self_commitments) for i in surv]
        msgs, sigs = [], []
        for c, kind, com in used:
            if c not in com:
                raise ValueError("%s %d has no %s commitments" % ("survivor" if kind else "dropped client", c, "self-mask" if kind else "key"))
            if c not in commitment_sigs or commitment_sigs[c].shape != (64,):
                raise ValueError("client %d: no signature on its %s commitments" % (c, "self-mask" if kind else "key"))
            if not 0 <= c < spk.shape[0]:
                raise ValueError("client %d has no public signing key" % c)
            msgs.append(secret_sharing.commitment_message(round_no, c, kind, com[c]))
            sigs.append(commitment_sigs[c])
        if used:
            verdict = signatures.verify(spk[[c for c, _, _ in used]], msgs, np.stack(sigs))
            for (c, kind, _), v in zip(used, verdict):
                if v != 0:
                    raise ValueError("client %d: the signature on its %s commitments does not verify (verdict %d)" % (c, "self-mask" if kind else "key", int(v)))
        return pedersen_ops.dropout_residual_terms_from_verified_shares(survivors, dropped, xs, key_shares, self_shares, key_commitments, self_commitments,
                                                                        public_keys, round_no)

    # ---- a round that rejects: the terms of the accepted set's residual blinding (accumulator.extract_opened_terms) ----
    @staticmethod
    def pairwise_residual_terms(accepted, rejected, seeds):
        """Pairwise masks (pairwise_blinding_vec) after rejections: the masks between two accepted clients cancel in the accepted clients'
        sum, the masks between an accepted i and a rejected j stay -- one term (seeds[(min(i, j), max(i, j))], +1 if i < j else -1) per
        such pair, the sign client i gave the stream.  seeds[(i, j)], i < j, is the seed clients i and j share.  A missing seed raises
        KeyError naming the pair, an index in both sets ValueError."""
        accepted, rejected = [int(i) for i in accepted], [int(j) for j in rejected]
        both = set(accepted) & set(rejected)
        if both:
            raise ValueError("client %d is both accepted and rejected" % min(both))
        terms = []
        for i in accepted:
            for j in rejected:
                pair = (i, j) if i < j else (j, i)
                if pair not in seeds:
                    raise KeyError("no shared seed of the pair %r" % (pair,))
                terms.append((seeds[pair], 1 if i < j else -1))
        return terms

    @staticmethod
    def cancelling_residual_terms(n_vec, seed, accept):
        """generate_cancelling_scalar_vec_seeded after rejections, accept[i] = vector i is in the sum: an accepted i < n_vec - 1 is
        +stream(seed_i), an accepted last vector -stream(seed_i) for every i < n_vec - 1; a stream taken with both signs is gone.  All
        accepted -> []."""
        n_vec = int(n_vec)
        accept = [bool(a) for a in accept]
        if n_vec < 1 or len(accept) != n_vec:
            raise ValueError("one verdict per vector")
        coef = [(1 if accept[i] else 0) - (1 if accept[-1] else 0) for i in range(n_vec - 1)]
        return [(pedersen_ops.cancelling_vec_seed(seed, i), c) for i, c in enumerate(coef) if c]

    @staticmethod
    def pairwise_round_seed(shared_secret, round_no):
        """SHA3-256("rofl-zk/blind/v1/round" || shared_secret || u64le(round_no)): the seed two clients use in round `round_no`.  A seed
        serves ONE round: masks of two rounds under one seed are equal, and the difference of the two masked updates would be in the clear."""
        return hashlib.sha3_256(b"rofl-zk/blind/v1/round" + bytes(shared_secret) + struct.pack("<Q", int(round_no))).digest()

    @staticmethod
    def quant_round_seed(secret, round_no):
        """SHA3-256("rofl-zk/quant/v1/round" || secret || u64le(round_no)): the seed a client rounds its update with in round `round_no`
        (range_proof_vec.quantize_probabilistic, the quant_seed of the containers' encrypt), from a long-lived secret of ITS OWN.  The seed is
        a per-round secret of the client: it decides which way every coordinate is rounded, so whoever learns it learns the update's
        fractional parts from its rounded values, and a seed used in two rounds rounds equal fractions the same way in both."""
        return hashlib.sha3_256(b"rofl-zk/quant/v1/round" + bytes(secret) + struct.pack("<Q", int(round_no))).digest()

    @staticmethod
    def noise_round_seed(secret, round_no):
        """SHA3-256("rofl-zk/noise/v1/round" || secret || u64le(round_no)): the seed a client draws its distributed noise from in round
        `round_no` (range_proof_vec.add_binomial_noise, the noise_seed of the containers' encrypt), from a long-lived secret of ITS OWN.
        The seed is a per-round secret of the client: whoever learns it computes the client's noise and removes it from the client's share
        of the released sum, and a seed used in two rounds adds the same noise in both, which their difference cancels."""
        return hashlib.sha3_256(b"rofl-zk/noise/v1/round" + bytes(secret) + struct.pack("<Q", int(round_no))).digest()

    @staticmethod
    def clip_round_seed(secret, round_no):
        """SHA3-256("rofl-zk/clip2/v1/round" || secret || u64le(round_no)): the seed a client rounds its norm-clipped update with in round
        `round_no` (l2_range_proof_vec.clip_l2, the clip_seed of the L2 containers' encrypt), from a long-lived secret of ITS OWN.  The
        seed is a per-round secret of the client: whoever learns it learns which way every scaled coordinate was rounded."""
        return hashlib.sha3_256(b"rofl-zk/clip2/v1/round" + bytes(secret) + struct.pack("<Q", int(round_no))).digest()

    @staticmethod
    def rotate_round_seed(public, round_no):
        """SHA3-256("rofl-zk/rotate/v1/round" || public || u64le(round_no)): the seed of the Hadamard rotation of round `round_no`
        (range_proof_vec.rotate / unrotate), from a value every participant knows, for instance the round's model hash.  Unlike
        quant_round_seed this seed is PUBLIC: every client and the server of a round use the same one, and nothing is hidden by it."""
        return hashlib.sha3_256(b"rofl-zk/rotate/v1/round" + bytes(public) + struct.pack("<Q", int(round_no))).digest()

    @staticmethod
    def compute_shifted_values_vec(values, offset):
        """pedersen_ops.rs:97-102 for scalars (the generic T: Add version; points: compute_shifted_values_rp)."""
        v = _u8(values)
        off = np.broadcast_to(np.ascontiguousarray(offset, dtype=np.uint8).reshape(1, 32), v.shape)
        return pedersen_ops.add_scalar_vec(v, np.ascontiguousarray(off))

    @staticmethod
    def zero_rp_vec(length):
        return np.zeros((length, 32), dtype=np.uint8)   # identity compresses to 32 zero bytes

    @staticmethod
    def zero_scalar_vec(length):
        return np.zeros((length, 32), dtype=np.uint8)

    @staticmethod
    def discrete_log_vec(points, table_size, bsgs_bits=16):
        """pedersen_ops.rs:37-53 (discrete_log_vec / discrete_log_vec_table over BSGSTable::new(table_size))."""
        p = _u8(points)
        out = np.zeros_like(p)
        _check(lib().rofl_discrete_log_vec(_ptr(p), _sz(p.shape[0]), _sz(table_size), bsgs_bits, _ptr(out)))
        return out

    @staticmethod
    def default_discrete_log_vec(points, fp=None):
        """pedersen_ops.rs:27-35: BSGSTable::default() = 2^(BSGS_N_BITS/2 + PRECOMP_BIAS) entries (fp.rs)."""
        table_size, bits = default_bsgs(fp)
        return pedersen_ops.discrete_log_vec(points, table_size, bits)

    @staticmethod
    def compute_shifted_values_rp(points, offset):
        p = _u8(points)
        o = np.ascontiguousarray(offset, dtype=np.uint8)
        out = np.zeros_like(p)
        _check(lib().rofl_shift_points(_ptr(p), _sz(p.shape[0]), _ptr(o), _ptr(out)))
        return out


class accumulator:
    """rofl_acc_*: a round's running sum of ElGamal pairs resident on the device (params.rs:74-147).  Handles are registry ids; records are
    host arrays or GPU tensors (read in place, every `stride` bytes)."""
    @staticmethod
    def create(d, init=0):
        h = ctypes.c_uint64()
        _check(lib().rofl_acc_create(_sz(d), int(init), ctypes.byref(h)))
        return h.value

    @staticmethod
    def add(h, records, counts, stride):
        """records: one pointer (int / c_void_p) per client; counts: records of each client (truncated to d by the library)"""
        n = len(records)
        rp = (ctypes.c_void_p * max(n, 1))(*records)
        cp = (_sz * max(n, 1))(*[int(c) for c in counts])
        _check(lib().rofl_acc_add(ctypes.c_uint64(h), _sz(n), rp, cp, _sz(stride)))

    @staticmethod
    def export(h, d):
        out = np.zeros((d, 64), dtype=np.uint8)
        _check(lib().rofl_acc_export(ctypes.c_uint64(h), _ptr(out)))
        return out

    @staticmethod
    def extract(h, d, table_size, bsgs_bits, fp):
        out = np.zeros(d, dtype=np.float32)
        ok = ctypes.c_int()
        _check(lib().rofl_acc_extract(ctypes.c_uint64(h), _sz(table_size), int(bsgs_bits), *fp, _ptr(out), ctypes.byref(ok)))
        return out if ok.value else None

    @staticmethod
    def extract_opened(h, d, opening, table_size, bsgs_bits, fp):
        """rofl_acc_extract_opened: `opening` = the d scalars s of the sum's residual blinding, a uint8[d, 32] numpy array or a contiguous
        torch uint8 tensor of d * 32 bytes on the accumulator's GPU (read in place).  -> (values, None) when every R equation holds, else
        (None, first_bad) with the smallest failing index; the accumulator is unchanged either way"""
        if _is_dev(opening):
            op, n = _dev_arg(opening, 1, 32)
        else:
            opening = _u8(opening)
            op, n = _ptr(opening), opening.size // 32
        if n != d:
            raise ValueError("the opening holds one 32-byte scalar per coordinate")
        out = np.zeros(d, dtype=np.float32)
        ok, bad = ctypes.c_int(), _sz()
        _check(lib().rofl_acc_extract_opened(ctypes.c_uint64(h), op, _sz(table_size), int(bsgs_bits), *fp, _ptr(out), ctypes.byref(ok), ctypes.byref(bad)))
        return (out, None) if ok.value else (None, bad.value)

    @staticmethod
    def extract_opened_terms(h, d, terms, table_size, bsgs_bits, fp):
        """rofl_acc_extract_opened_terms: the opening as its terms [(seed32, sign), ...] (pedersen_ops.pairwise_residual_terms /
        cancelling_residual_terms), summed on the device as blinding_vecs sums them -- it never exists on the host.  Returns as extract_opened."""
        terms = list(terms)
        arr = (_BlindTerm * max(len(terms), 1))()
        out = np.zeros(d, dtype=np.float32)
        ok, bad = ctypes.c_int(), _sz()
        try:
            for t, (seed, sign) in enumerate(terms):
                seed = bytes(seed)
                if len(seed) != 32:
                    raise ValueError("a seed is 32 bytes")
                if sign not in (1, -1):
                    raise ValueError("a term's sign is +1 or -1")
                ctypes.memmove(arr[t].seed, seed, 32)
                arr[t].sign = int(sign)
            _check(lib().rofl_acc_extract_opened_terms(ctypes.c_uint64(h), _sz(len(terms)), arr, _sz(table_size), int(bsgs_bits), *fp, _ptr(out),
                                                       ctypes.byref(ok), ctypes.byref(bad)))
        finally:
            ctypes.memset(arr, 0, ctypes.sizeof(arr))
        return (out, None) if ok.value else (None, bad.value)

    @staticmethod
    def reset(h):
        _check(lib().rofl_acc_reset(ctypes.c_uint64(h)))

    @staticmethod
    def destroy(h):
        _check(lib().rofl_acc_destroy(ctypes.c_uint64(h)))


class device_round:
    """rofl_round_*: a round's records resident on the device -- uploaded and decoded once by ingest, read by both verification legs and by
    the accumulation.  Handles are registry ids; records / proofs are pointers (int / c_void_p; a proof pointer may be None: client left out)."""
    COMPRESSED = 1      # ROFL_ROUND_COMPRESSED: ingest keeps every client's CompressedRandProof transcript prefix (verify_compressed)

    @staticmethod
    def create(d, record_len, max_clients, flags=0):
        h = ctypes.c_uint64()
        _check(lib().rofl_round_create_ex(_sz(d), _sz(record_len), _sz(max_clients), ctypes.c_uint(int(flags)), ctypes.byref(h)))
        return h.value

    @staticmethod
    def create_rand(d, record_len, max_clients):
        """rofl_round_create_rand: a round that keeps every client's CompressedRandProof transcript prefix (verify_compressed) for records
        of either length -- 64 is create(..., COMPRESSED); 96 is a round of EncL2Compressed updates whose randomness proof is checked"""
        h = ctypes.c_uint64()
        _check(lib().rofl_round_create_rand(_sz(d), _sz(record_len), _sz(max_clients), ctypes.byref(h)))
        return h.value

    @staticmethod
    def ingest(h, records):
        n = len(records)
        rp = (ctypes.c_void_p * max(n, 1))(*records)
        first = _sz()
        _check(lib().rofl_round_ingest(ctypes.c_uint64(h), _sz(n), rp, ctypes.byref(first)))
        return first.value

    @staticmethod
    def verify_sigma(h, kind, proofs, want_csq=False):
        """(verdicts, csq sums or None), one per ingested client"""
        n = len(proofs)
        pp = (ctypes.c_void_p * max(n, 1))(*proofs)
        ok = (ctypes.c_int * max(n, 1))()
        sums = np.zeros((n, 32), dtype=np.uint8) if want_csq else None
        _check(lib().rofl_round_verify_sigma(ctypes.c_uint64(h), int(kind), pp, ok, _ptr(sums) if want_csq and n else None))
        return [bool(ok[i]) for i in range(n)], sums

    @staticmethod
    def verify_range(h, proofs, proof_len, n_proofs, k_checked, prove_range, verifier_seed=None, fp=None):
        n = len(proofs)
        pp = (ctypes.c_void_p * max(n, 1))(*proofs)
        ok = (ctypes.c_int * max(n, 1))()
        seed = bytes(verifier_seed) if verifier_seed is not None else os.urandom(32)
        _check(lib().rofl_round_verify_range(ctypes.c_uint64(h), pp, _sz(proof_len), _sz(n_proofs), _sz(k_checked), _sz(prove_range), *_fp(fp), seed, ok))
        return [bool(ok[i]) for i in range(n)]

    @staticmethod
    def verify_compressed(h, proofs):
        """the 128-byte CompressedRandProofs of a round created with COMPRESSED or create_rand, one pointer (or None) per ingested client -> list[bool]"""
        n = len(proofs)
        pp = (ctypes.c_void_p * max(n, 1))(*proofs)
        ok = (ctypes.c_int * max(n, 1))()
        _check(lib().rofl_round_verify_compressed(ctypes.c_uint64(h), pp, ok))
        return [bool(ok[i]) for i in range(n)]

    @staticmethod
    def accumulate(h, acc, accept=None):
        a = None if accept is None else (ctypes.c_int * max(len(accept), 1))(*[1 if x else 0 for x in accept])
        _check(lib().rofl_round_accumulate(ctypes.c_uint64(h), ctypes.c_uint64(acc), a))

    @staticmethod
    def reset(h):
        _check(lib().rofl_round_reset(ctypes.c_uint64(h)))

    @staticmethod
    def destroy(h):
        _check(lib().rofl_round_destroy(ctypes.c_uint64(h)))


def point_decodes():
    """test hook (include/rofl_zk_debug.h): compressed points handed to the device's Ristretto decoder so far, process-wide"""
    out = ctypes.c_uint64()
    _check(lib().rofl_dbg_point_decodes(ctypes.byref(out)))
    return int(out.value)


def default_bsgs(fp=None):
    """(table_size, bsgs_bits) of BSGSTable::default() for the fixed-point type (fp.rs; pedersen_ops.rs:27-35)"""
    bits, bias = {8: (8, 3), 16: (16, 7), 32: (16, 7), 64: (16, 0)}[_fp(fp)[0]]
    return 1 << (bits // 2 + bias), bits


class conversion32:
    @staticmethod
    def f32_to_scalar_vec(values, fp=None):
        v = np.ascontiguousarray(values, dtype=np.float32)
        out = np.zeros((v.size, 32), dtype=np.uint8)
        _check(lib().rofl_f32_to_scalar_vec(_ptr(v), _sz(v.size), *_fp(fp), _ptr(out)))
        return out

    @staticmethod
    def scalar_to_f32_vec(scalars, fp=None):
        s = _u8(scalars)
        out = np.zeros(s.shape[0], dtype=np.float32)
        _check(lib().rofl_scalar_to_f32_vec(_ptr(s), _sz(s.shape[0]), *_fp(fp), _ptr(out)))
        return out

    @staticmethod
    def square(scalars, fp=None):
        """conversion32.rs:66-88 (element-wise over a vector of scalars); overflow -> RoflError 8 (the reference panics)."""
        a = _u8(scalars)
        out = np.zeros_like(a)
        _check(lib().rofl_fp_square_vec(_ptr(a), _sz(a.shape[0]), *_fp(fp), _ptr(out)))
        return out

    @staticmethod
    def precompute_exponentiate(value, exp):
        """conversion32.rs:101-111: [1, v, ..., v^(exp-1)]."""
        v = np.ascontiguousarray(value, dtype=np.uint8).reshape(32)
        out = np.zeros((exp, 32), dtype=np.uint8)
        _check(lib().rofl_scalar_powers(_ptr(v), _sz(exp), _ptr(out)))
        return out

    @staticmethod
    def exponentiate(value, exp):
        """conversion32.rs:113-122."""
        return conversion32.precompute_exponentiate(value, exp + 1)[exp]

    @staticmethod
    def f32_to_fp_vec(values, fp=None):
        v = np.ascontiguousarray(values, dtype=np.float32)
        out = np.zeros(v.size, dtype=np.uint64)
        _check(lib().rofl_f32_to_fp_vec(_ptr(v), _sz(v.size), *_fp(fp), _ptr(out)))
        return out

    @staticmethod
    def uint_to_f32_vec(values, fp=None):
        v = np.ascontiguousarray(values, dtype=np.uint64)
        out = np.zeros(v.size, dtype=np.float32)
        _check(lib().rofl_uint_to_f32_vec(_ptr(v), _sz(v.size), *_fp(fp), _ptr(out)))
        return out

    @staticmethod
    def get_clip_bounds(prove_range, fp=None):
        mn, mx = ctypes.c_float(), ctypes.c_float()
        _check(lib().rofl_get_clip_bounds(_sz(prove_range), *_fp(fp), ctypes.byref(mn), ctypes.byref(mx)))
        return mn.value, mx.value

    @staticmethod
    def get_l2_clip_bounds(prove_range, fp=None):
        out = ctypes.c_float()
        _check(lib().rofl_get_l2_clip_bounds(_sz(prove_range), *_fp(fp), ctypes.byref(out)))
        return out.value
