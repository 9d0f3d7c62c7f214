"""Host-side mirror of the encrypted-update containers of rofl_service:

    EncParamsRange / EncParamsRangeCompressed / EncParamsL2 / EncParamsL2Compressed
        .encrypt(...)  .verify()  .serialize()  .deserialize(data)        rofl_service/src/flserver/params.rs:462-541, 683-775, 544-681, 790-885
    EncParamsL2CompressedStrict: EncParamsL2Compressed whose verify() also checks the update's CompressedRandProof (the reference's arm skips it)
    EncModelParamsAccumulator (.unity, .accumulate_other, .extract)         params.rs:74-138

Same names, argument meaning and composition as the reference; every group operation runs through the C ABI
(include/rofl_zk.h) on the GPU, the wire codec (proto3, length-delimited) is the library's rofl_wire_* host code.
Values are numpy byte arrays in the reference's to_bytes layouts: ElGamalPair 64 B (L | R), SquareRandProofCommitments
96 B (L | R | c_sq), RandProof 128 B, SquareRandProof 192 B, SquareProof 160 B, CompressedRandProof 128 B, RangeProof per chunk.
"""
import ctypes
import hashlib
import os

import numpy as np

from . import api
from .api import (RoflError, Nonce, DiscreteGaussian, lib, _check, _ptr, _sz, range_proof_vec, l2_range_proof_vec, rand_proof_vec,
                  square_rand_proof_vec, square_proof_vec, compressed_rand_proof, pedersen_ops, conversion32)

WIRE_ENC_RANGE, WIRE_ENC_NORM, WIRE_ENC_NORM_COMPRESSED = 0, 1, 2


class _WireMsg(ctypes.Structure):
    _fields_ = [("kind", ctypes.c_int),
                ("enc_values", ctypes.c_void_p), ("enc_values_len", ctypes.c_size_t),
                ("rand_proof", ctypes.c_void_p), ("rand_proof_len", ctypes.c_size_t),
                ("square_proof", ctypes.c_void_p), ("square_proof_len", ctypes.c_size_t),
                ("range_proofs", ctypes.c_void_p), ("range_proof_len", ctypes.c_size_t), ("n_range_proofs", ctypes.c_size_t),
                ("square_range_proof", ctypes.c_void_p), ("square_range_proof_len", ctypes.c_size_t),
                ("range_bits", ctypes.c_int32), ("l2_range_bits", ctypes.c_int32), ("check_percentage", ctypes.c_float)]


def _flat(a):
    return np.ascontiguousarray(a, dtype=np.uint8).reshape(-1)


class wire:
    """rofl_wire_encode / rofl_wire_decode (flservice.proto:75-100)."""

    @staticmethod
    def encode(kind, enc_values=None, rand_proof=None, square_proof=None, range_proofs=None, square_range_proof=None,
               range_bits=0, l2_range_bits=0, check_percentage=0.0, as_array=False):
        keep = []
        m = _WireMsg(); m.kind = kind

        def put(name, arr):
            if arr is None:
                return
            a = _flat(arr); keep.append(a)
            setattr(m, name, a.ctypes.data if a.size else None); setattr(m, name + "_len", a.size)
        put("enc_values", enc_values); put("rand_proof", rand_proof); put("square_proof", square_proof); put("square_range_proof", square_range_proof)
        if range_proofs is not None:
            rp = np.ascontiguousarray(range_proofs, dtype=np.uint8)
            if rp.ndim < 2:
                rp = rp.reshape(1, -1)
            elif rp.ndim > 2 or rp.size == 0:
                rp = rp.reshape(rp.shape[0], int(np.prod(rp.shape[1:])))
            keep.append(rp)
            m.range_proofs = rp.ctypes.data if rp.size else None; m.range_proof_len = rp.shape[1]; m.n_range_proofs = rp.shape[0]
        m.range_bits, m.l2_range_bits, m.check_percentage = int(range_bits), int(l2_range_bits), float(check_percentage)
        n = lib().rofl_wire_encoded_size(ctypes.byref(m))
        out = np.empty(max(n, 1), dtype=np.uint8); ln = ctypes.c_size_t()
        _check(lib().rofl_wire_encode(ctypes.byref(m), _ptr(out), _sz(out.size), ctypes.byref(ln)))
        return out[:ln.value] if as_array else out[:ln.value].tobytes()      # as_array: no second copy of a 16 MB message

    @staticmethod
    def decode(kind, data, copy=True):
        """copy=False: `data` is a contiguous uint8 array that outlives the result; the payload fields are VIEWS into it (a server that
        verifies a round of 16 MB messages does not copy each of them twice on the way in)."""
        if not copy and isinstance(data, np.ndarray) and data.dtype == np.uint8 and data.flags["C_CONTIGUOUS"]:
            buf = data.reshape(-1)
        else:
            buf = np.frombuffer(bytes(data), dtype=np.uint8); copy = True
        m = _WireMsg()
        _check(lib().rofl_wire_decode(kind, _ptr(buf), _sz(buf.size), ctypes.byref(m), None, _sz(0)))
        rp = np.zeros((m.n_range_proofs, m.range_proof_len), dtype=np.uint8)
        if rp.size:
            _check(lib().rofl_wire_decode(kind, _ptr(buf), _sz(buf.size), ctypes.byref(m), _ptr(rp), _sz(rp.size)))
        base = buf.ctypes.data

        def span(name):
            p, n = getattr(m, name), getattr(m, name + "_len")
            if not (p and n):
                return np.zeros(0, dtype=np.uint8)
            return buf[p - base:p - base + n].copy() if copy else buf[p - base:p - base + n]
        return {"enc_values": span("enc_values"), "rand_proof": span("rand_proof"), "square_proof": span("square_proof"),
                "square_range_proof": span("square_range_proof"), "range_proofs": rp, "range_bits": m.range_bits,
                "l2_range_bits": m.l2_range_bits, "check_percentage": m.check_percentage}


_pool = None


kernel_time_sink = None      # measurement hook (bench.py): called with api.last_kernel_times() on the thread of every proof call of a container


def _timed(thunk):
    def run():
        r = thunk()
        if kernel_time_sink is not None:
            kernel_time_sink(api.last_kernel_times())      # rofl_last_kernel_times is per calling thread
        return r
    return run


def _range_commitments(clipped, bl, prove_range, fp):
    """The commitments create_rangeproof returns for these (clipped) values and blindings, computed ahead of it so that the legs which complete
    them can run beside the range proof: commit(read_from_bytes(f32_to_scalar(v) + 2^(n-1)) - 2^(n-1), r) (range_proof_vec/mod.rs:36-43, 96-99).
    That is commit(f32_to_scalar(v), r) except where the shift leaves the fp_bits bits that read_from_bytes keeps: at a 32- or 64-bit range
    get_clip_bounds rounds up to a power of two in f32, so the closed upper bound quantizes to 2^(n-1) and commits as the lower bound."""
    off = np.frombuffer((1 << (prove_range - 1)).to_bytes(32, "little"), np.uint8)
    s = pedersen_ops.compute_shifted_values_vec(conversion32.f32_to_scalar_vec(clipped, fp=fp), off)
    s[:, fp[0] // 8:] = 0
    return pedersen_ops.commit_vec(pedersen_ops.add_scalar_vec(s, np.ascontiguousarray(np.broadcast_to(off, s.shape)), subtract=True), bl)


def _concurrently(*thunks):
    """Run independent proof calls on separate library lanes (each call takes a free lane: HIP stream + workspace).  The
    reference runs them one after the other, each spread over the rayon pool; on the GPU the latency-bound tails of one proof
    (a 5-round sum proof, the per-element Sigma-proof kernels) overlap the throughput-bound phases of another."""
    global _pool
    if kernel_time_sink is not None:
        thunks = [_timed(t) for t in thunks]
    if len(thunks) == 1:
        return [thunks[0]()]
    if _pool is None:
        from concurrent.futures import ThreadPoolExecutor
        _pool = ThreadPoolExecutor(max_workers=32, thread_name_prefix="rofl-params")      # three proofs per container, several containers in flight (threads start on demand)
    # The device is a property of the calling THREAD (rofl_set_device): the pool's workers run every leg of a container on the device of the
    # thread that asked for it, not on the process default (which only the first rofl_set_device of the process moves).
    dev = api.get_device()

    def bound(t):
        def run():
            api.bind_device(dev)
            return t()
        return run
    futs = [_pool.submit(bound(t)) for t in thunks]
    return [f.result() for f in futs]


# What a container's verify() may turn into "does not verify": errors that a crafted MESSAGE can provoke (FormatError, a bit size or an
# aggregation no proof can have, lengths that do not match).  Everything else -- HIP / RCCL runtime errors (>= 99), a bad parameter of the
# call itself, a batch that has to be split, a missing /dev/urandom -- is a fault of the SERVER and is raised: rejecting a round of honest
# clients (server.rs:474-484) because the verifier broke would look the same as a round of cheaters.
# Code 11 (bad parameter; the reference panics) is both: range_bits = 0 or more proofs than commitments come off the wire, "batch too large
# (split it)" does not.  A single update's verify() counts it as the message's fault; verify_batch falls back to per-client verification.
_MESSAGE_ERRORS = (1, 3, 4, 5, 6, 11)


def _is_message_error(e):
    return isinstance(e, (ValueError, OverflowError, IndexError)) or (isinstance(e, RoflError) and e.code in _MESSAGE_ERRORS)


try:
    import xxhash as _xxhash
except ImportError:      # pragma: no cover
    _xxhash = None


def witness_digest(*arrays):
    """Digest of the raw bytes of the witness arrays (values, blindings, ...) of one container: XXH3-128 when the xxhash module is
    there (1.7 MB of witness in ~0.2 ms; SHA3-256 needed ~5 ms, on the critical path of encrypt), else BLAKE2b-128.  It only has to
    tell different witnesses apart for an honest prover -- the seed stays secret and goes through SHA3 with it (_sub_nonce)."""
    h = _xxhash.xxh3_128() if _xxhash is not None else hashlib.blake2b(digest_size=16)
    for a in arrays:
        h.update(np.ascontiguousarray(a).data)
    return (b"x" if _xxhash is not None else b"b") + h.digest()


def _sub_nonce(seed, tag, witness):
    """Independent nonce streams for the proofs of one container (the reference draws all of them from thread_rng).
    `nonce_seed` is for reproducible tests / benchmarks only; even then the effective seed is bound to the witness
    (values and blindings), like bulletproofs' witness-rekeyed transcript RNG: re-using a seed with different inputs
    never repeats a nonce (two proofs with equal nonces and different challenges would reveal the witness)."""
    if seed is None:
        return Nonce.random()
    return Nonce.seeded(hashlib.sha3_256(b"rofl-zk/params/v2" + bytes(seed) + tag + witness).digest())


def _sub_seed(seed, tag):
    return os.urandom(32) if seed is None else hashlib.sha3_256(b"rofl-zk/params/v1" + bytes(seed) + tag).digest()


def _num_checked(d, check_percentage):
    # (len as f32 * check_percentage).round() as usize  -- f32 arithmetic, round half away from zero (params.rs:192-193, 487)
    # The field comes off the wire: NaN / inf / values outside [0, 1] (the reference would slice out of bounds and panic) are
    # a malformed message here.
    cp = np.float32(check_percentage)
    if not np.isfinite(cp) or cp < 0 or cp > 1:
        raise RoflError(11, "check_percentage outside [0, 1]")
    x = np.float32(d) * cp
    return min(int(d), int(np.floor(np.float64(x) + 0.5)))


# The order of a client's steps: rotate -> round -> clip -> noise -> legs.  The first one, the randomized Hadamard rotation
# (range_proof_vec.rotate / rotate_vecs, rofl_rotate), changes the vector's LENGTH -- d elements become rotated_len(d, block_log2) -- so it
# stands IN FRONT of the containers, not inside them: encrypt / encrypt_batch* take the rotated vector and a blinding vector of
# rotated_len entries, and their parameter lists stay as they are.  Its seed is PUBLIC, one per round for every client and the server
# (pedersen_ops.rotate_round_seed).  The rotation is orthonormal, so l2_range and l2_clip mean the same before and after it, and the sum
# commutes with it: the server undoes it ONCE, range_proof_vec.unrotate(acc.extract(...), seed, block_log2, d).  The steps below are the
# keywords of the containers and act on the rotated vector.
#
# The containers' quant_seed / quant_seeds (probabilistic quantization, range_proof_vec.quantize_probabilistic): with a seed the quantize
# call stands where clip_f32_to_range_vec stands, and its output -- on the fixed-point grid, inside the clip range -- is the plaintext of
# EVERY leg from there on, the witness digest included: the legs that take the un-clipped plaintext (params.rs:499) would otherwise round
# the raw values deterministically and prove something else than the range proof commits to.  Without a seed nothing changes.
# The seed is a per-round SECRET of the client (pedersen_ops.quant_round_seed).  For the L2 containers rounding up can push an update that
# sat just under the norm bound over it; the sum proof then reports NormOutOfRangeError (7) as for any other update over the bound.
#
# The containers' noise_seed + noise_k / noise_seeds + noise_k (distributed noise, range_proof_vec.add_binomial_noise): both or neither.
# The noise is added after the rounding of a quant_seed, where one is given (without one the noise call rounds to nearest itself), and
# before everything else; its output -- again on the grid and inside the clip range -- is the plaintext of every leg and of the witness
# digest in the same way.  The seed is a per-round SECRET of the client (pedersen_ops.noise_round_seed).  A value within noise_k steps of
# a clip bound can saturate there (range_proof_vec.clip_f32_for_noise avoids it), and for the L2 containers the noise raises the norm --
# by about sqrt(d noise_k / 2) steps: an update that then exceeds the bound fails with NormOutOfRangeError (7) like any other.
# noise_k is an int for the binomial noise, or a DiscreteGaussian(sigma2) for the discrete Gaussian noise (range_proof_vec.add_dgauss_noise:
# any integer sigma2 from 1 to 2^24, a cost that does not grow with it); the seed serves either, their stream labels differ.
def _noise_args(noise_seed, noise_k):
    if (noise_seed is None) != (noise_k is None):
        raise ValueError("noise_seed(s) and noise_k are given together or not at all")
    return noise_seed is not None


#
# The L2 containers' l2_clip + clip_seed / clip_seeds (norm clipping, l2_range_proof_vec.clip_l2): l2_clip is the budget max_sq in grid
# steps^2 (l2_range_proof_vec.norm_budget(l2_range) for the whole bound of the norm check), clip_seed an optional 32-byte seed that rounds
# the scaled steps instead of truncating them (pedersen_ops.clip_round_seed, a per-round SECRET of the client).  The clip stands between
# the rounding and the noise: after it the exact integer sum of squares the sum proof computes is at most l2_clip, so a quant_seed can no
# longer push an update over the bound, and the noise can only by more than the steps norm_budget reserved for it.  Its output is the
# plaintext of every leg and of the witness digest.  Without l2_clip nothing changes.
def _clip_args(l2_clip, clip_seed):
    if l2_clip is None and clip_seed is not None:
        raise ValueError("clip_seed(s) without l2_clip")
    return l2_clip is not None


def _apply_where(xs, clipped, marks, call):
    """ONE call(vectors, marks) -> rows over the clients whose mark is not None; a row becomes its client's plaintext and clipped vector"""
    idx = [i for i, m in enumerate(marks) if m is not None]
    if idx:
        rows = call([xs[i] for i in idx], [marks[i] for i in idx])
        for row, i in zip(rows, idx):
            xs[i] = clipped[i] = row.reshape(xs[i].shape)


def _clip_or_quantize_batch(xs, prove_range, quant_seeds, fp, noise_seeds=None, noise_k=None, l2_clip=None, clip_seeds=None):
    """-> (plaintexts, clipped) of the clients of encrypt_batch: ONE quantize call for all clients that have a quant seed, then ONE clip
    call for all clients where there is an l2_clip, then ONE noise call for all clients that have a noise seed.  Every step takes the
    vector the step before it left -- the rounded one where there is one, else the raw one: the clip and the noise call clip and round to
    nearest themselves -- and a client that no step touched keeps its raw vector, clipped like clip_f32_to_range_vec."""
    noisy, clipping = _noise_args(noise_seeds, noise_k), _clip_args(l2_clip, clip_seeds)
    if quant_seeds is None and not noisy and not clipping:
        return xs, [range_proof_vec.clip_f32_to_range_vec(x, prove_range, fp=fp) for x in xs]
    n = len(xs)
    noise_seeds, quant_seeds = [None] * n if noise_seeds is None else list(noise_seeds), [None] * n if quant_seeds is None else list(quant_seeds)
    for what, seeds in (("noise", noise_seeds), ("quant", quant_seeds)):
        if len(seeds) != n:
            raise ValueError("one %s seed (or None) per client" % what)
    if any(x.size != xs[0].size for x in xs):
        raise ValueError("the clients of a batch have one vector length")
    xs, clipped = list(xs), [None] * n
    _apply_where(xs, clipped, quant_seeds, lambda vs, seeds: range_proof_vec.quantize_probabilistic_vecs(vs, prove_range, seeds, fp=fp))
    if clipping and xs:      # (every client: the clip call tells the seeded from the unseeded itself)
        for i, row in enumerate(l2_range_proof_vec.clip_l2_vecs(xs, prove_range, l2_clip, clip_seeds, fp=fp)):
            xs[i] = clipped[i] = row.reshape(xs[i].shape)
    if isinstance(noise_k, DiscreteGaussian):      # the mechanism is the type of noise_k: an int is the binomial's k
        _apply_where(xs, clipped, noise_seeds, lambda vs, seeds: range_proof_vec.add_dgauss_noise_vecs(vs, prove_range, seeds, noise_k.sigma2, fp=fp))
    else:
        _apply_where(xs, clipped, noise_seeds, lambda vs, seeds: range_proof_vec.add_binomial_noise_vecs(vs, prove_range, seeds, noise_k, fp=fp))
    for i in range(n):
        if clipped[i] is None:
            clipped[i] = range_proof_vec.clip_f32_to_range_vec(xs[i], prove_range, fp=fp)
    return xs, clipped


def _clip_or_quantize(x, prove_range, quant_seed, fp, noise_seed=None, noise_k=None, l2_clip=None, clip_seed=None):
    """-> (plaintext, clipped) of one client: a batch of one"""
    one = lambda a: None if a is None else [a]
    xs, clipped = _clip_or_quantize_batch([x], prove_range, one(quant_seed), fp, one(noise_seed), noise_k, one(l2_clip), one(clip_seed))
    return xs[0], clipped[0]


class _HostLegs:
    """Where verify_batch takes the batched legs of the majority-shape members from: caller memory, through the existing batch entry points.
    DeviceRound supplies the same three legs over the commitments it holds on the device (us = the members, idx = their positions in the
    list verify_batch was given)."""

    @staticmethod
    def rand(cls, us, idx):
        return cls._rand_batch(us)

    @staticmethod
    def square(cls, us, idx):
        return cls._square_batch(us)

    @staticmethod
    def range(us, idx, k, prove_range, seed, fp, stride):
        return range_proof_vec.verify_rangeproof_batch([u.range_proofs for u in us], [u.enc_values[:k] for u in us], prove_range, verifier_seed=seed, fp=fp, commit_stride=stride)


class EncParamsRange:
    """params.rs:456-541."""
    kind = WIRE_ENC_RANGE

    def __init__(self, enc_values, rand_proofs, range_proofs, prove_range, check_percentage):
        self.enc_values = np.ascontiguousarray(enc_values, dtype=np.uint8).reshape(-1, 64)
        self.rand_proofs = np.ascontiguousarray(rand_proofs, dtype=np.uint8).reshape(-1, 128)
        self.range_proofs = np.ascontiguousarray(range_proofs, dtype=np.uint8)
        self.prove_range, self.check_percentage = int(prove_range), float(check_percentage)

    @classmethod
    def encrypt(cls, plaintext_vec, blinding_vec, prove_range, n_partition, check_percentage, nonce_seed=None, fp=None, quant_seed=None, noise_seed=None, noise_k=None):
        fp = api._fp(fp)                       # resolved in the caller's thread; the proof calls below run on pool threads
        x = np.ascontiguousarray(plaintext_vec, dtype=np.float32)
        bl = api._u8(blinding_vec)
        x, clipped = _clip_or_quantize(x, prove_range, quant_seed, fp, noise_seed, noise_k)
        wd = witness_digest(x, bl) if nonce_seed is not None else b""
        if check_percentage >= 1.0:
            enc_com = _range_commitments(clipped, bl, prove_range, fp)      # == the range proof's commitments
            # NB the reference passes the un-clipped plaintext here (params.rs:499)
            (rp, rp_com), (proofs, pairs) = _concurrently(
                lambda: range_proof_vec.create_rangeproof(clipped, bl, prove_range, n_partition, nonce=_sub_nonce(nonce_seed, b"range", wd), fp=fp),
                lambda: rand_proof_vec.create_randproof_vec_existing(x, enc_com, bl, nonce=_sub_nonce(nonce_seed, b"rand", wd), fp=fp))
            assert (rp_com == enc_com).all()
        else:
            k = _num_checked(x.size, check_percentage)
            (rp, _), (proofs, pairs) = _concurrently(
                lambda: range_proof_vec.create_rangeproof(clipped[:k], bl[:k], prove_range, n_partition, nonce=_sub_nonce(nonce_seed, b"range", wd), fp=fp),
                lambda: rand_proof_vec.create_randproof_vec(x, bl, nonce=_sub_nonce(nonce_seed, b"rand", wd), fp=fp))
        return cls(pairs, proofs, rp, prove_range, check_percentage)

    @staticmethod
    def _rand_create_batch(xs, bls, enc_coms, nonces, fp):
        """The randomness leg of encrypt_batch: (thunks, collect) -- the thunks run beside the range proofs (_concurrently), collect(their
        results) is the list of (rand proofs, pairs) per client.  enc_coms[i]: the commitments to complete, or None.  Here: ONE
        rofl_create_sigmaproof_vec_batch (create_randproof_vec(_existing) of every client) for all clients."""
        return [lambda: rand_proof_vec.create_randproof_vec_batch(xs, bls, nonces=nonces, existing_list=enc_coms, fp=fp)], lambda res: res[0]

    @classmethod
    def encrypt_batch(cls, clients, prove_range, n_partition, check_percentage, nonce_seeds=None, fp=None):
        """_encrypt_batch (below) without probabilistic quantization: the clients' values are clipped, as encrypt() without a quant_seed does."""
        return cls._encrypt_batch(clients, prove_range, n_partition, check_percentage, nonce_seeds, fp, None)

    @classmethod
    def encrypt_batch_quantized(cls, clients, prove_range, n_partition, check_percentage, quant_seeds, nonce_seeds=None, fp=None):
        """encrypt_batch with quant_seeds = one 32-byte seed (or None: clip only) per client: ONE rofl_quantize_prob call rounds the values of
        all hosted clients, then the legs run as in encrypt_batch.  Byte-identical to encrypt(quant_seed=...) per client.  (A method of
        its own: the parameter list of encrypt_batch is pinned.)"""
        return cls._encrypt_batch(clients, prove_range, n_partition, check_percentage, nonce_seeds, fp, quant_seeds)

    @classmethod
    def encrypt_batch_private(cls, clients, prove_range, n_partition, check_percentage, nonce_seeds=None, fp=None, quant_seeds=None, noise_seeds=None, noise_k=None):
        """encrypt_batch_quantized with distributed noise: noise_seeds = one 32-byte seed (or None: no noise) per client and noise_k, both or
        neither.  After the ONE rofl_quantize_prob call of the quant_seeds, ONE rofl_noise_binomial call adds the noise of all hosted clients,
        then the legs run as in encrypt_batch.  Byte-identical to encrypt(quant_seed=..., noise_seed=..., noise_k=...) per client, and
        without noise seeds to encrypt_batch_quantized.  (A method of its own: the parameter lists of encrypt_batch and
        encrypt_batch_quantized are pinned.)"""
        _noise_args(noise_seeds, noise_k)
        return cls._encrypt_batch(clients, prove_range, n_partition, check_percentage, nonce_seeds, fp, quant_seeds, noise_seeds, noise_k)

    @classmethod
    def _encrypt_batch(cls, clients, prove_range, n_partition, check_percentage, nonce_seeds, fp, quant_seeds, noise_seeds=None, noise_k=None):
        """encrypt() for several clients of one process (rofl_service's client binary hosts its clients as tasks of one process,
        client.rs:265-266): clients = [(plaintext_vec, blinding_vec), ...] of one length.  The L-inf legs of all of them are ONE
        rofl_create_rangeproof_batch call -- over the first k values of every client when check_percentage < 1 -- and the randomness leg
        (_rand_create_batch: ONE rofl_create_sigmaproof_vec_batch here, ONE rofl_create_compressed_randproof_batch for EncParamsRangeCompressed)
        runs beside it.  Every container is byte-identical to what encrypt() returns for that client with the same nonce seed; a client that fails
        raises."""
        fp = api._fp(fp)
        n = len(clients)
        if n == 0:
            return []
        seeds = list(nonce_seeds) if nonce_seeds is not None else [None] * n
        xs, bls, clipped = [], [], []
        for (x, bl) in clients:
            x = np.ascontiguousarray(x, dtype=np.float32); bl = api._u8(bl)
            xs.append(x); bls.append(bl)
        xs, clipped = _clip_or_quantize_batch(xs, prove_range, quant_seeds, fp, noise_seeds, noise_k)      # (ONE quantize and ONE noise call for all hosted clients)
        d = xs[0].size
        if any(x.size != d for x in xs):
            raise ValueError("the clients of a batch have one vector length")
        wds = [witness_digest(x, bl) if sd is not None else b"" for x, bl, sd in zip(xs, bls, seeds)]
        range_nonces = [_sub_nonce(sd, b"range", wd) for sd, wd in zip(seeds, wds)]
        rand_nonces = [_sub_nonce(sd, b"rand", wd) for sd, wd in zip(seeds, wds)]
        if check_percentage >= 1.0:
            # the range proofs' commitments, computed first (one call for all clients) so that the randomness proofs can complete them while the range proofs run
            enc_all = _range_commitments(np.concatenate(clipped), np.concatenate(bls), prove_range, fp)
            enc_coms = [enc_all[i * d:(i + 1) * d] for i in range(n)]
            rv, rb = clipped, bls
        else:
            k = _num_checked(d, check_percentage)
            enc_coms = [None] * n
            rv, rb = [c[:k] for c in clipped], [bl[:k] for bl in bls]
        # NB the reference passes the un-clipped plaintext to the randomness proof (params.rs:499)
        thunks, collect = cls._rand_create_batch(xs, bls, enc_coms, rand_nonces, fp)
        res = _concurrently(lambda: range_proof_vec.create_rangeproof_batch(rv, rb, prove_range, n_partition, nonces=range_nonces, fp=fp), *thunks)
        rand = collect(res[1:])
        out = []
        for i in range(n):
            for r in (res[0][i], rand[i]):
                if isinstance(r, Exception):
                    raise r
            rp, rp_com = res[0][i]
            assert enc_coms[i] is None or (rp_com == enc_coms[i]).all()
            proofs, pairs = rand[i]
            out.append(cls(pairs, proofs, rp, prove_range, check_percentage))
        return out

    def verify(self, verifier_seed=None, fp=None):
        """EncModelParams::verify, EncRange arm (params.rs:185-203): any Err counts as false (and so does anything else a
        crafted message can provoke while it is parsed)."""
        fp = api._fp(fp)
        try:
            k = _num_checked(self.enc_values.shape[0], self.check_percentage)
            ok, ok_range = _concurrently(
                lambda: rand_proof_vec.verify_randproof_vec(self.rand_proofs, self.enc_values),
                lambda: range_proof_vec.verify_rangeproof(self.range_proofs, self.enc_values[:k, :32], self.prove_range, verifier_seed=_sub_seed(verifier_seed, b"v"), fp=fp))
        except (RoflError, ValueError, OverflowError, IndexError) as e:
            if not _is_message_error(e):
                raise      # a fault of the verifier, not a verdict (see _MESSAGE_ERRORS)
            return False
        return bool(ok and ok_range)

    def _rand_key(self):      # the randomness proof's part of the shape key: the number of RandProofs (one per pair when well-formed)
        return self.rand_proofs.shape[0]

    @staticmethod
    def _rand_key_ok(key, d):
        return key == d

    @staticmethod
    def _rand_batch(us):
        return rand_proof_vec.verify_randproof_vec_batch([u.rand_proofs for u in us], [u.enc_values for u in us])

    @classmethod
    def verify_batch(cls, updates, verifier_seed=None, fp=None, _legs=_HostLegs):
        """The server's side of a round (server.rs:656-687 hands every client's update to the verification pool; :474-484 rejects the round
        when one fails): EncModelParams::verify, EncRange / EncRangeCompressed arms (params.rs:185-203, 235-256), for ALL clients of the round as two
        batched calls that run side by side -- the randomness proofs of every client in one launch sequence (_rand_batch) and the L-inf legs
        through rofl_verify_rangeproof_batch_strided over the first k pairs of every client, read in place from the 64-byte records.  One
        verdict per update, the same as update.verify() gives it; updates whose shape (d, the randomness proof's count or size, the range
        proofs' shape, prove_range, k) differs from the majority's are verified on their own.
        `_legs` is internal (not part of the interface): where the batched legs take the commitments from -- DeviceRound passes itself."""
        fp = api._fp(fp)
        n = len(updates)
        res = [False] * n
        if n == 0:
            return res

        def shape(u):
            try:
                d = u.enc_values.shape[0]
                return (d, u._rand_key(), u.range_proofs.shape if u.range_proofs.ndim == 2 else None, u.prove_range, _num_checked(d, u.check_percentage))
            except (AttributeError, RoflError):
                return None
        shapes = [shape(u) for u in updates]
        ok_shape = [sh for sh in shapes if sh is not None and sh[0] > 0 and cls._rand_key_ok(sh[1], sh[0]) and sh[2] is not None and sh[2][0] > 0 and sh[4] > 0]
        major = max(set(ok_shape), key=ok_shape.count) if ok_shape else None
        idx = [i for i, sh in enumerate(shapes) if major is not None and sh == major]
        for i, sh in enumerate(shapes):
            if major is None or sh != major:
                res[i] = bool(updates[i].verify(verifier_seed=verifier_seed, fp=fp))
        if not idx:
            return res
        us = [updates[i] for i in idx]
        k = major[4]
        try:
            ok_rand, ok_range = _concurrently(
                lambda: _legs.rand(cls, us, idx),
                lambda: _legs.range(us, idx, k, major[3], _sub_seed(verifier_seed, b"v"), fp, 64))
        except (RoflError, ValueError, OverflowError, IndexError) as e:
            if not _is_message_error(e):
                raise      # the verifier itself failed (HIP / RCCL runtime error): not a verdict about any client
            # a parameter of a batched call (a batch that has to be split, code 11) or a field of the majority shape that no proof can have:
            # client by client, which gives every member the verdict its own verify() gives
            for i in idx:
                res[i] = bool(updates[i].verify(verifier_seed=verifier_seed, fp=fp))
            return res
        for j, i in enumerate(idx):
            res[i] = bool(ok_rand[j] and ok_range[j])
        return res

    def serialize(self, as_array=False):
        return wire.encode(self.kind, enc_values=self.enc_values, rand_proof=self.rand_proofs, range_proofs=self.range_proofs,
                           range_bits=self.prove_range, check_percentage=self.check_percentage, as_array=as_array)

    @classmethod
    def deserialize(cls, data, copy=True):
        m = wire.decode(cls.kind, data, copy=copy)
        if m["enc_values"].size % 64 or m["rand_proof"].size % 128:
            raise RoflError(5, "FormatError")
        return cls(m["enc_values"], m["rand_proof"], m["range_proofs"], m["range_bits"], m["check_percentage"])

    def pedersen_part(self):
        return self.enc_values            # ElGamal pairs: accumulated as they are (gamal_accumulate)


class EncParamsRangeCompressed(EncParamsRange):
    """params.rs:683-775: same message, one CompressedRandProof (128 B) instead of d RandProofs."""

    def __init__(self, enc_values, rand_proof, range_proofs, prove_range, check_percentage):
        self.enc_values = np.ascontiguousarray(enc_values, dtype=np.uint8).reshape(-1, 64)
        self.rand_proof = np.ascontiguousarray(rand_proof, dtype=np.uint8).reshape(-1)
        self.range_proofs = np.ascontiguousarray(range_proofs, dtype=np.uint8)
        self.prove_range, self.check_percentage = int(prove_range), float(check_percentage)

    @classmethod
    def encrypt(cls, plaintext_vec, blinding_vec, prove_range, n_partition, check_percentage, nonce_seed=None, fp=None, quant_seed=None, noise_seed=None, noise_k=None):
        fp = api._fp(fp)
        x = np.ascontiguousarray(plaintext_vec, dtype=np.float32)
        bl = api._u8(blinding_vec)
        x, clipped = _clip_or_quantize(x, prove_range, quant_seed, fp, noise_seed, noise_k)
        wd = witness_digest(x, bl) if nonce_seed is not None else b""
        if check_percentage >= 1.0:
            enc_com = _range_commitments(clipped, bl, prove_range, fp)
            (rp, rp_com), (proof, pairs) = _concurrently(
                lambda: range_proof_vec.create_rangeproof(clipped, bl, prove_range, n_partition, nonce=_sub_nonce(nonce_seed, b"range", wd), fp=fp),
                lambda: compressed_rand_proof.helper_prove_existing(x, enc_com, bl, nonce=_sub_nonce(nonce_seed, b"rand", wd), fp=fp))
            assert (rp_com == enc_com).all()
        else:
            k = _num_checked(x.size, check_percentage)
            (rp, _), (proof, pairs) = _concurrently(
                lambda: range_proof_vec.create_rangeproof(clipped[:k], bl[:k], prove_range, n_partition, nonce=_sub_nonce(nonce_seed, b"range", wd), fp=fp),
                lambda: compressed_rand_proof.helper_prove(x, bl, nonce=_sub_nonce(nonce_seed, b"rand", wd), fp=fp))
        return cls(pairs, proof, rp, prove_range, check_percentage)

    @staticmethod
    def _rand_create_batch(xs, bls, enc_coms, nonces, fp):      # ONE rofl_create_compressed_randproof_batch for all clients
        return [lambda: compressed_rand_proof.helper_prove_batch(xs, bls, nonces=nonces, existing_list=enc_coms, fp=fp)], lambda res: res[0]

    def verify(self, verifier_seed=None, fp=None):
        fp = api._fp(fp)
        try:
            if self.rand_proof.size != 128:
                return False
            k = _num_checked(self.enc_values.shape[0], self.check_percentage)
            ok, ok_range = _concurrently(
                lambda: compressed_rand_proof.helper_verify(self.rand_proof, self.enc_values),
                lambda: range_proof_vec.verify_rangeproof(self.range_proofs, self.enc_values[:k, :32], self.prove_range, verifier_seed=_sub_seed(verifier_seed, b"v"), fp=fp))
        except (RoflError, ValueError, OverflowError, IndexError) as e:
            if not _is_message_error(e):
                raise      # a fault of the verifier, not a verdict (see _MESSAGE_ERRORS)
            return False
        return bool(ok and ok_range)

    def _rand_key(self):      # the size of the one CompressedRandProof
        return self.rand_proof.size

    @staticmethod
    def _rand_key_ok(key, d):
        return key == 128

    @staticmethod
    def _rand_batch(us):
        return compressed_rand_proof.helper_verify_batch([u.rand_proof for u in us], [u.enc_values for u in us])

    def serialize(self, as_array=False):
        return wire.encode(self.kind, enc_values=self.enc_values, rand_proof=self.rand_proof, range_proofs=self.range_proofs,
                           range_bits=self.prove_range, check_percentage=self.check_percentage, as_array=as_array)

    @classmethod
    def deserialize(cls, data, copy=True):
        m = wire.decode(cls.kind, data, copy=copy)
        if m["enc_values"].size % 64 or m["rand_proof"].size != 128:
            raise RoflError(5, "FormatError")
        return cls(m["enc_values"], m["rand_proof"], m["range_proofs"], m["range_bits"], m["check_percentage"])


def _rand_scalars(d, rand_scalars, rand_seed):
    """the r2 of one client: handed in, or the blinding stream of `rand_seed` (generated on the GPU), or fresh host randomness"""
    if rand_scalars is not None and rand_seed is not None:
        raise ValueError("rand_scalars and rand_seed exclude each other")
    if rand_scalars is not None:
        return api._u8(rand_scalars)
    return pedersen_ops.rnd_scalar_vec(d) if rand_seed is None else pedersen_ops.rnd_scalar_vec_seeded(d, rand_seed)


class EncParamsL2:
    """params.rs:544-681: per-element SquareRandProofs, L-inf range proofs, one L2 sum range proof."""
    kind = WIRE_ENC_NORM

    def __init__(self, enc_values, square_proofs, range_proofs, square_range_proof, prove_range, l2_prove_range):
        self.enc_values = np.ascontiguousarray(enc_values, dtype=np.uint8).reshape(-1, 96)
        self.square_proofs = np.ascontiguousarray(square_proofs, dtype=np.uint8).reshape(-1, 192)
        self.range_proofs = np.ascontiguousarray(range_proofs, dtype=np.uint8)
        self.square_range_proof = np.ascontiguousarray(square_range_proof, dtype=np.uint8).reshape(-1)
        self.prove_range, self.l2_prove_range = int(prove_range), int(l2_prove_range)

    @classmethod
    def encrypt(cls, plaintext_vec, blinding_vec, prove_range, n_partition, l2_range, nonce_seed=None, rand_scalars=None, fp=None, rand_seed=None, quant_seed=None, noise_seed=None, noise_k=None,
                l2_clip=None, clip_seed=None):
        # r2: rand_scalars, or the blinding stream of rand_seed (pedersen_ops.rnd_scalar_vec_seeded, on the GPU), or fresh host randomness
        fp = api._fp(fp)
        x = np.ascontiguousarray(plaintext_vec, dtype=np.float32)
        bl = api._u8(blinding_vec)
        r2 = _rand_scalars(x.size, rand_scalars, rand_seed)
        x, clipped = _clip_or_quantize(x, prove_range, quant_seed, fp, noise_seed, noise_k, l2_clip, clip_seed)
        wd = witness_digest(x, bl, r2) if nonce_seed is not None else b""
        # the square proofs take the range proof's commitments (params.rs:623-637); committing first (same points) lets the
        # three proofs run side by side
        enc_com = _range_commitments(clipped, bl, prove_range, fp)
        (rp, rp_com), (sum_proof, _), (proofs, commits) = _concurrently(
            lambda: range_proof_vec.create_rangeproof(clipped, bl, prove_range, n_partition, nonce=_sub_nonce(nonce_seed, b"range", wd), fp=fp),
            lambda: l2_range_proof_vec.create_rangeproof_l2(clipped, r2, l2_range, n_partition, nonce=_sub_nonce(nonce_seed, b"l2", wd), fp=fp),
            lambda: square_rand_proof_vec.create_l2rangeproof_vec_existing(clipped, enc_com, bl, r2, nonce=_sub_nonce(nonce_seed, b"sq", wd), fp=fp))
        assert (rp_com == enc_com).all()
        return cls(commits, proofs, rp, sum_proof, prove_range, l2_range)

    @classmethod
    def encrypt_batch(cls, clients, prove_range, n_partition, l2_range, nonce_seeds=None, fp=None):
        """_encrypt_batch (below) without probabilistic quantization: the clients' values are clipped, as encrypt() without a quant_seed does."""
        return cls._encrypt_batch(clients, prove_range, n_partition, l2_range, nonce_seeds, fp, None)

    @classmethod
    def encrypt_batch_quantized(cls, clients, prove_range, n_partition, l2_range, quant_seeds, nonce_seeds=None, fp=None):
        """encrypt_batch with quant_seeds = one 32-byte seed (or None: clip only) per client: ONE rofl_quantize_prob call rounds the values of
        all hosted clients, then the legs run as in encrypt_batch.  Byte-identical to encrypt(quant_seed=...) per client.  (A method of
        its own: the parameter list of encrypt_batch is pinned.)"""
        return cls._encrypt_batch(clients, prove_range, n_partition, l2_range, nonce_seeds, fp, quant_seeds)

    @classmethod
    def encrypt_batch_private(cls, clients, prove_range, n_partition, l2_range, nonce_seeds=None, fp=None, quant_seeds=None, noise_seeds=None, noise_k=None):
        """encrypt_batch_quantized with distributed noise: noise_seeds = one 32-byte seed (or None: no noise) per client and noise_k, both or
        neither.  After the ONE rofl_quantize_prob call of the quant_seeds, ONE rofl_noise_binomial call adds the noise of all hosted clients,
        then the legs run as in encrypt_batch.  Byte-identical to encrypt(quant_seed=..., noise_seed=..., noise_k=...) per client, and
        without noise seeds to encrypt_batch_quantized.  The noise raises the norm: an update it pushes over the L2 bound fails with
        NormOutOfRangeError (7).  (A method of its own: the parameter lists of encrypt_batch and encrypt_batch_quantized are pinned.)"""
        _noise_args(noise_seeds, noise_k)
        return cls._encrypt_batch(clients, prove_range, n_partition, l2_range, nonce_seeds, fp, quant_seeds, noise_seeds, noise_k)

    @classmethod
    def encrypt_batch_clipped(cls, clients, prove_range, n_partition, l2_range, nonce_seeds=None, fp=None, quant_seeds=None, noise_seeds=None, noise_k=None, l2_clip=None, clip_seeds=None):
        """encrypt_batch_private with norm clipping: l2_clip = the budget in grid steps^2 (an int, or one per client;
        l2_range_proof_vec.norm_budget) and clip_seeds = None or one 32-byte seed (or None: truncate) per client.  Between the ONE
        rofl_quantize_prob call and the ONE rofl_noise_binomial call, ONE rofl_clip_l2 call projects the updates of all hosted clients
        onto the ball, so that none of them fails the norm check of its sum proof.  Byte-identical to encrypt(..., l2_clip=, clip_seed=)
        per client, and with l2_clip=None to encrypt_batch_private.  (A method of its own: the parameter lists of the other
        encrypt_batch* methods are pinned.)"""
        _noise_args(noise_seeds, noise_k); _clip_args(l2_clip, clip_seeds)
        return cls._encrypt_batch(clients, prove_range, n_partition, l2_range, nonce_seeds, fp, quant_seeds, noise_seeds, noise_k, l2_clip, clip_seeds)

    @classmethod
    def _encrypt_batch(cls, clients, prove_range, n_partition, l2_range, nonce_seeds, fp, quant_seeds, noise_seeds=None, noise_k=None, l2_clip=None, clip_seeds=None):
        """encrypt() for several clients of one process (rofl_service's client binary hosts its clients as tasks of one process,
        client.rs:265-266): clients = [(plaintext_vec, blinding_vec, rand_scalars or None), ...] of one length.  The L-inf legs of all of
        them are ONE rofl_create_rangeproof_batch call (one launch sequence, one set of host hops), their sum proofs ONE
        rofl_create_rangeproof_l2_batch and their square proofs ONE rofl_create_sigmaproof_vec_batch: three calls side by side on three
        lanes.  Every container is byte-identical to what encrypt() returns for that client with the same nonce seed; a client that fails
        raises.  (Seeded r2 for a batch: ONE pedersen_ops.blinding_vecs call over the clients' seeds, its rows handed in as rand_scalars --
        the bytes of encrypt(rand_seed=...).)"""
        fp = api._fp(fp)
        n = len(clients)
        if n == 0:
            return []
        seeds = list(nonce_seeds) if nonce_seeds is not None else [None] * n
        xs, bls, r2s, wds, clipped = [], [], [], [], []
        for (x, bl, r2) in clients:
            x = np.ascontiguousarray(x, dtype=np.float32); bl = api._u8(bl)
            r2 = pedersen_ops.rnd_scalar_vec(x.size) if r2 is None else api._u8(r2)
            xs.append(x); bls.append(bl); r2s.append(r2)
        xs, clipped = _clip_or_quantize_batch(xs, prove_range, quant_seeds, fp, noise_seeds, noise_k, l2_clip, clip_seeds)      # (ONE quantize, ONE clip and ONE noise call for all hosted clients)
        d = xs[0].size
        if any(x.size != d for x in xs):
            raise ValueError("the clients of a batch have one vector length")
        wds = [witness_digest(x, bl, r2) if sd is not None else b"" for x, bl, r2, sd in zip(xs, bls, r2s, seeds)]
        # the range proofs' commitments, computed first (one call for all clients) so that the square proofs can complete them while the range proofs run
        enc_all = _range_commitments(np.concatenate(clipped), np.concatenate(bls), prove_range, fp)
        enc_com = [enc_all[i * d:(i + 1) * d] for i in range(n)]
        def nonces(tag):
            return [_sub_nonce(sd, tag, wd) for sd, wd in zip(seeds, wds)]
        res = _concurrently(
            lambda: range_proof_vec.create_rangeproof_batch(clipped, bls, prove_range, n_partition, nonces=nonces(b"range"), fp=fp),
            lambda: l2_range_proof_vec.create_rangeproof_l2_batch(clipped, r2s, l2_range, n_partition, nonces=nonces(b"l2"), fp=fp),
            lambda: square_rand_proof_vec.create_l2rangeproof_vec_batch(clipped, bls, r2s, nonces=nonces(b"sq"), existing_list=enc_com, fp=fp))
        out = []
        for i in range(n):
            for r in (res[0][i], res[1][i], res[2][i]):
                if isinstance(r, Exception):
                    raise r
            (rp, rp_com), (sum_proof, _), (proofs, commits) = res[0][i], res[1][i], res[2][i]
            assert (rp_com == enc_com[i]).all()
            out.append(cls(commits, proofs, rp, sum_proof, prove_range, l2_range))
        return out

    def _sum_c_sq(self):
        return pedersen_ops.sum_rp_vec(self.enc_values[:, 64:96])

    def verify(self, verifier_seed=None, fp=None):
        """EncModelParams::verify, EncL2 arm (params.rs:204-232)."""
        fp = api._fp(fp)
        try:
            ok, ok_range, ok_sum = _concurrently(
                lambda: square_rand_proof_vec.verify_l2rangeproof_vec(self.square_proofs, self.enc_values),
                lambda: range_proof_vec.verify_rangeproof(self.range_proofs, self.enc_values[:, :32], self.prove_range, verifier_seed=_sub_seed(verifier_seed, b"v"), fp=fp),
                lambda: l2_range_proof_vec.verify_rangeproof_l2(self.square_range_proof, self._sum_c_sq(), self.l2_prove_range, verifier_seed=_sub_seed(verifier_seed, b"s"), fp=fp))
        except (RoflError, ValueError, OverflowError, IndexError) as e:
            if not _is_message_error(e):
                raise      # a fault of the verifier, not a verdict (see _MESSAGE_ERRORS)
            return False
        return bool(ok and ok_range and ok_sum)

    @staticmethod
    def _square_batch(us):
        return square_rand_proof_vec.verify_l2rangeproof_vec_batch([u.square_proofs for u in us], [u.enc_values for u in us], with_csq_sums=True)

    _checks_rand = False      # a randomness leg of its own beside the square proofs (EncParamsL2CompressedStrict; here the SquareRandProofs bind R)

    def _rand_key(self):      # the randomness leg's part of the shape key
        return ()

    @classmethod
    def verify_batch(cls, updates, verifier_seed=None, fp=None, _legs=_HostLegs):
        """The server's side of a round (server.rs:656-687 hands every client's update to the verification pool; :474-484 rejects the round
        when one fails): EncModelParams::verify, EncL2 arm (params.rs:204-232), for ALL clients of the round as three batched calls that run
        side by side -- the square proofs of every client in one launch sequence (rofl_verify_squarerandproof_vec_batch, which also hands
        back every client's sum of c_sq), the L-inf legs through rofl_verify_rangeproof_batch_strided (commitments read in place from the
        96-byte SquareRandProofCommitments; one random-weighted equation per batch with verify_batch = 2) and, once the sums are there, the
        L2 sum proofs through rofl_verify_rangeproof_l2_batch.  One verdict per client, the same as update.verify() gives each of them;
        clients whose shapes differ from the majority's are verified on their own.
        `_legs` is internal (not part of the interface): where the batched legs take the commitments from -- DeviceRound passes itself."""
        fp = api._fp(fp)
        n = len(updates)
        res = [False] * n
        if n == 0:
            return res
        def shape(u):
            try:
                return (u.enc_values.shape[0], u.square_proofs.shape[0], u.range_proofs.shape if u.range_proofs.ndim == 2 else None, u.square_range_proof.size, u.prove_range, u.l2_prove_range) + u._rand_key()
            except AttributeError:
                return None
        shapes = [shape(u) for u in updates]
        ok_shape = [sh for sh in shapes if sh is not None and sh[0] == sh[1] and sh[0] > 0 and sh[2] is not None and sh[2][0] > 0 and all(sh[6:])]
        if not ok_shape:
            return [u.verify(verifier_seed=verifier_seed, fp=fp) if sh is not None else False for u, sh in zip(updates, shapes)]
        major = max(set(ok_shape), key=ok_shape.count)
        idx = [i for i, sh in enumerate(shapes) if sh == major]
        for i, sh in enumerate(shapes):
            if sh != major:
                res[i] = bool(sh is not None and updates[i].verify(verifier_seed=verifier_seed, fp=fp))
        us = [updates[i] for i in idx]
        def sigma_then_sum():
            ok_sq, sums = _legs.square(cls, us, idx)
            if kernel_time_sink is not None:
                kernel_time_sink(api.last_kernel_times())      # (this thread makes two calls; _timed reports the second)
            ok_sum = l2_range_proof_vec.verify_rangeproof_l2_batch([u.square_range_proof for u in us], sums, major[5], verifier_seed=_sub_seed(verifier_seed, b"s"), fp=fp)
            return ok_sq, ok_sum
        try:
            (ok_sq, ok_sum), ok_range, *ok_rand = _concurrently(
                sigma_then_sum,
                lambda: _legs.range(us, idx, major[0], major[4], _sub_seed(verifier_seed, b"v"), fp, 96),
                *([lambda: _legs.rand(cls, us, idx)] if cls._checks_rand else []))
        except (RoflError, ValueError, OverflowError, IndexError) as e:
            if not _is_message_error(e):
                raise      # the verifier itself failed (HIP / RCCL runtime error): not a verdict about any client
            if isinstance(e, RoflError) and e.code == 11:      # a parameter of the batched call (a batch that has to be split, or a field of the majority shape): client by client
                for i in idx:
                    res[i] = bool(updates[i].verify(verifier_seed=verifier_seed, fp=fp))
                return [bool(r) for r in res]
            # (a call-level error -- a proof length no proof can have, a bit size outside 8 / 16 / 32 / 64: every member of this shape is malformed the same way)
            return [bool(r) for r in res]
        for k, i in enumerate(idx):
            res[i] = bool(ok_sq[k] and ok_range[k] and ok_sum[k] and all(r[k] for r in ok_rand))
        return res

    def serialize(self, as_array=False):
        return wire.encode(self.kind, enc_values=self.enc_values, square_proof=self.square_proofs, range_proofs=self.range_proofs,
                           square_range_proof=self.square_range_proof, range_bits=self.prove_range, l2_range_bits=self.l2_prove_range, as_array=as_array)

    @classmethod
    def deserialize(cls, data, copy=True):
        m = wire.decode(cls.kind, data, copy=copy)
        if m["enc_values"].size % 96 or m["square_proof"].size % 192:
            raise RoflError(5, "FormatError")
        return cls(m["enc_values"], m["square_proof"], m["range_proofs"], m["square_range_proof"], m["range_bits"], m["l2_range_bits"])

    def pedersen_part(self):
        return self.enc_values[:, :64]    # the ElGamal pair c of every SquareRandProofCommitments (l2_vec_accumulate)


class EncParamsL2Compressed(EncParamsL2):
    """params.rs:790-885: SquareProofs (160 B) + one CompressedRandProof; commitments kept as SquareRandProofCommitments."""
    kind = WIRE_ENC_NORM_COMPRESSED

    def __init__(self, enc_values, square_proofs, rand_proof, range_proofs, square_range_proof, prove_range, l2_prove_range):
        self.enc_values = np.ascontiguousarray(enc_values, dtype=np.uint8).reshape(-1, 96)
        self.square_proofs = np.ascontiguousarray(square_proofs, dtype=np.uint8).reshape(-1, 160)
        self.rand_proof = np.ascontiguousarray(rand_proof, dtype=np.uint8).reshape(-1)
        self.range_proofs = np.ascontiguousarray(range_proofs, dtype=np.uint8)
        self.square_range_proof = np.ascontiguousarray(square_range_proof, dtype=np.uint8).reshape(-1)
        self.prove_range, self.l2_prove_range = int(prove_range), int(l2_prove_range)

    @classmethod
    def encrypt(cls, plaintext_vec, blinding_vec, prove_range, n_partition, l2_range, nonce_seed=None, rand_scalars=None, fp=None, rand_seed=None, quant_seed=None, noise_seed=None, noise_k=None,
                l2_clip=None, clip_seed=None):
        fp = api._fp(fp)
        x = np.ascontiguousarray(plaintext_vec, dtype=np.float32)
        bl = api._u8(blinding_vec)
        r2 = _rand_scalars(x.size, rand_scalars, rand_seed)
        x, clipped = _clip_or_quantize(x, prove_range, quant_seed, fp, noise_seed, noise_k, l2_clip, clip_seed)
        wd = witness_digest(x, bl, r2) if nonce_seed is not None else b""
        enc_com = _range_commitments(clipped, bl, prove_range, fp)
        (rp, rp_com), (sum_proof, _), (rand_proof, pairs) = _concurrently(
            lambda: range_proof_vec.create_rangeproof(clipped, bl, prove_range, n_partition, nonce=_sub_nonce(nonce_seed, b"range", wd), fp=fp),
            lambda: l2_range_proof_vec.create_rangeproof_l2(clipped, r2, l2_range, n_partition, nonce=_sub_nonce(nonce_seed, b"l2", wd), fp=fp),
            lambda: compressed_rand_proof.helper_prove_existing(clipped, enc_com, bl, nonce=_sub_nonce(nonce_seed, b"rand", wd), fp=fp))
        assert (rp_com == enc_com).all()
        sq_proofs, sq_commits = square_proof_vec.create_l2rangeproof_vec_existing(clipped, enc_com, bl, r2, nonce=_sub_nonce(nonce_seed, b"sq", wd), fp=fp)
        merged = np.concatenate([pairs, sq_commits[:, 32:64]], axis=1)        # merge(): c = ElGamal pair, c_sq from the square proof (params.rs:777-787)
        return cls(merged, sq_proofs, rand_proof, rp, sum_proof, prove_range, l2_range)

    @classmethod
    def encrypt_batch(cls, clients, prove_range, n_partition, l2_range, nonce_seeds=None, fp=None):
        """_encrypt_batch (below) without probabilistic quantization: the clients' values are clipped, as encrypt() without a quant_seed does."""
        return cls._encrypt_batch(clients, prove_range, n_partition, l2_range, nonce_seeds, fp, None)

    @classmethod
    def encrypt_batch_quantized(cls, clients, prove_range, n_partition, l2_range, quant_seeds, nonce_seeds=None, fp=None):
        """encrypt_batch with quant_seeds = one 32-byte seed (or None: clip only) per client: ONE rofl_quantize_prob call rounds the values of
        all hosted clients, then the legs run as in encrypt_batch.  Byte-identical to encrypt(quant_seed=...) per client.  (A method of
        its own: the parameter list of encrypt_batch is pinned.)"""
        return cls._encrypt_batch(clients, prove_range, n_partition, l2_range, nonce_seeds, fp, quant_seeds)

    @classmethod
    def encrypt_batch_private(cls, clients, prove_range, n_partition, l2_range, nonce_seeds=None, fp=None, quant_seeds=None, noise_seeds=None, noise_k=None):
        """encrypt_batch_quantized with distributed noise: noise_seeds = one 32-byte seed (or None: no noise) per client and noise_k, both or
        neither.  After the ONE rofl_quantize_prob call of the quant_seeds, ONE rofl_noise_binomial call adds the noise of all hosted clients,
        then the legs run as in encrypt_batch.  Byte-identical to encrypt(quant_seed=..., noise_seed=..., noise_k=...) per client, and
        without noise seeds to encrypt_batch_quantized.  The noise raises the norm: an update it pushes over the L2 bound fails with
        NormOutOfRangeError (7).  (A method of its own: the parameter lists of encrypt_batch and encrypt_batch_quantized are pinned.)"""
        _noise_args(noise_seeds, noise_k)
        return cls._encrypt_batch(clients, prove_range, n_partition, l2_range, nonce_seeds, fp, quant_seeds, noise_seeds, noise_k)

    @classmethod
    def encrypt_batch_clipped(cls, clients, prove_range, n_partition, l2_range, nonce_seeds=None, fp=None, quant_seeds=None, noise_seeds=None, noise_k=None, l2_clip=None, clip_seeds=None):
        """encrypt_batch_private with norm clipping: l2_clip = the budget in grid steps^2 (an int, or one per client;
        l2_range_proof_vec.norm_budget) and clip_seeds = None or one 32-byte seed (or None: truncate) per client.  Between the ONE
        rofl_quantize_prob call and the ONE rofl_noise_binomial call, ONE rofl_clip_l2 call projects the updates of all hosted clients
        onto the ball, so that none of them fails the norm check of its sum proof.  Byte-identical to encrypt(..., l2_clip=, clip_seed=)
        per client, and with l2_clip=None to encrypt_batch_private.  (A method of its own: the parameter lists of the other
        encrypt_batch* methods are pinned.)"""
        _noise_args(noise_seeds, noise_k); _clip_args(l2_clip, clip_seeds)
        return cls._encrypt_batch(clients, prove_range, n_partition, l2_range, nonce_seeds, fp, quant_seeds, noise_seeds, noise_k, l2_clip, clip_seeds)

    @classmethod
    def _encrypt_batch(cls, clients, prove_range, n_partition, l2_range, nonce_seeds, fp, quant_seeds, noise_seeds=None, noise_k=None, l2_clip=None, clip_seeds=None):
        """encrypt() for several clients of one process: clients = [(plaintext_vec, blinding_vec, rand_scalars or None), ...] of one
        length.  The 8-bit legs of all of them are ONE rofl_create_rangeproof_batch call, their compressed randomness proofs ONE
        rofl_create_compressed_randproof_batch over the range proofs' commitments, their sum proofs ONE rofl_create_rangeproof_l2_batch and
        their SquareProofs ONE rofl_create_sigmaproof_vec_batch: four calls side by side on the lanes.  Every container is byte-identical to what encrypt() returns for that client with the same nonce
        seed; a client that fails raises."""
        fp = api._fp(fp)
        n = len(clients)
        if n == 0:
            return []
        seeds = list(nonce_seeds) if nonce_seeds is not None else [None] * n
        xs, bls, r2s, clipped = [], [], [], []
        for (x, bl, r2) in clients:
            x = np.ascontiguousarray(x, dtype=np.float32); bl = api._u8(bl)
            r2 = pedersen_ops.rnd_scalar_vec(x.size) if r2 is None else api._u8(r2)
            xs.append(x); bls.append(bl); r2s.append(r2)
        xs, clipped = _clip_or_quantize_batch(xs, prove_range, quant_seeds, fp, noise_seeds, noise_k, l2_clip, clip_seeds)      # (ONE quantize, ONE clip and ONE noise call for all hosted clients)
        d = xs[0].size
        if any(x.size != d for x in xs):
            raise ValueError("the clients of a batch have one vector length")
        wds = [witness_digest(x, bl, r2) if sd is not None else b"" for x, bl, r2, sd in zip(xs, bls, r2s, seeds)]
        enc_all = _range_commitments(np.concatenate(clipped), np.concatenate(bls), prove_range, fp)
        enc_com = [enc_all[i * d:(i + 1) * d] for i in range(n)]
        def nonces(tag):
            return [_sub_nonce(sd, tag, wd) for sd, wd in zip(seeds, wds)]
        res = _concurrently(
            lambda: range_proof_vec.create_rangeproof_batch(clipped, bls, prove_range, n_partition, nonces=nonces(b"range"), fp=fp),
            lambda: compressed_rand_proof.helper_prove_batch(clipped, bls, nonces=nonces(b"rand"), existing_list=enc_com, fp=fp),
            lambda: l2_range_proof_vec.create_rangeproof_l2_batch(clipped, r2s, l2_range, n_partition, nonces=nonces(b"l2"), fp=fp),
            lambda: square_proof_vec.create_l2rangeproof_vec_batch(clipped, bls, r2s, nonces=nonces(b"sq"), existing_list=enc_com, fp=fp))
        out = []
        for i in range(n):
            for r in (res[0][i], res[1][i], res[2][i], res[3][i]):
                if isinstance(r, Exception):
                    raise r
            (rp, rp_com), (rand_proof, pairs), (sum_proof, _), (sq_proofs, sq_commits) = res[0][i], res[1][i], res[2][i], res[3][i]
            assert (rp_com == enc_com[i]).all()
            merged = np.concatenate([pairs, sq_commits[:, 32:64]], axis=1)        # merge(), as in encrypt()
            out.append(cls(merged, sq_proofs, rand_proof, rp, sum_proof, prove_range, l2_range))
        return out

    @staticmethod
    def _square_batch(us):      # SquareProofCommitments { c_l: c.L, c_sq } (params.rs:262-266); the reference's arm skips the compressed randomness proof, as verify() does -- EncParamsL2CompressedStrict checks it
        return square_proof_vec.verify_l2rangeproof_vec_batch([u.square_proofs for u in us], [np.concatenate([u.enc_values[:, :32], u.enc_values[:, 64:96]], axis=1) for u in us], with_csq_sums=True)

    def verify(self, verifier_seed=None, fp=None):
        """EncModelParams::verify, EncL2Compressed arm (params.rs:255-289).  NB: the reference's arm skips the compressed randomness
        proof (it only verifies the square proofs, the range proofs and the sum, none of which reads R), and so does this class, verdict
        for verdict.  EncParamsL2CompressedStrict is the class that checks it."""
        fp = api._fp(fp)
        try:
            oks = _concurrently(*self._verify_legs(verifier_seed, fp))
        except (RoflError, ValueError, OverflowError, IndexError) as e:
            if not _is_message_error(e):
                raise      # a fault of the verifier, not a verdict (see _MESSAGE_ERRORS)
            return False
        return all(bool(ok) for ok in oks)

    def _verify_legs(self, verifier_seed, fp):
        """the legs of verify() as thunks that run side by side: the SquareProofs, the L-inf range proofs, the L2 sum proof"""
        sqc = np.concatenate([self.enc_values[:, :32], self.enc_values[:, 64:96]], axis=1)      # SquareProofCommitments { c_l: c.L, c_sq }
        return [lambda: square_proof_vec.verify_l2rangeproof_vec(self.square_proofs, sqc),
                lambda: range_proof_vec.verify_rangeproof(self.range_proofs, self.enc_values[:, :32], self.prove_range, verifier_seed=_sub_seed(verifier_seed, b"v"), fp=fp),
                lambda: l2_range_proof_vec.verify_rangeproof_l2(self.square_range_proof, self._sum_c_sq(), self.l2_prove_range, verifier_seed=_sub_seed(verifier_seed, b"s"), fp=fp)]

    def serialize(self, as_array=False):
        return wire.encode(self.kind, enc_values=self.enc_values, square_proof=self.square_proofs, rand_proof=self.rand_proof,
                           range_proofs=self.range_proofs, square_range_proof=self.square_range_proof, range_bits=self.prove_range,
                           l2_range_bits=self.l2_prove_range, as_array=as_array)

    @classmethod
    def deserialize(cls, data, copy=True):
        m = wire.decode(cls.kind, data, copy=copy)
        if m["enc_values"].size % 96 or m["square_proof"].size % 160 or m["rand_proof"].size != 128:
            raise RoflError(5, "FormatError")
        return cls(m["enc_values"], m["square_proof"], m["rand_proof"], m["range_proofs"], m["square_range_proof"], m["range_bits"], m["l2_range_bits"])


class EncParamsL2CompressedStrict(EncParamsL2Compressed):
    """EncParamsL2Compressed -- same wire kind, same bytes, same encrypt / encrypt_batch / serialize / deserialize -- whose verify() and
    verify_batch() also check the update's CompressedRandProof, over enc_values in place (the pair is the first 64 bytes of every 96-byte
    record).  The reference's EncL2Compressed arm (params.rs:257-289) never reads rand_proof: the SquareProofs and the range proofs read
    only L and c_sq, so ANY valid points pass as R, the round's aggregate R is then not the identity, extract() returns None and the
    server cannot tell which client did it.  This class is the opt-in that closes the hole; a verdict is True only if the three legs of
    EncParamsL2Compressed and the randomness proof all hold."""
    _checks_rand = True

    def _rand_key(self):      # the size of the one CompressedRandProof (128 when well-formed: anything else is off the majority shape)
        return (self.rand_proof.size == 128,)

    @staticmethod
    def _rand_batch(us):
        return compressed_rand_proof.helper_verify_batch_strided([u.rand_proof for u in us], [u.enc_values for u in us], 96)

    def _verify_legs(self, verifier_seed, fp):
        """verify() runs four legs side by side and is true only if all four are: the three of EncParamsL2Compressed and the
        CompressedRandProof (params.rs:235-256, the check of the EncRangeCompressed arm) over (L, R) of enc_values in place.  A proof
        that is not 128 bytes is False there without reaching the library."""
        return EncParamsL2Compressed._verify_legs(self, verifier_seed, fp) + [
            lambda: compressed_rand_proof.helper_verify_batch_strided([self.rand_proof], [self.enc_values], 96)[0]]


class EncModelParamsAccumulator:
    """params.rs:74-138 (Enc variant): element-wise sum of ElGamal pairs, then unity check + BSGS extraction."""

    def __init__(self, size):
        # (identity, identity) = 64 zero bytes, unity check R == identity: extract() returns the true sum.  The reference starts from
        # ElGamalPair::unity() = (B, B) instead (el_gamal.rs:83-88, params.rs:173) and checks R == B: DeviceAccumulator(reference_unity=True)
        self.acc = np.zeros((size, 64), dtype=np.uint8)

    @classmethod
    def unity(cls, size):
        return cls(size)

    def accumulate_other(self, other):
        pairs = np.ascontiguousarray(other.pedersen_part(), dtype=np.uint8).reshape(-1, 64)
        n = min(pairs.shape[0], self.acc.shape[0])             # zip() truncates
        summed = pedersen_ops.add_rp_vec(self.acc[:n].reshape(-1, 32), pairs[:n].reshape(-1, 32))
        self.acc[:n] = summed.reshape(-1, 64)
        return True

    def extract(self, table_size=None, bsgs_bits=16, fp=None, opening=None):
        """None when some R component is not the identity (the blindings did not cancel), else the f32 aggregate.
        opening (uint8[size, 32]): the sum of the summed clients' blinding vectors, for a round that left somebody out -- every R must be
        opening * B (else None), and opening * B~ is taken off L first.  Composed from commit_vec / add_rp_vec / discrete_log_vec: the
        host-side counterpart of DeviceAccumulator.extract_opened, three device calls and their transfers instead of one."""
        fp = api._fp(fp)
        if opening is not None:
            s = pedersen_ops.add_scalar_vec(api._u8(opening), pedersen_ops.zero_scalar_vec(self.acc.shape[0]))      # canonical
            if self.acc[:, 32:64].tobytes() != pedersen_ops.commit_no_blinding_vec(s).tobytes():      # (encodings are canonical: byte equality is point equality)
                return None
            minus = pedersen_ops.add_scalar_vec(pedersen_ops.zero_scalar_vec(s.shape[0]), s, subtract=True)
            pts = pedersen_ops.add_rp_vec(np.ascontiguousarray(self.acc[:, :32]), pedersen_ops.commit_vec(pedersen_ops.zero_scalar_vec(s.shape[0]), minus))
        elif np.any(self.acc[:, 32:64]):
            return None
        else:
            pts = np.ascontiguousarray(self.acc[:, :32])
        sc = pedersen_ops.default_discrete_log_vec(pts, fp=fp) if table_size is None else pedersen_ops.discrete_log_vec(pts, table_size, bsgs_bits)
        return conversion32.scalar_to_f32_vec(sc, fp=fp)


class DeviceAccumulator:
    """EncModelParamsAccumulator with the round's running sum kept on the device (rofl_acc_*): every update is decoded once and added in
    extended coordinates; nothing is encoded until export() / extract(), and extraction (unity check, BSGS) runs on the device too.

    reference_unity=False: starts from (identity, identity) and checks R == identity -- the same bytes and values as EncModelParamsAccumulator.
    reference_unity=True: starts from ElGamalPair::unity() = (B, B) and checks R == B, as the reference does (params.rs:173, 176;
    el_gamal.rs:83-88, 101-103): its aggregate is the sum plus one raw fixed-point unit per coordinate.
    The accumulator lives on the device of the calling thread; partial sums of several devices merge by accumulate_pairs(other.export())
    (partials created with reference_unity=False: a (B, B) partial would count B twice)."""

    def __init__(self, size, reference_unity=False):
        self.size, self.reference_unity = int(size), bool(reference_unity)
        self._open = False
        self.last_first_bad = None      # after extract_opened() returned None: the smallest failing coordinate
        self._h = api.accumulator.create(self.size, 1 if self.reference_unity else 0)
        self._open = True

    @classmethod
    def unity(cls, size, reference_unity=False):
        return cls(size, reference_unity)

    @staticmethod
    def _records(update):
        """(array, stride) of an update's ElGamal pairs as they are held: L2 containers keep SquareRandProofCommitments (96 B, the pair c
        first), read in place without a copy"""
        if isinstance(update, EncParamsL2):
            return update.enc_values, 96
        return np.ascontiguousarray(update.pedersen_part(), dtype=np.uint8).reshape(-1, 64), 64

    def _add(self, arrays, stride):
        ptrs, counts = [], []
        for a in arrays:
            if api._is_dev(a):
                p, nbytes = api._dev_arg(a, 1)
                ptrs.append(p.value); counts.append(nbytes // stride)
            else:
                if not (a.flags.c_contiguous and a.dtype == np.uint8 and a.ndim == 2 and a.shape[1] == stride):
                    raise ValueError("records must be a contiguous uint8 array of shape (n, stride)")
                ptrs.append(a.ctypes.data); counts.append(a.shape[0])
        api.accumulator.add(self._h, ptrs, counts, stride)
        return arrays      # (kept alive by the caller until here)

    def accumulate_other(self, other):
        """gamal_accumulate / l2_vec_accumulate of one update (params.rs:81-104): zip() truncates to the accumulator's length"""
        a, stride = self._records(other)
        self._add([a], stride)
        return True

    def accumulate_batch(self, updates):
        """all updates of a round (or a part of it) in ONE rofl_acc_add: all or nothing -- a record that does not decode raises FormatError
        and leaves the sum as it was"""
        recs = [self._records(u) for u in updates]
        if not recs:
            return True
        strides = {st for _, st in recs}
        if len(strides) == 1:
            self._add([a for a, _ in recs], strides.pop())
        else:      # mixed containers: the pairs of the 96-byte records packed (one call keeps the batch all or nothing)
            self._add([a if st == 64 else np.ascontiguousarray(a[:, :64]) for a, st in recs], 64)
        return True

    def accumulate_pairs(self, pairs, stride=64):
        """one client's records: a (n, stride) uint8 array, or a contiguous uint8 GPU tensor of n * stride bytes (read on the device)"""
        if api._is_dev(pairs):
            self._add([pairs], int(stride))
        else:
            self._add([np.ascontiguousarray(pairs, dtype=np.uint8).reshape(-1, int(stride))], int(stride))
        return True

    def export(self):
        """(size, 64) encodings of the current sums (EncModelParamsAccumulator.acc for reference_unity=False)"""
        return api.accumulator.export(self._h, self.size)

    def extract(self, table_size=None, bsgs_bits=16, fp=None):
        """None when some R is not the initial one (the blindings did not cancel), else the f32 aggregate -- as
        EncModelParamsAccumulator.extract (table_size None: BSGSTable::default() of the fixed-point type)"""
        fp = api._fp(fp)
        if table_size is None:
            table_size, bsgs_bits = api.default_bsgs(fp)
        return api.accumulator.extract(self._h, self.size, table_size, bsgs_bits, fp)

    def extract_opened(self, opening=None, opening_terms=None, table_size=None, bsgs_bits=16, fp=None):
        """extract() for a round that left somebody out: the summed clients' blindings leave a residual in every pair, and the caller hands
        in its opening -- as `opening` (uint8[size, 32], or a torch uint8 tensor on the GPU: the sum of the summed clients' blinding
        vectors) or as `opening_terms` ([(seed32, sign), ...] from pedersen_ops.pairwise_residual_terms / cancelling_residual_terms: the
        opening is then built on the device and never exists on the host).  Exactly one of the two, else ValueError.  The opening is checked
        against every R before anything is extracted: a wrong one gives None, and last_first_bad holds the smallest coordinate it fails at
        (None after a success).  The accumulator is not changed.  (A method of its own: extract()'s parameter list is pinned.)"""
        if (opening is None) == (opening_terms is None):
            raise ValueError("exactly one of opening and opening_terms")
        fp = api._fp(fp)
        if table_size is None:
            table_size, bsgs_bits = api.default_bsgs(fp)
        if opening is not None:
            values, self.last_first_bad = api.accumulator.extract_opened(self._h, self.size, opening, table_size, bsgs_bits, fp)
        else:
            values, self.last_first_bad = api.accumulator.extract_opened_terms(self._h, self.size, opening_terms, table_size, bsgs_bits, fp)
        return values

    def reset(self):
        api.accumulator.reset(self._h)

    def close(self):
        """frees the device memory (once); later calls on the accumulator raise RoflError 11"""
        if getattr(self, "_open", False):
            self._open = False
            api.accumulator.destroy(self._h)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class DeviceRound:
    """One round of updates of container class `cls`, resident on the device (rofl_round_*): every update is uploaded once and every point
    of its enc_values decoded once, as it is ingested; verify() runs the legs of cls.verify_batch over the decoded points and
    accumulate_into() adds the accepted updates to a DeviceAccumulator from the same points -- no second upload, no second decode.

        with DeviceRound(EncParamsL2, d, max_clients=48) as rnd:
            rnd.ingest(updates[:20]); rnd.ingest(updates[20:])      # as the messages arrive (enc_values read in place)
            ok = rnd.verify()                                       # == EncParamsL2.verify_batch(updates)
            rnd.accumulate_into(acc, accept=ok)                     # acc.export() == acc.accumulate_batch(accepted updates)

    Updates whose enc_values are not `size` records cannot sit in the cache: they are kept in the list, verified on their own and
    accumulated through acc.accumulate_batch (zip truncation included), as are members whose proofs are off the round's majority shape.
    The records are a snapshot: enc_values are copied to the device at ingest() and never read again, while the proofs are read from the
    update objects at verify() -- an update changed in place after it was ingested must be ingested again (reset()).
    A round of EncParamsRangeCompressed also hashes, at ingest, each update's CompressedRandProof transcript up to the proof's C' from the
    bytes that go to the device (rofl_round_create_ex, ROFL_ROUND_COMPRESSED): its randomness leg continues those transcripts over the
    decoded points (rofl_round_verify_compressed) and, like every other leg, gives its verdict about the snapshot that accumulate_into
    adds.  A round of EncParamsL2CompressedStrict does the same over its 96-byte records (rofl_round_create_rand: the pair is the first 64
    bytes of each); a round of EncParamsL2Compressed hashes nothing at ingest and checks no randomness proof, as the reference's arm.
    The round lives on the device of the thread that created it."""

    def __init__(self, cls, size, max_clients):
        if cls not in (EncParamsRange, EncParamsRangeCompressed, EncParamsL2, EncParamsL2Compressed, EncParamsL2CompressedStrict):
            raise ValueError("cls must be one of the encrypted-update containers")
        self.cls, self.size, self.max_clients = cls, int(size), int(max_clients)
        self.record_len = 96 if issubclass(cls, EncParamsL2) else 64
        self.updates, self._slot, self._n_cached = [], [], 0
        self._open = False
        # (d >= 900 000 is past what a CompressedRandProof can have: such a round keeps the host call, which refuses it member by member)
        self._compressed = cls in (EncParamsRangeCompressed, EncParamsL2CompressedStrict) and self.size < 900000
        if self._compressed and cls is EncParamsL2CompressedStrict:
            self._h = api.device_round.create_rand(self.size, self.record_len, self.max_clients)
        else:
            self._h = api.device_round.create(self.size, self.record_len, self.max_clients, api.device_round.COMPRESSED if self._compressed else 0)
        self._open = True

    def __len__(self):
        return len(self.updates)

    def _check_open(self):
        if not self._open:
            raise RoflError(11, "unknown round handle")

    def ingest(self, updates, device_records=None):
        """Appends updates (instances of cls) to the round; more than max_clients in all raises RoflError 11 and ingests nothing.
        device_records[i] (optional): a contiguous uint8 GPU tensor holding update i's enc_values bytes, read on the device instead."""
        self._check_open()
        updates = list(updates)
        if len(self.updates) + len(updates) > self.max_clients:
            raise RoflError(11, "the round is full (nothing ingested)")
        ptrs, slots = [], []
        for j, u in enumerate(updates):
            if not isinstance(u, self.cls):
                raise ValueError("the updates of a round are of its container class")
            ev = u.enc_values
            fits = ev.ndim == 2 and ev.shape == (self.size, self.record_len) and ev.dtype == np.uint8 and ev.flags.c_contiguous
            dv = device_records[j] if device_records is not None else None
            if fits and dv is not None:
                p, nbytes = api._dev_arg(dv, 1)
                if nbytes != ev.size:
                    raise ValueError("device_records[i] holds the bytes of update i's enc_values")
                ptrs.append(p.value)
            elif fits:
                ptrs.append(ev.ctypes.data)
            slots.append(len(ptrs) - 1 if fits else None)
        first = api.device_round.ingest(self._h, ptrs) if ptrs else self._n_cached
        assert first == self._n_cached
        self.updates.extend(updates)
        self._slot.extend(None if sl is None else first + sl for sl in slots)
        self._n_cached += len(ptrs)
        return True

    # ---- the legs of cls.verify_batch over the round (the interface of _HostLegs) ----
    def _on_round(self, idx):
        """the majority members sit in the cache (their d is the round's): the legs can run there"""
        return all(self._slot[i] is not None for i in idx)

    def _ptrs(self, us, idx, arr):
        p = [None] * self._n_cached      # clients of the cache that are not among `us` are left out of the leg
        for u, i in zip(us, idx):
            p[self._slot[i]] = arr(u).ctypes.data
        return p

    def rand(self, cls, us, idx):
        comp = cls in (EncParamsRangeCompressed, EncParamsL2CompressedStrict)      # one CompressedRandProof per update
        if not self._on_round(idx) or (comp and not self._compressed):
            return _HostLegs.rand(cls, us, idx)
        if comp:
            ok = api.device_round.verify_compressed(self._h, self._ptrs(us, idx, lambda u: u.rand_proof))
            return [ok[self._slot[i]] for i in idx]
        ok, _ = api.device_round.verify_sigma(self._h, 0, self._ptrs(us, idx, lambda u: u.rand_proofs))
        return [ok[self._slot[i]] for i in idx]

    def square(self, cls, us, idx):
        if not self._on_round(idx):
            return _HostLegs.square(cls, us, idx)
        ok, sums = api.device_round.verify_sigma(self._h, 2 if issubclass(cls, EncParamsL2Compressed) else 1, self._ptrs(us, idx, lambda u: u.square_proofs), want_csq=True)
        sl = [self._slot[i] for i in idx]
        return [ok[s] for s in sl], sums[sl]

    def range(self, us, idx, k, prove_range, seed, fp, stride):
        if not self._on_round(idx):
            return _HostLegs.range(us, idx, k, prove_range, seed, fp, stride)
        n_proofs, proof_len = us[0].range_proofs.shape
        ok = api.device_round.verify_range(self._h, self._ptrs(us, idx, lambda u: u.range_proofs), proof_len, n_proofs, k, prove_range, verifier_seed=seed, fp=fp)
        return [ok[self._slot[i]] for i in idx]

    def verify(self, verifier_seed=None, fp=None):
        """list[bool], one per ingested update, in order: exactly cls.verify_batch(updates) -- the same majority-shape rule, the legs side by
        side on the round's device, the same error policy (a HIP error is raised, never a verdict)"""
        self._check_open()
        return self.cls.verify_batch(self.updates, verifier_seed=verifier_seed, fp=fp, _legs=self)

    def accumulate_into(self, acc, accept=None):
        """Adds the updates with accept[i] true (None: all) to the DeviceAccumulator `acc`: the cached ones from the decoded points
        (rofl_round_accumulate), the others through accumulate_batch.  acc.export() afterwards ==
        acc.accumulate_batch([u for u, a in zip(updates, accept) if a]), and like that call it is all or nothing: RoflError 5 when an accepted
        update has an undecodable L or R, `acc` unchanged.  For that the members outside the cache are summed into a partial accumulator of
        their own first (nothing of `acc` is touched if one of them fails), the cached ones are added next (refused before anything is
        launched if one of them has a bad point), and the partial -- valid points by then -- is merged last."""
        self._check_open()
        n = len(self.updates)
        accept = [True] * n if accept is None else [bool(a) for a in accept]
        if len(accept) != n:
            raise ValueError("one accept flag per ingested update")
        flags = [0] * self._n_cached
        others = []
        for u, sl, a in zip(self.updates, self._slot, accept):
            if a and sl is not None:
                flags[sl] = 1
            elif a:
                others.append(u)
        part = DeviceAccumulator(acc.size) if others else None
        try:
            if others:
                part.accumulate_batch(others)
            if self._n_cached:
                api.device_round.accumulate(self._h, acc._h, flags)
            if others:
                acc.accumulate_pairs(part.export())
        finally:
            if part is not None:
                part.close()
        return True

    def reset(self):
        """no updates; the device memory is kept for the next round"""
        self._check_open()
        api.device_round.reset(self._h)
        self.updates, self._slot, self._n_cached = [], [], 0

    def close(self):
        """frees the device memory (once); later calls on the round raise RoflError 11"""
        if getattr(self, "_open", False):
            self._open = False
            api.device_round.destroy(self._h)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
