//! `extern "C"` declarations for include/rofl_zk.h, plus the marshalling helpers shared by the overlay modules.
//! Scalars travel as 32-byte little-endian canonical strings, points as 32-byte compressed Ristretto, proofs in their
//! upstream `to_bytes` layouts; every output buffer is allocated by the caller.
use crate::fp::{Frac, N_BITS};
use curve25519_dalek_ng::ristretto::{CompressedRistretto, RistrettoPoint};
use curve25519_dalek_ng::scalar::Scalar;
use rand::RngCore;
use std::os::raw::{c_char, c_float, c_int, c_uint};
use fixed::frac::Unsigned;          // fixed re-exports typenum (fp.rs:3 takes U0..U12 from the same module)

#[repr(C)]
pub struct RoflNonce {
    pub mode: c_int,            // 0: explicit 64-byte wide scalars in the upstream draw order; 1: 32-byte seed
    pub stream: *const u8,
    pub stream_scalars: usize,
    pub seed: [u8; 32],
}

extern "C" {
    /// Binds the CALLING THREAD to `device` (like hipSetDevice) and makes it the default of threads that never call this.
    /// A server that drives N GPUs from its rayon pool either binds each pool thread once (`rayon::ThreadPoolBuilder::start_handler`)
    /// or calls `rofl_set_option(b"devices\0".., (1 << N) - 1)` and hands all clients of a round to the `_batch` entry points.
    pub fn rofl_set_device(device: c_int) -> c_int;
    pub fn rofl_get_device(device_out: *mut c_int) -> c_int;
    pub fn rofl_bind_device(device: c_int) -> c_int;
    pub fn rofl_last_error(buf: *mut c_char, len: usize) -> c_int;
    pub fn rofl_bp_gens_prepare(n_bits: usize, m: usize) -> c_int;
    pub fn rofl_bp_gens_prepare_verify(n_bits: usize, m: usize) -> c_int;
    pub fn rofl_bp_gens_table_bytes(n_bits: usize, m: usize, bytes_out: *mut usize) -> c_int;
    /// process-wide behaviour options ("verify_zip_truncate", "verify_batch" 0 / 1 / 2, "sigma_batch", "blocking_sync", "devices" = bit
    /// mask of the devices the `_batch` entry points spread their clients over); the ROFL_* environment variables only provide defaults.  A server that wants the reference's zip-truncating verify bit for bit calls
    /// `rofl_set_option(b"verify_zip_truncate\0".as_ptr() as *const c_char, 1)` once after `rofl_set_device`.
    pub fn rofl_set_option(key: *const c_char, value: std::os::raw::c_long) -> c_int;
    pub fn rofl_get_option(key: *const c_char, value_out: *mut std::os::raw::c_long) -> c_int;
    pub fn rofl_rangeproof_chunks(d: usize, n_partition: usize) -> usize;
    pub fn rofl_rangeproof_size(n_bits: usize, d: usize, n_partition: usize) -> usize;
    pub fn rofl_create_rangeproof(values: *const c_float, d: usize, blindings32: *const u8, d_blindings: usize,
        prove_range: usize, n_partition: usize, fp_bits: c_uint, fp_frac: c_uint, nonce: *const RoflNonce,
        proofs_out: *mut u8, proof_len_out: *mut usize, n_proofs_out: *mut usize, commits_out: *mut u8) -> c_int;
    pub fn rofl_create_rangeproof_chunks(values: *const c_float, d: usize, blindings32: *const u8, d_blindings: usize,
        prove_range: usize, n_partition: usize, fp_bits: c_uint, fp_frac: c_uint, nonce: *const RoflNonce,
        chunk_first: usize, chunk_count: usize, proofs_out: *mut u8, proof_len_out: *mut usize, commits_out: *mut u8,
        n_commits_out: *mut usize) -> c_int;
    pub fn rofl_verify_rangeproof_chunks(proofs: *const u8, proof_len: usize, n_proofs: usize, chunk_first: usize,
        chunk_count: usize, commits32: *const u8, d: usize, prove_range: usize, fp_bits: c_uint, fp_frac: c_uint,
        verifier_seed: *const u8, ok_out: *mut c_int) -> c_int;
    pub fn rofl_create_rangeproof_batch(n_clients: usize, values: *const *const c_float, d: usize, blindings32: *const *const u8,
        prove_range: usize, n_partition: usize, fp_bits: c_uint, fp_frac: c_uint, nonces: *const RoflNonce,
        proofs_out: *const *mut u8, proof_len_out: *mut usize, n_proofs_out: *mut usize, commits_out: *const *mut u8,
        rc_out: *mut c_int) -> c_int;
    pub fn rofl_verify_rangeproof(proofs: *const u8, proof_len: usize, n_proofs: usize, commits32: *const u8, d: usize,
        prove_range: usize, fp_bits: c_uint, fp_frac: c_uint, verifier_seed: *const u8, ok_out: *mut c_int) -> c_int;
    pub fn rofl_verify_rangeproof_batch(n_clients: usize, proofs: *const *const u8, proof_len: usize, n_proofs: usize,
        commits32: *const *const u8, d: usize, prove_range: usize, fp_bits: c_uint, fp_frac: c_uint,
        verifier_seed: *const u8, ok_out: *mut c_int) -> c_int;
    pub fn rofl_create_rangeproof_l2(values: *const c_float, d: usize, blindings32: *const u8, d_blindings: usize,
        prove_range: usize, n_partition: usize, fp_bits: c_uint, fp_frac: c_uint, nonce: *const RoflNonce,
        proof_out: *mut u8, proof_len_out: *mut usize, commit_out: *mut u8) -> c_int;
    pub fn rofl_verify_rangeproof_l2(proof: *const u8, proof_len: usize, commit: *const u8, prove_range: usize,
        fp_bits: c_uint, fp_frac: c_uint, verifier_seed: *const u8, ok_out: *mut c_int) -> c_int;
    pub fn rofl_create_sigmaproof_vec_range(kind: c_int, values: *const c_float, d: usize, r1_32: *const u8, r2_32: *const u8,
        existing32: *const u8, fp_bits: c_uint, fp_frac: c_uint, nonce: *const RoflNonce, elem_first: usize, elem_count: usize,
        proofs_out: *mut u8, commits_out: *mut u8) -> c_int;
    pub fn rofl_create_randproof_vec(values: *const c_float, d: usize, r32: *const u8, d_r: usize, existing32: *const u8,
        fp_bits: c_uint, fp_frac: c_uint, nonce: *const RoflNonce, proofs_out: *mut u8, pairs_out: *mut u8) -> c_int;
    pub fn rofl_verify_randproof_vec(proofs: *const u8, pairs: *const u8, d: usize, ok_out: *mut c_int) -> c_int;
    pub fn rofl_create_squarerandproof_vec(values: *const c_float, d: usize, r1_32: *const u8, d_r1: usize, r2_32: *const u8,
        existing32: *const u8, fp_bits: c_uint, fp_frac: c_uint, nonce: *const RoflNonce, proofs_out: *mut u8,
        commits_out: *mut u8) -> c_int;
    pub fn rofl_verify_squarerandproof_vec(proofs: *const u8, commits: *const u8, d: usize, ok_out: *mut c_int) -> c_int;
    pub fn rofl_commit_vec(values32: *const u8, blindings32: *const u8, d: usize, out32: *mut u8) -> c_int;
    pub fn rofl_add_points_vec(a32: *const u8, b32: *const u8, d: usize, out32: *mut u8) -> c_int;
    pub fn rofl_shift_points(a32: *const u8, d: usize, offset32: *const u8, out32: *mut u8) -> c_int;
    pub fn rofl_discrete_log_vec(points32: *const u8, d: usize, table_size: usize, bsgs_bits: c_uint, scalars_out32: *mut u8) -> c_int;
    /// server-side aggregation on the device (EncModelParamsAccumulator, params.rs:74-147): a handle from the library's registry;
    /// init 1 = ElGamalPair::unity() = (B, B), the reference's bytes
    pub fn rofl_acc_create(d: usize, init: c_int, handle_out: *mut u64) -> c_int;
    pub fn rofl_acc_add(h: u64, n_clients: usize, records: *const *const u8, d_each: *const usize, stride: usize) -> c_int;
    pub fn rofl_acc_export(h: u64, pairs_out: *mut u8) -> c_int;
    pub fn rofl_acc_extract(h: u64, table_size: usize, bsgs_bits: c_uint, fp_bits: c_uint, fp_frac: c_uint, out: *mut c_float,
        ok_out: *mut c_int) -> c_int;
    /// extraction after rejections: the opening s of the accepted set's residual blinding (d x 32 bytes, host or device; or the signed
    /// seeds it is the sum of) is checked against every R (ok_out = 0, first_bad_out = the smallest failing index) and stripped from L
    pub fn rofl_acc_extract_opened(h: u64, opening32: *const u8, table_size: usize, bsgs_bits: c_uint, fp_bits: c_uint, fp_frac: c_uint,
        out: *mut c_float, ok_out: *mut c_int, first_bad_out: *mut usize) -> c_int;
    pub fn rofl_acc_extract_opened_terms(h: u64, term_count: usize, terms: *const RoflBlindTerm, table_size: usize, bsgs_bits: c_uint,
        fp_bits: c_uint, fp_frac: c_uint, out: *mut c_float, ok_out: *mut c_int, first_bad_out: *mut usize) -> c_int;
    pub fn rofl_acc_reset(h: u64) -> c_int;
    pub fn rofl_acc_destroy(h: u64) -> c_int;
    /// a round resident on the device (server.rs:474-521, 656-714): records ingested once (one upload, one decode per point), both
    /// verification legs and the accumulation read the decoded points; handles as for rofl_acc_*
    pub fn rofl_round_create(d: usize, record_len: usize, max_clients: usize, handle_out: *mut u64) -> c_int;
    /// flags = ROFL_ROUND_COMPRESSED (1): the round keeps each client's CompressedRandProof transcript prefix for rofl_round_verify_compressed
    pub fn rofl_round_create_ex(d: usize, record_len: usize, max_clients: usize, flags: c_uint, handle_out: *mut u64) -> c_int;
    /// a round that keeps the CompressedRandProof transcript prefixes for records of either length (96: the strict check of EncL2Compressed)
    pub fn rofl_round_create_rand(d: usize, record_len: usize, max_clients: usize, handle_out: *mut u64) -> c_int;
    pub fn rofl_round_ingest(h: u64, n_clients: usize, records: *const *const u8, first_index_out: *mut usize) -> c_int;
    pub fn rofl_round_verify_sigma(h: u64, kind: c_int, proofs: *const *const u8, ok_out: *mut c_int, csq_sum_out32: *mut u8) -> c_int;
    pub fn rofl_round_verify_range(h: u64, proofs: *const *const u8, proof_len: usize, n_proofs: usize, k_checked: usize,
        prove_range: usize, fp_bits: c_uint, fp_frac: c_uint, verifier_seed: *const u8, ok_out: *mut c_int) -> c_int;
    pub fn rofl_round_verify_compressed(h: u64, proofs: *const *const u8, ok_out: *mut c_int) -> c_int;
    pub fn rofl_round_accumulate(h: u64, acc: u64, accept: *const c_int) -> c_int;
    pub fn rofl_round_reset(h: u64) -> c_int;
    pub fn rofl_round_destroy(h: u64) -> c_int;

    // ---- the rest of include/rofl_zk.h (scripts/check_ffi.py keeps this block and the header in step: names and arity)
    pub fn rofl_bp_gens_export(n_bits: usize, m: usize, g_out: *mut u8, h_out: *mut u8) -> c_int;
    pub fn rofl_next_pow2(v: usize) -> usize;
    pub fn rofl_nonces_per_chunk(n_bits: usize, m: usize) -> usize;
    /// commitments of client i read every `commit_stride` bytes from commits32[i] (64: ElGamal pairs, 96: SquareRandProofCommitments as they
    /// arrive on the wire) -- what params.rs:197, 215 do with `enc_values.iter().map(|x| x.c.L)`
    pub fn rofl_verify_rangeproof_batch_strided(n_clients: usize, proofs: *const *const u8, proof_len: usize, n_proofs: usize,
        commits32: *const *const u8, commit_stride: usize, d: usize, prove_range: usize, fp_bits: c_uint, fp_frac: c_uint,
        verifier_seed: *const u8, ok_out: *mut c_int) -> c_int;
    pub fn rofl_clip_f32(input: *const c_float, d: usize, prove_range: usize, fp_bits: c_uint, fp_frac: c_uint, out: *mut c_float) -> c_int;
    /// seeded stochastic rounding onto the fixed-point grid, n_vec vectors (own seed, input, output each) in one launch: out[v][k] = the
    /// clipped values[v][k] rounded up or down by word first + k of the rounding stream of seeds32[32 v ..]; values[v] / out[v] are host
    /// memory or device memory of the library's device, and may be the same array
    pub fn rofl_quantize_prob(n_vec: usize, seeds32: *const u8, values: *const *const c_float, first: usize, d: usize, prove_range: usize,
        fp_bits: c_uint, fp_frac: c_uint, out: *const *mut c_float) -> c_int;
    /// seeded centered-binomial noise on the fixed-point grid, n_vec vectors (own seed, input, output each) in one launch: out[v][i] = the
    /// clipped, rounded values[v][i] plus popcount(2k bits of the noise stream of seeds32[32 v ..] for element first + i) - k grid steps,
    /// clipped again; values[v] / out[v] are host memory or device memory of the library's device, and may be the same array
    pub fn rofl_noise_binomial(n_vec: usize, seeds32: *const u8, values: *const *const c_float, first: usize, d: usize, k: u32,
        prove_range: usize, fp_bits: c_uint, fp_frac: c_uint, out: *const *mut c_float) -> c_int;
    /// seeded discrete Gaussian noise on the fixed-point grid (the exact integer sampler of Canonne, Kamath and Steinke on a stream per
    /// element), n_vec vectors (own seed, input, output each) in one launch: out[v][i] = the clipped, rounded values[v][i] plus the noise
    /// of element first + i under seeds32[32 v ..] and sigma2 (an integer from 1 to 2^24) in grid steps, clipped again; values[v] / out[v]
    /// are host memory or device memory of the library's device, and may be the same array
    pub fn rofl_noise_dgauss(n_vec: usize, seeds32: *const u8, values: *const *const c_float, first: usize, d: usize, sigma2: u32,
        prove_range: usize, fp_bits: c_uint, fp_frac: c_uint, out: *const *mut c_float) -> c_int;
    /// projection onto the L2 ball on the fixed-point grid, n_vec vectors (own input, output, max_sq and optional seed each) in one call:
    /// out[v] = values[v] on the grid when its sum of squared steps is at most max_sq[v], else scaled by m / 2^32 so that the sum of
    /// squares of the result is; seeds32 null: truncation, else seeded rounding of the scaled steps; scale_out (n_vec u64) may be null
    pub fn rofl_clip_l2(n_vec: usize, seeds32: *const u8, values: *const *const c_float, d: usize, max_sq: *const u64, prove_range: usize,
        fp_bits: c_uint, fp_frac: c_uint, out: *const *mut c_float, scale_out: *mut u64) -> c_int;
    /// randomized Hadamard rotation, n_vec vectors (own PUBLIC seed, input, output each) in one call: per block of 2^block_log2 elements
    /// out = (1 / sqrt(B)) H D values (inverse = 1: D H), bit-defined; forward reads d floats and writes ceil(d / B) B, the inverse takes
    /// and returns whole blocks; values[v] / out[v] are host memory or device memory of the library's device
    pub fn rofl_rotate(n_vec: usize, seeds32: *const u8, values: *const *const c_float, d: usize, block_log2: c_uint, inverse: c_int,
        out: *const *mut c_float) -> c_int;
    pub fn rofl_verify_rangeproof_l2_batch(n_clients: usize, proofs: *const *const u8, proof_len: usize, commits32: *const u8,
        prove_range: usize, fp_bits: c_uint, fp_frac: c_uint, verifier_seed: *const u8, ok_out: *mut c_int) -> c_int;
    pub fn rofl_verify_randproof_vec_batch(n_clients: usize, proofs: *const *const u8, commits: *const *const u8, d: usize, ok_out: *mut c_int) -> c_int;
    pub fn rofl_verify_squarerandproof_vec_batch(n_clients: usize, proofs: *const *const u8, commits: *const *const u8, d: usize,
        ok_out: *mut c_int, csq_sum_out32: *mut u8) -> c_int;
    pub fn rofl_create_squareproof_vec(values: *const c_float, d: usize, r1_32: *const u8, d_r1: usize, r2_32: *const u8,
        existing32: *const u8, fp_bits: c_uint, fp_frac: c_uint, nonce: *const RoflNonce, proofs_out: *mut u8,
        commits_out: *mut u8) -> c_int;
    pub fn rofl_verify_squareproof_vec(proofs: *const u8, commits: *const u8, d: usize, ok_out: *mut c_int) -> c_int;
    pub fn rofl_verify_squareproof_vec_batch(n_clients: usize, proofs: *const *const u8, commits: *const *const u8, d: usize,
        ok_out: *mut c_int, csq_sum_out32: *mut u8) -> c_int;
    pub fn rofl_create_compressed_randproof(values: *const c_float, d: usize, r32: *const u8, d_r: usize, existing32: *const u8,
        fp_bits: c_uint, fp_frac: c_uint, nonce: *const RoflNonce, proof_out: *mut u8, pairs_out: *mut u8) -> c_int;
    pub fn rofl_verify_compressed_randproof(proof: *const u8, pairs: *const u8, d: usize, ok_out: *mut c_int) -> c_int;
    /// the compressed randomness proofs of a round's clients (d pairs each) in one launch sequence; ok_out[i] = client i's verdict,
    /// exactly the single call's (a malformed member is 0, the others are still verified)
    pub fn rofl_verify_compressed_randproof_batch(n_clients: usize, proofs: *const *const u8, pairs: *const *const u8, d: usize,
        ok_out: *mut c_int) -> c_int;
    /// the same over records read in place every `stride` bytes (64, or 96: SquareRandProofCommitments, the pair is the first 64 bytes)
    pub fn rofl_verify_compressed_randproof_batch_strided(n_clients: usize, proofs: *const *const u8, records: *const *const u8,
        stride: usize, d: usize, ok_out: *mut c_int) -> c_int;
    /// the compressed randomness proofs of the clients of one process in one launch sequence; proofs_out[i] / pairs_out[i] are the single
    /// call's bytes for client i, rc_out[i] its own outcome (0, 10, 5, 12: it is left out, the others are still proved); existing32 or any
    /// of its entries may be null
    pub fn rofl_create_compressed_randproof_batch(n_clients: usize, values: *const *const c_float, d: usize, r32: *const *const u8,
        existing32: *const *const u8, fp_bits: c_uint, fp_frac: c_uint, nonces: *const RoflNonce, proofs_out: *const *mut u8,
        pairs_out: *const *mut u8, rc_out: *mut c_int) -> c_int;
    /// the per-element Sigma-proof vectors (kind 0 RandProof, 1 SquareRandProof, 2 SquareProof) of the clients of one process in one launch
    /// sequence; proofs_out[i] / commits_out[i] are the single call's bytes for client i, rc_out[i] its own outcome (0, 10, 5, 12: it is
    /// left out, the others are still proved); r2_32 is null for kind 0, existing32 or any of its entries may be null
    pub fn rofl_create_sigmaproof_vec_batch(kind: c_int, n_clients: usize, values: *const *const c_float, d: usize, r1_32: *const *const u8,
        r2_32: *const *const u8, existing32: *const *const u8, fp_bits: c_uint, fp_frac: c_uint, nonces: *const RoflNonce,
        proofs_out: *const *mut u8, commits_out: *const *mut u8, rc_out: *mut c_int) -> c_int;
    /// the L2 sum proofs of the clients of one process in one launch sequence; proofs_out[i] / commits_out32 + 32 i are the single call's
    /// bytes for client i, rc_out[i] the code the single call returns for it (it is left out, the others are still proved)
    pub fn rofl_create_rangeproof_l2_batch(n_clients: usize, values: *const *const c_float, d: usize, blindings32: *const *const u8,
        prove_range: usize, n_partition: usize, fp_bits: c_uint, fp_frac: c_uint, nonces: *const RoflNonce, proofs_out: *const *mut u8,
        proof_len_out: *mut usize, commits_out32: *mut u8, rc_out: *mut c_int) -> c_int;
    pub fn rofl_sum_points(points: *const u8, d: usize, stride: usize, out32: *mut u8) -> c_int;
    pub fn rofl_f32_to_scalar_vec(input: *const c_float, d: usize, fp_bits: c_uint, fp_frac: c_uint, out32: *mut u8) -> c_int;
    pub fn rofl_scalar_to_f32_vec(in32: *const u8, d: usize, fp_bits: c_uint, fp_frac: c_uint, out: *mut c_float) -> c_int;
    pub fn rofl_get_clip_bounds(range: usize, fp_bits: c_uint, fp_frac: c_uint, min_out: *mut c_float, max_out: *mut c_float) -> c_int;
    pub fn rofl_fp_square_vec(in32: *const u8, d: usize, fp_bits: c_uint, fp_frac: c_uint, out32: *mut u8) -> c_int;
    pub fn rofl_scalar_powers(value32: *const u8, count: usize, out32: *mut u8) -> c_int;
    pub fn rofl_scalar_add_vec(a32: *const u8, b32: *const u8, d: usize, subtract: c_int, out32: *mut u8) -> c_int;
    /// out32[v][k] = sum_t terms[v][t].sign * stream(terms[v][t].seed)[first + k] mod l for k in [0, d): n_vec blinding vectors in one launch
    /// (out32[v]: d * 32 bytes of host memory, or 16-byte aligned device memory of the library's device)
    pub fn rofl_blinding_vecs(n_vec: usize, term_count: *const usize, terms: *const *const RoflBlindTerm, first: usize, d: usize,
        out32: *const *mut u8) -> c_int;
    pub fn rofl_rnd_scalar_vec(seed: *const u8, first: usize, d: usize, out32: *mut u8) -> c_int;
    /// Ristretto255 key agreement for the pairwise masks: pk = encode(sk * B) for n secret keys (32 bytes each, reduced mod l; 0 is refused)
    pub fn rofl_dh_public_keys(n: usize, sk32: *const u8, pk_out32: *mut u8) -> c_int;
    /// shared secrets of (own, peer) pairs, one launch chain: pairs null = all n_own x n_peer pairs, own-major; status 1 / 2 per pair = the
    /// peer key is not canonical / is the identity (32 zero bytes out); own_pk_out32 may be null
    pub fn rofl_dh_shared(n_own: usize, sk32: *const u8, own_pk_out32: *mut u8, n_peer: usize, peer_pk32: *const u8,
        n_pairs: usize, pairs: *const RoflDhPair, out32: *mut u8, status_out: *mut u8) -> c_int;
    /// Shamir shares of n_secrets scalars (32 bytes each, reduced mod l) at threshold `threshold`: shares_out32[s][i] = f_s(xs[i]), secret-major;
    /// the coefficients of f_s come from coef_seeds32[s]; xs null = the points 1 .. n_shares, otherwise nonzero and distinct
    pub fn rofl_shamir_share(n_secrets: usize, secrets32: *const u8, coef_seeds32: *const u8, threshold: usize, n_shares: usize, xs: *const u32,
        shares_out32: *mut u8) -> c_int;
    /// the secrets from n_shares shares each at the points xs (one set for all secrets): Lagrange interpolation at 0 over ALL shares handed in
    pub fn rofl_shamir_reconstruct(n_secrets: usize, n_shares: usize, xs: *const u32, shares32: *const u8, secrets_out32: *mut u8) -> c_int;
    /// include/rofl_zk_debug.h: the two calls above on the host's arithmetic, one thread, no GPU -- same parameters, same bytes
    pub fn rofl_dbg_host_shamir_share(n_secrets: usize, secrets32: *const u8, coef_seeds32: *const u8, threshold: usize, n_shares: usize,
        xs: *const u32, shares_out32: *mut u8) -> c_int;
    pub fn rofl_dbg_host_shamir_reconstruct(n_secrets: usize, n_shares: usize, xs: *const u32, shares32: *const u8, secrets_out32: *mut u8) -> c_int;
    /// Feldman commitments of the sharing polynomials of rofl_shamir_share: commitments_out32[s][k] = encode(a_k B), a_0 = the secret mod l,
    /// secret-major, `threshold` per secret; C_0 of a DH key is its public key
    pub fn rofl_feldman_commit(n_secrets: usize, secrets32: *const u8, coef_seeds32: *const u8, threshold: usize, commitments_out32: *mut u8) -> c_int;
    /// verdict_out[s][i] for shares32[s][i] at xs[i] (null = 1 .. n_shares) against the commitments of secret s: 0 consistent, 1 not, 2 = a
    /// commitment of that secret is not a canonical encoding (the whole row)
    pub fn rofl_feldman_verify(n_secrets: usize, threshold: usize, commitments32: *const u8, n_shares: usize, xs: *const u32, shares32: *const u8,
        verdict_out: *mut u8) -> c_int;
    /// include/rofl_zk_debug.h: the two calls above on the host's arithmetic, one thread, no GPU -- same parameters, same bytes
    pub fn rofl_dbg_host_feldman_commit(n_secrets: usize, secrets32: *const u8, coef_seeds32: *const u8, threshold: usize,
        commitments_out32: *mut u8) -> c_int;
    pub fn rofl_dbg_host_feldman_verify(n_secrets: usize, threshold: usize, commitments32: *const u8, n_shares: usize, xs: *const u32,
        shares32: *const u8, verdict_out: *mut u8) -> c_int;
    /// Deterministic Schnorr signatures over Ristretto255 (the authenticated broadcast of keys and commitments): signature i = key refs[i].key
    /// on message refs[i].msg, message j = msg_bytes[msg_off[j] .. msg_off[j + 1]); refs null = (i, i); sig_out64 n x 64; pk_out32 may be null
    pub fn rofl_sig_sign(n_keys: usize, sk32: *const u8, pk_out32: *mut u8, n_msgs: usize, msg_bytes: *const u8, msg_off: *const u64,
        n: usize, refs: *const RoflSigRef, sig_out64: *mut u8) -> c_int;
    /// verdict_out[i]: 0 valid, 1 not, 2 = the key is not a canonical encoding or is the identity, or s >= l
    pub fn rofl_sig_verify(n_keys: usize, pk32: *const u8, n_msgs: usize, msg_bytes: *const u8, msg_off: *const u64,
        n: usize, refs: *const RoflSigRef, sig64: *const u8, verdict_out: *mut u8) -> c_int;
    /// RFC 8439 ChaCha20-Poly1305 on the share bundles a server relays: record i under key key_idx[i] (null = key i), nonce12 n x 12, AD and
    /// payload packed with n + 1 offsets; sealed_out holds CT || tag of record i at pt_off[i] + 16 i.  derive_round non-null: a row of key32 is
    /// a rofl_dh_shared output and the key is SHAKE256("rofl-zk/seal/v1\0" || row || u64le(round))[0 .. 32)
    pub fn rofl_aead_seal(n_keys: usize, key32: *const u8, derive_round: *const u64, n: usize, key_idx: *const u32, nonce12: *const u8,
        ad_bytes: *const u8, ad_off: *const u64, pt_bytes: *const u8, pt_off: *const u64, sealed_out: *mut u8) -> c_int;
    /// verdict_out[i]: 0 opened (plaintext at pt_out[sealed_off[i] ..)), 1 the tag does not match (zeros there), 2 shorter than 16 bytes
    pub fn rofl_aead_open(n_keys: usize, key32: *const u8, derive_round: *const u64, n: usize, key_idx: *const u32, nonce12: *const u8,
        ad_bytes: *const u8, ad_off: *const u64, sealed_bytes: *const u8, sealed_off: *const u64, pt_out: *mut u8, verdict_out: *mut u8) -> c_int;
    /// A complaint against a dealer: pair i = (own key pairs[i].own, peer key pairs[i].peer), null = all pairs own-major; reveal i is the pair's
    /// raw DH point, proof i the 64-byte DLEQ proof that it was made with the own key, bound to ctx32[i]; a refused peer key gives status 1 / 2
    /// and zeros; own_pk_out32 may be null
    pub fn rofl_dleq_prove(n_own: usize, sk32: *const u8, own_pk_out32: *mut u8, n_peer: usize, peer_pk32: *const u8,
        n_pairs: usize, pairs: *const RoflDhPair, ctx32: *const u8, reveal_out32: *mut u8, proof_out64: *mut u8, status_out: *mut u8) -> c_int;
    /// verdict_out[i]: 0 the proof holds (shared_out32[i], may be null, is then the pair's rofl_dh_shared secret), 1 it does not, 2 a key or
    /// the reveal is not a canonical encoding or is the identity, or c or s >= l
    pub fn rofl_dleq_verify(n_own: usize, own_pk32: *const u8, n_peer: usize, peer_pk32: *const u8,
        n_pairs: usize, pairs: *const RoflDhPair, ctx32: *const u8, reveal32: *const u8, proof64: *const u8,
        shared_out32: *mut u8, verdict_out: *mut u8) -> c_int;
    /// a Merkle tree over n messages (msg_off null: msg_bytes is n x 32 leaf digests): the root, the leaf digests (leaves_out32 may be null)
    /// and the paths of the leaves path_idx names, n_paths x depth(n) x 32 bytes, depth(n) = bit_length(n - 1)
    pub fn rofl_merkle_build(n: usize, msg_bytes: *const u8, msg_off: *const u64, root_out32: *mut u8, leaves_out32: *mut u8,
        n_paths: usize, path_idx: *const u32, paths_out32: *mut u8) -> c_int;
    /// verdict_out[i]: 0 the path of leaf refs[i].index climbs to root refs[i].root (refs null: root 0, index i), 1 it does not, 2 the index is
    /// not below the root's leaf count or a slot the shape leaves empty (up to `stride`) has a nonzero byte
    pub fn rofl_merkle_verify(n_roots: usize, root32: *const u8, n_leaves: *const u32, n_paths: usize, refs: *const RoflMerkleRef,
        msg_bytes: *const u8, msg_off: *const u64, paths32: *const u8, stride: usize, verdict_out: *mut u8) -> c_int;
    pub fn rofl_f32_to_fp_vec(input: *const c_float, d: usize, fp_bits: c_uint, fp_frac: c_uint, out: *mut u64) -> c_int;
    pub fn rofl_uint_to_f32_vec(input: *const u64, d: usize, fp_bits: c_uint, fp_frac: c_uint, out: *mut c_float) -> c_int;
    pub fn rofl_get_l2_clip_bounds(range: usize, fp_bits: c_uint, fp_frac: c_uint, out: *mut c_float) -> c_int;
    pub fn rofl_wire_encoded_size(m: *const RoflWireMsg) -> usize;
    pub fn rofl_wire_encode(m: *const RoflWireMsg, out: *mut u8, cap: usize, len_out: *mut usize) -> c_int;
    pub fn rofl_wire_decode(kind: c_int, data: *const u8, len: usize, m: *mut RoflWireMsg, range_proofs_out: *mut u8, range_proofs_cap: usize) -> c_int;
    // one process per GPU: the exchange of a round over the library's own RCCL communicator
    pub fn rofl_comm_unique_id(id_out: *mut u8) -> c_int;
    pub fn rofl_comm_init(id: *const u8, rank: c_int, world: c_int) -> c_int;
    pub fn rofl_comm_allgather(local: *const u8, n: usize, all_out: *mut u8) -> c_int;
    pub fn rofl_comm_allreduce_f64(inout: *mut f64, count: usize, op: c_int) -> c_int;
    pub fn rofl_comm_barrier() -> c_int;
    pub fn rofl_comm_info(rank_out: *mut c_int, world_out: *mut c_int, rccl_version_out: *mut c_int, lib_path_out: *mut c_char, len: usize) -> c_int;
    pub fn rofl_comm_destroy() -> c_int;
}

/// rofl_wire_msg_t (include/rofl_zk.h): the proto3 messages of flservice.proto:75-100 as spans over `to_bytes` concatenations
/// rofl_blind_term_t: one term of a blinding vector -- the 32-byte seed of a stream and its sign (+1 or -1)
#[repr(C)]
pub struct RoflBlindTerm {
    pub seed: [u8; 32],
    pub sign: i32,
}
/// rofl_dh_pair_t: one pair of rofl_dh_shared -- indices into its own secret keys and its peer public keys
#[repr(C)]
pub struct RoflDhPair {
    pub own: u32,
    pub peer: u32,
}

/// rofl_sig_ref_t: one signature of rofl_sig_sign / rofl_sig_verify -- indices into the call's keys and its messages
#[repr(C)]
#[derive(Clone, Copy)]
pub struct RoflSigRef {
    pub key: u32,
    pub msg: u32,
}

/// rofl_merkle_ref_t: one path of rofl_merkle_verify -- the root it is checked under and the index of its leaf
#[repr(C)]
#[derive(Clone, Copy)]
pub struct RoflMerkleRef {
    pub root: u32,
    pub index: u32,
}

#[repr(C)]
pub struct RoflWireMsg {
    pub kind: c_int,                       // 0 EncRangeData, 1 EncNormData, 2 EncNormDataCompressed
    pub enc_values: *const u8, pub enc_values_len: usize,
    pub rand_proof: *const u8, pub rand_proof_len: usize,
    pub square_proof: *const u8, pub square_proof_len: usize,
    pub range_proofs: *const u8, pub range_proof_len: usize, pub n_range_proofs: usize,
    pub square_range_proof: *const u8, pub square_range_proof_len: usize,
    pub range_bits: i32, pub l2_range_bits: i32,
    pub check_percentage: c_float,
}

// return codes of include/rofl_zk.h
pub const ROFL_OK: c_int = 0;
pub const ROFL_WRONG_NUM_BLINDING_FACTORS: c_int = 1;
pub const ROFL_VALUE_OUT_OF_RANGE: c_int = 2;
pub const ROFL_INVALID_BITSIZE: c_int = 3;
pub const ROFL_INVALID_AGGREGATION: c_int = 4;
pub const ROFL_FORMAT_ERROR: c_int = 5;
pub const ROFL_INVALID_GENERATORS_LENGTH: c_int = 6;
pub const ROFL_NORM_OUT_OF_RANGE: c_int = 7;
pub const ROFL_OVERFLOW: c_int = 8;
pub const ROFL_SUM_ERROR: c_int = 9;
pub const ROFL_NON_FINITE: c_int = 10;
pub const ROFL_BAD_PARAM: c_int = 11;
pub const ROFL_NONCE_SHORT: c_int = 12;
pub const ROFL_COMM_ERROR: c_int = 99;
pub const ROFL_HIP_ERROR: c_int = 100;

/// The ONE verdict on which the library's default differs from the reference: a proof set that covers fewer chunks than the padded
/// commitment vector (range_proof_vec/mod.rs:169-176 zips and silently drops the tail -> `Ok(true)`; the library's default says
/// `Ok(false)`).  Built with `--features reference_semantics` the overlay asks for the reference's behaviour bit for bit, once per
/// process, before its first verification; without the feature the hardened default stays.
pub fn ensure_options() {
    static ONCE: std::sync::Once = std::sync::Once::new();
    ONCE.call_once(|| {
        if cfg!(feature = "reference_semantics") {
            let rc = unsafe { rofl_set_option(b"verify_zip_truncate\0".as_ptr() as *const c_char, 1) };
            assert_eq!(rc, ROFL_OK, "rofl_set_option(verify_zip_truncate): {}", last_error());
        }
    });
}

pub fn fp_bits() -> c_uint { N_BITS as c_uint }
pub fn fp_frac() -> c_uint { <Frac as Unsigned>::U32 }

/// What `thread_rng()` was to the upstream prover: fresh randomness per call, expanded on the device.
pub fn fresh_nonce() -> RoflNonce {
    let mut seed = [0u8; 32];
    rand::thread_rng().fill_bytes(&mut seed);
    RoflNonce { mode: 1, stream: std::ptr::null(), stream_scalars: 0, seed }
}
pub fn fresh_seed() -> [u8; 32] {
    let mut seed = [0u8; 32];
    rand::thread_rng().fill_bytes(&mut seed);
    seed
}
pub fn scalars_to_bytes(v: &[Scalar]) -> Vec<u8> { v.iter().flat_map(|s| s.to_bytes().to_vec()).collect() }
pub fn points_to_bytes(v: &[RistrettoPoint]) -> Vec<u8> { v.iter().flat_map(|p| p.compress().to_bytes().to_vec()).collect() }
pub fn bytes_to_points(b: &[u8]) -> Vec<RistrettoPoint> {
    b.chunks(32).map(|c| CompressedRistretto::from_slice(c).decompress().expect("librofl_zk returns valid encodings")).collect()
}
pub fn bytes_to_scalars(b: &[u8]) -> Vec<Scalar> {
    b.chunks(32).map(|c| { let mut a = [0u8; 32]; a.copy_from_slice(c); Scalar::from_canonical_bytes(a).expect("canonical") }).collect()
}
/// rofl_create_sigmaproof_vec_batch over typed inputs: the bytes (proofs, commitments) of every client, for the `*_batch` wrappers of
/// rand_proof_vec, square_rand_proof_vec and square_proof_vec.  All vectors have the length of values[0]; r2 is None for kind 0.  A
/// client whose inputs the library refuses (a non-finite value, an undecodable commitment) panics as in the single calls.
pub fn sigma_create_batch_bytes(kind: c_int, proof_len: usize, commit_len: usize, values: &[&Vec<f32>], existing: &[Option<&Vec<RistrettoPoint>>],
                                r1: &[&Vec<Scalar>], r2: Option<&[&Vec<Scalar>]>) -> Vec<(Vec<u8>, Vec<u8>)> {
    let n = values.len();
    if n == 0 { return Vec::new(); }
    let d = values[0].len();
    let a: Vec<Vec<u8>> = r1.iter().map(|v| scalars_to_bytes(v)).collect();
    let b: Option<Vec<Vec<u8>>> = r2.map(|r| r.iter().map(|v| scalars_to_bytes(v)).collect());
    let ex: Vec<Option<Vec<u8>>> = existing.iter().map(|c| c.map(|v| points_to_bytes(v))).collect();
    let mut proofs: Vec<Vec<u8>> = (0..n).map(|_| vec![0u8; d * proof_len]).collect();
    let mut commits: Vec<Vec<u8>> = (0..n).map(|_| vec![0u8; d * commit_len]).collect();
    let nonces: Vec<RoflNonce> = (0..n).map(|_| fresh_nonce()).collect();
    let vp: Vec<*const f32> = values.iter().map(|v| v.as_ptr()).collect();
    let ap: Vec<*const u8> = a.iter().map(|v| v.as_ptr()).collect();
    let bp: Option<Vec<*const u8>> = b.as_ref().map(|b| b.iter().map(|v| v.as_ptr()).collect());
    let ep: Vec<*const u8> = ex.iter().map(|e| e.as_ref().map_or(std::ptr::null(), |v| v.as_ptr())).collect();
    let pp: Vec<*mut u8> = proofs.iter_mut().map(|v| v.as_mut_ptr()).collect();
    let cp: Vec<*mut u8> = commits.iter_mut().map(|v| v.as_mut_ptr()).collect();
    let mut rcs: Vec<c_int> = vec![0; n];
    let rc = unsafe {
        rofl_create_sigmaproof_vec_batch(kind, n, vp.as_ptr(), d, ap.as_ptr(), bp.as_ref().map_or(std::ptr::null(), |v| v.as_ptr()), ep.as_ptr(),
                                         fp_bits(), fp_frac(), nonces.as_ptr(), pp.as_ptr(), cp.as_ptr(), rcs.as_mut_ptr())
    };
    if rc != ROFL_OK { panic!("rofl_zk: {}", last_error()); }
    for i in 0..n { if rcs[i] != ROFL_OK { panic!("rofl_zk: client {} of the batch: error {}", i, rcs[i]); } }
    proofs.into_iter().zip(commits.into_iter()).collect()
}
pub fn last_error() -> String {
    let mut buf = vec![0 as c_char; 512];
    unsafe { rofl_last_error(buf.as_mut_ptr(), buf.len()); std::ffi::CStr::from_ptr(buf.as_ptr()).to_string_lossy().into_owned() }
}

/// Batched signatures over the library (rofl_sig_sign / rofl_sig_verify).  A signing key is NOT the key-agreement key: that one is revealed
/// when its owner drops out.  Not constant-time; deterministic nonces.
pub mod signatures {
    use super::{last_error, rofl_sig_sign, rofl_sig_verify, RoflSigRef, ROFL_OK};

    fn pack(messages: &[&[u8]]) -> (Vec<u8>, Vec<u64>) {
        let mut bytes = Vec::with_capacity(messages.iter().map(|m| m.len()).sum());
        let mut off = Vec::with_capacity(messages.len() + 1);
        off.push(0u64);
        for m in messages { bytes.extend_from_slice(m); off.push(bytes.len() as u64); }
        (bytes, off)
    }
    /// signature i = key refs[i].key on message refs[i].msg; refs None = key i on message i.  Panics on a refused parameter (a zero key).
    pub fn sign(sks: &[[u8; 32]], messages: &[&[u8]], refs: Option<&[RoflSigRef]>) -> Vec<[u8; 64]> {
        let n = refs.map_or(sks.len(), |r| r.len());
        let (bytes, off) = pack(messages);
        let mut out = vec![[0u8; 64]; n];
        let rc = unsafe { rofl_sig_sign(sks.len(), sks.as_ptr() as *const u8, std::ptr::null_mut(), messages.len(), bytes.as_ptr(), off.as_ptr(),
                                        n, refs.map_or(std::ptr::null(), |r| r.as_ptr()), out.as_mut_ptr() as *mut u8) };
        if rc != ROFL_OK { panic!("rofl_zk: {}", last_error()); }
        out
    }
    /// one verdict per signature: 0 valid, 1 not, 2 = a refused key or s >= l
    pub fn verify(pks: &[[u8; 32]], messages: &[&[u8]], sigs: &[[u8; 64]], refs: Option<&[RoflSigRef]>) -> Vec<u8> {
        let n = sigs.len();
        assert_eq!(n, refs.map_or(pks.len(), |r| r.len()), "one signature per ref");
        let (bytes, off) = pack(messages);
        let mut out = vec![0u8; n];
        let rc = unsafe { rofl_sig_verify(pks.len(), pks.as_ptr() as *const u8, messages.len(), bytes.as_ptr(), off.as_ptr(),
                                          n, refs.map_or(std::ptr::null(), |r| r.as_ptr()), sigs.as_ptr() as *const u8, out.as_mut_ptr()) };
        if rc != ROFL_OK { panic!("rofl_zk: {}", last_error()); }
        out
    }
}

/// Batched RFC 8439 ChaCha20-Poly1305 over the library (rofl_aead_seal / rofl_aead_open): the share bundles a server relays.  The keys come
/// from a CHANNEL key pair of its own (never the mask key, which is reconstructed when its owner drops out) through rofl_dh_shared and
/// derive_round.  Not constant-time; the caller owns nonce uniqueness.
pub mod sealed {
    use super::{last_error, rofl_aead_open, rofl_aead_seal, ROFL_OK};

    fn pack(items: &[&[u8]]) -> (Vec<u8>, Vec<u64>) {
        let mut bytes = Vec::with_capacity(items.iter().map(|m| m.len()).sum());
        let mut off = Vec::with_capacity(items.len() + 1);
        off.push(0u64);
        for m in items { bytes.extend_from_slice(m); off.push(bytes.len() as u64); }
        (bytes, off)
    }
    /// record i = payload i under key i, nonce i and AD i -> CT || tag.  Panics on a refused parameter.
    pub fn seal(keys: &[[u8; 32]], derive_round: Option<u64>, nonces: &[[u8; 12]], ads: &[&[u8]], payloads: &[&[u8]]) -> Vec<Vec<u8>> {
        let n = payloads.len();
        assert!(keys.len() == n && nonces.len() == n && ads.len() == n, "one key, nonce and AD per payload");
        let ((ad, ad_off), (pt, pt_off)) = (pack(ads), pack(payloads));
        let mut out = vec![0u8; pt.len() + 16 * n];
        let rc = unsafe { rofl_aead_seal(n, keys.as_ptr() as *const u8, derive_round.as_ref().map_or(std::ptr::null(), |r| r as *const u64), n, std::ptr::null(),
                                         nonces.as_ptr() as *const u8, ad.as_ptr(), ad_off.as_ptr(), pt.as_ptr(), pt_off.as_ptr(), out.as_mut_ptr()) };
        if rc != ROFL_OK { panic!("rofl_zk: {}", last_error()); }
        (0..n).map(|i| out[pt_off[i] as usize + 16 * i..pt_off[i + 1] as usize + 16 * (i + 1)].to_vec()).collect()
    }
    /// (plaintexts, verdicts): verdict 0 opened, 1 the tag does not match (a zero plaintext), 2 shorter than 16 bytes (an empty plaintext)
    pub fn open(keys: &[[u8; 32]], derive_round: Option<u64>, nonces: &[[u8; 12]], ads: &[&[u8]], records: &[&[u8]]) -> (Vec<Vec<u8>>, Vec<u8>) {
        let n = records.len();
        assert!(keys.len() == n && nonces.len() == n && ads.len() == n, "one key, nonce and AD per record");
        let ((ad, ad_off), (ct, ct_off)) = (pack(ads), pack(records));
        let (mut pt, mut verdict) = (vec![0u8; ct.len().max(1)], vec![0u8; n]);
        let rc = unsafe { rofl_aead_open(n, keys.as_ptr() as *const u8, derive_round.as_ref().map_or(std::ptr::null(), |r| r as *const u64), n, std::ptr::null(),
                                         nonces.as_ptr() as *const u8, ad.as_ptr(), ad_off.as_ptr(), ct.as_ptr(), ct_off.as_ptr(), pt.as_mut_ptr(), verdict.as_mut_ptr()) };
        if rc != ROFL_OK { panic!("rofl_zk: {}", last_error()); }
        let out = (0..n).map(|i| { let (a, b) = (ct_off[i] as usize, ct_off[i + 1] as usize); pt[a..a + (b - a).saturating_sub(16)].to_vec() }).collect();
        (out, verdict)
    }
}
