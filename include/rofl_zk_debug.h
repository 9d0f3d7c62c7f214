/*
 * Test, self-check and measurement hooks of librofl_zk.so.  NOT part of the operator API (include/rofl_zk.h): nothing a
 * rofl_crypto / rofl_service binding needs lives here.  tests/ and bench.py use them; a deployment can ignore this header.
 */
#ifndef ROFL_ZK_DEBUG_H
#define ROFL_ZK_DEBUG_H
#include "rofl_zk.h"
#ifdef __cplusplus
extern "C" {
#endif

/* ---- measurement hooks (bench.py) ---- */
/* Time of the kernels of the last create / verify call, from HIP events on the library's stream. */
typedef struct {
    double total_ms;          /* first launch -> last completion, device clock */
    double msm_accumulate_ms; /* sum over launches of k_msm_accumulate */
    uint64_t msm_accumulate_launches;
    uint64_t msm_terms;       /* non-trivial (scalar, point) terms fed to Pippenger */
    double fold_ms;           /* sum over launches of k_fold_gens */
    uint64_t fold_launches;
    uint64_t fold_point_reads;   /* niels points read by k_fold_gens (96 B each) */
    double host_ms;           /* host-side (transcript, Horner, fixed-base) time */
    uint64_t msm_additions;   /* mixed point additions executed by k_msm_accumulate: terms x windows (7 field multiplications each) */
} rofl_timing_t;
int rofl_last_timing(rofl_timing_t *out);
/* Per-kernel table of the last instrumented call of the calling thread: HIP-event time, launches and the ALGORITHMIC work of
 * those launches -- field multiplications (7 per mixed point addition, 8 per doubling, 9 per extended addition) and the bytes
 * a launch has to move at least once (32 B per scalar or point, 4 B per bucket-list entry). */
enum { ROFL_TK_MSM_ACCUMULATE_FB = 0, ROFL_TK_MSM_ACCUMULATE_GEN = 1, ROFL_TK_MSM_SCATTER = 2, ROFL_TK_MSM_REDUCE = 3,
       ROFL_TK_MSM_SMALL = 4, ROFL_TK_FOLD_TAB = 5, ROFL_TK_FOLD = 6, ROFL_TK_OTHER = 7,
       ROFL_TK_SIGMA = 8,            /* k_sigma_prove / k_sigma_vprep / k_sigma_verify: the per-element Sigma-proofs (the L2 composite of cfg 3 / 5) */
       ROFL_TK_VERIFY_SCALARS = 9,   /* k_verify_scalars: the verifier's 2N generator scalars, summed over the proofs of a group (scalar field: no fe_muls) */
       ROFL_TK_CODEC = 10,           /* k_decode / k_commit: Ristretto decoding / commitment + encoding of d points */
       ROFL_TK_COUNT = 11 };
typedef struct { double ms; uint64_t launches, fe_muls, bytes; } rofl_kernel_time_t;
int rofl_last_kernel_times(rofl_kernel_time_t out[ROFL_TK_COUNT]);
/* 0 = off; 1 = HIP events around every instrumented launch (~150 event records per proof: ~0.7 ms of a 25 ms proof); 2 = only around the
 * fixed-base accumulation, the kernel bench.py prices against the roofline (ten records per proof) */
int rofl_set_timing(int enabled);
/* ---- devices on a one-GPU test box ----
 * rofl_dbg_map_device: logical device `logical` (what rofl_set_device and the "devices" option name) is HIP device `physical`; allowed
 * until the logical device is first used (ROFL_DEVICE_MAP="0,0,..." does the same from the environment).  Two logical devices on GPU 0
 * are two full device contexts -- own streams, workspaces and generator tables -- which is how the multi-device paths are tested here.
 * rofl_dbg_bind_device: the thread-binding half of rofl_set_device without touching HIP (-1 = unbind). */
int rofl_dbg_map_device(int logical, int physical);
int rofl_dbg_bind_device(int device);

/* GPU multi-scalar multiplication sum_i k_i * P_i through the production Pippenger pipeline (dalek
 * vartime_multiscalar_mul as used by upstream verify_multiple); test hook for skewed / extreme scalars. */
int rofl_dbg_msm(const uint8_t *scalars32, const uint8_t *points32, size_t n, uint8_t out32[32]);
/* The same driver with the shape and the scalars chosen by the caller, for the tests that push its fixed-size structures (bucket lists,
 * slots, the overflow list, coarse bins) to their capacity and over it.  Both run ONE msm_run; scalars are reduced mod l as rofl_dbg_msm
 * does.  The L/R-merged mode of the inner-product rounds (MsmOpt::lr_nh != 0) needs scalar arrays in which every term belongs to one side
 * by construction (k_lr_first, k_ipp_round) and is NOT reachable through these entries: tests/test_gpu_nonce_collide.py drives it to the
 * same capacities through the prover itself, with nonce streams (Nonce.stream) that make the rounds' scalars collide, and reads every
 * round's attempts with rofl_dbg_msm_trace_all.
 *   rofl_dbg_msm_many:  out32[p] = sum_i scalars32[p][i] * points32[i]: np generic problems of n terms over one shared point array
 *                       (decoded as rofl_dbg_msm decodes it; 5 = a point that is no Ristretto encoding).
 *   rofl_dbg_msm_fixed: out32[p] = sum_k s[p][k] G_k + sum_k s[p][N + k] H_k over the generators of BulletproofGens::new(n_bits, m), N = n_bits m,
 *                       in the order [G | H], party-major; scalars32 is [np][2N].  The MsmOpt carries the shape's window table the way the
 *                       verifier sets it (the table chosen for np problems, slice stride 2N).  11 when the shape has no window table
 *                       (2N < ROFL_MSM_FB_MIN), np == 0 or a null pointer. */
int rofl_dbg_msm_many(size_t np, size_t n, const uint8_t *scalars32, const uint8_t *points32, uint8_t *out32);
int rofl_dbg_msm_fixed(size_t n_bits, size_t m, size_t np, const uint8_t *scalars32, uint8_t *out32);
/* The attempts of the calling thread's last msm_run, first to last: an MSM whose attempt overflowed one of its fixed-size structures is
 * repeated on the next variant (csrc/host_msm.hpp).  At most `max` records are written, *count_out is the number of attempts made.
 *   kind         the variant that ran (ROFL_MSM_*); two = 1: fixed-base through the two-level sort, 0: through the slot sort
 *   c, W         window width and window count of the attempt's layout
 *   cap          slots per bucket of the slot sort, as the plan sized them (the other variants do not use it)
 *   cap_bin      entries of a coarse bin (two-level sort), else 0;  sets: bucket sets per problem (fixed-base), else 0
 *   small_group  windows per block of the fused small launch, else 0
 *   finisher     who combines the windows (ROFL_MSM_FIN_*): host chains, k_msm_horner, or k_msm_wsum + the host's eight-lane chains
 *   overflow     the overflow word the host read back: small launch / two-level sort: non-zero = a list / a bin overflowed; slot sort: the
 *                number of entries that found their bucket's slots full (up to 4096 of them are added from the overflow list)
 *   repeated     1: the MSM was run again on the next variant */
enum { ROFL_MSM_FIXED_BASE = 0, ROFL_MSM_SMALL = 1, ROFL_MSM_SLOTS = 2, ROFL_MSM_COUNT_SORT = 3 };
enum { ROFL_MSM_FIN_HOST = 0, ROFL_MSM_FIN_DEVICE = 1, ROFL_MSM_FIN_HOST8 = 2 };
typedef struct { uint32_t kind, two, c, W, cap, cap_bin, sets, small_group, finisher, overflow, repeated; } rofl_msm_attempt_t;
int rofl_dbg_msm_trace(rofl_msm_attempt_t *attempts_out, size_t max, size_t *count_out);
/* Every msm_run of the calling thread, not only the last: a prover call makes one per inner-product round.  rofl_dbg_msm_trace_begin empties
 * the calling thread's store and switches it on (it is off until then, and stays on for that thread); from then on each msm_run appends one
 * record when it returns: tag (which hop of its caller: 99 = the S commitment, 100 + r = inner-product round r, 0 = unknown), np problems of
 * n terms, lr = 1 for the L/R-merged mode (np = 2 x chunks, n = 2 n_g: one scalar array over [Gc | Hc] serves problems 2q and 2q + 1), and
 * its n_attempts attempts as above.  rofl_dbg_msm_trace_all copies at most `max` records, oldest first; *count_out is the number of msm_runs
 * since begin (the store keeps the first 1024).  The verifier's paired MSMs (msm_run2) are not recorded.  A few stores per attempt on the
 * host, nothing that a launch depends on.  tests/test_gpu_nonce_collide.py reads the repeats of every round of a proof with it. */
typedef struct { uint32_t tag, np, n, lr, n_attempts; rofl_msm_attempt_t attempts[8]; } rofl_msm_run_t;
int rofl_dbg_msm_trace_begin(void);
int rofl_dbg_msm_trace_all(rofl_msm_run_t *out, size_t max, size_t *count_out);
/* RangeProof::verify_multiple(&BulletproofGens::new(gens_capacity, m), &PedersenGens::default(), &mut Transcript::new(label), commits, n_bits)
 * on one aggregated proof, called the way upstream's own tests call it: any transcript label, the m (a power of two) commitments as they
 * are -- no shift by 2^(n-1) B, no padding.  The operator API fixes the labels ("RangeProof", "L2RangeProof") and the shift as the reference
 * does; upstream's serialized-proof test vectors use another label (b"Deserialize-And-Verify Test", 64 x 8 generators), so this is the entry
 * through which a byte vector of bulletproofs 4.0.0 would reach the HIP verifier.  5 = malformed proof or commitment, 6 = gens_capacity < n_bits. */
int rofl_dbg_verify_labelled(const uint8_t *label, size_t label_len, size_t gens_capacity, const uint8_t *proof, size_t proof_len,
                             const uint8_t *commits32, size_t m, size_t n_bits, const uint8_t verifier_seed[32], int *ok_out);
/* process-wide counters of the MSM driver: out[0] MSMs that finished on their first attempt's variant, out[1] repeats after a bucket-list
 * overflow of the fused small launch, out[2] repeats on the slot path after a coarse bin of the two-level sort overflowed (scalars built to
 * collide), out[3] repeats after the slot path's overflow list ran out.  The server-path tests use them to show which path a scenario took. */
int rofl_dbg_msm_retries(uint64_t out[4]);
/* process-wide: the number of compressed points handed to the device's Ristretto decoder so far, added up on the host where the decoding
 * kernels are launched (padding entries that are not decoded do not count).  The round tests use it to show, without a clock, that a
 * rofl_round_* round decodes every record point once. */
int rofl_dbg_point_decodes(uint64_t *count_out);
/* field-multiply micro-benchmark: returns GF(2^255-19) multiplications per second on the device */
int rofl_bench_femul(unsigned iters, double *fe_mul_per_sec_out);
/* self-test of the quad-parallel point arithmetic (csrc/quad26.hpp): pair i = (P, Q) -> 2^doublings P + Q, one thread per pair and one quad of lanes per pair */
int rofl_dbg_quad_ops(const uint8_t *pairs64, size_t pairs, unsigned doublings, uint8_t *out_serial32, uint8_t *out_quad32);
/* The kernels' field and point arithmetic (csrc/fe26.hpp, csrc/quad26.hpp) on RAW limbs: op table csrc/fd_dbg.hpp, kernel k_dbg_fd, one
 * launch, one thread per case.  Case i reads in[80 i .. 80 i + 79] and writes out[80 i ..]; a field element is 10 limbs of radix 2^25.5
 * (limb k at bit ceil(25.5 k)) taken as they are -- not carried, not reduced -- so the caller picks the representation and must stay inside
 * the bounds the header of fe26.hpp states.  Output words an op does not write come back as the caller sent them.  a, b, c, d = elements
 * 0 .. 3 of the input; p = elements 0 .. 3 (X, Y, Z, T), q = elements 4 .. 7 (or ypx, ymx, t2d in 4 .. 6).
 *    0 fd_unpack(in[0..7] as 8 words, bit 255 kept)  -> 10 limbs        1 fd_carry(a)        2 fd_pack(a) -> 8 words, then fe_tobytes of them as 8 words
 *    3 fd_add(a, b)   4 fd_sub(a, b)   5 fd_neg(a)   6 fd_mul(a, b)   7 fd_sq(a)   8 fd_mul(fd_sub(a, b), fd_add(c, d))   9 fd_sq(fd_add(a, b))
 *   10 fd_invert(a)  11 fd_pow22523(a)  12 fd_sqrt_ratio_i(u = a, v = b) -> root in 0 .. 9, was_square in word 10   13 fd_abs(a)
 *   14 -> word 0 fd_isneg(a), word 1 fd_iszero(a), word 2 fd_eq(a, b)
 *   15 gd_madd(p, q, false)  16 gd_madd(p, q, true)  17 gd_add(p, q)  18 gd_double(p)  19 gd_double_not(p)      -> X, Y, Z, T in words 0 .. 39
 *   20 gd_to_niels(p)  21 gd_to_niels_zinv(p, element 4)                                      -> ypx, ymx, t2d as 3 x 8 packed words
 *   22 gq_double(p)  23 gq_add(p, q): one quad of lanes per case -> the quad's X, Y, Z, T in words 0 .. 39 and the one-thread gd_double /
 *      gd_add of the same case in words 40 .. 79 (device only).
 * 11 = bad parameter (op out of range, n == 0 or n > 2^20). */
int rofl_dbg_fd_ops(unsigned op, size_t n, const uint32_t *in, uint32_t *out);
/* The scalar field mod l as the kernels compile it (csrc/fe32.hpp sc_*, kernels.hpp load_sc_reduced): kernel k_dbg_sc, one thread per case.
 * Case i reads in[264 i ..]: scalars of 8 little-endian words, a = words 0 .. 7, b = 8 .. 15; writes the 8 words out[8 i ..].
 *    0 sc_montmul(a, b)  1 sc_to_mont(a)  2 sc_from_mont(a)  3 sc_mul_plain(a, b)  4 sc_add(a, b)  5 sc_neg(a)  6 sc_sub(a, b)  7 load_sc_reduced(a)
 *    8 sc_from_wide(lo = a, hi = b)  9 sc_from_wide_mont(lo = a, hi = b)
 *   10 sc_mac_wide over the in[264 i + 256] <= 16 pairs (scalar 2k, scalar 2k + 1), then ONE sc_redc_wide     11 sc_invert_mont(a) */
int rofl_dbg_sc_ops(unsigned op, size_t n, const uint32_t *in, uint32_t *out);
/* Every Ristretto encoder and identity predicate of the library on the CALLER'S representatives.  A point the library holds stands for a
 * Ristretto class, and each of K + T, T in E[4] = {(0, 1), (0, -1), (i, 0), (-i, 0)}, is a legal stand-in for the class K; which one a sum of
 * decoded points lands on is decided by the summands.  Case i is the projective point (X, Y, Z, T) of xyzt[128 i .. 128 i + 127]: four
 * canonical 32-byte field elements, any Z, loaded as they are into the site's own point type; out32[32 i ..] is the site's encoding of it
 * and is_identity_out[i] what the site's predicate says (1 / 0).  The caller answers for X Y = Z T and for the point being on the curve.
 *   site 0  gd_ristretto_encode and sg_is_identity on the device (csrc/fe26.hpp, csrc/kernels.hpp): kernel k_dbg_encode_reps, one launch,
 *           one thread per case
 *   site 1  the host build of the same fe26.hpp functions (the predicate as sg_is_identity's body: gd_pack, then ge_is_identity_ristretto)
 *   site 2  ristretto_encode and ge_is_identity_ristretto (csrc/fe32.hpp), on the host
 *   site 3  h51::encode and h51::is_identity_ristretto (csrc/host51.hpp)
 *   site 4  h8::encode8 (csrc/host51x8.hpp), eight lanes a batch in the order given -- the caller mixes the lanes; a short last batch is
 *           filled with (0, 1, 1, 0).  There is no eight-lane predicate: is_identity_out is h51's on the lanes as loaded.  Returns -1 where
 *           the CPU has no AVX-512 IFMA (nothing written).
 * Sites 1 .. 4 need no GPU.  11 = bad parameter: a null pointer, site > 4, n > 2^20, a coordinate that is not a canonical field element. */
int rofl_dbg_encode_reps(unsigned site, size_t n, const uint8_t *xyzt /* n x 4 x 32 */, uint8_t *out32 /* n x 32 */,
                         uint8_t *is_identity_out /* n */);
/* The float-to-fixed rule (conversion32.rs:11-18: |v| 2^fp_frac rounded to nearest, ties to even, saturated at 2^fp_bits - 1, negated mod l
 * for v < 0) at each of its device sites, on RAW values -- un-clipped, ties, infinities, NaN: nothing is checked on the way in.  `values` is
 * [rows][d] floats.  The production kernels are launched unchanged, with the clip bounds (get_clip_bounds(prove_range)), the grid and the
 * block count per client of their launch sites; a row is what a client is there.
 *   site 0  k_quantize_shift (range-proof create): out = uint64 [rows][dpad], dpad >= d: word i < d of a row is the shifted value
 *           ((+-k + 2^(prove_range-1)) mod l, low fp_bits bits), 0 where the value is flagged, and the padding words i >= d are 0;
 *           status_out[row] = OR over the row of 1 (outside the closed clip range) and 2 (NaN).  1 <= prove_range <= fp_bits.
 *   site 1  k_l2_sumsq_batch + k_l2_sumsq_combine (L2 sum proof): blindings32 = [rows][d][32] (any 256-bit value: reduced mod l);
 *           terms_out = float [rows][d], the element's term q q 2^fp_frac of the reference's f32 shadow sum (k taken as 0 for NaN);
 *           out = [rows][2][32]: the integer sum of k^2 (below 2^192) and the blinding sum mod l; status_out[row] as at site 0.
 *   site 2  sg_f32_to_sc (every Sigma-proof kernel, the ElGamal pairs, the compressed proof's dot product) through k_dbg_quant, one thread
 *           per value: out = [rows d][32] scalars.  prove_range, dpad, blindings32, terms_out and status_out are not read.
 * 11 = bad parameter: site > 2, (fp_bits, fp_frac) not a supported format, rows or d == 0, rows dpad > 2^20, a missing array. */
int rofl_dbg_quantize(unsigned site, size_t rows, size_t d, size_t dpad, size_t prove_range, unsigned fp_bits, unsigned fp_frac,
                      const float *values, const uint8_t *blindings32, void *out, float *terms_out, uint32_t *status_out);

/* ---- host-side self-test hooks (same source as the device math, compiled for the CPU) ---- */
/* rofl_dbg_fd_ops (ops 0 .. 21) and rofl_dbg_sc_ops through the host build, where fd_mul / fd_sq assert their operand bounds */
int rofl_dbg_host_fd_ops_raw(unsigned op, size_t n, const uint32_t *in, uint32_t *out);
int rofl_dbg_host_sc_ops(unsigned op, size_t n, const uint32_t *in, uint32_t *out);
int rofl_dbg_host_pool_stress(unsigned threads, unsigned jobs);   /* host thread pool: every index of every job runs exactly once */
int rofl_dbg_host_fe_mul(const uint8_t a[32], const uint8_t b[32], uint8_t out[32]);
int rofl_dbg_host_fe_ops(const uint8_t a[32], const uint8_t b[32], uint8_t out_add[32], uint8_t out_sub[32], uint8_t out_sq[32], uint8_t out_inv[32]);
int rofl_dbg_host_sc_invert(const uint8_t a[32], uint8_t out_ref[32], uint8_t out_fast[32], double *ns_ref, double *ns_fast);
int rofl_dbg_host_sc_mul(const uint8_t a[32], const uint8_t b[32], uint8_t out[32]);
int rofl_dbg_host_sc_wide(const uint8_t in[64], uint8_t out[32]);
/* the same through the Montgomery-form reduction the nonce kernel uses ((lo R^2 + hi R^3) R^-1, then out of Montgomery form) */
int rofl_dbg_host_sc_wide_mont(const uint8_t in[64], uint8_t out[32]);
/* sum of `count` <= 16 products a_k * b_k (operands < l) through the lazily reduced accumulator of k_verify_scalars2 (sc_mac_wide + ONE
 * sc_redc_wide) and as a sum of Montgomery products: both are sum a_k b_k / 2^256 mod l, canonical */
int rofl_dbg_host_sc_lazy(const uint8_t *a32, const uint8_t *b32, size_t count, uint8_t out_lazy[32], uint8_t out_ref[32]);
int rofl_dbg_host_from_uniform(const uint8_t in[64], uint8_t out[32]);
int rofl_dbg_host_scalarmult_base(const uint8_t k[32], int use_blinding_base, uint8_t out[32]);
int rofl_dbg_host_fd_codec(const uint8_t in[32], uint8_t out[32]);
int rofl_dbg_host_decode_encode(const uint8_t in[32], uint8_t out[32]);   /* returns 5 if invalid */
/* radix-2^25.5 kernel arithmetic (fe26.hpp) compiled for the host with bound assertions enabled */
int rofl_dbg_host_fd_ops(const uint8_t a[32], const uint8_t b[32], uint8_t out_mul[32], uint8_t out_sq[32], uint8_t out_add[32], uint8_t out_sub[32], uint8_t out_inv[32]);
int rofl_dbg_host_fd_scalarmult(const uint8_t k[32], const uint8_t p[32], uint8_t out[32]);   /* k P on the kernel point formulas; k is reduced mod l first */
int rofl_dbg_host_merlin(const uint8_t *label, size_t label_len, const uint8_t *msg, size_t msg_len, uint8_t out[64]);
int rofl_dbg_host_nonce(const uint8_t seed[32], uint64_t idx, uint8_t out[32]);
/* scalar idx of the blinding stream of a seed (rofl_blinding_vecs), computed on the host from the source the kernel is compiled from */
int rofl_dbg_host_blind(const uint8_t seed[32], uint64_t idx, uint8_t out[32]);
/* word idx of the rounding stream of a seed (rofl_quantize_prob): word idx & 31 of block idx >> 5, on the host from the kernel's source */
int rofl_dbg_host_quant(const uint8_t seed[32], uint64_t idx, uint32_t *word_out);
/* The rounding rule of rofl_quantize_prob on caller-supplied words instead of a seed's stream: out[i] = the rule applied to values[i] with
 * words[i], so that a test can sit exactly on word = t - 1, t, 0 and 2^32 - 1.  site 0: the host copy (no GPU); site 1: the device copy
 * (k_dbg_quant_round, one thread per case).  11: site > 1, an invalid format, prove_range = 0, a null array with n > 0, n > 2^20. */
int rofl_dbg_quant_round(unsigned site, size_t n, const float *values, const uint32_t *words, size_t prove_range, unsigned fp_bits,
                         unsigned fp_frac, float *out);
/* rofl_quantize_prob with the route chosen by the caller instead of by the pointers and the size: route 0 = the host copy of the rule (host
 * pointers only, else 11), 1 = the kernel.  Same checks, same bytes; what scripts/gpu_prob_quant.py finds the crossover with. */
int rofl_dbg_quantize_prob_route(unsigned route, size_t n_vec, const uint8_t *seeds32, const float *const *values, size_t first, size_t d,
                                 size_t prove_range, unsigned fp_bits, unsigned fp_frac, float *const *out);
/* noise integer n_e of element index e of a seed's noise stream (rofl_noise_binomial), on the host from the kernel's source.  11: a null
 * pointer, a k the call rejects, (e + 1) k / 16 > 2^63. */
int rofl_dbg_host_noise(const uint8_t seed[32], uint64_t e, uint32_t k, int32_t *n_out);
/* The value rule of rofl_noise_binomial on caller-supplied noise instead of a seed's stream: out[i] = the rule applied to values[i] with
 * noise_i32[i], so that a test can sit exactly on the clip bounds.  site 0: the host copy (no GPU); site 1: the device copy
 * (k_dbg_noise_apply, one thread per case).  11: site > 1, an invalid format, prove_range = 0, a null array with n > 0, n > 2^20. */
int rofl_dbg_noise_apply(unsigned site, size_t n, const float *values, const int32_t *noise_i32, size_t prove_range, unsigned fp_bits,
                         unsigned fp_frac, float *out);
/* rofl_noise_binomial with the route chosen by the caller instead of by the pointers and the size: route 0 = the host copy of the rule (host
 * pointers only, else 11), 1 = the kernel.  Same checks, same bytes; what scripts/gpu_binomial_noise.py finds the crossover with. */
int rofl_dbg_noise_binomial_route(unsigned route, size_t n_vec, const uint8_t *seeds32, const float *const *values, size_t first, size_t d,
                                  uint32_t k, size_t prove_range, unsigned fp_bits, unsigned fp_frac, float *const *out);
/* noise integer of element index e of a seed under rofl_noise_dgauss and the stream words it consumed (words_used_out may be null), on the
 * host from the kernel's source.  11: a null seed or noise_out, a sigma2 the call rejects, e >= 2^55. */
int rofl_dbg_host_dgauss(const uint8_t seed[32], uint64_t e, uint32_t sigma2, int32_t *noise_out, uint32_t *words_used_out);
/* The sampler of rofl_noise_dgauss on caller-supplied words instead of a seed's stream: case i runs over words[i stride .. i stride +
 * lens[i]) with sigma2s[i] and leaves its noise, the words it read and whether it finished (0: it asked for a word past lens[i] or past
 * word 8 191; the noise is then 0).  site 0: the host copy (no GPU); site 1: the device copy (k_dbg_dgauss_words, one thread per case).
 * 11: site > 1, n_cases > 2^20, stride > 8 192, n_cases stride > 2^26, lens[i] > stride, a sigma2 the call rejects, a null array. */
int rofl_dbg_dgauss_words(unsigned site, size_t n_cases, const uint32_t *words, size_t stride, const uint32_t *lens, const uint32_t *sigma2s,
                          int32_t *noise_out, uint32_t *used_out, uint32_t *finished_out);
/* rofl_noise_dgauss with the route chosen by the caller instead of by the pointers and the size: route 0 = the host copy of the rule (host
 * pointers only, else 11), 1 = the kernel.  Same checks, same bytes; what scripts/gpu_dgauss_noise.py finds the crossover with. */
int rofl_dbg_noise_dgauss_route(unsigned route, size_t n_vec, const uint8_t *seeds32, const float *const *values, size_t first, size_t d,
                                uint32_t sigma2, size_t prove_range, unsigned fp_bits, unsigned fp_frac, float *const *out);
/* How k_noise_dgauss lays out a call of ONE vector of d elements (more vectors only raise the first figure): the elements a lane owns,
 * and the XOF blocks a lane's LDS ring holds -- an element that needs more than those wraps the ring.  No GPU.  11: a null pointer, d >= 2^28. */
int rofl_dbg_dgauss_geometry(size_t d, uint32_t *elements_per_lane, uint32_t *lds_blocks);
/* Step 4 of rofl_clip_l2 on caller-supplied step counts, scale and words instead of a vector's sum and a seed's stream: out[i] =
 * trunc24((q[i] m >> 32) + (words[i] < q[i] m mod 2^32 ? 1 : 0)) 2^-fp_frac, positive; words == NULL: the unseeded rule (no + 1).
 * site 0: the host copy (no GPU); site 1: the device copy (k_dbg_clip_l2_round, one thread per case).  11: site > 1, fp_frac > 12, a null
 * q or out with n > 0, n > 2^20. */
int rofl_dbg_clip_l2_round(unsigned site, size_t n, const uint64_t *q, uint32_t m, const uint32_t *words, unsigned fp_frac, float *out);
/* rofl_clip_l2 with the route chosen by the caller instead of by the pointers and the size: route 0 = the host copy of the rule (host
 * pointers only, else 11), 1 = the kernels.  Same checks, same bytes; what scripts/gpu_l2_clip.py finds the crossover with. */
int rofl_dbg_clip_l2_route(unsigned route, size_t n_vec, const uint8_t *seeds32, const float *const *values, size_t d, const uint64_t *max_sq,
                           size_t prove_range, unsigned fp_bits, unsigned fp_frac, float *const *out, uint64_t *scale_out);
/* rofl_rotate with the route chosen by the caller instead of by the pointers and the size: route 0 = the host copy of the network (host
 * pointers only, else 11), 1 = the kernels.  Same checks, same bytes; what scripts/gpu_rotate.py finds the crossover with. */
int rofl_dbg_rotate_route(unsigned route, size_t n_vec, const uint8_t *seeds32, const float *const *values, size_t d, unsigned block_log2, int inverse,
                          float *const *out);
/* log2 of the elements a workgroup of k_rotate_tile owns: blocks up to this size take one launch, longer ones also k_rotate_cols.  No GPU. */
int rofl_dbg_rotate_tile_log2(void);
/* one pair of rofl_dh_shared from the host arithmetic (no GPU): out32 and *status as that call gives them; own_pk32 == NULL: computed from sk32.
 * Returns 11 for a null pointer or a secret key that is 0 mod l. */
int rofl_dbg_host_dh(const uint8_t sk32[32], const uint8_t *own_pk32, const uint8_t peer_pk32[32], uint8_t out32[32], uint8_t *status);
/* rofl_shamir_share / rofl_shamir_reconstruct on the host's scalar arithmetic and host Keccak, one thread, no GPU: the same parameters, the
 * same checks (11) and the same bytes.  What the host tests pin the definition with, and the baseline of profiles/shamir_sharing.json. */
int rofl_dbg_host_shamir_share(size_t n_secrets, const uint8_t *secrets32, const uint8_t *coef_seeds32, size_t threshold, size_t n_shares,
                               const uint32_t *xs, uint8_t *shares_out32);
int rofl_dbg_host_shamir_reconstruct(size_t n_secrets, size_t n_shares, const uint32_t *xs, const uint8_t *shares32, uint8_t *secrets_out32);
/* rofl_feldman_commit / rofl_feldman_verify on the host's 51-bit point arithmetic, scalar arithmetic and host Keccak, one thread, no GPU: the
 * same parameters, the same checks (11) and the same bytes.  What the host tests pin the definition with, and the baseline of
 * profiles/feldman_vss.json. */
int rofl_dbg_host_feldman_commit(size_t n_secrets, const uint8_t *secrets32, const uint8_t *coef_seeds32, size_t threshold,
                                 uint8_t *commitments_out32);
int rofl_dbg_host_feldman_verify(size_t n_secrets, size_t threshold, const uint8_t *commitments32, size_t n_shares, const uint32_t *xs,
                                 const uint8_t *shares32, uint8_t *verdict_out);
/* rofl_sig_sign / rofl_sig_verify on the host's 51-bit point arithmetic, scalar arithmetic and host Keccak, one thread, no GPU: the same
 * parameters, the same checks (11) and the same bytes.  What the host tests pin the definition with, and the baseline of
 * profiles/signatures.json. */
int rofl_dbg_host_sig_sign(size_t n_keys, const uint8_t *sk32, uint8_t *pk_out32, size_t n_msgs, const uint8_t *msg_bytes,
                           const uint64_t *msg_off, size_t n, const rofl_sig_ref_t *refs, uint8_t *sig_out64);
int rofl_dbg_host_sig_verify(size_t n_keys, const uint8_t *pk32, size_t n_msgs, const uint8_t *msg_bytes, const uint64_t *msg_off,
                             size_t n, const rofl_sig_ref_t *refs, const uint8_t *sig64, uint8_t *verdict_out);
/* rofl_aead_seal / rofl_aead_open in plain C++ on one thread, no GPU: the same parameters, the same checks (11) and the same bytes.  What the
 * host tests pin the definition with, and the baseline of profiles/share_seal.json on a box without libsodium. */
int rofl_dbg_host_aead_seal(size_t n_keys, const uint8_t *key32, const uint64_t *derive_round, size_t n, const uint32_t *key_idx,
                            const uint8_t *nonce12, const uint8_t *ad_bytes, const uint64_t *ad_off, const uint8_t *pt_bytes,
                            const uint64_t *pt_off, uint8_t *sealed_out);
int rofl_dbg_host_aead_open(size_t n_keys, const uint8_t *key32, const uint64_t *derive_round, size_t n, const uint32_t *key_idx,
                            const uint8_t *nonce12, const uint8_t *ad_bytes, const uint64_t *ad_off, const uint8_t *sealed_bytes,
                            const uint64_t *sealed_off, uint8_t *pt_out, uint8_t *verdict_out);
/* Poly1305 alone, because an AEAD call cannot choose (r, s): tag_out16[j] = the tag of message j = msg_bytes[msg_off[j] .. msg_off[j + 1])
 * under key32[j] = r || s (r is clamped inside).  rofl_dbg_poly1305 runs the AEAD kernels' own device function, one thread per message, one
 * launch; rofl_dbg_host_poly1305 the host route's.  11 for a null pointer, n above 2^20, bad offsets, a message above 2^24 bytes. */
int rofl_dbg_poly1305(size_t n, const uint8_t *key32 /* n x 32 */, const uint8_t *msg_bytes, const uint64_t *msg_off /* n + 1 */,
                      uint8_t *tag_out16 /* n x 16 */);
int rofl_dbg_host_poly1305(size_t n, const uint8_t *key32, const uint8_t *msg_bytes, const uint64_t *msg_off, uint8_t *tag_out16);
/* rofl_dleq_prove / rofl_dleq_verify on the host's 51-bit point arithmetic, scalar arithmetic and host Keccak, one thread, no GPU: the same
 * parameters, the same checks (11) and the same bytes.  What the host tests pin the definition with, and the baseline of profiles/dleq.json. */
int rofl_dbg_host_dleq_prove(size_t n_own, const uint8_t *sk32, uint8_t *own_pk_out32, size_t n_peer, const uint8_t *peer_pk32, size_t n_pairs,
                             const rofl_dh_pair_t *pairs, const uint8_t *ctx32, uint8_t *reveal_out32, uint8_t *proof_out64, uint8_t *status_out);
int rofl_dbg_host_dleq_verify(size_t n_own, const uint8_t *own_pk32, size_t n_peer, const uint8_t *peer_pk32, size_t n_pairs,
                              const rofl_dh_pair_t *pairs, const uint8_t *ctx32, const uint8_t *reveal32, const uint8_t *proof64,
                              uint8_t *shared_out32, uint8_t *verdict_out);
/* rofl_merkle_build / rofl_merkle_verify on the host's sponge, one thread, no GPU: the same parameters, the same checks (11) and the same
 * bytes and verdicts.  What the host tests pin the definition with, and the baseline of profiles/merkle.json.
 * rofl_dbg_merkle_tile_leaves: the number of nodes a workgroup of k_mt_tile owns, so that tests can place n around it; no output byte
 * depends on it. */
int rofl_dbg_host_merkle_build(size_t n, const uint8_t *msg_bytes, const uint64_t *msg_off, uint8_t *root_out32, uint8_t *leaves_out32,
                               size_t n_paths, const uint32_t *path_idx, uint8_t *paths_out32);
int rofl_dbg_host_merkle_verify(size_t n_roots, const uint8_t *root32, const uint32_t *n_leaves, size_t n_paths, const rofl_merkle_ref_t *refs,
                                const uint8_t *msg_bytes, const uint64_t *msg_off, const uint8_t *paths32, size_t stride, uint8_t *verdict_out);
size_t rofl_dbg_merkle_tile_leaves(void);
/* out32[i] = encode(k1[i] decode(p1[i]) + k2[i] decode(p2[i])) through the kernels' own device functions, one thread per item, n <= 2^24:
 * rofl_dbg_var_mul2 on the joint chain sg_var_mul2 (two tables, one chain of doublings), rofl_dbg_var_mul_sum as the sum of two sg_var_mul
 * products.  Scalars are reduced mod l; a point that does not decode counts as the identity.  *kernel_ms (may be NULL): the launch alone,
 * between two events on the lane's stream -- the A/B of profiles/dleq.json. */
int rofl_dbg_var_mul2(size_t n, const uint8_t *k1_32, const uint8_t *p1_32, const uint8_t *k2_32, const uint8_t *p2_32, uint8_t *out32, double *kernel_ms);
int rofl_dbg_var_mul_sum(size_t n, const uint8_t *k1_32, const uint8_t *p1_32, const uint8_t *k2_32, const uint8_t *p2_32, uint8_t *out32, double *kernel_ms);
/* What the protocol calls above, the seeded update-preparation calls (rofl_quantize_prob, rofl_noise_binomial, rofl_clip_l2) and the term
 * lists of rofl_blinding_vecs / rofl_acc_extract_opened_terms leave behind: the n >= 16 bytes at `needle` are searched for in the staging buffers of every initialised lane
 * of the calling thread's device -- the pinned buffers h_misc and h_misc2 and host copies of the device workspaces tmp_in, tmp_in2 and
 * tmp_out, each up to its capacity, under the lane's mutex and after a synchronisation of its stream.  *found = the number of buffers that
 * hold the needle (0 on a device no call has used yet).  Nothing is written to any of them: tests/test_gpu_lane_residue.py scans for
 * every secret of a call (none may be found) and for one public by-product (which must be).  Cost: every device workspace is copied to
 * the host in full with a blocking hipMemcpy and searched linearly -- the workspaces only grow, so after a large call that is gigabytes
 * and seconds per scan.  A hook for tests on small shapes, nothing to call on a serving path. */
int rofl_dbg_lane_scan(const uint8_t *needle, size_t n, int *found);

/* host micro-benchmarks of the code the per-round hops run (nanoseconds per operation on the calling core).
 * what: 0 Keccak-f[1600]; 1 point doubling, 2 point addition, 3 Ristretto encoding (51-bit host arithmetic);
 *       4 fixed-base scalar multiplication; 5 scalar inversion; 6 Merlin transcript prefix of `iters` commitments (ns per commitment);
 *       7 / 8 / 9 one pool hand-off of a hop: 16 tasks of 30 us after a 300 us / 30 us wait of the caller, 128 tasks of 8 us after 300 us */
int rofl_dbg_host_bench(int what, unsigned iters, double *ns_out);
/* csrc/host51x8.hpp (eight window chains per AVX-512 IFMA stream) against the scalar chain of host51.hpp on 8 x W pseudo-random points,
 * windows c bits apart: 0 = all `lanes` results agree, 1 = mismatch, -1 = the CPU has no AVX-512 IFMA (nothing tested) */
int rofl_dbg_host_horner8_selftest(unsigned W, unsigned c, int lanes, double *us_simd, double *us_scalar);
/* h8::encode8 (eight Ristretto encodings per AVX-512 IFMA stream) against the scalar host encoder: 0 = all equal, 1 = mismatch, -1 = no IFMA */
int rofl_dbg_host_encode8_selftest(unsigned batches, double *us_simd, double *us_scalar);
/* csrc/keccak_x8.hpp (eight Merlin transcripts per AVX-512 stream: the verifier's transcript prefixes) against the scalar transcript:
 * `lanes` transcripts, `count` commitments each, `skew` extra prefix bytes (moves the records across the rate block): 0 = states and the
 * next challenge agree, 1 = mismatch, -1 = no AVX-512 on this CPU */
int rofl_dbg_host_merlin8_selftest(int lanes, unsigned count, unsigned skew, double *us_simd, double *us_scalar);
/* the same for the labelled pairs of a CompressedRandProof transcript (k8::append_lbl3_run_x8: eight transcripts of count x
 * append_lbl({3i, 3i + 1, 3i + 2}, pair_i, 64) per AVX-512 stream) against the scalar Merlin::append_lbl loop: `lanes` transcripts,
 * `count` pairs each, `skew` (<= 400) extra prefix bytes; 0 = states, positions and the challenge drawn after C' agree, 1 = mismatch,
 * -1 = no AVX-512 on this CPU */
int rofl_dbg_host_merlin8_lbl3_selftest(int lanes, unsigned count, unsigned skew, double *us_simd, double *us_scalar);
/* the same with the pairs read every `stride` bytes (64 .. 256; 96: the pairs inside SquareRandProofCommitments records, as a strict
 * EncL2Compressed check hashes them): bytes 64 .. stride of every record are filler that differs per lane and per record, and the scalar
 * side hashes a packed copy of the first 64 bytes of each record -- 0 = states, positions and the challenge drawn after C' agree (no
 * filler byte reached a transcript), 1 = mismatch, -1 = no AVX-512 on this CPU, 11 = bad parameter.  CPU-only. */
int rofl_dbg_host_merlin8_lbl3_strided_selftest(int lanes, unsigned count, unsigned skew, unsigned stride, double *us_simd, double *us_scalar);
/* Merlin::append32_run (the run of m commitment appends of a chunk, records assembled in registers and split at the end of the rate block)
 * against `count` plain appends after `skew` (<= 400) extra prefix bytes: 0 = state, positions and next challenge equal, 1 = mismatch */
int rofl_dbg_host_merlin_run_selftest(unsigned count, unsigned skew);
/* csrc/keccak.hpp keccak_f1600_zmm (ONE Keccak-f[1600] state across five AVX-512 registers: what every host transcript runs where the CPU has
 * it) against the scalar permutation: `states` pseudo-random states permuted `chain` times each, and the known answer of the zero state.
 * 0 = all equal, 1 = mismatch, -1 = no AVX-512 on this CPU; ns per permutation of both on request */
int rofl_dbg_host_keccak_zmm_selftest(unsigned states, unsigned chain, double *ns_zmm, double *ns_scalar);
/* host share of the hops of the calling thread's last create / verify: out[0] hops, [1] enqueue ms, [2] wait ms, [3] window-combination wall ms,
 * [4] sum of each hop's slowest pool task ms, [5..8] the maxima over the hops of enqueue, wait, combination wall, slowest task */
int rofl_dbg_last_hops(double out[10]);

#ifdef __cplusplus
}
#endif
#endif
