// librofl_zk.so: C ABI (include/rofl_zk.h) + host orchestration of the HIP kernels.  One translation unit, in sections:
//   host_rt.hpp (knobs, pool, buffers, lanes, generator cache) | host_msm.hpp (MSM driver) | host_prover.hpp | host_verifier.hpp |
//   this file: conversion32 helpers, create / verify entry logic, the extern "C" block.
//
// Host responsibilities: Merlin transcripts (sequential), final window/bit combination of MSM partial
// sums (a 256-step Horner chain that would serialise a single GPU lane), fixed-base multiples of B and
// B_blinding, proof (de)serialisation.  Everything proportional to d * n_bits runs in kernels.hpp.
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>      // types only: the library is loaded with dlopen when rofl_comm_* is first used (no link-time dependency)
#include <dlfcn.h>
#include <immintrin.h>
#include <chrono>
#include <time.h>
#include <sched.h>
#include <unistd.h>
#include <sys/syscall.h>
#include <linux/futex.h>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <memory>
#include <atomic>
#include <condition_variable>
#include <deque>
#include <exception>
#include <functional>
#include <mutex>
#include <shared_mutex>
#include <stdexcept>
#include <thread>
#include <string>
#include <vector>

#include "../../include/rofl_zk.h"
#include "../../include/rofl_zk_debug.h"
#include "kernels.hpp"
#if ROFL_KGROUP != 0
#include "kernel_protos.hpp"      // kernels live in their own translation units (build.py)
#endif
#include "wire.hpp"
#include "host51.hpp"
#include "host51x8.hpp"
#include "keccak_x8.hpp"

using namespace rofl;

namespace {

#include "host_rt.hpp"
#include "host_msm.hpp"
#include "host_prover.hpp"
#include "host_verifier.hpp"

// ---------------------------------------------------------------- conversion32.rs helpers (host)
u64 fix_max_bits(unsigned fp_bits) { return fp_bits >= 64 ? ~0ULL : ((1ULL << fp_bits) - 1); }
int fix_from_abs_f32(float v, unsigned fp_bits, unsigned fp_frac, u64 *out) {
    if (std::isnan(v)) return ROFL_NON_FINITE;
    double x = std::fabs((double)v) * (double)(1ULL << fp_frac);
    double lim = std::ldexp(1.0, (int)fp_bits);
    if (std::isinf(x) || x >= lim) { *out = fix_max_bits(fp_bits); return 0; }
    double k = std::nearbyint(x);
    *out = (k >= lim) ? fix_max_bits(fp_bits) : (u64)k;
    return 0;
}
float fix_to_f32(u64 k, unsigned fp_frac) { volatile float f = (float)k; return f / (float)(1ULL << fp_frac); }
u64 read_from_bytes(const sc &s, unsigned fp_bits) { u64 r = (u64)s.v[0] | ((u64)s.v[1] << 32); return r & fix_max_bits(fp_bits); }
int f32_to_sc(float v, unsigned fp_bits, unsigned fp_frac, sc *out) {
    u64 k; int rc = fix_from_abs_f32(v, fp_bits, fp_frac, &k); if (rc) return rc;
    sc s = sc_from_u64(k); *out = (v < 0.0f) ? sc_neg(s) : s; return 0;
}
float sc_to_f32(const sc &s, unsigned fp_bits, unsigned fp_frac) {
    if ((s.v[7] >> 24) != 0) return -fix_to_f32(read_from_bytes(sc_neg(s), fp_bits), fp_frac);
    return fix_to_f32(read_from_bytes(s, fp_bits), fp_frac);
}
void clip_bounds(size_t range, unsigned fp_bits, unsigned fp_frac, float *mn, float *mx) {
    unsigned __int128 v = ((unsigned __int128)1 << (range - 1)) - 1;
    *mx = fix_to_f32((u64)v & fix_max_bits(fp_bits), fp_frac); *mn = -*mx;
}
float l2_clip_bound(size_t range, unsigned fp_bits, unsigned fp_frac) {
    unsigned __int128 v = ((unsigned __int128)1 << range) - 1;
    return fix_to_f32((u64)v & fix_max_bits(fp_bits), fp_frac);
}
bool valid_fp(unsigned fp_bits, unsigned fp_frac) { return (fp_bits == 8 || fp_bits == 16 || fp_bits == 32 || fp_bits == 64) && fp_frac <= 12 && fp_frac < fp_bits; }

thread_local rofl_timing_t g_last_timing{};
thread_local double g_last_hops[10] = {0};      // rofl_dbg_last_hops: the HopStats of the calling thread's last range-proof call
thread_local rofl_kernel_time_t g_last_ktimes[ROFL_TK_COUNT]{};
void timing_begin(Ctx &C) {
    C.tm.reset();
    if (C.tm.enabled) { C.tm.first = C.tm.get(); C.tm.last = C.tm.get(); HIPCHK(hipEventRecord(C.tm.first, C.stream)); }
}
void timing_end(Ctx &C) {
    { const auto &h = C.hs; double v[10] = {(double)h.n, h.enqueue, h.sync, h.horner_wall, h.horner_cpu, h.max_enqueue, h.max_sync, h.max_horner, h.max_task, 0}; memcpy(g_last_hops, v, sizeof v); C.hs = Ctx::HopStats(); }
    if (!C.tm.enabled) {
        g_last_timing = C.tm.t; memset(g_last_ktimes, 0, sizeof g_last_ktimes);
        if (C.tm.acc_only && !C.tm.kev.empty()) {      // the stream has been synchronised by the caller's last wait: the few recorded spans are complete
            float ms = 0;
            for (auto &k : C.tm.kev) {
                if (hipEventSynchronize(k.e1) != hipSuccess || hipEventElapsedTime(&ms, k.e0, k.e1) != hipSuccess) continue;
                rofl_kernel_time_t &o = g_last_ktimes[k.kind]; o.ms += ms; o.launches++; o.fe_muls += k.fe_muls; o.bytes += k.bytes;
            }
        }
        return;
    }
    HIPCHK(hipEventRecord(C.tm.last, C.stream));
    HIPCHK(hipEventSynchronize(C.tm.last));
    float ms = 0; HIPCHK(hipEventElapsedTime(&ms, C.tm.first, C.tm.last)); C.tm.t.total_ms = ms;
    bool trace = knob("ROFL_TRACE") != nullptr;
    for (size_t i = 0; i < C.tm.acc_ev.size(); i++) { auto &e = C.tm.acc_ev[i]; HIPCHK(hipEventElapsedTime(&ms, e.first, e.second)); C.tm.t.msm_accumulate_ms += ms; if (trace) fprintf(stderr, "[rofl] %-40s accumulate %.3f ms\n", C.tm.acc_tag[i].c_str(), ms); }
    for (size_t i = 0; i < C.tm.fold_ev.size(); i++) { auto &e = C.tm.fold_ev[i]; HIPCHK(hipEventElapsedTime(&ms, e.first, e.second)); C.tm.t.fold_ms += ms; if (trace) fprintf(stderr, "[rofl] %-40s %.3f ms\n", C.tm.fold_tag[i].c_str(), ms); }
    for (auto &k : C.tm.kev) {
        HIPCHK(hipEventElapsedTime(&ms, k.e0, k.e1));
        rofl_kernel_time_t &o = C.tm.kt[k.kind]; o.ms += ms; o.launches++; o.fe_muls += k.fe_muls; o.bytes += k.bytes;
    }
    memcpy(g_last_ktimes, C.tm.kt, sizeof g_last_ktimes);
    g_last_timing = C.tm.t;
}


// BSGSTable::new(table_size) on the device, built once per table_size and cached on the device's primary lane (callers hold it: acquire_lane(true)),
// then one k_bsgs_solve over the d compressed points at dp (device) -> canonical scalars at dout; status bit 8: a log that was not found
void bsgs_solve_launch(Ctx &C, size_t d, const uint8_t *dp, size_t table_size, unsigned bsgs_bits, uint8_t *dout, u32 *status) {
    auto it = C.bsgs.find(table_size);
    if (it == C.bsgs.end()) {
        Ctx::Bsgs b; u32 nslots = 1; while (nslots < 2 * (table_size + 1)) nslots <<= 1;
        b.mask = nslots - 1;
        HIPCHK(hipMalloc(&b.keys, 32 * (table_size + 1))); HIPCHK(hipMalloc(&b.slots, sizeof(u32) * nslots));
        HIPCHK(hipMemsetAsync(b.slots, 0, sizeof(u32) * nslots, C.stream));
        ROFL_LAUNCH(k_bsgs_build, dim3((unsigned)((table_size + 1 + 63) / 64)), dim3(64), 0, C.stream, (u32)table_size, C.d_tabB, b.keys, b.slots, b.mask);
        it = C.bsgs.emplace(table_size, b).first;
    }
    const Ctx::Bsgs &B = it->second;
    u64 mask = bsgs_bits >= 32 ? 0xffffffffULL : ((1ULL << bsgs_bits) - 1);
    // mG = B * Scalar::from(m as BSGS_URawFix)  (bsgs32.rs:18): the multiplier wraps to bsgs_bits bits
    niels neg_mG = h51::to_niels32(h_fixed_mul(C.ht.B5, sc_neg(sc_from_u64((u64)table_size & mask))));
    u64 max_it = (1ULL << bsgs_bits) / table_size;
    ROFL_LAUNCH(k_bsgs_solve, dim3((unsigned)((d + 63) / 64)), dim3(64), 0, C.stream, (u32)d, dp, (u32)table_size, bsgs_bits, max_it, neg_mG, B.keys, B.slots, B.mask, dout, status);
}

// The commitments of a batched verification leg that come from a round (rofl_round_*) instead of caller memory: the records' bytes and
// their decoded points are on the device already (k_round_ingest), and what did not decode is known per client and slot.
struct RoundSrc {
    size_t d, npts;            // the records: d per client, npts points each (2: ElGamal pair, 3: SquareRandProofCommitments)
    const uint8_t *rec;        // device: [client][d][32 npts], as ingested
    niels *pts;                // device: [client][2 npts][d], record points in the even slots (see k_round_ingest)
    const u32 *bad;            // host: [client][3] -- smallest index of an undecodable L / R / c_sq, 0xffffffff: none
};

constexpr size_t kMaxBatchMembers = 65535;      // gridDim.y: what a batch entry point accepts in one call (the launches themselves are checked too, ROFL_LAUNCH)

template <class F> int guarded(F f) {
    try { return f(); }
    catch (const HipErr &e) {
        char buf[256]; snprintf(buf, sizeof buf, "HIP error %d (%s) in %s", (int)e.e, hipGetErrorString(e.e), e.what);
        return fail(ROFL_HIP_ERROR + (int)e.e, buf);
    }
    catch (const std::exception &e) { return fail(ROFL_HIP_ERROR, std::string("exception: ") + e.what()); }
}

// create_rangeproof for `nc` clients of one shape (d, prove_range, n_partition) as ONE launch sequence: the clients' chunks are laid
// side by side ([client][chunk]), every kernel of the proof covers all of them (blockIdx.y = chunk), and every IPP round carries the
// L / R problems of all clients -- the host hops, the latency-bound tail and the launch overheads are paid once per batch instead of
// once per client.  rcs[i] = the per-client outcome (ValueOutOfRange, NaN, nonce stream too short); clients that fail are left out,
// the others are proved.  Returns non-zero only for errors that concern the whole call.
int create_impl(Ctx &C, size_t nc, const float *const *values, size_t d, const uint8_t *const *blind, size_t prove_range, size_t n_partition,
                unsigned fp_bits, unsigned fp_frac, const rofl_nonce_t *nonces, uint8_t *const *proofs_out, size_t *plen_out, size_t *np_out,
                uint8_t *const *commits_out, int *rcs, bool single, size_t chunk_first = 0, size_t chunk_count = 0) {
    // `single`: the call is rofl_create_rangeproof (one client: its errors are the call's errors); batch calls -- also their one-client
    // shards when a batch is spread over several devices -- report per client in rcs.
    // [chunk_first, chunk_first + chunk_count) (count 0: all): the chunks of every client that THIS call proves -- the reference proves a
    // client's chunks independently of each other (range_proof_vec/mod.rs:54-78: par_iter over the chunks, a transcript and a generator set
    // per chunk), so a device or a rank can take any run of them.  values / blindings are still the client's whole vectors (the range check
    // of :27-29 is over the slice this call reads; the caller of a split combines the outcomes); proofs_out[i] receives chunk_count proofs,
    // commits_out[i] the commitments of the run's own elements, i.e. it points at element chunk_first * m of the client's array; the nonce
    // index space stays the client's (chunk c draws from c * m * (2n + 4)), so the bytes are those of the unsplit call.
    for (size_t i = 0; i < nc; i++) rcs[i] = ROFL_OK;
    if (!valid_fp(fp_bits, fp_frac) || d == 0 || n_partition == 0 || prove_range == 0 || prove_range > fp_bits || !nonces || nc == 0)
        return fail(ROFL_BAD_PARAM, "bad parameter (the reference panics here)");
    const size_t d_all = d, dp_all = next_pow2(d);
    size_t n_chunks = std::min(dp_all, n_partition), chunk = dp_all / n_chunks;
    const size_t P_all = (dp_all + chunk - 1) / chunk;
    if (chunk_count == 0) { chunk_first = 0; chunk_count = P_all; }
    if (chunk_first >= P_all || chunk_count > P_all - chunk_first) return fail(ROFL_BAD_PARAM, "chunk range outside the client's chunks");
    // from here on d, dp, P describe the run: `d` real elements (possibly none: a run of padding chunks) at the front of dp = P * chunk
    const size_t el0 = chunk_first * chunk;
    const size_t P = chunk_count, dp = P * chunk;
    d = el0 >= d_all ? 0 : std::min(d_all - el0, dp);
    float mn, mx; clip_bounds(prove_range, fp_bits, fp_frac, &mn, &mx);
    C.init();
    C.batch_mode = nc > 1;
    timing_begin(C);
    float *d_vals = C.vals.as<float>(nc * d + 1);
    u64 *vshift = C.vshift.as<u64>(nc * dp);
    sc *d_blind_buf = C.blind.as<sc>(nc * dp);
    HIPCHK(hipMemsetAsync(d_blind_buf, 0, sizeof(sc) * nc * dp, C.stream));
    for (size_t i = 0; i < nc && d; i++) {      // the callers' arrays: host or device memory
        C.up(d_vals + i * d, values[i] + el0, sizeof(float) * d, C.stream);
        C.up(d_blind_buf + i * dp, blind[i] + el0 * 32, 32 * d, C.stream);
    }
    u32 *status = C.status.as<u32>(nc + 4);
    HIPCHK(hipMemsetAsync(status, 0, 4 * (nc + 4), C.stream));
    ROFL_LAUNCH(k_quantize_shift, grid1(dp, (u32)nc), dim3(TPB), 0, C.stream, d_vals, (u32)d, (u32)dp, (u32)prove_range, fp_bits, fp_frac, mn, mx, vshift, status);
    u32 *h_status = C.h_misc.as<u32>(nc + 4);
    HIPCHK(hipMemcpyAsync(h_status, status, 4 * nc, hipMemcpyDeviceToHost, C.stream));
    C.sync();
    // the reference's order of checks (range_proof_vec/mod.rs:22-29, then the upstream errors)
    bool any = false;
    for (size_t i = 0; i < nc; i++) {
        if (h_status[i] & 1) rcs[i] = ROFL_VALUE_OUT_OF_RANGE;
        else if (h_status[i] & 2) rcs[i] = ROFL_NON_FINITE;
        any |= rcs[i] == ROFL_OK;
    }
    if (single && rcs[0] == ROFL_VALUE_OUT_OF_RANGE) return fail(ROFL_VALUE_OUT_OF_RANGE, "ValueOutOfRangeError");
    if (single && rcs[0] == ROFL_NON_FINITE) return fail(ROFL_NON_FINITE, "non-finite value (the reference panics in fixed::saturating_from_float)");
    if (!is_pow2(chunk) || dp % chunk) return fail(ROFL_INVALID_AGGREGATION, "InvalidAggregation (the reference panics)");
    if (!(prove_range == 8 || prove_range == 16 || prove_range == 32 || prove_range == 64)) return fail(ROFL_INVALID_BITSIZE, "InvalidBitsize");
    for (size_t i = 0; i < nc; i++)
        if (rcs[i] == ROFL_OK && nonces[i].mode == 0 && nonces[i].stream_scalars < P_all * chunk * (2 * prove_range + 4)) {
            rcs[i] = ROFL_NONCE_SHORT;
            if (single) return fail(ROFL_NONCE_SHORT, "nonce stream too short");
        }
    size_t plen = 32 * (9 + 2 * (size_t)lg2u(prove_range * chunk));
    *plen_out = plen; *np_out = P;
    if (2 * nc * P > kMaxBatchMembers) return fail(ROFL_BAD_PARAM, "batch too large (split it)");      // the L / R problems of all chunks index gridDim.y
    std::vector<size_t> act;
    for (size_t i = 0; i < nc; i++) if (rcs[i] == ROFL_OK) act.push_back(i);
    if (act.empty()) { timing_end(C); return ROFL_OK; }
    size_t na = act.size();
    if (na != nc)      // close the gaps: the proof kernels index chunks densely
        for (size_t k = 0; k < na; k++) if (act[k] != k) {
            HIPCHK(hipMemcpyAsync(vshift + k * dp, vshift + act[k] * dp, 8 * dp, hipMemcpyDeviceToDevice, C.stream));
            HIPCHK(hipMemcpyAsync(d_blind_buf + k * dp, d_blind_buf + act[k] * dp, 32 * dp, hipMemcpyDeviceToDevice, C.stream));
        }
    // explicit nonce streams go to the device once
    std::vector<ChunkNonce> cn(na * P);
    { const u64 per = (u64)chunk * (2 * prove_range + 4);      // nonces of one chunk; a run reads scalars [chunk_first * per, (chunk_first + P) * per) of the client's stream
      const size_t run_bytes = (size_t)(P * per) * 64, run_off = (size_t)(chunk_first * per) * 64;
      size_t tot = 0; for (size_t k = 0; k < na; k++) if (nonces[act[k]].mode == 0) tot += run_bytes;
      uint8_t *sb = tot ? C.stream_buf.as<uint8_t>(tot + 64) : nullptr; size_t off = 0;
      for (size_t k = 0; k < na; k++) {
          const rofl_nonce_t &nn = nonces[act[k]];
          ChunkNonce base{}; base.mode = nn.mode;
          if (nn.mode == 1) memcpy(base.seed.w, nn.seed, 32);
          else {      // only the run's part of the stream goes up; the kernel indexes the stream by the client's nonce index, so the base address is moved back by the part that stayed behind (never dereferenced there)
              C.up(sb + off, nn.stream + run_off, run_bytes, C.stream);
              base.d_stream = reinterpret_cast<const uint8_t *>(reinterpret_cast<uintptr_t>(sb + off) - run_off); base.stream_scalars = (chunk_first + P) * per; off += run_bytes; }
          for (size_t c = 0; c < P; c++) { cn[k * P + c] = base; cn[k * P + c].base = (chunk_first + c) * per; }
      } }
    // V_j and un-shifted commitments C_j = V_j - 2^(range-1) B   (range_proof_vec/mod.rs:96-99)
    sc negoff = sc_neg(sc_from_u64(1ULL << (prove_range - 1)));
    niels h_shift = h51::to_niels32(h_fixed_mul(C.ht.B5, negoff));
    niels *d_shift = C.tmp_in.as<niels>(1);
    uint8_t *Vb = C.Vbytes.as<uint8_t>(na * dp * 32), *Cb = C.Cbytes.as<uint8_t>(na * dp * 32);
    // The commitment kernel is a latency chain on d threads (two fixed-base multiplications and two encodings each: 0.4 ms on a tenth
    // of the chip) and nothing in the prover reads its output on the device: it runs on the side stream, beside the nonce expansion and the
    // A / S launches.  The host needs the V bytes when it hashes them into the transcripts (ev_v), the caller's commitment arrays when the
    // call returns.
    if (!C.stream2) HIPCHK(hipStreamCreateWithFlags(&C.stream2, hipStreamNonBlocking));
    if (!C.ev_v) { HIPCHK(hipEventCreateWithFlags(&C.ev_v, hipEventDisableTiming)); HIPCHK(hipEventCreateWithFlags(&C.ev_fork, hipEventDisableTiming)); }
    GensPin gens_pin = get_gens(C, prove_range, chunk);           // may throw (allocation): before anything is queued on the side stream
    struct Join { hipStream_t s; ~Join() { (void)hipStreamSynchronize(s); } } join{C.stream2};      // also on the error paths: the side stream copies into caller memory
    HIPCHK(hipEventRecord(C.ev_fork, C.stream));                  // inputs quantised (and compacted)
    HIPCHK(hipStreamWaitEvent(C.stream2, C.ev_fork, 0));
    HIPCHK(hipMemcpyAsync(d_shift, &h_shift, sizeof(niels), hipMemcpyHostToDevice, C.stream2));
    { KSpan ks(C.tm, C.stream2, ROFL_TK_CODEC, (uint64_t)na * dp * ((8 + 1 + 32) * 7 + 2 * 265), (uint64_t)na * dp * (8 + 32 + 64));      // 8 + carry + 32 radix-256 windows, two encodings
    ROFL_LAUNCH(k_commit, grid1(na * dp), dim3(TPB), 0, C.stream2, (u32)(na * dp), vshift, (const sc *)nullptr, d_blind_buf, C.d_tabB8, C.d_tabBb8, d_shift, Vb, Cb, (u32)d, (u32)dp); }
    uint8_t *hV = C.h_V.as<uint8_t>(na * dp * 32);
    HIPCHK(hipMemcpyAsync(hV, Vb, na * dp * 32, hipMemcpyDeviceToHost, C.stream2));
    HIPCHK(hipEventRecord(C.ev_v, C.stream2));
    for (size_t k = 0; k < na && d; k++) C.down(commits_out[act[k]], Cb + k * dp * 32, d * 32, C.stream2);
    std::vector<uint8_t *> pout(na * P);
    for (size_t k = 0; k < na; k++) for (size_t c = 0; c < P; c++) pout[k * P + c] = proofs_out[act[k]] + c * plen;
    prove_chunks(C, "RangeProof", na * P, prove_range, chunk, vshift, d_blind_buf, cn, hV, pout.data(), C.ev_v);
    HIPCHK(hipStreamSynchronize(C.stream2));
    timing_end(C);
    return ROFL_OK;
}

// The reference zips `commits.chunks(len / proofs.len())` with the proofs (range_proof_vec/mod.rs:169-176): when the proof count does
// not divide the padded length the zip silently drops the tail, i.e. commitments that NO proof covers are accepted (3 proofs for
// 8 commitments check 6 of them; dp/2 + 1 proofs check half).  The proof count comes off the wire, so that is a soundness hole, not
// a format quirk: here a set whose proofs do not cover every chunk exactly is reported as "does not verify" (ok = 0, return code 0).
// rofl_set_option("verify_zip_truncate", 1) restores the reference's behaviour bit for bit (byte-level comparisons).
// `single`: the call is rofl_verify_rangeproof (a malformed set is the call's FormatError); batch calls -- also their one-client shards
// when a batch is spread over several devices -- give every client its own verdict.  gid[i] (nullptr: i) = client i's index in the
// caller's batch: it keys the client's random weights, so that a shard draws what the whole batch would have drawn for it.
// cstride: distance in bytes between two commitments of a client's array (32 = packed; 64 / 96 = the L component of ElGamal pairs /
// SquareRandProofCommitments as they arrive on the wire, params.rs:197, 215: `enc_values.iter().map(|x| x.c.L)`).
int verify_impl(Ctx &C, size_t n_clients, const uint8_t *const *proofs, size_t proof_len, size_t n_proofs, const uint8_t *const *commits,
                size_t d, size_t prove_range, unsigned fp_bits, unsigned fp_frac, const uint8_t seed[32], int *ok_out, bool single,
                const size_t *gid = nullptr, size_t cstride = 32, size_t chunk_first = 0, size_t chunk_count = 0, const RoundSrc *rs = nullptr) {
    // rs: the commitments are the first d cached L of the round's clients (`commits` is not read); a client without proofs (proofs[i] null)
    // is left out: it takes part as a malformed member and gets ok = 0.
    // [chunk_first, chunk_first + chunk_count) (count 0: all): the proofs of every client that THIS call checks -- the reference verifies a
    // client's proofs independently of each other and ANDs the bits (range_proof_vec/mod.rs:168-181), so a device or a rank can take any run
    // of them.  n_proofs and d stay the client's (they fix the chunk length); proofs[i] points at the run's first proof, commits[i] at the
    // run's first commitment (element chunk_first * m of the client's array).
    for (size_t i = 0; i < n_clients; i++) ok_out[i] = 0;
    if (!valid_fp(fp_bits, fp_frac) || d == 0 || n_proofs == 0 || prove_range == 0 || prove_range > fp_bits || n_clients == 0 || cstride < 32)
        return fail(ROFL_BAD_PARAM, "bad parameter (the reference panics here)");
    const size_t d_all = d;
    size_t dp = next_pow2(d);
    size_t chunk = dp / n_proofs;
    if (chunk == 0) return fail(ROFL_BAD_PARAM, "more proofs than padded commitments (the reference panics in chunks(0))");
    size_t n_chunks = (dp + chunk - 1) / chunk;
    size_t nv = std::min(n_proofs, n_chunks);            // zip truncates (range_proof_vec/mod.rs:173-176)
    const bool zip_truncate = opts().zip_truncate.load() != 0;      // rofl_set_option("verify_zip_truncate")
    if (n_proofs * chunk != dp) {
        if (!zip_truncate) { g_err = "proof count does not cover the padded commitment vector: not verified"; return ROFL_OK; }
        if (dp % chunk) return fail(ROFL_BAD_PARAM, "ragged chunks are not supported");
    }
    if (chunk_count) {      // a run of the client's verified chunks: from here on d, dp, nv describe the run
        if (chunk_first >= nv || chunk_count > nv - chunk_first) return fail(ROFL_BAD_PARAM, "chunk range outside the client's proofs");
        const size_t el0 = chunk_first * chunk;
        nv = chunk_count; dp = nv * chunk;
        d = el0 >= d_all ? 0 : std::min(d_all - el0, dp);
    } else chunk_first = 0;
    // Everything below allocates per (prove_range, chunk): check the proofs' own shape against it first (RangeProof::from_bytes,
    // then the N == 2^lg test of verify_multiple), so that a forged proof count cannot make the device build tables.
    if (proof_len % 32 != 0 || proof_len < 7 * 32) return fail(ROFL_FORMAT_ERROR, "FormatError: proof length");
    size_t ne = (proof_len - 7 * 32) / 32;
    if (ne < 2 || (ne - 2) % 2 != 0 || (ne - 2) / 2 >= 32) return fail(ROFL_FORMAT_ERROR, "FormatError: proof length");
    size_t lg = (ne - 2) / 2;
    size_t P = n_clients * nv;
    // every (client, chunk) pair is a row of gridDim.y in the verifier's kernels (and, with the closer look of verify_batch = 2, a few padding rows more)
    if (P + 2 * nv * (size_t)std::ceil(std::sqrt((double)n_clients)) > kMaxBatchMembers) return fail(ROFL_BAD_PARAM, "batch too large (split it)");
    std::vector<uint8_t> pf(P * proof_len);
    for (size_t i = 0; i < n_clients; i++) {      // host or device memory; caller memory is not handed to the HIP runtime
        if (rs && !proofs[i]) continue;      // (zero bytes: a proof that fails on its own)
        if (is_device_ptr(proofs[i])) HIPCHK(hipMemcpy(&pf[i * nv * proof_len], proofs[i], nv * proof_len, hipMemcpyDeviceToHost));
        else memcpy(&pf[i * nv * proof_len], proofs[i], nv * proof_len);
    }
    // RangeProof::from_bytes rejects non-canonical scalars.  A single set: FormatError, as the reference (the caller cannot even build
    // its Vec<RangeProof>).  In a batch every client has its own verdict (server.rs:656-687 verifies each client on its own): the
    // offender gets ok = 0 and the others are still verified -- its scalars are zeroed in the local copy so that the shared launch
    // sequence stays well-formed (its check then fails on its own; clients never share a check).
    std::vector<char> bad_format(n_clients, 0);
    if (rs) for (size_t i = 0; i < n_clients; i++) bad_format[i] = !proofs[i];
    for (size_t q = 0; q < P; q++) {
        uint8_t *pb = &pf[q * proof_len];
        const size_t offs[5] = {128, 160, 192, 7 * 32 + 64 * lg, 7 * 32 + 64 * lg + 32};
        for (size_t o : offs)
            if (!sc_is_canonical_bytes(pb + o)) {
                if (single) return fail(ROFL_FORMAT_ERROR, "proof rejected before verification (format / bitsize)");
                bad_format[q / nv] = 1; memset(pb + o, 0, 32);
            }
    }
    if (!(prove_range == 8 || prove_range == 16 || prove_range == 32 || prove_range == 64)) return fail(ROFL_INVALID_BITSIZE, "proof rejected before verification (format / bitsize)");
    if (prove_range * chunk != ((size_t)1 << lg)) return ROFL_OK;      // VerificationError for every chunk -> Ok(false)
    C.init();
    C.batch_mode = n_clients > 1;
    timing_begin(C);
    // shift up by 2^(range-1) B, pad with identity, compress (:155-167)
    niels h_shift = h51::to_niels32(h_fixed_mul(C.ht.B5, sc_from_u64(1ULL << (prove_range - 1))));
    niels *d_shift = C.tmp_out.as<niels>(1);
    HIPCHK(hipMemcpyAsync(d_shift, &h_shift, sizeof(niels), hipMemcpyHostToDevice, C.stream));
    size_t tot = n_clients * dp;
    uint8_t *d_in = rs ? nullptr : C.Cbytes.as<uint8_t>(tot * 32);      // (a round brings no commitment bytes in)
    uint8_t *d_enc = C.Vbytes.as<uint8_t>(tot * 32);
    niels *d_vn = C.gbuf[0].as<niels>(tot);
    u32 *status = C.status.as<u32>(n_clients + 4);       // one status word per client: an undecodable commitment fails that client only
    HIPCHK(hipMemsetAsync(status, 0, 4 * (n_clients + 4), C.stream));
    uint8_t *hV = C.h_V.as<uint8_t>(tot * 32);            // pinned: the encodings of the shifted commitments, for the transcripts
    u32 *h_st = C.h_misc.as<u32>(n_clients + 4);
    // Commitments in, decoded, shifted encodings out -- in groups of a few clients: the host hashes the encodings of group g into the
    // transcripts (verify_chunks) while the device decodes group g + 1.  Host memory is staged (one parallel copy per group on the pool);
    // device pointers go straight in.
    const size_t GC = std::max<size_t>(1, std::min<size_t>(n_clients, ((size_t)1 << 19) / dp));      // ~2^19 commitments per group
    std::vector<VerifyReady> ready;
    bool used_up = false;
    struct JoinUp { Ctx &c; bool &used; ~JoinUp() { if (used && c.stream_up) (void)hipStreamSynchronize(c.stream_up); } } join_up{C, used_up};      // nothing of the upload stream outlives the call
    bool all_host = true; for (size_t i = 0; i < n_clients && !rs; i++) all_host &= !is_device_ptr(commits[i]);
    if (rs) for (size_t i = 0; i < n_clients; i++) h_st[i] = rs->bad[3 * i] < d ? 4u : 0u;      // an undecodable L fails the leg only where the leg reads it
    for (size_t i0 = 0; i0 < n_clients; i0 += GC) {
        const size_t gc = std::min(GC, n_clients - i0);
        if (rs || d == 0) {      // the round's cache, or a run of padding chunks: nothing to bring in (the decode kernel writes identities)
        } else if (all_host && (d * 32 >= Stage::kMin || cstride != 32)) {
            uint8_t *st = (uint8_t *)C.stg.alloc(gc * d * 32);
            const size_t slices = std::max<size_t>(1, (d * 32) >> 18);      // ~256 KB per task
            C.pool->run(gc * slices, [&](size_t t) { size_t i = t / slices, k = t % slices;
                                                     if (cstride == 32) { size_t lo = d * 32 * k / slices, hi = d * 32 * (k + 1) / slices; stage_copy(st + i * d * 32 + lo, commits[i0 + i] + lo, hi - lo); }
                                                     else { const uint8_t *src = commits[i0 + i]; uint8_t *dst = st + i * d * 32;      // gather: the staging copy is also the packing
                                                            for (size_t e = d * k / slices, e1 = d * (k + 1) / slices; e < e1; e++) memcpy(dst + e * 32, src + e * cstride, 32); } });
            if (n_clients > GC) {
                // several groups: the upload of group g + 1 runs beside the decoding of group g (a stream of its own; the decode kernel waits for its group's bytes)
                if (!C.stream_up) HIPCHK(hipStreamCreateWithFlags(&C.stream_up, hipStreamNonBlocking));
                if (i0 == 0) { HIPCHK(hipEventRecord(C.pool_event(0), C.stream)); HIPCHK(hipStreamWaitEvent(C.stream_up, C.pool_event(0), 0)); }      // (after the shift upload and the status memset)
                HIPCHK(hipMemcpy2DAsync(d_in + i0 * dp * 32, dp * 32, st, d * 32, d * 32, gc, hipMemcpyHostToDevice, C.stream_up));
                HIPCHK(hipEventRecord(C.pool_event(1 + (ready.size() & 1)), C.stream_up));
                HIPCHK(hipStreamWaitEvent(C.stream, C.pool_event(1 + (ready.size() & 1)), 0));
                used_up = true;
            } else      // one group (a single client: the latency case): no second stream, no events
                HIPCHK(hipMemcpy2DAsync(d_in + i0 * dp * 32, dp * 32, st, d * 32, d * 32, gc, hipMemcpyHostToDevice, C.stream));
        } else
            for (size_t i = i0; i < i0 + gc; i++) {
                if (cstride == 32) C.up(d_in + i * dp * 32, commits[i], d * 32, C.stream);
                else if (is_device_ptr(commits[i])) HIPCHK(hipMemcpy2DAsync(d_in + i * dp * 32, 32, commits[i], cstride, 32, d, hipMemcpyDeviceToDevice, C.stream));
                else { uint8_t *st = (uint8_t *)C.stg.alloc(d * 32); for (size_t e = 0; e < d; e++) memcpy(st + e * 32, commits[i] + e * cstride, 32);
                       HIPCHK(hipMemcpyAsync(d_in + i * dp * 32, st, d * 32, hipMemcpyHostToDevice, C.stream)); }
            }
        if (rs) { KSpan ks(C.tm, C.stream, ROFL_TK_CODEC, (uint64_t)gc * d * (265 + 14), (uint64_t)gc * d * (96 + 96 + 32));      // no decode: shift + encode from the cached point
          ROFL_LAUNCH(k_round_shift_encode, grid1(dp, (u32)gc), dim3(TPB), 0, C.stream, (u32)dp, (u32)d, (const niels *)(rs->pts + i0 * 2 * rs->npts * rs->d), 2 * rs->npts * rs->d,
                      (const niels *)d_shift, d_vn + i0 * dp, d_enc + i0 * dp * 32); }
        else { KSpan ks(C.tm, C.stream, ROFL_TK_CODEC, (uint64_t)gc * d * (2 * 265 + 7), (uint64_t)gc * d * 64);
          count_decodes(gc * d);
          ROFL_LAUNCH(k_decode, grid1(dp, (u32)gc), dim3(TPB), 0, C.stream, (u32)dp, (u32)d, d_in + i0 * dp * 32, d_shift, d_vn + i0 * dp, d_enc + i0 * dp * 32, status + i0); }
        HIPCHK(hipMemcpyAsync(hV + i0 * dp * 32, d_enc + i0 * dp * 32, gc * dp * 32, hipMemcpyDeviceToHost, C.stream));
        if (!rs) HIPCHK(hipMemcpyAsync(h_st + i0, status + i0, 4 * gc, hipMemcpyDeviceToHost, C.stream));
        ready.push_back(VerifyReady{(i0 + gc) * nv, C.pool_event(3 + ready.size())});      // (events 0..2 of the call: the upload stream's)
        HIPCHK(hipEventRecord(ready.back().ev, C.stream));
    }
    // flatten (client, chunk) -> problem list.  A client's verified chunks are a prefix of its dp commitments: when the proofs cover
    // everything (the normal case) the per-client arrays ARE the per-proof arrays; otherwise one strided copy each
    std::vector<u64> cidx(P);
    for (size_t i = 0; i < n_clients; i++) for (size_t c = 0; c < nv; c++) cidx[i * nv + c] = chunk_first + c;      // the chunk's index in its client: keys its random weights
    const uint8_t *Vh = hV; const niels *d_vn2 = d_vn;
    std::vector<uint8_t> Vh_own;
    if (nv * chunk != dp) {
        C.sync();
        Vh_own.resize(P * chunk * 32);
        for (size_t i = 0; i < n_clients; i++) memcpy(&Vh_own[i * nv * chunk * 32], hV + i * dp * 32, nv * chunk * 32);
        Vh = Vh_own.data();
        niels *cp2 = C.gbuf[1].as<niels>(P * chunk);
        HIPCHK(hipMemcpy2DAsync(cp2, nv * chunk * sizeof(niels), d_vn, dp * sizeof(niels), nv * chunk * sizeof(niels), n_clients, hipMemcpyDeviceToDevice, C.stream));
        d_vn2 = cp2;
    }
    std::vector<int> okc(P);
    GensPin gens_pin = get_gens(C, prove_range, chunk, GENS_VERIFY);      // generators + window slices; a verifier never builds the prover's fold table
    const int vbatch = opts().verify_batch.load();            // rofl_set_option("verify_batch")
    size_t grp = vbatch ? nv : 1;
    // verify_batch = 2: one check for the whole batch, a closer look only when it fails (verify_chunks); clients already known to be
    // malformed are kept out of the shared checks
    const bool hier = vbatch == 2 && n_clients > 1;
    std::vector<u64> ridx(P); std::vector<char> skip(P, 0);
    for (size_t q = 0; q < P; q++) { size_t i = q / nv; ridx[q] = ((u64)(gid ? gid[i] : i) << 24) | cidx[q]; skip[q] = hier && bad_format[i]; }
    // all (client, chunk) pairs in one pass; a client's chunks form one batch of the random-weighted check
    sc v_shift = sc_from_u64(1ULL << (prove_range - 1));
    std::vector<u64> v_real(P);
    for (size_t q = 0; q < P; q++) { size_t lo = cidx[q] * chunk; v_real[q] = lo >= d_all ? 0 : std::min(chunk, d_all - lo); }
    // (an undecodable commitment is known only when its group has been decoded: verify_chunks asks for the client's status word then)
    VerifyInputs vin{&ready, h_st, nv};
    int rc = verify_chunks(C, "RangeProof", prove_range, P, prove_range, chunk, pf.data(), proof_len, Vh, d_vn2, seed, cidx.data(), okc.data(), grp, &v_shift, v_real.data(),
                           n_clients > 1 ? ridx.data() : nullptr, hier, skip.data(), &vin);
    C.sync();      // (a no-op after the checks; verify_chunks may have left before its first wait)
    std::vector<char> bad_commit(n_clients, 0);
    for (size_t i = 0; i < n_clients; i++) bad_commit[i] = (h_st[i] & 4u) != 0;
    // a single set with an invalid encoding: the reference cannot even build its Vec<RistrettoPoint> (decompress fails) -> FormatError;
    // in a batch the other clients are still verified and the offender gets ok = 0
    if (single && bad_commit[0]) { timing_end(C); return fail(ROFL_FORMAT_ERROR, "commitment is not a valid Ristretto encoding"); }
    timing_end(C);
    if (rc) return fail(rc, "proof rejected before verification (format / bitsize)");
    for (size_t i = 0; i < n_clients; i++) { int r = (bad_commit[i] || bad_format[i]) ? 0 : 1; for (size_t c = 0; c < nv; c++) r &= okc[i * nv + c]; ok_out[i] = r; }
    return ROFL_OK;
}

// One persistent worker thread per logical device for the sharded batch calls.  A worker serves one job at a time (concurrent sharded calls
// queue on the device's worker: the device is the shared resource anyway); jobs never throw (their body is guarded()).
class ShardWorkers {
    struct W { std::thread th; std::mutex mu; std::condition_variable cv; std::deque<std::pair<uint64_t, std::function<void()>>> q; uint64_t next_id = 1, done_id = 0; bool stop = false; };
    std::mutex mu; std::map<int, std::unique_ptr<W>> ws;
public:
    struct Ticket { bool ok = false; int dev = 0; uint64_t id = 0; };
    // Up to kPerDevice workers per device: the three legs of ONE L2 update (range proof by chunks, square proofs by elements, their verifiers)
    // split over the devices at the same time, and a leg's share of a device must not wait behind another leg's.  A job goes to an idle
    // worker of its device when there is one (created on demand), otherwise to the one with the shortest queue.
    static constexpr int kPerDevice = 3;
    Ticket submit(int dev, std::function<void()> job) {
        W *w = nullptr; int key = dev * kPerDevice;
        {   std::lock_guard<std::mutex> lk(mu);
            size_t best_load = ~(size_t)0;
            for (int sl = 0; sl < kPerDevice; sl++) {
                auto f = ws.find(dev * kPerDevice + sl);
                if (f == ws.end()) { if (best_load) { key = dev * kPerDevice + sl; best_load = 0; } break; }      // a worker that does not exist yet is idle
                size_t load; { std::lock_guard<std::mutex> lk2(f->second->mu); load = (size_t)(f->second->next_id - 1 - f->second->done_id); }
                if (load < best_load) { best_load = load; key = dev * kPerDevice + sl; }
                if (load == 0) break;
            }
            auto it = ws.find(key);
            if (it == ws.end()) {
                std::unique_ptr<W> nw(new W());
                W *raw = nw.get();
                try {
                    raw->th = std::thread([raw] {
                        for (;;) {
                            std::pair<uint64_t, std::function<void()>> j;
                            { std::unique_lock<std::mutex> lk(raw->mu); raw->cv.wait(lk, [&] { return raw->stop || !raw->q.empty(); }); if (raw->q.empty()) return; j = std::move(raw->q.front()); raw->q.pop_front(); }
                            j.second();
                            { std::lock_guard<std::mutex> lk(raw->mu); raw->done_id = j.first; }
                            raw->cv.notify_all();
                        }
                    });
                } catch (...) { return Ticket{}; }      // EAGAIN / bad_alloc: reported by the caller as an error code
                it = ws.emplace(key, std::move(nw)).first;
            }
            w = it->second.get();
        }
        Ticket t; t.ok = true; t.dev = key;
        { std::lock_guard<std::mutex> lk(w->mu); t.id = w->next_id++; w->q.emplace_back(t.id, std::move(job)); }
        w->cv.notify_all();
        return t;
    }
    void wait(const Ticket &t) {
        W *w; { std::lock_guard<std::mutex> lk(mu); w = ws[t.dev].get(); }
        std::unique_lock<std::mutex> lk(w->mu); w->cv.wait(lk, [&] { return w->done_id >= t.id; });
    }
    ~ShardWorkers() { for (auto &kv : ws) { { std::lock_guard<std::mutex> lk(kv.second->mu); kv.second->stop = true; } kv.second->cv.notify_all(); if (kv.second->th.joinable()) kv.second->th.join(); } }
};
ShardWorkers &shard_workers() { static ShardWorkers s; return s; }

// The devices a call spreads its work over: rofl_set_option("devices", mask).  Empty = the calling thread's device.
std::vector<int> batch_devices() {
    std::vector<int> v; long m = opts().devices.load();
    for (int i = 0; i < kMaxDevices && m; i++, m >>= 1) if (m & 1) v.push_back(i);
    return v;
}
// A call that is not dealt to several devices runs on the listed one: a one-client call when the mask names exactly one device, a batch
// call (`first_of_many`) on the first of however many it names.  Otherwise the thread stays where it is.
struct ListedDevice : DeviceBinding {
    explicit ListedDevice(const std::vector<int> &devs, bool first_of_many = false) : DeviceBinding(devs.size() == 1 || (first_of_many && !devs.empty()) ? devs[0] : t_device) {}
};
// run(k) for k < nd, each on the worker of devs[k] (k = 0 on the calling thread), bound to its device; rcs[k] / errs[k] = what it returned.
// Results land in the caller's arrays, in host memory -- in one process there is no collective to run.
// The return value is non-zero only when a worker thread could not be started.
template <class F> int run_on_devices(const std::vector<int> &devs, size_t nd, std::vector<int> &rcs, std::vector<std::string> &errs, F run) {
    rcs.assign(nd, ROFL_OK); errs.assign(nd, std::string());
    auto body = [&](size_t k) { DeviceBinding bind(devs[k]); rcs[k] = guarded([&]() -> int { return run(k); }); if (rcs[k]) errs[k] = g_err; };
    // one persistent worker per device (ShardWorkers): no thread is created on the call path, and a thread that cannot be created at
    // start-up is an error code, not std::terminate from a vector of joinable threads
    ShardWorkers &sw = shard_workers();
    std::vector<ShardWorkers::Ticket> tickets;
    for (size_t k = 1; k < nd; k++) {
        ShardWorkers::Ticket t = sw.submit(devs[k], [&body, k] { body(k); });
        if (!t.ok) { for (auto &q : tickets) sw.wait(q); return fail(ROFL_HIP_ERROR, "could not start the worker thread of a device"); }
        tickets.push_back(t);
    }
    body(0);
    for (auto &t : tickets) sw.wait(t);
    return ROFL_OK;
}
// the first failing run or share in device order is the call's return code and rofl_last_error text
int first_failure(const std::vector<int> &rcs, const std::vector<std::string> &errs) {
    for (size_t k = 0; k < rcs.size(); k++) if (rcs[k]) return fail(rcs[k], errs[k]);
    return ROFL_OK;
}

// What the body of a batch entry sees of the call's clients: all of them, as the caller passed them (idx == nullptr: every array is handed
// through and every result is written in place -- nothing is allocated, nothing is copied), or the share of one device.
struct Share {
    size_t n; const std::vector<size_t> *idx;      // idx: the members' positions in the caller's arrays
    size_t size() const { return n; }
    bool whole() const { return !idx; }
    const size_t *positions() const { return idx ? idx->data() : nullptr; }
    // a per-client array of the caller as the implementation reads it: the array itself, or the members' entries gathered (null entries for
    // an array that is null or, `live` false, not read at this shape)
    template <class T> struct In { const T *src; std::vector<T> own; const T *data() const { return own.empty() ? src : own.data(); } };
    template <class T> In<T> view(const T *a, bool live = true) const {
        In<T> v{a, {}};
        if (idx) { v.own.resize(n); if (a && live) for (size_t j = 0; j < n; j++) v.own[j] = a[(*idx)[j]]; }
        return v;
    }
    // per-member results, `row` elements each: the caller's array itself, or zeroed rows of the share's own that scatter() copies to the
    // members' positions (a null array stays null)
    template <class T> struct Out { T *dst; size_t row; std::vector<T> own; T *data() { return own.empty() ? dst : own.data(); } };
    template <class T> Out<T> out(T *dst, size_t row = 1) const { return Out<T>{dst, row, std::vector<T>(idx && dst ? n * row : 0)}; }
    template <class T, class Keep> void scatter(const Out<T> &o, Keep keep) const {
        if (!o.own.empty()) for (size_t j = 0; j < n; j++) if (keep(j)) memcpy(o.dst + o.row * (*idx)[j], &o.own[o.row * j], o.row * sizeof(T));
    }
    template <class T> void scatter(const Out<T> &o) const { scatter(o, [](size_t) { return true; }); }
};
// THE policy of rofl_set_option("devices", mask) for a batch entry; body(share) is the entry's implementation call, written once.
// No listed device, or fewer than two clients: one guarded call of the body on all clients, on the first listed device if there is one.
// Otherwise the clients are dealt round-robin, client i to share i % nd, one persistent worker per device (share 0 on the calling thread),
// each running the ordinary single-device path on its share; the first failing share in device order is the call's error.
// `verdicts` (the verifiers' ok_out; nullptr for the creators, whose rc_out is not touched) is zeroed before the clients are dealt.
template <class F> int over_devices(size_t n_clients, int *verdicts, F body) {
    const std::vector<int> devs = batch_devices();
    if (devs.empty() || n_clients < 2) return guarded([&]() -> int { ListedDevice bind(devs, true); return body(Share{n_clients, nullptr}); });
    if (verdicts) for (size_t i = 0; i < n_clients; i++) verdicts[i] = 0;
    return guarded([&]() -> int {
        const size_t nd = std::min(devs.size(), n_clients);
        std::vector<std::vector<size_t>> share(nd);
        for (size_t i = 0; i < n_clients; i++) share[i % nd].push_back(i);
        std::vector<int> rcs; std::vector<std::string> errs;
        if (int rc = run_on_devices(devs, nd, rcs, errs, [&](size_t k) -> int { return body(Share{share[k].size(), &share[k]}); })) return rc;
        return first_failure(rcs, errs);
    });
}

// ONE client over several devices ("cfg 2/3 at > 1 GPU -> chunks over ranks").  The reference proves and verifies a client's
// chunks in parallel on its rayon pool (range_proof_vec/mod.rs:54-78, 168-181: every chunk is its own Bulletproof with its own transcript);
// here device k takes the k-th contiguous run of the P chunks -- a run's commitments are one span of the caller's array, the cost of a
// chunk does not depend on its data (padding chunks are proved like any other), so contiguous runs balance exactly like a round-robin deal.
// No collective: proofs and commitments land in the caller's host arrays.  The bytes are those of the unsplit call (the nonce index space is
// the client's).
// (first, count) of the contiguous runs that n units -- a range proof's chunks, a Sigma vector's elements -- are cut into for nd devices; no
// run is shorter than min_len (1 for chunks; 2048 for elements: a shorter run is not worth a device)
typedef std::vector<std::pair<size_t, size_t>> Runs;
Runs split_runs(size_t n, size_t nd, size_t min_len) {
    Runs r;
    nd = std::max<size_t>(1, std::min(nd, n / min_len));
    for (size_t k = 0; k < nd; k++) { size_t a = k * n / nd, b = (k + 1) * n / nd; if (b > a) r.emplace_back(a, b - a); }
    return r;
}
// The runs of ONE client's proofs verified on the listed devices, run(first, count, &ok) each, and the call's one verdict: a failing run is
// the call's error (a malformed set is the call's FormatError, whichever run met it), otherwise the AND of the runs' verdicts.
template <class F> int verify_runs(const std::vector<int> &devs, const Runs &runs, int *ok_out, F run) {
    std::vector<int> rcs, oks(runs.size(), 0); std::vector<std::string> errs;
    if (int rc = run_on_devices(devs, runs.size(), rcs, errs, [&](size_t k) -> int { return run(runs[k].first, runs[k].second, &oks[k]); })) return rc;
    *ok_out = 0;
    if (int rc = first_failure(rcs, errs)) return rc;
    int ok = 1; for (int o : oks) ok &= o;
    *ok_out = ok;
    return ROFL_OK;
}
int create_split(const std::vector<int> &devs, const float *values, size_t d, const uint8_t *blind, size_t prove_range, size_t n_partition, unsigned fp_bits,
                 unsigned fp_frac, const rofl_nonce_t *nonce, uint8_t *proofs_out, size_t *plen_out, size_t *np_out, uint8_t *commits_out) {
    const size_t dp = next_pow2(d), nch = std::min(dp, n_partition), chunk = dp / nch, P = (dp + chunk - 1) / chunk;
    const size_t plen = 32 * (9 + 2 * (size_t)lg2u(prove_range * chunk));      // (every run reports the same; needed here to place the runs' proofs)
    auto runs = split_runs(P, devs.size(), 1);
    std::vector<int> rcs, rc1(runs.size(), ROFL_OK); std::vector<std::string> errs;
    if (int rc = run_on_devices(devs, runs.size(), rcs, errs, [&](size_t k) -> int {
            LaneLock lane_lock = acquire_lane(); Ctx &C = *lane_lock.c;
            uint8_t *po = proofs_out + runs[k].first * plen, *co = commits_out + std::min(runs[k].first * chunk, d) * 32;
            size_t pl = 0, np = 0;
            return create_impl(C, 1, &values, d, &blind, prove_range, n_partition, fp_bits, fp_frac, nonce, &po, &pl, &np, &co, &rc1[k], false, runs[k].first, runs[k].second); }))
        return rc;
    // the outcome of the unsplit call, in the reference's order of checks: parameters, the range check over ALL values (:27-29), the
    // conversion's panic, then the upstream errors
    auto any = [&](const std::vector<int> &v, int code) { return std::find(v.begin(), v.end(), code) != v.end(); };
    if (any(rcs, ROFL_BAD_PARAM)) return fail(ROFL_BAD_PARAM, "bad parameter (the reference panics here)");
    for (size_t k = 0; k < rcs.size(); k++) if (rcs[k] >= ROFL_HIP_ERROR || rcs[k] == ROFL_COMM_ERROR) return fail(rcs[k], errs[k]);
    if (any(rc1, ROFL_VALUE_OUT_OF_RANGE)) return fail(ROFL_VALUE_OUT_OF_RANGE, "ValueOutOfRangeError");
    if (any(rc1, ROFL_NON_FINITE)) return fail(ROFL_NON_FINITE, "non-finite value (the reference panics in fixed::saturating_from_float)");
    if (int rc = first_failure(rcs, errs)) return rc;
    if (any(rc1, ROFL_NONCE_SHORT)) return fail(ROFL_NONCE_SHORT, "nonce stream too short");
    *plen_out = plen; *np_out = P;
    return ROFL_OK;
}
int verify_split(const std::vector<int> &devs, const uint8_t *proofs, size_t proof_len, size_t n_proofs, const uint8_t *commits, size_t d, size_t prove_range,
                 unsigned fp_bits, unsigned fp_frac, const uint8_t seed[32], int *ok_out) {
    const size_t chunk = next_pow2(d) / n_proofs;
    return verify_runs(devs, split_runs(n_proofs, devs.size(), 1), ok_out, [&](size_t first, size_t count, int *ok) -> int {
        LaneLock lane_lock = acquire_lane(); Ctx &C = *lane_lock.c;
        const uint8_t *pp = proofs + first * proof_len, *cc = commits + std::min(first * chunk, d) * 32;
        return verify_impl(C, 1, &pp, proof_len, n_proofs, &cc, d, prove_range, fp_bits, fp_frac, seed, ok, true, nullptr, 32, first, count); });
}
// can this (d, n_proofs) set be split?  Only the regular case: the proofs cover the padded vector exactly
bool verify_splittable(size_t d, size_t n_proofs) { if (!d || n_proofs < 2) return false; size_t dp = next_pow2(d); return n_proofs <= dp && (dp / n_proofs) * n_proofs == dp; }

// ---------------------------------------------------------------- server-side aggregation on the device (rofl_acc_*; params.rs:74-147)
// An accumulator is a resident d x 2 array of extended points on the device of the thread that created it, named by a handle from this
// registry (never a pointer: an unknown or destroyed handle is a bad parameter, not a crash).  Calls on one accumulator are serialised by
// its lock; calls on different accumulators take different lanes of their device.
template <class T> struct Registry {
    std::mutex mu; std::map<uint64_t, std::shared_ptr<T>> m; uint64_t next = 1;
    std::shared_ptr<T> find(uint64_t h) { std::lock_guard<std::mutex> lk(mu); auto it = m.find(h); return it == m.end() ? nullptr : it->second; }
    uint64_t add(std::shared_ptr<T> p) { std::lock_guard<std::mutex> lk(mu); m.emplace(next, std::move(p)); return next++; }
    void erase(uint64_t h) { std::lock_guard<std::mutex> lk(mu); m.erase(h); }
};
struct Acc {
    int device = 0, init = 0; size_t d = 0;
    ge *sum = nullptr;      // [d][2]: L, R of every pair
    ge *work = nullptr;     // a copy of sum for an add that takes several passes (all or nothing: committed by the last fold); allocated on first use
    std::mutex mu; bool dead = false, released = false;      // dead: being or been destroyed (every call but destroy refuses it); released: memory freed
};
Registry<Acc> g_accs;
// the initial state of every pair and the R of the unity check: init 0 the identity, init 1 ElGamalPair::unity() = (B, B) (el_gamal.rs:83-88)
ge acc_init_point(int init) {
    if (!init) return ge_identity();
    static const uint8_t kB[32] = {0xe2, 0xf2, 0xae, 0x0a, 0x6a, 0xbc, 0x4e, 0x71, 0xa8, 0x84, 0xa9, 0x61, 0xc5, 0x00, 0x51, 0x5f,
                                   0x58, 0xe3, 0x0b, 0x6a, 0xa5, 0x82, 0xdd, 0x8d, 0xb6, 0xa6, 0x59, 0x45, 0xe0, 0x8d, 0x2d, 0x76};      // RISTRETTO_BASEPOINT_COMPRESSED
    ge b; ristretto_decode(b, kB); return b;
}
void acc_reset_launch(Ctx &C, Acc &A) {
    ROFL_LAUNCH(k_acc_fold, grid1(2 * A.d), dim3(TPB), 0, C.stream, (u32)(2 * A.d), 0u, (const ge *)nullptr, (const ge *)nullptr, acc_init_point(A.init), A.sum, (const u32 *)nullptr);
}
// An addition that takes several passes is all or nothing: its passes fold into a copy of the sum (acc_work_begin returns where they fold:
// the copy, or the sum itself for a single pass), and one last fold makes the copy the sum (acc_work_commit) -- unless bit 4 of the device
// word *status says that a decode of the call failed (nullptr: unconditionally).
ge *acc_work_begin(Ctx &C, Acc &A, bool multi) {
    if (!multi) return A.sum;
    if (!A.work) HIPCHK(hipMalloc(&A.work, sizeof(ge) * 2 * A.d));
    HIPCHK(hipMemcpyAsync(A.work, A.sum, sizeof(ge) * 2 * A.d, hipMemcpyDeviceToDevice, C.stream));
    return A.work;
}
void acc_work_commit(Ctx &C, Acc &A, const u32 *status) {
    ROFL_LAUNCH(k_acc_fold, grid1(2 * A.d), dim3(TPB), 0, C.stream, (u32)(2 * A.d), 0u, (const ge *)nullptr, (const ge *)A.work, acc_init_point(A.init), A.sum, status);
}
// Points are taken in tiles of kAccTile; the clients of a tile in groups of at most kAccGroupRecords records (the device copy of a group's
// records and the S x tile partials are the only scratch, whatever the round's size).  Per group: the records are packed into 64-byte
// pairs (host memory: one parallel gather into pinned staging + one upload; device memory: a strided device-to-device copy), one
// k_acc_decode_partial with S client slices, one k_acc_fold.  S is chosen so that the decode launch has ~4 waves per SIMD (256 CUs x 4
// SIMDs; the decode chain runs at one wave per SIMD).  A group holds at most 1.5 M records (96 MB of packed pairs): the two staging buffers
// of a call with several groups and its small per-group arrays stay inside the 256 MB of pinned memory a lane keeps between calls
// (Stage::finish, ROFL_STAGE_KEEP_MB) -- larger buffers would be released and pinned again by every add.
constexpr size_t kAccTile = (size_t)1 << 17, kAccGroupRecords = (size_t)3 << 19, kAccThreads = (size_t)256 * 4 * 4 * 64;
int acc_add_impl(Ctx &C, Acc &A, const std::vector<size_t> &cl, const std::vector<size_t> &nrec, const uint8_t *const *records, size_t stride) {
    const size_t d = A.d;
    size_t max_n = 0; for (size_t n : nrec) max_n = std::max(max_n, n);
    const size_t tile = std::min(max_n, kAccTile), ntiles = (max_n + tile - 1) / tile;
    size_t first_tile = 0; for (size_t n : nrec) first_tile += std::min(n, tile);
    const size_t rec_cap = std::min(first_tile, kAccGroupRecords);      // no group of any tile holds more records than the first tile's clients
    const size_t S_max = std::max<size_t>(1, std::min(cl.size(), (kAccThreads + 2 * tile - 1) / (2 * tile)));
    const bool multi = ntiles > 1 || first_tile > kAccGroupRecords;
    C.init();
    uint8_t *rec = C.tmp_in.as<uint8_t>(rec_cap * 64);
    ge *part = C.partial2.as<ge>(S_max * tile * 2);
    u64 *d_off = C.tmp_in2.as<u64>(cl.size()); u32 *d_cnt = C.tmp_out.as<u32>(cl.size());
    u32 *status = C.status.as<u32>(4);
    HIPCHK(hipMemsetAsync(status, 0, 16, C.stream));
    ge *tgt = acc_work_begin(C, A, multi);
    // (host work per call is O(clients): one pointer query per client here and, per group, one strided copy per device-resident client --
    //  ~1-2 us each, nothing at a round's 48 clients, about a second per add of 10^6 single-record clients)
    std::vector<char> on_dev(cl.size());
    for (size_t k = 0; k < cl.size(); k++) on_dev[k] = is_device_ptr(records[cl[k]]);
    const ge init = acc_init_point(A.init);
    uint8_t *stb[2] = {nullptr, nullptr}; size_t gi = 0;
    for (size_t t = 0; t < ntiles; t++) {
        const size_t j0 = t * tile;
        size_t k = 0;
        while (k < cl.size()) {
            // the next group: clients k.. that reach into this tile, up to kAccGroupRecords records
            std::vector<size_t> gk; std::vector<u64> off; std::vector<u32> cnt; size_t nr = 0, tn = 0;
            for (; k < cl.size(); k++) {
                if (nrec[k] <= j0) continue;
                size_t c = std::min(nrec[k] - j0, tile);
                if (nr + c > kAccGroupRecords && !gk.empty()) break;
                gk.push_back(k); off.push_back(nr); cnt.push_back((u32)c); nr += c; tn = std::max(tn, c);
            }
            if (gk.empty()) break;
            const size_t gc = gk.size();
            // host clients: gathered into pinned staging on the pool (the gather is the packing: the first 64 bytes of every record)
            bool any_host = false; for (size_t q : gk) any_host |= !on_dev[q];
            if (any_host) {
                // two staging buffers: the gather of group g + 1 runs while the device works on group g (a buffer is reused once its upload is done)
                const int b = (int)(gi & 1);
                if (!stb[b]) stb[b] = (uint8_t *)C.stg.alloc(rec_cap * 64);
                else C.wait_event(C.pool_event(b));
                uint8_t *st = stb[b];
                const size_t per = (size_t)1 << 12;      // records per task (256 KB)
                std::vector<std::pair<size_t, size_t>> tasks;      // (group member, first record)
                for (size_t g = 0; g < gc; g++) if (!on_dev[gk[g]]) for (size_t e = 0; e < cnt[g]; e += per) tasks.push_back({g, e});
                C.pool->run(tasks.size(), [&](size_t ti) {
                    const size_t g = tasks[ti].first, e0 = tasks[ti].second, e1 = std::min<size_t>(cnt[g], e0 + per);
                    const uint8_t *src = records[cl[gk[g]]] + (j0 + e0) * stride; uint8_t *dst = st + (off[g] + e0) * 64;
                    if (stride == 64) stage_copy(dst, src, (e1 - e0) * 64);
                    else for (size_t e = e0; e < e1; e++) memcpy(dst + (e - e0) * 64, src + (e - e0) * stride, 64);
                });
                HIPCHK(hipMemcpyAsync(rec, st, nr * 64, hipMemcpyHostToDevice, C.stream));
                HIPCHK(hipEventRecord(C.pool_event(b), C.stream));
            }
            gi++;
            for (size_t g = 0; g < gc; g++)      // device clients: after the upload, which carries no bytes of theirs
                if (on_dev[gk[g]]) HIPCHK(hipMemcpy2DAsync(rec + off[g] * 64, 64, records[cl[gk[g]]] + j0 * stride, stride, 64, cnt[g], hipMemcpyDeviceToDevice, C.stream));
            u64 *h_off = (u64 *)C.stg.alloc(gc * 8); u32 *h_cnt = (u32 *)C.stg.alloc(gc * 4);
            memcpy(h_off, off.data(), gc * 8); memcpy(h_cnt, cnt.data(), gc * 4);
            HIPCHK(hipMemcpyAsync(d_off, h_off, gc * 8, hipMemcpyHostToDevice, C.stream));
            HIPCHK(hipMemcpyAsync(d_cnt, h_cnt, gc * 4, hipMemcpyHostToDevice, C.stream));
            const size_t S = std::min(S_max, gc);
            count_decodes(2 * nr);
            ROFL_LAUNCH(k_acc_decode_partial, grid1(2 * tn * S), dim3(TPB), 0, C.stream, (u32)tn, (u32)S, (u32)gc, (const u64 *)d_off, (const u32 *)d_cnt, (const uint8_t *)rec, part, status);
            ROFL_LAUNCH(k_acc_fold, grid1(2 * tn), dim3(TPB), 0, C.stream, (u32)(2 * tn), (u32)S, (const ge *)part, (const ge *)(tgt + 2 * j0), init, tgt + 2 * j0, (const u32 *)status);
        }
    }
    if (multi) acc_work_commit(C, A, status);      // sum <- work, unless a decode of the call failed (the kernel reads the status word)
    u32 st = 0;
    HIPCHK(hipMemcpyAsync(&st, status, 4, hipMemcpyDeviceToHost, C.stream));
    C.sync();
    if (st & 4u) return fail(ROFL_FORMAT_ERROR, "FormatError: a record is not a valid Ristretto encoding (the accumulator is unchanged)");
    return ROFL_OK;
}

// ---------------------------------------------------------------- a round resident on the device (rofl_round_*; server.rs:474-521, 656-714)
// The clients' records as ingested and their decoded points (RoundSrc's layout), allocated once for max_clients by create.  Ingest,
// accumulate, reset and destroy hold the round exclusively; the two verification legs hold it shared (they only read the record points --
// the Sigma leg also writes the odd slots, which no other call reads) and may run side by side on two lanes, one leg of each kind at a time.
// A round created with ROFL_ROUND_COMPRESSED (or by rofl_round_create_rand, which also allows 96-byte records: the pair is the first 64 bytes
// of each) also keeps, per client, the CompressedRandProof transcript as it stands after the client's d labelled pairs (everything the
// transcript absorbs before C' depends on the records alone): hashed at ingest from the bytes that are
// decoded, so that the compressed leg's verdict is about the snapshot the accumulation adds, whatever became of the caller's memory since.
struct Round {
    int device = 0; size_t d = 0, rec_len = 0, npts = 0, max_clients = 0, n = 0; unsigned flags = 0;
    uint8_t *rec = nullptr; niels *pts = nullptr; u32 *d_bad = nullptr;
    std::vector<u32> bad;      // host copy of d_bad: [client][3]
    std::vector<Merlin> prefix;      // ROFL_ROUND_COMPRESSED: [client], the Merlin state after the last pair (n of them)
    std::shared_mutex rw; std::mutex sigma_mu, range_mu, comp_mu;
    bool dead = false, released = false;
    RoundSrc src() const { return RoundSrc{d, npts, rec, pts, bad.data()}; }
};
Registry<Round> g_rounds;

// The Merlin states of nc CompressedRandProof transcripts after their d labelled pairs (everything they absorb before C'), on the lane's
// host pool.  Having absorbed messages of the same lengths, the transcripts' STROBE bookkeeping is identical at every step: eight of them
// share one AVX-512 instruction stream (keccak_x8.hpp); groups of fewer than five, and CPUs without AVX-512, keep the scalar transcript, one
// client per task.  pairs[j]: d records of `stride` bytes in host memory, the ElGamal pair in the first 64 of each (64: packed pairs; 96:
// SquareRandProofCommitments, hashed where they lie -- c_sq is not part of the transcript).
void compressed_prefixes(Ctx &C, size_t nc, const uint8_t *const *pairs, size_t d, Merlin *out, size_t stride = 64) {
    static const bool x8_on = k8::available();
    const Merlin start = [] { Merlin t("CompressedRandProof", 19); t.append("dom-sep", (const uint8_t *)"randomness proof v1", 19); return t; }();
    std::vector<std::pair<size_t, size_t>> tasks;      // (first client, count)
    for (size_t j0 = 0; j0 < nc; j0 += 8) {
        const size_t cnt = std::min<size_t>(8, nc - j0);
        if (x8_on && cnt >= 5) tasks.emplace_back(j0, cnt);
        else for (size_t l = 0; l < cnt; l++) tasks.emplace_back(j0 + l, 1);
    }
    C.pool->run(tasks.size(), [&](size_t k) {
        const size_t j0 = tasks[k].first, cnt = tasks[k].second;
        for (size_t l = 0; l < cnt; l++) out[j0 + l] = start;
        if (cnt == 1) {      // label = UNIQUE_U8_TRIPLETS[i] (generate_unique_u8_triplets.py:8-13)
            for (size_t i = 0; i < d; i++) { uint8_t lbl[3] = {(uint8_t)(3 * i), (uint8_t)(3 * i + 1), (uint8_t)(3 * i + 2)}; out[j0].append_lbl(lbl, 3, pairs[j0] + stride * i, 64); }
            return;
        }
        Merlin *tp[8]; const uint8_t *msg[8];
        for (size_t l = 0; l < cnt; l++) { tp[l] = &out[j0 + l]; msg[l] = pairs[j0 + l]; }
        if (d) k8::append_lbl3_run_x8(tp, (int)cnt, 0, msg, d, stride);
    });
}
// the challenge c of a transcript that stands after its pairs: C' absorbed, c drawn (the state is a copy: a round keeps its prefixes)
sc compressed_challenge(Merlin t, const uint8_t cprime[64]) { t.append("C_prime_eg", cprime, 64); return t.challenge_scalar("c"); }
// the challenges of nc proofs over host pairs (records of `stride` bytes, as compressed_prefixes reads them)
void compressed_challenges(Ctx &C, size_t nc, const uint8_t *const *proofs, const uint8_t *const *pairs, size_t d, sc *out, size_t stride = 64) {
    std::vector<Merlin> t(nc, Merlin("CompressedRandProof", 19));
    compressed_prefixes(C, nc, pairs, d, t.data(), stride);
    for (size_t j = 0; j < nc; j++) out[j] = compressed_challenge(t[j], proofs[j]);
}
// One array of a group of gc clients onto the device, on the lane's stream: client j's `per` bytes src(j) (null: the client has none, its
// slot is left alone) go to dst + j per.  Host clients are staged on the pool (~256 KB per task) into the pinned stg + j per and uploaded
// run by run; then the clients that on_dev(j) names are copied on the device.  True if anything was uploaded from stg (the caller records
// the event that guards its reuse).
template <class Src, class OnDev>
bool bring_group(Ctx &C, size_t gc, uint8_t *dst, uint8_t *stg, size_t per, Src src, OnDev on_dev) {
    const size_t slices = std::max<size_t>(1, per >> 18);
    auto host = [&](size_t j) { return src(j) && !on_dev(j); };
    bool any = false; for (size_t j = 0; j < gc; j++) any |= host(j);
    if (any) C.pool->run(gc * slices, [&](size_t t) { const size_t j = t / slices, k = t % slices; if (!host(j)) return;
                                             const size_t lo = per * k / slices, hi = per * (k + 1) / slices; stage_copy(stg + j * per + lo, src(j) + lo, hi - lo); });
    for (size_t j = 0; j < gc; ) {      // one upload per run of host clients
        if (!host(j)) { j++; continue; }
        size_t e = j; while (e < gc && host(e)) e++;
        HIPCHK(hipMemcpyAsync(dst + j * per, stg + j * per, (e - j) * per, hipMemcpyHostToDevice, C.stream));
        j = e;
    }
    for (size_t j = 0; j < gc; j++) if (src(j) && on_dev(j)) HIPCHK(hipMemcpyAsync(dst + j * per, src(j), per, hipMemcpyDeviceToDevice, C.stream));
    return any;
}
// clients [R.n, R.n + n): the records go up in groups of ~64 MB through two pinned staging buffers (the pool copies group g + 1 while group g
// is on its way and being decoded; device-resident records are copied on the device), one k_round_ingest per group: every point decoded once.
// A ROFL_ROUND_COMPRESSED round hashes each group's transcript prefixes on the pool while the device uploads and decodes the group: host
// records from the pinned staging copy that is being uploaded (the bytes that are decoded, not the caller's memory), device records from
// one copy back of what was copied into the round.  The states join the round with its client count, after the last synchronisation.
int round_ingest_impl(Ctx &C, Round &R, size_t n, const uint8_t *const *records) {
    const size_t d = R.d, per = d * R.rec_len, first = R.n;
    const bool comp = (R.flags & ROFL_ROUND_COMPRESSED) != 0;
    C.init();
    HIPCHK(hipMemsetAsync(R.d_bad + 3 * first, 0xff, 12 * n, C.stream));
    const size_t G = std::max<size_t>(1, std::min<size_t>(n, ((size_t)64 << 20) / per));
    std::vector<char> on_dev(n);
    for (size_t i = 0; i < n; i++) on_dev[i] = is_device_ptr(records[i]);
    std::vector<Merlin> prefix;
    if (comp) prefix.assign(n, Merlin("CompressedRandProof", 19));
    uint8_t *stb[2] = {nullptr, nullptr}; bool uploaded[2] = {false, false};
    for (size_t g0 = 0, gi = 0; g0 < n; g0 += G, gi++) {
        const size_t gc = std::min(G, n - g0);
        uint8_t *dst = R.rec + (first + g0) * per;
        bool any_host = false, any_dev = false; for (size_t i = g0; i < g0 + gc; i++) { any_host |= !on_dev[i]; any_dev |= (bool)on_dev[i]; }
        const int b = (int)(gi & 1);
        if (any_host || (comp && any_dev)) {      // (without the flag: only a group with host records touches the staging buffers)
            if (!stb[b]) stb[b] = (uint8_t *)C.stg.alloc(G * per); else if (uploaded[b]) C.wait_event(C.pool_event(b));
        }
        uint8_t *st = stb[b];
        // (the event marks the end of the uploads from st -- and of the device copies queued behind them, which cost nothing to wait for)
        if (bring_group(C, gc, dst, st, per, [&](size_t i) { return records[g0 + i]; }, [&](size_t i) { return (bool)on_dev[g0 + i]; })) {
            HIPCHK(hipEventRecord(C.pool_event(b), C.stream)); uploaded[b] = true; }
        if (comp && any_dev) {      // the round's copy of the device records comes back once, for the transcripts (before the decode is queued: the wait below covers copies only)
            for (size_t i = 0; i < gc; i++) if (on_dev[g0 + i]) HIPCHK(hipMemcpyAsync(st + i * per, dst + i * per, per, hipMemcpyDeviceToHost, C.stream));
            HIPCHK(hipEventRecord(C.pool_event(2), C.stream));
        }
        count_decodes(gc * R.npts * d);
        ROFL_LAUNCH(k_round_ingest, dim3((unsigned)((R.npts * d + TPB - 1) / TPB), (unsigned)gc), dim3(TPB), 0, C.stream, (u32)d, (u32)R.npts, (const uint8_t *)dst,
                    R.pts + (first + g0) * 2 * R.npts * d, R.d_bad + 3 * (first + g0));
        if (comp) {      // beside the upload and the decode of this group
            if (any_dev) C.wait_event(C.pool_event(2));
            std::vector<const uint8_t *> src(gc);
            for (size_t i = 0; i < gc; i++) src[i] = st + i * per;
            compressed_prefixes(C, gc, src.data(), d, prefix.data() + g0, R.rec_len);
        }
    }
    u32 *hb = C.h_misc.as<u32>(3 * n);
    HIPCHK(hipMemcpyAsync(hb, R.d_bad + 3 * first, 12 * n, hipMemcpyDeviceToHost, C.stream));
    C.sync();
    memcpy(&R.bad[3 * first], hb, 12 * n);
    if (comp) { R.prefix.resize(first, Merlin("CompressedRandProof", 19)); R.prefix.insert(R.prefix.end(), prefix.begin(), prefix.end()); }
    R.n = first + n;
    return ROFL_OK;
}
// sum += the cached (L, R) of the clients in `cl`: mixed additions from the cache in tiles of kAccTile points, S client slices per tile
// folded into the sum by k_acc_fold.  All or nothing is decided before anything is launched: what did not decode is known since ingest.
int round_accumulate_impl(Ctx &C, Round &R, Acc &A, const std::vector<u32> &cl) {
    for (u32 c : cl) if (R.bad[3 * c] != ~0u || R.bad[3 * c + 1] != ~0u)
        return fail(ROFL_FORMAT_ERROR, "FormatError: a record is not a valid Ristretto encoding (the accumulator is unchanged)");
    if (cl.empty()) return ROFL_OK;
    const size_t d = R.d, tile = std::min(d, kAccTile), na = cl.size();
    const size_t S = std::max<size_t>(1, std::min(na, (kAccThreads + 2 * tile - 1) / (2 * tile)));
    C.init();
    ge *part = C.partial2.as<ge>(S * tile * 2);
    u32 *d_idx = C.tmp_out.as<u32>(na);
    u32 *h_idx = (u32 *)C.stg.alloc(na * 4); memcpy(h_idx, cl.data(), na * 4);
    HIPCHK(hipMemcpyAsync(d_idx, h_idx, na * 4, hipMemcpyHostToDevice, C.stream));
    const ge init = acc_init_point(A.init);
    const bool multi = d > tile;      // several tiles: into a copy of the sum that a last fold commits, as acc_add_impl (a runtime error on the way leaves the sum as it was)
    ge *tgt = acc_work_begin(C, A, multi);
    for (size_t j0 = 0; j0 < d; j0 += tile) {
        const size_t tn = std::min(tile, d - j0);
        ROFL_LAUNCH(k_round_sum, grid1(2 * tn * S), dim3(TPB), 0, C.stream, (u32)tn, (u32)j0, (u32)S, (u32)na, (const u32 *)d_idx, (const niels *)R.pts, (u32)d, (u32)(2 * R.npts), part);
        ROFL_LAUNCH(k_acc_fold, grid1(2 * tn), dim3(TPB), 0, C.stream, (u32)(2 * tn), (u32)S, (const ge *)part, (const ge *)(tgt + 2 * j0), init, tgt + 2 * j0, (const u32 *)nullptr);
    }
    if (multi) {
        C.sync();      // every tile is in the copy: only now does the sum change
        acc_work_commit(C, A, nullptr);
    }
    C.sync();
    return ROFL_OK;
}
// What every rofl_acc_* / rofl_round_* entry does before its own work, f(object), which runs bound to the object's device with the object
// locked (Lock on its mutex; then `leg`, if any) and alive: the handle is looked up, pre(object) checks the arguments against what create
// fixed (before the lock, as ever), a handle that is being or has been destroyed is as unknown as one that never was.
template <class Lock, class T, class M, class Pre, class F>
int with_handle(Registry<T> &reg, uint64_t h, M T::*mu, const char *unknown, std::mutex T::*leg, Pre pre, F f) {
    std::shared_ptr<T> p = reg.find(h);
    if (!p) return fail(ROFL_BAD_PARAM, unknown);
    if (int rc = pre(*p)) return rc;
    Lock lk((*p).*mu);
    if (p->dead) return fail(ROFL_BAD_PARAM, unknown);
    std::unique_lock<std::mutex> leg_lk;
    if (leg) leg_lk = std::unique_lock<std::mutex>((*p).*leg);
    DeviceBinding bind(p->device);
    return guarded([&]() -> int { return f(*p); });
}
constexpr const char *kNoAcc = "unknown accumulator handle", *kNoRound = "unknown round handle";
template <class Pre, class F> int with_acc(uint64_t h, Pre pre, F f) { return with_handle<std::lock_guard<std::mutex>>(g_accs, h, &Acc::mu, kNoAcc, (std::mutex Acc::*)nullptr, pre, f); }
template <class Lock, class Pre, class F> int with_round(uint64_t h, std::mutex Round::*leg, Pre pre, F f) { return with_handle<Lock>(g_rounds, h, &Round::rw, kNoRound, leg, pre, f); }
using RoundShared = std::shared_lock<std::shared_mutex>; using RoundExclusive = std::unique_lock<std::shared_mutex>;
// destroy: the object is marked dead (from here on only a destroy may use the handle), what it holds on the device is freed, and only then
// does the handle leave the registry -- a free that fails leaves it there for another try, which frees what is left.  `released` is for a
// destroy that found the handle before it left the registry: it waits for the lock and then sees that another thread was first.
template <class T, class M, class F> int destroy_handle(Registry<T> &reg, uint64_t h, M T::*mu, const char *unknown, F free_all) {
    std::shared_ptr<T> p = reg.find(h);
    if (!p) return fail(ROFL_BAD_PARAM, unknown);
    std::unique_lock<M> lk((*p).*mu);
    if (p->released) return fail(ROFL_BAD_PARAM, unknown);
    p->dead = true;
    DeviceBinding bind(p->device);
    if (int rc = guarded([&]() -> int { LaneLock lane_lock = acquire_lane(); free_all(*p); return ROFL_OK; })) return rc;
    p->released = true;
    reg.erase(h);
    return ROFL_OK;
}
template <class T> void dev_free(T *&p) { if (p) HIPCHK(hipFree(p)); p = nullptr; }
const auto no_check = [](auto &) { return ROFL_OK; };
// ---- the driver of k_blind_combine, shared by rofl_blinding_vecs and rofl_acc_extract_opened_terms ----
// one term list of a call, checked before the device is touched; *total: the terms of the call so far
int blind_terms_check(size_t term_count, const rofl_blind_term_t *terms, size_t *total) {
    if (term_count && !terms) return fail(ROFL_BAD_PARAM, "bad parameter");
    if (term_count > ((size_t)1 << 22) || (*total += term_count) > ((size_t)1 << 22)) return fail(ROFL_BAD_PARAM, "more than 2^22 terms in one call");
    for (size_t t = 0; t < term_count; t++)
        if (terms[t].sign != 1 && terms[t].sign != -1) return fail(ROFL_BAD_PARAM, "a term's sign is +1 or -1");
    return ROFL_OK;
}
// the lane's copies of a call's term list (pinned host memory, device workspace): overwritten with zeros when the call returns or unwinds
// (h == nullptr: a device workspace that has no host copy)
struct BlindWipe { uint8_t *h = nullptr, *dv = nullptr; size_t n = 0; hipStream_t s = nullptr;
                   ~BlindWipe() { if (!n) return; (void)hipMemsetAsync(dv, 0, n, s); (void)hipStreamSynchronize(s); volatile uint8_t *p = h; for (size_t i = 0; p && i < n; i++) p[i] = 0; } };
// vector v = sum of its terms' streams [first, first + d) into dst[v] (device memory, 16-byte aligned), every vector in ONE launch on the
// lane's stream; the term list is staged in C.h_misc and in `term_buf`, which the caller leaves alone until `wipe` has run
void blind_combine_launch(Ctx &C, DevBuf &term_buf, BlindWipe &wipe, size_t n_vec, const size_t *term_count, const rofl_blind_term_t *const *terms, size_t total,
                          size_t first, size_t d, uint8_t *const *dst) {
    const size_t bytes = n_vec * sizeof(BlindVec) + total * sizeof(BlindTerm);
    uint8_t *h = C.h_misc.as<uint8_t>(bytes), *dv = term_buf.as<uint8_t>(bytes);
    wipe.h = h; wipe.dv = dv; wipe.n = bytes; wipe.s = C.stream;
    BlindVec *hv = reinterpret_cast<BlindVec *>(h); BlindTerm *ht = reinterpret_cast<BlindTerm *>(h + n_vec * sizeof(BlindVec));
    size_t at = 0;
    for (size_t v = 0; v < n_vec; v++) {
        hv[v].out = dst[v]; hv[v].term_first = (u32)at; hv[v].term_count = (u32)term_count[v];
        for (size_t t = 0; t < term_count[v]; t++, at++) { memcpy(ht[at].seed, terms[v][t].seed, 32); ht[at].neg = terms[v][t].sign < 0; ht[at].pad = 0; }
    }
    HIPCHK(hipMemcpyAsync(dv, h, bytes, hipMemcpyHostToDevice, C.stream));
    const size_t nblk = ((first + d + 1) >> 1) - (first >> 1);
    ROFL_LAUNCH(k_blind_combine, grid1(nblk, (u32)n_vec), dim3(TPB), 0, C.stream, reinterpret_cast<const BlindVec *>(dv),
                reinterpret_cast<const BlindTerm *>(dv + n_vec * sizeof(BlindVec)), (u64)first, (u32)d);
}
// The opening of a sum's residual blinding, for the two rofl_acc_extract_opened entries: d raw scalars in caller memory (host or device),
// or the term list they are built from on the device.  rofl_acc_extract hands none in.
struct AccOpening { const uint8_t *bytes; size_t term_count; const rofl_blind_term_t *terms; };
// What the extraction entries share -- the primary lane, the finishing launch, the verdict, BSGS, the download and the conversion; they
// differ in the finishing launch only: k_acc_finish (R == the initial R, L encoded as it is) or, with an opening, k_acc_open (R == initial R
// + s B, L - s B~ encoded).  The sum is read, never written.
int acc_extract(uint64_t h, const AccOpening *op, size_t table_size, unsigned bsgs_bits, unsigned fp_bits, unsigned fp_frac, float *out, int *ok_out, size_t *first_bad_out) {
    if (!out || !ok_out || table_size == 0 || table_size >= (1u << 30) || !(bsgs_bits == 8 || bsgs_bits == 16 || bsgs_bits == 32) || !valid_fp(fp_bits, fp_frac))
        return fail(ROFL_BAD_PARAM, "bad parameter");
    std::vector<uint8_t> hv;      // (outlives the lane: its release delivers the staged scalars here)
    return with_acc(h, no_check, [&](Acc &A) -> int {
        LaneLock lane_lock = acquire_lane(true); Ctx &C = *lane_lock.c;      // the primary lane: the baby-step tables rofl_discrete_log_vec caches
        C.init();
        const size_t d = A.d;
        if (op && !op->bytes && d >= ((size_t)1 << 28)) return fail(ROFL_BAD_PARAM, "vector length of 2^28 or more");      // (as rofl_blinding_vecs)
        uint8_t *enc = C.tmp_in.as<uint8_t>(d * 32), *dout = C.Cbytes.as<uint8_t>(d * 32);
        u32 *status = C.status.as<u32>(4);      // [0] BSGS, [1] some R equation fails, [2] the smallest index of one
        HIPCHK(hipMemsetAsync(status, 0, 16, C.stream));
        const ge b = acc_init_point(A.init);
        BlindWipe wipe;
        if (!op) ROFL_LAUNCH(k_acc_finish, grid1(d), dim3(TPB), 0, C.stream, (u32)d, 0, (const ge *)A.sum, b.X, b.Y, enc, status + 1);
        else {
            const uint8_t *s = op->bytes;
            if (!s || !is_device_ptr(s)) {      // a device opening is read in place; a host opening is uploaded, a term list expanded, into the lane's scratch
                uint8_t *ws = C.blind.as<uint8_t>(d * 32);
                if (s) C.up(ws, s, d * 32, C.stream);
                else { const size_t one = op->term_count; blind_combine_launch(C, C.tmp_in2, wipe, 1, &one, &op->terms, op->term_count, 0, d, &ws); }
                s = ws;
            } else if ((uintptr_t)s & 15) return fail(ROFL_BAD_PARAM, "a device opening must be 16-byte aligned");
            HIPCHK(hipMemsetAsync(status + 2, 0xff, 4, C.stream));
            ROFL_LAUNCH(k_acc_open, grid1(d, 2), dim3(TPB), 0, C.stream, (u32)d, (const ge *)A.sum, reinterpret_cast<const sc *>(s), b, C.d_tabB8, C.d_tabBb8, enc, status + 1);
        }
        u32 st[3] = {0, 0, 0};
        HIPCHK(hipMemcpyAsync(st, status, 12, hipMemcpyDeviceToHost, C.stream));
        C.sync();
        if (st[1]) {      // some R is not the initial one (plus the opening's s B): the blindings did not cancel (the reference's None) / the opening is wrong
            *ok_out = 0;
            if (op && first_bad_out) *first_bad_out = st[2];
            return ROFL_OK;
        }
        bsgs_solve_launch(C, d, enc, table_size, bsgs_bits, dout, status);
        hv.resize(d * 32);
        const uint8_t *hs = (const uint8_t *)C.down(hv.data(), dout, d * 32, C.stream);
        HIPCHK(hipMemcpyAsync(st, status, 4, hipMemcpyDeviceToHost, C.stream));
        C.sync();
        if (st[0] & 4u) return fail(ROFL_FORMAT_ERROR, "invalid Ristretto encoding");
        if (st[0] & 8u) return fail(ROFL_BAD_PARAM, "discrete log not found (the reference unwraps None)");
        for (size_t i = 0; i < d; i++) out[i] = sc_to_f32(sc_frombytes(hs + 32 * i), fp_bits, fp_frac);
        *ok_out = 1;
        if (op && first_bad_out) *first_bad_out = (size_t)-1;
        return ROFL_OK;
    });
}
}  // namespace

// ================================================================ C ABI
extern "C" {

// rofl_set_device binds the calling thread to `device` (and makes it the default of threads that have no binding of their own), then
// brings that device's context up so that a missing device shows here and not in the first proof.
int rofl_set_device(int device) {
    if (device < 0 || device >= kMaxDevices) return fail(ROFL_BAD_PARAM, "bad device index");
    const int prev = t_device;
    t_device = device;
    int rc = guarded([&]() -> int { LaneLock lane_lock = acquire_lane(); Ctx &C = *lane_lock.c; C.init(); return ROFL_OK; });
    if (rc) {      // a device that cannot be used is not selected -- and leaves no half-built context behind (rofl_dbg_map_device would see it "in use")
        t_device = prev;
        std::lock_guard<std::mutex> lk(g_ctx_mu);
        auto it = g_ctxs.find(device);
        if (it != g_ctxs.end() && !it->second->inited && it->second->active_calls.load() == 0) { delete it->second; g_ctxs.erase(it); }
        return rc;
    }
    // The process default -- what threads without a binding of their own follow -- is set by the FIRST successful call only: in a server whose
    // pool threads each bind their own device, the default of unbound threads must not become whichever thread called last.
    // rofl_set_option("default_device", d) moves it explicitly.
    bool expected = false;
    if (g_default_set.compare_exchange_strong(expected, true)) g_default_device.store(device);
    return rc;
}
int rofl_get_device(int *device_out) { if (!device_out) return fail(ROFL_BAD_PARAM, "bad parameter"); *device_out = current_device(); return ROFL_OK; }
int rofl_bind_device(int device) { if (device < -1 || device >= kMaxDevices) return fail(ROFL_BAD_PARAM, "bad device index"); t_device = device; return ROFL_OK; }
int rofl_dbg_bind_device(int device) { if (device < -1 || device >= kMaxDevices) return ROFL_BAD_PARAM; t_device = device; return ROFL_OK; }
int rofl_dbg_map_device(int logical, int physical) {
    if (logical < 0 || logical >= kMaxDevices || physical < 0) return ROFL_BAD_PARAM;
    devmap_init();
    std::lock_guard<std::mutex> lk(g_ctx_mu);
    if (g_ctxs.count(logical)) return g_devmap[logical] == physical ? ROFL_OK : fail(ROFL_BAD_PARAM, "the device is already in use");      // (asking for the mapping it already has is fine)
    g_devmap[logical] = physical; return ROFL_OK;
}
int rofl_last_error(char *buf, size_t len) { if (!buf || !len) return ROFL_BAD_PARAM; snprintf(buf, len, "%s", g_err.c_str()); return ROFL_OK; }
size_t rofl_next_pow2(size_t v) { return v ? next_pow2(v) : 0; }
size_t rofl_rangeproof_chunks(size_t d, size_t n_partition) {
    if (!d || !n_partition) return 0;
    size_t dp = next_pow2(d), nc = std::min(dp, n_partition), chunk = dp / nc; return (dp + chunk - 1) / chunk;
}
size_t rofl_rangeproof_size(size_t n_bits, size_t d, size_t n_partition) {
    if (!d || !n_partition) return 0;
    size_t dp = next_pow2(d), nc = std::min(dp, n_partition), chunk = dp / nc; return 32 * (9 + 2 * (size_t)lg2u(n_bits * chunk));
}
size_t rofl_nonces_per_chunk(size_t n_bits, size_t m) { return m * (2 * n_bits + 4); }

int rofl_bp_gens_prepare(size_t n_bits, size_t m) {
    return guarded([&]() -> int { LaneLock lane_lock = acquire_lane(); Ctx &C = *lane_lock.c; C.init(); if (!n_bits || !m) return fail(ROFL_BAD_PARAM, "bad parameter"); { GensPin pin = get_gens(C, n_bits, m); }
        if (!gens_wait_full(C, n_bits, m)) g_err = "HBM is short: the shape keeps its compact fold table (same results, slower first fold)";      // not an error: see rofl_zk.h
        return ROFL_OK; });
}
int rofl_bp_gens_prepare_verify(size_t n_bits, size_t m) {
    return guarded([&]() -> int { LaneLock lane_lock = acquire_lane(); Ctx &C = *lane_lock.c; C.init(); if (!n_bits || !m) return fail(ROFL_BAD_PARAM, "bad parameter");
        { GensPin pin = get_gens(C, n_bits, m, GENS_VERIFY); }
        return ROFL_OK; });
}
int rofl_bp_gens_table_bytes(size_t n_bits, size_t m, size_t *bytes_out) {
    return guarded([&]() -> int {
        if (!bytes_out) return fail(ROFL_BAD_PARAM, "bad parameter");
        Ctx &P = ctx(); { std::lock_guard<std::mutex> g(P.init_mu); P.init(); }
        std::lock_guard<std::mutex> lk(P.gens_mu);
        auto it = P.gens.find(std::make_pair(n_bits, m));
        *bytes_out = it == P.gens.end() ? 0 : it->second->bytes;
        return ROFL_OK;
    });
}
int rofl_bp_gens_export(size_t n_bits, size_t m, uint8_t *G_out, uint8_t *H_out) {
    return guarded([&]() -> int {
        LaneLock lane_lock = acquire_lane(); Ctx &C = *lane_lock.c; C.init();
        if (!n_bits || !m) return fail(ROFL_BAD_PARAM, "bad parameter");
        GensPin gens = get_gens(C, n_bits, m, GENS_VERIFY); niels *tbl = gens.tbl(); size_t N = n_bits * m;
        // encode through the commit path: decode-free -- use k_msm-free helper: copy niels back and encode on host
        std::vector<niels> h(2 * N);
        HIPCHK(hipMemcpy(h.data(), tbl, sizeof(niels) * 2 * N, hipMemcpyDeviceToHost));
        for (size_t i = 0; i < 2 * N; i++) { ge p = ge_from_niels(h[i]); ristretto_encode((i < N ? G_out + 32 * i : H_out + 32 * (i - N)), p); }
        return ROFL_OK;
    });
}

int rofl_create_rangeproof(const float *values, size_t d, const uint8_t *blindings32, size_t d_blindings, size_t prove_range, size_t n_partition,
                           unsigned fp_bits, unsigned fp_frac, const rofl_nonce_t *nonce, uint8_t *proofs_out, size_t *proof_len_out,
                           size_t *n_proofs_out, uint8_t *commits_out) {
    return guarded([&]() -> int {
        if (d != d_blindings) return fail(ROFL_WRONG_NUM_BLINDING, "WrongNumBlindingFactors");
        // rofl_set_option("devices", mask) with several devices: the client's chunks are dealt to them (create_split); malformed parameters take the ordinary path and get its diagnostics
        std::vector<int> devs = batch_devices();
        if (devs.size() > 1 && values && blindings32 && nonce && proofs_out && commits_out && proof_len_out && n_proofs_out && d && n_partition && valid_fp(fp_bits, fp_frac) &&
            prove_range && prove_range <= fp_bits && rofl_rangeproof_chunks(d, n_partition) > 1)
            return create_split(devs, values, d, blindings32, prove_range, n_partition, fp_bits, fp_frac, nonce, proofs_out, proof_len_out, n_proofs_out, commits_out);
        ListedDevice bind(devs);
        LaneLock lane_lock = acquire_lane(); Ctx &C = *lane_lock.c;
        int rc1 = ROFL_OK;
        int rc = create_impl(C, 1, &values, d, &blindings32, prove_range, n_partition, fp_bits, fp_frac, nonce, &proofs_out, proof_len_out, n_proofs_out, &commits_out, &rc1, true);
        return rc ? rc : rc1; });
}
int rofl_create_rangeproof_chunks(const float *values, size_t d, const uint8_t *blindings32, size_t d_blindings, size_t prove_range, size_t n_partition,
                                  unsigned fp_bits, unsigned fp_frac, const rofl_nonce_t *nonce, size_t chunk_first, size_t chunk_count,
                                  uint8_t *proofs_out, size_t *proof_len_out, uint8_t *commits_out, size_t *n_commits_out) {
    return guarded([&]() -> int {
        if (!values || !blindings32 || !nonce || !proofs_out || !proof_len_out || !commits_out || !n_commits_out || chunk_count == 0) return fail(ROFL_BAD_PARAM, "bad parameter");
        if (d != d_blindings) return fail(ROFL_WRONG_NUM_BLINDING, "WrongNumBlindingFactors");
        LaneLock lane_lock = acquire_lane(); Ctx &C = *lane_lock.c;
        int rc1 = ROFL_OK; size_t np = 0;
        int rc = create_impl(C, 1, &values, d, &blindings32, prove_range, n_partition, fp_bits, fp_frac, nonce, &proofs_out, proof_len_out, &np, &commits_out, &rc1, true, chunk_first, chunk_count);
        if (rc || rc1) return rc ? rc : rc1;
        const size_t dp = next_pow2(d), chunk = dp / std::min(dp, n_partition), el0 = chunk_first * chunk;
        *n_commits_out = el0 >= d ? 0 : std::min(d - el0, chunk_count * chunk);
        return ROFL_OK; });
}
int rofl_create_rangeproof_batch(size_t n_clients, const float *const *values, size_t d, const uint8_t *const *blindings32, size_t prove_range,
                                 size_t n_partition, unsigned fp_bits, unsigned fp_frac, const rofl_nonce_t *nonces, uint8_t *const *proofs_out,
                                 size_t *proof_len_out, size_t *n_proofs_out, uint8_t *const *commits_out, int *rc_out) {
    if (!values || !blindings32 || !proofs_out || !commits_out || !rc_out || !proof_len_out || !n_proofs_out || !nonces) return fail(ROFL_BAD_PARAM, "bad parameter");
    const bool single = false;      // per-client outcomes in rc_out, also for a batch of ONE (the return value is for errors of the whole call)
    std::mutex out_mu;
    return over_devices(n_clients, nullptr, [&](const Share &sh) -> int {
        auto v = sh.view(values); auto b = sh.view(blindings32); auto nn = sh.view(nonces); auto po = sh.view(proofs_out); auto co = sh.view(commits_out); auto rc = sh.out(rc_out);
        size_t plen = 0, np = 0;      // a share's own geometry: the caller's proof_len_out / n_proofs_out are written only by a share that succeeded (unlike the L2 creator's, set before dispatch)
        LaneLock lane_lock = acquire_lane(); Ctx &C = *lane_lock.c;
        int r = create_impl(C, sh.size(), v.data(), d, b.data(), prove_range, n_partition, fp_bits, fp_frac, nn.data(), po.data(), sh.whole() ? proof_len_out : &plen,
                            sh.whole() ? n_proofs_out : &np, co.data(), rc.data(), single);
        sh.scatter(rc);
        if (!sh.whole() && !r) { std::lock_guard<std::mutex> lk(out_mu); *proof_len_out = plen; *n_proofs_out = np; }
        return r; });
}
int rofl_verify_rangeproof(const uint8_t *proofs, size_t proof_len, size_t n_proofs, const uint8_t *commits32, size_t d, size_t prove_range,
                           unsigned fp_bits, unsigned fp_frac, const uint8_t verifier_seed[32], int *ok_out) {
    return guarded([&]() -> int {
        std::vector<int> devs = batch_devices();
        if (devs.size() > 1 && proofs && commits32 && ok_out && verifier_seed && verify_splittable(d, n_proofs))      // the client's proofs over the listed devices (verify_split)
            return verify_split(devs, proofs, proof_len, n_proofs, commits32, d, prove_range, fp_bits, fp_frac, verifier_seed, ok_out);
        ListedDevice bind(devs);
        LaneLock lane_lock = acquire_lane(); Ctx &C = *lane_lock.c;
        return verify_impl(C, 1, &proofs, proof_len, n_proofs, &commits32, d, prove_range, fp_bits, fp_frac, verifier_seed, ok_out, true); });
}
int rofl_verify_rangeproof_chunks(const uint8_t *proofs, size_t proof_len, size_t n_proofs, size_t chunk_first, size_t chunk_count, const uint8_t *commits32,
                                  size_t d, size_t prove_range, unsigned fp_bits, unsigned fp_frac, const uint8_t verifier_seed[32], int *ok_out) {
    return guarded([&]() -> int {
        if (!proofs || !commits32 || !ok_out || !verifier_seed || chunk_count == 0) return fail(ROFL_BAD_PARAM, "bad parameter");
        { const size_t dp = d ? next_pow2(d) : 0;
          if (!d || !n_proofs || n_proofs > dp || (dp / n_proofs) * n_proofs != dp) return fail(ROFL_BAD_PARAM, "a run of chunks needs a proof count that covers the padded vector exactly"); }
        LaneLock lane_lock = acquire_lane(); Ctx &C = *lane_lock.c;
        return verify_impl(C, 1, &proofs, proof_len, n_proofs, &commits32, d, prove_range, fp_bits, fp_frac, verifier_seed, ok_out, true, nullptr, 32, chunk_first, chunk_count); });
}
int rofl_verify_rangeproof_batch(size_t n_clients, const uint8_t *const *proofs, size_t proof_len, size_t n_proofs, const uint8_t *const *commits32,
                                 size_t d, size_t prove_range, unsigned fp_bits, unsigned fp_frac, const uint8_t verifier_seed[32], int *ok_out) {
    return rofl_verify_rangeproof_batch_strided(n_clients, proofs, proof_len, n_proofs, commits32, 32, d, prove_range, fp_bits, fp_frac, verifier_seed, ok_out);
}
int rofl_verify_rangeproof_batch_strided(size_t n_clients, const uint8_t *const *proofs, size_t proof_len, size_t n_proofs, const uint8_t *const *commits32, size_t commit_stride,
                                         size_t d, size_t prove_range, unsigned fp_bits, unsigned fp_frac, const uint8_t verifier_seed[32], int *ok_out) {
    if (!proofs || !commits32 || !ok_out || !verifier_seed || commit_stride < 32) return fail(ROFL_BAD_PARAM, "bad parameter");
    const bool single = false;      // a batch has per-member verdicts, also a batch of ONE: a malformed member gets ok = 0, not the FormatError of rofl_verify_rangeproof (found by the long batch fuzz)
    return over_devices(n_clients, ok_out, [&](const Share &sh) -> int {
        auto p = sh.view(proofs); auto c = sh.view(commits32); auto ok = sh.out(ok_out);
        LaneLock lane_lock = acquire_lane(); Ctx &C = *lane_lock.c;
        // (only this verifier is told the members' positions in the whole batch)
        int r = verify_impl(C, sh.size(), p.data(), proof_len, n_proofs, c.data(), d, prove_range, fp_bits, fp_frac, verifier_seed, ok.data(), single, sh.positions(), commit_stride);
        sh.scatter(ok);
        return r; });
}
int rofl_clip_f32(const float *in, size_t d, size_t prove_range, unsigned fp_bits, unsigned fp_frac, float *out) {
    if (!valid_fp(fp_bits, fp_frac) || prove_range == 0) return fail(ROFL_BAD_PARAM, "bad parameter");
    float mn, mx; clip_bounds(prove_range, fp_bits, fp_frac, &mn, &mx);
    for (size_t i = 0; i < d; i++) { float t = fmaxf(mn, in[i]); out[i] = fminf(mx, t); }
    return ROFL_OK;
}

namespace {
// What create_rangeproof_l2 decides on the host once a client's sums are known (l2_range_proof_vec/mod.rs:62-79, then the upstream errors), in
// the reference's order: the f32 shadow sum against the scalar sum (OverflowError), the norm bound, the bit size, the nonce stream.
// *v_out: the value the sum proof commits to.
int l2_sum_outcome(const sc &val, float val_float, size_t prove_range, unsigned fp_bits, unsigned fp_frac, const rofl_nonce_t *nonce, u64 *v_out) {
    float val_f = sc_to_f32(val, fp_bits, fp_frac);
    volatile float diff = val_f - val_float;
    if (std::fabs(diff) > 1.1920929e-07f) return ROFL_OVERFLOW;
    if (val_f > l2_clip_bound(prove_range, fp_bits, fp_frac)) return ROFL_NORM_OUT_OF_RANGE;
    if (!(prove_range == 8 || prove_range == 16 || prove_range == 32 || prove_range == 64)) return ROFL_INVALID_BITSIZE;
    if (nonce->mode == 0 && nonce->stream_scalars < 2 * prove_range + 4) return ROFL_NONCE_SHORT;
    *v_out = read_from_bytes(val, fp_bits);
    return ROFL_OK;
}
const char *l2_outcome_text(int rc) {
    switch (rc) {
        case ROFL_VALUE_OUT_OF_RANGE: return "ValueOutOfRangeError";
        case ROFL_NON_FINITE: return "non-finite value";
        case ROFL_OVERFLOW: return "OverflowError";
        case ROFL_NORM_OUT_OF_RANGE: return "NormOutOfRangeError";
        case ROFL_INVALID_BITSIZE: return "InvalidBitsize";
        case ROFL_NONCE_SHORT: return "nonce stream too short";
    }
    return "";
}
// THE creator of L2 sum proofs: create_rangeproof_l2 for the clients of one process (the one-value sum proofs of a round's L2 updates) as
// ONE launch sequence; rofl_create_rangeproof_l2 is a group of one.  rcs[i] is client i's own outcome in the reference's order (within a
// client ValueOutOfRange 2 wins over NaN 10 wherever they sit, then 8, 7, 3, 12; l2_outcome_text has the texts).
// k_l2_sumsq_batch (client = grid row, kL2SumBlocks blocks striding over the d values) leaves per client the status bits, the block
// partials of sum k^2 (192-bit integers) and of the blinding sum, and per element the f32 term of the reference's shadow sum;
// k_l2_sumsq_combine adds the partials.  WAIT 1: status words, sums and terms are on the host (4 d bytes per client: the shadow sum is
// serial left to right by definition, so the pool adds every client's terms in order and decides with l2_sum_outcome what the reference
// returns).  The surviving clients are compacted densely: one k_commit over them (WAIT 2: their V bytes, for the
// transcripts) and one prove_chunks over na chunks of one value -- the host hops of the Bulletproof are paid once per batch.
constexpr u32 kL2SumBlocks = 8;      // per client: 2 048 threads stride over d; 48 clients are 384 blocks on 256 CUs
u32 l2_sum_blocks(size_t d) { return (u32)std::min<size_t>(kL2SumBlocks, (d + TPB - 1) / TPB); }
int l2_create_batch(size_t nc, const float *const *values, size_t d, const uint8_t *const *blind, size_t prove_range, unsigned fp_bits, unsigned fp_frac,
                    const rofl_nonce_t *nonces, uint8_t *const *proofs_out, uint8_t *commits_out32, int *rcs) {
    LaneLock lane_lock = acquire_lane(false, nc == 1); Ctx &C = *lane_lock.c;
    for (size_t i = 0; i < nc; i++) rcs[i] = ROFL_OK;
    C.init();
    C.batch_mode = nc > 1;
    timing_begin(C);
    float mn, mx; clip_bounds(prove_range, fp_bits, fp_frac, &mn, &mx);
    std::vector<char> dev_v(nc), dev_b(nc); bool any_host = false;
    for (size_t i = 0; i < nc; i++) { dev_v[i] = is_device_ptr(values[i]); dev_b[i] = is_device_ptr(blind[i]); any_host |= !dev_v[i] || !dev_b[i]; }
    const u32 nblk = l2_sum_blocks(d);
    float *dv = C.vals.as<float>(nc * d), *dterms = C.tmp_out.as<float>(nc * d);
    sc *dbl = C.blind.as<sc>(std::max<size_t>(nc * d, nc)), *part_bl = C.tmp_in2.as<sc>(nc * nblk), *dsums = C.aux_scal.as<sc>(2 * nc);
    u64 *part_sq = C.tmp_in.as<u64>(nc * nblk * 3);
    u32 *status = C.status.as<u32>(nc + 4), *h_st = C.h_misc.as<u32>(nc + 4);
    HIPCHK(hipMemsetAsync(status, 0, 4 * (nc + 4), C.stream));
    uint8_t *stg = any_host ? (uint8_t *)C.stg.alloc(nc * d * 36) : nullptr;
    bring_group(C, nc, (uint8_t *)dv, stg, 4 * d, [&](size_t j) { return (const uint8_t *)values[j]; }, [&](size_t j) { return (bool)dev_v[j]; });
    bring_group(C, nc, (uint8_t *)dbl, stg ? stg + nc * d * 4 : nullptr, 32 * d, [&](size_t j) { return blind[j]; }, [&](size_t j) { return (bool)dev_b[j]; });
    ROFL_LAUNCH(k_l2_sumsq_batch, dim3(nblk, (unsigned)nc), dim3(TPB), 0, C.stream, (u32)d, fp_bits, fp_frac, mn, mx, (const float *)dv, (const sc *)dbl, dterms, part_sq, part_bl, status);
    ROFL_LAUNCH(k_l2_sumsq_combine, dim3((unsigned)((nc + 63) / 64)), dim3(64), 0, C.stream, (u32)nc, nblk, (const u64 *)part_sq, (const sc *)part_bl, dsums);
    float *h_terms = (float *)C.stg.alloc(nc * d * 4); sc *h_sums = C.h_misc2.as<sc>(2 * nc);
    HIPCHK(hipMemcpyAsync(h_terms, dterms, nc * d * 4, hipMemcpyDeviceToHost, C.stream));
    HIPCHK(hipMemcpyAsync(h_sums, dsums, sizeof(sc) * 2 * nc, hipMemcpyDeviceToHost, C.stream));
    HIPCHK(hipMemcpyAsync(h_st, status, 4 * nc, hipMemcpyDeviceToHost, C.stream));
    C.sync();                                    // wait 1
    std::vector<u64> v64(nc, 0);
    C.pool->run(nc, [&](size_t i) {
        if (h_st[i] & 1u) { rcs[i] = ROFL_VALUE_OUT_OF_RANGE; return; }      // (the range loop runs to its end before anything is converted)
        if (h_st[i] & 2u) { rcs[i] = ROFL_NON_FINITE; return; }
        const float *t = h_terms + i * d;
        volatile float val_float = 0.0f;
        for (size_t e = 0; e < d; e++) { volatile float term = t[e]; val_float = (e == 0) ? term : val_float + term; }
        rcs[i] = l2_sum_outcome(h_sums[2 * i], val_float, prove_range, fp_bits, fp_frac, &nonces[i], &v64[i]);
    });
    std::vector<size_t> act;
    for (size_t i = 0; i < nc; i++) if (rcs[i] == ROFL_OK) act.push_back(i);
    if (act.empty()) { timing_end(C); return ROFL_OK; }
    const size_t na = act.size();
    // the survivors, densely (the proof kernels index chunks densely): value and blinding sum of each
    u64 *h_v = C.h_auxc.as<u64>(na); sc *h_b = C.h_auxs.as<sc>(na);
    for (size_t k = 0; k < na; k++) { h_v[k] = v64[act[k]]; h_b[k] = h_sums[2 * act[k] + 1]; }
    u64 *vshift = C.vshift.as<u64>(na); sc *d_bl = dbl;      // (the blindings themselves have been read)
    HIPCHK(hipMemcpyAsync(vshift, h_v, 8 * na, hipMemcpyHostToDevice, C.stream));
    HIPCHK(hipMemcpyAsync(d_bl, h_b, sizeof(sc) * na, hipMemcpyHostToDevice, C.stream));
    uint8_t *Vb = C.Vbytes.as<uint8_t>(na * 32), *hV = C.h_V.as<uint8_t>(na * 32);
    ROFL_LAUNCH(k_commit, grid1(na), dim3(TPB), 0, C.stream, (u32)na, vshift, (const sc *)nullptr, d_bl, C.d_tabB8, C.d_tabBb8, (const niels *)nullptr, Vb, (uint8_t *)nullptr, 0u, 1u);
    HIPCHK(hipMemcpyAsync(hV, Vb, na * 32, hipMemcpyDeviceToHost, C.stream));
    // explicit nonce streams: the 2 n + 4 scalars a one-value proof draws, every client's at index 0 of its own stream
    const size_t per = 2 * prove_range + 4;
    size_t n_streams = 0; for (size_t k = 0; k < na; k++) n_streams += nonces[act[k]].mode == 0;
    uint8_t *sb = n_streams ? C.stream_buf.as<uint8_t>(n_streams * per * 64 + 64) : nullptr; size_t off = 0;
    std::vector<ChunkNonce> cn(na);
    for (size_t k = 0; k < na; k++) {
        const rofl_nonce_t &nn = nonces[act[k]];
        cn[k] = ChunkNonce{}; cn[k].mode = nn.mode;
        if (nn.mode == 1) memcpy(cn[k].seed.w, nn.seed, 32);
        else { C.up(sb + off, nn.stream, per * 64, C.stream); cn[k].d_stream = sb + off; cn[k].stream_scalars = per; off += per * 64; }
    }
    C.sync();                                    // wait 2
    std::vector<uint8_t *> pout(na);
    for (size_t k = 0; k < na; k++) pout[k] = proofs_out[act[k]];
    // BulletproofGens::new(64, 1), label "L2RangeProof" (l2_range_proof_vec/mod.rs:156-171), one chunk of one value per client
    prove_chunks(C, "L2RangeProof", na, prove_range, 1, vshift, d_bl, cn, hV, pout.data());
    for (size_t k = 0; k < na; k++) memcpy(commits_out32 + 32 * act[k], hV + 32 * k, 32);
    timing_end(C);
    return ROFL_OK;
}
}  // namespace
int rofl_create_rangeproof_l2(const float *values, size_t d, const uint8_t *blindings32, size_t d_blindings, size_t prove_range, size_t n_partition,
                              unsigned fp_bits, unsigned fp_frac, const rofl_nonce_t *nonce, uint8_t *proof_out, size_t *proof_len_out, uint8_t commit_out[32]) {
    return guarded([&]() -> int {      // a batch of one on the caller's device (the batch entry would bind the first of the `devices` option)
        if (d != d_blindings) return fail(ROFL_WRONG_NUM_BLINDING, "WrongNumBlindingFactors");
        if (!valid_fp(fp_bits, fp_frac) || d == 0 || d >= ((size_t)1 << 28) || n_partition == 0 || prove_range == 0 || !nonce)      // (2^28: the kernel's u32 d)
            return fail(ROFL_BAD_PARAM, "bad parameter (the reference panics here)");
        int rc = ROFL_OK;
        if (int r = l2_create_batch(1, &values, d, &blindings32, prove_range, fp_bits, fp_frac, nonce, &proof_out, commit_out, &rc)) return r;
        if (rc) return fail(rc, l2_outcome_text(rc));
        *proof_len_out = 32 * (9 + 2 * (size_t)lg2u(prove_range));
        return ROFL_OK;
    });
}
int rofl_create_rangeproof_l2_batch(size_t n_clients, const float *const *values, size_t d, const uint8_t *const *blindings32, size_t prove_range, size_t n_partition,
                                    unsigned fp_bits, unsigned fp_frac, const rofl_nonce_t *nonces, uint8_t *const *proofs_out, size_t *proof_len_out, uint8_t *commits_out32, int *rc_out) {
    // (everything here is decided before a device is touched)
    if (!valid_fp(fp_bits, fp_frac) || d == 0 || d >= ((size_t)1 << 28) || n_partition == 0 || prove_range == 0 || prove_range > 128 || 2 * n_clients > kMaxBatchMembers)
        return fail(ROFL_BAD_PARAM, "bad parameter");
    if (!values || !blindings32 || !nonces || !proofs_out || !proof_len_out || !commits_out32 || !rc_out) return fail(ROFL_BAD_PARAM, "bad parameter");
    for (size_t i = 0; i < n_clients; i++)
        if (!values[i] || !blindings32[i] || !proofs_out[i] || (nonces[i].mode == 0 && nonces[i].stream_scalars && !nonces[i].stream)) return fail(ROFL_BAD_PARAM, "bad parameter");
    *proof_len_out = 32 * (9 + 2 * (size_t)lg2u(prove_range));
    if (n_clients == 0) return ROFL_OK;
    return over_devices(n_clients, nullptr, [&](const Share &sh) -> int {
        auto v = sh.view(values); auto b = sh.view(blindings32); auto nn = sh.view(nonces); auto po = sh.view(proofs_out); auto co = sh.out(commits_out32, 32); auto rc = sh.out(rc_out);
        int r = l2_create_batch(sh.size(), v.data(), d, b.data(), prove_range, fp_bits, fp_frac, nn.data(), po.data(), co.data(), rc.data());
        sh.scatter(rc);
        sh.scatter(co, [&](size_t j) { return rc.data()[j] == ROFL_OK && r == ROFL_OK; });      // a commitment only for a member that succeeded in a share that succeeded (unlike the Sigma verifier's sums)
        return r; });
}
int rofl_verify_rangeproof_l2(const uint8_t *proof, size_t proof_len, const uint8_t commit[32], size_t prove_range, unsigned fp_bits, unsigned fp_frac,
                              const uint8_t verifier_seed[32], int *ok_out) {
    return guarded([&]() -> int {
        LaneLock lane_lock = acquire_lane(false, true); Ctx &C = *lane_lock.c;
        *ok_out = 0;
        if (!valid_fp(fp_bits, fp_frac) || prove_range == 0) return fail(ROFL_BAD_PARAM, "bad parameter");
        C.init();
        timing_begin(C);
        uint8_t *d_in = C.Cbytes.as<uint8_t>(32), *d_enc = C.Vbytes.as<uint8_t>(32);
        niels *d_vn = C.gbuf[0].as<niels>(1);
        u32 *status = C.status.as<u32>(4);
        HIPCHK(hipMemsetAsync(status, 0, 16, C.stream));
        HIPCHK(hipMemcpyAsync(d_in, commit, 32, hipMemcpyHostToDevice, C.stream));
        count_decodes(1);
        ROFL_LAUNCH(k_decode, grid1(1), dim3(TPB), 0, C.stream, 1u, 1u, d_in, (const niels *)nullptr, d_vn, d_enc, status);
        uint8_t hV[32]; u32 st = 0;
        HIPCHK(hipMemcpyAsync(hV, d_enc, 32, hipMemcpyDeviceToHost, C.stream));
        HIPCHK(hipMemcpyAsync(&st, status, 4, hipMemcpyDeviceToHost, C.stream));
        C.sync();
        if (st & 4u) return fail(ROFL_FORMAT_ERROR, "commitment is not a valid Ristretto encoding");
        u64 cidx = 0; int ok = 0;
        int rc = verify_chunks(C, "L2RangeProof", 64, 1, prove_range, 1, proof, proof_len, hV, d_vn, verifier_seed, &cidx, &ok);
        timing_end(C);
        if (rc) return fail(rc, "proof rejected before verification (format / bitsize)");
        *ok_out = ok;
        return ROFL_OK;
    });
}

// verify_rangeproof_l2 for the clients of a round (params.rs:220-231, server.rs:656-687): n_clients one-value proofs over the (64, 1)
// generators, commitments = each client's sum of c_sq.  The proofs share the generators, so with verify_batch = 2 they are ONE
// random-weighted equation (a closer look only when it fails); with 1 one check per client, all in one launch sequence.  Per-client
// verdicts either way; a malformed member (length is per call; non-canonical scalar, undecodable commitment, identity point) fails alone.
int rofl_verify_rangeproof_l2_batch(size_t n_clients, const uint8_t *const *proofs, size_t proof_len, const uint8_t *commits32, size_t prove_range,
                                    unsigned fp_bits, unsigned fp_frac, const uint8_t verifier_seed[32], int *ok_out) {
    if (!ok_out || !verifier_seed || (n_clients && (!proofs || !commits32))) return fail(ROFL_BAD_PARAM, "bad parameter");
    return guarded([&]() -> int {
        LaneLock lane_lock = acquire_lane(false, true); Ctx &C = *lane_lock.c;
        for (size_t i = 0; i < n_clients; i++) ok_out[i] = 0;
        if (!valid_fp(fp_bits, fp_frac) || prove_range == 0) return fail(ROFL_BAD_PARAM, "bad parameter");
        if (n_clients == 0) return ROFL_OK;
        if (proof_len % 32 != 0 || proof_len < 7 * 32) return fail(ROFL_FORMAT_ERROR, "FormatError: proof length");
        const size_t ne = (proof_len - 7 * 32) / 32;
        if (ne < 2 || (ne - 2) % 2 != 0 || (ne - 2) / 2 >= 32) return fail(ROFL_FORMAT_ERROR, "FormatError: proof length");
        const size_t lg = (ne - 2) / 2, nc = n_clients;
        if (nc > kMaxBatchMembers / 2) return fail(ROFL_BAD_PARAM, "batch too large (split it)");      // a member = a row of gridDim.y
        std::vector<uint8_t> pf(nc * proof_len);
        std::vector<char> skip(nc, 0);
        for (size_t i = 0; i < nc; i++) {
            if (is_device_ptr(proofs[i])) HIPCHK(hipMemcpy(&pf[i * proof_len], proofs[i], proof_len, hipMemcpyDeviceToHost)); else memcpy(&pf[i * proof_len], proofs[i], proof_len);
            uint8_t *pb = &pf[i * proof_len];
            const size_t offs[5] = {128, 160, 192, 7 * 32 + 64 * lg, 7 * 32 + 64 * lg + 32};
            for (size_t o : offs) if (!sc_is_canonical_bytes(pb + o)) { skip[i] = 1; memset(pb + o, 0, 32); }      // its own verdict: false; the others go on
        }
        if (!(prove_range == 8 || prove_range == 16 || prove_range == 32 || prove_range == 64)) return fail(ROFL_INVALID_BITSIZE, "proof rejected before verification (format / bitsize)");
        if (prove_range != ((size_t)1 << lg)) return ROFL_OK;      // VerificationError for every client -> false
        C.init();
        C.batch_mode = nc > 1;
        timing_begin(C);
        uint8_t *d_in = C.Cbytes.as<uint8_t>(nc * 32), *d_enc = C.Vbytes.as<uint8_t>(nc * 32);
        niels *d_vn = C.gbuf[0].as<niels>(nc);
        u32 *status = C.status.as<u32>(nc + 4);
        HIPCHK(hipMemsetAsync(status, 0, 4 * (nc + 4), C.stream));
        C.up(d_in, commits32, nc * 32, C.stream);
        count_decodes(nc);
        ROFL_LAUNCH(k_decode, grid1(1, (u32)nc), dim3(TPB), 0, C.stream, 1u, 1u, d_in, (const niels *)nullptr, d_vn, d_enc, status);
        uint8_t *hV = C.h_V.as<uint8_t>(nc * 32); u32 *h_st = C.h_misc.as<u32>(nc + 4);
        HIPCHK(hipMemcpyAsync(hV, d_enc, nc * 32, hipMemcpyDeviceToHost, C.stream));
        HIPCHK(hipMemcpyAsync(h_st, status, 4 * nc, hipMemcpyDeviceToHost, C.stream));
        C.sync();
        for (size_t i = 0; i < nc; i++) if (h_st[i] & 4u) skip[i] = 1;
        std::vector<u64> cidx(nc, 0), ridx(nc); std::vector<int> okc(nc, 0);
        for (size_t i = 0; i < nc; i++) ridx[i] = (u64)i << 24;
        const bool hier = opts().verify_batch.load() == 2 && nc > 1;
        int rc = verify_chunks(C, "L2RangeProof", 64, nc, prove_range, 1, pf.data(), proof_len, hV, d_vn, verifier_seed, cidx.data(), okc.data(), 1, nullptr, nullptr,
                               ridx.data(), hier, skip.data());
        timing_end(C);
        if (rc) return fail(rc, "proof rejected before verification (format / bitsize)");
        for (size_t i = 0; i < nc; i++) ok_out[i] = skip[i] ? 0 : okc[i];
        return ROFL_OK;
    });
}

namespace {
DMerlin sigma_init_state(int kind) {
    const char *lbl = kind == 0 ? "RandProof" : (kind == 1 ? "SquareRandProof" : "SquareProof");
    Merlin t(lbl, strlen(lbl));
    // rand_proof_domain_sep (rand_proof/transcript.rs:20-22) -- but the begin_op of the NEXT append depends on pos_begin,
    // so the whole state (bytes, pos, pos_begin) is handed to the kernel
    t.append("dom-sep", (const uint8_t *)"randomness proof v1", 19);
    DMerlin d; memcpy(d.st, t.b(), 200); d.pos = t.pos; d.pos_begin = t.pos_begin;
    return d;
}
// [elem_first, elem_first + d) of a vector of d_all elements (d_all = 0: the whole vector): the elements of a Sigma-proof vector are independent
// of each other (rand_proof_vec/mod.rs:45-58, square_rand_proof_vec/mod.rs:45-58: one proof per element on the rayon pool), so a device or a
// rank can take any run of them -- SURVEY 8(e), the third unit of independence.  The arrays passed in are the RUN's (values, r1, r2, existing
// and both outputs start at the run's first element); the nonce index space stays the vector's (element i draws from nn * i), so the bytes
// are those of the unsplit call.
int sigma_create(int kind, const float *values, size_t d, const uint8_t *r1, size_t d_r1, const uint8_t *r2, const uint8_t *existing,
                 unsigned fp_bits, unsigned fp_frac, const rofl_nonce_t *nonce, uint8_t *proofs_out, uint8_t *commits_out, size_t elem_first = 0, size_t d_all = 0) {
    LaneLock lane_lock = acquire_lane(false, true); Ctx &C = *lane_lock.c;
    if (d != d_r1) return fail(ROFL_WRONG_NUM_BLINDING, "WrongNumBlindingFactors");
    if (!valid_fp(fp_bits, fp_frac) || !nonce) return fail(ROFL_BAD_PARAM, "bad parameter");
    if (d_all == 0) { d_all = d; elem_first = 0; }
    if (elem_first > d_all || d > d_all - elem_first) return fail(ROFL_BAD_PARAM, "element range outside the vector");
    bool has_sq = kind != 0;
    size_t npts = 1 + (kind != 2) + (has_sq ? 1 : 0), nn = has_sq ? 3 : 2, clen = 32 * npts, plen = 32 * (npts + nn);
    if (nonce->mode == 0 && nonce->stream_scalars < nn * d_all) return fail(ROFL_NONCE_SHORT, "nonce stream too short");
    if (d == 0) return ROFL_OK;
    C.init();
    timing_begin(C);
    float *dv = C.vals.as<float>(d); sc *dr1 = C.tmp_in.as<sc>(d); sc *dr2 = has_sq ? C.tmp_in2.as<sc>(d) : nullptr;
    uint8_t *dex = existing ? C.Cbytes.as<uint8_t>(d * 32) : nullptr;
    uint8_t *dp = C.aux_pts.as<uint8_t>(d * plen), *dc = C.aux_scal.as<uint8_t>(d * clen);
    u32 *status = C.status.as<u32>(4);
    HIPCHK(hipMemsetAsync(status, 0, 16, C.stream));
    C.up(dv, values, 4 * d, C.stream);
    C.up(dr1, r1, 32 * d, C.stream);
    if (has_sq) C.up(dr2, r2, 32 * d, C.stream);
    if (dex) C.up(dex, existing, 32 * d, C.stream);
    NonceSeed seed{}; const uint8_t *d_stream = nullptr; u64 ss = 0;
    const u64 nonce_base = (u64)nn * elem_first;
    if (nonce->mode == 1) memcpy(seed.w, nonce->seed, 32);
    else {      // only the run's part of the stream goes up; the kernels index it by the vector's nonce index, so the base address is moved back by what stayed behind
        const size_t run_bytes = nn * d * 64, run_off = (size_t)nonce_base * 64;
        uint8_t *sb = C.stream_buf.as<uint8_t>(run_bytes + 64); C.up(sb, nonce->stream + run_off, run_bytes, C.stream);
        d_stream = reinterpret_cast<const uint8_t *>(reinterpret_cast<uintptr_t>(sb) - run_off); ss = nonce_base + nn * d; }
    // algorithmic work per element AS BUILT: fixed-base multiplications of 32 mixed additions (radix-256 tables) -- L, L' and c_sq, c_sq' two each,
    // R, R' one each -- and 2 * npts encodings; bytes as SURVEY 8(d): value + randomness in, commitments + proof out
    const uint64_t sg_muls = (uint64_t)(4 + (kind != 2 ? 2 : 0) + (has_sq ? 4 : 0)) * 32 * 7 + 2 * npts * 265;
    { KSpan ks_sigma(C.tm, C.stream, ROFL_TK_SIGMA, (uint64_t)d * sg_muls, (uint64_t)d * (4 + 32 * (has_sq ? 2 : 1) + clen + plen));
      // one thread per point (blockIdx.y = slot), then transcripts + responses per element
      SgSlots sl{}; auto add = [&](int id) { sl.id[sl.n++] = id; };
      // c_sq' in its fixed-base form (SG_CSQP_F: the prover knows the opening of L); a commitment handed in is compared with m B + r1 Bb first
      // (SG_LCMP) and the elements where it differs -- none, unless the caller's commitments are not the values' -- are redone by
      // k_sigma_point_var exactly as the reference computes them
      uint8_t *marks = nullptr;
      if (has_sq && dex) marks = C.vspart.as<uint8_t>(d);      // (written for every element by the SG_LCMP slot: no clearing)
      if (!dex) add(SG_L); else add(has_sq ? SG_LCMP : SG_LCHK);
      if (has_sq) { add(SG_CSQP_F); add(SG_CSQ); }
      add(SG_LP);
      if (kind != 2) { add(SG_R); add(SG_RP); }
      ROFL_LAUNCH(k_sigma_points, dim3((unsigned)((d + 63) / 64), (unsigned)sl.n), dim3(64), 0, C.stream, kind, sl, (u32)d, dv, fp_bits, fp_frac, dr1, dr2, dex,
                  nonce->mode, seed, d_stream, ss, nonce_base, C.d_tabB8, C.d_tabBb8, dp, dc, status, marks);
      if (marks)
          ROFL_LAUNCH(k_sigma_point_var, dim3((unsigned)std::min<size_t>((d + 63) / 64, 256)), dim3(64), 0, C.stream, kind, (u32)d, dv, fp_bits, fp_frac, dr1, dr2, dex,      // (walks the marks: one block per CU at most)
                      nonce->mode, seed, d_stream, ss, nonce_base, C.d_tabB, C.d_tabBb, dp, dc, status, marks);
      ROFL_LAUNCH(k_sigma_finish, grid1(d), dim3(TPB), 0, C.stream, kind, (u32)d, dv, fp_bits, fp_frac, dr1, dr2, dex, nonce->mode, seed, d_stream, ss, nonce_base,
                  sigma_init_state(kind), dp, dc, status); }
    u32 st = 0;
    C.down(proofs_out, dp, d * plen, C.stream);
    C.down(commits_out, dc, d * clen, C.stream);
    HIPCHK(hipMemcpyAsync(&st, status, 4, hipMemcpyDeviceToHost, C.stream));
    C.sync();
    timing_end(C);
    if (st & 2u) return fail(ROFL_NON_FINITE, "non-finite value (the reference panics in fixed::saturating_from_float)");
    if (st & 4u) return fail(ROFL_FORMAT_ERROR, "invalid Ristretto encoding");
    return ROFL_OK;
}
// sigma_create for the clients of one process (the reference's client binary runs its clients as tasks of one process, client.rs:265-266):
// the vectors of a GROUP of clients are one launch of each of the three kernels, the client on a grid dimension of its own
// (k_sigma_points_batch and its companions read what varies by client from an SgClient descriptor on the device).  5 000 elements alone
// are 79 waves per slot on 1 024 SIMDs; a group fills the chip and pays the launches, the status hop and the wait once.  rcs[i] is client i's
// own outcome as sigma_create reports it (NaN 10 before an undecodable commitment 5; a mode-0 stream shorter than nn d scalars 12 -- that
// one before any device work) and a client that fails is left out: its output arrays are not written.
// Groups: at most sixteen clients and ~64 MB of staged bytes (kind 1: 100 d in, 288 d out per client -- three clients at d = 55 000; explicit
// nonce streams count too).  Per group: every input array is staged on the host pool and goes up with one copy per run of host clients
// (device-resident arrays are copied on the device), the descriptors go up, the three launches run, proofs, commitments and status words
// come down into pinned memory.  ONE WAIT per group (the event after its download); the pool then hands the group's bytes to the callers'
// arrays.  Two sets of device and staging buffers alternate: group g + 1 is staged, uploaded and launched BEFORE the host waits for group g,
// so the device computes it while group g comes down and is handed over.
constexpr size_t kSigmaCreateGroup = 16;
int sigma_create_batch(int kind, size_t nc, const float *const *values, size_t d, const uint8_t *const *r1, const uint8_t *const *r2, const uint8_t *const *existing,
                       unsigned fp_bits, unsigned fp_frac, const rofl_nonce_t *nonces, uint8_t *const *proofs_out, uint8_t *const *commits_out, int *rcs) {
    const bool has_sq = kind != 0;
    const size_t npts = 1 + (kind != 2) + (has_sq ? 1 : 0), nn = has_sq ? 3 : 2, clen = 32 * npts, plen = 32 * (npts + nn);
    std::vector<size_t> act;      // the clients that reach the device
    for (size_t i = 0; i < nc; i++) {
        rcs[i] = nonces[i].mode == 0 && nonces[i].stream_scalars < nn * d ? ROFL_NONCE_SHORT : ROFL_OK;
        if (!rcs[i]) act.push_back(i);
    }
    if (act.empty() || d == 0) return ROFL_OK;
    LaneLock lane_lock = acquire_lane(false, nc == 1); Ctx &C = *lane_lock.c;
    C.init();
    C.batch_mode = nc > 1;
    timing_begin(C);
    const size_t na = act.size();
    std::vector<char> dev_v(na), dev_r1(na), dev_r2(na), dev_e(na), dev_s(na), has_e(na), has_s(na);
    bool any_host = false, any_e = false, any_s = false;
    for (size_t a = 0; a < na; a++) {
        const size_t i = act[a];
        has_e[a] = existing && existing[i]; has_s[a] = nonces[i].mode == 0;
        dev_v[a] = is_device_ptr(values[i]); dev_r1[a] = is_device_ptr(r1[i]); dev_r2[a] = has_sq && is_device_ptr(r2[i]);
        dev_e[a] = has_e[a] && is_device_ptr(existing[i]); dev_s[a] = has_s[a] && is_device_ptr(nonces[i].stream);
        any_host |= !dev_v[a] || !dev_r1[a] || (has_sq && !dev_r2[a]) || (has_e[a] && !dev_e[a]) || (has_s[a] && !dev_s[a]);
        any_e |= (bool)has_e[a]; any_s |= (bool)has_s[a];
    }
    // staged bytes of a client: values | r1 | r2 | commitments handed in | nonce stream, and its proofs | commitments
    const size_t o_r1 = 4 * d, o_r2 = o_r1 + 32 * d, o_ex = o_r2 + (has_sq ? 32 * d : 0), o_st = o_ex + 32 * d, per_s = any_s ? nn * d * 64 : 0;
    const size_t in_per = o_st + per_s, out_per = d * (plen + clen);
    const size_t G = std::max<size_t>(1, std::min<size_t>(std::min<size_t>(na, kSigmaCreateGroup), ((size_t)64 << 20) / (in_per + out_per)));
    const size_t ngroups = (na + G - 1) / G, nbuf = ngroups > 1 ? 2 : 1;
    float *dv = C.vals.as<float>(nbuf * G * d); sc *dr1 = C.tmp_in.as<sc>(nbuf * G * d); sc *dr2 = has_sq ? C.tmp_in2.as<sc>(nbuf * G * d) : nullptr;
    uint8_t *dex = any_e ? C.Cbytes.as<uint8_t>(nbuf * G * d * 32) : nullptr, *dst = any_s ? C.stream_buf.as<uint8_t>(nbuf * G * per_s + 64) : nullptr;
    uint8_t *dout = C.aux_pts.as<uint8_t>(nbuf * G * out_per);      // per buffer set: [G][d] proofs | [G][d] commitments
    uint8_t *marks = has_sq && any_e ? C.vspart.as<uint8_t>(nbuf * G * d) : nullptr;      // (written for every element by the SG_LCMP slot: no clearing)
    SgClient *dcl = C.tmp_out.as<SgClient>(nbuf * G), *hcl = C.h_misc2.as<SgClient>(nbuf * G);
    u32 *status = C.status.as<u32>(na + 4), *h_st = C.h_misc.as<u32>(na + 4);
    HIPCHK(hipMemsetAsync(status, 0, 4 * (na + 4), C.stream));
    uint8_t *stg_in[2] = {nullptr, nullptr}, *stg_out[2] = {nullptr, nullptr};
    for (size_t b = 0; b < nbuf; b++) { if (any_host) stg_in[b] = (uint8_t *)C.stg.alloc(G * in_per); stg_out[b] = (uint8_t *)C.stg.alloc(G * out_per); }
    SgSlots sl{}; auto add = [&](int id) { sl.id[sl.n++] = id; };      // the slots of a client WITHOUT a commitment handed in; with one, SG_L becomes SG_LCMP / SG_LCHK in the kernel
    add(SG_L);
    if (has_sq) { add(SG_CSQP_F); add(SG_CSQ); }
    add(SG_LP);
    if (kind != 2) { add(SG_R); add(SG_RP); }
    const DMerlin init = sigma_init_state(kind);
    const uint64_t sg_muls = (uint64_t)(4 + (kind != 2 ? 2 : 0) + (has_sq ? 4 : 0)) * 32 * 7 + 2 * npts * 265;
    auto enqueue = [&](size_t g) {      // upload, the three launches, download of group g in buffer set g & 1; event g & 1 marks the end
        const size_t a0 = g * G, gc = std::min(G, na - a0), b = g & (nbuf - 1);
        uint8_t *si = stg_in[b];
        auto sub = [&](size_t o) { return si ? si + G * o : nullptr; };      // (array by array: [G] values, [G] r1, ...)
        float *gv = dv + b * G * d; sc *gr1 = dr1 + b * G * d, *gr2 = dr2 ? dr2 + b * G * d : nullptr;
        uint8_t *gex = dex ? dex + b * G * d * 32 : nullptr, *gst = dst ? dst + b * G * per_s : nullptr, *gp = dout + b * G * out_per, *gc_ = gp + G * d * plen;
        uint8_t *gm = marks ? marks + b * G * d : nullptr;
        bring_group(C, gc, (uint8_t *)gv, sub(0), 4 * d, [&](size_t j) { return (const uint8_t *)values[act[a0 + j]]; }, [&](size_t j) { return (bool)dev_v[a0 + j]; });
        bring_group(C, gc, (uint8_t *)gr1, sub(o_r1), 32 * d, [&](size_t j) { return r1[act[a0 + j]]; }, [&](size_t j) { return (bool)dev_r1[a0 + j]; });
        if (has_sq) bring_group(C, gc, (uint8_t *)gr2, sub(o_r2), 32 * d, [&](size_t j) { return r2[act[a0 + j]]; }, [&](size_t j) { return (bool)dev_r2[a0 + j]; });
        if (gex) bring_group(C, gc, gex, sub(o_ex), 32 * d, [&](size_t j) { return has_e[a0 + j] ? existing[act[a0 + j]] : nullptr; }, [&](size_t j) { return (bool)dev_e[a0 + j]; });
        if (gst) bring_group(C, gc, gst, sub(o_st), per_s, [&](size_t j) { return has_s[a0 + j] ? nonces[act[a0 + j]].stream : nullptr; }, [&](size_t j) { return (bool)dev_s[a0 + j]; });
        bool var = false;
        for (size_t j = 0; j < gc; j++) {
            const rofl_nonce_t &nz = nonces[act[a0 + j]];
            SgClient c{}; c.mode = nz.mode; c.has_existing = has_e[a0 + j] ? 1u : 0u;
            if (nz.mode == 1) memcpy(c.seed.w, nz.seed, 32); else { c.stream = gst + j * per_s; c.stream_scalars = nn * d; }
            c.vals = gv + j * d; c.r1c = gr1 + j * d; c.r2c = gr2 ? gr2 + j * d : nullptr; c.existing = gex ? gex + j * d * 32 : nullptr;
            c.proofs = gp + j * d * plen; c.commits = gc_ + j * d * clen; c.slow_mark = gm ? gm + j * d : nullptr;
            hcl[b * G + j] = c; var |= has_sq && has_e[a0 + j];
        }
        HIPCHK(hipMemcpyAsync(dcl + b * G, hcl + b * G, sizeof(SgClient) * gc, hipMemcpyHostToDevice, C.stream));
        { KSpan ks_sigma(C.tm, C.stream, ROFL_TK_SIGMA, (uint64_t)gc * d * sg_muls, (uint64_t)gc * d * (4 + 32 * (has_sq ? 2 : 1) + clen + plen));
          ROFL_LAUNCH(k_sigma_points_batch, dim3((unsigned)((d + 63) / 64), (unsigned)sl.n, (unsigned)gc), dim3(64), 0, C.stream, kind, sl, (u32)d, fp_bits, fp_frac, (const SgClient *)(dcl + b * G),
                      C.d_tabB8, C.d_tabBb8, status + a0);
          if (var)
              ROFL_LAUNCH(k_sigma_point_var_batch, dim3((unsigned)std::min<size_t>((d + 63) / 64, 256), (unsigned)gc), dim3(64), 0, C.stream, kind, (u32)d, fp_bits, fp_frac, (const SgClient *)(dcl + b * G),
                          C.d_tabB, C.d_tabBb, status + a0);
          ROFL_LAUNCH(k_sigma_finish_batch, grid1(d, (u32)gc), dim3(TPB), 0, C.stream, kind, (u32)d, fp_bits, fp_frac, (const SgClient *)(dcl + b * G), init, status + a0); }
        HIPCHK(hipMemcpyAsync(stg_out[b], gp, gc * d * plen, hipMemcpyDeviceToHost, C.stream));
        HIPCHK(hipMemcpyAsync(stg_out[b] + G * d * plen, gc_, gc * d * clen, hipMemcpyDeviceToHost, C.stream));
        HIPCHK(hipMemcpyAsync(h_st + a0, status + a0, 4 * gc, hipMemcpyDeviceToHost, C.stream));
        HIPCHK(hipEventRecord(C.pool_event(b), C.stream));
    };
    enqueue(0);
    for (size_t g = 0; g < ngroups; g++) {
        const size_t a0 = g * G, gc = std::min(G, na - a0), b = g & (nbuf - 1);
        if (g + 1 < ngroups) enqueue(g + 1);      // (its buffers are those of group g - 1, which is finished)
        C.wait_event(C.pool_event(b));           // the group's one wait: proofs, commitments and status words are on the host
        std::vector<size_t> good;                // positions in the group
        for (size_t j = 0; j < gc; j++) {
            const u32 st = h_st[a0 + j];
            rcs[act[a0 + j]] = (st & 2u) ? ROFL_NON_FINITE : (st & 4u) ? ROFL_FORMAT_ERROR : ROFL_OK;
            if (!(st & 6u)) good.push_back(j);
        }
        if (good.empty()) continue;
        const uint8_t *hp = stg_out[b], *hc = stg_out[b] + G * d * plen;
        const size_t sp = std::max<size_t>(1, (d * plen) >> 18), sc_ = std::max<size_t>(1, (d * clen) >> 18);
        C.pool->run(good.size() * (sp + sc_), [&](size_t t) {
            const size_t j = good[t / (sp + sc_)], i = act[a0 + j]; size_t k = t % (sp + sc_);
            if (k < sp) { const size_t lo = d * plen * k / sp, hi = d * plen * (k + 1) / sp; memcpy(proofs_out[i] + lo, hp + j * d * plen + lo, hi - lo); }
            else { k -= sp; const size_t lo = d * clen * k / sc_, hi = d * clen * (k + 1) / sc_; memcpy(commits_out[i] + lo, hc + j * d * clen + lo, hi - lo); } });
    }
    timing_end(C);
    return ROFL_OK;
}
// Verification of the per-element Sigma-proofs of `nc` vectors of d elements (the clients of a round: the reference's server verifies every
// client's update, server.rs:656-687, each with verify_randproof_vec / verify_l2rangeproof_vec, params.rs:188-189, 208, 262).  One launch
// sequence for all of them: the clients' bytes are staged and uploaded group by group (the pool copies group g + 1 while group g is on its
// way and being decoded), k_sigma_vprep runs over (element, client), and every client is ONE problem of a multi-problem Pippenger launch --
// its own random linear combination, hence its own verdict, with no closer look needed (clients share nothing here, unlike the range
// proofs' generator MSM).  55 000 elements alone are less than one wave per SIMD; 48 clients fill the chip.
// csq_sum_out (kinds 1, 2; may be null): sum_i c_sq_i of every client, compressed (params.rs:220, 277) -- the points are decoded here anyway.
// `single`: the call is one of the rofl_verify_*_vec entry points (a malformed vector is the call's FormatError); batch calls give the
// offender ok = 0 and go on.
// rs: the commitments are the round's (`commits` is not read): their bytes are on the device for the transcripts, their points decoded in
// the even slots of the round's point array, which IS the MSM's input for kinds 0 / 1 (kind 2 reads L and c_sq of 96-byte records: a
// packing kernel for the bytes, two strided device copies for the points); only the proofs' own points are decoded here.  A client without proofs (proofs[i] null) is left out (ok = 0).
int sigma_verify_batch(int kind, size_t nc, const uint8_t *const *proofs, const uint8_t *const *commits, size_t d, int *ok_out, uint8_t *csq_sum_out, bool single,
                       const RoundSrc *rs = nullptr) {
    LaneLock lane_lock = acquire_lane(false, nc == 1); Ctx &C = *lane_lock.c;
    for (size_t i = 0; i < nc; i++) ok_out[i] = 0;
    const bool has_R = kind != 2, has_sq = kind != 0;
    if (csq_sum_out) memset(csq_sum_out, 0, 32 * nc);      // the identity (also the sum of an empty vector)
    if (nc == 0) return ROFL_OK;
    if (d == 0) { for (size_t i = 0; i < nc; i++) ok_out[i] = 1; return ROFL_OK; }
    const size_t npts = 1 + (has_R ? 1 : 0) + (has_sq ? 1 : 0), clen = 32 * npts, plen = 32 * (npts + (has_sq ? 3 : 2));
    const size_t nslots = 2 * npts, nblk = (d + TPB - 1) / TPB;
    // (the members of a batch index gridDim.y of the decode / transcript / sum kernels and the problems of the Pippenger launches: 65 535 at most)
    if (nc > kMaxBatchMembers || nc * nslots * d >= ((size_t)1 << 31) || nc * nblk > ((size_t)1 << 22)) return fail(ROFL_BAD_PARAM, "batch too large (split it)");
    C.init();
    C.batch_mode = nc > 1;
    timing_begin(C);
    if (!rs && !opts().sigma_batch.load()) {      // rofl_set_option("sigma_batch", 0): one check per element (the reference's form), client by client
        int rc_all = ROFL_OK;
        for (size_t i = 0; i < nc; i++) {
            uint8_t *dp = C.aux_pts.as<uint8_t>(d * plen), *dc = C.aux_scal.as<uint8_t>(d * clen);
            u32 *status = C.status.as<u32>(4);
            HIPCHK(hipMemsetAsync(status, 0, 16, C.stream));
            C.up(dp, proofs[i], d * plen, C.stream); C.up(dc, commits[i], d * clen, C.stream);
            count_decodes(nslots * d + (csq_sum_out && has_sq ? d : 0));
            { KSpan ks_sigma(C.tm, C.stream, ROFL_TK_SIGMA, (uint64_t)d * (2 * npts * 265 + (kind ? 3 : 2) * 2 * 325 * 8), (uint64_t)d * (clen + plen));
              ROFL_LAUNCH(k_sigma_verify, dim3((unsigned)((d + 63) / 64)), dim3(64), 0, C.stream, kind, (u32)d, dp, dc, sigma_init_state(kind), C.d_tabB, C.d_tabBb, status + 1, status); }
            u32 *st = C.h_misc.as<u32>(4);
            HIPCHK(hipMemcpyAsync(st, status, 8, hipMemcpyDeviceToHost, C.stream));
            if (csq_sum_out && has_sq) {
                u32 nb2 = (u32)std::min<size_t>(64, nblk); ge *part = C.partial2.as<ge>(nb2);
                ROFL_LAUNCH(k_decode_sum, dim3(nb2), dim3(TPB), TPB * sizeof(ge), C.stream, dc + (has_R ? 64 : 32), (u32)d, (u32)clen, part, status + 2);
                ge *hp = C.h_part.as<ge>(nb2);
                HIPCHK(hipMemcpyAsync(hp, part, sizeof(ge) * nb2, hipMemcpyDeviceToHost, C.stream));
                C.sync();
                ge5 acc = h51::identity(); for (u32 k = 0; k < nb2; k++) acc = h51::gadd(acc, h51::from_ge(hp[k]));
                h51::encode(csq_sum_out + 32 * i, acc);
            } else C.sync();
            if (st[0] & 4u) { if (single) { timing_end(C); return fail(ROFL_FORMAT_ERROR, "FormatError: non-canonical scalar or invalid point"); } if (csq_sum_out) memset(csq_sum_out + 32 * i, 0, 32); continue; }
            ok_out[i] = st[1] == 0;
        }
        timing_end(C);
        return rc_all;
    }
    static const bool strace = knob("ROFL_TRACE") && atoi(knob("ROFL_TRACE")) >= 2;
    double st0 = now_ms(), stl = st0;
    auto smark = [&](const char *what) { if (!strace) return; double t = now_ms(); fprintf(stderr, "[rofl-trace sigma-verify] %-18s +%.3f ms  (t=%.3f)\n", what, t - stl, t - st0); stl = t; };
    const bool rs_direct = rs && clen == 32 * rs->npts;      // kinds 0 / 1: the records are the leg's commitments as they lie
    uint8_t *dp = C.aux_pts.as<uint8_t>(nc * d * plen);
    const uint8_t *dc = rs_direct ? rs->rec : C.aux_scal.as<uint8_t>(nc * d * clen);
    u32 *status = C.status.as<u32>(nc + 4);
    HIPCHK(hipMemsetAsync(status, 0, 4 * (nc + 4), C.stream));
    NonceSeed ws{};
    { FILE *f = fopen("/dev/urandom", "rb"); bool got = f && fread(ws.w, 1, 32, f) == 32; if (f) fclose(f);
      if (!got) return fail(ROFL_HIP_ERROR, "no randomness for the batched Sigma-proof check"); }
    niels *pts = rs_direct ? rs->pts : C.gbuf[0].as<niels>(nc * nslots * d);
    if (rs && !rs_direct) {      // kind 2 over 96-byte records: (L, c_sq) of every record packed for the transcripts, their cached points into slots 0 / 2
        uint8_t *pk = const_cast<uint8_t *>(dc);
        ROFL_LAUNCH(k_round_pack_lcsq, grid1(nc * d), dim3(TPB), 0, C.stream, (u32)(nc * d), rs->rec, pk);
        HIPCHK(hipMemcpy2DAsync(pts, 4 * d * sizeof(niels), rs->pts, 6 * d * sizeof(niels), d * sizeof(niels), nc, hipMemcpyDeviceToDevice, C.stream));
        HIPCHK(hipMemcpy2DAsync(pts + 2 * d, 4 * d * sizeof(niels), rs->pts + 4 * d, 6 * d * sizeof(niels), d * sizeof(niels), nc, hipMemcpyDeviceToDevice, C.stream));
    }
    const size_t cup = rs ? 0 : clen;      // commitment bytes per element that this call brings in
    sc *scal = C.SL.as<sc>(nc * nslots * d);
    sc *d_fixed = C.tmp_out.as<sc>(nc * nblk * 2);
    const DMerlin init = sigma_init_state(kind);
    // the weights' size: their top bit must not be the top bit of a window of the layout the MSM will use (see k_sigma_vprep)
    static const u32 wbits = [] {      // (whichever of the generic layouts the MSM driver ends up with, retries included)
        for (u32 cand = 127; cand > 96; cand--) {
            bool hit = false;
            for (u32 c : {4u, 7u, 10u, 13u, 16u}) { MsmPlan mp = msm_plan_c(c); for (u32 w = 0, end = 0; w < mp.W; w++) { end += w + 1 == mp.W ? mp.c + 1 : (w < mp.wide ? mp.c : mp.c - 1); hit |= end == cand; } }
            if (!hit) return cand;
        }
        return 96u; }();
    // groups of clients: ~64 MB of caller bytes each, through two staging buffers
    const size_t per = d * (plen + cup);
    const size_t G = std::max<size_t>(1, std::min<size_t>(std::min<size_t>(nc, 16), ((size_t)64 << 20) / per));      // (at most sixteen: a group is also a row count of gridDim.y and part of one Pippenger launch)
    bool all_host = true; for (size_t i = 0; i < nc; i++) all_host &= !is_device_ptr(proofs[i]) && (rs || !is_device_ptr(commits[i]));
    // three staging buffers; the uploads run on a stream of their own (the copy of group g + 1 beside the kernels of group g: on one stream they
    // alternated, and the "staging" time of the first version was the host waiting for that stream)
    constexpr size_t NST = 3;
    uint8_t *stage[NST] = {nullptr, nullptr, nullptr}; bool used[NST] = {false, false, false};
    if (all_host && per >= Stage::kMin) for (size_t b = 0; b < NST && b * G < nc; b++) stage[b] = (uint8_t *)C.stg.alloc(G * per);
    if (stage[0] && !C.stream_up) HIPCHK(hipStreamCreateWithFlags(&C.stream_up, hipStreamNonBlocking));
    struct JoinUp { hipStream_t s; ~JoinUp() { if (s) (void)hipStreamSynchronize(s); } } join_up{stage[0] ? C.stream_up : nullptr};
    // events of the call: 0..2 upload of staging buffer b done, 3 / 4 a launch's clients decoded, 5 / 6 a launch finished
    if (stage[0]) { HIPCHK(hipEventRecord(C.pool_event(7), C.stream)); HIPCHK(hipStreamWaitEvent(C.stream_up, C.pool_event(7), 0)); }      // (after the status memset)
    // Every client is one problem of a multi-problem Pippenger launch; launches of 16 to 31 clients (whole decode groups; the slot array of a launch grows with
    // its problems) go to the SIDE stream as soon as their clients are decoded, so that they run while the host is still staging and the main
    // stream still uploading and decoding the later clients.  Two MSM workspaces alternate: launch k + 2 waits for launch k's results.
    if (!C.stream2) HIPCHK(hipStreamCreateWithFlags(&C.stream2, hipStreamNonBlocking));
    struct Join { hipStream_t s; ~Join() { (void)hipStreamSynchronize(s); } } join{C.stream2};      // nothing of the side stream outlives the call, error paths included
    struct Job { size_t c0, cnt; MsmJob J; MsmAllow al; std::vector<MsmProb> pr; std::vector<ge5> res; bool done = false, redo = false; };
    std::vector<std::unique_ptr<Job>> jobs;
    const size_t SGC = 16;
    auto finish_job = [&](Job &jb, size_t k) {
        C.wait_event(C.pool_event(5 + (k & 1)));
        if (msm_retry(jb.J, jb.al)) jb.redo = true;      // a fixed-size structure overflowed (scalars built to collide): repeated on its own after the pipeline
        else msm_finish(C, jb.J, jb.res, MsmOpt());
        jb.done = true;
    };
    auto launch_job = [&](size_t c0, size_t cnt) {
        const size_t k = jobs.size();
        if (k >= 2 && !jobs[k - 2]->done) finish_job(*jobs[k - 2], k - 2);      // its workspace is taken over
        std::unique_ptr<Job> jb(new Job()); jb->c0 = c0; jb->cnt = cnt; jb->pr.resize(cnt);
        for (size_t q = 0; q < cnt; q++) jb->pr[q] = MsmProb{pts + (c0 + q) * nslots * d, scal + (c0 + q) * nslots * d};
        C.tm.t.msm_terms += cnt * nslots * d;
        HIPCHK(hipEventRecord(C.pool_event(3 + (k & 1)), C.stream));                 // the clients of this launch are decoded, their scalars written
        HIPCHK(hipStreamWaitEvent(C.stream2, C.pool_event(3 + (k & 1)), 0));
        jb->J = msm_enqueue(C, C.mws[k & 1], jb->pr, nslots * d, MsmOpt(), jb->al, C.stream2);
        HIPCHK(hipEventRecord(C.pool_event(5 + (k & 1)), C.stream2));
        jobs.push_back(std::move(jb));
    };
    size_t sg_start = 0;
    for (size_t g0 = 0, gi = 0; g0 < nc; g0 += G, gi++) {
        const size_t gc = std::min(G, nc - g0), b = gi % NST;
        if (stage[0]) {
            if (used[b]) C.wait_event(C.pool_event(b));      // the upload that read this buffer three groups ago
            uint8_t *sp = stage[b], *sq = stage[b] + gc * d * plen;
            const size_t sl_p = std::max<size_t>(1, (d * plen) >> 18), sl_c = cup ? std::max<size_t>(1, (d * clen) >> 18) : 0;      // ~256 KB per task
            C.pool->run(gc * (sl_p + sl_c), [&](size_t t) {
                size_t i = t / (sl_p + sl_c), k = t % (sl_p + sl_c);
                if (k < sl_p) { size_t lo = d * plen * k / sl_p, hi = d * plen * (k + 1) / sl_p;
                                if (proofs[g0 + i]) stage_copy(sp + i * d * plen + lo, proofs[g0 + i] + lo, hi - lo); else memset(sp + i * d * plen + lo, 0, hi - lo); }
                else { k -= sl_p; size_t lo = d * clen * k / sl_c, hi = d * clen * (k + 1) / sl_c; stage_copy(sq + i * d * clen + lo, commits[g0 + i] + lo, hi - lo); }
            });
            HIPCHK(hipMemcpyAsync(dp + g0 * d * plen, sp, gc * d * plen, hipMemcpyHostToDevice, C.stream_up));
            if (cup) HIPCHK(hipMemcpyAsync(const_cast<uint8_t *>(dc) + g0 * d * clen, sq, gc * d * clen, hipMemcpyHostToDevice, C.stream_up));
            HIPCHK(hipEventRecord(C.pool_event(b), C.stream_up)); used[b] = true;
            HIPCHK(hipStreamWaitEvent(C.stream, C.pool_event(b), 0));      // this group's kernels wait for its bytes
        } else
            for (size_t i = g0; i < g0 + gc; i++) {
                if (proofs[i]) C.up(dp + i * d * plen, proofs[i], d * plen, C.stream); else HIPCHK(hipMemsetAsync(dp + i * d * plen, 0, d * plen, C.stream));
                if (cup) C.up(const_cast<uint8_t *>(dc) + i * d * clen, commits[i], d * clen, C.stream); }
        {   KSpan ks_sigma(C.tm, C.stream, ROFL_TK_SIGMA, (uint64_t)gc * d * ((rs ? 1 : 2) * npts * 265), (uint64_t)gc * d * (cup + plen));      // decoding of 2 npts points per element (a round: the proofs' npts)
            count_decodes(gc * (rs ? npts : nslots) * d);
            if (rs) ROFL_LAUNCH(k_sigma_vdecode_proofs, dim3((unsigned)((npts * d + TPB - 1) / TPB), (unsigned)gc), dim3(TPB), 0, C.stream, kind, (u32)d, (const uint8_t *)(dp + g0 * d * plen),
                               pts + g0 * nslots * d, status + g0);
            else
            ROFL_LAUNCH(k_sigma_vdecode, dim3((unsigned)((nslots * d + TPB - 1) / TPB), (unsigned)gc), dim3(TPB), 0, C.stream, kind, (u32)d, dp + g0 * d * plen, dc + g0 * d * clen,
                               pts + g0 * nslots * d, status + g0);
            ROFL_LAUNCH(k_sigma_vprep, dim3((unsigned)nblk, (unsigned)gc), dim3(TPB), 0, C.stream, kind, (u32)d, dp + g0 * d * plen, dc + g0 * d * clen, init, ws, (u64)(g0 * d), wbits,
                               scal + g0 * nslots * d, d_fixed + g0 * nblk * 2, status + g0); }
        if (g0 + gc - sg_start >= SGC || g0 + gc == nc) { launch_job(sg_start, g0 + gc - sg_start); sg_start = g0 + gc; }
    }
    smark("staged + enqueued");
    sc *h_fixed = C.h_part.as<sc>(nc * nblk * 2);
    u32 *h_st = C.h_misc.as<u32>(nc + 4);
    HIPCHK(hipMemcpyAsync(h_fixed, d_fixed, sizeof(sc) * nc * nblk * 2, hipMemcpyDeviceToHost, C.stream));
    HIPCHK(hipMemcpyAsync(h_st, status, 4 * nc, hipMemcpyDeviceToHost, C.stream));
    const u32 nb2 = (u32)std::min<size_t>(64, nblk);
    ge *h_csq = nullptr;
    if (csq_sum_out && has_sq) {
        ge *part = C.partial2.as<ge>(nc * nb2);
        ROFL_LAUNCH(k_niels_sum, dim3(nb2, (unsigned)nc), dim3(TPB), TPB * sizeof(ge), C.stream, (const niels *)(pts + (nslots - 2) * d), (u32)d, nslots * d, part);
        h_csq = C.h_misc2.as<ge>(nc * nb2);
        HIPCHK(hipMemcpyAsync(h_csq, part, sizeof(ge) * nc * nb2, hipMemcpyDeviceToHost, C.stream));
    }
    C.sync();
    smark("decoded");
    for (size_t k = 0; k < jobs.size(); k++) if (!jobs[k]->done) finish_job(*jobs[k], k);
    HIPCHK(hipStreamSynchronize(C.stream2));
    for (auto &jb : jobs) if (jb->redo) { jb->res.clear(); msm_run(C, jb->pr, nslots * d, jb->res); }
    std::vector<size_t> good;
    std::vector<char> is_bad(nc, 0);
    for (size_t i = 0; i < nc; i++) {
        bool bad = (h_st[i] & 4u) != 0;
        if (rs) bad |= !proofs[i] || rs->bad[3 * i] != ~0u || (has_R && rs->bad[3 * i + 1] != ~0u) || (has_sq && rs->bad[3 * i + 2] != ~0u);      // the slots this kind reads
        if (bad) { is_bad[i] = 1; if (single) { timing_end(C); return fail(ROFL_FORMAT_ERROR, "FormatError: non-canonical scalar or invalid point"); } }
        else good.push_back(i);
    }
    for (auto &jb : jobs)
        for (size_t q = 0; q < jb->cnt; q++) {
            const size_t i = jb->c0 + q;
            if (is_bad[i]) continue;      // (its problem ran with the others -- the scalars of a malformed member are still well-formed numbers -- and its result is ignored)
            sc sB = h_canon(sum_partials(h_fixed + i * nblk * 2, nblk, 2, 0)), sBb = h_canon(sum_partials(h_fixed + i * nblk * 2, nblk, 2, 1));
            ge5 tot = h51::gadd(jb->res[q], h51::gadd(h_fixed_mul(C.ht.B5, sB), h_fixed_mul(C.ht.Bb5, sBb)));
            ok_out[i] = h51::is_identity_ristretto(tot) ? 1 : 0;
        }
    smark("msm + verdicts");
    if (h_csq) for (size_t i : good) {
        ge5 acc = h51::identity(); for (u32 k = 0; k < nb2; k++) acc = h51::gadd(acc, h51::from_ge(h_csq[i * nb2 + k]));
        h51::encode(csq_sum_out + 32 * i, acc);
    }
    timing_end(C);
    return ROFL_OK;
}
int sigma_verify(int kind, const uint8_t *proofs, const uint8_t *commits, size_t d, int *ok_out) {
    return sigma_verify_batch(kind, 1, &proofs, &commits, d, ok_out, nullptr, true);
}
// ---- compressed_rand_proof
// The CompressedRandProofs of the clients of one process (the reference's client binary runs its clients as tasks of one process,
// client.rs:265-266); the one-client call is a group of one.  rcs[i] is client i's own outcome (NaN 10 before an undecodable commitment 5; a
// mode-0 stream of fewer than two scalars 12 -- that one before any device work) and a client that fails is left out from there on.
// d alone is less than one wave per SIMD for the pairs and a handful of blocks for the dot products; the clients
// go in GROUPS of at most sixteen (gridDim.y, one bit of the pairs kernel's `existing` mask each) and at most ~64 MB of staged bytes.
// Per group: the inputs are staged on the host pool and uploaded (device-resident inputs are copied on the device), k_eg_pairs_batch
// computes every pair one thread per point, and the pairs come back into pinned memory -- they are the output and the transcripts'
// input.  While that runs the pool computes the group's nonces and C'.  WAIT 1 (the event after the download).  Then the pairs are handed
// to the callers' arrays and the transcripts of the group's good clients hashed (compressed_challenges, eight per AVX-512 stream), the
// tables c^(2^b) go up, k_cpow_dot_batch sums every client's two dot products in kCompDotBlocks blocks, the partials come down: WAIT 2.
// The upload and the pairs launch of group g + 1 are enqueued BEFORE the host turns to group g (two sets of device and staging buffers
// alternate), so the device computes the next group's pairs while the host hashes: two waits per group instead of two per client.
constexpr size_t kCompCreateGroup = 16;      // clients per launch: a row of gridDim.y and a bit of the pairs kernel's `existing` mask each
constexpr u32 kCompDotBlocks = 64;      // per client: a group of sixteen is 1 024 blocks of four waves, four waves on every SIMD of 256 CUs
int compressed_create_batch(size_t nc, const float *const *values, size_t d, const uint8_t *const *r32, const uint8_t *const *existing, unsigned fp_bits,
                            unsigned fp_frac, const rofl_nonce_t *nonces, uint8_t *const *proofs_out, uint8_t *const *pairs_out, int *rcs) {
    std::vector<size_t> act;      // the clients that reach the device
    for (size_t i = 0; i < nc; i++) {
        rcs[i] = nonces[i].mode == 0 && nonces[i].stream_scalars < 2 ? ROFL_NONCE_SHORT : ROFL_OK;
        if (!rcs[i]) act.push_back(i);
    }
    if (act.empty()) return ROFL_OK;
    LaneLock lane_lock = acquire_lane(false, nc == 1); Ctx &C = *lane_lock.c;
    C.init();
    C.batch_mode = nc > 1;
    timing_begin(C);
    const size_t na = act.size();
    // nonces m', r' at index 0, 1 of the client's own stream or seed (party.rs:66-67), C' = commit(m', r')
    std::vector<sc> nz(2 * na);
    auto nonces_and_cprime = [&](size_t a0, size_t cnt) {
        C.pool->run(cnt, [&](size_t k) {
            const size_t i = act[a0 + k]; const rofl_nonce_t &nn = nonces[i];
            for (int j = 0; j < 2; j++) {
                uint8_t b[32];
                if (nn.mode == 1) rofl_dbg_host_nonce(nn.seed, (uint64_t)j, b);
                else { sc w = sc_from_wide(sc_frombytes(nn.stream + 64 * j), sc_frombytes(nn.stream + 64 * j + 32)); sc_tobytes(b, w); }
                nz[2 * (a0 + k) + j] = sc_frombytes(b);
            }
            h51::encode(proofs_out[i], h51::gadd(h_fixed_mul(C.ht.B5, nz[2 * (a0 + k)]), h_fixed_mul(C.ht.Bb5, nz[2 * (a0 + k) + 1])));
            h51::encode(proofs_out[i] + 32, h_fixed_mul(C.ht.B5, nz[2 * (a0 + k) + 1]));
        });
    };
    if (d == 0) {      // Z = (m', r'): no device work
        nonces_and_cprime(0, na);
        for (size_t a = 0; a < na; a++) { sc_tobytes(proofs_out[act[a]] + 64, nz[2 * a]); sc_tobytes(proofs_out[act[a]] + 96, nz[2 * a + 1]); }
        timing_end(C);
        return ROFL_OK;
    }
    const size_t in_per = d * 68, out_per = d * 64;      // staged bytes of a client: values | blindings | commitments, and its pairs
    const size_t G = std::max<size_t>(1, std::min<size_t>(std::min<size_t>(na, kCompCreateGroup), ((size_t)64 << 20) / (in_per + out_per)));
    const size_t ngroups = (na + G - 1) / G, nbuf = ngroups > 1 ? 2 : 1;
    std::vector<char> dev_v(na), dev_r(na), dev_e(na), has_e(na);
    bool any_host = false;
    for (size_t a = 0; a < na; a++) {
        const size_t i = act[a];
        has_e[a] = existing && existing[i];
        dev_v[a] = is_device_ptr(values[i]); dev_r[a] = is_device_ptr(r32[i]); dev_e[a] = has_e[a] && is_device_ptr(existing[i]);
        any_host |= !dev_v[a] || !dev_r[a] || (has_e[a] && !dev_e[a]);
    }
    float *dv = C.vals.as<float>(nbuf * G * d); sc *dr = C.tmp_in.as<sc>(nbuf * G * d);
    uint8_t *dex = C.Cbytes.as<uint8_t>(nbuf * G * d * 32), *dpairs = C.aux_scal.as<uint8_t>(nbuf * G * out_per);
    u32 *status = C.status.as<u32>(na + 4), *h_st = C.h_misc.as<u32>(na + 4);
    HIPCHK(hipMemsetAsync(status, 0, 4 * (na + 4), C.stream));
    sc *dtab = C.tmp_out.as<sc>(G * (MAX_LG + 2 * kCompDotBlocks)), *dpart = dtab + G * MAX_LG;
    sc *htab = C.h_cp.as<sc>(G * MAX_LG), *hpart = C.h_part.as<sc>(G * 2 * kCompDotBlocks);
    uint8_t *stg_in[2] = {nullptr, nullptr}, *stg_out[2] = {nullptr, nullptr};
    for (size_t b = 0; b < nbuf; b++) { if (any_host) stg_in[b] = (uint8_t *)C.stg.alloc(G * in_per); stg_out[b] = (uint8_t *)C.stg.alloc(G * out_per); }
    auto enqueue = [&](size_t g) {      // upload, pairs, download of group g into buffer set g & 1; event g & 1 marks the end
        const size_t a0 = g * G, gc = std::min(G, na - a0), b = g & (nbuf - 1);
        uint8_t *si = stg_in[b];
        bring_group(C, gc, (uint8_t *)(dv + b * G * d), si, 4 * d, [&](size_t j) { return (const uint8_t *)values[act[a0 + j]]; }, [&](size_t j) { return (bool)dev_v[a0 + j]; });
        bring_group(C, gc, (uint8_t *)(dr + b * G * d), si ? si + G * 4 * d : nullptr, 32 * d, [&](size_t j) { return r32[act[a0 + j]]; }, [&](size_t j) { return (bool)dev_r[a0 + j]; });
        bring_group(C, gc, dex + b * G * d * 32, si ? si + G * 36 * d : nullptr, 32 * d, [&](size_t j) { return has_e[a0 + j] ? existing[act[a0 + j]] : nullptr; },
                    [&](size_t j) { return (bool)dev_e[a0 + j]; });
        u32 ex_mask = 0; for (size_t j = 0; j < gc; j++) if (has_e[a0 + j]) ex_mask |= 1u << j;
        ROFL_LAUNCH(k_eg_pairs_batch, dim3((unsigned)((d + 63) / 64), (unsigned)gc, 2), dim3(64), 0, C.stream, (u32)d, (const float *)(dv + b * G * d), fp_bits, fp_frac,
                    (const sc *)(dr + b * G * d), (const uint8_t *)(dex + b * G * d * 32), ex_mask, C.d_tabB8, C.d_tabBb8, dpairs + b * G * out_per, status + a0);
        HIPCHK(hipMemcpyAsync(stg_out[b], dpairs + b * G * out_per, gc * out_per, hipMemcpyDeviceToHost, C.stream));
        HIPCHK(hipMemcpyAsync(h_st + a0, status + a0, 4 * gc, hipMemcpyDeviceToHost, C.stream));
        HIPCHK(hipEventRecord(C.pool_event(b), C.stream));
    };
    enqueue(0);
    for (size_t g = 0; g < ngroups; g++) {
        const size_t a0 = g * G, gc = std::min(G, na - a0), b = g & (nbuf - 1);
        if (g + 1 < ngroups) enqueue(g + 1);      // (its buffers are those of group g - 1, which is finished)
        nonces_and_cprime(a0, gc);
        C.wait_event(C.pool_event(b));           // wait 1: the group's pairs and status words are on the host
        std::vector<size_t> good;                // positions in the group
        for (size_t j = 0; j < gc; j++) {
            const u32 st = h_st[a0 + j];
            rcs[act[a0 + j]] = (st & 2u) ? ROFL_NON_FINITE : (st & 4u) ? ROFL_FORMAT_ERROR : ROFL_OK;
            if (!(st & 6u)) good.push_back(j);
        }
        if (good.empty()) continue;
        const uint8_t *hp = stg_out[b];
        const size_t slices = std::max<size_t>(1, out_per >> 18);
        C.pool->run(good.size() * slices, [&](size_t t) { const size_t j = good[t / slices], k = t % slices, lo = out_per * k / slices, hi = out_per * (k + 1) / slices;
                                                          memcpy(pairs_out[act[a0 + j]] + lo, hp + j * out_per + lo, hi - lo); });
        std::vector<const uint8_t *> pf(good.size()), pr(good.size()); std::vector<sc> c(good.size());
        for (size_t q = 0; q < good.size(); q++) { pf[q] = proofs_out[act[a0 + good[q]]]; pr[q] = hp + good[q] * out_per; }
        compressed_challenges(C, good.size(), pf.data(), pr.data(), d, c.data());
        memset(htab, 0, sizeof(sc) * MAX_LG * gc);      // (a client that failed keeps its row of the launch; its sums are not read)
        for (size_t q = 0; q < good.size(); q++) fill_pow2(htab + good[q] * MAX_LG, h_mont(c[q]), MAX_LG);
        const u32 nblk = (u32)std::min<size_t>(kCompDotBlocks, (d + TPB - 1) / TPB);
        HIPCHK(hipMemcpyAsync(dtab, htab, sizeof(sc) * MAX_LG * gc, hipMemcpyHostToDevice, C.stream));
        ROFL_LAUNCH(k_cpow_dot_batch, dim3(nblk, (unsigned)gc), dim3(TPB), 0, C.stream, (u32)d, (const float *)(dv + b * G * d), fp_bits, fp_frac, (const sc *)(dr + b * G * d),
                    (const sc *)dtab, dpart);
        HIPCHK(hipMemcpyAsync(hpart, dpart, sizeof(sc) * gc * nblk * 2, hipMemcpyDeviceToHost, C.stream));
        C.sync();                                // wait 2
        for (size_t j : good) {
            const sc *p = hpart + j * nblk * 2; uint8_t *po = proofs_out[act[a0 + j]];
            sc_tobytes(po + 64, sc_add(nz[2 * (a0 + j)], h_canon(sum_partials(p, nblk, 2, 0))));
            sc_tobytes(po + 96, sc_add(nz[2 * (a0 + j) + 1], h_canon(sum_partials(p, nblk, 2, 1))));
        }
    }
    timing_end(C);
    return ROFL_OK;
}
// What every CompressedRandProof verifier does with the proof's 128 bytes: L', R' decoded, Z_m, Z_r canonical (the reference's FormatError
// otherwise), and, given sumL = sum_i c^(i+1) L_i and sumR = sum_i c^(i+1) R_i, the two exact group equations (params.rs:235-256)
//   z_m B + z_r B~ - (L' + sumL) == 0  and  z_r B - (R' + sumR) == 0   on the Ristretto coset.
struct CompProof { ge Lp, Rp; sc zm, zr; bool ok = false; };
CompProof compressed_parse(const uint8_t *proof) {
    CompProof q;
    q.ok = ristretto_decode(q.Lp, proof) && ristretto_decode(q.Rp, proof + 32) && sc_is_canonical_bytes(proof + 64) && sc_is_canonical_bytes(proof + 96);
    if (q.ok) { q.zm = sc_frombytes(proof + 64); q.zr = sc_frombytes(proof + 96); }
    return q;
}
bool compressed_equations(const Ctx &C, const CompProof &q, const ge5 &sumL, const ge5 &sumR) {
    auto neg5 = [](const ge5 &p) { ge5 r = p; r.X = h51::neg(p.X); r.T = h51::neg(p.T); return r; };
    ge5 e1 = h51::gadd(h51::gadd(h_fixed_mul(C.ht.B5, q.zm), h_fixed_mul(C.ht.Bb5, q.zr)), neg5(h51::gadd(h51::from_ge(q.Lp), sumL)));
    ge5 e2 = h51::gadd(h_fixed_mul(C.ht.B5, q.zr), neg5(h51::gadd(h51::from_ge(q.Rp), sumR)));
    return h51::is_identity_ristretto(e1) && h51::is_identity_ristretto(e2);
}
// The device half of every verifier.  A client is its challenge c and the device addresses of its d decoded L and its d decoded R; the
// clients go in groups of at most sixteen (one scalar array of sixteen clients, whatever their number): per group the power tables c^(2^b)
// go up, k_cpow_rows writes c^(i+1), and ONE multi-problem MSM -- two problems per client, naming the client's one scalar array -- gives
// sumL and sumR.  enqueue(g0), if any, runs before the launches of every group but the first (the group's points may be made then:
// msm_run has waited for the lane's stream, the previous group's MSM has finished); stage(g0), if any, runs on the host inside the MSM
// of the group before g0.
struct CompClient { sc c; const niels *L, *R; };
constexpr size_t kCompGroup = 16;
void compressed_sums(Ctx &C, size_t d, const std::vector<CompClient> &cl, std::vector<ge5> &sumL, std::vector<ge5> &sumR,
                     const std::function<void(size_t)> &enqueue = nullptr, const std::function<void(size_t)> &stage = nullptr) {
    const size_t ns = cl.size(), G = std::min<size_t>(ns, kCompGroup);
    sumL.assign(ns, h51::identity()); sumR.assign(ns, h51::identity());
    if (!ns || !d) return;
    sc *scal = C.aux_scal.as<sc>(G * d);
    sc *dtab = C.tmp_out.as<sc>(G * MAX_LG), *htab = C.h_cp.as<sc>(G * MAX_LG);
    for (size_t g0 = 0; g0 < ns; g0 += G) {
        const size_t gc = std::min(G, ns - g0);      // (gridDim.y = gc <= 16)
        if (g0 && enqueue) enqueue(g0);
        for (size_t j = 0; j < gc; j++) fill_pow2(htab + j * MAX_LG, h_mont(cl[g0 + j].c), MAX_LG);
        HIPCHK(hipMemcpyAsync(dtab, htab, sizeof(sc) * MAX_LG * gc, hipMemcpyHostToDevice, C.stream));
        ROFL_LAUNCH(k_cpow_rows, grid1((d + kCpowRun - 1) / kCpowRun, (u32)gc), dim3(TPB), 0, C.stream, (u32)d, (const sc *)dtab, scal);
        std::vector<MsmProb> pr(2 * gc);
        for (size_t j = 0; j < gc; j++) { pr[2 * j] = MsmProb{cl[g0 + j].L, scal + j * d}; pr[2 * j + 1] = MsmProb{cl[g0 + j].R, scal + j * d}; }
        C.tm.t.msm_terms += 2 * gc * d;
        MsmOpt opt;
        if (stage && g0 + gc < ns) opt.overlap = [&] { stage(g0 + gc); };
        std::vector<ge5> res;
        msm_run(C, pr, d, res, opt);      // (returns after the lane's stream has been waited for: the next group may overwrite the tables and the scalars)
        for (size_t j = 0; j < gc; j++) { sumL[g0 + j] = res[2 * j]; sumR[g0 + j] = res[2 * j + 1]; }
    }
}
// The server's check of the CompressedRandProofs of a round's clients on host bytes (it checks every RangeCompressed update,
// server.rs:656-687, params.rs:235-256): ok_out[i] is client i's own two equations (no random weights); a member whose proof or pairs do not
// decode gets 0 and the others go on -- every member is computed, the bad ones are ignored afterwards.  A group's pairs are staged on the
// host pool, uploaded and decoded one thread per point (k_decode_pairs_batch, one status word per client) into the device buffers of one
// group; two pinned staging buffers of a group alternate.  The pairs do not depend on the challenges: the first group is enqueued before
// the transcripts are hashed on the host pool, so the device decodes while the host hashes; the host stages group g + 1 inside the MSM of
// group g.  The final equalities (three fixed-base multiplications per client) run on the host pool.
// single: the one-client call (rofl_verify_compressed_randproof), which reports a malformed member as the reference does -- a FormatError,
// the proof's before anything else, the pairs' after their decode -- instead of the verdict 0.
// stride 96: pairs[i] are SquareRandProofCommitments records, verified in place -- staged as they lie (one contiguous copy per client, as
// ingest stages them), uploaded whole, hashed every 96 bytes and decoded by k_decode_pairs_strided_batch, which reads L | R of every
// record and never c_sq.  Everything after the decode is the same.
int compressed_verify_batch(size_t nc, const uint8_t *const *proofs, const uint8_t *const *pairs, size_t d, int *ok_out, bool single = false, size_t stride = 64) {
    LaneLock lane_lock = acquire_lane(false, nc == 1); Ctx &C = *lane_lock.c;
    for (size_t i = 0; i < nc; i++) ok_out[i] = 0;
    if (nc == 0) return ROFL_OK;
    std::vector<CompProof> q(nc);
    if (single) {
        q[0] = compressed_parse(proofs[0]);
        if (!q[0].ok) return fail(ROFL_FORMAT_ERROR, "FormatError");
        if (d >= 900000) return fail(ROFL_BAD_PARAM, "bad parameter");
    }
    C.init();
    C.batch_mode = nc > 1;
    timing_begin(C);
    const size_t G = std::min<size_t>(nc, kCompGroup);
    u32 *status = C.status.as<u32>(nc + 4);
    HIPCHK(hipMemsetAsync(status, 0, 4 * (nc + 4), C.stream));
    const size_t per = d * stride;      // a client's records
    uint8_t *dpairs = C.tmp_in.as<uint8_t>(G * per);
    niels *pts = C.aux_pts.as<niels>(2 * G * d);
    // group g + 2 is staged into group g's buffer while group g + 1 runs, and by then group g's upload has completed
    uint8_t *stg_buf[2] = {d ? (uint8_t *)C.stg.alloc(G * per) : nullptr, d && nc > G ? (uint8_t *)C.stg.alloc(G * per) : nullptr};
    auto stage = [&](size_t g0) {      // caller memory -> pinned staging, one pool task per client
        uint8_t *sp = stg_buf[(g0 / G) & 1];
        C.pool->run(std::min(G, nc - g0), [&](size_t i) { stage_copy(sp + i * per, pairs[g0 + i], per); });
    };
    auto decode = [&](size_t g0) {
        const size_t gc = std::min(G, nc - g0);
        HIPCHK(hipMemcpyAsync(dpairs, stg_buf[(g0 / G) & 1], gc * per, hipMemcpyHostToDevice, C.stream));
        count_decodes(2 * d * gc);
        if (stride == 64) ROFL_LAUNCH(k_decode_pairs_batch, grid1(2 * d, (u32)gc), dim3(TPB), 0, C.stream, (u32)d, (const uint8_t *)dpairs, pts, status + g0);
        else ROFL_LAUNCH(k_decode_pairs_strided_batch, grid1(2 * d, (u32)gc), dim3(TPB), 0, C.stream, (u32)d, (u32)stride, (const uint8_t *)dpairs, pts, status + g0);
    };
    if (d) { stage(0); decode(0); }
    std::vector<sc> c(nc);
    compressed_challenges(C, nc, proofs, pairs, d, c.data(), stride);      // (the device decodes the first group meanwhile)
    std::vector<CompClient> cl(nc);
    for (size_t i = 0; i < nc; i++) cl[i] = CompClient{c[i], pts + 2 * (i % G) * d, pts + (2 * (i % G) + 1) * d};
    std::vector<ge5> sumL, sumR;
    compressed_sums(C, d, cl, sumL, sumR, decode, stage);
    u32 *h_st = C.h_misc.as<u32>(nc + 4);
    HIPCHK(hipMemcpyAsync(h_st, status, 4 * nc, hipMemcpyDeviceToHost, C.stream));
    C.sync();
    if (single && (h_st[0] & 4u)) return fail(ROFL_FORMAT_ERROR, "FormatError: invalid ElGamal pair");
    C.pool->run(nc, [&](size_t i) {
        if (!single) q[i] = compressed_parse(proofs[i]);      // (the single call has parsed its proof before anything else)
        ok_out[i] = !(h_st[i] & 4u) && q[i].ok && compressed_equations(C, q[i], sumL[i], sumR[i]);
    });
    timing_end(C);
    return ROFL_OK;
}
// compressed_verify_batch for the clients of a round that keeps prefixes (ROFL_ROUND_COMPRESSED or rofl_round_create_rand; 64- or 96-byte
// records, the slot arithmetic below holds for both), from what ingest left on the device and in the round: nothing is
// uploaded but the power tables, nothing is decoded and no pair is hashed.  Per client with a proof and without a bad L or R (known since
// ingest): the proof is parsed and, from a copy of the stored transcript state, c drawn, on the host pool -- a proof that does not parse is
// out before anything is launched, as is a client left out or with a bad point (verdict 0 either way, as compressed_verify_batch gives them
// after its MSM).  The others are the selection: compressed_sums over slots 0 (L) and 2 (R) of the cache as they lie.  The final equalities
// run on the host pool.
int round_verify_compressed_impl(Ctx &C, Round &R, const uint8_t *const *proofs, int *ok_out) {
    const size_t n = R.n, d = R.d;
    for (size_t i = 0; i < n; i++) ok_out[i] = 0;
    std::vector<u32> cand;
    for (size_t i = 0; i < n; i++) if (proofs[i] && R.bad[3 * i] == ~0u && R.bad[3 * i + 1] == ~0u) cand.push_back((u32)i);
    if (cand.empty()) return ROFL_OK;
    C.init();
    C.batch_mode = n > 1;
    timing_begin(C);
    std::vector<CompProof> q(cand.size()); std::vector<sc> c(cand.size());
    C.pool->run(cand.size(), [&](size_t k) {
        q[k] = compressed_parse(proofs[cand[k]]);
        if (q[k].ok) c[k] = compressed_challenge(R.prefix[cand[k]], proofs[cand[k]]);
    });
    std::vector<size_t> sel; std::vector<CompClient> cl;      // sel: the selected among the candidates
    const size_t cstride = 2 * R.npts * d;      // a client's slots in the cache
    for (size_t k = 0; k < cand.size(); k++) if (q[k].ok) {
        const niels *base = R.pts + (size_t)cand[k] * cstride;
        sel.push_back(k); cl.push_back(CompClient{c[k], base, base + 2 * d});
    }
    std::vector<ge5> sumL, sumR;
    compressed_sums(C, d, cl, sumL, sumR);
    C.pool->run(sel.size(), [&](size_t j) { ok_out[cand[sel[j]]] = compressed_equations(C, q[sel[j]], sumL[j], sumR[j]); });
    timing_end(C);
    return ROFL_OK;
}
}  // namespace

namespace {
// ONE vector of per-element Sigma-proofs over several devices: contiguous runs of elements (rofl_set_option("devices", mask)), as the single-client
// range-proof calls deal chunks.  Runs shorter than kSigmaRunMin elements are not worth a device.
constexpr size_t kSigmaRunMin = 2048;
int sigma_create_any(int kind, const float *values, size_t d, const uint8_t *r1, size_t d_r1, const uint8_t *r2, const uint8_t *existing, unsigned fp_bits, unsigned fp_frac,
                     const rofl_nonce_t *nonce, uint8_t *proofs_out, uint8_t *commits_out) {
    std::vector<int> devs = batch_devices();
    auto runs = split_runs(d, devs.size(), kSigmaRunMin);
    if (devs.size() < 2 || runs.size() < 2 || d != d_r1 || !values || !r1 || !nonce || !proofs_out || !commits_out || (kind != 0 && !r2)) {
        ListedDevice bind(devs);
        return sigma_create(kind, values, d, r1, d_r1, r2, existing, fp_bits, fp_frac, nonce, proofs_out, commits_out);
    }
    const bool has_sq = kind != 0;
    const size_t npts = 1 + (kind != 2) + (has_sq ? 1 : 0), nn = has_sq ? 3 : 2, clen = 32 * npts, plen = 32 * (npts + nn);
    std::vector<int> rcs; std::vector<std::string> errs;
    if (int rc = run_on_devices(devs, runs.size(), rcs, errs, [&](size_t k) -> int {
            const size_t e0 = runs[k].first, cnt = runs[k].second;
            return sigma_create(kind, values + e0, cnt, r1 + 32 * e0, cnt, r2 ? r2 + 32 * e0 : nullptr, existing ? existing + 32 * e0 : nullptr, fp_bits, fp_frac, nonce,
                                proofs_out + e0 * plen, commits_out + e0 * clen, e0, d); }))
        return rc;
    // the unsplit call's outcome: the NaN check comes before anything is decoded (k_sigma_finish reports 2 before 4 per element; across
    // elements the call reports NON_FINITE first, sigma_create)
    for (size_t k = 0; k < rcs.size(); k++) if (rcs[k] >= ROFL_HIP_ERROR || rcs[k] == ROFL_BAD_PARAM || rcs[k] == ROFL_NONCE_SHORT) return fail(rcs[k], errs[k]);
    for (size_t k = 0; k < rcs.size(); k++) if (rcs[k] == ROFL_NON_FINITE) return fail(rcs[k], errs[k]);
    return first_failure(rcs, errs);
}
int sigma_verify_any(int kind, const uint8_t *proofs, const uint8_t *commits, size_t d, int *ok_out) {
    std::vector<int> devs = batch_devices();
    auto runs = split_runs(d, devs.size(), kSigmaRunMin);
    if (devs.size() < 2 || runs.size() < 2 || !proofs || !commits || !ok_out) {
        ListedDevice bind(devs);
        return sigma_verify_batch(kind, 1, &proofs, &commits, d, ok_out, nullptr, true);
    }
    const bool has_sq = kind != 0;
    const size_t npts = 1 + (kind != 2) + (has_sq ? 1 : 0), nn = has_sq ? 3 : 2, clen = 32 * npts, plen = 32 * (npts + nn);
    return verify_runs(devs, runs, ok_out, [&](size_t first, size_t count, int *ok) -> int {      // every run is its own random linear combination
        const uint8_t *pp = proofs + first * plen, *cc = commits + first * clen;
        return sigma_verify_batch(kind, 1, &pp, &cc, count, ok, nullptr, true); });
}
}  // namespace
int rofl_create_sigmaproof_vec_range(int kind, const float *values, size_t d, const uint8_t *r1_32, const uint8_t *r2_32, const uint8_t *existing32, unsigned fp_bits, unsigned fp_frac,
                                     const rofl_nonce_t *nonce, size_t elem_first, size_t elem_count, uint8_t *proofs_out, uint8_t *commits_out) {
    return guarded([&]() -> int {
        if (kind < 0 || kind > 2 || !values || !r1_32 || !nonce || !proofs_out || !commits_out || (kind != 0 && !r2_32) || elem_first > d || elem_count > d - elem_first)
            return fail(ROFL_BAD_PARAM, "bad parameter");
        return sigma_create(kind, values + elem_first, elem_count, r1_32 + 32 * elem_first, elem_count, r2_32 ? r2_32 + 32 * elem_first : nullptr,
                            existing32 ? existing32 + 32 * elem_first : nullptr, fp_bits, fp_frac, nonce, proofs_out, commits_out, elem_first, d); });
}
int rofl_create_squareproof_vec(const float *values, size_t d, const uint8_t *r1_32, size_t d_r1, const uint8_t *r2_32, const uint8_t *existing32,
                                unsigned fp_bits, unsigned fp_frac, const rofl_nonce_t *nonce, uint8_t *proofs_out, uint8_t *commits_out) {
    return guarded([&]() -> int { return sigma_create_any(2, values, d, r1_32, d_r1, r2_32, existing32, fp_bits, fp_frac, nonce, proofs_out, commits_out); });
}
int rofl_verify_squareproof_vec(const uint8_t *proofs, const uint8_t *commits, size_t d, int *ok_out) {
    return guarded([&]() -> int { return sigma_verify_any(2, proofs, commits, d, ok_out); });
}
int rofl_create_compressed_randproof(const float *values, size_t d, const uint8_t *r32, size_t d_r, const uint8_t *existing32, unsigned fp_bits, unsigned fp_frac,
                                     const rofl_nonce_t *nonce, uint8_t proof_out[128], uint8_t *pairs_out) {
    return guarded([&]() -> int {      // a batch of one on the caller's device (the batch entry would bind the first of the `devices` option)
        if (d != d_r) return fail(ROFL_WRONG_NUM_BLINDING, "WrongNumBlindingFactors");
        if (!valid_fp(fp_bits, fp_frac) || !nonce || d >= 900000) return fail(ROFL_BAD_PARAM, "bad parameter");
        int rc = ROFL_OK;
        int r = compressed_create_batch(1, &values, d, &r32, &existing32, fp_bits, fp_frac, nonce, &proof_out, &pairs_out, &rc);
        if (r != ROFL_OK) return r;
        switch (rc) {
            case ROFL_NONCE_SHORT: return fail(rc, "nonce stream too short");
            case ROFL_NON_FINITE: return fail(rc, "non-finite value (the reference panics in fixed::saturating_from_float)");
            case ROFL_FORMAT_ERROR: return fail(rc, "invalid Ristretto encoding");
        }
        return rc; });
}
int rofl_verify_compressed_randproof(const uint8_t proof[128], const uint8_t *pairs, size_t d, int *ok_out) {
    return guarded([&]() -> int { return compressed_verify_batch(1, &proof, &pairs, d, ok_out, true); });
}
int rofl_verify_compressed_randproof_batch(size_t n_clients, const uint8_t *const *proofs, const uint8_t *const *pairs, size_t d, int *ok_out) {
    return rofl_verify_compressed_randproof_batch_strided(n_clients, proofs, pairs, 64, d, ok_out);
}
int rofl_verify_compressed_randproof_batch_strided(size_t n_clients, const uint8_t *const *proofs, const uint8_t *const *pairs, size_t stride, size_t d, int *ok_out) {
    // (a fixed cap on the round, half of kMaxBatchMembers as for the other batch entries; the clients themselves run in groups of sixteen)
    if (stride != 64 && stride != 96) return fail(ROFL_BAD_PARAM, "bad parameter");
    if (!ok_out || (n_clients && (!proofs || !pairs)) || d >= 900000 || n_clients > kMaxBatchMembers / 2) return fail(ROFL_BAD_PARAM, "bad parameter");
    for (size_t i = 0; i < n_clients; i++) if (!proofs[i] || (d && !pairs[i])) return fail(ROFL_BAD_PARAM, "bad parameter");
    if (n_clients == 0) return ROFL_OK;
    return over_devices(n_clients, ok_out, [&](const Share &sh) -> int {
        auto p = sh.view(proofs); auto c = sh.view(pairs); auto ok = sh.out(ok_out);
        int r = compressed_verify_batch(sh.size(), p.data(), c.data(), d, ok.data(), false, stride);
        sh.scatter(ok);
        return r; });
}
int rofl_create_compressed_randproof_batch(size_t n_clients, const float *const *values, size_t d, const uint8_t *const *r32, const uint8_t *const *existing32,
                                           unsigned fp_bits, unsigned fp_frac, const rofl_nonce_t *nonces, uint8_t *const *proofs_out, uint8_t *const *pairs_out, int *rc_out) {
    // (everything here is decided before a device is touched)
    if (d >= 900000 || !valid_fp(fp_bits, fp_frac) || n_clients > kMaxBatchMembers) return fail(ROFL_BAD_PARAM, "bad parameter");
    if (n_clients == 0) return ROFL_OK;
    if (!nonces || !proofs_out || !rc_out || (d && (!values || !r32 || !pairs_out))) return fail(ROFL_BAD_PARAM, "bad parameter");
    for (size_t i = 0; i < n_clients; i++)
        if (!proofs_out[i] || (nonces[i].mode == 0 && nonces[i].stream_scalars && !nonces[i].stream) || (d && (!values[i] || !r32[i] || !pairs_out[i]))) return fail(ROFL_BAD_PARAM, "bad parameter");
    return over_devices(n_clients, nullptr, [&](const Share &sh) -> int {
        // (at d == 0 the value, blinding and pair arrays may be null: a share hands null entries down)
        auto v = sh.view(values, d != 0); auto r = sh.view(r32, d != 0); auto e = sh.view(existing32); auto nn = sh.view(nonces); auto po = sh.view(proofs_out); auto co = sh.view(pairs_out, d != 0);
        auto rc = sh.out(rc_out);
        int rcode = compressed_create_batch(sh.size(), v.data(), d, r.data(), e.data(), fp_bits, fp_frac, nn.data(), po.data(), co.data(), rc.data());
        sh.scatter(rc);
        return rcode; });
}
int rofl_create_sigmaproof_vec_batch(int kind, size_t n_clients, const float *const *values, size_t d, const uint8_t *const *r1_32, const uint8_t *const *r2_32,
                                     const uint8_t *const *existing32, unsigned fp_bits, unsigned fp_frac, const rofl_nonce_t *nonces, uint8_t *const *proofs_out,
                                     uint8_t *const *commits_out, int *rc_out) {
    // (everything here is decided before a device is touched)
    if (kind < 0 || kind > 2 || d >= ((size_t)1 << 28) || !valid_fp(fp_bits, fp_frac) || n_clients > kMaxBatchMembers) return fail(ROFL_BAD_PARAM, "bad parameter");
    if (n_clients == 0) return ROFL_OK;
    if (!nonces || !rc_out || (kind != 0 && !r2_32) || (d && (!values || !r1_32 || !proofs_out || !commits_out))) return fail(ROFL_BAD_PARAM, "bad parameter");
    for (size_t i = 0; i < n_clients; i++)
        if ((nonces[i].mode == 0 && nonces[i].stream_scalars && !nonces[i].stream) || (d && (!values[i] || !r1_32[i] || (kind != 0 && !r2_32[i]) || !proofs_out[i] || !commits_out[i])))
            return fail(ROFL_BAD_PARAM, "bad parameter");
    return over_devices(n_clients, nullptr, [&](const Share &sh) -> int {
        // (at d == 0 every array but the nonces may be null, and r2 is not read by kind 0: a share hands null entries down)
        auto v = sh.view(values, d != 0); auto a = sh.view(r1_32, d != 0); auto b = sh.view(r2_32, d != 0 && kind != 0); auto e = sh.view(existing32); auto nn = sh.view(nonces);
        auto po = sh.view(proofs_out, d != 0); auto co = sh.view(commits_out, d != 0); auto rc = sh.out(rc_out);
        int rcode = sigma_create_batch(kind, sh.size(), v.data(), d, a.data(), b.data(), e.data(), fp_bits, fp_frac, nn.data(), po.data(), co.data(), rc.data());
        sh.scatter(rc);
        return rcode; });
}
int rofl_create_randproof_vec(const float *values, size_t d, const uint8_t *r32, size_t d_r, const uint8_t *existing32, unsigned fp_bits, unsigned fp_frac,
                              const rofl_nonce_t *nonce, uint8_t *proofs_out, uint8_t *commits_out) {
    return guarded([&]() -> int { return sigma_create_any(0, values, d, r32, d_r, nullptr, existing32, fp_bits, fp_frac, nonce, proofs_out, commits_out); });
}
int rofl_verify_randproof_vec(const uint8_t *proofs, const uint8_t *commits, size_t d, int *ok_out) {
    return guarded([&]() -> int { return sigma_verify_any(0, proofs, commits, d, ok_out); });
}
int rofl_create_squarerandproof_vec(const float *values, size_t d, const uint8_t *r1_32, size_t d_r1, const uint8_t *r2_32, const uint8_t *existing32,
                                    unsigned fp_bits, unsigned fp_frac, const rofl_nonce_t *nonce, uint8_t *proofs_out, uint8_t *commits_out) {
    return guarded([&]() -> int { return sigma_create_any(1, values, d, r1_32, d_r1, r2_32, existing32, fp_bits, fp_frac, nonce, proofs_out, commits_out); });
}
int rofl_verify_squarerandproof_vec(const uint8_t *proofs, const uint8_t *commits, size_t d, int *ok_out) {
    return guarded([&]() -> int { return sigma_verify_any(1, proofs, commits, d, ok_out); });
}
namespace {
int sigma_batch_entry(int kind, size_t n_clients, const uint8_t *const *proofs, const uint8_t *const *commits, size_t d, int *ok_out, uint8_t *csq_sum_out32) {
    if (!ok_out || (n_clients && (!proofs || !commits))) return fail(ROFL_BAD_PARAM, "bad parameter");
    return over_devices(n_clients, ok_out, [&](const Share &sh) -> int {
        auto p = sh.view(proofs); auto c = sh.view(commits); auto ok = sh.out(ok_out); auto sums = sh.out(csq_sum_out32, 32);
        int r = sigma_verify_batch(kind, sh.size(), p.data(), c.data(), d, ok.data(), sums.data(), false);
        sh.scatter(ok);
        sh.scatter(sums);      // every member's c_sq sum, whatever its verdict and the share's outcome (unlike the L2 creator's commitments)
        return r; });
}
}  // namespace
int rofl_verify_randproof_vec_batch(size_t n_clients, const uint8_t *const *proofs, const uint8_t *const *commits, size_t d, int *ok_out) {
    return sigma_batch_entry(0, n_clients, proofs, commits, d, ok_out, nullptr);
}
int rofl_verify_squarerandproof_vec_batch(size_t n_clients, const uint8_t *const *proofs, const uint8_t *const *commits, size_t d, int *ok_out, uint8_t *csq_sum_out32) {
    return sigma_batch_entry(1, n_clients, proofs, commits, d, ok_out, csq_sum_out32);
}
int rofl_verify_squareproof_vec_batch(size_t n_clients, const uint8_t *const *proofs, const uint8_t *const *commits, size_t d, int *ok_out, uint8_t *csq_sum_out32) {
    return sigma_batch_entry(2, n_clients, proofs, commits, d, ok_out, csq_sum_out32);
}

int rofl_commit_vec(const uint8_t *values32, const uint8_t *blindings32, size_t d, uint8_t *out32) {
    return guarded([&]() -> int {
        LaneLock lane_lock = acquire_lane(); Ctx &C = *lane_lock.c;
        if (d == 0) return ROFL_OK;
        C.init();
        sc *dv = C.tmp_in.as<sc>(d); sc *db = blindings32 ? C.tmp_in2.as<sc>(d) : nullptr;
        uint8_t *o = C.Cbytes.as<uint8_t>(d * 32);
        C.up(dv, values32, 32 * d, C.stream);
        if (db) C.up(db, blindings32, 32 * d, C.stream);
        ROFL_LAUNCH(k_commit, grid1(d), dim3(TPB), 0, C.stream, (u32)d, (const u64 *)nullptr, dv, db, C.d_tabB8, C.d_tabBb8, (const niels *)nullptr, (uint8_t *)nullptr, o, (u32)d, (u32)d);
        C.down(out32, o, 32 * d, C.stream);
        C.sync();
        return ROFL_OK;
    });
}
int rofl_add_points_vec(const uint8_t *a32, const uint8_t *b32, size_t d, uint8_t *out32) {
    return guarded([&]() -> int {
        LaneLock lane_lock = acquire_lane(); Ctx &C = *lane_lock.c;
        if (d == 0) return ROFL_OK;
        C.init();
        uint8_t *da = C.tmp_in.as<uint8_t>(d * 32), *db = C.tmp_in2.as<uint8_t>(d * 32), *o = C.Cbytes.as<uint8_t>(d * 32);
        u32 *status = C.status.as<u32>(4);
        HIPCHK(hipMemsetAsync(status, 0, 16, C.stream));
        C.up(da, a32, 32 * d, C.stream);
        C.up(db, b32, 32 * d, C.stream);
        count_decodes(2 * d);
        ROFL_LAUNCH(k_add_points, grid1(d), dim3(TPB), 0, C.stream, (u32)d, da, db, o, status);
        u32 st = 0;
        C.down(out32, o, 32 * d, C.stream);
        HIPCHK(hipMemcpyAsync(&st, status, 4, hipMemcpyDeviceToHost, C.stream));
        C.sync();
        if (st & 4u) return fail(ROFL_FORMAT_ERROR, "invalid Ristretto encoding");
        return ROFL_OK;
    });
}
int rofl_sum_points(const uint8_t *points, size_t d, size_t stride, uint8_t out32[32]) {
    return guarded([&]() -> int {
        LaneLock lane_lock = acquire_lane(); Ctx &C = *lane_lock.c;
        if (stride < 32 || !out32 || (d && !points)) return fail(ROFL_BAD_PARAM, "bad parameter");
        if (d == 0) { memset(out32, 0, 32); return ROFL_OK; }      // empty sum = identity
        C.init();
        uint8_t *da = C.tmp_in.as<uint8_t>(d * stride);
        u32 nblk = (u32)std::min<size_t>(64, (d + TPB - 1) / TPB);
        ge *part = C.partial2.as<ge>(nblk);
        u32 *status = C.status.as<u32>(4);
        HIPCHK(hipMemsetAsync(status, 0, 16, C.stream));
        C.up(da, points, stride * d, C.stream);
        count_decodes(d);
        ROFL_LAUNCH(k_decode_sum, dim3(nblk), dim3(TPB), TPB * sizeof(ge), C.stream, da, (u32)d, (u32)stride, part, status);
        std::vector<ge> hp(nblk); u32 st = 0;
        HIPCHK(hipMemcpyAsync(hp.data(), part, sizeof(ge) * nblk, hipMemcpyDeviceToHost, C.stream));
        HIPCHK(hipMemcpyAsync(&st, status, 4, hipMemcpyDeviceToHost, C.stream));
        C.sync();
        if (st & 4u) return fail(ROFL_FORMAT_ERROR, "invalid Ristretto encoding");
        ge5 acc = h51::identity();
        for (u32 i = 0; i < nblk; i++) acc = h51::gadd(acc, h51::from_ge(hp[i]));
        h51::encode(out32, acc);
        return ROFL_OK;
    });
}
int rofl_shift_points(const uint8_t *a32, size_t d, const uint8_t offset32[32], uint8_t *out32) {
    return guarded([&]() -> int {
        LaneLock lane_lock = acquire_lane(); Ctx &C = *lane_lock.c;
        if (d == 0) return ROFL_OK;
        C.init();
        ge off; if (!ristretto_decode(off, offset32)) return fail(ROFL_FORMAT_ERROR, "invalid Ristretto encoding");
        niels hs = ge_to_niels(off);
        niels *ds = C.tmp_in2.as<niels>(1);
        uint8_t *da = C.tmp_in.as<uint8_t>(d * 32), *o = C.Cbytes.as<uint8_t>(d * 32);
        u32 *status = C.status.as<u32>(4);
        HIPCHK(hipMemsetAsync(status, 0, 16, C.stream));
        HIPCHK(hipMemcpyAsync(ds, &hs, sizeof hs, hipMemcpyHostToDevice, C.stream));
        C.up(da, a32, 32 * d, C.stream);
        count_decodes(d);
        ROFL_LAUNCH(k_decode, grid1(d), dim3(TPB), 0, C.stream, (u32)d, (u32)d, da, ds, (niels *)nullptr, o, status);
        u32 st = 0;
        C.down(out32, o, 32 * d, C.stream);
        HIPCHK(hipMemcpyAsync(&st, status, 4, hipMemcpyDeviceToHost, C.stream));
        C.sync();
        if (st & 4u) return fail(ROFL_FORMAT_ERROR, "invalid Ristretto encoding");
        return ROFL_OK;
    });
}
int rofl_f32_to_scalar_vec(const float *in, size_t d, unsigned fp_bits, unsigned fp_frac, uint8_t *out32) {
    if (!valid_fp(fp_bits, fp_frac)) return fail(ROFL_BAD_PARAM, "bad parameter");
    for (size_t i = 0; i < d; i++) { sc s; int rc = f32_to_sc(in[i], fp_bits, fp_frac, &s); if (rc) return fail(rc, "non-finite value"); sc_tobytes(out32 + 32 * i, s); }
    return ROFL_OK;
}
int rofl_scalar_to_f32_vec(const uint8_t *in32, size_t d, unsigned fp_bits, unsigned fp_frac, float *out) {
    if (!valid_fp(fp_bits, fp_frac)) return fail(ROFL_BAD_PARAM, "bad parameter");
    for (size_t i = 0; i < d; i++) out[i] = sc_to_f32(sc_frombytes(in32 + 32 * i), fp_bits, fp_frac);
    return ROFL_OK;
}
// conversion32::square (conversion32.rs:66-88): |s| as Fix, checked_mul (fixed 0.3.3: wide product >> frac, truncated), panic on overflow
int rofl_fp_square_vec(const uint8_t *in32, size_t d, unsigned fp_bits, unsigned fp_frac, uint8_t *out32) {
    if (!valid_fp(fp_bits, fp_frac)) return fail(ROFL_BAD_PARAM, "bad parameter");
    for (size_t i = 0; i < d; i++) {
        sc s = sc_frombytes(in32 + 32 * i);
        u64 v = (s.v[7] >> 24) != 0 ? read_from_bytes(sc_neg(s), fp_bits) : read_from_bytes(s, fp_bits);
        unsigned __int128 prod = ((unsigned __int128)v * v) >> fp_frac;
        if (prod > (unsigned __int128)fix_max_bits(fp_bits)) return fail(ROFL_OVERFLOW, "square overflows the fixed-point type (the reference panics)");
        sc_tobytes(out32 + 32 * i, sc_from_u64((u64)prod));
    }
    return ROFL_OK;
}
// conversion32::precompute_exponentiate (conversion32.rs:101-111): 1, v, v^2, ..., v^(count-1); exponentiate(v, e) = element e
int rofl_scalar_powers(const uint8_t value32[32], size_t count, uint8_t *out32) {
    sc v = h_mont(sc_frombytes(value32)), acc = sc_one_mont();
    for (size_t i = 0; i < count; i++) { sc_tobytes(out32 + 32 * i, h_canon(acc)); acc = sc_montmul(acc, v); }
    return ROFL_OK;
}
// pedersen_ops::add_scalar_vec (pedersen_ops.rs:78-81); subtract != 0 gives a - b (generate_cancelling_scalar_vec negates a running sum)
int rofl_scalar_add_vec(const uint8_t *a32, const uint8_t *b32, size_t d, int subtract, uint8_t *out32) {
    for (size_t i = 0; i < d; i++) {
        sc a = sc_frombytes(a32 + 32 * i), b = sc_frombytes(b32 + 32 * i);
        if (sc_geq_l(a.v)) a = sc_from_mont(sc_to_mont(a));
        if (sc_geq_l(b.v)) b = sc_from_mont(sc_to_mont(b));
        sc_tobytes(out32 + 32 * i, subtract ? sc_sub(a, b) : sc_add(a, b));
    }
    return ROFL_OK;
}
// Blinding vectors from seeds: out32[v][k] = sum_t sign_t * stream(seed_t)[first + k] mod l (k_blind_combine), every vector of the call in ONE
// launch.  Covers pedersen_ops::rnd_scalar_vec (one +1 term), generate_cancelling_scalar_vec (the last vector = the negated others) and
// pairwise masks (one term per peer).  Seeds are secrets: they are never put into an error text, and the lane's copies of the term list
// (pinned host memory and device workspace) are overwritten with zeros before the call returns or unwinds.
int rofl_blinding_vecs(size_t n_vec, const size_t *term_count, const rofl_blind_term_t *const *terms, size_t first, size_t d, uint8_t *const *out32) {
    if (n_vec == 0) return ROFL_OK;
    if (!term_count || !terms || !out32) return fail(ROFL_BAD_PARAM, "bad parameter");
    if (n_vec > kMaxBatchMembers) return fail(ROFL_BAD_PARAM, "more than 65 535 vectors in one call");
    if (d >= ((size_t)1 << 28)) return fail(ROFL_BAD_PARAM, "vector length of 2^28 or more");
    if (first > ((size_t)1 << 63) - d) return fail(ROFL_BAD_PARAM, "first + d exceeds 2^63");
    size_t total = 0;
    for (size_t v = 0; v < n_vec; v++) {
        if (d && !out32[v]) return fail(ROFL_BAD_PARAM, "bad parameter");
        if (int rc = blind_terms_check(term_count[v], terms[v], &total)) return rc;
    }
    if (d == 0) return ROFL_OK;
    return guarded([&]() -> int {
        LaneLock lane_lock = acquire_lane(); Ctx &C = *lane_lock.c;
        C.init();
        std::vector<char> on_dev(n_vec); size_t n_host = 0;
        for (size_t v = 0; v < n_vec; v++) {
            on_dev[v] = is_device_ptr(out32[v]);
            if (on_dev[v] && ((uintptr_t)out32[v] & 15)) return fail(ROFL_BAD_PARAM, "a device output must be 16-byte aligned");
            if (!on_dev[v]) n_host++;
        }
        // a device output is written in place; a host output goes through the lane's workspace and the staging path
        uint8_t *ws = n_host ? C.Cbytes.as<uint8_t>(n_host * d * 32) : nullptr;
        std::vector<uint8_t *> dst(n_vec); size_t slot = 0;
        for (size_t v = 0; v < n_vec; v++) dst[v] = on_dev[v] ? out32[v] : ws + (slot++) * d * 32;
        BlindWipe wipe;
        blind_combine_launch(C, C.tmp_in, wipe, n_vec, term_count, terms, total, first, d, dst.data());
        for (size_t v = 0; v < n_vec; v++) if (!on_dev[v]) C.down(out32[v], dst[v], d * 32, C.stream);
        C.sync();
        return ROFL_OK;
    });
}
// pedersen_ops::rnd_scalar_vec (pedersen_ops.rs:124-127) with the randomness an explicit input: one vector of one +1 term
int rofl_rnd_scalar_vec(const uint8_t seed[32], size_t first, size_t d, uint8_t *out32) {
    if (!seed) return fail(ROFL_BAD_PARAM, "bad parameter");
    rofl_blind_term_t term; memcpy(term.seed, seed, 32); term.sign = 1;
    const rofl_blind_term_t *tp = &term; const size_t one = 1; uint8_t *op = out32;
    int rc = rofl_blinding_vecs(1, &one, &tp, first, d, &op);
    volatile uint8_t *p = term.seed; for (int i = 0; i < 32; i++) p[i] = 0;
    return rc;
}
#include "prepare_calls.hpp"
#include "protocol_calls.hpp"
// what the calls above left in the lanes' staging buffers (described in the debug header): reads only; every device buffer is copied whole
int rofl_dbg_lane_scan(const uint8_t *needle, size_t n, int *found) {
    if (!needle || !found || n < 16) return fail(ROFL_BAD_PARAM, "bad parameter");
    *found = 0;
    return guarded([&]() -> int {
        Ctx *P = nullptr;
        { std::lock_guard<std::mutex> lk(g_ctx_mu); auto it = g_ctxs.find(current_device()); if (it != g_ctxs.end()) P = it->second; }
        if (!P) return ROFL_OK;
        std::vector<Ctx *> lanes;
        { std::lock_guard<std::mutex> g(P->init_mu); if (P->inited) { lanes.push_back(P); lanes.insert(lanes.end(), P->sibs.begin(), P->sibs.end()); } }
        std::vector<uint8_t> copy;
        const auto holds = [&](const uint8_t *p, size_t cap) { return p && std::search(p, p + cap, needle, needle + n) != p + cap; };
        for (Ctx *c : lanes) {
            std::lock_guard<std::mutex> lk(c->mu);
            HIPCHK(hipSetDevice(P->phys));
            HIPCHK(hipStreamSynchronize(c->stream));
            for (const PinBuf *b : {&c->h_misc, &c->h_misc2}) *found += holds((const uint8_t *)b->p, b->cap);
            for (const DevBuf *b : {&c->tmp_in, &c->tmp_in2, &c->tmp_out}) {
                if (!b->p) continue;
                copy.resize(b->cap);
                HIPCHK(hipMemcpy(copy.data(), b->p, b->cap, hipMemcpyDeviceToHost));
                *found += holds(copy.data(), b->cap);
            }
        }
        return ROFL_OK;
    });
}
// conversion32::f32_to_fp_vec / uint_to_f32_vec (conversion32.rs:41-54): Fix is unsigned, negative inputs saturate to 0
int rofl_f32_to_fp_vec(const float *in, size_t d, unsigned fp_bits, unsigned fp_frac, uint64_t *out) {
    if (!valid_fp(fp_bits, fp_frac)) return fail(ROFL_BAD_PARAM, "bad parameter");
    for (size_t i = 0; i < d; i++) {
        if (std::isnan(in[i])) return fail(ROFL_NON_FINITE, "non-finite value (the reference panics in fixed::saturating_from_float)");
        if (in[i] < 0.0f) { out[i] = 0; continue; }
        sc s; int rc = f32_to_sc(in[i], fp_bits, fp_frac, &s); if (rc) return fail(rc, "non-finite value");
        out[i] = read_from_bytes(s, fp_bits);
    }
    return ROFL_OK;
}
int rofl_uint_to_f32_vec(const uint64_t *in, size_t d, unsigned fp_bits, unsigned fp_frac, float *out) {
    if (!valid_fp(fp_bits, fp_frac)) return fail(ROFL_BAD_PARAM, "bad parameter");
    for (size_t i = 0; i < d; i++) out[i] = fix_to_f32(in[i] & fix_max_bits(fp_bits), fp_frac);
    return ROFL_OK;
}
int rofl_get_clip_bounds(size_t range, unsigned fp_bits, unsigned fp_frac, float *mn, float *mx) {
    if (!valid_fp(fp_bits, fp_frac) || range == 0 || range > 128) return fail(ROFL_BAD_PARAM, "bad parameter");
    clip_bounds(range, fp_bits, fp_frac, mn, mx); return ROFL_OK;
}
int rofl_get_l2_clip_bounds(size_t range, unsigned fp_bits, unsigned fp_frac, float *out) {
    if (!valid_fp(fp_bits, fp_frac) || range == 0 || range > 127) return fail(ROFL_BAD_PARAM, "bad parameter");
    *out = l2_clip_bound(range, fp_bits, fp_frac); return ROFL_OK;
}

int rofl_dbg_msm(const uint8_t *scalars32, const uint8_t *points32, size_t n, uint8_t out32[32]) {
    return guarded([&]() -> int {
        LaneLock lane_lock = acquire_lane(); Ctx &C = *lane_lock.c;
        if (n == 0) return fail(ROFL_BAD_PARAM, "bad parameter");
        C.init();
        std::vector<sc> hs(n);
        for (size_t i = 0; i < n; i++) { hs[i] = sc_frombytes(scalars32 + 32 * i); if (sc_geq_l(hs[i].v)) hs[i] = sc_from_mont(sc_to_mont(hs[i])); }
        uint8_t *dp = C.tmp_in.as<uint8_t>(n * 32); niels *dn = C.aux_pts.as<niels>(n); sc *ds = C.aux_scal.as<sc>(n);
        u32 *status = C.status.as<u32>(4);
        HIPCHK(hipMemsetAsync(status, 0, 16, C.stream));
        C.up(dp, points32, n * 32, C.stream);
        C.up(ds, hs.data(), n * 32, C.stream);
        count_decodes(n);
        ROFL_LAUNCH(k_decode, grid1(n), dim3(TPB), 0, C.stream, (u32)n, (u32)n, dp, (const niels *)nullptr, dn, (uint8_t *)nullptr, status);
        u32 st = 0;
        HIPCHK(hipMemcpyAsync(&st, status, 4, hipMemcpyDeviceToHost, C.stream));
        C.sync();
        if (st & 4u) return fail(ROFL_FORMAT_ERROR, "invalid Ristretto encoding");
        std::vector<MsmProb> pr(1, MsmProb{dn, ds}); std::vector<ge5> res;
        msm_run(C, pr, n, res);
        h51::encode(out32, res[0]);
        return ROFL_OK;
    });
}
// np generic problems over one shared point array in one msm_run (test hook: the many-problem finishers under chosen scalars)
int rofl_dbg_msm_many(size_t np, size_t n, const uint8_t *scalars32, const uint8_t *points32, uint8_t *out32) {
    return guarded([&]() -> int {
        LaneLock lane_lock = acquire_lane(); Ctx &C = *lane_lock.c;
        if (np == 0 || n == 0 || !scalars32 || !points32 || !out32 || np * n > ((size_t)1 << 24)) return fail(ROFL_BAD_PARAM, "bad parameter");
        C.init();
        std::vector<sc> hs(np * n);
        for (size_t i = 0; i < np * n; i++) { hs[i] = sc_frombytes(scalars32 + 32 * i); if (sc_geq_l(hs[i].v)) hs[i] = sc_from_mont(sc_to_mont(hs[i])); }
        uint8_t *dp = C.tmp_in.as<uint8_t>(n * 32); niels *dn = C.aux_pts.as<niels>(n); sc *ds = C.aux_scal.as<sc>(np * n);
        u32 *status = C.status.as<u32>(4);
        HIPCHK(hipMemsetAsync(status, 0, 16, C.stream));
        C.up(dp, points32, n * 32, C.stream);
        C.up(ds, hs.data(), np * n * 32, C.stream);
        count_decodes(n);
        ROFL_LAUNCH(k_decode, grid1(n), dim3(TPB), 0, C.stream, (u32)n, (u32)n, dp, (const niels *)nullptr, dn, (uint8_t *)nullptr, status);
        u32 st = 0;
        HIPCHK(hipMemcpyAsync(&st, status, 4, hipMemcpyDeviceToHost, C.stream));
        C.sync();
        if (st & 4u) return fail(ROFL_FORMAT_ERROR, "invalid Ristretto encoding");
        std::vector<MsmProb> pr(np); std::vector<ge5> res;
        for (size_t p = 0; p < np; p++) pr[p] = MsmProb{dn, ds + p * n};
        msm_run(C, pr, n, res);
        for (size_t p = 0; p < np; p++) h51::encode(out32 + 32 * p, res[p]);
        return ROFL_OK;
    });
}
// np problems over the generators of (n_bits, m) in one msm_run, with the shape's window table in the MsmOpt as verify_chunks sets it
// (test hook: the fixed-base variants under chosen scalars)
int rofl_dbg_msm_fixed(size_t n_bits, size_t m, size_t np, const uint8_t *scalars32, uint8_t *out32) {
    return guarded([&]() -> int {
        LaneLock lane_lock = acquire_lane(); Ctx &C = *lane_lock.c;
        if (n_bits == 0 || m == 0 || np == 0 || !scalars32 || !out32 || n_bits * m > ((size_t)1 << 22) || np * 2 * n_bits * m > ((size_t)1 << 24)) return fail(ROFL_BAD_PARAM, "bad parameter");
        C.init();
        const size_t N = n_bits * m;
        GensPin gens = get_gens(C, n_bits, m, GENS_VERIFY);
        if (!gens.wtab()) return fail(ROFL_BAD_PARAM, "the shape has no window table");
        std::vector<sc> hs(np * 2 * N);
        for (size_t i = 0; i < hs.size(); i++) { hs[i] = sc_frombytes(scalars32 + 32 * i); if (sc_geq_l(hs[i].v)) hs[i] = sc_from_mont(sc_to_mont(hs[i])); }
        sc *ds = C.SL.as<sc>(np * 2 * N);
        C.up(ds, hs.data(), hs.size() * 32, C.stream);
        C.sync();
        std::vector<MsmProb> pr(np); std::vector<ge5> res;
        for (size_t p = 0; p < np; p++) pr[p] = MsmProb{gens.tbl(), ds + p * 2 * N};
        MsmOpt mo; gens.fb_for(np, &mo.fb_wtab, &mo.fb_c); mo.fb_stride = 2 * N;
        msm_run(C, pr, 2 * N, res, mo);
        for (size_t p = 0; p < np; p++) h51::encode(out32 + 32 * p, res[p]);
        return ROFL_OK;
    });
}
int rofl_dbg_msm_trace(rofl_msm_attempt_t *attempts_out, size_t max, size_t *count_out) {
    if (!count_out || (max && !attempts_out)) return ROFL_BAD_PARAM;
    *count_out = t_msm_trace_n;
    for (size_t i = 0; i < max && i < t_msm_trace_n; i++) attempts_out[i] = t_msm_trace[i];
    return ROFL_OK;
}
int rofl_dbg_msm_trace_begin(void) { t_msm_runs.clear(); t_msm_runs_n = 0; t_msm_runs_on = true; return ROFL_OK; }
int rofl_dbg_msm_trace_all(rofl_msm_run_t *out, size_t max, size_t *count_out) {
    if (!count_out || (max && !out)) return ROFL_BAD_PARAM;
    *count_out = t_msm_runs_n;
    for (size_t i = 0; i < max && i < t_msm_runs.size(); i++) out[i] = t_msm_runs[i];
    return ROFL_OK;
}
// bulletproofs' RangeProof::verify_multiple(&bp_gens, &pc_gens, &mut Transcript::new(label), &value_commitments, n) on ONE aggregated proof
// exactly as upstream's own tests call it: any transcript label (upstream's serialized-proof vectors use b"Deserialize-And-Verify Test"),
// the commitments as they are (no shift, no padding: m must be a power of two), generators of capacity >= n.  If byte vectors of
// bulletproofs 4.0.0 ever become reachable, they go straight through the HIP verifier here (the crate-level pin the oracle lacks).
int rofl_dbg_verify_labelled(const uint8_t *label, size_t label_len, size_t gens_capacity, const uint8_t *proof, size_t proof_len,
                             const uint8_t *commits32, size_t m, size_t n_bits, const uint8_t verifier_seed[32], int *ok_out) {
    return guarded([&]() -> int {
        LaneLock lane_lock = acquire_lane(false, true); Ctx &C = *lane_lock.c;
        if (!label || !label_len || label_len > 255 || !proof || !commits32 || !m || !is_pow2(m) || !verifier_seed || !ok_out) return fail(ROFL_BAD_PARAM, "bad parameter");
        *ok_out = 0;
        std::string lbl((const char *)label, label_len);
        if (lbl.find('\0') != std::string::npos) return fail(ROFL_BAD_PARAM, "the label holds a NUL byte");
        C.init();
        timing_begin(C);
        uint8_t *d_in = C.Cbytes.as<uint8_t>(m * 32), *d_enc = C.Vbytes.as<uint8_t>(m * 32);
        niels *d_vn = C.gbuf[0].as<niels>(m);
        u32 *status = C.status.as<u32>(4);
        HIPCHK(hipMemsetAsync(status, 0, 16, C.stream));
        C.up(d_in, commits32, m * 32, C.stream);
        count_decodes(m);
        ROFL_LAUNCH(k_decode, grid1(m), dim3(TPB), 0, C.stream, (u32)m, (u32)m, d_in, (const niels *)nullptr, d_vn, d_enc, status);
        std::vector<uint8_t> hV(m * 32); u32 *h_st = C.h_misc.as<u32>(4);
        uint8_t *hp = C.h_V.as<uint8_t>(m * 32);
        HIPCHK(hipMemcpyAsync(hp, d_enc, m * 32, hipMemcpyDeviceToHost, C.stream));
        HIPCHK(hipMemcpyAsync(h_st, status, 4, hipMemcpyDeviceToHost, C.stream));
        C.sync();
        if (h_st[0] & 4u) { timing_end(C); return fail(ROFL_FORMAT_ERROR, "commitment is not a valid Ristretto encoding"); }
        u64 cidx = 0; int ok = 0;
        int rc = verify_chunks(C, lbl.c_str(), gens_capacity, 1, n_bits, m, proof, proof_len, hp, d_vn, verifier_seed, &cidx, &ok);
        timing_end(C);
        if (rc) return fail(rc, "proof rejected before verification (format / bitsize / generator capacity)");
        *ok_out = ok;
        return ROFL_OK;
    });
}
int rofl_dbg_msm_retries(uint64_t out[4]) { if (!out) return ROFL_BAD_PARAM; for (int i = 0; i < 4; i++) out[i] = g_msm_stat[i].load(); return ROFL_OK; }
int rofl_dbg_quad_ops(const uint8_t *pairs64, size_t pairs, unsigned doublings, uint8_t *out_serial32, uint8_t *out_quad32) {
    return guarded([&]() -> int {
        LaneLock lane_lock = acquire_lane(); Ctx &C = *lane_lock.c;
        if (pairs == 0) return fail(ROFL_BAD_PARAM, "bad parameter");
        C.init();
        uint8_t *din = C.tmp_in.as<uint8_t>(pairs * 64), *dout = C.tmp_out.as<uint8_t>(pairs * 64);
        u32 *status = C.status.as<u32>(4);
        HIPCHK(hipMemsetAsync(status, 0, 16, C.stream));
        HIPCHK(hipMemsetAsync(dout, 0, pairs * 64, C.stream));
        C.up(din, pairs64, pairs * 64, C.stream);
        ROFL_LAUNCH(k_dbg_quad, grid1(pairs * 4), dim3(TPB), 0, C.stream, (u32)pairs, doublings, (const uint8_t *)din, dout, dout + pairs * 32, status);
        u32 st = 0;
        HIPCHK(hipMemcpyAsync(&st, status, 4, hipMemcpyDeviceToHost, C.stream));
        C.down(out_serial32, dout, pairs * 32, C.stream);
        C.down(out_quad32, dout + pairs * 32, pairs * 32, C.stream);
        C.sync();
        if (st & 4u) return fail(ROFL_FORMAT_ERROR, "invalid Ristretto encoding");
        return ROFL_OK;
    });
}
// the op tables of fd_dbg.hpp on the device: n cases of `in_words` words in, `out_words` words out, one launch
static int dbg_ops_device(bool scalar_field, unsigned op, size_t n, const uint32_t *in, uint32_t *out) {
    const size_t in_words = scalar_field ? SC_DBG_IN : FD_DBG_IN, out_words = scalar_field ? SC_DBG_OUT : FD_DBG_OUT;
    if (op >= (unsigned)(scalar_field ? SC_DBG_OPS : FD_DBG_OPS)) return fail(ROFL_BAD_PARAM, "bad parameter");
    return guarded([&]() -> int {
        LaneLock lane_lock = acquire_lane(); Ctx &C = *lane_lock.c;
        if (n == 0 || n > (1u << 20) || !in || !out) return fail(ROFL_BAD_PARAM, "bad parameter");
        C.init();
        u32 *din = C.tmp_in.as<u32>(n * in_words), *dout = C.tmp_out.as<u32>(n * out_words);
        C.up(din, in, n * in_words * 4, C.stream);
        C.up(dout, out, n * out_words * 4, C.stream);      // words an op does not write come back as the caller sent them
        if (scalar_field) ROFL_LAUNCH(k_dbg_sc, grid1(n), dim3(TPB), 0, C.stream, (u32)op, (u32)n, (const u32 *)din, dout);
        else ROFL_LAUNCH(k_dbg_fd, grid1(op < FD_DBG_THREAD_OPS ? n : n * 4), dim3(TPB), 0, C.stream, (u32)op, (u32)n, (const u32 *)din, dout);
        C.down(out, dout, n * out_words * 4, C.stream);
        C.sync();
        return ROFL_OK;
    });
}
int rofl_dbg_fd_ops(unsigned op, size_t n, const uint32_t *in, uint32_t *out) { return dbg_ops_device(false, op, n, in, out); }
int rofl_dbg_sc_ops(unsigned op, size_t n, const uint32_t *in, uint32_t *out) { return dbg_ops_device(true, op, n, in, out); }
// Every Ristretto encoder and identity predicate of the library on the caller's own representatives: case i is the projective point
// (X, Y, Z, T) of xyzt[128 i ..], four canonical field elements, loaded into the site's point type as it is -- any Z, any of the four
// representatives K + E[4] of a class.  Nothing here encodes or tests by itself: each site calls the production function.
int rofl_dbg_encode_reps(unsigned site, size_t n, const uint8_t *xyzt, uint8_t *out32, uint8_t *is_identity_out) {
    if (site > 4 || n > (1u << 20) || !xyzt || !out32 || !is_identity_out) return fail(ROFL_BAD_PARAM, "bad parameter");
    std::vector<ge> pts(n);
    for (size_t i = 0; i < n; i++) {
        fe *const c[4] = {&pts[i].X, &pts[i].Y, &pts[i].Z, &pts[i].T};
        for (int k = 0; k < 4; k++) {
            const uint8_t *b = xyzt + 128 * i + 32 * k;
            *c[k] = fe_frombytes(b);
            uint8_t chk[32]; fe_tobytes(chk, *c[k]);
            if (memcmp(chk, b, 32) != 0) return fail(ROFL_BAD_PARAM, "a coordinate is not a canonical field element");
        }
    }
    if (site == 0) {
        if (n == 0) return ROFL_OK;
        return guarded([&]() -> int {
            LaneLock lane_lock = acquire_lane(); Ctx &C = *lane_lock.c;
            C.init();
            ge *din = C.tmp_in.as<ge>(n);
            uint8_t *dout = C.tmp_out.as<uint8_t>(n * 33);
            C.up(din, pts.data(), n * sizeof(ge), C.stream);
            ROFL_LAUNCH(k_dbg_encode_reps, grid1(n), dim3(TPB), 0, C.stream, (u32)n, (const ge *)din, dout, dout + n * 32);
            C.down(out32, dout, n * 32, C.stream);
            C.down(is_identity_out, dout + n * 32, n, C.stream);
            C.sync();
            return ROFL_OK;
        });
    }
    if (site == 4 && !h8::available()) return -1;
    for (size_t i = 0; i < n; i++) {
        if (site == 1) { const gd p = gd_unpack(pts[i]); gd_ristretto_encode(out32 + 32 * i, p); is_identity_out[i] = ge_is_identity_ristretto(gd_pack(p)) ? 1 : 0; }      // (sg_is_identity's body: that wrapper is device-only)
        else if (site == 2) { ristretto_encode(out32 + 32 * i, pts[i]); is_identity_out[i] = ge_is_identity_ristretto(pts[i]) ? 1 : 0; }
        else if (site == 3) { const ge5 p = h51::from_ge(pts[i]); h51::encode(out32 + 32 * i, p); is_identity_out[i] = h51::is_identity_ristretto(p) ? 1 : 0; }
    }
    for (size_t first = 0; site == 4 && first < n; first += 8) {      // eight lanes a batch, in the caller's order; a short last batch is filled with (0, 1, 1, 0)
        ge5 lanes[8]; uint8_t enc[8][32];
        const size_t cnt = n - first < 8 ? n - first : 8;
        for (size_t l = 0; l < 8; l++) lanes[l] = l < cnt ? h51::from_ge(pts[first + l]) : h51::identity();
        h8::encode8(enc, lanes);
        for (size_t l = 0; l < cnt; l++) { memcpy(out32 + 32 * (first + l), enc[l], 32); is_identity_out[first + l] = h51::is_identity_ristretto(lanes[l]) ? 1 : 0; }
    }
    return ROFL_OK;
}
// The float-to-fixed rule (conversion32.rs:11-18) as each device site compiles it, on the caller's raw values: the production kernels with the
// launch geometry, clip bounds and block count of their launch sites (create_batch_impl, l2_create_batch), and k_dbg_quant for sg_f32_to_sc.
int rofl_dbg_quantize(unsigned site, size_t rows, size_t d, size_t dpad, size_t prove_range, unsigned fp_bits, unsigned fp_frac,
                      const float *values, const uint8_t *blindings32, void *out, float *terms_out, uint32_t *status_out) {
    if (site > 2 || !valid_fp(fp_bits, fp_frac) || rows == 0 || d == 0 || !values || !out) return fail(ROFL_BAD_PARAM, "bad parameter");
    if (site != 0) dpad = d;
    if (dpad < d || rows > (1u << 20) || dpad > (1u << 20) || rows * dpad > (1u << 20)) return fail(ROFL_BAD_PARAM, "bad parameter");
    if (site == 0 && (prove_range == 0 || prove_range > fp_bits || !status_out)) return fail(ROFL_BAD_PARAM, "bad parameter");
    if (site == 1 && (prove_range == 0 || prove_range > 128 || !blindings32 || !terms_out || !status_out)) return fail(ROFL_BAD_PARAM, "bad parameter");
    return guarded([&]() -> int {
        LaneLock lane_lock = acquire_lane(); Ctx &C = *lane_lock.c;
        C.init();
        const size_t n = rows * d;
        float *dv = C.vals.as<float>(n + 1);
        u32 *status = C.status.as<u32>(rows + 4);
        HIPCHK(hipMemsetAsync(status, 0, 4 * (rows + 4), C.stream));
        C.up(dv, values, 4 * n, C.stream);
        float mn = 0, mx = 0; if (site != 2) clip_bounds(prove_range, fp_bits, fp_frac, &mn, &mx);
        if (site == 0) {
            u64 *vshift = C.vshift.as<u64>(rows * dpad);
            HIPCHK(hipMemsetAsync(vshift, 0xff, 8 * rows * dpad, C.stream));      // (padding words come back 0 because the kernel writes them)
            ROFL_LAUNCH(k_quantize_shift, grid1(dpad, (u32)rows), dim3(TPB), 0, C.stream, dv, (u32)d, (u32)dpad, (u32)prove_range, fp_bits, fp_frac, mn, mx, vshift, status);
            C.down(out, vshift, 8 * rows * dpad, C.stream);
        } else if (site == 1) {
            const u32 nblk = l2_sum_blocks(d);
            float *dterms = C.tmp_out.as<float>(n);
            sc *dbl = C.blind.as<sc>(n), *part_bl = C.tmp_in2.as<sc>(rows * nblk), *dsums = C.aux_scal.as<sc>(2 * rows);
            u64 *part_sq = C.tmp_in.as<u64>(rows * nblk * 3);
            C.up(dbl, blindings32, 32 * n, C.stream);
            ROFL_LAUNCH(k_l2_sumsq_batch, dim3(nblk, (unsigned)rows), dim3(TPB), 0, C.stream, (u32)d, fp_bits, fp_frac, mn, mx, (const float *)dv, (const sc *)dbl, dterms, part_sq, part_bl, status);
            ROFL_LAUNCH(k_l2_sumsq_combine, dim3((unsigned)((rows + 63) / 64)), dim3(64), 0, C.stream, (u32)rows, nblk, (const u64 *)part_sq, (const sc *)part_bl, dsums);
            C.down(terms_out, dterms, 4 * n, C.stream);
            C.down(out, dsums, sizeof(sc) * 2 * rows, C.stream);
        } else {
            sc *ds = C.aux_scal.as<sc>(n);
            ROFL_LAUNCH(k_dbg_quant, grid1(n), dim3(TPB), 0, C.stream, (u32)n, fp_bits, fp_frac, (const float *)dv, ds);
            C.down(out, ds, sizeof(sc) * n, C.stream);
        }
        if (site != 2) C.down(status_out, status, 4 * rows, C.stream);
        C.sync();
        return ROFL_OK;
    });
}
int rofl_discrete_log_vec(const uint8_t *points32, size_t d, size_t table_size, unsigned bsgs_bits, uint8_t *scalars_out32) {
    return guarded([&]() -> int {
        LaneLock lane_lock = acquire_lane(true); Ctx &C = *lane_lock.c;
        if (table_size == 0 || table_size >= (1u << 30) || !(bsgs_bits == 8 || bsgs_bits == 16 || bsgs_bits == 32)) return fail(ROFL_BAD_PARAM, "bad parameter");
        if (d == 0) return ROFL_OK;
        C.init();
        timing_begin(C);
        uint8_t *dp = C.tmp_in.as<uint8_t>(d * 32), *dout = C.Cbytes.as<uint8_t>(d * 32);
        u32 *status = C.status.as<u32>(4);
        HIPCHK(hipMemsetAsync(status, 0, 16, C.stream));
        C.up(dp, points32, 32 * d, C.stream);
        bsgs_solve_launch(C, d, dp, table_size, bsgs_bits, dout, status);
        u32 st = 0;
        C.down(scalars_out32, dout, 32 * d, C.stream);
        HIPCHK(hipMemcpyAsync(&st, status, 4, hipMemcpyDeviceToHost, C.stream));
        C.sync();
        timing_end(C);
        if (st & 4u) return fail(ROFL_FORMAT_ERROR, "invalid Ristretto encoding");
        if (st & 8u) return fail(ROFL_BAD_PARAM, "discrete log not found (the reference unwraps None)");
        return ROFL_OK;
    });
}
// ---- server-side aggregation on the device (params.rs:74-147, server.rs:504-507, 696-714) ----
int rofl_acc_create(size_t d, int init, uint64_t *handle_out) {
    if (!handle_out || d == 0 || (init != 0 && init != 1)) return fail(ROFL_BAD_PARAM, "bad parameter");
    if (d >= ((size_t)1 << 31)) return fail(ROFL_BAD_PARAM, "accumulator too large");
    auto A = std::make_shared<Acc>();
    A->d = d; A->init = init; A->device = current_device();
    DeviceBinding bind(A->device);
    int rc = guarded([&]() -> int {
        LaneLock lane_lock = acquire_lane(); Ctx &C = *lane_lock.c;
        C.init();
        HIPCHK(hipMalloc(&A->sum, sizeof(ge) * 2 * d));
        acc_reset_launch(C, *A);
        C.sync();
        return ROFL_OK;
    });
    if (rc) { if (A->sum) (void)hipFree(A->sum); return rc; }
    *handle_out = g_accs.add(A);
    return ROFL_OK;
}
int rofl_acc_add(uint64_t h, size_t n_clients, const uint8_t *const *records, const size_t *d_each, size_t stride) {
    if (stride < 64 || (n_clients && !records)) return fail(ROFL_BAD_PARAM, "bad parameter");
    std::vector<size_t> cl, nrec;      // the clients that add anything: zip truncation to the accumulator's length (params.rs:81-90)
    return with_acc(h, [&](Acc &A) -> int {
        size_t bytes;
        if (__builtin_mul_overflow(n_clients, A.d, &bytes) || __builtin_mul_overflow(bytes, stride, &bytes)) return fail(ROFL_BAD_PARAM, "batch too large");
        for (size_t c = 0; c < n_clients; c++) {
            size_t n = std::min(d_each ? d_each[c] : A.d, A.d);
            if (!n) continue;
            if (!records[c]) return fail(ROFL_BAD_PARAM, "bad parameter");
            cl.push_back(c); nrec.push_back(n);
        }
        return ROFL_OK;
    }, [&](Acc &A) -> int {
        if (cl.empty()) return ROFL_OK;
        LaneLock lane_lock = acquire_lane(); return acc_add_impl(*lane_lock.c, A, cl, nrec, records, stride); });
}
int rofl_acc_export(uint64_t h, uint8_t *pairs_out) {
    if (!pairs_out) return fail(ROFL_BAD_PARAM, "bad parameter");
    return with_acc(h, no_check, [&](Acc &A) -> int {
        LaneLock lane_lock = acquire_lane(); Ctx &C = *lane_lock.c;
        C.init();
        const size_t d = A.d;
        uint8_t *o = C.Cbytes.as<uint8_t>(d * 64);
        const ge b = acc_init_point(A.init);
        ROFL_LAUNCH(k_acc_finish, grid1(2 * d), dim3(TPB), 0, C.stream, (u32)d, 1, (const ge *)A.sum, b.X, b.Y, o, (u32 *)nullptr);
        C.down(pairs_out, o, d * 64, C.stream);
        C.sync();
        return ROFL_OK;
    });
}
int rofl_acc_extract(uint64_t h, size_t table_size, unsigned bsgs_bits, unsigned fp_bits, unsigned fp_frac, float *out, int *ok_out) {
    return acc_extract(h, nullptr, table_size, bsgs_bits, fp_bits, fp_frac, out, ok_out, nullptr);
}
// Extraction after rejections: the accepted clients' blindings leave a residual s in every pair of the sum, and the caller hands in its
// opening -- as d scalars (host or device memory) or as the signed seeds it is the sum of.  Every R equation is checked before anything is
// extracted; see include/rofl_zk.h.
int rofl_acc_extract_opened(uint64_t h, const uint8_t *opening32, size_t table_size, unsigned bsgs_bits, unsigned fp_bits, unsigned fp_frac,
                            float *out, int *ok_out, size_t *first_bad_out) {
    if (!opening32) return fail(ROFL_BAD_PARAM, "bad parameter");
    const AccOpening op{opening32, 0, nullptr};
    return acc_extract(h, &op, table_size, bsgs_bits, fp_bits, fp_frac, out, ok_out, first_bad_out);
}
int rofl_acc_extract_opened_terms(uint64_t h, size_t term_count, const rofl_blind_term_t *terms, size_t table_size, unsigned bsgs_bits, unsigned fp_bits,
                                  unsigned fp_frac, float *out, int *ok_out, size_t *first_bad_out) {
    size_t total = 0;
    if (int rc = blind_terms_check(term_count, terms, &total)) return rc;
    const AccOpening op{nullptr, term_count, terms};
    return acc_extract(h, &op, table_size, bsgs_bits, fp_bits, fp_frac, out, ok_out, first_bad_out);
}
int rofl_acc_reset(uint64_t h) {
    return with_acc(h, no_check, [&](Acc &A) -> int { LaneLock lane_lock = acquire_lane(); Ctx &C = *lane_lock.c; C.init(); acc_reset_launch(C, A); C.sync(); return ROFL_OK; });
}
int rofl_acc_destroy(uint64_t h) {
    return destroy_handle(g_accs, h, &Acc::mu, kNoAcc, [](Acc &A) { dev_free(A.sum); dev_free(A.work); });
}
// ---- a round resident on the device: ingested once, verified and accumulated from the decoded points; a ROFL_ROUND_COMPRESSED round also
// ---- hashes its CompressedRandProof transcript prefixes at ingest, and its compressed leg reads nothing but the round ----
int rofl_round_create(size_t d, size_t record_len, size_t max_clients, uint64_t *handle_out) { return rofl_round_create_ex(d, record_len, max_clients, 0, handle_out); }
namespace {
// what rofl_round_create_ex and rofl_round_create_rand share, after their own checks of (record_len, flags); keep_prefixes: ingest hashes
// and keeps the CompressedRandProof transcript prefixes (Round::flags carries ROFL_ROUND_COMPRESSED for it, whatever the record length)
int round_create(size_t d, size_t record_len, size_t max_clients, bool keep_prefixes, uint64_t *handle_out) {
    if (!handle_out || d == 0 || max_clients == 0 || (record_len != 64 && record_len != 96)) return fail(ROFL_BAD_PARAM, "bad parameter");
    if (keep_prefixes && d >= 900000)      // (the label table of the reference's transcript ends there, as in rofl_verify_compressed_randproof)
        return fail(ROFL_BAD_PARAM, "a round that keeps CompressedRandProof transcripts holds records of d < 900000");
    const unsigned flags = keep_prefixes ? ROFL_ROUND_COMPRESSED : 0u;
    const size_t npts = record_len / 32;
    size_t bytes;      // the larger array: max_clients * 2 npts * d decoded points
    if (__builtin_mul_overflow(max_clients, d, &bytes) || __builtin_mul_overflow(bytes, 2 * npts * sizeof(niels), &bytes)) return fail(ROFL_BAD_PARAM, "round too large");
    if (max_clients > kMaxBatchMembers || max_clients * 2 * npts * d >= ((size_t)1 << 31)) return fail(ROFL_BAD_PARAM, "round too large (split it)");      // what the Sigma leg's kernels index
    auto R = std::make_shared<Round>();
    R->d = d; R->rec_len = record_len; R->npts = npts; R->max_clients = max_clients; R->flags = flags; R->device = current_device();
    DeviceBinding bind(R->device);
    int rc = guarded([&]() -> int {
        LaneLock lane_lock = acquire_lane(); Ctx &C = *lane_lock.c;
        C.init();
        R->bad.assign(3 * max_clients, ~0u);
        if (flags & ROFL_ROUND_COMPRESSED) R->prefix.reserve(max_clients);
        HIPCHK(hipMalloc(&R->rec, max_clients * d * record_len));
        HIPCHK(hipMalloc(&R->pts, max_clients * 2 * npts * d * sizeof(niels)));
        HIPCHK(hipMalloc(&R->d_bad, 12 * max_clients));
        return ROFL_OK;
    });
    if (rc) { if (R->rec) (void)hipFree(R->rec); if (R->pts) (void)hipFree(R->pts); if (R->d_bad) (void)hipFree(R->d_bad); return rc; }
    *handle_out = g_rounds.add(R);
    return ROFL_OK;
}
}  // namespace
int rofl_round_create_ex(size_t d, size_t record_len, size_t max_clients, unsigned flags, uint64_t *handle_out) {
    if (!handle_out || d == 0 || max_clients == 0 || (record_len != 64 && record_len != 96)) return fail(ROFL_BAD_PARAM, "bad parameter");
    if (flags & ~(unsigned)ROFL_ROUND_COMPRESSED) return fail(ROFL_BAD_PARAM, "unknown round flag");
    if ((flags & ROFL_ROUND_COMPRESSED) && record_len != 64) return fail(ROFL_BAD_PARAM, "a compressed round holds 64-byte records of d < 900000 (96-byte records: rofl_round_create_rand)");
    return round_create(d, record_len, max_clients, (flags & ROFL_ROUND_COMPRESSED) != 0, handle_out);
}
int rofl_round_create_rand(size_t d, size_t record_len, size_t max_clients, uint64_t *handle_out) { return round_create(d, record_len, max_clients, true, handle_out); }
int rofl_round_ingest(uint64_t h, size_t n_clients, const uint8_t *const *records, size_t *first_index_out) {
    if (n_clients && !records) return fail(ROFL_BAD_PARAM, "bad parameter");
    return with_round<RoundExclusive>(h, nullptr, [&](Round &) -> int {
        for (size_t i = 0; i < n_clients; i++) if (!records[i]) return fail(ROFL_BAD_PARAM, "bad parameter");
        return ROFL_OK;
    }, [&](Round &R) -> int {
        if (n_clients > R.max_clients - R.n) return fail(ROFL_BAD_PARAM, "the round is full (nothing ingested)");
        if (first_index_out) *first_index_out = R.n;
        if (!n_clients) return ROFL_OK;
        LaneLock lane_lock = acquire_lane(); return round_ingest_impl(*lane_lock.c, R, n_clients, records); });
}
int rofl_round_verify_sigma(uint64_t h, int kind, const uint8_t *const *proofs, int *ok_out, uint8_t *csq_sum_out32) {
    if (!ok_out || !proofs || kind < 0 || kind > 2) return fail(ROFL_BAD_PARAM, "bad parameter");
    return with_round<RoundShared>(h, &Round::sigma_mu, [&](Round &R) -> int {
        return (kind == 0) != (R.rec_len == 64) ? fail(ROFL_BAD_PARAM, "the proof kind does not fit the round's records") : ROFL_OK;
    }, [&](Round &R) -> int {
        const RoundSrc rs = R.src();
        return sigma_verify_batch(kind, R.n, proofs, nullptr, R.d, ok_out, csq_sum_out32, false, &rs); });
}
int rofl_round_verify_range(uint64_t h, const uint8_t *const *proofs, size_t proof_len, size_t n_proofs, size_t k_checked, size_t prove_range,
                            unsigned fp_bits, unsigned fp_frac, const uint8_t verifier_seed[32], int *ok_out) {
    if (!ok_out || !proofs || !verifier_seed) return fail(ROFL_BAD_PARAM, "bad parameter");
    return with_round<RoundShared>(h, &Round::range_mu, [&](Round &R) -> int {
        return k_checked == 0 || k_checked > R.d ? fail(ROFL_BAD_PARAM, "k_checked outside the round's records") : ROFL_OK;
    }, [&](Round &R) -> int {
        if (R.n == 0) return ROFL_OK;
        const RoundSrc rs = R.src();
        LaneLock lane_lock = acquire_lane(); Ctx &C = *lane_lock.c;
        return verify_impl(C, R.n, proofs, proof_len, n_proofs, nullptr, k_checked, prove_range, fp_bits, fp_frac, verifier_seed, ok_out, false, nullptr, 32, 0, 0, &rs); });
}
int rofl_round_verify_compressed(uint64_t h, const uint8_t *const *proofs, int *ok_out) {
    if (!ok_out || !proofs) return fail(ROFL_BAD_PARAM, "bad parameter");
    return with_round<RoundShared>(h, &Round::comp_mu, [&](Round &R) -> int {
        return !(R.flags & ROFL_ROUND_COMPRESSED) ? fail(ROFL_BAD_PARAM, "the round keeps no transcript prefixes (create it with ROFL_ROUND_COMPRESSED or rofl_round_create_rand)") : ROFL_OK;
    }, [&](Round &R) -> int {
        if (R.n == 0) return ROFL_OK;
        LaneLock lane_lock = acquire_lane(); return round_verify_compressed_impl(*lane_lock.c, R, proofs, ok_out); });
}
int rofl_round_accumulate(uint64_t h, uint64_t acc, const int *accept) {
    std::shared_ptr<Acc> A;
    return with_round<RoundExclusive>(h, nullptr, [&](Round &) -> int {
        A = g_accs.find(acc);
        return A ? ROFL_OK : fail(ROFL_BAD_PARAM, kNoAcc);
    }, [&](Round &R) -> int {
        std::lock_guard<std::mutex> la(A->mu);
        if (A->dead) return fail(ROFL_BAD_PARAM, kNoAcc);
        if (A->d != R.d || A->device != R.device) return fail(ROFL_BAD_PARAM, "the accumulator does not fit the round (length or device)");
        std::vector<u32> cl;
        for (size_t i = 0; i < R.n; i++) if (!accept || accept[i]) cl.push_back((u32)i);
        LaneLock lane_lock = acquire_lane(); return round_accumulate_impl(*lane_lock.c, R, *A, cl); });
}
int rofl_round_reset(uint64_t h) {
    return with_round<RoundExclusive>(h, nullptr, no_check, [&](Round &R) -> int { R.n = 0; R.prefix.clear(); return ROFL_OK; });
}
int rofl_round_destroy(uint64_t h) {
    return destroy_handle(g_rounds, h, &Round::rw, kNoRound, [](Round &R) { dev_free(R.rec); dev_free(R.pts); dev_free(R.d_bad); });
}
int rofl_dbg_point_decodes(uint64_t *count_out) { if (!count_out) return ROFL_BAD_PARAM; *count_out = g_point_decodes.load(); return ROFL_OK; }
size_t rofl_wire_encoded_size(const rofl_wire_msg_t *m) { return m ? wire::encoded_size(*m) : 0; }
int rofl_wire_encode(const rofl_wire_msg_t *m, uint8_t *out, size_t cap, size_t *len_out) {
    if (!m || !out) return fail(ROFL_BAD_PARAM, "bad parameter");
    int rc = wire::encode(*m, out, cap, len_out);
    return rc ? fail(rc, "wire encode: unknown message kind or output buffer too small") : ROFL_OK;
}
int rofl_wire_decode(int kind, const uint8_t *data, size_t len, rofl_wire_msg_t *m, uint8_t *range_proofs_out, size_t range_proofs_cap) {
    if (!m || !data) return fail(ROFL_BAD_PARAM, "bad parameter");
    int rc = wire::decode(kind, data, len, m, range_proofs_out, range_proofs_cap);
    return rc ? fail(rc, rc == ROFL_FORMAT_ERROR ? "malformed message (prost's decode_length_delimited would return Err; the reference unwraps it)" : "bad parameter") : ROFL_OK;
}
}  // extern "C"

// ================================================================ multi-process exchange (RCCL over xGMI)
// One process per GPU: the exchange steps of a round -- all-gather of [verdict | proof bytes | commitments] of every rank, MIN / MAX / SUM
// reductions of a few numbers -- for hosts that are NOT Python (a C / Rust rofl_service has no torch.distributed), and so that every rank of
// a node runs the proof path AND its collectives on ONE HIP runtime: librccl is loaded here, next to the runtime this library is bound to.
// Payloads live in host memory at the ABI (proofs and commitments are returned to the host; SURVEY 8(e): no collective inside the proof
// path): they are staged through the communicator's pinned buffers, all-gathered device to device, and handed back in host memory.
namespace {
struct Rccl {
    void *h = nullptr; std::string path, err;
    ncclResult_t (*GetVersion)(int *) = nullptr;
    ncclResult_t (*GetUniqueId)(ncclUniqueId *) = nullptr;
    ncclResult_t (*CommInitRank)(ncclComm_t *, int, ncclUniqueId, int) = nullptr;
    ncclResult_t (*AllGather)(const void *, void *, size_t, ncclDataType_t, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*AllReduce)(const void *, void *, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
    const char *(*GetErrorString)(ncclResult_t) = nullptr;
};
Rccl &rccl() {
    static Rccl r; static std::once_flag once;
    std::call_once(once, [] {
        // ROFL_RCCL_LIB: which librccl (default: by soname, i.e. the one of the ROCm installation the process links).  A Python host that has
        // imported torch names /opt/rocm/lib/librccl.so.1 explicitly: "librccl.so.1" alone would resolve to the copy torch bundles.
        const char *e = knob("ROFL_RCCL_LIB");
        r.path = e && *e ? e : "librccl.so.1";
        r.h = dlopen(r.path.c_str(), RTLD_NOW | RTLD_LOCAL);
        if (!r.h) { const char *m = dlerror(); r.err = m ? m : "dlopen failed"; return; }
        auto sym = [&](const char *n) { void *f = dlsym(r.h, n); if (!f && r.err.empty()) r.err = std::string("missing symbol ") + n; return f; };
        r.GetVersion = reinterpret_cast<decltype(r.GetVersion)>(sym("ncclGetVersion"));
        r.GetUniqueId = reinterpret_cast<decltype(r.GetUniqueId)>(sym("ncclGetUniqueId"));
        r.CommInitRank = reinterpret_cast<decltype(r.CommInitRank)>(sym("ncclCommInitRank"));
        r.AllGather = reinterpret_cast<decltype(r.AllGather)>(sym("ncclAllGather"));
        r.AllReduce = reinterpret_cast<decltype(r.AllReduce)>(sym("ncclAllReduce"));
        r.CommDestroy = reinterpret_cast<decltype(r.CommDestroy)>(sym("ncclCommDestroy"));
        r.GetErrorString = reinterpret_cast<decltype(r.GetErrorString)>(sym("ncclGetErrorString"));
        if (!r.err.empty()) { dlclose(r.h); r.h = nullptr; }
    });
    return r;
}
struct NcclErr { ncclResult_t e; const char *what; };
#define NCCLCHK(x) do { ncclResult_t e__ = (x); if (e__ != ncclSuccess) throw NcclErr{e__, #x}; } while (0)
struct CommState {
    std::mutex mu; ncclComm_t comm = nullptr; int rank = 0, world = 0, phys = 0; hipStream_t st = nullptr;
    DevBuf send, recv; PinBuf hsend, hrecv;
};
CommState g_comm;
template <class F> int comm_guarded(F f) {
    return guarded([&]() -> int {
        try { return f(); }
        catch (const NcclErr &e) {
            Rccl &R = rccl();
            return fail(ROFL_COMM_ERROR, std::string("RCCL error ") + std::to_string((int)e.e) + " (" + (R.GetErrorString ? R.GetErrorString(e.e) : "?") + ") in " + e.what);
        }
    });
}
int comm_ready(Rccl *&R) {
    R = &rccl();
    if (!R->h) return fail(ROFL_COMM_ERROR, "librccl could not be loaded (" + R->path + "): " + R->err);
    return ROFL_OK;
}
}  // namespace

extern "C" {
int rofl_comm_unique_id(uint8_t id_out[128]) {
    return comm_guarded([&]() -> int {
        Rccl *R; if (int rc = comm_ready(R)) return rc;
        if (!id_out) return fail(ROFL_BAD_PARAM, "bad parameter");
        static_assert(sizeof(ncclUniqueId) == 128, "ncclUniqueId is 128 bytes");
        ncclUniqueId id; NCCLCHK(R->GetUniqueId(&id)); memcpy(id_out, &id, 128); return ROFL_OK;
    });
}
int rofl_comm_init(const uint8_t id[128], int rank, int world) {
    return comm_guarded([&]() -> int {
        Rccl *R; if (int rc = comm_ready(R)) return rc;
        if (!id || world < 1 || rank < 0 || rank >= world) return fail(ROFL_BAD_PARAM, "bad parameter");
        std::lock_guard<std::mutex> lk(g_comm.mu);
        if (g_comm.comm) return fail(ROFL_BAD_PARAM, "a communicator already exists in this process (rofl_comm_destroy first)");
        Ctx &P = ctx(); { std::lock_guard<std::mutex> g(P.init_mu); P.init(); }      // the calling thread's device: one process per GPU
        HIPCHK(hipSetDevice(P.phys));
        ncclUniqueId uid; memcpy(&uid, id, 128);
        ncclComm_t c = nullptr;
        NCCLCHK(R->CommInitRank(&c, world, uid, rank));
        g_comm.comm = c; g_comm.rank = rank; g_comm.world = world; g_comm.phys = P.phys;
        HIPCHK(hipStreamCreateWithFlags(&g_comm.st, hipStreamNonBlocking));
        return ROFL_OK;
    });
}
int rofl_comm_info(int *rank_out, int *world_out, int *rccl_version_out, char *lib_path_out, size_t len) {
    Rccl &R = rccl();
    std::lock_guard<std::mutex> lk(g_comm.mu);
    if (rank_out) *rank_out = g_comm.comm ? g_comm.rank : -1;
    if (world_out) *world_out = g_comm.comm ? g_comm.world : 0;
    if (rccl_version_out) { int v = 0; if (R.h && R.GetVersion) (void)R.GetVersion(&v); *rccl_version_out = v; }
    if (lib_path_out && len) {      // the file that was mapped, not the name it was asked for
        std::string real = R.path;
        if (R.h) { Dl_info di; if (dladdr((void *)R.GetVersion, &di) && di.dli_fname) real = di.dli_fname; }
        snprintf(lib_path_out, len, "%s", real.c_str());
    }
    return R.h ? ROFL_OK : fail(ROFL_COMM_ERROR, "librccl could not be loaded (" + R.path + "): " + R.err);
}
int rofl_comm_allgather(const uint8_t *local, size_t n, uint8_t *all_out) {
    return comm_guarded([&]() -> int {
        Rccl *R; if (int rc = comm_ready(R)) return rc;
        std::lock_guard<std::mutex> lk(g_comm.mu);
        if (!g_comm.comm) return fail(ROFL_BAD_PARAM, "no communicator (rofl_comm_init)");
        if (!n) return ROFL_OK;
        if (!local || !all_out) return fail(ROFL_BAD_PARAM, "bad parameter");
        HIPCHK(hipSetDevice(g_comm.phys));
        const size_t W = (size_t)g_comm.world;
        uint8_t *ds = g_comm.send.as<uint8_t>(n), *dr = g_comm.recv.as<uint8_t>(n * W);
        uint8_t *hs = g_comm.hsend.as<uint8_t>(n), *hr = g_comm.hrecv.as<uint8_t>(n * W);
        memcpy(hs, local, n);
        HIPCHK(hipMemcpyAsync(ds, hs, n, hipMemcpyHostToDevice, g_comm.st));
        NCCLCHK(R->AllGather(ds, dr, n, ncclUint8, g_comm.comm, g_comm.st));
        HIPCHK(hipMemcpyAsync(hr, dr, n * W, hipMemcpyDeviceToHost, g_comm.st));
        HIPCHK(hipStreamSynchronize(g_comm.st));
        memcpy(all_out, hr, n * W);
        return ROFL_OK;
    });
}
int rofl_comm_allreduce_f64(double *inout, size_t count, int op) {
    return comm_guarded([&]() -> int {
        Rccl *R; if (int rc = comm_ready(R)) return rc;
        std::lock_guard<std::mutex> lk(g_comm.mu);
        if (!g_comm.comm) return fail(ROFL_BAD_PARAM, "no communicator (rofl_comm_init)");
        if (!inout || !count || count > 4096 || op < 0 || op > 2) return fail(ROFL_BAD_PARAM, "bad parameter");
        HIPCHK(hipSetDevice(g_comm.phys));
        double *d = g_comm.send.as<double>(count), *h = g_comm.hsend.as<double>(count);
        memcpy(h, inout, 8 * count);
        HIPCHK(hipMemcpyAsync(d, h, 8 * count, hipMemcpyHostToDevice, g_comm.st));
        NCCLCHK(R->AllReduce(d, d, count, ncclFloat64, op == 0 ? ncclSum : op == 1 ? ncclMin : ncclMax, g_comm.comm, g_comm.st));
        HIPCHK(hipMemcpyAsync(h, d, 8 * count, hipMemcpyDeviceToHost, g_comm.st));
        HIPCHK(hipStreamSynchronize(g_comm.st));
        memcpy(inout, h, 8 * count);
        return ROFL_OK;
    });
}
int rofl_comm_barrier(void) { double one = 1.0; return rofl_comm_allreduce_f64(&one, 1, 0); }
int rofl_comm_destroy(void) {
    return comm_guarded([&]() -> int {
        std::lock_guard<std::mutex> lk(g_comm.mu);
        if (!g_comm.comm) return ROFL_OK;
        Rccl &R = rccl();
        (void)hipSetDevice(g_comm.phys);
        if (g_comm.st) { (void)hipStreamSynchronize(g_comm.st); (void)hipStreamDestroy(g_comm.st); g_comm.st = nullptr; }
        ncclComm_t c = g_comm.comm; g_comm.comm = nullptr; g_comm.world = 0;
        NCCLCHK(R.CommDestroy(c));
        return ROFL_OK;
    });
}
}  // extern "C"

extern "C" {
namespace {
struct OptSlot { std::atomic<int> *i; std::atomic<long> *l; long lo, hi; };
bool option_slot(const char *key, OptSlot *o) {
    Options &O = opts();
    const struct { const char *k; OptSlot s; } tab[] = {
        {"verify_zip_truncate", {&O.zip_truncate, nullptr, 0, 1}}, {"verify_batch", {&O.verify_batch, nullptr, 0, 2}},
        {"sigma_batch", {&O.sigma_batch, nullptr, 0, 1}}, {"blocking_sync", {&O.blocking_sync, nullptr, -1, 1}},
        {"devices", {nullptr, &O.devices, 0, (long)(~0UL >> 1)}}};
    for (auto &t : tab) if (key && !strcmp(key, t.k)) { *o = t.s; return true; }
    return false;
}
}  // namespace
int rofl_set_option(const char *key, long value) {
    if (key && !strcmp(key, "default_device")) {      // the device of threads that never called rofl_set_device (otherwise: the first device that was set)
        if (value < 0 || value >= kMaxDevices) return fail(ROFL_BAD_PARAM, "unknown option or value out of range");
        g_default_device.store((int)value); g_default_set.store(true); return ROFL_OK;
    }
    OptSlot o;
    if (!option_slot(key, &o) || value < o.lo || value > o.hi) return fail(ROFL_BAD_PARAM, "unknown option or value out of range");
    if (o.i) o.i->store((int)value); else o.l->store(value);
    return ROFL_OK;
}
int rofl_get_option(const char *key, long *value_out) {
    if (!value_out) return fail(ROFL_BAD_PARAM, "bad parameter");
    if (key && !strcmp(key, "lanes")) {      // read-only: the lanes of the calling thread's device (ROFL_LANES after clamping)
        return guarded([&]() -> int { Ctx &P = ctx(); { std::lock_guard<std::mutex> g(P.init_mu); P.init(); } *value_out = P.nlanes; return ROFL_OK; });
    }
    if (key && !strcmp(key, "default_device")) { *value_out = g_default_device.load(); return ROFL_OK; }
    OptSlot o;
    if (!option_slot(key, &o)) return fail(ROFL_BAD_PARAM, "unknown option");
    *value_out = o.i ? (long)o.i->load() : o.l->load();
    return ROFL_OK;
}
int rofl_set_timing(int enabled) {
    return guarded([&]() -> int {
        Ctx &P = ctx(); { std::lock_guard<std::mutex> g(P.init_mu); P.init(); }
        { std::lock_guard<std::mutex> lk(P.mu); P.tm.enabled = enabled == 1; P.tm.acc_only = enabled == 2; }
        for (Ctx *s : P.sibs) { std::lock_guard<std::mutex> lk(s->mu); s->tm.enabled = enabled == 1; s->tm.acc_only = enabled == 2; }
        return ROFL_OK;
    });
}
/* timing of the last instrumented call made by the calling thread */
int rofl_last_timing(rofl_timing_t *out) { if (!out) return ROFL_BAD_PARAM; *out = g_last_timing; return ROFL_OK; }
int rofl_last_kernel_times(rofl_kernel_time_t *out) { if (!out) return ROFL_BAD_PARAM; memcpy(out, g_last_ktimes, sizeof g_last_ktimes); return ROFL_OK; }
int rofl_bench_femul(unsigned iters, double *out) {
    return guarded([&]() -> int {
        LaneLock lane_lock = acquire_lane(); Ctx &C = *lane_lock.c; C.init();
        const u32 blocks = 256 * 8, threads = blocks * TPB;
        fe *din, *dout; HIPCHK(hipMalloc(&din, sizeof(fe) * 256)); HIPCHK(hipMalloc(&dout, sizeof(fe) * threads));
        std::vector<fe> h(256); for (int i = 0; i < 256; i++) for (int k = 0; k < 8; k++) h[i].v[k] = 0x9e3779b9u * (i * 8 + k + 1);
        HIPCHK(hipMemcpy(din, h.data(), sizeof(fe) * 256, hipMemcpyHostToDevice));
        hipEvent_t e0, e1; HIPCHK(hipEventCreate(&e0)); HIPCHK(hipEventCreate(&e1));
        // ROFL_FEMUL_LDS: dynamic LDS per block, to hold the microbenchmark at the occupancy of a real kernel (40960 -> 4 blocks per CU =
        // 4 waves/SIMD, what k_msm_accumulate's 127 VGPRs allow); default 0 = 8 waves/SIMD
        static const size_t fl = knob("ROFL_FEMUL_LDS") ? (size_t)atol(knob("ROFL_FEMUL_LDS")) : 0;
        if (fl) HIPCHK(hipFuncSetAttribute((const void *)k_bench_femul, hipFuncAttributeMaxDynamicSharedMemorySize, (int)fl));
        // ROFL_FEMUL_MODE = 1 / 2: the 7-multiplication mixed addition instead (entry held in registers / fetched per addition from a 32 KB table)
        static const int mode = knob("ROFL_FEMUL_MODE") ? atoi(knob("ROFL_FEMUL_MODE")) : 0;
        if (mode) {
            // mode 3: ROFL_FEMUL_TABLE entries (power of two, default 2^21 = 256 MB) gathered at random, like the window table is
            static const size_t tab = knob("ROFL_FEMUL_TABLE") ? (size_t)atol(knob("ROFL_FEMUL_TABLE")) : ((size_t)1 << 21);
            size_t entries = mode == 3 ? tab : 256;
            ndm *dt; ge *dg; HIPCHK(hipMalloc(&dt, sizeof(ndm) * entries)); HIPCHK(hipMalloc(&dg, sizeof(ge) * threads));
            HIPCHK(hipMemset(dt, 0x11, sizeof(ndm) * entries));
            std::vector<ndm> ht(256); for (int i = 0; i < 256; i++) for (int k = 0; k < 32; k++) ht[i].v[k] = (0x9e3779b9u * (i * 32 + k + 1)) >> 8;
            HIPCHK(hipMemcpy(dt, ht.data(), sizeof(ndm) * 256, hipMemcpyHostToDevice));
            auto launch = [&](u32 it) {
                if (mode == 3) ROFL_LAUNCH(k_bench_madd_gather, dim3(blocks), dim3(TPB), fl, C.stream, it, (u32)entries, dt, dg);
                else if (mode == 2) ROFL_LAUNCH(k_bench_madd_l1, dim3(blocks), dim3(TPB), fl, C.stream, it, (u32)entries, dt, dg);
                else ROFL_LAUNCH(k_bench_madd_regs, dim3(blocks), dim3(TPB), fl, C.stream, it, (u32)entries, dt, dg);
            };
            launch(8u);
            HIPCHK(hipEventRecord(e0, C.stream));
            launch(iters);
            HIPCHK(hipEventRecord(e1, C.stream));
            HIPCHK(hipEventSynchronize(e1));
            float ms = 0; HIPCHK(hipEventElapsedTime(&ms, e0, e1));
            *out = (double)threads * iters * 7.0 / (ms * 1e-3);
            HIPCHK(hipFree(dt)); HIPCHK(hipFree(dg)); HIPCHK(hipFree(din)); HIPCHK(hipFree(dout)); HIPCHK(hipEventDestroy(e0)); HIPCHK(hipEventDestroy(e1));
            return ROFL_OK;
        }
        ROFL_LAUNCH(k_bench_femul, dim3(blocks), dim3(TPB), fl, C.stream, 8u, din, dout);
        HIPCHK(hipEventRecord(e0, C.stream));
        ROFL_LAUNCH(k_bench_femul, dim3(blocks), dim3(TPB), fl, C.stream, iters, din, dout);
        HIPCHK(hipEventRecord(e1, C.stream));
        HIPCHK(hipEventSynchronize(e1));
        float ms = 0; HIPCHK(hipEventElapsedTime(&ms, e0, e1));
        *out = (double)threads * iters * 4.0 / (ms * 1e-3);
        HIPCHK(hipFree(din)); HIPCHK(hipFree(dout)); HIPCHK(hipEventDestroy(e0)); HIPCHK(hipEventDestroy(e1));
        return ROFL_OK;
    });
}

// ---- host-side self-tests of the shared host/device math (no GPU needed)
int rofl_dbg_host_pool_stress(unsigned threads, unsigned jobs) {
    // many tiny jobs back to back: every index of every job must run exactly once (a lost index would hang run())
    HostPool pool((int)threads);
    for (unsigned it = 0; it < jobs; it++) {
        size_t n = 2 + it % 7;
        std::atomic<int> hits[8];
        for (auto &h : hits) h = 0;
        pool.run(n, [&](size_t i) { hits[i].fetch_add(1); });
        for (size_t i = 0; i < n; i++) if (hits[i].load() != 1) return ROFL_BAD_PARAM;
    }
    return ROFL_OK;
}
int rofl_dbg_host_bench(int what, unsigned iters, double *ns_out) {
    if (!ns_out || !iters) return ROFL_BAD_PARAM;
    static const uint8_t Bc[32] = {0xe2, 0xf2, 0xae, 0x0a, 0x6a, 0xbc, 0x4e, 0x71, 0xa8, 0x84, 0xa9, 0x61, 0xc5, 0x00, 0x51, 0x5f,
                                   0x58, 0xe3, 0x0b, 0x6a, 0xa5, 0x82, 0xdd, 0x8d, 0xb6, 0xa6, 0x59, 0x45, 0xe0, 0x8d, 0x2d, 0x76};
    ge b; ristretto_decode(b, Bc);
    ge5 p = h51::from_ge(b), q = h51::gdouble(p);
    volatile u64 sink = 0;
    double t0 = now_ms();
    if (what == 0) { u64 st[25]; memset(st, 1, sizeof st); for (unsigned i = 0; i < iters; i++) keccak_f1600_host(st); sink = st[0]; }
    else if (what == 1) { for (unsigned i = 0; i < iters; i++) p = h51::gdouble(p); sink = p.X.v[0]; }
    else if (what == 2) { for (unsigned i = 0; i < iters; i++) p = h51::gadd(p, q); sink = p.X.v[0]; }
    else if (what == 3) { uint8_t e[32]; for (unsigned i = 0; i < iters; i++) { h51::encode(e, p); p = h51::gadd(p, q); } sink = p.X.v[0]; }
    else if (what == 4) {
        std::vector<niels> T; std::vector<niels5> T5; build_fixed_table(T, b); to_tab5(T5, T);
        sc k = sc_from_u64(0x123456789abcdefULL); t0 = now_ms();
        for (unsigned i = 0; i < iters; i++) { ge5 r = h_fixed_mul(T5, k); k.v[3] ^= (u32)r.X.v[0]; k.v[7] &= 0x0fffffffu; } sink = k.v[3];
    } else if (what == 5) { sc a = h_mont(sc_from_u64(0xdeadbeefcafeULL)); for (unsigned i = 0; i < iters; i++) { a = h51::sc_invert_mont_fast(a); a.v[0] |= 1; } sink = a.v[0]; }
    else if (what == 6) {
        std::vector<uint8_t> V((size_t)iters * 32); for (size_t i = 0; i < V.size(); i++) V[i] = (uint8_t)(i * 131 + 7);
        t0 = now_ms();
        Merlin t("RangeProof", 10);
        t.append32_run('V', V.data(), iters);
        sink = t.stw[0];
    } else if (what >= 7 && what <= 9) {
        // the pool hand-off of a hop: `iters` times { the caller busy-waits 300 us (what = 7, 9) or 30 us (8) as it does for the GPU, then runs 16
        // tasks of ~30 us (7, 8) or 128 tasks of ~8 us (9) }; result = ns per hand-off beyond nothing (ideal: 16 x 30 / threads, at least 30 us)
        int nt = std::min(16, std::max(2, usable_cores())); if (const char *e = knob("ROFL_HOST_THREADS")) nt = atoi(e);
        HostPool pool(nt);
        auto spin = [](double us) { double t = now_ms(); while ((now_ms() - t) * 1e3 < us) __builtin_ia32_pause(); };
        const size_t ntask = what == 9 ? 128 : 16; const double task_us = what == 9 ? 8.0 : 30.0, gap_us = what == 8 ? 30.0 : 300.0;
        double tot = 0;
        for (unsigned i = 0; i < iters; i++) {
            spin(gap_us);
            double a = now_ms();
            pool.run(ntask, [&](size_t) { spin(task_us); });
            tot += now_ms() - a;
        }
        *ns_out = tot * 1e6 / iters; return ROFL_OK;
    } else return ROFL_BAD_PARAM;
    *ns_out = (now_ms() - t0) * 1e6 / iters; (void)sink;
    return ROFL_OK;
}
// host51x8.hpp against host51.hpp: 8 x W pseudo-random window sums through the SIMD chain and through the scalar one.
// Returns 0 when all eight results agree, 1 on a mismatch, -1 when the CPU has no AVX-512 IFMA (nothing tested).
int rofl_dbg_host_horner8_selftest(unsigned W, unsigned c, int lanes, double *us_simd, double *us_scalar) {
    if (!h8::available()) return -1;
    if (W < 2 || W > 64 || c < 2 || c > 16 || lanes < 1 || lanes > 8) return ROFL_BAD_PARAM;
    static const uint8_t Bc[32] = {0xe2, 0xf2, 0xae, 0x0a, 0x6a, 0xbc, 0x4e, 0x71, 0xa8, 0x84, 0xa9, 0x61, 0xc5, 0x00, 0x51, 0x5f,
                                   0x58, 0xe3, 0x0b, 0x6a, 0xa5, 0x82, 0xdd, 0x8d, 0xb6, 0xa6, 0x59, 0x45, 0xe0, 0x8d, 0x2d, 0x76};
    ge b; ristretto_decode(b, Bc);
    u32 pos[64]; for (unsigned w = 0; w < W; w++) pos[w] = w * c;
    std::vector<ge> pts(8 * W);
    ge5 cur = h51::from_ge(b);
    for (size_t i = 0; i < pts.size(); i++) {
        cur = h51::gadd(h51::gdouble(cur), h51::from_ge(b)); if (i % 3 == 0) cur = h51::gdouble(cur);
        pts[i] = h51::to_ge(cur);
        if (i % 4 == 1) { u64 cy = 0; const u32 pw[8] = {0xffffffedu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0x7fffffffu};      // a loose representative: X + p
                          for (int k = 0; k < 8; k++) { cy += (u64)pts[i].X.v[k] + pw[k]; pts[i].X.v[k] = (u32)cy; cy >>= 32; } }
    }
    auto wsum = [&](int l, int w) { return (const ge *)&pts[(size_t)l * W + w]; };
    uint8_t ref[8][32], got[8][32];
    double t0 = now_ms();
    for (int l = 0; l < lanes; l++) {
        ge5 acc = h51::from_ge_loose(*wsum(l, (int)W - 1));
        for (int w = (int)W - 2; w >= 0; w--) { for (u32 i = pos[w]; i < pos[w + 1]; i++) acc = h51::gdouble(acc); acc = h51::gadd(acc, h51::from_ge_loose(*wsum(l, w))); }
        h51::encode(ref[l], acc);
    }
    double t1 = now_ms();
    ge5 out[8];
    h8::horner8(out, lanes, (int)W, pos, wsum);
    double t2 = now_ms();
    int bad = 0;
    for (int l = 0; l < lanes; l++) { h51::encode(got[l], out[l]); bad |= memcmp(got[l], ref[l], 32) != 0; }
    if (us_simd) *us_simd = (t2 - t1) * 1e3;
    if (us_scalar) *us_scalar = (t1 - t0) * 1e3;
    return bad;
}
// h8::encode8 against h51::encode on `batches` x 8 points of a pseudo-random walk (arbitrary Z), the identity and small multiples included.
// Returns 0 when every encoding agrees, 1 on a mismatch, -1 without AVX-512 IFMA.
int rofl_dbg_host_encode8_selftest(unsigned batches, double *us_simd, double *us_scalar) {
    if (!h8::available()) return -1;
    static const uint8_t Bc[32] = {0xe2, 0xf2, 0xae, 0x0a, 0x6a, 0xbc, 0x4e, 0x71, 0xa8, 0x84, 0xa9, 0x61, 0xc5, 0x00, 0x51, 0x5f,
                                   0x58, 0xe3, 0x0b, 0x6a, 0xa5, 0x82, 0xdd, 0x8d, 0xb6, 0xa6, 0x59, 0x45, 0xe0, 0x8d, 0x2d, 0x76};
    ge b; ristretto_decode(b, Bc);
    ge5 b5 = h51::from_ge(b), cur = b5;
    int bad = 0; double ts = 0, tv = 0;
    for (unsigned it = 0; it < batches; it++) {
        ge5 pts[8];
        for (int l = 0; l < 8; l++) {
            cur = h51::gadd(h51::gdouble(cur), b5); if ((it + l) % 3 == 0) cur = h51::gdouble(cur);
            pts[l] = cur;
        }
        if (it == 0) { pts[0] = h51::identity(); pts[1] = b5; pts[2] = h51::gdouble(b5); pts[3] = h51::gadd(b5, h51::identity()); }
        uint8_t ref[8][32], got[8][32];
        double t0 = now_ms();
        for (int l = 0; l < 8; l++) h51::encode(ref[l], pts[l]);
        double t1 = now_ms();
        h8::encode8(got, pts);
        double t2 = now_ms();
        ts += t1 - t0; tv += t2 - t1;
        bad |= memcmp(ref, got, sizeof ref) != 0;
    }
    if (us_simd) *us_simd = tv * 1e3 / (batches ? batches : 1);
    if (us_scalar) *us_scalar = ts * 1e3 / (batches ? batches : 1);
    return bad;
}
// k8::append32_run_x8 against Merlin::append32_run: `lanes` transcripts that have absorbed the same prefix, `count` commitments each, from every
// starting position of the rate block (`skew` extra prefix bytes shift it); the challenge drawn afterwards must agree.  0 = equal, 1 = mismatch,
// -1 = no AVX-512.  Timings: microseconds for all lanes together.
// Merlin::append32_run (records put together in registers, split at the end of the rate block) against `count` plain append("V", msg, 32)
// calls after `skew` extra prefix bytes: state, positions and the next challenge.  0 = equal, 1 = mismatch.
int rofl_dbg_host_merlin_run_selftest(unsigned count, unsigned skew) {
    if (skew > 400) return ROFL_BAD_PARAM;
    std::vector<uint8_t> data((size_t)count * 32 + 1);
    for (size_t i = 0; i < data.size(); i++) data[i] = (uint8_t)((i * 2246822519u) >> 11);
    std::vector<uint8_t> pre(skew, 0xa5);
    Merlin a("RangeProof", 10), b("RangeProof", 10);
    if (skew) { a.append("skew", pre.data(), skew); b.append("skew", pre.data(), skew); }
    a.append32_run('V', data.data(), count);
    for (unsigned j = 0; j < count; j++) b.append("V", data.data() + (size_t)j * 32, 32);
    int bad = a.pos != b.pos || a.pos_begin != b.pos_begin || a.cur_flags != b.cur_flags || memcmp(a.stw, b.stw, 200) != 0;
    uint8_t ca[64], cb[64]; a.challenge_bytes("y", ca, 64); b.challenge_bytes("y", cb, 64); bad |= memcmp(ca, cb, 64) != 0;
    return bad;
}
// keccak_f1600_zmm (one state across AVX-512 registers) against the scalar permutation on `states` pseudo-random states, chained `chain` deep,
// plus the known answer of the all-zero state.  0 = all equal, 1 = mismatch, -1 = no AVX-512 on this CPU.
int rofl_dbg_host_keccak_zmm_selftest(unsigned states, unsigned chain, double *ns_zmm, double *ns_scalar) {
    if (!__builtin_cpu_supports("avx512f")) return -1;
    if (!states || !chain) return ROFL_BAD_PARAM;
    int bad = 0;
    { u64 z[25] = {0}; keccak_f1600_zmm(z); bad |= z[0] != 0xF1258F7940E1DDE7ULL || z[24] != 0xEAF1FF7B5CECA249ULL; }
    u64 x = 0x9e3779b97f4a7c15ULL;
    double tz = 0, ts = 0;
    for (unsigned i = 0; i < states; i++) {
        u64 a[25], b[25];
        for (int k = 0; k < 25; k++) { x ^= x << 13; x ^= x >> 7; x ^= x << 17; a[k] = b[k] = (i % 5 == 4 && k % 3 == 0) ? 0 : x; }
        double t0 = now_ms();
        for (unsigned c = 0; c < chain; c++) keccak_f1600_zmm(a);
        double t1 = now_ms();
        for (unsigned c = 0; c < chain; c++) keccak_f1600_host(b);
        double t2 = now_ms();
        tz += t1 - t0; ts += t2 - t1;
        bad |= memcmp(a, b, sizeof a) != 0;
    }
    if (ns_zmm) *ns_zmm = tz * 1e6 / ((double)states * chain);
    if (ns_scalar) *ns_scalar = ts * 1e6 / ((double)states * chain);
    return bad;
}
int rofl_dbg_host_merlin8_selftest(int lanes, unsigned count, unsigned skew, double *us_simd, double *us_scalar) {
    if (!k8::available()) return -1;
    if (lanes < 1 || lanes > 8 || skew > 400) return ROFL_BAD_PARAM;
    std::vector<uint8_t> data((size_t)8 * count * 32);
    for (size_t i = 0; i < data.size(); i++) data[i] = (uint8_t)((i * 2654435761u) >> 13);
    std::vector<uint8_t> pre(skew, 0x5a);
    std::vector<Merlin> a, b;
    for (int l = 0; l < lanes; l++) { a.emplace_back("RangeProof", 10); b.emplace_back("RangeProof", 10); }
    for (int l = 0; l < lanes; l++) { uint8_t id = (uint8_t)l; a[l].append("id", &id, 1); b[l].append("id", &id, 1); if (skew) { a[l].append("skew", pre.data(), skew); b[l].append("skew", pre.data(), skew); } }
    double t0 = now_ms();
    for (int l = 0; l < lanes; l++) a[l].append32_run('V', data.data() + (size_t)l * count * 32, count);
    double t1 = now_ms();
    Merlin *t[8]; const uint8_t *msg[8];
    for (int l = 0; l < lanes; l++) { t[l] = &b[l]; msg[l] = data.data() + (size_t)l * count * 32; }
    k8::append32_run_x8(t, lanes, 'V', msg, count);
    double t2 = now_ms();
    int bad = 0;
    for (int l = 0; l < lanes; l++) {
        bad |= a[l].pos != b[l].pos || a[l].pos_begin != b[l].pos_begin || a[l].cur_flags != b[l].cur_flags || memcmp(a[l].stw, b[l].stw, 200) != 0;
        uint8_t ca[64], cb[64]; a[l].challenge_bytes("y", ca, 64); b[l].challenge_bytes("y", cb, 64); bad |= memcmp(ca, cb, 64) != 0;
    }
    if (us_simd) *us_simd = (t2 - t1) * 1e3;
    if (us_scalar) *us_scalar = (t1 - t0) * 1e3;
    return bad;
}
// k8::append_lbl3_run_x8 against `count` Merlin::append_lbl calls per transcript (the labelled pairs of compressed_prefixes): `lanes`
// CompressedRandProof transcripts, `skew` extra prefix bytes, then the pairs, C' and the challenge.  0 = equal, 1 = mismatch, -1 = no AVX-512.
int rofl_dbg_host_merlin8_lbl3_selftest(int lanes, unsigned count, unsigned skew, double *us_simd, double *us_scalar) {
    if (!k8::available()) return -1;
    if (lanes < 1 || lanes > 8 || skew > 400) return ROFL_BAD_PARAM;
    std::vector<uint8_t> data((size_t)8 * count * 64 + 64);
    for (size_t i = 0; i < data.size(); i++) data[i] = (uint8_t)((i * 2654435761u) >> 13);
    std::vector<uint8_t> pre(skew, 0x5a);
    std::vector<Merlin> a, b;
    for (int l = 0; l < lanes; l++) { a.emplace_back("CompressedRandProof", 19); b.emplace_back("CompressedRandProof", 19); }
    for (int l = 0; l < lanes; l++) {
        a[l].append("dom-sep", (const uint8_t *)"randomness proof v1", 19); b[l].append("dom-sep", (const uint8_t *)"randomness proof v1", 19);
        if (skew) { a[l].append("skew", pre.data(), skew); b[l].append("skew", pre.data(), skew); }
    }
    double t0 = now_ms();
    for (int l = 0; l < lanes; l++)
        for (size_t i = 0; i < count; i++) {
            uint8_t lbl[3] = {(uint8_t)(3 * i), (uint8_t)(3 * i + 1), (uint8_t)(3 * i + 2)};
            a[l].append_lbl(lbl, 3, data.data() + ((size_t)l * count + i) * 64, 64);
        }
    double t1 = now_ms();
    Merlin *t[8]; const uint8_t *msg[8];
    for (int l = 0; l < lanes; l++) { t[l] = &b[l]; msg[l] = data.data() + (size_t)l * count * 64; }
    k8::append_lbl3_run_x8(t, lanes, 0, msg, count);
    double t2 = now_ms();
    int bad = 0;
    for (int l = 0; l < lanes; l++) {
        bad |= a[l].pos != b[l].pos || a[l].pos_begin != b[l].pos_begin || a[l].cur_flags != b[l].cur_flags || memcmp(a[l].stw, b[l].stw, 200) != 0;
        const uint8_t *cp = data.data() + data.size() - 64;
        a[l].append("C_prime_eg", cp, 64); b[l].append("C_prime_eg", cp, 64);
        uint8_t ca[64], cb[64]; a[l].challenge_bytes("c", ca, 64); b[l].challenge_bytes("c", cb, 64); bad |= memcmp(ca, cb, 64) != 0;
    }
    if (us_simd) *us_simd = (t2 - t1) * 1e3;
    if (us_scalar) *us_scalar = (t1 - t0) * 1e3;
    return bad;
}
// the same over records `stride` bytes apart (64 <= stride <= 256; bytes 64 .. stride of every record are filler that differs per lane and per
// record): the strided x8 path against Merlin::append_lbl over the first 64 bytes of each record -- nothing of the filler may reach a state
int rofl_dbg_host_merlin8_lbl3_strided_selftest(int lanes, unsigned count, unsigned skew, unsigned stride, double *us_simd, double *us_scalar) {
    if (!k8::available()) return -1;
    if (lanes < 1 || lanes > 8 || skew > 400 || stride < 64 || stride > 256) return ROFL_BAD_PARAM;
    std::vector<uint8_t> data((size_t)8 * count * stride + 64);
    for (size_t i = 0; i < data.size(); i++) data[i] = (uint8_t)((i * 2654435761u) >> 13);
    for (int l = 0; l < 8; l++)
        for (size_t i = 0; i < count; i++)
            for (size_t b = 64; b < stride; b++) data[((size_t)l * count + i) * stride + b] = (uint8_t)(0xA5 ^ (37 * l + 11 * i + b));
    std::vector<uint8_t> pre(skew, 0x5a);
    std::vector<Merlin> a, b;
    for (int l = 0; l < lanes; l++) { a.emplace_back("CompressedRandProof", 19); b.emplace_back("CompressedRandProof", 19); }
    for (int l = 0; l < lanes; l++) {
        a[l].append("dom-sep", (const uint8_t *)"randomness proof v1", 19); b[l].append("dom-sep", (const uint8_t *)"randomness proof v1", 19);
        if (skew) { a[l].append("skew", pre.data(), skew); b[l].append("skew", pre.data(), skew); }
    }
    double t0 = now_ms();
    for (int l = 0; l < lanes; l++)
        for (size_t i = 0; i < count; i++) {
            uint8_t lbl[3] = {(uint8_t)(3 * i), (uint8_t)(3 * i + 1), (uint8_t)(3 * i + 2)}, pair[64];
            memcpy(pair, data.data() + ((size_t)l * count + i) * stride, 64);      // (the packed pair: the scalar side never sees the filler)
            a[l].append_lbl(lbl, 3, pair, 64);
        }
    double t1 = now_ms();
    Merlin *t[8]; const uint8_t *msg[8];
    for (int l = 0; l < lanes; l++) { t[l] = &b[l]; msg[l] = data.data() + (size_t)l * count * stride; }
    k8::append_lbl3_run_x8(t, lanes, 0, msg, count, stride);
    double t2 = now_ms();
    int bad = 0;
    for (int l = 0; l < lanes; l++) {
        bad |= a[l].pos != b[l].pos || a[l].pos_begin != b[l].pos_begin || a[l].cur_flags != b[l].cur_flags || memcmp(a[l].stw, b[l].stw, 200) != 0;
        const uint8_t *cp = data.data() + data.size() - 64;
        a[l].append("C_prime_eg", cp, 64); b[l].append("C_prime_eg", cp, 64);
        uint8_t ca[64], cb[64]; a[l].challenge_bytes("c", ca, 64); b[l].challenge_bytes("c", cb, 64); bad |= memcmp(ca, cb, 64) != 0;
    }
    if (us_simd) *us_simd = (t2 - t1) * 1e3;
    if (us_scalar) *us_scalar = (t1 - t0) * 1e3;
    return bad;
}
// the host hops of the calling thread's last create / verify call: out[0..8] = number of MSM hops, enqueue ms, wait ms, window-combination
// wall ms, sum of each hop's slowest task ms, then the maxima over the hops: enqueue, wait, combination wall, slowest task
int rofl_dbg_last_hops(double out[10]) { if (!out) return fail(ROFL_BAD_PARAM, "bad parameter"); memcpy(out, g_last_hops, sizeof g_last_hops); return ROFL_OK; }
int rofl_dbg_host_fe_mul(const uint8_t a[32], const uint8_t b[32], uint8_t out[32]) { fe_tobytes(out, fe_mul(fe_frombytes(a), fe_frombytes(b))); return 0; }
int rofl_dbg_host_fe_ops(const uint8_t a[32], const uint8_t b[32], uint8_t oa[32], uint8_t os[32], uint8_t oq[32], uint8_t oi[32]) {
    fe x = fe_frombytes(a), y = fe_frombytes(b);
    // exercise the non-canonical range as well: add 2p-ish slack by doubling through fe_add
    fe_tobytes(oa, fe_add(x, y)); fe_tobytes(os, fe_sub(x, y)); fe_tobytes(oq, fe_sq(x)); fe_tobytes(oi, fe_invert(x)); return 0;
}
// both inversion routines (canonical in / out) and their timings in nanoseconds per call
int rofl_dbg_host_sc_invert(const uint8_t a[32], uint8_t out_ref[32], uint8_t out_fast[32], double *ns_ref, double *ns_fast) {
    sc am = h_mont(sc_frombytes(a));
    sc r1 = sc_invert_mont(am), r2 = h51::sc_invert_mont_fast(am);
    sc_tobytes(out_ref, h_canon(r1)); sc_tobytes(out_fast, h_canon(r2));
    if (ns_ref && ns_fast) {
        const int reps = 200; volatile u32 sink = 0;
        double t0 = now_ms(); for (int i = 0; i < reps; i++) { am.v[0] ^= (u32)i; sink += sc_invert_mont(am).v[0]; } double t1 = now_ms();
        for (int i = 0; i < reps; i++) { am.v[0] ^= (u32)i; sink += h51::sc_invert_mont_fast(am).v[0]; } double t2 = now_ms();
        *ns_ref = (t1 - t0) * 1e6 / reps; *ns_fast = (t2 - t1) * 1e6 / reps; (void)sink;
    }
    return 0;
}
int rofl_dbg_host_sc_mul(const uint8_t a[32], const uint8_t b[32], uint8_t out[32]) { sc_tobytes(out, h_mul(sc_frombytes(a), sc_frombytes(b))); return 0; }
int rofl_dbg_host_sc_lazy(const uint8_t *a32, const uint8_t *b32, size_t count, uint8_t out_lazy[32], uint8_t out_ref[32]) {
    if (count > 16) return ROFL_BAD_PARAM;      // sc_redc_wide's bound: sixteen products of operands < l
    u32 acc[17]; for (int i = 0; i < 17; i++) acc[i] = 0;
    sc ref = sc_zero();
    for (size_t k = 0; k < count; k++) {
        const sc a = sc_frombytes(a32 + 32 * k), b = sc_frombytes(b32 + 32 * k);
        sc_mac_wide(acc, a, b);
        ref = sc_add(ref, sc_montmul(a, b));
    }
    sc_tobytes(out_lazy, sc_redc_wide(acc)); sc_tobytes(out_ref, ref);
    return 0;
}
int rofl_dbg_host_sc_wide_mont(const uint8_t in[64], uint8_t out[32]) { sc_tobytes(out, sc_from_mont(sc_from_wide_mont(sc_frombytes(in), sc_frombytes(in + 32)))); return 0; }
int rofl_dbg_host_sc_wide(const uint8_t in[64], uint8_t out[32]) { sc_tobytes(out, sc_from_wide(sc_frombytes(in), sc_frombytes(in + 32))); return 0; }
int rofl_dbg_host_from_uniform(const uint8_t in[64], uint8_t out[32]) { ristretto_encode(out, ristretto_from_uniform(in)); return 0; }
int rofl_dbg_host_scalarmult_base(const uint8_t k[32], int use_bb, uint8_t out[32]) {
    static HostTables ht; static bool init = false; static std::mutex mu;
    std::lock_guard<std::mutex> lk(mu);
    if (!init) {
        static const uint8_t Bc[32] = {0xe2, 0xf2, 0xae, 0x0a, 0x6a, 0xbc, 0x4e, 0x71, 0xa8, 0x84, 0xa9, 0x61, 0xc5, 0x00, 0x51, 0x5f,
                                       0x58, 0xe3, 0x0b, 0x6a, 0xa5, 0x82, 0xdd, 0x8d, 0xb6, 0xa6, 0x59, 0x45, 0xe0, 0x8d, 0x2d, 0x76};
        ristretto_decode(ht.base, Bc); uint8_t h[64]; sha3_512(h, Bc, 32); ht.bblind = ristretto_from_uniform(h);
        build_fixed_table(ht.B, ht.base); build_fixed_table(ht.Bb, ht.bblind); init = true;
    }
    if (use_bb & 2) { to_tab5(ht.B5, ht.B); to_tab5(ht.Bb5, ht.Bb); h51::encode(out, h_fixed_mul((use_bb & 1) ? ht.Bb5 : ht.B5, sc_frombytes(k))); return 0; }
    ristretto_encode(out, h_fixed_mul32((use_bb & 1) ? ht.Bb : ht.B, sc_frombytes(k))); return 0;
}
int rofl_dbg_host_fd_ops(const uint8_t a[32], const uint8_t b[32], uint8_t om[32], uint8_t oq[32], uint8_t oa[32], uint8_t os[32], uint8_t oi[32]) {
    fe fa = fe_frombytes(a), fb = fe_frombytes(b);
    fa.v[7] |= (u32)(a[31] & 0x80) << 24; fb.v[7] |= (u32)(b[31] & 0x80) << 24;   // keep bit 255 to exercise the unpack fold
    fd x = fd_unpack(fa), y = fd_unpack(fb);
    fe_tobytes(om, fd_pack(fd_mul(fd_sub(fd_add(x, x), x), fd_add(y, fd_zero()))));   // (2x - x) * y with a loose first operand
    fe_tobytes(oq, fd_pack(fd_sq(x))); fe_tobytes(oa, fd_pack(fd_add(x, y))); fe_tobytes(os, fd_pack(fd_sub(x, y)));
    fe_tobytes(oi, fd_pack(fd_invert(x)));
    return 0;
}
// double-and-add ladder on the kernel point formulas: exercises gd_double, gd_madd (+/-), gd_add, gd_to_niels
int rofl_dbg_host_fd_scalarmult(const uint8_t k[32], const uint8_t p[32], uint8_t out[32]) {
    ge P; if (!ristretto_decode(P, p)) return ROFL_FORMAT_ERROR;
    nd q = nd_unpack(ge_to_niels(P));
    sc s = sc_frombytes(k);
    if (sc_geq_l(s.v)) s = sc_from_mont(sc_to_mont(s));      // as load_sc_reduced: sc_naf's 256 digits hold a canonical scalar, not 2^256 - 1
    int8_t naf[256]; int top = sc_naf(naf, s);
    gd acc = gd_identity();
    for (int i = top; i >= 0; i--) { acc = gd_double(acc); if (naf[i]) acc = gd_madd(acc, q, naf[i] < 0); }
    gd twice = gd_add(acc, acc);                   // 2kP by the unified addition
    gd back = gd_madd(twice, nd_unpack(gd_to_niels(acc)), true);   // 2kP - kP
    ristretto_encode(out, gd_pack(back));
    return 0;
}
// the register-radix codec on the host (limb bounds asserted): decode, add the identity, re-encode
int rofl_dbg_host_fd_codec(const uint8_t in[32], uint8_t out[32]) {
    gd p; if (!gd_ristretto_decode(p, in)) return ROFL_FORMAT_ERROR;
    gd q = gd_add(gd_double(p), gd_madd(gd_identity(), nd_unpack(gd_to_niels(p)), true));     // 2P - P through the kernel formulas
    gd_ristretto_encode(out, q); return 0;
}
// the op tables of fd_dbg.hpp through the host build (bound assertions on); the two quad ops exist on the device only
int rofl_dbg_host_fd_ops_raw(unsigned op, size_t n, const uint32_t *in, uint32_t *out) {
    if (op >= FD_DBG_THREAD_OPS || !in || !out) return ROFL_BAD_PARAM;
    for (size_t i = 0; i < n; i++) fd_dbg_apply(op, in + i * FD_DBG_IN, out + i * FD_DBG_OUT);
    return 0;
}
int rofl_dbg_host_sc_ops(unsigned op, size_t n, const uint32_t *in, uint32_t *out) {
    if (op >= SC_DBG_OPS || !in || !out) return ROFL_BAD_PARAM;
    for (size_t i = 0; i < n; i++) { const sc r = sc_dbg_apply(op, in + i * SC_DBG_IN); for (int k = 0; k < 8; k++) out[i * SC_DBG_OUT + k] = r.v[k]; }
    return 0;
}
int rofl_dbg_host_decode_encode(const uint8_t in[32], uint8_t out[32]) { ge p; if (!ristretto_decode(p, in)) return ROFL_FORMAT_ERROR; ristretto_encode(out, ge_add(p, ge_identity())); return 0; }
int rofl_dbg_host_merlin(const uint8_t *label, size_t label_len, const uint8_t *msg, size_t msg_len, uint8_t out[64]) {
    Merlin t((const char *)label, label_len); t.append("msg", msg, msg_len); t.challenge_bytes("chal", out, 64); return 0;
}
int rofl_dbg_host_nonce(const uint8_t seed[32], uint64_t idx, uint8_t out[32]) {
    const u64 dom[2] = ROFL_NONCE_DOM;
    u64 sd[4]; memcpy(sd, seed, 32); u64 st[25]; shake256_seeded_block(st, dom, sd, idx >> 1);
    const int h = (int)(idx & 1);
    sc lo, hi; for (int i = 0; i < 4; i++) { lo.v[2 * i] = (u32)st[8 * h + i]; lo.v[2 * i + 1] = (u32)(st[8 * h + i] >> 32); hi.v[2 * i] = (u32)st[8 * h + 4 + i]; hi.v[2 * i + 1] = (u32)(st[8 * h + 4 + i] >> 32); }
    sc_tobytes(out, sc_from_wide(lo, hi)); return 0;
}
int rofl_dbg_host_blind(const uint8_t seed[32], uint64_t idx, uint8_t out[32]) {
    const u64 dom[2] = ROFL_BLIND_DOM;
    u64 sd[4]; memcpy(sd, seed, 32); u64 st[25]; shake256_seeded_block(st, dom, sd, idx >> 1);
    sc_tobytes(out, xof_block_scalar(st, (int)(idx & 1))); return 0;
}

}  // extern "C"
