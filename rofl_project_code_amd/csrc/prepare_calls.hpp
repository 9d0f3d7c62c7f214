// The preparation steps of a client's update -- probabilistic quantization, distributed noise, norm clipping, Hadamard rotation -- each with
// its kernel route, its one-core host twin and its debug entries, on one parameter check, host stream cursor, driver and probe helper.
// Included by rofl_zk.hip at file scope, inside its extern "C" section: the file closes and reopens that and the anonymous namespace.
#pragma once
}  // extern "C"
namespace {
// ---- what the four calls share ----
// The arguments every call has, in the order the failures are reported; own() -> the return code of the call's checks that stand between
// the length and the empty vector.  -> kPrepGo when there is work to do, else what the call returns (ROFL_OK: an empty call).
constexpr int kPrepGo = -1;
template <class Own>
int prep_check(size_t n_vec, const uint8_t *seeds32, bool seeds_required, const float *const *values, float *const *out, size_t d, Own own,
               const char *too_long = "vector length of 2^28 or more") {
    if (n_vec == 0) return ROFL_OK;
    if ((seeds_required && !seeds32) || !values || !out) return fail(ROFL_BAD_PARAM, "bad parameter");
    if (n_vec > kMaxBatchMembers) return fail(ROFL_BAD_PARAM, "more than 65 535 vectors in one call");
    if (d >= ((size_t)1 << 28)) return fail(ROFL_BAD_PARAM, too_long);
    if (int rc = own()) return rc;
    if (d == 0) return ROFL_OK;
    for (size_t v = 0; v < n_vec; v++) if (!values[v] || !out[v]) return fail(ROFL_BAD_PARAM, "bad parameter");
    return kPrepGo;
}
int no_own_check() { return ROFL_OK; }
// A seeded stream read word by word on the host: the seed, its domain label, the XOF block squeezed last and that block's index.  Seed and
// block are the caller's secrets: zeroed when the cursor goes out of scope.  A cursor nobody reads (seed32 null) squeezes nothing.
struct HostStream {
    u64 dom[2], sd[4] = {0, 0, 0, 0}, st[25], cur = ~0ULL;
    HostStream(const u64 (&label)[2], const uint8_t *seed32) : dom{label[0], label[1]} { if (seed32) memcpy(sd, seed32, 32); }
    u32 word(u64 w) { if ((w >> 5) != cur) { cur = w >> 5; shake256_seeded_block(st, dom, sd, cur); } return quant_block_word(st, (u32)(w & 31)); }
    ~HostStream() { volatile u64 *p = sd; for (int i = 0; i < 4; i++) p[i] = 0; p = st; for (int i = 0; i < 25; i++) p[i] = 0; }
};
// One call, its parameters checked.  route: -1 = by the pointers and the size, 0 = the host twin, 1 = the kernels (rofl_dbg_*_route).
// host_below: under its measured crossover, so on route -1 it runs on the host if every pointer is host memory.  seeds32: 32 bytes per
// vector, or null (clipping without seeds): zeros in the descriptors, nothing to wipe.  d_out >= d: the elements of an output (the rotation's
// whole blocks).  side_out (host memory or null), side_bytes: what the kernels leave besides the vectors (clipping's scales), downloaded first.
struct PrepCall {
    int route; bool host_below; size_t n_vec; const uint8_t *seeds32; const float *const *values; size_t d, d_out; float *const *out;
    void *side_out = nullptr; size_t side_bytes = 0;
};
static_assert(offsetof(ClipVec, in) == offsetof(QuantVec, in) && offsetof(ClipVec, out) == offsetof(QuantVec, out) && offsetof(ClipVec, seed) == offsetof(QuantVec, seed) &&
              sizeof(ClipVec::in) == sizeof(QuantVec::in) && sizeof(ClipVec::out) == sizeof(QuantVec::out) && sizeof(ClipVec::seed) == sizeof(QuantVec::seed), "a ClipVec begins as a QuantVec");
// The way of a checked call.  Vec: QuantVec or ClipVec, one descriptor per vector.  host(v) runs the rule of vector v on the host;
// fill(v, desc) writes what a descriptor holds behind in / out / seed; launch(C, vecs) enqueues the kernels over the device copy of the
// descriptors on C.stream and returns where they leave the side output (device memory; null: none).  A device input is read and a device
// output written in place; a vector with a host pointer gets ONE slot of the lane's workspace (C.vals): a host input is uploaded into
// it, the kernels write a host output into it (in place when both are host memory).  The descriptors are staged in C.h_misc and
// C.tmp_in; they hold the seeds, so both copies are zeroed when the call returns or unwinds (BlindWipe, before the lane is released).
template <class Vec, class Host, class Fill, class Launch>
int prep_run(const PrepCall &p, Host host, Fill fill, Launch launch) {
    return guarded([&]() -> int {
        const size_t n_vec = p.n_vec, d = p.d, d_out = p.d_out;
        std::vector<char> dev_in(n_vec, 0), dev_out(n_vec, 0); bool all_host = true;
        for (size_t v = 0; v < n_vec; v++) { dev_in[v] = is_device_ptr(p.values[v]); dev_out[v] = is_device_ptr(p.out[v]); all_host &= !dev_in[v] && !dev_out[v]; }
        if (p.route == 0 && !all_host) return fail(ROFL_BAD_PARAM, "the host route takes host pointers only");
        if (p.route == 0 || (p.route == -1 && all_host && p.host_below)) {
            for (size_t v = 0; v < n_vec; v++) host(v);
            return ROFL_OK;
        }
        LaneLock lane_lock = acquire_lane(); Ctx &C = *lane_lock.c;
        C.init();
        size_t n_slot = 0;
        for (size_t v = 0; v < n_vec; v++) if (!dev_in[v] || !dev_out[v]) n_slot++;
        float *ws = n_slot ? C.vals.as<float>(n_slot * d_out) : nullptr;
        const size_t bytes = n_vec * sizeof(Vec);
        Vec *h = C.h_misc.as<Vec>(n_vec), *dv = C.tmp_in.as<Vec>(n_vec);
        BlindWipe wipe; wipe.h = reinterpret_cast<uint8_t *>(h); wipe.dv = reinterpret_cast<uint8_t *>(dv); wipe.n = p.seeds32 ? bytes : 0; wipe.s = C.stream;
        size_t slot = 0;
        for (size_t v = 0; v < n_vec; v++) {
            float *s = (!dev_in[v] || !dev_out[v]) ? ws + (slot++) * d_out : nullptr;
            h[v].in = dev_in[v] ? p.values[v] : s; h[v].out = dev_out[v] ? p.out[v] : s;
            if (p.seeds32) memcpy(h[v].seed, p.seeds32 + 32 * v, 32); else memset(h[v].seed, 0, 32);
            fill(v, h[v]);
            if (!dev_in[v]) {
                C.up(s, p.values[v], 4 * d, C.stream);
                if (d_out > d) HIPCHK(hipMemsetAsync(s + d, 0, 4 * (d_out - d), C.stream));
            }
        }
        HIPCHK(hipMemcpyAsync(dv, h, bytes, hipMemcpyHostToDevice, C.stream));
        const void *side = launch(C, (const Vec *)dv);
        if (p.side_out) C.down(p.side_out, side, p.side_bytes, C.stream);
        for (size_t v = 0; v < n_vec; v++) if (!dev_out[v]) C.down(p.out[v], h[v].out, 4 * d_out, C.stream);
        C.sync();
        return ROFL_OK;
    });
}
void no_fill(size_t, QuantVec &) {}
// Site 1 of the rule probes (rofl_dbg_quant_round, rofl_dbg_noise_apply, rofl_dbg_clip_l2_round): n cases, one thread each.  Array a (A per
// case) and, where there is one, array b (B per case) are uploaded, launch(C, n, a, b, out) enqueues the probe kernel, n floats come back.
template <class A, class B, class Launch>
int probe_run(size_t n, const A *a, const B *b, float *out, Launch launch) {
    return guarded([&]() -> int {
        LaneLock lane_lock = acquire_lane(); Ctx &C = *lane_lock.c;
        C.init();
        A *da = C.vals.as<A>(n); float *dout = C.tmp_out.as<float>(n);
        B *db = b ? C.tmp_in.as<B>(n) : nullptr;
        C.up(da, a, sizeof(A) * n, C.stream); if (b) C.up(db, b, sizeof(B) * n, C.stream);
        launch(C, (u32)n, (const A *)da, (const B *)db, dout);
        C.down(out, dout, 4 * n, C.stream);
        C.sync();
        return ROFL_OK;
    });
}

// ---- probabilistic quantization (rofl_quantize_prob: the definition is in the header, the rule and the kernel in kernels.hpp) ----
// Below this many elements in all, a call whose pointers are all host memory runs the rule on the host: one Keccak-f per 32 elements on one
// core against the fixed cost of two staged copies, a launch and a synchronisation.  The measured crossover (profiles/prob_quant.json,
// DESIGN section 7); a constant, not a knob: both routes give the same bytes.
constexpr size_t kQuantProbHostBelow = 8192;
void quant_prob_host(const uint8_t *seed32, const float *in, u64 first, size_t d, float mn, float mx, unsigned fp_frac, float *out) {
    HostStream xs(ROFL_QUANT_DOM, seed32);
    for (size_t k = 0; k < d; k++) out[k] = quant_prob_round(in[k], xs.word(first + k), mn, mx, fp_frac);
}
// route: as PrepCall (rofl_dbg_quantize_prob_route)
int quantize_prob_impl(int route, size_t n_vec, const uint8_t *seeds32, const float *const *values, size_t first, size_t d,
                       size_t prove_range, unsigned fp_bits, unsigned fp_frac, float *const *out) {
    if (!valid_fp(fp_bits, fp_frac) || prove_range == 0) return fail(ROFL_BAD_PARAM, "bad parameter");
    if (int rc = prep_check(n_vec, seeds32, true, values, out, d, [&]() -> int {
        return first > ((size_t)1 << 63) - d ? fail(ROFL_BAD_PARAM, "first + d exceeds 2^63") : ROFL_OK; }); rc != kPrepGo) return rc;
    float mn, mx; clip_bounds(prove_range, fp_bits, fp_frac, &mn, &mx);
    return prep_run<QuantVec>(PrepCall{route, n_vec * d < kQuantProbHostBelow, n_vec, seeds32, values, d, d, out},
        [&](size_t v) { quant_prob_host(seeds32 + 32 * v, values[v], first, d, mn, mx, fp_frac, out[v]); }, no_fill,
        [&](Ctx &C, const QuantVec *vecs) -> const void * {
            const size_t nblk = ((first + d + 31) >> 5) - (first >> 5);      // XOF blocks that hold an element of [first, first + d): <= 2^23 + 1
            ROFL_LAUNCH(k_quantize_prob, dim3((unsigned)((nblk + QP_TPB - 1) / QP_TPB), (unsigned)n_vec), dim3(QP_TPB), 0, C.stream,
                        vecs, (u64)first, (u32)d, mn, mx, (u32)fp_frac);
            return nullptr;
        });
}

// ---- distributed noise (rofl_noise_binomial: the definition is in the header, the value rule and the kernel in kernels.hpp) ----
// Below this many Keccak permutations in all (n_vec d W / 32), a call whose pointers are all host memory runs on the host: one core's
// permutations against the fixed cost of two staged copies, a launch and a synchronisation.  The measured crossover
// (profiles/binomial_noise.json); a constant, not a knob: both routes give the same bytes.
constexpr u64 kNoiseHostBelowPerms = 256;
// elements of a workgroup's group in k_noise_binomial: the words of a group, plus the 31 its first block can hold of a neighbour, fill
// `passes` x 64 blocks -- one pass for W <= 32, W / 32 passes up to 32 (a wide element then wastes at most a few per cent of the lanes of
// its group's last pass), and a single element whatever its width beyond that
u32 noise_epw(u32 W) {
    const u32 passes = std::min(std::max(W / 32, 1u), 32u);
    return std::min(std::max((2048 * passes - 31) / W, 1u), (u32)NB_EPW_MAX);
}
// noise integer of element index e: popcount of stream words e W .. e W + W - 1, minus k
int noise_host_element(HostStream &xs, u64 e, u32 W) {
    u32 cnt = 0;
    for (u64 w = e * W; w < e * W + W; w++) cnt += (u32)__builtin_popcount(xs.word(w));
    return (int)cnt - (int)(16 * W);
}
void noise_host(const uint8_t *seed32, const float *in, u64 first, size_t d, u32 W, float mn, float mx, unsigned fp_frac, float *out) {
    HostStream xs(ROFL_NOISE_DOM, seed32);
    for (size_t i = 0; i < d; i++) out[i] = noise_apply(in[i], noise_host_element(xs, first + i, W), mn, mx, fp_frac);
}
bool noise_k_ok(uint32_t k) { return k >= 16 && k <= (1u << 20) && k % 16 == 0; }
// route: as PrepCall (rofl_dbg_noise_binomial_route)
int noise_binomial_impl(int route, size_t n_vec, const uint8_t *seeds32, const float *const *values, size_t first, size_t d, uint32_t k,
                        size_t prove_range, unsigned fp_bits, unsigned fp_frac, float *const *out) {
    if (!valid_fp(fp_bits, fp_frac) || prove_range == 0) return fail(ROFL_BAD_PARAM, "bad parameter");
    if (!noise_k_ok(k)) return fail(ROFL_BAD_PARAM, "k is a multiple of 16 from 16 to 2^20");
    const u32 W = k / 16;
    if (int rc = prep_check(n_vec, seeds32, true, values, out, d, [&]() -> int {
        return first > ((size_t)1 << 63) - d || first + d > ((u64)1 << 63) / W ? fail(ROFL_BAD_PARAM, "(first + d) k / 16 exceeds 2^63") : ROFL_OK; }); rc != kPrepGo) return rc;
    float mn, mx; clip_bounds(prove_range, fp_bits, fp_frac, &mn, &mx);
    return prep_run<QuantVec>(PrepCall{route, (u64)n_vec * d * W < 32 * kNoiseHostBelowPerms, n_vec, seeds32, values, d, d, out},
        [&](size_t v) { noise_host(seeds32 + 32 * v, values[v], first, d, W, mn, mx, fp_frac, out[v]); }, no_fill,
        [&](Ctx &C, const QuantVec *vecs) -> const void * {
            const u32 epw = noise_epw(W), n_grp = (u32)((d + epw - 1) / epw);
            ROFL_LAUNCH(k_noise_binomial, dim3(std::min(n_grp, 1u << 22), (unsigned)n_vec), dim3(NB_TPB), 0, C.stream,
                        vecs, (u64)first, (u32)d, W, epw, n_grp, mn, mx, (u32)fp_frac);
            return nullptr;
        });
}

// ---- discrete Gaussian noise (rofl_noise_dgauss: the definition is in the header, the sampler and the kernel in kernels.hpp) ----
// Below this many elements in all, a call whose pointers are all host memory runs on the host: about 1.2 permutations and one run of the
// sampler per element on one core against the fixed cost of two staged copies, a launch and a synchronisation.  The measured crossover
// (profiles/dgauss_noise.json); a constant, not a knob: both routes give the same bytes.
constexpr size_t kDgaussHostBelow = 768;
// The grid of k_noise_dgauss for one vector of d elements.  No more waves in all than the chip holds at once at two per SIMD (256 CUs x
// 8): beyond that a lane owns more elements instead -- the blocks an element needs vary, a wave waits for its slowest lane, and the sum
// over a lane's elements varies less.  Below that a small call is a matter of latency, a lane's elements run one after the other, and
// waves are free: two elements per lane, so that a lane's second element fills some of the trips its wave waits for the slowest first.
constexpr u32 kDgaussLaneElems = 2, kDgaussWaves = 2048;
u32 dgauss_grid(size_t n_vec, size_t d) {
    const u32 want = (u32)((d + (size_t)DG_TPB * kDgaussLaneElems - 1) / ((size_t)DG_TPB * kDgaussLaneElems));
    return std::max(1u, std::min(want, kDgaussWaves / (u32)std::min<size_t>(n_vec, kDgaussWaves)));
}
// The per-element streams of one seed, read on the host: the on-demand source of kernels.hpp with its seed words and its block of 32 stream
// words.  Both are the caller's secrets, as the seed and block of a HostStream: zeroed when the owner goes out of scope (the state of
// each squeeze zeroes itself, dg_squeeze).
struct DgaussHostStream {
    DgSeeded src; u32 blk[32];
    explicit DgaussHostStream(const uint8_t *seed32) : src{0, 0, 0, 0, 0, blk, ~0u, 0} { memcpy(&src.s0, seed32, 8); memcpy(&src.s1, seed32 + 8, 8); memcpy(&src.s2_, seed32 + 16, 8); memcpy(&src.s3, seed32 + 24, 8); }
    DgaussHostStream(const DgaussHostStream &) = delete;
    // noise integer of element index e, and the words it consumed (not finished: dry at word 8 192, noise 0)
    int element(u64 e, u32 s2, u32 *used) {
        src.e = e; src.cur = ~0u; src.pos = 0;
        const DgaussOut r = dgauss_run(src, s2);
        if (used) *used = r.used;
        return r.noise;
    }
    ~DgaussHostStream() {
        volatile u64 *p = &src.s0; p[0] = 0; p = &src.s1; p[0] = 0; p = &src.s2_; p[0] = 0; p = &src.s3; p[0] = 0;
        volatile u32 *q = blk; for (int i = 0; i < 32; i++) q[i] = 0;
    }
};
void noise_dgauss_host(const uint8_t *seed32, const float *in, u64 first, size_t d, u32 s2, float mn, float mx, unsigned fp_frac, float *out) {
    DgaussHostStream xs(seed32);
    for (size_t i = 0; i < d; i++) out[i] = noise_apply(in[i], xs.element(first + i, s2, nullptr), mn, mx, fp_frac);
}
bool dgauss_sigma2_ok(uint32_t s2) { return s2 >= 1 && s2 <= (1u << 24); }
// route: as PrepCall (rofl_dbg_noise_dgauss_route)
int noise_dgauss_impl(int route, size_t n_vec, const uint8_t *seeds32, const float *const *values, size_t first, size_t d, uint32_t sigma2,
                      size_t prove_range, unsigned fp_bits, unsigned fp_frac, float *const *out) {
    if (!valid_fp(fp_bits, fp_frac) || prove_range == 0) return fail(ROFL_BAD_PARAM, "bad parameter");
    if (!dgauss_sigma2_ok(sigma2)) return fail(ROFL_BAD_PARAM, "sigma2 is an integer from 1 to 2^24");
    if (int rc = prep_check(n_vec, seeds32, true, values, out, d, [&]() -> int {
        return first > ((size_t)1 << 55) || first + d > ((size_t)1 << 55) ? fail(ROFL_BAD_PARAM, "first + d exceeds 2^55") : ROFL_OK; }); rc != kPrepGo) return rc;
    float mn, mx; clip_bounds(prove_range, fp_bits, fp_frac, &mn, &mx);
    return prep_run<QuantVec>(PrepCall{route, n_vec * d < kDgaussHostBelow, n_vec, seeds32, values, d, d, out},
        [&](size_t v) { noise_dgauss_host(seeds32 + 32 * v, values[v], first, d, sigma2, mn, mx, fp_frac, out[v]); }, no_fill,
        [&](Ctx &C, const QuantVec *vecs) -> const void * {
            ROFL_LAUNCH(k_noise_dgauss, dim3(dgauss_grid(n_vec, d), (unsigned)n_vec), dim3(DG_TPB), 0, C.stream,
                        vecs, (u64)first, (u32)d, (u32)sigma2, mn, mx, (u32)fp_frac);
            return nullptr;
        });
}

// ---- norm clipping (rofl_clip_l2: the definition is in the header, the rule, the search and the kernels in kernels.hpp) ----
// Below this many elements in all, a call whose pointers are all host memory runs the rule on the host: two passes of one core over the
// values (and one Keccak-f per 32 elements with seeds) against the fixed cost of two staged copies, two launches and a synchronisation.
// The measured crossovers, the first size of the sweep at which the kernels win (profiles/l2_clip.json); constants,
// not knobs: both routes give the same bytes.
constexpr size_t kClipL2HostBelow = 16384, kClipL2HostBelowSeeded = 8192;
constexpr u32 kClipL2Blocks = 8;      // k_clip_l2_sumsq, per vector: 2 048 threads stride over d, as the sums of the L2 proof (kL2SumBlocks)
u64 isqrt_u64(u64 x) {
    u64 r = (u64)std::sqrt((long double)x);
    while ((unsigned __int128)r * r > x) r--;
    while ((unsigned __int128)(r + 1) * (r + 1) <= x) r++;
    return r;
}
// Te of a seeded vector: (isqrt(T) - ceil(sqrt(d)))^2; false when the difference is negative
bool clip_l2_seeded_budget(u64 T, size_t d, u64 *te) {
    const u64 rt = isqrt_u64(T), rd = d ? isqrt_u64(d - 1) + 1 : 0;
    if (rt < rd) return false;
    *te = (rt - rd) * (rt - rd); return true;
}
void clip_l2_host(const uint8_t *seed32 /* or null */, const float *in, size_t d, u64 T, u64 te, float mn, float mx, unsigned fp_bits, unsigned fp_frac,
                  float *out, uint64_t *scale) {
    u64 S[3] = {0, 0, 0};
    for (size_t i = 0; i < d; i++) {
        float c; const u64 q = clip_l2_steps(in[i], mn, mx, fp_bits, fp_frac, &c);
        u64 lo, hi; mul64_wide(q, q, &lo, &hi); u192_add(S, lo, hi, 0);
    }
    if (clip_l2_fits(S, T)) {
        for (size_t i = 0; i < d; i++) out[i] = noise_apply(in[i], 0, mn, mx, fp_frac);
        if (scale) *scale = 1ULL << 32;
        return;
    }
    const u32 m = clip_l2_scale(S, te);
    HostStream xs(ROFL_CLIP_DOM, seed32);      // (read with a seed only)
    for (size_t i = 0; i < d; i++) {
        float c; const u64 q = clip_l2_steps(in[i], mn, mx, fp_bits, fp_frac, &c);
        out[i] = clip_l2_round(q, m, seed32 != nullptr, seed32 ? xs.word(i) : 0u, c, fp_frac);
    }
    if (scale) *scale = m;
}
// route: as PrepCall (rofl_dbg_clip_l2_route)
int clip_l2_impl(int route, size_t n_vec, const uint8_t *seeds32, const float *const *values, size_t d, const uint64_t *max_sq, size_t prove_range,
                 unsigned fp_bits, unsigned fp_frac, float *const *out, uint64_t *scale_out) {
    if (!valid_fp(fp_bits, fp_frac) || prove_range == 0) return fail(ROFL_BAD_PARAM, "bad parameter");
    if (n_vec && !max_sq) return fail(ROFL_BAD_PARAM, "bad parameter");
    if (int rc = prep_check(n_vec, seeds32, false, values, out, d, no_own_check); rc != kPrepGo) return rc;
    std::vector<u64> te(max_sq, max_sq + n_vec);
    if (seeds32) for (size_t v = 0; v < n_vec; v++)
        if (!clip_l2_seeded_budget(max_sq[v], d, &te[v])) return fail(ROFL_BAD_PARAM, "max_sq leaves no room for the rounding of d elements: isqrt(max_sq) < ceil(sqrt(d))");
    float mn, mx; clip_bounds(prove_range, fp_bits, fp_frac, &mn, &mx);
    return prep_run<ClipVec>(PrepCall{route, n_vec * d < (seeds32 ? kClipL2HostBelowSeeded : kClipL2HostBelow), n_vec, seeds32, values, d, d, out, scale_out, 8 * n_vec},
        [&](size_t v) { clip_l2_host(seeds32 ? seeds32 + 32 * v : nullptr, values[v], d, max_sq[v], te[v], mn, mx, fp_bits, fp_frac, out[v], scale_out ? scale_out + v : nullptr); },
        [&](size_t v, ClipVec &cv) { cv.max_sq = max_sq[v]; cv.te = te[v]; },
        [&](Ctx &C, const ClipVec *vecs) -> const void * {
            const u32 n_part = (u32)std::min<size_t>(kClipL2Blocks, (d + CL_TPB - 1) / CL_TPB);
            u64 *part = C.tmp_out.as<u64>(n_vec * (3 * (size_t)n_part + 1)), *dscale = part + 3 * (size_t)n_part * n_vec;
            ROFL_LAUNCH(k_clip_l2_sumsq, dim3(n_part, (unsigned)n_vec), dim3(CL_TPB), 0, C.stream, vecs, (u32)d, mn, mx, (u32)fp_bits, (u32)fp_frac, part);
            const dim3 grid((unsigned)((d + 32 * QP_TPB - 1) / (32 * QP_TPB)), (unsigned)n_vec);
            if (seeds32) ROFL_LAUNCH(k_clip_l2_apply_seeded, grid, dim3(QP_TPB), 0, C.stream, vecs, (u32)d, n_part, (const u64 *)part, mn, mx, (u32)fp_bits, (u32)fp_frac, dscale);
            else ROFL_LAUNCH(k_clip_l2_apply, grid, dim3(QP_TPB), 0, C.stream, vecs, (u32)d, n_part, (const u64 *)part, mn, mx, (u32)fp_bits, (u32)fp_frac, dscale);
            return dscale;      // a scale per vector: the call's side output
        });
}

// ---- Hadamard rotation (rofl_rotate: the definition is in the header, the element rules and the kernels in kernels.hpp) ----
// Below this many padded elements in all, a call whose pointers are all host memory runs the network on the host: k passes of one core
// over a block against the fixed cost of two staged copies, one or two launches and a synchronisation.  The measured crossover
// (profiles/rotate.json); a constant, not a knob: both routes give the same bytes.
constexpr size_t kRotateHostBelow = 32768;
// one vector on the host: block by block through `buf` (B floats), so that out may be in.  (Its stream is not a HostStream: blocks of
// 1 024 sign bits under a 17-byte label, and a seed that is public.)  Out of line, its butterfly loop aligned: the loop is bound by
// instruction fetch, and where it happens to stand is worth 6 -- 20 % of the call (profiles/prepare_calls/rotate_host_variants.txt).
__attribute__((noinline)) void rotate_host(const uint8_t *seed32, const float *in, size_t d, size_t dp, unsigned k, bool inverse, float *out, std::vector<float> &buf) {
    const size_t B = (size_t)1 << k;
    buf.resize(B);
    float *z = buf.data();
    const float c = rot_scale(k);
    u64 sd[4], st[25], cur = ~0ULL; memcpy(sd, seed32, 32);
    auto signs = [&](size_t e0) {      // step 1 over the block that starts at element e0
        for (size_t i = 0; i < B; i++) {
            const u64 e = e0 + i;
            if ((e >> 10) != cur) { cur = e >> 10; shake256_rotate_block(st, sd, cur); }
            z[i] = rot_flip(z[i], rot_sign_bit(st, (u32)e));
        }
    };
    for (size_t e0 = 0; e0 < dp; e0 += B) {
        for (size_t i = 0; i < B; i++) z[i] = rot_clamp(e0 + i < d ? in[e0 + i] : 0.0f);
        if (!inverse) signs(e0);
        for (size_t h = 1; h < B; h <<= 1)
            for (size_t j = 0; j < B; j += 2 * h)
                [[clang::code_align(32)]] for (size_t i = j; i < j + h; i++) { const float a = z[i], b = z[i + h]; z[i] = a + b; z[i + h] = a - b; }
        for (size_t i = 0; i < B; i++) z[i] = z[i] * c;
        if (inverse) signs(e0);
        memcpy(out + e0, z, 4 * B);
    }
}
// route: as PrepCall (rofl_dbg_rotate_route)
int rotate_impl(int route, size_t n_vec, const uint8_t *seeds32, const float *const *values, size_t d, unsigned k, int inverse, float *const *out) {
    if (k > ROT_MAX_LOG2 || (inverse != 0 && inverse != 1)) return fail(ROFL_BAD_PARAM, "bad parameter");
    const size_t B = (size_t)1 << k, dp = (d + B - 1) / B * B;      // (d < 2^28 where `own` reads dp)
    if (int rc = prep_check(n_vec, seeds32, true, values, out, d, [&]() -> int {
        if (dp >= ((size_t)1 << 28)) return fail(ROFL_BAD_PARAM, "padded vector length of 2^28 or more");
        if (inverse && dp != d) return fail(ROFL_BAD_PARAM, "the inverse takes whole blocks: d is not a multiple of 2^block_log2");
        return ROFL_OK; }, "padded vector length of 2^28 or more"); rc != kPrepGo) return rc;
    std::vector<float> buf;
    return prep_run<QuantVec>(PrepCall{route, n_vec * dp < kRotateHostBelow, n_vec, seeds32, values, d, dp, out},
        [&](size_t v) { rotate_host(seeds32 + 32 * v, values[v], d, dp, k, inverse != 0, out[v], buf); }, no_fill,
        [&](Ctx &C, const QuantVec *vecs) -> const void * {
            const bool cols = k > ROT_T_LOG2;
            // (the inverse of a block longer than a tile: the tile kernel leaves the sign words where the column kernel finds them)
            u32 *signs = (cols && inverse) ? C.tmp_out.as<u32>(n_vec * (dp >> 5)) : nullptr;
            ROFL_LAUNCH(k_rotate_tile, dim3((unsigned)((dp + ROT_T - 1) >> ROT_T_LOG2), (unsigned)n_vec), dim3(ROT_TPB), 0, C.stream,
                        vecs, (u32)d, (u32)dp, (u32)k, (u32)inverse, signs);
            if (cols) {
                const unsigned rl = k - ROT_T_LOG2, wl = rl <= 8 ? ROT_T_LOG2 - rl : 5;      // as k_rotate_cols: R = 2^rl rows, strips of W = 2^wl columns
                const size_t lds = rl > 3 ? ((size_t)4 << (rl + wl)) : 0;                    // (at most 64 KB)
                ROFL_LAUNCH(k_rotate_cols, dim3((unsigned)((dp >> k) << (ROT_T_LOG2 - wl)), (unsigned)n_vec), dim3(ROT_COL_TPB), lds, C.stream,
                            vecs, (u32)dp, (u32)k, (u32)inverse, (const u32 *)signs);
            }
            return nullptr;
        });
}
}  // namespace
extern "C" {
int rofl_quantize_prob(size_t n_vec, const uint8_t *seeds32, const float *const *values, size_t first, size_t d, size_t prove_range,
                       unsigned fp_bits, unsigned fp_frac, float *const *out) {
    return quantize_prob_impl(-1, n_vec, seeds32, values, first, d, prove_range, fp_bits, fp_frac, out);
}
int rofl_noise_binomial(size_t n_vec, const uint8_t *seeds32, const float *const *values, size_t first, size_t d, uint32_t k, size_t prove_range,
                        unsigned fp_bits, unsigned fp_frac, float *const *out) {
    return noise_binomial_impl(-1, n_vec, seeds32, values, first, d, k, prove_range, fp_bits, fp_frac, out);
}
int rofl_noise_dgauss(size_t n_vec, const uint8_t *seeds32, const float *const *values, size_t first, size_t d, uint32_t sigma2, size_t prove_range,
                      unsigned fp_bits, unsigned fp_frac, float *const *out) {
    return noise_dgauss_impl(-1, n_vec, seeds32, values, first, d, sigma2, prove_range, fp_bits, fp_frac, out);
}
int rofl_clip_l2(size_t n_vec, const uint8_t *seeds32, const float *const *values, size_t d, const uint64_t *max_sq, size_t prove_range, unsigned fp_bits,
                 unsigned fp_frac, float *const *out, uint64_t *scale_out) {
    return clip_l2_impl(-1, n_vec, seeds32, values, d, max_sq, prove_range, fp_bits, fp_frac, out, scale_out);
}
int rofl_rotate(size_t n_vec, const uint8_t *seeds32, const float *const *values, size_t d, unsigned block_log2, int inverse, float *const *out) {
    return rotate_impl(-1, n_vec, seeds32, values, d, block_log2, inverse, out);
}
// ---- the debug entries of the calls above (include/rofl_zk_debug.h) ----
int rofl_dbg_host_quant(const uint8_t seed[32], uint64_t idx, uint32_t *word_out) {
    if (!seed || !word_out) return ROFL_BAD_PARAM;
    *word_out = HostStream(ROFL_QUANT_DOM, seed).word(idx); return 0;
}
int rofl_dbg_quant_round(unsigned site, size_t n, const float *values, const uint32_t *words, size_t prove_range, unsigned fp_bits, unsigned fp_frac, float *out) {
    if (site > 1 || !valid_fp(fp_bits, fp_frac) || prove_range == 0 || n > (1u << 20) || (n && (!values || !words || !out))) return fail(ROFL_BAD_PARAM, "bad parameter");
    if (n == 0) return ROFL_OK;
    float mn, mx; clip_bounds(prove_range, fp_bits, fp_frac, &mn, &mx);
    if (site == 0) { for (size_t i = 0; i < n; i++) out[i] = quant_prob_round(values[i], words[i], mn, mx, fp_frac); return ROFL_OK; }
    return probe_run(n, values, words, out, [&](Ctx &C, u32 cnt, const float *dv, const u32 *dw, float *dout) {
        ROFL_LAUNCH(k_dbg_quant_round, grid1(n), dim3(TPB), 0, C.stream, cnt, dv, dw, mn, mx, (u32)fp_frac, dout); });
}
int rofl_dbg_quantize_prob_route(unsigned route, size_t n_vec, const uint8_t *seeds32, const float *const *values, size_t first, size_t d,
                                 size_t prove_range, unsigned fp_bits, unsigned fp_frac, float *const *out) {
    if (route > 1) return fail(ROFL_BAD_PARAM, "bad parameter");
    return quantize_prob_impl((int)route, n_vec, seeds32, values, first, d, prove_range, fp_bits, fp_frac, out);
}
int rofl_dbg_host_noise(const uint8_t seed[32], uint64_t e, uint32_t k, int32_t *n_out) {
    if (!seed || !n_out || !noise_k_ok(k) || e >= ((u64)1 << 63) / (k / 16)) return ROFL_BAD_PARAM;
    HostStream xs(ROFL_NOISE_DOM, seed);
    *n_out = noise_host_element(xs, e, k / 16); return 0;
}
int rofl_dbg_noise_apply(unsigned site, size_t n, const float *values, const int32_t *noise_i32, size_t prove_range, unsigned fp_bits, unsigned fp_frac, float *out) {
    if (site > 1 || !valid_fp(fp_bits, fp_frac) || prove_range == 0 || n > (1u << 20) || (n && (!values || !noise_i32 || !out))) return fail(ROFL_BAD_PARAM, "bad parameter");
    if (n == 0) return ROFL_OK;
    float mn, mx; clip_bounds(prove_range, fp_bits, fp_frac, &mn, &mx);
    if (site == 0) { for (size_t i = 0; i < n; i++) out[i] = noise_apply(values[i], noise_i32[i], mn, mx, fp_frac); return ROFL_OK; }
    return probe_run(n, values, noise_i32, out, [&](Ctx &C, u32 cnt, const float *dv, const int *dn, float *dout) {
        ROFL_LAUNCH(k_dbg_noise_apply, grid1(n), dim3(TPB), 0, C.stream, cnt, dv, dn, mn, mx, (u32)fp_frac, dout); });
}
int rofl_dbg_noise_binomial_route(unsigned route, size_t n_vec, const uint8_t *seeds32, const float *const *values, size_t first, size_t d,
                                  uint32_t k, size_t prove_range, unsigned fp_bits, unsigned fp_frac, float *const *out) {
    if (route > 1) return fail(ROFL_BAD_PARAM, "bad parameter");
    return noise_binomial_impl((int)route, n_vec, seeds32, values, first, d, k, prove_range, fp_bits, fp_frac, out);
}
int rofl_dbg_host_dgauss(const uint8_t seed[32], uint64_t e, uint32_t sigma2, int32_t *noise_out, uint32_t *words_used_out) {
    if (!seed || !noise_out || !dgauss_sigma2_ok(sigma2) || e >= ((u64)1 << 55)) return ROFL_BAD_PARAM;
    u32 used;
    *noise_out = DgaussHostStream(seed).element(e, sigma2, &used);
    if (words_used_out) *words_used_out = used;
    return 0;
}
int rofl_dbg_dgauss_words(unsigned site, size_t n_cases, const uint32_t *words, size_t stride, const uint32_t *lens, const uint32_t *sigma2s,
                          int32_t *noise_out, uint32_t *used_out, uint32_t *finished_out) {
    if (site > 1 || n_cases > (1u << 20) || stride > DG_STREAM_WORDS || n_cases * stride > ((size_t)1 << 26) ||
        (n_cases && (!lens || !sigma2s || !noise_out || !used_out || !finished_out || (stride && !words)))) return fail(ROFL_BAD_PARAM, "bad parameter");
    for (size_t i = 0; i < n_cases; i++) if (lens[i] > stride || !dgauss_sigma2_ok(sigma2s[i])) return fail(ROFL_BAD_PARAM, "bad parameter");
    if (n_cases == 0) return ROFL_OK;
    if (site == 0) {
        for (size_t i = 0; i < n_cases; i++) {
            const DgaussOut r = dgauss_sample(words + i * stride, lens[i], sigma2s[i]);
            noise_out[i] = r.noise; used_out[i] = r.used; finished_out[i] = r.finished;
        }
        return ROFL_OK;
    }
    return guarded([&]() -> int {      // (as probe_run, with three arrays in and three out)
        LaneLock lane_lock = acquire_lane(); Ctx &C = *lane_lock.c;
        C.init();
        const size_t n = n_cases;
        u32 *dw = C.vals.as<u32>(std::max<size_t>(n * stride, 1)), *dl = C.tmp_in.as<u32>(2 * n); int *dres = C.tmp_out.as<int>(3 * n);
        if (stride) C.up(dw, words, 4 * n * stride, C.stream);
        C.up(dl, lens, 4 * n, C.stream); C.up(dl + n, sigma2s, 4 * n, C.stream);
        ROFL_LAUNCH(k_dbg_dgauss_words, grid1(n), dim3(TPB), 0, C.stream, (u32)n, (const u32 *)dw, (u32)stride, (const u32 *)dl, (const u32 *)(dl + n), dres);
        C.down(noise_out, dres, 4 * n, C.stream); C.down(used_out, dres + n, 4 * n, C.stream); C.down(finished_out, dres + 2 * n, 4 * n, C.stream);
        C.sync();
        return ROFL_OK;
    });
}
int rofl_dbg_noise_dgauss_route(unsigned route, size_t n_vec, const uint8_t *seeds32, const float *const *values, size_t first, size_t d,
                                uint32_t sigma2, size_t prove_range, unsigned fp_bits, unsigned fp_frac, float *const *out) {
    if (route > 1) return fail(ROFL_BAD_PARAM, "bad parameter");
    return noise_dgauss_impl((int)route, n_vec, seeds32, values, first, d, sigma2, prove_range, fp_bits, fp_frac, out);
}
int rofl_dbg_dgauss_geometry(size_t d, uint32_t *elements_per_lane, uint32_t *lds_blocks) {
    if (!elements_per_lane || !lds_blocks || d >= ((size_t)1 << 28)) return ROFL_BAD_PARAM;
    const size_t lanes = (size_t)dgauss_grid(1, d) * DG_TPB;
    *elements_per_lane = (uint32_t)((d + lanes - 1) / lanes); *lds_blocks = DG_R;
    return 0;
}
int rofl_dbg_clip_l2_round(unsigned site, size_t n, const uint64_t *q, uint32_t m, const uint32_t *words, unsigned fp_frac, float *out) {
    if (site > 1 || fp_frac > 12 || n > (1u << 20) || (n && (!q || !out))) return fail(ROFL_BAD_PARAM, "bad parameter");
    if (n == 0) return ROFL_OK;
    if (site == 0) { for (size_t i = 0; i < n; i++) out[i] = clip_l2_round(q[i], m, words != nullptr, words ? words[i] : 0u, 1.0f, fp_frac); return ROFL_OK; }
    return probe_run(n, q, words, out, [&](Ctx &C, u32 cnt, const u64 *dq, const u32 *dw, float *dout) {
        ROFL_LAUNCH(k_dbg_clip_l2_round, grid1(n), dim3(TPB), 0, C.stream, cnt, dq, (u32)m, dw, (u32)fp_frac, dout); });
}
int rofl_dbg_clip_l2_route(unsigned route, size_t n_vec, const uint8_t *seeds32, const float *const *values, size_t d, const uint64_t *max_sq,
                           size_t prove_range, unsigned fp_bits, unsigned fp_frac, float *const *out, uint64_t *scale_out) {
    if (route > 1) return fail(ROFL_BAD_PARAM, "bad parameter");
    return clip_l2_impl((int)route, n_vec, seeds32, values, d, max_sq, prove_range, fp_bits, fp_frac, out, scale_out);
}
int rofl_dbg_rotate_route(unsigned route, size_t n_vec, const uint8_t *seeds32, const float *const *values, size_t d, unsigned block_log2, int inverse,
                          float *const *out) {
    if (route > 1) return fail(ROFL_BAD_PARAM, "bad parameter");
    return rotate_impl((int)route, n_vec, seeds32, values, d, block_log2, inverse, out);
}
int rofl_dbg_rotate_tile_log2(void) { return ROT_T_LOG2; }
