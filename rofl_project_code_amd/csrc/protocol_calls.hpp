// The protocol primitives of a secure-aggregation round -- key agreement, Shamir shares, Feldman commitments, Schnorr signatures, sealed
// shares, DLEQ complaints -- each with its device driver and its one-thread host twin.  Included by rofl_zk.hip at file scope, inside its
// extern "C" section: the file closes and reopens that section and the anonymous namespace as it goes.
#pragma once
// ---- the staging every device driver below shares ----
}  // extern "C"
namespace {
void dh_wipe(void *p, size_t n) { volatile uint8_t *q = (volatile uint8_t *)p; for (size_t i = 0; i < n; i++) q[i] = 0; }
// One call's way through a lane: declare the parts, upload(), launch, finish().  The inputs are packed into ONE upload (pinned C.h_misc ->
// device C.tmp_in), the outputs into ONE download (device C.tmp_out -> pinned C.h_misc2); C.tmp_in2 is the call's device-only workspace.
// Every part starts 8-byte aligned (kAlign16: 16, the signatures); a kPadded byte string is rounded up to 8 bytes and followed by 8 more,
// because the kernels read whole aligned words; gaps and padding are zero.  An input whose source is null is absent: it takes no room
// and its device pointer is null -- EXCEPT a kPadded one, which keeps its 8 zero bytes and a non-null pointer (an empty byte string: the
// kernels are handed a pointer they may read a word from).  An output whose destination is null is computed but not delivered.
// kSecret parts come first in their buffer (a secret declared behind a public part is refused, so nothing can shorten the wiped range by
// accident): the lane's copies of them -- device and pinned -- and a kSecret workspace are overwritten with zeros when the call returns or
// unwinds, under ONE synchronisation and before the lane is released.  The public bulk behind them is left alone.
enum : unsigned { kSecret = 1, kPadded = 2, kAlign16 = 4 };
struct InPart { size_t at, room; };
struct OutPart { size_t at; };
struct StagedCall {
    LaneLock lane; Ctx &C;      // (the lane is the first member: released after the destructor's wipe)
    struct Item { void *user; size_t at, bytes; } ins[8], outs[4];
    int n_in = 0, n_out = 0;
    size_t up_bytes = 0, up_secret = 0, dn_bytes = 0, dn_secret = 0, ws_secret = 0;
    uint8_t *hu = nullptr, *du = nullptr, *hd = nullptr, *dd = nullptr, *ws = nullptr;
    StagedCall() : lane(acquire_lane()), C(*lane.c) { C.init(); }
    StagedCall(const StagedCall &) = delete; StagedCall &operator=(const StagedCall &) = delete;
    static size_t place(Item *list, int &count, int max, void *user, size_t bytes, size_t room, unsigned flags, size_t &end, size_t &secret) {
        const size_t a = flags & kAlign16 ? 15 : 7, at = (end + a) & ~a;
        if (room && count == max) throw std::logic_error("StagedCall: more parts than the call has slots for");
        if ((flags & kSecret) && at != secret) throw std::logic_error("StagedCall: a secret part declared behind a public one");
        end = at + room;
        if (flags & kSecret) secret = end;
        if (room) list[count++] = {user, at, bytes};
        return at;
    }
    InPart in(const void *src, size_t bytes, unsigned flags = 0) {
        if (!src) bytes = 0;
        const size_t room = flags & kPadded ? ((bytes + 7) & ~(size_t)7) + 8 : bytes;
        return {place(ins, n_in, 8, const_cast<void *>(src), bytes, room, flags, up_bytes, up_secret), room};
    }
    OutPart out(void *dst, size_t bytes, unsigned flags = 0) { return {place(outs, n_out, 4, dst, bytes, bytes, flags, dn_bytes, dn_secret)}; }
    template <class T> T *work(size_t count, unsigned flags = 0) {
        ws = C.tmp_in2.as<uint8_t>(std::max<size_t>(count * sizeof(T), 1));
        if (flags & kSecret) ws_secret = count * sizeof(T);
        return reinterpret_cast<T *>(ws);
    }
    void upload() {
        hu = C.h_misc.as<uint8_t>(up_bytes); du = C.tmp_in.as<uint8_t>(up_bytes);
        hd = C.h_misc2.as<uint8_t>(dn_bytes); dd = C.tmp_out.as<uint8_t>(dn_bytes);
        for (int i = 0; i < n_in; i++) {
            const size_t end = ins[i].at + ins[i].bytes, next = i + 1 < n_in ? ins[i + 1].at : up_bytes;
            if (ins[i].bytes) memcpy(hu + ins[i].at, ins[i].user, ins[i].bytes);
            memset(hu + end, 0, next - end);
        }
        HIPCHK(hipMemcpyAsync(du, hu, up_bytes, hipMemcpyHostToDevice, C.stream));
    }
    // the parts as the kernels see them, after upload(); T: what a kernel reads or writes the bytes as
    template <class T> const T *dev(InPart p) const { return p.room ? reinterpret_cast<const T *>(du + p.at) : nullptr; }
    template <class T> T *dev(OutPart p) const { return reinterpret_cast<T *>(dd + p.at); }
    // one download, the call's wait, and every output that has a destination handed over
    void finish() {
        HIPCHK(hipMemcpyAsync(hd, dd, dn_bytes, hipMemcpyDeviceToHost, C.stream));
        C.sync();
        for (int i = 0; i < n_out; i++) if (outs[i].user) memcpy(outs[i].user, hd + outs[i].at, outs[i].bytes);
    }
    const uint8_t *host(OutPart p) const { return hd + p.at; }      // after finish(): a part the driver delivers itself
    ~StagedCall() {
        const bool up = du && up_secret, dn = dd && dn_secret, w = ws && ws_secret;
        if (up) (void)hipMemsetAsync(du, 0, up_secret, C.stream);
        if (dn) (void)hipMemsetAsync(dd, 0, dn_secret, C.stream);
        if (w) (void)hipMemsetAsync(ws, 0, ws_secret, C.stream);
        if (up || dn || w) (void)hipStreamSynchronize(C.stream);
        if (hu) dh_wipe(hu, up_secret);
        if (hd) dh_wipe(hd, dn_secret);
    }
};
// ---- key agreement: where the pairwise masks' shared secrets come from (k_dh_public, k_dh_decode, k_dh_shared) ----
// a secret key as the kernels read it (load_sc_reduced): 32 little-endian bytes reduced mod l
sc dh_key_scalar(const uint8_t *sk32) { sc r = sc_frombytes(sk32); if (sc_geq_l(r.v)) r = sc_from_mont(sc_to_mont(r)); return r; }
// own keys that are 0 mod l are refused before the device is touched; the text names the index, never the bytes
int dh_check_keys(size_t n, const uint8_t *sk32) {
    for (size_t i = 0; i < n; i++) {
        sc k = dh_key_scalar(sk32 + 32 * i); const bool zero = sc_iszero(k); dh_wipe(&k, sizeof k);
        if (zero) { char buf[96]; snprintf(buf, sizeof buf, "secret key %zu is zero mod l", i); return fail(ROFL_BAD_PARAM, buf); }
    }
    return ROFL_OK;
}
// k P on the host's 51-bit arithmetic, signed radix-16 windows like sg_var_mul (k canonical)
h51::ge5 dh_host_mul(const sc &k, const h51::ge5 &P) {
    h51::ge5 tab[8]; tab[0] = P;
    for (int e = 1; e < 8; e++) tab[e] = h51::gadd(tab[e - 1], P);
    int8_t dg[65]; int carry = 0;
    for (int i = 0; i < 64; i++) { int v = (int)((k.v[i >> 3] >> ((i & 7) * 4)) & 15) + carry; carry = (v + 8) >> 4; dg[i] = (int8_t)(v - (carry << 4)); }
    dg[64] = (int8_t)carry;
    h51::ge5 acc = h51::identity();
    for (int i = 64; i >= 0; i--) {
        if (i != 64) for (int q = 0; q < 4; q++) acc = h51::gdouble(acc);
        const int d = dg[i], ad = d < 0 ? -d : d;
        if (ad) { h51::ge5 q = tab[ad - 1]; if (d < 0) { q.X = h51::neg(q.X); q.T = h51::neg(q.T); } acc = h51::gadd(acc, q); }
    }
    dh_wipe(dg, sizeof dg);
    return acc;
}
// the shared secret of rofl_dh_shared from S = encode(a decode(P_b)) and the two public keys, in either order
void dh_host_secret(uint8_t out32[32], const uint8_t S[32], const uint8_t own[32], const uint8_t peer[32]) {
    uint8_t m[112] = {'r', 'o', 'f', 'l', '-', 'z', 'k', '/', 'd', 'h', '/', 'v', '1', 0, 0, 0};
    memcpy(m + 16, S, 32);
    const bool own_first = memcmp(own, peer, 32) <= 0;
    memcpy(m + 48, own_first ? own : peer, 32); memcpy(m + 80, own_first ? peer : own, 32);
    u64 st[25]; memset(st, 0, sizeof st); memcpy(st, m, 112);
    st[14] ^= 0x1FULL; st[16] ^= 0x8000000000000000ULL;
    keccak_f1600_host(st);
    memcpy(out32, st, 32);
    dh_wipe(m, sizeof m); dh_wipe(st, sizeof st);
}
const uint8_t kDhBase[32] = {0xe2, 0xf2, 0xae, 0x0a, 0x6a, 0xbc, 0x4e, 0x71, 0xa8, 0x84, 0xa9, 0x61, 0xc5, 0x00, 0x51, 0x5f,
                             0x58, 0xe3, 0x0b, 0x6a, 0xa5, 0x82, 0xdd, 0x8d, 0xb6, 0xa6, 0x59, 0x45, 0xe0, 0x8d, 0x2d, 0x76};
h51::ge5 host_base() { ge B; ristretto_decode(B, kDhBase); return h51::from_ge(B); }
// the keys of a host route decoded once: refused[j] as k_dh_decode's status word (1 not canonical, 2 the identity)
void host_decode_keys(size_t n, const uint8_t *pk32, std::vector<uint8_t> &refused, std::vector<h51::ge5> &pts) {
    refused.assign(n, 0); pts.resize(n);
    for (size_t j = 0; j < n; j++) {
        ge P;
        refused[j] = !ristretto_decode(P, pk32 + 32 * j) ? 1 : ge_is_identity_ristretto(P) ? 2 : 0;
        if (!refused[j]) pts[j] = h51::from_ge(P);
    }
}
// how the signing and the proving host route begin: per secret key its scalar, its canonical bytes and its public key; returns the base point
h51::ge5 host_own_keys(size_t n, const uint8_t *sk32, std::vector<sc> &keys, std::vector<uint8_t> &can, std::vector<uint8_t> &pk) {
    const h51::ge5 B = host_base();
    keys.resize(n); can.resize(n * 32); pk.resize(n * 32);
    for (size_t a = 0; a < n; a++) {
        keys[a] = dh_key_scalar(sk32 + 32 * a);
        sc_tobytes(can.data() + 32 * a, keys[a]);
        h51::encode(pk.data() + 32 * a, dh_host_mul(keys[a], B));
    }
    return B;
}
// int_le(SHAKE256(label16 || the parts, 32 bytes each)[0 .. 64)) mod l: the nonces and challenges of the signatures ("rofl-zk/sig/v1/k" over
// two parts, ".../c" over three) and of the DLEQ proofs ("rofl-zk/dleq/v1k" over three, "...c" over six)
sc host_wide(const char *label16, const uint8_t *const *parts, int n_parts) {
    uint8_t m[208], w[64];
    memcpy(m, label16, 16);
    for (int p = 0; p < n_parts; p++) memcpy(m + 16 + 32 * p, parts[p], 32);
    Sponge sp(136, 0x1F); sp.absorb(m, 16 + 32 * (size_t)n_parts); sp.squeeze(w, 64);
    sc r = sc_from_wide(sc_frombytes(w), sc_frombytes(w + 32));
    dh_wipe(m, sizeof m); dh_wipe(w, sizeof w); dh_wipe(&sp, sizeof sp);
    return r;
}
// the pair list of rofl_dh_shared and of the DLEQ calls
int dh_check_pairs(size_t n_own, size_t n_peer, size_t n_pairs, const rofl_dh_pair_t *pairs) {
    if (n_own == 0 || n_peer == 0) return fail(ROFL_BAD_PARAM, "pairs without keys");
    if (n_own > ((size_t)1 << 20) || n_peer > ((size_t)1 << 20)) return fail(ROFL_BAD_PARAM, "more than 2^20 keys in one call");
    if (n_pairs > ((size_t)1 << 24)) return fail(ROFL_BAD_PARAM, "more than 2^24 pairs in one call");
    if (!pairs && n_pairs != n_own * n_peer) return fail(ROFL_BAD_PARAM, "without a pair list n_pairs is n_own x n_peer");
    if (pairs) for (size_t i = 0; i < n_pairs; i++)
        if (pairs[i].own >= n_own || pairs[i].peer >= n_peer) { char buf[96]; snprintf(buf, sizeof buf, "pair %zu names a key that is not in the call", i); return fail(ROFL_BAD_PARAM, buf); }
    return ROFL_OK;
}
}  // namespace
extern "C" {
int rofl_dh_public_keys(size_t n, const uint8_t *sk32, uint8_t *pk_out32) {
    if (n == 0) return ROFL_OK;
    if (!sk32 || !pk_out32) return fail(ROFL_BAD_PARAM, "bad parameter");
    if (n > ((size_t)1 << 20)) return fail(ROFL_BAD_PARAM, "more than 2^20 keys in one call");
    if (int rc = dh_check_keys(n, sk32)) return rc;
    return guarded([&]() -> int {
        StagedCall st; Ctx &C = st.C;
        const InPart keys = st.in(sk32, n * 32, kSecret);
        const OutPart pk = st.out(pk_out32, n * 32);      // (on purpose through tmp_out / h_misc2 like every other call; it used to be the second half of tmp_in / h_misc)
        st.upload();
        ROFL_LAUNCH(k_dh_public, per_item(n), dim3(64), 0, C.stream, (u32)n, st.dev<sc>(keys), C.d_tabB8, st.dev<uint8_t>(pk));
        st.finish();
        return ROFL_OK;
    });
}
// The lane's copies of the secret keys and of the shared secrets -- pinned staging and device workspace -- are overwritten with zeros before the
// call returns or unwinds (the product encodings never leave the threads' registers and scratch).
int rofl_dh_shared(size_t n_own, const uint8_t *sk32, uint8_t *own_pk_out32, size_t n_peer, const uint8_t *peer_pk32,
                   size_t n_pairs, const rofl_dh_pair_t *pairs, uint8_t *out32, uint8_t *status_out) {
    if (n_pairs == 0) return ROFL_OK;
    if (!sk32 || !peer_pk32 || !out32 || !status_out) return fail(ROFL_BAD_PARAM, "bad parameter");
    if (int rc = dh_check_pairs(n_own, n_peer, n_pairs, pairs)) return rc;
    if (int rc = dh_check_keys(n_own, sk32)) return rc;
    return guarded([&]() -> int {
        StagedCall st; Ctx &C = st.C;
        const InPart keys = st.in(sk32, n_own * 32, kSecret), peer = st.in(peer_pk32, n_peer * 32), pl = st.in(pairs, n_pairs * sizeof(rofl_dh_pair_t));
        const OutPart shared = st.out(out32, n_pairs * 32, kSecret), pk = st.out(own_pk_out32, n_own * 32), status = st.out(status_out, n_pairs);
        ge *pts = C.aux_pts.as<ge>(n_peer); u32 *pst = C.status.as<u32>(n_peer);
        st.upload();
        ROFL_LAUNCH(k_dh_public, per_item(n_own), dim3(64), 0, C.stream, (u32)n_own, st.dev<sc>(keys), C.d_tabB8, st.dev<uint8_t>(pk));
        ROFL_LAUNCH(k_dh_decode, per_item(n_peer), dim3(64), 0, C.stream, (u32)n_peer, st.dev<uint8_t>(peer), pts, pst);
        ROFL_LAUNCH(k_dh_shared, per_item(n_pairs), dim3(64), 0, C.stream, (u32)n_pairs, (u32)n_peer, st.dev<uint2>(pl), st.dev<sc>(keys), (const uint8_t *)st.dev<uint8_t>(pk),
                    st.dev<uint8_t>(peer), (const ge *)pts, (const u32 *)pst, st.dev<uint8_t>(shared), st.dev<uint8_t>(status));
        st.finish();
        return ROFL_OK;
    });
}
// one pair of rofl_dh_shared from the host arithmetic (no GPU): status 0 / 1 / 2 as there, 11 for a zero own key
int rofl_dbg_host_dh(const uint8_t sk32[32], const uint8_t *own_pk32, const uint8_t peer_pk32[32], uint8_t out32[32], uint8_t *status) {
    if (!sk32 || !peer_pk32 || !out32 || !status) return fail(ROFL_BAD_PARAM, "bad parameter");
    if (int rc = dh_check_keys(1, sk32)) return rc;
    memset(out32, 0, 32);
    std::vector<uint8_t> refused; std::vector<h51::ge5> pp;
    host_decode_keys(1, peer_pk32, refused, pp);
    *status = refused[0];
    if (refused[0]) return ROFL_OK;
    sc k = dh_key_scalar(sk32);
    uint8_t own[32], S[32];
    if (own_pk32) memcpy(own, own_pk32, 32);
    else h51::encode(own, dh_host_mul(k, host_base()));
    h51::encode(S, dh_host_mul(k, pp[0]));
    dh_host_secret(out32, S, own, peer_pk32);
    dh_wipe(&k, sizeof k); dh_wipe(S, sizeof S);
    return ROFL_OK;
}
// ---- secret sharing: Shamir shares of mask secrets over the scalar field (k_shamir_coeffs, k_shamir_eval, k_shamir_weights, k_shamir_combine) ----
}  // extern "C"
namespace {
// the evaluation points of a call: nonzero and distinct; the text names positions, never values of anything secret
int shamir_check_xs(size_t n, const uint32_t *xs) {
    std::vector<std::pair<uint32_t, uint32_t>> v(n);
    for (size_t i = 0; i < n; i++) {
        if (xs[i] == 0) { char buf[96]; snprintf(buf, sizeof buf, "evaluation point %zu is zero", i); return fail(ROFL_BAD_PARAM, buf); }
        v[i] = {xs[i], (uint32_t)i};
    }
    std::sort(v.begin(), v.end());
    for (size_t i = 1; i < n; i++)
        if (v[i].first == v[i - 1].first) { char buf[96]; snprintf(buf, sizeof buf, "evaluation points %u and %u are equal", v[i - 1].second, v[i].second); return fail(ROFL_BAD_PARAM, buf); }
    return ROFL_OK;
}
// every check of rofl_shamir_share, shared with its host route; *done: the call is empty and returns 0
int shamir_share_check(size_t n_secrets, const uint8_t *secrets32, const uint8_t *coef_seeds32, size_t threshold, size_t n_shares, const uint32_t *xs,
                       const uint8_t *shares_out32, bool *done) {
    *done = n_secrets == 0;
    if (*done) return ROFL_OK;
    if (!secrets32 || !coef_seeds32 || !shares_out32) return fail(ROFL_BAD_PARAM, "bad parameter");
    if (n_shares == 0) return fail(ROFL_BAD_PARAM, "secrets without shares");
    if (threshold == 0 || threshold > n_shares) return fail(ROFL_BAD_PARAM, "the threshold is in [1, n_shares]");
    if (threshold > 65536) return fail(ROFL_BAD_PARAM, "a threshold above 65536");
    if (n_secrets > 65535) return fail(ROFL_BAD_PARAM, "more than 65535 secrets in one call");
    if (n_shares > ((size_t)1 << 20)) return fail(ROFL_BAD_PARAM, "more than 2^20 shares of a secret in one call");
    if (n_secrets * n_shares > ((size_t)1 << 24)) return fail(ROFL_BAD_PARAM, "more than 2^24 shares in one call");
    if (n_secrets * (threshold - 1) > ((size_t)1 << 24)) return fail(ROFL_BAD_PARAM, "more than 2^24 coefficients in one call");
    return xs ? shamir_check_xs(n_shares, xs) : ROFL_OK;
}
int shamir_reconstruct_check(size_t n_secrets, size_t n_shares, const uint32_t *xs, const uint8_t *shares32, const uint8_t *secrets_out32, bool *done) {
    *done = n_secrets == 0;
    if (*done) return ROFL_OK;
    if (!xs || !shares32 || !secrets_out32) return fail(ROFL_BAD_PARAM, "bad parameter");
    if (n_shares == 0) return fail(ROFL_BAD_PARAM, "secrets without shares");
    if (n_secrets > 65535) return fail(ROFL_BAD_PARAM, "more than 65535 secrets in one call");
    if (n_shares > 65536) return fail(ROFL_BAD_PARAM, "more than 65536 shares of a secret in one call");
    if (n_secrets * n_shares > ((size_t)1 << 24)) return fail(ROFL_BAD_PARAM, "more than 2^24 shares in one call");
    return shamir_check_xs(n_shares, xs);
}
}  // namespace
extern "C" {
// The lane's copies of the secrets, the coefficient seeds, the coefficients and the shares -- pinned staging and device workspace -- are
// overwritten with zeros before the call returns or unwinds.
int rofl_shamir_share(size_t n_secrets, const uint8_t *secrets32, const uint8_t *coef_seeds32, size_t threshold, size_t n_shares, const uint32_t *xs,
                      uint8_t *shares_out32) {
    bool done;
    if (int rc = shamir_share_check(n_secrets, secrets32, coef_seeds32, threshold, n_shares, xs, shares_out32, &done)) return rc;
    if (done) return ROFL_OK;
    return guarded([&]() -> int {
        StagedCall st; Ctx &C = st.C;
        const size_t m = threshold - 1;
        const InPart sec = st.in(secrets32, n_secrets * 32, kSecret), seeds = st.in(coef_seeds32, n_secrets * 32, kSecret), pts = st.in(xs, n_shares * 4);
        const OutPart shares = st.out(shares_out32, n_secrets * n_shares * 32, kSecret);      // secret-major
        sc *coef = st.work<sc>(n_secrets * m, kSecret);
        st.upload();
        if (m) ROFL_LAUNCH(k_shamir_coeffs, grid1((m + 1) / 2, (u32)n_secrets), dim3(TPB), 0, C.stream, (u32)m, st.dev<u64>(seeds), coef);
        ROFL_LAUNCH(k_shamir_eval, grid1(n_shares, (u32)n_secrets), dim3(TPB), 0, C.stream, (u32)m, (u32)n_shares, st.dev<sc>(sec), (const sc *)coef, st.dev<u32>(pts), st.dev<sc>(shares));
        st.finish();
        return ROFL_OK;
    });
}
int rofl_shamir_reconstruct(size_t n_secrets, size_t n_shares, const uint32_t *xs, const uint8_t *shares32, uint8_t *secrets_out32) {
    bool done;
    if (int rc = shamir_reconstruct_check(n_secrets, n_shares, xs, shares32, secrets_out32, &done)) return rc;
    if (done) return ROFL_OK;
    return guarded([&]() -> int {
        StagedCall st; Ctx &C = st.C;
        const InPart shares = st.in(shares32, n_secrets * n_shares * 32, kSecret), pts = st.in(xs, n_shares * 4);      // the shares secret-major
        const OutPart sec = st.out(secrets_out32, n_secrets * 32, kSecret);
        sc *w = st.work<sc>(n_shares);      // the weights: a function of the points alone
        st.upload();
        ROFL_LAUNCH(k_shamir_weights, grid1(n_shares), dim3(TPB), 0, C.stream, (u32)n_shares, st.dev<u32>(pts), w);
        ROFL_LAUNCH(k_shamir_combine, dim3((unsigned)n_secrets), dim3(TPB), 0, C.stream, (u32)n_shares, (const sc *)w, st.dev<sc>(shares), st.dev<sc>(sec));
        st.finish();
        return ROFL_OK;
    });
}
// the two calls on the host's scalar arithmetic and host Keccak, one thread, no GPU: same parameters, same checks, same bytes
int rofl_dbg_host_shamir_share(size_t n_secrets, const uint8_t *secrets32, const uint8_t *coef_seeds32, size_t threshold, size_t n_shares, const uint32_t *xs,
                               uint8_t *shares_out32) {
    bool done;
    if (int rc = shamir_share_check(n_secrets, secrets32, coef_seeds32, threshold, n_shares, xs, shares_out32, &done)) return rc;
    if (done) return ROFL_OK;
    const size_t m = threshold - 1;
    const u64 dom[2] = ROFL_SHARE_DOM;
    std::vector<sc> coef(m + 1);
    for (size_t s = 0; s < n_secrets; s++) {
        u64 sd[4], st[25]; memcpy(sd, coef_seeds32 + 32 * s, 32);
        for (size_t blk = 0; 2 * blk < m; blk++) {
            shake256_seeded_block(st, dom, sd, blk);
            coef[2 * blk] = xof_block_scalar(st, 0); coef[2 * blk + 1] = xof_block_scalar(st, 1);      // (coef has room for one past m)
        }
        sc sec = dh_key_scalar(secrets32 + 32 * s);
        for (size_t i = 0; i < n_shares; i++) {
            const sc xR = sc_to_mont(sc_from_u64(xs ? xs[i] : (u64)i + 1));
            sc acc = sc_zero();
            for (size_t k = m; k-- > 0;) acc = sc_add(sc_montmul(acc, xR), coef[k]);
            acc = sc_add(sc_montmul(acc, xR), sec);
            sc_tobytes(shares_out32 + (s * n_shares + i) * 32, acc);
            dh_wipe(&acc, sizeof acc);
        }
        dh_wipe(&sec, sizeof sec); dh_wipe(sd, sizeof sd); dh_wipe(st, sizeof st);
    }
    dh_wipe(coef.data(), coef.size() * sizeof(sc));
    return ROFL_OK;
}
int rofl_dbg_host_shamir_reconstruct(size_t n_secrets, size_t n_shares, const uint32_t *xs, const uint8_t *shares32, uint8_t *secrets_out32) {
    bool done;
    if (int rc = shamir_reconstruct_check(n_secrets, n_shares, xs, shares32, secrets_out32, &done)) return rc;
    if (done) return ROFL_OK;
    std::vector<sc> w(n_shares);      // lambda_j in Montgomery form; N and D carry the same power of R (k_shamir_weights)
    for (size_t j = 0; j < n_shares; j++) {
        sc N = sc_one_plain(), D = sc_one_plain();
        for (size_t k = 0; k < n_shares; k++) {
            if (k == j) continue;
            const u32 xm = xs[k], xj = xs[j];
            sc fd = sc_from_u64(xm > xj ? xm - xj : xj - xm); if (xm < xj) fd = sc_neg(fd);
            N = sc_montmul(N, sc_from_u64(xm)); D = sc_montmul(D, fd);
        }
        w[j] = sc_montmul(N, h51::sc_invert_mont_fast(D));
    }
    for (size_t s = 0; s < n_secrets; s++) {
        sc acc = sc_zero();
        for (size_t j = 0; j < n_shares; j++) acc = sc_add(acc, sc_montmul(w[j], dh_key_scalar(shares32 + (s * n_shares + j) * 32)));
        sc_tobytes(secrets_out32 + 32 * s, acc);
        dh_wipe(&acc, sizeof acc);
    }
    return ROFL_OK;
}
// ---- verifiable sharing: Feldman commitments to the polynomials above, one exact equation per share (k_feldman_commit, k_dh_decode, k_feldman_check) ----
}  // extern "C"
namespace {
// every check of rofl_feldman_commit / rofl_feldman_verify, shared with their host routes; *done: the call is empty and returns 0
int feldman_commit_check(size_t n_secrets, const uint8_t *secrets32, const uint8_t *coef_seeds32, size_t threshold, const uint8_t *commitments_out32, bool *done) {
    *done = n_secrets == 0;
    if (*done) return ROFL_OK;
    if (!secrets32 || !coef_seeds32 || !commitments_out32) return fail(ROFL_BAD_PARAM, "bad parameter");
    if (threshold == 0) return fail(ROFL_BAD_PARAM, "the threshold is at least 1");
    if (threshold > 65536) return fail(ROFL_BAD_PARAM, "a threshold above 65536");
    if (n_secrets > 65535) return fail(ROFL_BAD_PARAM, "more than 65535 secrets in one call");
    if (n_secrets * threshold > ((size_t)1 << 22)) return fail(ROFL_BAD_PARAM, "more than 2^22 commitments in one call");
    return ROFL_OK;
}
int feldman_verify_check(size_t n_secrets, size_t threshold, const uint8_t *commitments32, size_t n_shares, const uint32_t *xs, const uint8_t *shares32,
                         const uint8_t *verdict_out, bool *done) {
    *done = n_secrets == 0;
    if (*done) return ROFL_OK;
    if (!commitments32 || !shares32 || !verdict_out) return fail(ROFL_BAD_PARAM, "bad parameter");
    if (n_shares == 0) return fail(ROFL_BAD_PARAM, "secrets without shares");
    if (threshold == 0) return fail(ROFL_BAD_PARAM, "the threshold is at least 1");
    if (threshold > 65536) return fail(ROFL_BAD_PARAM, "a threshold above 65536");
    if (n_secrets > 65535) return fail(ROFL_BAD_PARAM, "more than 65535 secrets in one call");
    if (n_shares > ((size_t)1 << 20)) return fail(ROFL_BAD_PARAM, "more than 2^20 shares of a secret in one call");
    if (n_secrets * n_shares > ((size_t)1 << 24)) return fail(ROFL_BAD_PARAM, "more than 2^24 shares in one call");
    if (n_secrets * threshold > ((size_t)1 << 22)) return fail(ROFL_BAD_PARAM, "more than 2^22 commitments in one call");
    return xs ? shamir_check_xs(n_shares, xs) : ROFL_OK;
}
// bit length of the largest evaluation point of a call (>= 1: the points are nonzero)
u32 feldman_xbits(size_t n_shares, const uint32_t *xs) {
    uint32_t mx = xs ? 0 : (uint32_t)n_shares;
    for (size_t i = 0; xs && i < n_shares; i++) mx = std::max(mx, xs[i]);
    u32 b = 0; while (b < 32 && mx >> b) b++;
    return b;
}
}  // namespace
extern "C" {
// The lane's copies of the secrets, the coefficient seeds and the coefficients -- pinned staging and device workspace -- are overwritten with
// zeros before the call returns or unwinds; the commitments are public.
int rofl_feldman_commit(size_t n_secrets, const uint8_t *secrets32, const uint8_t *coef_seeds32, size_t threshold, uint8_t *commitments_out32) {
    bool done;
    if (int rc = feldman_commit_check(n_secrets, secrets32, coef_seeds32, threshold, commitments_out32, &done)) return rc;
    if (done) return ROFL_OK;
    return guarded([&]() -> int {
        StagedCall st; Ctx &C = st.C;
        const size_t m = threshold - 1, n_com = n_secrets * threshold;
        const InPart sec = st.in(secrets32, n_secrets * 32, kSecret), seeds = st.in(coef_seeds32, n_secrets * 32, kSecret);
        const OutPart com = st.out(commitments_out32, n_com * 32);      // secret-major
        sc *coef = st.work<sc>(n_secrets * m, kSecret);
        st.upload();
        if (m) ROFL_LAUNCH(k_shamir_coeffs, grid1((m + 1) / 2, (u32)n_secrets), dim3(TPB), 0, C.stream, (u32)m, st.dev<u64>(seeds), coef);
        ROFL_LAUNCH(k_feldman_commit, per_item(n_com), dim3(64), 0, C.stream, (u32)n_secrets, (u32)threshold, st.dev<sc>(sec), (const sc *)coef, C.d_tabB8, st.dev<uint8_t>(com));
        st.finish();
        return ROFL_OK;
    });
}
// The lane's copies of the shares are overwritten with zeros before the call returns or unwinds; commitments, points and verdicts are public.
int rofl_feldman_verify(size_t n_secrets, size_t threshold, const uint8_t *commitments32, size_t n_shares, const uint32_t *xs, const uint8_t *shares32,
                        uint8_t *verdict_out) {
    bool done;
    if (int rc = feldman_verify_check(n_secrets, threshold, commitments32, n_shares, xs, shares32, verdict_out, &done)) return rc;
    if (done) return ROFL_OK;
    const u32 xbits = feldman_xbits(n_shares, xs);
    return guarded([&]() -> int {
        StagedCall st; Ctx &C = st.C;
        const size_t n_pairs = n_secrets * n_shares, n_com = n_secrets * threshold;
        const InPart shares = st.in(shares32, n_pairs * 32, kSecret), com = st.in(commitments32, n_com * 32), xp = st.in(xs, n_shares * 4);      // both secret-major
        const OutPart verdict = st.out(verdict_out, n_pairs);
        ge *pts = C.aux_pts.as<ge>(n_com); u32 *pst = C.status.as<u32>(n_com);      // the decoded commitments and their status words
        st.upload();
        ROFL_LAUNCH(k_dh_decode, per_item(n_com), dim3(64), 0, C.stream, (u32)n_com, st.dev<uint8_t>(com), pts, pst);
        ROFL_LAUNCH(k_feldman_check, per_item(n_pairs), dim3(64), 0, C.stream, (u32)n_secrets, (u32)n_shares, (u32)threshold, xbits, st.dev<u32>(xp), (const ge *)pts, (const u32 *)pst,
                    st.dev<sc>(shares), C.d_tabB8, st.dev<uint8_t>(verdict));
        st.finish();
        return ROFL_OK;
    });
}
// the two calls on the host's 51-bit point arithmetic, scalar arithmetic and host Keccak, one thread, no GPU: same parameters, same checks, same bytes
int rofl_dbg_host_feldman_commit(size_t n_secrets, const uint8_t *secrets32, const uint8_t *coef_seeds32, size_t threshold, uint8_t *commitments_out32) {
    bool done;
    if (int rc = feldman_commit_check(n_secrets, secrets32, coef_seeds32, threshold, commitments_out32, &done)) return rc;
    if (done) return ROFL_OK;
    const size_t m = threshold - 1;
    const u64 dom[2] = ROFL_SHARE_DOM;
    const h51::ge5 B = host_base();
    std::vector<sc> coef(m + 2);      // [s mod l | a_1 .. a_{t-1}] and room for one past the end
    for (size_t s = 0; s < n_secrets; s++) {
        u64 sd[4], st[25]; memcpy(sd, coef_seeds32 + 32 * s, 32);
        coef[0] = dh_key_scalar(secrets32 + 32 * s);
        for (size_t blk = 0; 2 * blk < m; blk++) {
            shake256_seeded_block(st, dom, sd, blk);
            coef[1 + 2 * blk] = xof_block_scalar(st, 0); coef[2 + 2 * blk] = xof_block_scalar(st, 1);
        }
        for (size_t k = 0; k < threshold; k++) h51::encode(commitments_out32 + (s * threshold + k) * 32, dh_host_mul(coef[k], B));
        dh_wipe(sd, sizeof sd); dh_wipe(st, sizeof st);
    }
    dh_wipe(coef.data(), coef.size() * sizeof(sc));
    return ROFL_OK;
}
int rofl_dbg_host_feldman_verify(size_t n_secrets, size_t threshold, const uint8_t *commitments32, size_t n_shares, const uint32_t *xs, const uint8_t *shares32,
                                 uint8_t *verdict_out) {
    bool done;
    if (int rc = feldman_verify_check(n_secrets, threshold, commitments32, n_shares, xs, shares32, verdict_out, &done)) return rc;
    if (done) return ROFL_OK;
    const h51::ge5 B = host_base();
    std::vector<h51::ge5> cp(threshold);
    for (size_t s = 0; s < n_secrets; s++) {
        bool refused = false;
        for (size_t k = 0; k < threshold; k++) {
            ge P;
            if (!ristretto_decode(P, commitments32 + (s * threshold + k) * 32)) { refused = true; break; }
            cp[k] = h51::from_ge(P);
        }
        uint8_t *vd = verdict_out + s * n_shares;
        if (refused) { memset(vd, 2, n_shares); continue; }
        for (size_t i = 0; i < n_shares; i++) {
            const u32 x = xs ? xs[i] : (u32)(i + 1);
            h51::ge5 acc = cp[threshold - 1];
            for (size_t k = threshold - 1; k-- > 0;) {      // acc = [x] acc + C_k, MSB-first over the bits of x
                h51::ge5 r = h51::identity();
                for (int b = 32; b-- > 0;) {
                    if (x >> b >> 1) r = h51::gdouble(r);      // (nothing to double above the top bit)
                    if ((x >> b) & 1u) r = h51::gadd(r, acc);
                }
                acc = h51::gadd(r, cp[k]);
            }
            sc y = dh_key_scalar(shares32 + (s * n_shares + i) * 32);
            const h51::ge5 P = dh_host_mul(y, B);
            dh_wipe(&y, sizeof y);
            const bool same = h51::eq(h51::mul(acc.X, P.Y), h51::mul(acc.Y, P.X)) || h51::eq(h51::mul(acc.Y, P.Y), h51::mul(acc.X, P.X));
            vd[i] = same ? 0 : 1;
        }
    }
    return ROFL_OK;
}
// ---- signatures: deterministic Schnorr over Ristretto255 on the commitments and views of a round (k_sig_digest, k_dh_public / k_dh_decode, k_sig_sign / k_sig_verify) ----
}  // extern "C"
namespace {
// the packed messages of a call (signatures, Merkle leaves): offsets that start at 0 and do not decrease, at most 2^30 bytes; *total: the bytes
int msg_off_check(size_t n_msgs, const uint8_t *msg_bytes, const uint64_t *msg_off, size_t *total) {
    if (msg_off[0] != 0) return fail(ROFL_BAD_PARAM, "the first message offset is 0");
    for (size_t j = 0; j < n_msgs; j++) {
        if (msg_off[j + 1] < msg_off[j]) { char buf[96]; snprintf(buf, sizeof buf, "message offset %zu is below the one before it", j + 1); return fail(ROFL_BAD_PARAM, buf); }
        if (msg_off[j + 1] > ((uint64_t)1 << 30)) return fail(ROFL_BAD_PARAM, "more than 2^30 message bytes in one call");
    }
    *total = (size_t)msg_off[n_msgs];
    if (*total && !msg_bytes) return fail(ROFL_BAD_PARAM, "bad parameter");
    return ROFL_OK;
}
// every check of rofl_sig_sign / rofl_sig_verify, shared with their host routes; keys32: secret keys (sign) or public keys (verify), sig: the
// signatures read or written, verdict: verify's output; *done: the call is empty and returns 0.  *total: the messages' bytes
int sig_check(bool sign, size_t n_keys, const uint8_t *keys32, size_t n_msgs, const uint8_t *msg_bytes, const uint64_t *msg_off, size_t n, const rofl_sig_ref_t *refs,
              const uint8_t *sig, const uint8_t *verdict, size_t *total, bool *done) {
    *done = n == 0; *total = 0;
    if (*done) return ROFL_OK;
    if (!keys32 || !msg_off || !sig || (!sign && !verdict)) return fail(ROFL_BAD_PARAM, "bad parameter");
    if (n_keys == 0 || n_msgs == 0) return fail(ROFL_BAD_PARAM, "signatures without keys or without messages");
    if (n_keys > ((size_t)1 << 20)) return fail(ROFL_BAD_PARAM, "more than 2^20 keys in one call");
    if (n_msgs > ((size_t)1 << 20)) return fail(ROFL_BAD_PARAM, "more than 2^20 messages in one call");
    if (n > ((size_t)1 << 24)) return fail(ROFL_BAD_PARAM, "more than 2^24 signatures in one call");
    if (int rc = msg_off_check(n_msgs, msg_bytes, msg_off, total)) return rc;
    if (!refs && !(n_keys == n && n_msgs == n)) return fail(ROFL_BAD_PARAM, "without a ref list n_keys, n_msgs and n are equal");
    if (refs) for (size_t i = 0; i < n; i++)
        if (refs[i].key >= n_keys || refs[i].msg >= n_msgs) { char buf[96]; snprintf(buf, sizeof buf, "ref %zu names a key or a message that is not in the call", i); return fail(ROFL_BAD_PARAM, buf); }
    return sign ? dh_check_keys(n_keys, keys32) : ROFL_OK;
}
// SHAKE256(label16 || u64le(len) || m)[0 .. 32) on the host's sponge: labelled_digest's bytes
void host_labelled_digest(uint8_t out[32], const char *label16, const uint8_t *m, uint64_t len) {
    uint8_t pre[24];
    memcpy(pre, label16, 16); memcpy(pre + 16, &len, 8);
    Sponge sp(136, 0x1F); sp.absorb(pre, 24); if (len) sp.absorb(m, (size_t)len); sp.squeeze(out, 32);
}
// h(m) = SHAKE256("rofl-zk/sig/v1/m" || u64le(len) || m)[0 .. 32)
void sig_host_digest(uint8_t out[32], const uint8_t *m, uint64_t len) { host_labelled_digest(out, "rofl-zk/sig/v1/m", m, len); }
}  // namespace
extern "C" {
// The lane's copies of the secret keys -- pinned staging and device workspace -- are overwritten with zeros before the call returns or
// unwinds; the nonces never leave their threads' registers; digests, public keys and signatures are public.
int rofl_sig_sign(size_t n_keys, const uint8_t *sk32, uint8_t *pk_out32, size_t n_msgs, const uint8_t *msg_bytes, const uint64_t *msg_off,
                  size_t n, const rofl_sig_ref_t *refs, uint8_t *sig_out64) {
    bool done; size_t total;
    if (int rc = sig_check(true, n_keys, sk32, n_msgs, msg_bytes, msg_off, n, refs, sig_out64, nullptr, &total, &done)) return rc;
    if (done) return ROFL_OK;
    return guarded([&]() -> int {
        StagedCall st; Ctx &C = st.C;
        const InPart keys = st.in(sk32, n_keys * 32, kSecret), off = st.in(msg_off, (n_msgs + 1) * 8), rf = st.in(refs, n * sizeof(rofl_sig_ref_t)), msg = st.in(msg_bytes, total, kPadded);
        const OutPart sig = st.out(sig_out64, n * 64, kAlign16), pk = st.out(pk_out32, n_keys * 32);
        u64 *dig = st.work<u64>(n_msgs * 4);
        st.upload();
        ROFL_LAUNCH(k_sig_digest, per_item(n_msgs), dim3(64), 0, C.stream, (u32)n_msgs, st.dev<uint8_t>(msg), st.dev<u64>(off), dig);
        ROFL_LAUNCH(k_dh_public, per_item(n_keys), dim3(64), 0, C.stream, (u32)n_keys, st.dev<sc>(keys), C.d_tabB8, st.dev<uint8_t>(pk));
        ROFL_LAUNCH(k_sig_sign, per_item(n), dim3(64), 0, C.stream, (u32)n, st.dev<uint2>(rf), st.dev<sc>(keys), (const uint8_t *)st.dev<uint8_t>(pk), (const u64 *)dig, C.d_tabB8,
                    st.dev<uint8_t>(sig));
        st.finish();
        return ROFL_OK;
    });
}
// nothing here is secret: public keys, messages, signatures, verdicts
int rofl_sig_verify(size_t n_keys, const uint8_t *pk32, size_t n_msgs, const uint8_t *msg_bytes, const uint64_t *msg_off, size_t n, const rofl_sig_ref_t *refs,
                    const uint8_t *sig64, uint8_t *verdict_out) {
    bool done; size_t total;
    if (int rc = sig_check(false, n_keys, pk32, n_msgs, msg_bytes, msg_off, n, refs, sig64, verdict_out, &total, &done)) return rc;
    if (done) return ROFL_OK;
    return guarded([&]() -> int {
        StagedCall st; Ctx &C = st.C;
        const InPart keys = st.in(pk32, n_keys * 32), sig = st.in(sig64, n * 64, kAlign16), off = st.in(msg_off, (n_msgs + 1) * 8), rf = st.in(refs, n * sizeof(rofl_sig_ref_t)),
                     msg = st.in(msg_bytes, total, kPadded);
        const OutPart verdict = st.out(verdict_out, n);
        u64 *dig = st.work<u64>(n_msgs * 4);
        ge *pts = C.aux_pts.as<ge>(n_keys); u32 *pst = C.status.as<u32>(n_keys);      // the decoded keys and their status words
        st.upload();
        ROFL_LAUNCH(k_sig_digest, per_item(n_msgs), dim3(64), 0, C.stream, (u32)n_msgs, st.dev<uint8_t>(msg), st.dev<u64>(off), dig);
        ROFL_LAUNCH(k_dh_decode, per_item(n_keys), dim3(64), 0, C.stream, (u32)n_keys, st.dev<uint8_t>(keys), pts, pst);
        ROFL_LAUNCH(k_sig_verify, per_item(n), dim3(64), 0, C.stream, (u32)n, st.dev<uint2>(rf), st.dev<uint8_t>(keys), (const ge *)pts, (const u32 *)pst, (const u64 *)dig,
                    st.dev<uint8_t>(sig), C.d_tabB8, st.dev<uint8_t>(verdict));
        st.finish();
        return ROFL_OK;
    });
}
// the two calls on the host's 51-bit point arithmetic, scalar arithmetic and host Keccak, one thread, no GPU: same parameters, same checks, same bytes
int rofl_dbg_host_sig_sign(size_t n_keys, const uint8_t *sk32, uint8_t *pk_out32, size_t n_msgs, const uint8_t *msg_bytes, const uint64_t *msg_off,
                           size_t n, const rofl_sig_ref_t *refs, uint8_t *sig_out64) {
    bool done; size_t total;
    if (int rc = sig_check(true, n_keys, sk32, n_msgs, msg_bytes, msg_off, n, refs, sig_out64, nullptr, &total, &done)) return rc;
    if (done) return ROFL_OK;
    std::vector<uint8_t> dig(n_msgs * 32), pk, can;
    std::vector<sc> keys;
    const h51::ge5 B = host_own_keys(n_keys, sk32, keys, can, pk);
    for (size_t j = 0; j < n_msgs; j++) sig_host_digest(dig.data() + 32 * j, msg_bytes + msg_off[j], msg_off[j + 1] - msg_off[j]);
    for (size_t i = 0; i < n; i++) {
        const size_t a = refs ? refs[i].key : i, b = refs ? refs[i].msg : i;
        uint8_t *o = sig_out64 + 64 * i;
        const uint8_t *kparts[2] = {can.data() + 32 * a, dig.data() + 32 * b}, *cparts[3] = {o, pk.data() + 32 * a, dig.data() + 32 * b};
        sc k = host_wide("rofl-zk/sig/v1/k", kparts, 2);
        h51::encode(o, dh_host_mul(k, B));
        sc c = host_wide("rofl-zk/sig/v1/c", cparts, 3);
        sc s = sc_add(k, sc_montmul(sc_to_mont(c), keys[a]));
        sc_tobytes(o + 32, s);
        dh_wipe(&k, sizeof k); dh_wipe(&c, sizeof c); dh_wipe(&s, sizeof s);
    }
    if (pk_out32) memcpy(pk_out32, pk.data(), n_keys * 32);
    dh_wipe(keys.data(), keys.size() * sizeof(sc)); dh_wipe(can.data(), can.size());
    return ROFL_OK;
}
int rofl_dbg_host_sig_verify(size_t n_keys, const uint8_t *pk32, size_t n_msgs, const uint8_t *msg_bytes, const uint64_t *msg_off, size_t n, const rofl_sig_ref_t *refs,
                             const uint8_t *sig64, uint8_t *verdict_out) {
    bool done; size_t total;
    if (int rc = sig_check(false, n_keys, pk32, n_msgs, msg_bytes, msg_off, n, refs, sig64, verdict_out, &total, &done)) return rc;
    if (done) return ROFL_OK;
    const h51::ge5 B = host_base();
    std::vector<uint8_t> dig(n_msgs * 32), refused;
    std::vector<h51::ge5> kp;
    for (size_t j = 0; j < n_msgs; j++) sig_host_digest(dig.data() + 32 * j, msg_bytes + msg_off[j], msg_off[j + 1] - msg_off[j]);
    host_decode_keys(n_keys, pk32, refused, kp);
    for (size_t i = 0; i < n; i++) {
        const size_t a = refs ? refs[i].key : i, b = refs ? refs[i].msg : i;
        const uint8_t *sg = sig64 + 64 * i;
        const sc s = sc_frombytes(sg + 32);
        if (refused[a] || sc_geq_l(s.v)) { verdict_out[i] = 2; continue; }
        const uint8_t *cparts[3] = {sg, pk32 + 32 * a, dig.data() + 32 * b};
        const sc c = host_wide("rofl-zk/sig/v1/c", cparts, 3);
        uint8_t enc[32];
        h51::encode(enc, h51::gadd(dh_host_mul(s, B), dh_host_mul(sc_neg(c), kp[a])));
        verdict_out[i] = memcmp(enc, sg, 32) == 0 ? 0 : 1;
    }
    return ROFL_OK;
}
// ---- sealed shares: RFC 8439 ChaCha20-Poly1305 under pairwise keys on the share bundles a server relays (k_aead_derive, k_aead_seal / k_aead_open) ----
}  // extern "C"
namespace {
// one packed byte string of a call: offsets that start at 0 and do not decrease, a total within `max_total`; what: "AD" / "payload" / "record"
int aead_check_off(const char *what, size_t n, const uint64_t *off, const uint8_t *bytes, uint64_t max_one, uint64_t max_total, size_t *total) {
    char buf[128];
    if (off[0] != 0) { snprintf(buf, sizeof buf, "the first %s offset is 0", what); return fail(ROFL_BAD_PARAM, buf); }
    for (size_t i = 0; i < n; i++) {
        if (off[i + 1] < off[i]) { snprintf(buf, sizeof buf, "%s offset %zu is below the one before it", what, i + 1); return fail(ROFL_BAD_PARAM, buf); }
        if (off[i + 1] - off[i] > max_one) { snprintf(buf, sizeof buf, "%s %zu is longer than 2^24 bytes", what, i); return fail(ROFL_BAD_PARAM, buf); }
        if (off[i + 1] > max_total) { snprintf(buf, sizeof buf, "more than 2^30 %s bytes in one call (at %s %zu)", what, what, i); return fail(ROFL_BAD_PARAM, buf); }
    }
    *total = (size_t)off[n];
    if (*total && !bytes) { snprintf(buf, sizeof buf, "a null pointer: the %s bytes", what); return fail(ROFL_BAD_PARAM, buf); }
    return ROFL_OK;
}
// every check of rofl_aead_seal / rofl_aead_open, shared with their host routes.  data / data_off: the payloads (seal) or the sealed records
// (open), whose lengths are 16 more; out: what the call writes; *done: the call is empty and returns 0.  Texts name indices, never bytes.
int aead_check(bool seal, size_t n_keys, const uint8_t *key32, size_t n, const uint32_t *key_idx, const uint8_t *nonce12, const uint8_t *ad_bytes, const uint64_t *ad_off,
               const uint8_t *data, const uint64_t *data_off, const uint8_t *out, const uint8_t *verdict, size_t *ad_total, size_t *data_total, bool *done) {
    *done = n == 0; *ad_total = *data_total = 0;
    if (*done) return ROFL_OK;
    if (n > ((size_t)1 << 24)) return fail(ROFL_BAD_PARAM, "more than 2^24 records in one call");
    if (n_keys > ((size_t)1 << 24)) return fail(ROFL_BAD_PARAM, "more than 2^24 keys in one call");
    if (n_keys == 0) return fail(ROFL_BAD_PARAM, "records without keys");
    if (!key32) return fail(ROFL_BAD_PARAM, "a null pointer: the keys");
    if (!nonce12) return fail(ROFL_BAD_PARAM, "a null pointer: the nonces");
    if (!ad_off) return fail(ROFL_BAD_PARAM, "a null pointer: the AD offsets");
    if (!data_off) return fail(ROFL_BAD_PARAM, seal ? "a null pointer: the payload offsets" : "a null pointer: the record offsets");
    if (!seal && !verdict) return fail(ROFL_BAD_PARAM, "a null pointer: the verdicts");
    if (!key_idx && n_keys != n) return fail(ROFL_BAD_PARAM, "without a key index list n_keys is n");
    if (key_idx) for (size_t i = 0; i < n; i++)
        if (key_idx[i] >= n_keys) { char buf[96]; snprintf(buf, sizeof buf, "record %zu names a key that is not in the call", i); return fail(ROFL_BAD_PARAM, buf); }
    const uint64_t tagged = seal ? 0 : 16;      // a sealed record carries its tag
    if (int rc = aead_check_off("AD", n, ad_off, ad_bytes, ~(uint64_t)0, (uint64_t)1 << 30, ad_total)) return rc;
    if (int rc = aead_check_off(seal ? "payload" : "record", n, data_off, data, ((uint64_t)1 << 24) + tagged, ((uint64_t)1 << 30) + tagged * n, data_total)) return rc;
    if (!out && (seal || *data_total)) return fail(ROFL_BAD_PARAM, "a null pointer: the output");
    return ROFL_OK;
}
// the key of a call's row: the row itself, or SHAKE256("rofl-zk/seal/v1\0" || row || u64le(round))[0 .. 32) on the host's sponge
void aead_host_key(uint32_t key[8], const uint8_t *row, const uint64_t *derive_round) {
    if (!derive_round) { memcpy(key, row, 32); return; }
    uint8_t m[56] = {'r', 'o', 'f', 'l', '-', 'z', 'k', '/', 's', 'e', 'a', 'l', '/', 'v', '1', 0};
    memcpy(m + 16, row, 32); memcpy(m + 48, derive_round, 8);
    Sponge sp(136, 0x1F); sp.absorb(m, sizeof m); sp.squeeze(reinterpret_cast<uint8_t *>(key), 32);
    dh_wipe(m, sizeof m); dh_wipe(&sp, sizeof sp);
}
// `len` bytes into the authenticator, the last block padded with zeros to sixteen bytes (every block full: the AEAD's framing)
void aead_host_absorb(poly1305 &P, const uint8_t *p, uint64_t len) {
    for (uint64_t pos = 0; pos < len; pos += 16) {
        uint32_t m[4] = {0, 0, 0, 0};
        memcpy(m, p + pos, (size_t)std::min<uint64_t>(16, len - pos));
        poly1305_block(P, m, 1);
    }
}
// block 0 -> the authenticator's key; then the tag over AD and CT
void aead_host_tag(uint32_t tag[4], const uint32_t key[8], const uint32_t nc[3], const uint8_t *ad, uint64_t alen, const uint8_t *ct, uint64_t len) {
    uint32_t ks[16];
    chacha20_block(ks, key, 0, nc);
    poly1305 P; poly1305_init(P, ks);
    aead_host_absorb(P, ad, alen); aead_host_absorb(P, ct, len);
    const uint32_t m[4] = {(uint32_t)alen, (uint32_t)(alen >> 32), (uint32_t)len, (uint32_t)(len >> 32)};
    poly1305_block(P, m, 1);
    poly1305_finish(tag, P, ks + 4);
    dh_wipe(ks, sizeof ks); dh_wipe(&P, sizeof P);
}
// dst = src ^ ChaCha20 keystream from block 1
void aead_host_xor(uint8_t *dst, const uint8_t *src, uint64_t len, const uint32_t key[8], const uint32_t nc[3]) {
    uint32_t ks[16];
    for (uint64_t b = 0; b < len; b += 64) {
        chacha20_block(ks, key, 1u + (uint32_t)(b >> 6), nc);
        const uint8_t *k = reinterpret_cast<const uint8_t *>(ks);
        for (uint64_t q = 0; q < 64 && b + q < len; q++) dst[b + q] = src[b + q] ^ k[q];
    }
    dh_wipe(ks, sizeof ks);
}
// the upload both calls make: [keys | payloads or records | ADs | nonces | AD offsets | data offsets | key indices]; the keys are secret, and
// with `data_secret` the payloads behind them as well
struct AeadParts { InPart keys, data, ad, nonce, ad_off, data_off, idx; };
AeadParts aead_parts(StagedCall &st, bool data_secret, size_t n_keys, const uint8_t *key32, size_t n, const uint32_t *key_idx, const uint8_t *nonce12, const uint8_t *ad_bytes,
                     const uint64_t *ad_off, size_t ad_total, const uint8_t *data, const uint64_t *data_off, size_t data_total) {
    AeadParts p;
    p.keys = st.in(key32, n_keys * 32, kSecret); p.data = st.in(data, data_total, kPadded | (data_secret ? kSecret : 0)); p.ad = st.in(ad_bytes, ad_total, kPadded);
    p.nonce = st.in(nonce12, n * 12); p.ad_off = st.in(ad_off, (n + 1) * 8); p.data_off = st.in(data_off, (n + 1) * 8); p.idx = st.in(key_idx, n * 4);
    return p;
}
// ... and the key derivation where asked for: in place, so the derived keys are wiped with the rows
void aead_upload(StagedCall &st, const AeadParts &p, size_t n_keys, const uint64_t *derive_round) {
    st.upload();
    if (derive_round) ROFL_LAUNCH(k_aead_derive, per_item(n_keys), dim3(64), 0, st.C.stream, (u32)n_keys, (u64)*derive_round, const_cast<u64 *>(st.dev<u64>(p.keys)));
}
// a packed list of messages for the Poly1305 hooks
int poly_check(size_t n, const uint8_t *key32, const uint8_t *msg_bytes, const uint64_t *msg_off, const uint8_t *tag_out16, size_t *total, bool *done) {
    *done = n == 0; *total = 0;
    if (*done) return ROFL_OK;
    if (!key32 || !msg_off || !tag_out16) return fail(ROFL_BAD_PARAM, "bad parameter");
    if (n > ((size_t)1 << 20)) return fail(ROFL_BAD_PARAM, "more than 2^20 messages in one call");
    return aead_check_off("message", n, msg_off, msg_bytes, (uint64_t)1 << 24, (uint64_t)1 << 30, total);
}
}  // namespace
extern "C" {
// The lane's copies of the keys (as given and derived) and of the plaintexts -- pinned staging and device workspace -- are overwritten with
// zeros before the call returns or unwinds; keystream and authenticator keys live in registers only.  The sealed records are public.
int rofl_aead_seal(size_t n_keys, const uint8_t *key32, const uint64_t *derive_round, size_t n, const uint32_t *key_idx, const uint8_t *nonce12,
                   const uint8_t *ad_bytes, const uint64_t *ad_off, const uint8_t *pt_bytes, const uint64_t *pt_off, uint8_t *sealed_out) {
    bool done; size_t ad_total, pt_total;
    if (int rc = aead_check(true, n_keys, key32, n, key_idx, nonce12, ad_bytes, ad_off, pt_bytes, pt_off, sealed_out, nullptr, &ad_total, &pt_total, &done)) return rc;
    if (done) return ROFL_OK;
    return guarded([&]() -> int {
        StagedCall st; Ctx &C = st.C;
        const AeadParts p = aead_parts(st, true, n_keys, key32, n, key_idx, nonce12, ad_bytes, ad_off, ad_total, pt_bytes, pt_off, pt_total);
        const OutPart sealed = st.out(sealed_out, pt_total + 16 * n);
        aead_upload(st, p, n_keys, derive_round);
        ROFL_LAUNCH(k_aead_seal, per_item(n), dim3(64), 0, C.stream, (u32)n, st.dev<u32>(p.idx), st.dev<u32>(p.keys), st.dev<u32>(p.nonce), st.dev<uint8_t>(p.ad), st.dev<u64>(p.ad_off),
                    st.dev<uint8_t>(p.data), st.dev<u64>(p.data_off), st.dev<uint8_t>(sealed));
        st.finish();
        return ROFL_OK;
    });
}
// the keys in the upload and the plaintexts in the download are wiped the same way; records, ADs, nonces and verdicts are public
int rofl_aead_open(size_t n_keys, const uint8_t *key32, const uint64_t *derive_round, size_t n, const uint32_t *key_idx, const uint8_t *nonce12,
                   const uint8_t *ad_bytes, const uint64_t *ad_off, const uint8_t *sealed_bytes, const uint64_t *sealed_off, uint8_t *pt_out, uint8_t *verdict_out) {
    bool done; size_t ad_total, s_total;
    if (int rc = aead_check(false, n_keys, key32, n, key_idx, nonce12, ad_bytes, ad_off, sealed_bytes, sealed_off, pt_out, verdict_out, &ad_total, &s_total, &done)) return rc;
    if (done) return ROFL_OK;
    return guarded([&]() -> int {
        StagedCall st; Ctx &C = st.C;
        const AeadParts p = aead_parts(st, false, n_keys, key32, n, key_idx, nonce12, ad_bytes, ad_off, ad_total, sealed_bytes, sealed_off, s_total);
        const OutPart pt = st.out(nullptr, s_total, kSecret), verdict = st.out(verdict_out, n);      // the plaintexts laid out like the records: delivered below
        aead_upload(st, p, n_keys, derive_round);
        ROFL_LAUNCH(k_aead_open, per_item(n), dim3(64), 0, C.stream, (u32)n, st.dev<u32>(p.idx), st.dev<u32>(p.keys), st.dev<u32>(p.nonce), st.dev<uint8_t>(p.ad), st.dev<u64>(p.ad_off),
                    st.dev<uint8_t>(p.data), st.dev<u64>(p.data_off), st.dev<uint8_t>(pt), st.dev<uint8_t>(verdict));
        st.finish();
        const uint8_t *hp = st.host(pt);
        for (size_t i = 0; i < n; i++)      // a record shorter than its tag writes nothing; the 16 bytes after a plaintext are not the library's
            if (verdict_out[i] != 2 && sealed_off[i + 1] - sealed_off[i] > 16) memcpy(pt_out + sealed_off[i], hp + sealed_off[i], (size_t)(sealed_off[i + 1] - sealed_off[i] - 16));
        return ROFL_OK;
    });
}
// the two calls in plain C++ on one thread, no GPU: same parameters, same checks, same bytes
int rofl_dbg_host_aead_seal(size_t n_keys, const uint8_t *key32, const uint64_t *derive_round, size_t n, const uint32_t *key_idx, const uint8_t *nonce12,
                            const uint8_t *ad_bytes, const uint64_t *ad_off, const uint8_t *pt_bytes, const uint64_t *pt_off, uint8_t *sealed_out) {
    bool done; size_t ad_total, pt_total;
    if (int rc = aead_check(true, n_keys, key32, n, key_idx, nonce12, ad_bytes, ad_off, pt_bytes, pt_off, sealed_out, nullptr, &ad_total, &pt_total, &done)) return rc;
    if (done) return ROFL_OK;
    std::vector<uint32_t> keys(n_keys * 8);
    for (size_t a = 0; a < n_keys; a++) aead_host_key(keys.data() + 8 * a, key32 + 32 * a, derive_round);
    for (size_t i = 0; i < n; i++) {
        const uint32_t *key = keys.data() + 8 * (key_idx ? key_idx[i] : i);
        const uint64_t len = pt_off[i + 1] - pt_off[i], alen = ad_off[i + 1] - ad_off[i];
        uint32_t nc[3], tag[4];
        memcpy(nc, nonce12 + 12 * i, 12);
        uint8_t *o = sealed_out + pt_off[i] + 16 * i;
        aead_host_xor(o, pt_bytes + pt_off[i], len, key, nc);
        aead_host_tag(tag, key, nc, ad_bytes + ad_off[i], alen, o, len);
        memcpy(o + len, tag, 16);
    }
    dh_wipe(keys.data(), keys.size() * 4);
    return ROFL_OK;
}
int rofl_dbg_host_aead_open(size_t n_keys, const uint8_t *key32, const uint64_t *derive_round, size_t n, const uint32_t *key_idx, const uint8_t *nonce12,
                            const uint8_t *ad_bytes, const uint64_t *ad_off, const uint8_t *sealed_bytes, const uint64_t *sealed_off, uint8_t *pt_out, uint8_t *verdict_out) {
    bool done; size_t ad_total, s_total;
    if (int rc = aead_check(false, n_keys, key32, n, key_idx, nonce12, ad_bytes, ad_off, sealed_bytes, sealed_off, pt_out, verdict_out, &ad_total, &s_total, &done)) return rc;
    if (done) return ROFL_OK;
    std::vector<uint32_t> keys(n_keys * 8);
    for (size_t a = 0; a < n_keys; a++) aead_host_key(keys.data() + 8 * a, key32 + 32 * a, derive_round);
    for (size_t i = 0; i < n; i++) {
        const uint64_t rlen = sealed_off[i + 1] - sealed_off[i], alen = ad_off[i + 1] - ad_off[i];
        if (rlen < 16) { verdict_out[i] = 2; continue; }
        const uint32_t *key = keys.data() + 8 * (key_idx ? key_idx[i] : i);
        const uint8_t *ct = sealed_bytes + sealed_off[i];
        uint32_t nc[3], tag[4];
        memcpy(nc, nonce12 + 12 * i, 12);
        aead_host_tag(tag, key, nc, ad_bytes + ad_off[i], alen, ct, rlen - 16);      // the tag over the ciphertext first
        verdict_out[i] = memcmp(tag, ct + rlen - 16, 16) == 0 ? 0 : 1;
        if (verdict_out[i]) { if (rlen > 16) memset(pt_out + sealed_off[i], 0, (size_t)(rlen - 16)); }
        else aead_host_xor(pt_out + sealed_off[i], ct, rlen - 16, key, nc);
    }
    dh_wipe(keys.data(), keys.size() * 4);
    return ROFL_OK;
}
// Poly1305 of n messages under n keys r || s through the kernels' own device functions (k_dbg_poly1305, one thread per message)
int rofl_dbg_poly1305(size_t n, const uint8_t *key32, const uint8_t *msg_bytes, const uint64_t *msg_off, uint8_t *tag_out16) {
    bool done; size_t total;
    if (int rc = poly_check(n, key32, msg_bytes, msg_off, tag_out16, &total, &done)) return rc;
    if (done) return ROFL_OK;
    return guarded([&]() -> int {
        StagedCall st; Ctx &C = st.C;
        const InPart keys = st.in(key32, n * 32), off = st.in(msg_off, (n + 1) * 8), msg = st.in(msg_bytes, total, kPadded);
        const OutPart tags = st.out(tag_out16, n * 16);
        st.upload();
        ROFL_LAUNCH(k_dbg_poly1305, per_item(n), dim3(64), 0, C.stream, (u32)n, st.dev<u32>(keys), st.dev<uint8_t>(msg), st.dev<u64>(off), st.dev<u32>(tags));
        st.finish();
        return ROFL_OK;
    });
}
int rofl_dbg_host_poly1305(size_t n, const uint8_t *key32, const uint8_t *msg_bytes, const uint64_t *msg_off, uint8_t *tag_out16) {
    bool done; size_t total;
    if (int rc = poly_check(n, key32, msg_bytes, msg_off, tag_out16, &total, &done)) return rc;
    if (done) return ROFL_OK;
    for (size_t j = 0; j < n; j++) {
        uint32_t k[8], m[4], tag[4];
        memcpy(k, key32 + 32 * j, 32);
        poly1305 P; poly1305_init(P, k);
        const uint8_t *p = msg_bytes + msg_off[j];
        const uint64_t len = msg_off[j + 1] - msg_off[j], full = len & ~(uint64_t)15;
        for (uint64_t pos = 0; pos < full; pos += 16) { memcpy(m, p + pos, 16); poly1305_block(P, m, 1); }
        if (len & 15) {
            uint8_t last[16] = {0};
            memcpy(last, p + full, (size_t)(len & 15)); last[len & 15] = 1;
            memcpy(m, last, 16); poly1305_block(P, m, 0);
        }
        poly1305_finish(tag, P, k + 4);
        memcpy(tag_out16 + 16 * j, tag, 16);
    }
    return ROFL_OK;
}
// ---- complaints: a DLEQ proof opens one pair's sealed channel to a judge (k_dh_public / k_dh_decode, k_dleq_prove / k_dleq_verify) ----
}  // extern "C"
namespace {
// every check of rofl_dleq_prove / rofl_dleq_verify, shared with their host routes: those of rofl_dh_shared.  own32: secret keys (prove) or
// public keys (verify); out: status or verdict bytes; *done: the call is empty and returns 0
int dleq_check(bool prove, size_t n_own, const uint8_t *own32, size_t n_peer, const uint8_t *peer_pk32, size_t n_pairs, const rofl_dh_pair_t *pairs, const uint8_t *ctx32,
               const uint8_t *reveal32, const uint8_t *proof64, const uint8_t *out, bool *done) {
    *done = n_pairs == 0;
    if (*done) return ROFL_OK;
    if (!own32 || !peer_pk32 || !ctx32 || !reveal32 || !proof64 || !out) return fail(ROFL_BAD_PARAM, "bad parameter");
    if (int rc = dh_check_pairs(n_own, n_peer, n_pairs, pairs)) return rc;
    return prove ? dh_check_keys(n_own, own32) : ROFL_OK;
}
// the driver of the two debug hooks below: one upload, one launch, one download; *kernel_ms (may be NULL) is the launch between two events
int dbg_var_mul_device(bool joint, size_t n, const uint8_t *k1_32, const uint8_t *p1_32, const uint8_t *k2_32, const uint8_t *p2_32, uint8_t *out32, double *kernel_ms) {
    if (n == 0) return ROFL_OK;
    if (!k1_32 || !p1_32 || !k2_32 || !p2_32 || !out32) return fail(ROFL_BAD_PARAM, "bad parameter");
    if (n > ((size_t)1 << 24)) return fail(ROFL_BAD_PARAM, "more than 2^24 items in one call");
    return guarded([&]() -> int {
        StagedCall st; Ctx &C = st.C;
        const InPart k1 = st.in(k1_32, n * 32), p1 = st.in(p1_32, n * 32), k2 = st.in(k2_32, n * 32), p2 = st.in(p2_32, n * 32);
        const OutPart out = st.out(out32, n * 32);
        st.upload();
        hipEvent_t e0 = nullptr, e1 = nullptr;
        if (kernel_ms) { HIPCHK(hipEventCreate(&e0)); HIPCHK(hipEventCreate(&e1)); HIPCHK(hipEventRecord(e0, C.stream)); }
        if (joint) ROFL_LAUNCH(k_dbg_var_mul2, per_item(n), dim3(64), 0, C.stream, (u32)n, st.dev<sc>(k1), st.dev<uint8_t>(p1), st.dev<sc>(k2), st.dev<uint8_t>(p2), st.dev<uint8_t>(out));
        else ROFL_LAUNCH(k_dbg_var_mul_sum, per_item(n), dim3(64), 0, C.stream, (u32)n, st.dev<sc>(k1), st.dev<uint8_t>(p1), st.dev<sc>(k2), st.dev<uint8_t>(p2), st.dev<uint8_t>(out));
        if (kernel_ms) HIPCHK(hipEventRecord(e1, C.stream));
        st.finish();
        if (kernel_ms) { float ms = 0; HIPCHK(hipEventElapsedTime(&ms, e0, e1)); *kernel_ms = ms; (void)hipEventDestroy(e0); (void)hipEventDestroy(e1); }
        return ROFL_OK;
    });
}
}  // namespace
extern "C" {
// The lane's copies of the secret keys -- pinned staging and device workspace -- are overwritten with zeros before the call returns or
// unwinds; the nonces never leave their threads' registers; reveals and proofs are what the caller publishes.
int rofl_dleq_prove(size_t n_own, const uint8_t *sk32, uint8_t *own_pk_out32, size_t n_peer, const uint8_t *peer_pk32, size_t n_pairs, const rofl_dh_pair_t *pairs,
                    const uint8_t *ctx32, uint8_t *reveal_out32, uint8_t *proof_out64, uint8_t *status_out) {
    bool done;
    if (int rc = dleq_check(true, n_own, sk32, n_peer, peer_pk32, n_pairs, pairs, ctx32, reveal_out32, proof_out64, status_out, &done)) return rc;
    if (done) return ROFL_OK;
    return guarded([&]() -> int {
        StagedCall st; Ctx &C = st.C;
        const InPart keys = st.in(sk32, n_own * 32, kSecret), peer = st.in(peer_pk32, n_peer * 32), cx = st.in(ctx32, n_pairs * 32), pl = st.in(pairs, n_pairs * sizeof(rofl_dh_pair_t));
        const OutPart reveal = st.out(reveal_out32, n_pairs * 32), proof = st.out(proof_out64, n_pairs * 64), pk = st.out(own_pk_out32, n_own * 32), status = st.out(status_out, n_pairs);
        ge *pts = C.aux_pts.as<ge>(n_peer); u32 *pst = C.status.as<u32>(n_peer);
        st.upload();
        ROFL_LAUNCH(k_dh_public, per_item(n_own), dim3(64), 0, C.stream, (u32)n_own, st.dev<sc>(keys), C.d_tabB8, st.dev<uint8_t>(pk));
        ROFL_LAUNCH(k_dh_decode, per_item(n_peer), dim3(64), 0, C.stream, (u32)n_peer, st.dev<uint8_t>(peer), pts, pst);
        ROFL_LAUNCH(k_dleq_prove, per_item(n_pairs), dim3(64), 0, C.stream, (u32)n_pairs, (u32)n_peer, st.dev<uint2>(pl), st.dev<sc>(keys), (const uint8_t *)st.dev<uint8_t>(pk),
                    st.dev<uint8_t>(peer), (const ge *)pts, (const u32 *)pst, st.dev<uint8_t>(cx), C.d_tabB8, st.dev<uint8_t>(reveal), st.dev<uint8_t>(proof), st.dev<uint8_t>(status));
        st.finish();
        return ROFL_OK;
    });
}
// The inputs are public; the shared secrets that come back open the pair's channel, so the lane's copies of them are overwritten with zeros.
int rofl_dleq_verify(size_t n_own, const uint8_t *own_pk32, size_t n_peer, const uint8_t *peer_pk32, size_t n_pairs, const rofl_dh_pair_t *pairs, const uint8_t *ctx32,
                     const uint8_t *reveal32, const uint8_t *proof64, uint8_t *shared_out32, uint8_t *verdict_out) {
    bool done;
    if (int rc = dleq_check(false, n_own, own_pk32, n_peer, peer_pk32, n_pairs, pairs, ctx32, reveal32, proof64, verdict_out, &done)) return rc;
    if (done) return ROFL_OK;
    return guarded([&]() -> int {
        StagedCall st; Ctx &C = st.C;
        const size_t n_keys = n_own + n_peer;
        const InPart own = st.in(own_pk32, n_own * 32), peer = st.in(peer_pk32, n_peer * 32), cx = st.in(ctx32, n_pairs * 32), reveal = st.in(reveal32, n_pairs * 32),
                     proof = st.in(proof64, n_pairs * 64), pl = st.in(pairs, n_pairs * sizeof(rofl_dh_pair_t));
        const OutPart shared = st.out(shared_out32, shared_out32 ? n_pairs * 32 : 0, kSecret), verdict = st.out(verdict_out, n_pairs);
        ge *pts = C.aux_pts.as<ge>(n_keys); u32 *pst = C.status.as<u32>(n_keys);
        st.upload();
        ROFL_LAUNCH(k_dh_decode, per_item(n_keys), dim3(64), 0, C.stream, (u32)n_keys, st.dev<uint8_t>(own), pts, pst);      // ONE launch decodes both key tables: the peer keys follow the prover keys
        ROFL_LAUNCH(k_dleq_verify, per_item(n_pairs), dim3(64), 0, C.stream, (u32)n_pairs, (u32)n_peer, st.dev<uint2>(pl), st.dev<uint8_t>(own), (const ge *)pts, (const u32 *)pst,
                    st.dev<uint8_t>(peer), (const ge *)(pts + n_own), (const u32 *)(pst + n_own), st.dev<uint8_t>(cx), st.dev<uint8_t>(reveal), st.dev<uint8_t>(proof), C.d_tabB8,
                    shared_out32 ? st.dev<uint8_t>(shared) : (uint8_t *)nullptr, st.dev<uint8_t>(verdict));
        st.finish();
        return ROFL_OK;
    });
}
// the two calls on the host's 51-bit point arithmetic, scalar arithmetic and host Keccak, one thread, no GPU: same parameters, same checks, same bytes
int rofl_dbg_host_dleq_prove(size_t n_own, const uint8_t *sk32, uint8_t *own_pk_out32, size_t n_peer, const uint8_t *peer_pk32, size_t n_pairs, const rofl_dh_pair_t *pairs,
                             const uint8_t *ctx32, uint8_t *reveal_out32, uint8_t *proof_out64, uint8_t *status_out) {
    bool done;
    if (int rc = dleq_check(true, n_own, sk32, n_peer, peer_pk32, n_pairs, pairs, ctx32, reveal_out32, proof_out64, status_out, &done)) return rc;
    if (done) return ROFL_OK;
    std::vector<uint8_t> pk, can, refused;
    std::vector<sc> keys;
    std::vector<h51::ge5> pp;
    const h51::ge5 B = host_own_keys(n_own, sk32, keys, can, pk);
    host_decode_keys(n_peer, peer_pk32, refused, pp);
    for (size_t i = 0; i < n_pairs; i++) {
        const size_t a = pairs ? pairs[i].own : i / n_peer, b = pairs ? pairs[i].peer : i % n_peer;
        uint8_t *S = reveal_out32 + 32 * i, *pf = proof_out64 + 64 * i, T1[32], T2[32];
        status_out[i] = refused[b];
        if (refused[b]) { memset(S, 0, 32); memset(pf, 0, 64); continue; }
        const uint8_t *P = peer_pk32 + 32 * b, *cx = ctx32 + 32 * i;
        const uint8_t *kparts[3] = {can.data() + 32 * a, P, cx};
        sc k = host_wide("rofl-zk/dleq/v1k", kparts, 3);
        h51::encode(S, dh_host_mul(keys[a], pp[b]));
        h51::encode(T1, dh_host_mul(k, B));
        h51::encode(T2, dh_host_mul(k, pp[b]));
        const uint8_t *cparts[6] = {pk.data() + 32 * a, P, S, T1, T2, cx};
        sc c = host_wide("rofl-zk/dleq/v1c", cparts, 6);
        sc s = sc_add(k, sc_montmul(sc_to_mont(c), keys[a]));
        sc_tobytes(pf, c); sc_tobytes(pf + 32, s);
        dh_wipe(&k, sizeof k); dh_wipe(&c, sizeof c); dh_wipe(&s, sizeof s);
    }
    if (own_pk_out32) memcpy(own_pk_out32, pk.data(), n_own * 32);
    dh_wipe(keys.data(), keys.size() * sizeof(sc)); dh_wipe(can.data(), can.size());
    return ROFL_OK;
}
int rofl_dbg_host_dleq_verify(size_t n_own, const uint8_t *own_pk32, size_t n_peer, const uint8_t *peer_pk32, size_t n_pairs, const rofl_dh_pair_t *pairs, const uint8_t *ctx32,
                              const uint8_t *reveal32, const uint8_t *proof64, uint8_t *shared_out32, uint8_t *verdict_out) {
    bool done;
    if (int rc = dleq_check(false, n_own, own_pk32, n_peer, peer_pk32, n_pairs, pairs, ctx32, reveal32, proof64, verdict_out, &done)) return rc;
    if (done) return ROFL_OK;
    const h51::ge5 B = host_base();
    std::vector<uint8_t> own_refused, peer_refused;
    std::vector<h51::ge5> op, pp;
    host_decode_keys(n_own, own_pk32, own_refused, op);
    host_decode_keys(n_peer, peer_pk32, peer_refused, pp);
    for (size_t i = 0; i < n_pairs; i++) {
        const size_t a = pairs ? pairs[i].own : i / n_peer, b = pairs ? pairs[i].peer : i % n_peer;
        const uint8_t *S = reveal32 + 32 * i, *pf = proof64 + 64 * i, *A = own_pk32 + 32 * a, *P = peer_pk32 + 32 * b, *cx = ctx32 + 32 * i;
        if (shared_out32) memset(shared_out32 + 32 * i, 0, 32);
        const sc c = sc_frombytes(pf), s = sc_frombytes(pf + 32);
        ge Sg;
        if (own_refused[a] || peer_refused[b] || sc_geq_l(c.v) || sc_geq_l(s.v) || !ristretto_decode(Sg, S) || ge_is_identity_ristretto(Sg)) { verdict_out[i] = 2; continue; }
        const sc nc = sc_neg(c);
        uint8_t T1[32], T2[32], c2[32];
        h51::encode(T1, h51::gadd(dh_host_mul(s, B), dh_host_mul(nc, op[a])));
        h51::encode(T2, h51::gadd(dh_host_mul(s, pp[b]), dh_host_mul(nc, h51::from_ge(Sg))));
        const uint8_t *cparts[6] = {A, P, S, T1, T2, cx};
        sc_tobytes(c2, host_wide("rofl-zk/dleq/v1c", cparts, 6));
        verdict_out[i] = memcmp(c2, pf, 32) == 0 ? 0 : 1;
        if (verdict_out[i] == 0 && shared_out32) dh_host_secret(shared_out32 + 32 * i, S, A, P);
    }
    return ROFL_OK;
}
// out32[i] = encode(k1[i] decode(p1[i]) + k2[i] decode(p2[i])) through the kernels' own device functions, one thread per item: on the joint
// chain sg_var_mul2 (rofl_dbg_var_mul2) and as gd_add(sg_var_mul, sg_var_mul) (rofl_dbg_var_mul_sum)
int rofl_dbg_var_mul2(size_t n, const uint8_t *k1_32, const uint8_t *p1_32, const uint8_t *k2_32, const uint8_t *p2_32, uint8_t *out32, double *kernel_ms) {
    return dbg_var_mul_device(true, n, k1_32, p1_32, k2_32, p2_32, out32, kernel_ms);
}
int rofl_dbg_var_mul_sum(size_t n, const uint8_t *k1_32, const uint8_t *p1_32, const uint8_t *k2_32, const uint8_t *p2_32, uint8_t *out32, double *kernel_ms) {
    return dbg_var_mul_device(false, n, k1_32, p1_32, k2_32, p2_32, out32, kernel_ms);
}
// ---- Merkle trees: a round's broadcast behind one root, single entries proved by a path (k_mt_leaves, k_mt_tile, k_mt_paths / k_mt_climb) ----
}  // extern "C"
namespace {
u32 mt_depth(size_t n) { u32 d = 0; while (((size_t)1 << d) < n) d++; return d; }      // bit_length(n - 1)
// every check of rofl_merkle_build, shared with its host route; *done: the call is empty and returns 0.  *total: the bytes behind msg_bytes
int merkle_build_check(size_t n, const uint8_t *msg_bytes, const uint64_t *msg_off, const uint8_t *root_out32, size_t n_paths, const uint32_t *path_idx,
                       const uint8_t *paths_out32, size_t *total, bool *done) {
    *done = n == 0 && n_paths == 0; *total = 0;
    if (*done) return ROFL_OK;
    if (n == 0) return fail(ROFL_BAD_PARAM, "paths of a tree without leaves");
    if (!root_out32 || (!msg_off && !msg_bytes)) return fail(ROFL_BAD_PARAM, "bad parameter");
    if (n > ((size_t)1 << 20)) return fail(ROFL_BAD_PARAM, "more than 2^20 leaves in one call");
    if (msg_off) { if (int rc = msg_off_check(n, msg_bytes, msg_off, total)) return rc; }
    else *total = n * 32;
    const size_t depth = mt_depth(n);
    if (n_paths > ((size_t)1 << 24)) return fail(ROFL_BAD_PARAM, "more than 2^24 paths in one call");
    if (n_paths * depth * 32 > ((size_t)1 << 30)) return fail(ROFL_BAD_PARAM, "more than 2^30 path bytes in one call");
    if (n_paths && (!path_idx || (depth && !paths_out32))) return fail(ROFL_BAD_PARAM, "bad parameter");
    for (size_t i = 0; i < n_paths; i++)
        if (path_idx[i] >= n) { char buf[96]; snprintf(buf, sizeof buf, "path %zu names a leaf that is not in the tree", i); return fail(ROFL_BAD_PARAM, buf); }
    return ROFL_OK;
}
// every check of rofl_merkle_verify, shared with its host route.  An index >= its root's leaf count is no parameter error: it is verdict 2
int merkle_verify_check(size_t n_roots, const uint8_t *root32, const uint32_t *n_leaves, size_t n_paths, const rofl_merkle_ref_t *refs, const uint8_t *msg_bytes,
                        const uint64_t *msg_off, const uint8_t *paths32, size_t stride, const uint8_t *verdict_out, size_t *total, bool *done) {
    *done = n_paths == 0; *total = 0;
    if (*done) return ROFL_OK;
    if (!root32 || !n_leaves || !verdict_out || (!msg_off && !msg_bytes) || (stride && !paths32)) return fail(ROFL_BAD_PARAM, "bad parameter");
    if (n_roots == 0) return fail(ROFL_BAD_PARAM, "paths without roots");
    if (n_roots > ((size_t)1 << 20)) return fail(ROFL_BAD_PARAM, "more than 2^20 roots in one call");
    if (n_paths > ((size_t)1 << 24)) return fail(ROFL_BAD_PARAM, "more than 2^24 paths in one call");
    if (stride > 20) return fail(ROFL_BAD_PARAM, "a stride above 20");
    if (n_paths * stride * 32 > ((size_t)1 << 30)) return fail(ROFL_BAD_PARAM, "more than 2^30 path bytes in one call");
    for (size_t r = 0; r < n_roots; r++)
        if (n_leaves[r] == 0 || n_leaves[r] > (1u << 20)) { char buf[96]; snprintf(buf, sizeof buf, "the leaf count of root %zu is not in [1, 2^20]", r); return fail(ROFL_BAD_PARAM, buf); }
    if (!refs && n_roots != 1) return fail(ROFL_BAD_PARAM, "without a ref list there is one root");
    for (size_t i = 0; i < (refs ? n_paths : 1); i++) {
        const size_t r = refs ? refs[i].root : 0;
        char buf[96];
        if (r >= n_roots) { snprintf(buf, sizeof buf, "ref %zu names a root that is not in the call", i); return fail(ROFL_BAD_PARAM, buf); }
        if (stride < mt_depth(n_leaves[r])) { snprintf(buf, sizeof buf, "the stride is below the depth of root %zu", r); return fail(ROFL_BAD_PARAM, buf); }
    }
    if (msg_off) return msg_off_check(n_paths, msg_bytes, msg_off, total);
    *total = n_paths * 32;
    return ROFL_OK;
}
void mt_host_node(uint8_t out[32], const uint8_t a[32], const uint8_t b[32]) {
    uint8_t m[80];
    memcpy(m, "rofl-zk/mtr/v1/n", 16); memcpy(m + 16, a, 32); memcpy(m + 48, b, 32);
    Sponge sp(136, 0x1F); sp.absorb(m, sizeof m); sp.squeeze(out, 32);
}
void mt_host_root(uint8_t out[32], uint64_t n, const uint8_t top[32]) {
    uint8_t m[56];
    memcpy(m, "rofl-zk/mtr/v1/r", 16); memcpy(m + 16, &n, 8); memcpy(m + 24, top, 32);
    Sponge sp(136, 0x1F); sp.absorb(m, sizeof m); sp.squeeze(out, 32);
}
}  // namespace
extern "C" {
size_t rofl_dbg_merkle_tile_leaves(void) { return ROFL_MT_TILE; }
// nothing here is secret: messages, digests, roots, paths, verdicts
int rofl_merkle_build(size_t n, const uint8_t *msg_bytes, const uint64_t *msg_off, uint8_t *root_out32, uint8_t *leaves_out32, size_t n_paths, const uint32_t *path_idx,
                      uint8_t *paths_out32) {
    bool done; size_t total;
    if (int rc = merkle_build_check(n, msg_bytes, msg_off, root_out32, n_paths, path_idx, paths_out32, &total, &done)) return rc;
    if (done) return ROFL_OK;
    const u32 depth = mt_depth(n);
    const bool hashed = !msg_off;      // msg_bytes holds the leaf digests
    int rc = guarded([&]() -> int {
        StagedCall st; Ctx &C = st.C;
        const InPart off = st.in(msg_off, (n + 1) * 8), idx = st.in(path_idx, n_paths * 4), msg = hashed ? st.in(msg_bytes, total, kAlign16) : st.in(msg_bytes, total, kPadded);
        const OutPart root = st.out(root_out32, 32, kAlign16), paths = st.out(paths_out32, n_paths * depth * 32, kAlign16);
        const bool own_leaves = !hashed && !leaves_out32;      // the leaf digests stay in the workspace: nobody asked for them
        OutPart leaves{0};
        if (!hashed && leaves_out32) leaves = st.out(leaves_out32, n * 32, kAlign16);
        size_t n_nodes = 0;      // levels 1 .. depth back to back
        for (size_t w = n; w > 1;) { w = (w + 1) / 2; n_nodes += w; }
        u64 *nodes = st.work<u64>(4 * (n_nodes + (own_leaves ? n : 0)));
        st.upload();
        const u64 *lf = hashed ? st.dev<u64>(msg) : own_leaves ? nodes + 4 * n_nodes : st.dev<u64>(leaves);
        if (!hashed) ROFL_LAUNCH(k_mt_leaves, per_item(n), dim3(64), 0, C.stream, (u32)n, st.dev<uint8_t>(msg), st.dev<u64>(off), const_cast<u64 *>(lf));
        // ceil(depth / log2 T) launches (one for a single leaf): each takes the level `in` up log2 T levels, and the next starts on its tile roots
        const u64 *in = lf; u64 *out = nodes; size_t w = n;
        do {
            ROFL_LAUNCH(k_mt_tile, dim3((unsigned)((w + ROFL_MT_TILE - 1) / ROFL_MT_TILE)), dim3(ROFL_MT_TILE / 2), 0, C.stream, (u32)w, in, out, (u64)n, st.dev<u64>(root));
            for (u32 k = 0; k < ROFL_MT_TILE_LOG2 && w > 1; k++) { w = (w + 1) / 2; in = out; out += 4 * w; }
        } while (w > 1);
        if (n_paths && depth)
            ROFL_LAUNCH(k_mt_paths, grid1(n_paths * depth), dim3(TPB), 0, C.stream, (u32)(n_paths * depth), depth, (u32)n, st.dev<u32>(idx), lf, (const u64 *)nodes, st.dev<u64>(paths));
        st.finish();
        return ROFL_OK;
    });
    if (rc == ROFL_OK && hashed && leaves_out32) memcpy(leaves_out32, msg_bytes, n * 32);
    return rc;
}
int rofl_merkle_verify(size_t n_roots, const uint8_t *root32, const uint32_t *n_leaves, size_t n_paths, const rofl_merkle_ref_t *refs, const uint8_t *msg_bytes,
                       const uint64_t *msg_off, const uint8_t *paths32, size_t stride, uint8_t *verdict_out) {
    bool done; size_t total;
    if (int rc = merkle_verify_check(n_roots, root32, n_leaves, n_paths, refs, msg_bytes, msg_off, paths32, stride, verdict_out, &total, &done)) return rc;
    if (done) return ROFL_OK;
    const bool hashed = !msg_off;
    return guarded([&]() -> int {
        StagedCall st; Ctx &C = st.C;
        const InPart roots = st.in(root32, n_roots * 32), cnt = st.in(n_leaves, n_roots * 4), rf = st.in(refs, n_paths * sizeof(rofl_merkle_ref_t)), off = st.in(msg_off, (n_paths + 1) * 8),
                     pt = st.in(paths32, n_paths * stride * 32), msg = hashed ? st.in(msg_bytes, total) : st.in(msg_bytes, total, kPadded);
        const OutPart verdict = st.out(verdict_out, n_paths);
        u64 *ws = st.work<u64>(hashed ? 0 : n_paths * 4);
        st.upload();
        const u64 *dig = hashed ? st.dev<u64>(msg) : ws;
        if (!hashed) ROFL_LAUNCH(k_mt_leaves, per_item(n_paths), dim3(64), 0, C.stream, (u32)n_paths, st.dev<uint8_t>(msg), st.dev<u64>(off), ws);
        ROFL_LAUNCH(k_mt_climb, per_item(n_paths), dim3(64), 0, C.stream, (u32)n_paths, st.dev<u64>(roots), st.dev<u32>(cnt), st.dev<uint2>(rf), dig, st.dev<u64>(pt), (u32)stride,
                    st.dev<uint8_t>(verdict));
        st.finish();
        return ROFL_OK;
    });
}
// the two calls on the host's sponge, one thread, no GPU: same parameters, same checks, same bytes and verdicts
int rofl_dbg_host_merkle_build(size_t n, const uint8_t *msg_bytes, const uint64_t *msg_off, uint8_t *root_out32, uint8_t *leaves_out32, size_t n_paths, const uint32_t *path_idx,
                               uint8_t *paths_out32) {
    bool done; size_t total;
    if (int rc = merkle_build_check(n, msg_bytes, msg_off, root_out32, n_paths, path_idx, paths_out32, &total, &done)) return rc;
    if (done) return ROFL_OK;
    const u32 depth = mt_depth(n);
    std::vector<std::vector<uint8_t>> lv(depth + 1);
    lv[0].resize(n * 32);
    if (!msg_off) memcpy(lv[0].data(), msg_bytes, n * 32);
    else for (size_t j = 0; j < n; j++) host_labelled_digest(lv[0].data() + 32 * j, "rofl-zk/mtr/v1/l", msg_bytes + msg_off[j], msg_off[j + 1] - msg_off[j]);
    for (u32 l = 0; l < depth; l++) {
        const size_t w = lv[l].size() / 32, up = (w + 1) / 2;
        lv[l + 1].resize(up * 32);
        for (size_t i = 0; i < w / 2; i++) mt_host_node(lv[l + 1].data() + 32 * i, lv[l].data() + 64 * i, lv[l].data() + 64 * i + 32);
        if (w & 1) memcpy(lv[l + 1].data() + 32 * (up - 1), lv[l].data() + 32 * (w - 1), 32);
    }
    mt_host_root(root_out32, n, lv[depth].data());
    if (leaves_out32) memcpy(leaves_out32, lv[0].data(), n * 32);
    for (size_t p = 0; p < n_paths; p++)
        for (u32 l = 0; l < depth; l++) {
            const size_t sib = ((size_t)path_idx[p] >> l) ^ 1;
            uint8_t *slot = paths_out32 + (p * depth + l) * 32;
            if (sib < lv[l].size() / 32) memcpy(slot, lv[l].data() + 32 * sib, 32); else memset(slot, 0, 32);
        }
    return ROFL_OK;
}
int rofl_dbg_host_merkle_verify(size_t n_roots, const uint8_t *root32, const uint32_t *n_leaves, size_t n_paths, const rofl_merkle_ref_t *refs, const uint8_t *msg_bytes,
                                const uint64_t *msg_off, const uint8_t *paths32, size_t stride, uint8_t *verdict_out) {
    bool done; size_t total;
    if (int rc = merkle_verify_check(n_roots, root32, n_leaves, n_paths, refs, msg_bytes, msg_off, paths32, stride, verdict_out, &total, &done)) return rc;
    if (done) return ROFL_OK;
    const uint8_t zero[32] = {0};
    for (size_t i = 0; i < n_paths; i++) {
        const size_t r = refs ? refs[i].root : 0, j = refs ? refs[i].index : i, n = n_leaves[r];
        const uint8_t *row = paths32 + i * stride * 32;
        uint8_t &v = verdict_out[i];
        v = j >= n ? 2 : 0;
        bool has[20]; size_t w = n;
        for (size_t l = 0; l < stride && v == 0; l++) {
            has[l] = w > 1 && ((j >> l) ^ 1) < w;
            if (!has[l] && memcmp(row + 32 * l, zero, 32) != 0) v = 2;
            w = (w + 1) / 2;
        }
        if (v) continue;
        uint8_t cur[32], up[32];
        if (!msg_off) memcpy(cur, msg_bytes + 32 * i, 32);
        else host_labelled_digest(cur, "rofl-zk/mtr/v1/l", msg_bytes + msg_off[i], msg_off[i + 1] - msg_off[i]);
        for (size_t l = 0; l < stride; l++) {
            if (!has[l]) continue;
            if ((j >> l) & 1) mt_host_node(up, row + 32 * l, cur); else mt_host_node(up, cur, row + 32 * l);
            memcpy(cur, up, 32);
        }
        mt_host_root(up, n, cur);
        v = memcmp(up, root32 + 32 * r, 32) == 0 ? 0 : 1;
    }
    return ROFL_OK;
}
