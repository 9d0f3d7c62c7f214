// SHA-512 (FIPS 180-4) for host and device: the block function and the padding of pre || M, the one hash of the standard signatures
// (RFC 8032 Ed25519: rofl_ed25519_*).  The kernels and their host twins compile this one text.
//
// Registers, not memory: the eight working words and a ROLLING window of sixteen schedule words (W[t] overwrites W[t - 16]) are all the
// state a block needs -- 24 words of 64 bits on top of the chaining value, no 80-entry schedule.  The round constants are a constant
// table read at a wave-uniform index (scalar loads on the device).  The 64-bit rotations are rotl64's two 32-bit funnel shifts.
#pragma once
#include "keccak.hpp"

namespace rofl {

HD u64 sha512_rotr(u64 x, int n) { return rotl64(x, 64 - n); }
HD void sha512_init(u64 H[8]) {
    H[0] = 0x6a09e667f3bcc908ULL; H[1] = 0xbb67ae8584caa73bULL; H[2] = 0x3c6ef372fe94f82bULL; H[3] = 0xa54ff53a5f1d36f1ULL;
    H[4] = 0x510e527fade682d1ULL; H[5] = 0x9b05688c2b3e6c1fULL; H[6] = 0x1f83d9abfb41bd6bULL; H[7] = 0x5be0cd19137e2179ULL;
}
// H <- compress(H, w): w holds the block's sixteen big-endian words and is used up as the schedule window
HDN inline void sha512_block(u64 H[8], u64 w[16]) {
    const u64 K[80] = {
        0x428a2f98d728ae22ULL, 0x7137449123ef65cdULL, 0xb5c0fbcfec4d3b2fULL, 0xe9b5dba58189dbbcULL,
        0x3956c25bf348b538ULL, 0x59f111f1b605d019ULL, 0x923f82a4af194f9bULL, 0xab1c5ed5da6d8118ULL,
        0xd807aa98a3030242ULL, 0x12835b0145706fbeULL, 0x243185be4ee4b28cULL, 0x550c7dc3d5ffb4e2ULL,
        0x72be5d74f27b896fULL, 0x80deb1fe3b1696b1ULL, 0x9bdc06a725c71235ULL, 0xc19bf174cf692694ULL,
        0xe49b69c19ef14ad2ULL, 0xefbe4786384f25e3ULL, 0x0fc19dc68b8cd5b5ULL, 0x240ca1cc77ac9c65ULL,
        0x2de92c6f592b0275ULL, 0x4a7484aa6ea6e483ULL, 0x5cb0a9dcbd41fbd4ULL, 0x76f988da831153b5ULL,
        0x983e5152ee66dfabULL, 0xa831c66d2db43210ULL, 0xb00327c898fb213fULL, 0xbf597fc7beef0ee4ULL,
        0xc6e00bf33da88fc2ULL, 0xd5a79147930aa725ULL, 0x06ca6351e003826fULL, 0x142929670a0e6e70ULL,
        0x27b70a8546d22ffcULL, 0x2e1b21385c26c926ULL, 0x4d2c6dfc5ac42aedULL, 0x53380d139d95b3dfULL,
        0x650a73548baf63deULL, 0x766a0abb3c77b2a8ULL, 0x81c2c92e47edaee6ULL, 0x92722c851482353bULL,
        0xa2bfe8a14cf10364ULL, 0xa81a664bbc423001ULL, 0xc24b8b70d0f89791ULL, 0xc76c51a30654be30ULL,
        0xd192e819d6ef5218ULL, 0xd69906245565a910ULL, 0xf40e35855771202aULL, 0x106aa07032bbd1b8ULL,
        0x19a4c116b8d2d0c8ULL, 0x1e376c085141ab53ULL, 0x2748774cdf8eeb99ULL, 0x34b0bcb5e19b48a8ULL,
        0x391c0cb3c5c95a63ULL, 0x4ed8aa4ae3418acbULL, 0x5b9cca4f7763e373ULL, 0x682e6ff3d6b2b8a3ULL,
        0x748f82ee5defb2fcULL, 0x78a5636f43172f60ULL, 0x84c87814a1f0ab72ULL, 0x8cc702081a6439ecULL,
        0x90befffa23631e28ULL, 0xa4506cebde82bde9ULL, 0xbef9a3f7b2c67915ULL, 0xc67178f2e372532bULL,
        0xca273eceea26619cULL, 0xd186b8c721c0c207ULL, 0xeada7dd6cde0eb1eULL, 0xf57d4f7fee6ed178ULL,
        0x06f067aa72176fbaULL, 0x0a637dc5a2c898a6ULL, 0x113f9804bef90daeULL, 0x1b710b35131c471bULL,
        0x28db77f523047d84ULL, 0x32caab7b40c72493ULL, 0x3c9ebe0a15c9bebcULL, 0x431d67c49c100d4cULL,
        0x4cc5d4becb3e42b6ULL, 0x597f299cfc657e2aULL, 0x5fcb6fab3ad6faecULL, 0x6c44198c4a475817ULL};
    u64 a = H[0], b = H[1], c = H[2], d = H[3], e = H[4], f = H[5], g = H[6], h = H[7];
    for (int t0 = 0; t0 < 80; t0 += 16) {
#pragma unroll
        for (int i = 0; i < 16; i++) {
            if (t0) {      // W[t] = s1(W[t - 2]) + W[t - 7] + s0(W[t - 15]) + W[t - 16], in place of W[t - 16]
                const u64 x = w[(i + 1) & 15], y = w[(i + 14) & 15];
                w[i] += (sha512_rotr(x, 1) ^ sha512_rotr(x, 8) ^ (x >> 7)) + w[(i + 9) & 15] + (sha512_rotr(y, 19) ^ sha512_rotr(y, 61) ^ (y >> 6));
            }
            const u64 t1 = h + (sha512_rotr(e, 14) ^ sha512_rotr(e, 18) ^ sha512_rotr(e, 41)) + ((e & f) ^ (~e & g)) + K[t0 + i] + w[i];
            const u64 t2 = (sha512_rotr(a, 28) ^ sha512_rotr(a, 34) ^ sha512_rotr(a, 39)) + ((a & b) ^ (a & c) ^ (b & c));
            h = g; g = f; f = e; e = d + t1; d = c; c = b; b = a; a = t1 + t2;
        }
    }
    H[0] += a; H[1] += b; H[2] += c; H[3] += d; H[4] += e; H[5] += f; H[6] += g; H[7] += h;
}
// H = SHA-512(pre || M).  pre: `pw` (0 .. 8) whole words as a little-endian load of their bytes gives them; M: `len` bytes behind the loader,
// msg(k) = bytes 8 k .. 8 k + 8 of M as a little-endian word (whatever lies past the end of M is masked off here; msg is asked only for
// words that hold a byte of M).  Stream word g of pre || M is pre[g] or message word g - pw; the word after the last whole one carries the
// remaining 0 .. 7 bytes and the 0x80 byte above them; the last block ends in the bit length (below 2^64: word 14 stays zero).  There
// are (8 pw + len + 17 + 127) / 128 blocks: with pw = 8 the padding spills into a block of its own from len = 48, 176, ...; with pw = 4
// from len = 80, 208, ...
template <class Msg> HDN inline void sha512_pre_msg(u64 H[8], const u64 pre[8], u32 pw, const Msg &msg, u64 len) {
    const u64 nw = len >> 3, gpad = pw + nw, total = 8 * (u64)pw + len, nblk = (total + 17 + 127) >> 7;
    const u32 rem = (u32)len & 7u;
    sha512_init(H);
    for (u64 b = 0; b < nblk; b++) {
        u64 w[16];
#pragma unroll
        for (int i = 0; i < 16; i++) {
            const u64 g = 16 * b + i;
            u64 v = 0;
            if (i < 8 && b == 0 && (u32)i < pw) v = pre[i < 8 ? i : 0];
            else if (g <= gpad) {
                const u64 k = g - pw;
                if (k < nw || rem) v = msg(k);
                if (k == nw) v = (v & ((1ULL << (8 * rem)) - 1)) | (0x80ULL << (8 * rem));
            }
            w[i] = __builtin_bswap64(v);
        }
        if (b + 1 == nblk) w[15] = total << 3;
        sha512_block(H, w);
    }
}
// int_le(the 64 digest bytes) mod l, canonical: what RFC 8032 makes of a nonce hash and of a challenge hash
HD sc sha512_scalar(const u64 H[8]) {
    sc lo, hi;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const u64 x = __builtin_bswap64(H[j]), y = __builtin_bswap64(H[4 + j]);
        lo.v[2 * j] = (u32)x; lo.v[2 * j + 1] = (u32)(x >> 32); hi.v[2 * j] = (u32)y; hi.v[2 * j + 1] = (u32)(y >> 32);
    }
    return sc_from_wide(lo, hi);
}

}  // namespace rofl
