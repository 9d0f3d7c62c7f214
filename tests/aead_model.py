"""Python model of rofl_aead_seal / rofl_aead_open (include/rofl_zk.h), independent of the library and of any crypto package: RFC 8439
ChaCha20-Poly1305 on Python integers, shared by test_aead_host.py and test_gpu_aead.py:
  record = CT || tag; the Poly1305 key is the first 32 bytes of ChaCha20 block 0, the data is encrypted from block 1, the tag runs over
    AD || pad16 || CT || pad16 || u64le(len AD) || u64le(len CT);
  derived key = SHAKE256("rofl-zk/seal/v1\\0" || row || u64le(round))[0 .. 32);
  verdict 2: the record is shorter than 16 bytes; 1: the tag does not match (a zero plaintext); 0: opened;
and of the share bundles of secret_sharing.seal_shares / open_shares (bundle_nonce, bundle_ad, the 64-byte payload)."""
import hashlib

import numpy as np

DOM = b"rofl-zk/seal/v1\0"
SHARES_LABEL = b"rofl-zk/shares/1"
assert len(DOM) == 16 and len(SHARES_LABEL) == 16
P1305 = (1 << 130) - 5
CLAMP = 0x0ffffffc0ffffffc0ffffffc0fffffff
M32 = 0xffffffff
# payload and AD lengths around the block ends of ChaCha20 (64) and Poly1305 (16)
PT_LENS = (0, 1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 300)
AD_LENS = (0, 1, 15, 16, 17, 32)
# RFC 8439 section 2.8.2
RFC_KEY = bytes(range(0x80, 0xa0))
RFC_NONCE = bytes.fromhex("070000004041424344454647")
RFC_AD = bytes.fromhex("50515253c0c1c2c3c4c5c6c7")
RFC_PT = b"Ladies and Gentlemen of the class of '99: If I could offer you only one tip for the future, sunscreen would be it."
RFC_CT_HEAD = bytes.fromhex("d31a8d34648e60db7b86afbc53ef7ec2")
RFC_TAG = bytes.fromhex("1ae10b594f09e26a7e902ecbd0600691")


def _rotl(x, n):
    return ((x << n) & M32) | (x >> (32 - n))


def _qr(x, a, b, c, d):
    x[a] = (x[a] + x[b]) & M32; x[d] = _rotl(x[d] ^ x[a], 16)
    x[c] = (x[c] + x[d]) & M32; x[b] = _rotl(x[b] ^ x[c], 12)
    x[a] = (x[a] + x[b]) & M32; x[d] = _rotl(x[d] ^ x[a], 8)
    x[c] = (x[c] + x[d]) & M32; x[b] = _rotl(x[b] ^ x[c], 7)


def chacha20_block(key, counter, nonce):
    """64 bytes (RFC 8439 section 2.3)"""
    key, nonce = bytes(key), bytes(nonce)
    assert len(key) == 32 and len(nonce) == 12
    init = [0x61707865, 0x3320646e, 0x79622d32, 0x6b206574] + [int.from_bytes(key[4 * i:4 * i + 4], "little") for i in range(8)] \
        + [counter & M32] + [int.from_bytes(nonce[4 * i:4 * i + 4], "little") for i in range(3)]
    x = list(init)
    for _ in range(10):
        _qr(x, 0, 4, 8, 12); _qr(x, 1, 5, 9, 13); _qr(x, 2, 6, 10, 14); _qr(x, 3, 7, 11, 15)
        _qr(x, 0, 5, 10, 15); _qr(x, 1, 6, 11, 12); _qr(x, 2, 7, 8, 13); _qr(x, 3, 4, 9, 14)
    return b"".join(((a + b) & M32).to_bytes(4, "little") for a, b in zip(x, init))


def chacha20_xor(key, nonce, data, counter=1):
    data = bytes(data)
    ks = b"".join(chacha20_block(key, counter + j, nonce) for j in range((len(data) + 63) // 64))
    return bytes(a ^ b for a, b in zip(data, ks))


def poly1305(key32, msg):
    """16 bytes: key32 = r || s, r clamped here (RFC 8439 section 2.5)"""
    key32, msg = bytes(key32), bytes(msg)
    assert len(key32) == 32
    r, s, acc = int.from_bytes(key32[:16], "little") & CLAMP, int.from_bytes(key32[16:], "little"), 0
    for i in range(0, len(msg), 16):
        blk = msg[i:i + 16]
        acc = (acc + int.from_bytes(blk + b"\x01", "little")) * r % P1305
    return ((acc + s) & ((1 << 128) - 1)).to_bytes(16, "little")


def _pad16(b):
    return b + bytes(-len(b) % 16)


def derive_key(row, round_no):
    row = bytes(row)
    assert len(row) == 32
    return hashlib.shake_256(DOM + row + int(round_no).to_bytes(8, "little")).digest(32)


def tag(key, nonce, ad, ct):
    otk = chacha20_block(key, 0, nonce)[:32]
    return poly1305(otk, _pad16(bytes(ad)) + _pad16(bytes(ct)) + len(ad).to_bytes(8, "little") + len(ct).to_bytes(8, "little"))


def seal(key, nonce, ad, pt):
    """-> CT || tag"""
    ct = chacha20_xor(key, nonce, pt)
    return ct + tag(key, nonce, ad, ct)


def open_(key, nonce, ad, record):
    """-> (plaintext, verdict)"""
    record = bytes(record)
    if len(record) < 16:
        return b"", 2
    ct, t = record[:-16], record[-16:]
    if tag(key, nonce, ad, ct) != t:
        return bytes(len(ct)), 1
    return chacha20_xor(key, nonce, ct), 0


def _keys(keys, key_idx, n, derive_round):
    keys = [bytes(k) for k in keys]
    assert all(len(k) == 32 for k in keys)
    if derive_round is not None:
        keys = [derive_key(k, derive_round) for k in keys]
    if key_idx is None:
        assert len(keys) == n
        return keys
    return [keys[int(a)] for a in key_idx]


def seal_batch(keys, nonces, ads, pts, key_idx=None, derive_round=None):
    """what aead.seal returns for lists: a list of bytes"""
    ks = _keys(keys, key_idx, len(pts), derive_round)
    return [seal(k, bytes(nc), bytes(ad), bytes(pt)) for k, nc, ad, pt in zip(ks, nonces, ads, pts)]


def open_batch(keys, nonces, ads, records, key_idx=None, derive_round=None):
    """what aead.open returns for lists: (a list of bytes, uint8[n])"""
    ks = _keys(keys, key_idx, len(records), derive_round)
    res = [open_(k, bytes(nc), bytes(ad), bytes(r)) for k, nc, ad, r in zip(ks, nonces, ads, records)]
    return [r[0] for r in res], np.array([r[1] for r in res], np.uint8)


def pack(items):
    """(uint8[total], uint64[n + 1]) as the C ABI takes byte strings"""
    items = [bytes(m) for m in items]
    off = np.zeros(len(items) + 1, np.uint64)
    for j, m in enumerate(items):
        off[j + 1] = off[j] + np.uint64(len(m))
    return np.frombuffer(b"".join(items) or b"\0", np.uint8)[:int(off[-1])].copy(), off


def unpack(data, off, shorten=0):
    """the byte strings of a packed pair; shorten: bytes taken off each one's end (never below zero length)"""
    raw = np.asarray(data, np.uint8).tobytes()
    return [raw[int(off[i]):max(int(off[i + 1]) - shorten, int(off[i]))] for i in range(len(off) - 1)]


def length_grid(rng):
    """Every payload length x every AD length as ONE call's records: (keys uint8[n, 32], nonces uint8[n, 12], ads, pts).  Fillers of 1 .. 7
    bytes (the trick of sig_model.misaligned_messages) put the payloads and the ADs at starts of every misalignment mod 8, aligned ones
    among them; a filler is a record of the call like any other."""
    pairs = [(p, a) for p in PT_LENS for a in AD_LENS]
    pts, ads, off_p, off_a = [], [], 0, 0
    for q, (p, a) in enumerate(pairs):
        fp, fa = ((1, 3, 5, 7, 0, 2, 4, 6)[q % 8] - off_p) % 8, ((2, 5, 0, 1, 6, 3, 7, 4)[q % 8] - off_a) % 8
        if fp or fa:
            pts.append(rng.bytes(fp)); ads.append(rng.bytes(fa)); off_p += fp; off_a += fa
        pts.append(rng.bytes(p)); ads.append(rng.bytes(a)); off_p += p; off_a += a
    n = len(pts)
    assert {len(x) for x in pts} >= set(PT_LENS) and {len(x) for x in ads} >= set(AD_LENS)
    keys = np.frombuffer(rng.bytes(32 * n), np.uint8).reshape(n, 32).copy()
    nonces = np.frombuffer(rng.bytes(12 * n), np.uint8).reshape(n, 12).copy()
    return keys, nonces, ads, pts


def verdict_cases(rng):
    """Every verdict class of open in one call: (keys uint8[n, 32], nonces uint8[n, 12], ads, records, expected plaintexts, expected
    verdicts uint8[n]).  The expectations are written down here, not computed: the callers hold the model to them as well."""
    key, nonce, ad = rng.bytes(32), rng.bytes(12), rng.bytes(20)
    pt = rng.bytes(70)
    good = seal(key, nonce, ad, pt)
    cases = []

    def add(k, nc, a, rec, want_pt, want):
        cases.append((bytes(k), bytes(nc), bytes(a), bytes(rec), bytes(want_pt), want))

    def flip(b, i, bit=1):
        b = bytearray(b); b[i] ^= bit
        return bytes(b)
    zero = bytes(len(pt))
    add(key, nonce, ad, good, pt, 0)
    add(key, nonce, ad, flip(good, 3, 0x10), zero, 1)                  # a bit of the ciphertext
    add(key, nonce, ad, good, pt, 0)
    add(key, nonce, ad, flip(good, len(good) - 1, 0x80), zero, 1)      # a bit of the tag
    add(key, nonce, flip(ad, 19), good, zero, 1)                       # a bit of the AD
    add(key, nonce, ad, good, pt, 0)
    add(key, flip(nonce, 0), ad, good, zero, 1)                        # a bit of the nonce
    add(flip(key, 31, 0x40), nonce, ad, good, zero, 1)                 # a bit of the key
    add(key, nonce, ad, good[:15], b"", 2)                             # shorter than a tag
    add(key, nonce, ad, good, pt, 0)
    add(key, nonce, ad, b"", b"", 2)                                   # the empty record
    add(key, nonce, ad, good[:-1], bytes(len(pt) - 1), 1)              # a truncated record
    e = seal(key, nonce, ad, b"")
    add(key, nonce, ad, e, b"", 0)                                     # the empty payload: a record of exactly 16 bytes
    add(key, nonce, ad, flip(e, 0), b"", 1)
    add(key, nonce, ad, good, pt, 0)
    K = np.frombuffer(b"".join(c[0] for c in cases), np.uint8).reshape(-1, 32).copy()
    N = np.frombuffer(b"".join(c[1] for c in cases), np.uint8).reshape(-1, 12).copy()
    return K, N, [c[2] for c in cases], [c[3] for c in cases], [c[4] for c in cases], np.array([c[5] for c in cases], np.uint8)


def poly_boundary_cases():
    """The Poly1305 family at the reduction boundary: [(key32 = r || s, message, expected tag or None)].  With r = 1 the accumulator is the
    plain sum of the blocks: ff x 16 || (b0 ff x 15) has the true residues p - 2 .. 3 mod p = 2^130 - 5 for b0 = fa .. ff; each with s = 0 and
    with s = 2^128 - 1, where the final addition carries out of 128 bits.  The expected tags are worked out with big integers by the host
    test; here only the one the issue states (r = 2, s = 0, ff x 16 -> 03 00 x 15) is written down."""
    le16 = lambda v: int(v).to_bytes(16, "little")      # noqa: E731
    cases = []
    for s in (0, (1 << 128) - 1):
        for b0 in (0xfa, 0xfb, 0xfc, 0xfd, 0xfe, 0xff):
            cases.append((le16(1) + le16(s), b"\xff" * 16 + bytes([b0]) + b"\xff" * 15, None))
    cases.append((le16(2) + le16(0), b"\xff" * 16, bytes([3]) + bytes(15)))
    for blocks in range(1, 6):
        for tail in (0, 1, 15):
            cases.append((le16(CLAMP) + le16(0x0123456789abcdef0123456789abcdef), b"\xff" * (16 * blocks + tail), None))
    unclamped = (1 << 128) - 1
    cases.append((le16(unclamped) + le16(7), b"\xff" * 47, None))
    cases.append((le16(unclamped & CLAMP) + le16(7), b"\xff" * 47, None))
    cases.append((le16(0x0f0f0f0f0f0f0f0f0f0f0f0f0f0f0f0f) + le16(1), b"", None))      # the empty message: the tag is s
    return cases


def bundle_nonce(sender, recipient):
    return int(sender).to_bytes(4, "little") + int(recipient).to_bytes(4, "little") + bytes(4)


def bundle_ad(round_no, sender, recipient):
    return SHARES_LABEL + int(round_no).to_bytes(8, "little") + int(sender).to_bytes(4, "little") + int(recipient).to_bytes(4, "little")


def seal_shares(shared, own_ids, peer_ids, round_no, key_shares, self_shares):
    """what secret_sharing.seal_shares returns, from the pairs' shared secrets shared[a][b] (32 bytes each): uint8[n_own, n_peer, 80]"""
    out = np.zeros((len(own_ids), len(peer_ids), 80), np.uint8)
    for a, o in enumerate(own_ids):
        for b, p in enumerate(peer_ids):
            if int(o) == int(p):
                continue
            pay = np.asarray(key_shares[a][b], np.uint8).tobytes() + np.asarray(self_shares[a][b], np.uint8).tobytes()
            rec = seal(derive_key(shared[a][b], round_no), bundle_nonce(o, p), bundle_ad(round_no, o, p), pay)
            out[a, b] = np.frombuffer(rec, np.uint8)
    return out


def open_shares(shared, own_ids, peer_ids, round_no, records):
    """what secret_sharing.open_shares returns: (key shares, self shares uint8[n_own, n_peer, 32], verdicts uint8[n_own, n_peer])"""
    n_own, n_peer = len(own_ids), len(peer_ids)
    ks, ss, v = np.zeros((n_own, n_peer, 32), np.uint8), np.zeros((n_own, n_peer, 32), np.uint8), np.zeros((n_own, n_peer), np.uint8)
    for a, o in enumerate(own_ids):
        for b, p in enumerate(peer_ids):
            if int(o) == int(p):
                continue
            pt, v[a, b] = open_(derive_key(shared[a][b], round_no), bundle_nonce(p, o), bundle_ad(round_no, p, o), np.asarray(records[a][b], np.uint8).tobytes())
            ks[a, b], ss[a, b] = np.frombuffer(pt[:32], np.uint8), np.frombuffer(pt[32:], np.uint8)
    return ks, ss, v
