//! GPU bodies for the vector operations of rofl_crypto/src/pedersen_ops.rs:9-59, 103-108 (same signatures; the scalar-only
//! helpers of that file -- add_scalar_vec, zero_*_vec -- and its rnd_scalar_vec / generate_cancelling_scalar_vec, which draw from
//! thread_rng, stay as they are).  The *_seeded functions and pairwise_blinding_vec at the end are additions: blinding vectors
//! expanded on the device from 32-byte seeds (rofl_blinding_vecs), for hosts that want :110-127 reproducible, or cancelling
//! blindings without the dealer of :110-122.  acc_extract_opened(_terms) extract the aggregate of a device accumulator (rofl_acc_*) whose
//! round rejected somebody, from the opening of the accepted clients' residual blinding.
//! dh_public_keys / dh_shared_secrets are the key agreement the pairwise masks' shared secrets come from (rofl_dh_*).
use curve25519_dalek_ng::ristretto::RistrettoPoint;
use curve25519_dalek_ng::scalar::Scalar;

use crate::ffi::*;
use crate::fp::BSGS_N_BITS;

pub fn commit_no_blinding_vec(scalar_vec: &Vec<Scalar>) -> Vec<RistrettoPoint> {
    let v = scalars_to_bytes(scalar_vec);
    let mut out = vec![0u8; scalar_vec.len() * 32];
    let rc = unsafe { rofl_commit_vec(v.as_ptr(), std::ptr::null(), scalar_vec.len(), out.as_mut_ptr()) };
    assert!(rc == ROFL_OK, "rofl_zk: {}", last_error());
    bytes_to_points(&out)
}
pub fn commit_vec(scalar_vec: &Vec<Scalar>, blinding_vec: &Vec<Scalar>) -> Vec<RistrettoPoint> {
    let (v, b) = (scalars_to_bytes(scalar_vec), scalars_to_bytes(blinding_vec));
    let mut out = vec![0u8; scalar_vec.len() * 32];
    let rc = unsafe { rofl_commit_vec(v.as_ptr(), b.as_ptr(), scalar_vec.len(), out.as_mut_ptr()) };
    assert!(rc == ROFL_OK, "rofl_zk: {}", last_error());
    bytes_to_points(&out)
}
pub fn add_rp_vec(a: &Vec<RistrettoPoint>, b: &Vec<RistrettoPoint>) -> Vec<RistrettoPoint> {
    let (x, y) = (points_to_bytes(a), points_to_bytes(b));
    let mut out = vec![0u8; a.len() * 32];
    let rc = unsafe { rofl_add_points_vec(x.as_ptr(), y.as_ptr(), a.len(), out.as_mut_ptr()) };
    assert!(rc == ROFL_OK, "rofl_zk: {}", last_error());
    bytes_to_points(&out)
}
pub fn compute_shifted_values_rp(rp_vec: &Vec<RistrettoPoint>, offset: &RistrettoPoint) -> Vec<RistrettoPoint> {
    let x = points_to_bytes(rp_vec);
    let off = offset.compress().to_bytes();
    let mut out = vec![0u8; rp_vec.len() * 32];
    let rc = unsafe { rofl_shift_points(x.as_ptr(), rp_vec.len(), off.as_ptr(), out.as_mut_ptr()) };
    assert!(rc == ROFL_OK, "rofl_zk: {}", last_error());
    bytes_to_points(&out)
}
/// `BSGSTable` shrinks to its size: the baby-step table lives (cached) on the device.
pub fn discrete_log_vec(rp_vec: &Vec<RistrettoPoint>, table_size: usize) -> Vec<Scalar> {
    let x = points_to_bytes(rp_vec);
    let mut out = vec![0u8; rp_vec.len() * 32];
    let rc = unsafe { rofl_discrete_log_vec(x.as_ptr(), rp_vec.len(), table_size, BSGS_N_BITS as u32, out.as_mut_ptr()) };
    assert!(rc == ROFL_OK, "rofl_zk: {}", last_error());
    bytes_to_scalars(&out)
}

/// `enc_values.iter().map(|x| x.c_sq).sum()` of rofl_service/src/flserver/params.rs:220, 277 on the device: the sum of d compressed points
/// read every `stride` bytes (96 over serialized SquareRandProofCommitments, 32 over a packed vector); an empty input gives the identity.
pub fn sum_points_strided(bytes: &[u8], d: usize, stride: usize) -> RistrettoPoint {
    assert!(stride >= 32 && bytes.len() >= d.saturating_sub(1) * stride + if d > 0 { 32 } else { 0 });
    let mut out = [0u8; 32];
    let rc = unsafe { rofl_sum_points(bytes.as_ptr(), d, stride, out.as_mut_ptr()) };
    assert!(rc == ROFL_OK, "rofl_zk: {}", last_error());
    bytes_to_points(&out)[0]
}
pub fn sum_rp_vec(rp_vec: &Vec<RistrettoPoint>) -> RistrettoPoint { sum_points_strided(&points_to_bytes(rp_vec), rp_vec.len(), 32) }

fn blinding_vecs(term_lists: &[Vec<RoflBlindTerm>], first: usize, d: usize) -> Vec<Vec<Scalar>> {
    let counts: Vec<usize> = term_lists.iter().map(|t| t.len()).collect();
    let tp: Vec<*const RoflBlindTerm> = term_lists.iter().map(|t| t.as_ptr()).collect();
    let mut out: Vec<Vec<u8>> = term_lists.iter().map(|_| vec![0u8; d * 32]).collect();
    let op: Vec<*mut u8> = out.iter_mut().map(|o| o.as_mut_ptr()).collect();
    let rc = unsafe { rofl_blinding_vecs(term_lists.len(), counts.as_ptr(), tp.as_ptr(), first, d, op.as_ptr()) };
    assert!(rc == ROFL_OK, "rofl_zk: {}", last_error());
    out.iter().map(|o| bytes_to_scalars(o)).collect()
}
/// rnd_scalar_vec (:124-127) with the randomness an explicit input: scalars [0, length) of the blinding stream of `seed`.
pub fn rnd_scalar_vec_seeded(length: usize, seed: &[u8; 32]) -> Vec<Scalar> {
    let mut out = vec![0u8; length * 32];
    let rc = unsafe { rofl_rnd_scalar_vec(seed.as_ptr(), 0, length, out.as_mut_ptr()) };
    assert!(rc == ROFL_OK, "rofl_zk: {}", last_error());
    bytes_to_scalars(&out)
}
/// generate_cancelling_scalar_vec (:110-122) from one seed, as one device call: vector i < n_vec - 1 is the stream of
/// seed_i = SHA3-256("rofl-zk/blind/v1/vec" || seed || u32le(i)), the last vector is minus their sum.
pub fn generate_cancelling_scalar_vec_seeded(n_vec: usize, n_dim: usize, seed: &[u8; 32]) -> Vec<Vec<Scalar>> {
    use sha3::{Digest, Sha3_256};
    assert!(n_vec >= 1);
    let seeds: Vec<[u8; 32]> = (0..n_vec - 1).map(|i| {
        let mut h = Sha3_256::new();
        h.update(b"rofl-zk/blind/v1/vec"); h.update(seed); h.update(&(i as u32).to_le_bytes());
        let mut s = [0u8; 32]; s.copy_from_slice(&h.finalize()); s
    }).collect();
    let mut lists: Vec<Vec<RoflBlindTerm>> = seeds.iter().map(|s| vec![RoflBlindTerm { seed: *s, sign: 1 }]).collect();
    lists.push(seeds.iter().map(|s| RoflBlindTerm { seed: *s, sign: -1 }).collect());
    blinding_vecs(&lists, 0, n_dim)
}
/// Dealer-free cancelling blindings: client `index` holds one shared seed per peer, `peers` = (peer index, seed), and its vector is
/// the sum over the peers of +stream(seed) where index < peer index, -stream(seed) otherwise.  A seed serves ONE round.
pub fn pairwise_blinding_vec(index: usize, peers: &[(usize, [u8; 32])], d: usize) -> Vec<Scalar> {
    let terms: Vec<RoflBlindTerm> = peers.iter().map(|(j, s)| {
        assert!(*j != index, "a client is not its own peer");
        RoflBlindTerm { seed: *s, sign: if index < *j { 1 } else { -1 } }
    }).collect();
    blinding_vecs(&[terms], 0, d).pop().unwrap()
}

/// Extraction after rejections (rofl_acc_extract_opened): `opening` = the sum of the accepted clients' blinding vectors, checked against
/// every R of accumulator `h` and stripped from every L.  Ok(values), or Err(k) with the smallest coordinate whose R equation fails (the
/// accumulator is unchanged either way).  `d` is the accumulator's length.
pub fn acc_extract_opened(h: u64, d: usize, opening: &Vec<Scalar>, table_size: usize, fp_bits: u32, fp_frac: u32) -> Result<Vec<f32>, usize> {
    assert!(opening.len() == d);
    let s = scalars_to_bytes(opening);
    let (mut out, mut ok, mut bad) = (vec![0f32; d], 0, usize::MAX);
    let rc = unsafe { rofl_acc_extract_opened(h, s.as_ptr(), table_size, BSGS_N_BITS as u32, fp_bits, fp_frac, out.as_mut_ptr(), &mut ok, &mut bad) };
    assert!(rc == ROFL_OK, "rofl_zk: {}", last_error());
    if ok != 0 { Ok(out) } else { Err(bad) }
}
/// The same with the opening given as the signed seeds it is the sum of (pairwise masks: one term per accepted-rejected pair; a dealer's
/// cancelling vectors: the accepted vectors' seeds): it is expanded on the device and never exists on the host.
pub fn acc_extract_opened_terms(h: u64, d: usize, terms: &[RoflBlindTerm], table_size: usize, fp_bits: u32, fp_frac: u32) -> Result<Vec<f32>, usize> {
    let (mut out, mut ok, mut bad) = (vec![0f32; d], 0, usize::MAX);
    let rc = unsafe { rofl_acc_extract_opened_terms(h, terms.len(), terms.as_ptr(), table_size, BSGS_N_BITS as u32, fp_bits, fp_frac, out.as_mut_ptr(), &mut ok, &mut bad) };
    assert!(rc == ROFL_OK, "rofl_zk: {}", last_error());
    if ok != 0 { Ok(out) } else { Err(bad) }
}

/// Public keys of `sk` (32 bytes each, reduced mod l; a key that is 0 mod l panics with the library's text): encode(sk * B).
pub fn dh_public_keys(sk: &[[u8; 32]]) -> Vec<[u8; 32]> {
    let mut out = vec![[0u8; 32]; sk.len()];
    let rc = unsafe { rofl_dh_public_keys(sk.len(), sk.as_ptr() as *const u8, out.as_mut_ptr() as *mut u8) };
    assert!(rc == ROFL_OK, "rofl_zk: {}", last_error());
    out
}
/// Shared secrets of own keys `sk` and peer public keys `peer_pks` for the listed (own, peer) pairs (None: all pairs, own-major), one device
/// call: Ok(32 bytes) per pair, or Err(status) -- 1 the peer key is not a canonical Ristretto encoding, 2 it is the identity.  The secret of
/// a pair is the same on both sides; pairwise_blinding_vec takes the round's seed derived from it.
pub fn dh_shared_secrets(sk: &[[u8; 32]], peer_pks: &[[u8; 32]], pairs: Option<&[RoflDhPair]>) -> Vec<Result<[u8; 32], u8>> {
    let n_pairs = pairs.map_or(sk.len() * peer_pks.len(), |p| p.len());
    let (mut out, mut status) = (vec![[0u8; 32]; n_pairs], vec![0u8; n_pairs]);
    let rc = unsafe { rofl_dh_shared(sk.len(), sk.as_ptr() as *const u8, std::ptr::null_mut(), peer_pks.len(), peer_pks.as_ptr() as *const u8,
        n_pairs, pairs.map_or(std::ptr::null(), |p| p.as_ptr()), out.as_mut_ptr() as *mut u8, status.as_mut_ptr()) };
    assert!(rc == ROFL_OK, "rofl_zk: {}", last_error());
    out.iter().zip(status.iter()).map(|(o, s)| if *s == 0 { Ok(*o) } else { Err(*s) }).collect()
}
/// Shamir shares of `secrets` (32 bytes each, reduced mod l) at threshold `threshold`, one device call: row s holds the shares of secret s
/// at the points `xs` (None: 1 ..= n_shares; otherwise nonzero and distinct, client i holds i + 1).  The coefficients of secret s come
/// from coef_seeds[s], which is as secret as the secret.  A bad parameter panics with the library's text.
pub fn shamir_share(secrets: &[[u8; 32]], coef_seeds: &[[u8; 32]], threshold: usize, n_shares: usize, xs: Option<&[u32]>) -> Vec<Vec<[u8; 32]>> {
    assert!(coef_seeds.len() == secrets.len() && xs.map_or(true, |x| x.len() == n_shares), "one seed per secret, one point per share");
    let mut out = vec![[0u8; 32]; secrets.len() * n_shares];
    let rc = unsafe { rofl_shamir_share(secrets.len(), secrets.as_ptr() as *const u8, coef_seeds.as_ptr() as *const u8, threshold, n_shares,
        xs.map_or(std::ptr::null(), |x| x.as_ptr()), out.as_mut_ptr() as *mut u8) };
    assert!(rc == ROFL_OK, "rofl_zk: {}", last_error());
    out.chunks(n_shares.max(1)).map(|r| r.to_vec()).collect()
}
/// The secrets from `shares` (row s: the shares of secret s at the points `xs`, one set of points for all rows): interpolation at 0 over
/// ALL shares handed in.  Checks nothing: a wrong share gives another secret, not an error -- check the shares with rofl_feldman_verify first.
pub fn shamir_reconstruct(xs: &[u32], shares: &[Vec<[u8; 32]>]) -> Vec<[u8; 32]> {
    assert!(shares.iter().all(|r| r.len() == xs.len()), "one share per point");
    let flat: Vec<[u8; 32]> = shares.iter().flat_map(|r| r.iter().copied()).collect();
    let mut out = vec![[0u8; 32]; shares.len()];
    let rc = unsafe { rofl_shamir_reconstruct(shares.len(), xs.len(), xs.as_ptr(), flat.as_ptr() as *const u8, out.as_mut_ptr() as *mut u8) };
    assert!(rc == ROFL_OK, "rofl_zk: {}", last_error());
    out
}
