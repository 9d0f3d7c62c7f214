//! Replacement bodies for rofl_crypto/src/l2_range_proof_vec/mod.rs:15-253.
use bulletproofs::{ProofError, RangeProof};
use curve25519_dalek_ng::ristretto::{CompressedRistretto, RistrettoPoint};
use curve25519_dalek_ng::scalar::Scalar;

use crate::ffi::*;
pub mod errors;
pub use self::errors::L2RangeProofError;

/// reference: l2_range_proof_vec/mod.rs:15-140 (sum of squares mod l, f32 shadow check, label b"L2RangeProof", gens (64, 1))
pub fn create_rangeproof_l2(
    value_vec: &Vec<f32>,
    blinding_vec: &Vec<Scalar>,
    prove_range: usize,
    n_partition: usize,
) -> Result<(RangeProof, RistrettoPoint), L2RangeProofError> {
    let bl = scalars_to_bytes(blinding_vec);
    let mut proof = vec![0u8; 32 * (9 + 2 * 6)];         // n = 64, m = 1 is the largest shape
    let mut commit = [0u8; 32];
    let mut plen = 0usize;
    let nonce = fresh_nonce();
    let rc = unsafe {
        rofl_create_rangeproof_l2(value_vec.as_ptr(), value_vec.len(), bl.as_ptr(), blinding_vec.len(), prove_range, n_partition,
                                  fp_bits(), fp_frac(), &nonce, proof.as_mut_ptr(), &mut plen, commit.as_mut_ptr())
    };
    match rc {
        ROFL_OK => Ok((RangeProof::from_bytes(&proof[..plen]).expect("librofl_zk proof layout"),
                       CompressedRistretto(commit).decompress().expect("valid encoding"))),
        ROFL_WRONG_NUM_BLINDING_FACTORS => Err(ProofError::WrongNumBlindingFactors.into()),
        ROFL_NORM_OUT_OF_RANGE => Err(L2RangeProofError::NormOutOfRangeError(last_error())),   // :60-64
        ROFL_OVERFLOW => Err(L2RangeProofError::OverflowError(last_error(), String::new())),   // :53-58
        ROFL_INVALID_BITSIZE => Err(ProofError::InvalidBitsize.into()),
        ROFL_SUM_ERROR => Err(L2RangeProofError::SumError),
        _ => panic!("Should not get here: {}", last_error()),
    }
}

/// reference: l2_range_proof_vec/mod.rs:185-253
pub fn verify_rangeproof_l2(range_proof: &RangeProof, commit: &RistrettoPoint, prove_range: usize) -> Result<bool, ProofError> {
    let pb = range_proof.to_bytes();
    let cb = commit.compress().to_bytes();
    let seed = fresh_seed();
    let mut ok: std::os::raw::c_int = 0;
    let rc = unsafe { rofl_verify_rangeproof_l2(pb.as_ptr(), pb.len(), cb.as_ptr(), prove_range, fp_bits(), fp_frac(), seed.as_ptr(), &mut ok) };
    match rc {
        ROFL_OK => Ok(ok != 0),
        ROFL_INVALID_BITSIZE => Err(ProofError::InvalidBitsize),
        ROFL_FORMAT_ERROR => Err(ProofError::FormatError),
        _ => panic!("rofl_zk: {}", last_error()),
    }
}

/// No counterpart in the reference (its trainer clips in float): projection of an update onto the L2 ball of `max_sq` grid steps^2 ON the
/// fixed-point grid, so that the sum of squares `create_rangeproof_l2` computes for the result is at most `max_sq` by construction.  A
/// vector inside the ball comes back on the grid unchanged; otherwise its steps are scaled by m / 2^32 and truncated (`seed` None) or
/// rounded by the words of the seed's stream -- a per-round secret of the client.  Returns (values, scale): scale is 2^32 for a vector
/// that fitted, else m.  Panics on a bad parameter (a seeded call needs isqrt(max_sq) >= ceil(sqrt(d))).
pub fn clip_l2(value_vec: &Vec<f32>, prove_range: usize, max_sq: u64, seed: Option<&[u8; 32]>) -> (Vec<f32>, u64) {
    let mut out = vec![0f32; value_vec.len()];
    let mut scale: u64 = 0;
    let (vp, op) = (value_vec.as_ptr(), out.as_mut_ptr());
    let sp = seed.map_or(std::ptr::null(), |s| s.as_ptr());
    let rc = unsafe { rofl_clip_l2(1, sp, &vp, value_vec.len(), &max_sq, prove_range, fp_bits(), fp_frac(), &op, &mut scale) };
    if rc != ROFL_OK { panic!("rofl_zk: {}", last_error()); }
    (out, scale)
}

/// `create_rangeproof_l2` for the clients of one process (client.rs:265-266 runs them as tasks of one process): ONE
/// rofl_create_rangeproof_l2_batch call -- one kernel for every client's sums, one Bulletproof launch sequence for all sum proofs.  Entry i
/// is what `create_rangeproof_l2` returns for client i, its error included.
pub fn create_rangeproof_l2_batch(value_vecs: &[&Vec<f32>], blinding_vecs: &[&Vec<Scalar>], prove_range: usize, n_partition: usize)
    -> Vec<Result<(RangeProof, RistrettoPoint), L2RangeProofError>> {
    let n = value_vecs.len();
    if n == 0 { return Vec::new(); }
    let d = value_vecs[0].len();
    if blinding_vecs.len() != n || (0..n).any(|i| value_vecs[i].len() != d || blinding_vecs[i].len() != d) {
        return (0..n).map(|_| Err(ProofError::WrongNumBlindingFactors.into())).collect();
    }
    let bl: Vec<Vec<u8>> = blinding_vecs.iter().map(|v| scalars_to_bytes(v)).collect();
    let mut proofs: Vec<Vec<u8>> = (0..n).map(|_| vec![0u8; 32 * (9 + 2 * 7)]).collect();
    let mut commits = vec![0u8; 32 * n];
    let mut plen = 0usize;
    let nonces: Vec<RoflNonce> = (0..n).map(|_| fresh_nonce()).collect();
    let vp: Vec<*const f32> = value_vecs.iter().map(|v| v.as_ptr()).collect();
    let bp: Vec<*const u8> = bl.iter().map(|v| v.as_ptr()).collect();
    let pp: Vec<*mut u8> = proofs.iter_mut().map(|v| v.as_mut_ptr()).collect();
    let mut rcs: Vec<std::os::raw::c_int> = vec![0; n];
    let rc = unsafe {
        rofl_create_rangeproof_l2_batch(n, vp.as_ptr(), d, bp.as_ptr(), prove_range, n_partition, fp_bits(), fp_frac(), nonces.as_ptr(),
                                        pp.as_ptr(), &mut plen, commits.as_mut_ptr(), rcs.as_mut_ptr())
    };
    if rc != ROFL_OK { panic!("rofl_zk: {}", last_error()); }
    (0..n).map(|i| match rcs[i] {
        ROFL_OK => Ok((RangeProof::from_bytes(&proofs[i][..plen]).expect("librofl_zk proof layout"),
                       CompressedRistretto::from_slice(&commits[32 * i..32 * i + 32]).decompress().expect("valid encoding"))),
        ROFL_NORM_OUT_OF_RANGE => Err(L2RangeProofError::NormOutOfRangeError(format!("client {} of the batch", i))),
        ROFL_OVERFLOW => Err(L2RangeProofError::OverflowError(format!("client {} of the batch", i), String::new())),
        ROFL_INVALID_BITSIZE => Err(ProofError::InvalidBitsize.into()),
        code => panic!("Should not get here: client {} of the batch: error {}", i, code),
    }).collect()
}
