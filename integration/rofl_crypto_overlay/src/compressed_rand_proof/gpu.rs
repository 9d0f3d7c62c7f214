//! Replacement bodies for the three helpers of rofl_crypto/src/compressed_rand_proof/mod.rs:134-160 (`helper_prove`,
//! `helper_prove_existing`, `helper_verify`): delete them there and add `mod gpu;` -- a second `impl` block in a child module sees the
//! private fields.  ONE 128-byte proof for all d ElGamal pairs; the device computes the pairs and the challenge-power dot products, the
//! transcript over the d pairs (labels UNIQUE_U8_TRIPLETS[i], unique_u8_triplets.rs) stays a host sponge inside the library.
//! NOT compiled in the build image (no Rust toolchain); the C entry points are tested through ctypes (tests/test_gpu_parity.py).
use curve25519_dalek_ng::ristretto::RistrettoPoint;
use curve25519_dalek_ng::scalar::Scalar;

use super::types::CompressedRandProofCommitments;
use super::{CompressedRandProof, ElGamalPair, ProofError};
use crate::ffi::*;

const PAIR_LEN: usize = 64;     // ElGamalPair::to_bytes: L | R (rand_proof/el_gamal.rs)

fn prove(m_vec: &Vec<f32>, m_com: Option<&Vec<RistrettoPoint>>, r_vec: &Vec<Scalar>)
    -> Result<(CompressedRandProof, CompressedRandProofCommitments), ProofError> {
    let d = m_vec.len();
    if r_vec.len() != d || m_com.map_or(false, |c| c.len() != d) { return Err(ProofError::WrongNumBlindingFactors); }   // party.rs:60-62
    let r = scalars_to_bytes(r_vec);
    let ex = m_com.map(|v| points_to_bytes(v));
    let (mut proof, mut pairs) = (vec![0u8; CompressedRandProof::serialized_size()], vec![0u8; d * PAIR_LEN]);
    let nonce = fresh_nonce();
    let rc = unsafe {
        rofl_create_compressed_randproof(m_vec.as_ptr(), d, r.as_ptr(), r_vec.len(), ex.as_ref().map_or(std::ptr::null(), |v| v.as_ptr()),
                                         fp_bits(), fp_frac(), &nonce, proof.as_mut_ptr(), pairs.as_mut_ptr())
    };
    if rc != ROFL_OK { panic!("rofl_zk: {}", last_error()); }
    let c_vec: Vec<ElGamalPair> = pairs.chunks(PAIR_LEN).map(|c| ElGamalPair::from_bytes(c).unwrap()).collect();
    Ok((CompressedRandProof::from_bytes(&proof)?, CompressedRandProofCommitments { c_vec }))
}

impl CompressedRandProof {
    pub fn helper_prove(m_vec: &Vec<f32>, r_vec: Vec<Scalar>) -> Result<(CompressedRandProof, CompressedRandProofCommitments), ProofError> {
        prove(m_vec, None, &r_vec)
    }
    pub fn helper_prove_existing(m_vec: &Vec<f32>, m_com: Vec<RistrettoPoint>, r_vec: Vec<Scalar>)
        -> Result<(CompressedRandProof, CompressedRandProofCommitments), ProofError> {
        prove(m_vec, Some(&m_com), &r_vec)
    }
    /// `helper_prove` / `helper_prove_existing` for the clients of one process (client.rs:265-266 runs them as tasks of one process):
    /// ONE rofl_create_compressed_randproof_batch call, every client's result what its own helper call returns.  m_com[i] = None: no
    /// commitments to complete for client i.  A client whose inputs the library refuses (a non-finite value, an undecodable commitment)
    /// panics as in the single helper.
    pub fn helper_prove_batch(m_vecs: &[&Vec<f32>], m_coms: &[Option<&Vec<RistrettoPoint>>], r_vecs: &[&Vec<Scalar>])
        -> Result<Vec<(CompressedRandProof, CompressedRandProofCommitments)>, ProofError> {
        let n = m_vecs.len();
        if n == 0 { return Ok(Vec::new()); }
        let d = m_vecs[0].len();
        if r_vecs.len() != n || m_coms.len() != n { return Err(ProofError::WrongNumBlindingFactors); }
        for i in 0..n {
            if m_vecs[i].len() != d || r_vecs[i].len() != d || m_coms[i].map_or(false, |c| c.len() != d) { return Err(ProofError::WrongNumBlindingFactors); }
        }
        let r: Vec<Vec<u8>> = r_vecs.iter().map(|v| scalars_to_bytes(v)).collect();
        let ex: Vec<Option<Vec<u8>>> = m_coms.iter().map(|c| c.map(|v| points_to_bytes(v))).collect();
        let mut proofs: Vec<Vec<u8>> = (0..n).map(|_| vec![0u8; CompressedRandProof::serialized_size()]).collect();
        let mut pairs: Vec<Vec<u8>> = (0..n).map(|_| vec![0u8; d * PAIR_LEN]).collect();
        let nonces: Vec<RoflNonce> = (0..n).map(|_| fresh_nonce()).collect();
        let vp: Vec<*const f32> = m_vecs.iter().map(|v| v.as_ptr()).collect();
        let rp: Vec<*const u8> = r.iter().map(|v| v.as_ptr()).collect();
        let ep: Vec<*const u8> = ex.iter().map(|e| e.as_ref().map_or(std::ptr::null(), |v| v.as_ptr())).collect();
        let pp: Vec<*mut u8> = proofs.iter_mut().map(|v| v.as_mut_ptr()).collect();
        let cp: Vec<*mut u8> = pairs.iter_mut().map(|v| v.as_mut_ptr()).collect();
        let mut rcs: Vec<std::os::raw::c_int> = vec![0; n];
        let rc = unsafe {
            rofl_create_compressed_randproof_batch(n, vp.as_ptr(), d, rp.as_ptr(), ep.as_ptr(), fp_bits(), fp_frac(), nonces.as_ptr(),
                                                   pp.as_ptr(), cp.as_ptr(), rcs.as_mut_ptr())
        };
        if rc != ROFL_OK { panic!("rofl_zk: {}", last_error()); }
        let mut out = Vec::with_capacity(n);
        for i in 0..n {
            if rcs[i] != ROFL_OK { panic!("rofl_zk: client {} of the batch: error {}", i, rcs[i]); }
            let c_vec: Vec<ElGamalPair> = pairs[i].chunks(PAIR_LEN).map(|c| ElGamalPair::from_bytes(c).unwrap()).collect();
            out.push((CompressedRandProof::from_bytes(&proofs[i])?, CompressedRandProofCommitments { c_vec }));
        }
        Ok(out)
    }
    pub fn helper_verify(&self, c_vec: Vec<ElGamalPair>) -> Result<(), ProofError> {
        let pairs: Vec<u8> = c_vec.iter().flat_map(|c| c.to_bytes()).collect();
        let proof = self.to_bytes();
        let mut ok: std::os::raw::c_int = 0;
        let rc = unsafe { rofl_verify_compressed_randproof(proof.as_ptr(), pairs.as_ptr(), c_vec.len(), &mut ok) };
        if rc == ROFL_FORMAT_ERROR { return Err(ProofError::FormatError); }
        if rc != ROFL_OK { panic!("rofl_zk: {}", last_error()); }
        if ok != 0 { Ok(()) } else { Err(ProofError::VerificationError) }
    }
    /// The proofs of a round's clients over records read in place: records[i] is client i's d records of `stride` bytes as they came off
    /// the wire -- 64 (ElGamalPair::to_bytes) or 96 (SquareRandProofCommitments::to_bytes: c.L | c.R | c_sq, of which only the pair is
    /// read).  ONE rofl_verify_compressed_randproof_batch_strided call; verdict i is what proofs[i].helper_verify gives on client i's
    /// pairs, a malformed member (FormatError there) is false and the others are still verified.  With stride 96 this is the check the
    /// EncL2Compressed arm of EncModelParams::verify (params.rs:257-289) leaves out: call it there, beside the square proofs and the
    /// range proofs, so that a client cannot send arbitrary R and cost the round its aggregate.
    pub fn helper_verify_batch_strided(proofs: &[&CompressedRandProof], records: &[&[u8]], stride: usize, d: usize) -> Vec<bool> {
        let n = proofs.len();
        assert!(records.len() == n && records.iter().all(|r| r.len() == d * stride));
        if n == 0 { return Vec::new(); }
        let pb: Vec<Vec<u8>> = proofs.iter().map(|p| p.to_bytes()).collect();
        let pp: Vec<*const u8> = pb.iter().map(|v| v.as_ptr()).collect();
        let rp: Vec<*const u8> = records.iter().map(|r| r.as_ptr()).collect();
        let mut ok: Vec<std::os::raw::c_int> = vec![0; n];
        let rc = unsafe { rofl_verify_compressed_randproof_batch_strided(n, pp.as_ptr(), rp.as_ptr(), stride, d, ok.as_mut_ptr()) };
        if rc != ROFL_OK { panic!("rofl_zk: {}", last_error()); }
        ok.iter().map(|&o| o != 0).collect()
    }
}
