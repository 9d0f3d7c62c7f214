"""Helper for test_gpu_blinding.py::test_device_output: blinding vectors written straight into a GPU tensor (torch in a child process, as
the other device-pointer checks do) -- same bytes as the host-output call, a misaligned device pointer is refused, and the tensor works as
the blindings32 of create_rangeproof without a host copy."""
import os, sys
import numpy as np
import torch
torch.cuda.init()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
import rofl_project_code_amd as R
from rofl_project_code_amd.api import pedersen_ops as P
R.set_device(0)
R.api.set_fp(32, 7)
seed, d = b"\x5b" * 32, 513
host = P.rnd_scalar_vec_seeded(d, seed, first=3)
dev = torch.zeros((d, 32), dtype=torch.uint8, device="cuda")
assert P.rnd_scalar_vec_seeded(d, seed, first=3, out=dev) is dev
assert (dev.cpu().numpy() == host).all()
# host and device destinations in one call, several terms
terms = [[(b"\x01" * 32, 1), (b"\x02" * 32, -1)], [(b"\x03" * 32, -1)]]
both = P.blinding_vecs(terms, 33)
d0, h1 = torch.zeros((33, 32), dtype=torch.uint8, device="cuda"), np.zeros((33, 32), dtype=np.uint8)
P.blinding_vecs(terms, 33, out=[d0, h1])
assert (d0.cpu().numpy() == both[0]).all() and (h1 == both[1]).all()
# a device pointer that is not 16-byte aligned: 11, nothing written
raw = torch.zeros(64 * 32 + 16, dtype=torch.uint8, device="cuda")
try:
    P.blinding_vecs([[(seed, 1)]], 8, out=[raw.data_ptr() + 8])
    raise SystemExit("a misaligned device output was accepted")
except R.RoflError as e:
    assert e.code == 11, e
assert not raw.cpu().numpy().any()
# the tensor as blindings32 of create_rangeproof (d = 5, 8-bit, one partition, fixed nonce seed) = the host copy of the same blindings
vals = np.array([0.5, -0.25, 0.0, 0.75, -0.5], dtype=np.float32)
bl_dev = torch.zeros((5, 32), dtype=torch.uint8, device="cuda")
P.rnd_scalar_vec_seeded(5, seed, out=bl_dev)
bl_host = P.rnd_scalar_vec_seeded(5, seed)
pr, cm = R.range_proof_vec.create_rangeproof(vals, bl_host, 8, 1, nonce=R.Nonce.seeded(b"\x42" * 32))
pr2, cm2 = R.range_proof_vec.create_rangeproof(torch.from_numpy(vals).cuda(), bl_dev, 8, 1, nonce=R.Nonce.seeded(b"\x42" * 32))
assert (pr == pr2).all() and (cm == cm2).all()
assert R.range_proof_vec.verify_rangeproof(pr2, cm2, 8, verifier_seed=b"\x01" * 32)
print("BLINDING_DEVICE_OUTPUT PASS")
