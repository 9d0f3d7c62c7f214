"""Helper for test_gpu_sigma_create_batch.py::test_device_resident_inputs: device pointers in, same bytes out."""
import os, sys
import numpy as np
import torch
torch.cuda.init()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
import rofl_project_code_amd as R
R.set_device(0)
FP = (16, 7)
d, n = 65, 3
xs, r1s, r2s, coms = [], [], [], []
for i in range(n):
    rng = np.random.default_rng(177 + i)
    x = (rng.integers(-100, 100, size=d) / 128.0).astype(np.float32)
    r1 = rng.integers(0, 256, size=(d, 32), dtype=np.uint8); r1[:, 31] &= 0x0F
    r2 = rng.integers(0, 256, size=(d, 32), dtype=np.uint8); r2[:, 31] &= 0x0F
    xs.append(x); r1s.append(r1); r2s.append(r2); coms.append(R.pedersen_ops.commit_vec(R.conversion32.f32_to_scalar_vec(x, fp=FP), r1))
seeds = [bytes([0x70 + i]) * 32 for i in range(n)]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def single(kind, i, ex):
    if kind == 0:
        return R.rand_proof_vec.create_randproof_vec(xs[i], r1s[i], nonce=R.Nonce.seeded(seeds[i]), existing=ex, fp=FP)
    cls = R.square_rand_proof_vec if kind == 1 else R.square_proof_vec
    return cls.create_l2rangeproof_vec(xs[i], r1s[i], r2s[i], nonce=R.Nonce.seeded(seeds[i]), existing=ex, fp=FP)


def batch(kind, vl, al, bl, el):
    nonces = [R.Nonce.seeded(s) for s in seeds]
    if kind == 0:
        return R.rand_proof_vec.create_randproof_vec_batch(vl, al, nonces=nonces, existing_list=el, fp=FP)
    cls = R.square_rand_proof_vec if kind == 1 else R.square_proof_vec
    return cls.create_l2rangeproof_vec_batch(vl, al, bl, nonces=nonces, existing_list=el, fp=FP)


for kind in (0, 1, 2):
    want = [single(kind, i, coms[i]) for i in range(n)]
    # client 1 lives on the device, its neighbours in host memory
    vl, al, bl, el = list(xs), list(r1s), list(r2s), list(coms)
    vl[1], al[1], bl[1], el[1] = dev(xs[1]), dev(r1s[1]), dev(r2s[1]), dev(coms[1])
    got = batch(kind, vl, al, bl, el)
    for i in range(n):
        assert not isinstance(got[i], Exception), (kind, i, got[i])
        assert (got[i][0] == want[i][0]).all() and (got[i][1] == want[i][1]).all(), (kind, i)
    # every client on the device, without commitments to complete
    want2 = [single(kind, i, None) for i in range(n)]
    got2 = batch(kind, [dev(x) for x in xs], [dev(a) for a in r1s], [dev(b) for b in r2s], None)
    for i in range(n):
        assert (got2[i][0] == want2[i][0]).all() and (got2[i][1] == want2[i][1]).all(), (kind, i)
# the single call (the C entry itself: the Python wrappers take host arrays) on device-resident values, r1, r2 and existing: the oracle's bytes
import ctypes
import orc
from rofl_project_code_amd import api
PLEN, CLEN = {0: 128, 1: 192, 2: 160}, {0: 64, 1: 96, 2: 64}
vp = lambda t: ctypes.c_void_p(t.data_ptr())
for kind in (0, 1, 2):
    for i, with_ex in ((0, True), (2, False)):
        tv, t1, t2, te = dev(xs[i]), dev(r1s[i]), dev(r2s[i]), dev(coms[i])
        ns = R.Nonce.seeded(seeds[i])._struct()
        proofs, commits = np.zeros((d, PLEN[kind]), np.uint8), np.zeros((d, CLEN[kind]), np.uint8)
        out = (FP[0], FP[1], ctypes.byref(ns), proofs.ctypes.data_as(ctypes.c_void_p), commits.ctypes.data_as(ctypes.c_void_p))
        ex = vp(te) if with_ex else None
        if kind == 0:
            rc = api.lib().rofl_create_randproof_vec(vp(tv), ctypes.c_size_t(d), vp(t1), ctypes.c_size_t(d), ex, *out)
        else:
            fn = api.lib().rofl_create_squarerandproof_vec if kind == 1 else api.lib().rofl_create_squareproof_vec
            rc = fn(vp(tv), ctypes.c_size_t(d), vp(t1), ctypes.c_size_t(d), vp(t2), ex, *out)
        orc_rc, opr, ocm = orc.sigma_create(kind, xs[i], r1s[i], r2s[i] if kind else None, FP[0], FP[1], seed=seeds[i], existing=coms[i] if with_ex else None)
        assert rc == 0 and orc_rc == 0 and (proofs == opr).all() and (commits == ocm).all(), ("single call, device inputs", kind, i, rc)
print("DEVICE_INPUTS PASS")
