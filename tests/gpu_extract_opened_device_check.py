"""Helper for test_gpu_extract_opened.py::test_the_opening_as_a_device_tensor (torch needs a process of its own, as the other device-pointer checks
do): the opening as a torch uint8 tensor on the GPU gives the accepted clients' sum for every d and both initial pairs, a wrong one is
located, a misaligned device pointer is refused, and the accumulator is unchanged throughout."""
import os, sys
import numpy as np
import torch
torch.cuda.init()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
import rofl_project_code_amd as R
import test_gpu_extract_opened as T

R.set_device(0); R.api.set_fp(*T.FP)
rounds = T._build_rounds(T.DS)
for d in T.DS:
    rd = rounds[d]
    for init in (0, 1):
        want = T._sum_f32([rd["ks"][i] for i in T.ACCEPTED], init).tobytes()
        with T._acc(R, rd, T.ACCEPTED, init) as a:
            before = a.export().tobytes()
            dev = torch.from_numpy(rd["s"].copy()).cuda()
            got = a.extract_opened(opening=dev)
            assert got is not None and got.tobytes() == want, (d, init)
            assert dev.cpu().numpy().tobytes() == rd["s"].tobytes()      # read in place, not written
            k = d - 1
            bad = rd["s"].copy(); bad[k, 31] ^= 1
            assert a.extract_opened(opening=torch.from_numpy(bad).cuda()) is None and a.last_first_bad == k
            buf = torch.zeros(d * 32 + 16, dtype=torch.uint8, device="cuda")
            buf[1:1 + d * 32] = dev.reshape(-1)
            try:
                a.extract_opened(opening=buf[1:1 + d * 32])
                raise SystemExit("a misaligned device opening was accepted")
            except R.api.RoflError as e:
                assert e.code == 11, e
            assert a.export().tobytes() == before
print("OPENING_DEVICE_TENSOR PASS")
