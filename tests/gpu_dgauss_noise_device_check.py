"""Helper for test_gpu_dgauss_noise.py::test_memory_spaces_and_in_place: rofl_noise_dgauss over GPU tensors (torch in a child process, as
the other device-pointer checks do) -- every combination of host and device inputs and outputs gives the model's bytes and leaves the
inputs alone, a host vector, a device vector and a mixed one go through one call of three, in place works in both spaces, and the Python
wrappers take and return GPU tensors."""
import os, sys
import numpy as np
import torch
torch.cuda.init()
HERE = os.path.dirname(os.path.abspath(__file__)); sys.path.insert(0, os.path.dirname(HERE)); sys.path.insert(0, HERE)
import rofl_project_code_amd as R
import dgauss_model as M
from test_binomial_noise_host import inputs
from test_gpu_dgauss_noise import run
R.set_device(0)
nb, fb, ff = 16, 16, 7
d, first, s2 = 257, 31, 50
rng = np.random.default_rng(12)
seeds = [b"\x31" * 32, b"\x32" * 32, b"\x33" * 32]
vals = [inputs(rng, d, nb, fb, ff) for _ in seeds]
want = [M.add_noise(v, s, s2, nb, fb, ff, first).tobytes() for v, s in zip(vals, seeds)]
dev = lambda a: torch.from_numpy(a.copy()).cuda()
for in_dev in (False, True):
    for out_dev in (False, True):
        ins = [dev(v) if in_dev else v.copy() for v in vals]
        outs = [torch.zeros(d, dtype=torch.float32, device="cuda") if out_dev else np.zeros(d, np.float32) for _ in vals]
        run(R, None if (in_dev or out_dev) else 1, seeds, ins, first, s2, nb, fb, ff, outs)      # (a device pointer always takes the kernel)
        assert [(o.cpu().numpy() if out_dev else o).tobytes() for o in outs] == want, (in_dev, out_dev)
        assert [(i.cpu().numpy() if in_dev else i).tobytes() for i in ins] == [v.tobytes() for v in vals], "an input was written"
# n_vec = 3 mixed within one call: device -> host, host -> device, host -> host
ins = [dev(vals[0]), vals[1].copy(), vals[2].copy()]
outs = [np.zeros(d, np.float32), torch.zeros(d, dtype=torch.float32, device="cuda"), np.zeros(d, np.float32)]
run(R, None, seeds, ins, first, s2, nb, fb, ff, outs)
assert [outs[0].tobytes(), outs[1].cpu().numpy().tobytes(), outs[2].tobytes()] == want
# in place: a device vector and a host vector in one call
t, h = dev(vals[0]), vals[1].copy()
run(R, None, seeds[:2], [t, h], first, s2, nb, fb, ff, [t, h])
assert [t.cpu().numpy().tobytes(), h.tobytes()] == want[:2]
# the Python wrappers
rp = R.range_proof_vec
assert rp.add_dgauss_noise(dev(vals[0]), nb, seeds[0], s2, first=first, fp=(fb, ff)).tobytes() == want[0]
t = dev(vals[1])
assert rp.add_dgauss_noise_vecs([t], nb, seeds[1:2], s2, first=first, fp=(fb, ff), out=[t])[0] is t and t.cpu().numpy().tobytes() == want[1]
print("DGAUSS_NOISE_DEVICE PASS")
