"""Helper for test_gpu_prob_quant.py::test_memory_spaces_and_in_place: rofl_quantize_prob over GPU tensors (torch in a child process, as
the other device-pointer checks do) -- every combination of host and device inputs and outputs gives the model's bytes and leaves the inputs
alone, host and device vectors mix within one call, in place works in both spaces, and the Python wrappers take and return GPU tensors."""
import os, sys
import numpy as np
import torch
torch.cuda.init()
HERE = os.path.dirname(os.path.abspath(__file__)); sys.path.insert(0, os.path.dirname(HERE)); sys.path.insert(0, HERE)
import rofl_project_code_amd as R
import pq_model as M
from test_gpu_prob_quant import quant, _inputs
R.set_device(0)
nb, fb, ff = 16, 16, 7
d, first = 257, 31
rng = np.random.default_rng(12)
seeds = [b"\x31" * 32, b"\x32" * 32]
vals = [_inputs(rng, d, nb, fb, ff) for _ in range(2)]
want = [M.quantize(v, s, nb, fb, ff, first).tobytes() for v, s in zip(vals, seeds)]
dev = lambda a: torch.from_numpy(a.copy()).cuda()
for in_dev in (False, True):
    for out_dev in (False, True):
        ins = [dev(v) if in_dev else v.copy() for v in vals]
        outs = [torch.zeros(d, dtype=torch.float32, device="cuda") if out_dev else np.zeros(d, np.float32) for _ in vals]
        quant(R, None if (in_dev or out_dev) else 1, seeds, ins, first, nb, fb, ff, outs)      # (a device pointer always takes the kernel)
        assert [(o.cpu().numpy() if out_dev else o).tobytes() for o in outs] == want, (in_dev, out_dev)
        assert [(i.cpu().numpy() if in_dev else i).tobytes() for i in ins] == [v.tobytes() for v in vals], "an input was written"
# mixed within one call
ins = [dev(vals[0]), vals[1].copy()]
outs = [np.zeros(d, np.float32), torch.zeros(d, dtype=torch.float32, device="cuda")]
quant(R, None, seeds, ins, first, nb, fb, ff, outs)
assert [outs[0].tobytes(), outs[1].cpu().numpy().tobytes()] == want
# in place, a device vector and a host vector in one call
t, h = dev(vals[0]), vals[1].copy()
quant(R, None, seeds, [t, h], first, nb, fb, ff, [t, h])
assert [t.cpu().numpy().tobytes(), h.tobytes()] == want
# the Python wrappers
rp = R.range_proof_vec
assert rp.quantize_probabilistic(dev(vals[0]), nb, seeds[0], first=first, fp=(fb, ff)).tobytes() == want[0]
t = dev(vals[1])
assert rp.quantize_probabilistic_vecs([t], nb, seeds[1:], first=first, fp=(fb, ff), out=[t])[0] is t and t.cpu().numpy().tobytes() == want[1]
# a quantized update on the device goes into create_rangeproof as a device input: the bytes of the host copy of the same values
x = np.full(5, 1 / 512, np.float32)
bl = np.zeros((5, 32), np.uint8); bl[:, 0] = np.arange(1, 6)
q_dev = dev(x)
rp.quantize_probabilistic_vecs([q_dev], 8, seeds[:1], fp=(fb, ff), out=[q_dev])
q_host = rp.quantize_probabilistic(x, 8, seeds[0], fp=(fb, ff))
pr, cm = rp.create_rangeproof(q_host, bl, 8, 1, nonce=R.Nonce.seeded(b"\x42" * 32), fp=(fb, ff))
pr2, cm2 = rp.create_rangeproof(q_dev, torch.from_numpy(bl).cuda(), 8, 1, nonce=R.Nonce.seeded(b"\x42" * 32), fp=(fb, ff))
assert (pr == pr2).all() and (cm == cm2).all()
print("PROB_QUANT_DEVICE PASS")
