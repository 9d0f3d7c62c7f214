"""Helper for test_gpu_rotate.py::test_memory_spaces_and_in_place: rofl_rotate over GPU tensors (torch in a child process, as the other
device-pointer checks do) -- every combination of host and device inputs and outputs gives the model's bytes and leaves the inputs
alone, a host vector, a device vector and a mixed one go through one call of three, in place works in both spaces and both directions,
an input that is not 16-byte aligned takes the scalar loads, and the Python wrappers take and return GPU tensors."""
import os, sys
import numpy as np
import torch
torch.cuda.init()
HERE = os.path.dirname(os.path.abspath(__file__)); sys.path.insert(0, os.path.dirname(HERE)); sys.path.insert(0, HERE)
import rofl_project_code_amd as R
import rot_model as M
from test_rotate_host import SEEDS, inputs, rot_call
R.set_device(0)
dev = lambda a: torch.from_numpy(a.copy()).cuda()
host = lambda o: o.cpu().numpy() if hasattr(o, "cpu") else o
sb = b"".join(SEEDS)
for k, d in ((12, 2 * 4096 + 5), (14, 16384 - 3)):      # one launch; two launches
    dp = M.rotated_len(d, k)
    rng = np.random.default_rng(40 + k)
    vals = [inputs(rng, d) for _ in SEEDS]
    fwd = [M.rotate(x, s, k) for x, s in zip(vals, SEEDS)]
    inv = [M.rotate(y, s, k, inverse=True) for y, s in zip(fwd, SEEDS)]
    for inverse, src, want, n_in in ((0, vals, fwd, d), (1, fwd, inv, dp)):
        wb = [w.tobytes() for w in want]
        for in_dev in (False, True):
            for out_dev in (False, True):
                ins = [dev(v) if in_dev else v.copy() for v in src]
                outs = [torch.zeros(dp, dtype=torch.float32, device="cuda") if out_dev else np.zeros(dp, np.float32) for _ in src]
                rc = rot_call(R.lib(), None if (in_dev or out_dev) else 1, sb, ins, n_in, k, inverse, outs)      # (a device pointer always takes the kernels)
                assert rc == 0 and [host(o).tobytes() for o in outs] == wb, (k, inverse, in_dev, out_dev)
                assert [host(i).tobytes() for i in ins] == [v.tobytes() for v in src], "an input was written"
        # n_vec = 3 mixed within one call: device -> host, host -> device, host -> host
        ins = [dev(src[0]), src[1].copy(), src[2].copy()]
        outs = [np.zeros(dp, np.float32), torch.zeros(dp, dtype=torch.float32, device="cuda"), np.zeros(dp, np.float32)]
        assert rot_call(R.lib(), None, sb, ins, n_in, k, inverse, outs) == 0 and [host(o).tobytes() for o in outs] == wb
        # in place: a device buffer and a host buffer of the output length in one call
        t, h = torch.zeros(dp, dtype=torch.float32, device="cuda"), np.zeros(dp, np.float32)
        t[:n_in] = dev(src[1]); h[:n_in] = src[2]
        if n_in < dp:      # what lies behind the d input elements is not read: the padding counts as zeros
            t[n_in:] = float("nan"); h[n_in:] = np.nan
        assert rot_call(R.lib(), None, sb[32:], [t, h], n_in, k, inverse, [t, h]) == 0 and [host(t).tobytes(), h.tobytes()] == wb[1:]
        # a device input and output 4 bytes off a 16-byte boundary
        big_in, big_out = torch.zeros(n_in + 1, dtype=torch.float32, device="cuda"), torch.zeros(dp + 1, dtype=torch.float32, device="cuda")
        big_in[1:] = dev(src[0])
        assert rot_call(R.lib(), None, sb, [big_in[1:]], n_in, k, inverse, [big_out[1:]]) == 0 and host(big_out[1:]).tobytes() == wb[0] and float(big_out[0]) == 0.0
    # the Python wrappers
    rp = R.range_proof_vec
    assert rp.rotate(dev(vals[1]), SEEDS[1], k).tobytes() == fwd[1].tobytes()
    t = torch.zeros(dp, dtype=torch.float32, device="cuda")
    assert rp.rotate_vecs([dev(vals[2])], SEEDS[2], k, out=[t])[0] is t and host(t).tobytes() == fwd[2].tobytes()
    assert rp.rotate_vecs([t], [SEEDS[2]], k, inverse=True, out=[t])[0] is t and host(t).tobytes() == inv[2].tobytes()
    assert rp.unrotate(dev(fwd[0]), SEEDS[0], k, d).tobytes() == inv[0][:d].tobytes()
print("ROTATE_DEVICE PASS")
