"""Helper for test_gpu_l2_clip.py::test_memory_spaces_and_in_place: rofl_clip_l2 over GPU tensors (torch in a child process, as the other
device-pointer checks do) -- every combination of host and device inputs and outputs gives the model's bytes and scales and leaves the
inputs alone, a host vector, a device vector and a mixed one go through one call of three, in place works in both spaces, and the Python
wrappers take and return GPU tensors."""
import os, sys
import numpy as np
import torch
torch.cuda.init()
HERE = os.path.dirname(os.path.abspath(__file__)); sys.path.insert(0, os.path.dirname(HERE)); sys.path.insert(0, HERE)
import rofl_project_code_amd as R
import l2clip_model as M
from test_l2_clip_host import clip_call, inputs
R.set_device(0)
nb, fb, ff = 16, 16, 7
d = 2100
rng = np.random.default_rng(12)
seeds = [b"\x31" * 32, b"\x32" * 32, b"\x33" * 32]
vals = [inputs(rng, d, nb, fb, ff) for _ in seeds]
S = [M.sum_sq(v, nb, fb, ff) for v in vals]
T = [S[0], S[1] // 2, S[2] // 7]      # fits, scaled, scaled
dev = lambda a: torch.from_numpy(a.copy()).cuda()
host = lambda o: o.cpu().numpy() if hasattr(o, "cpu") else o
for seeded in (False, True):
    sb = b"".join(seeds) if seeded else None
    model = [M.clip_l2(v, t, nb, fb, ff, s if seeded else None) for v, t, s in zip(vals, T, seeds)]
    want, scales = [m[0].tobytes() for m in model], [m[1] for m in model]
    for in_dev in (False, True):
        for out_dev in (False, True):
            ins = [dev(v) if in_dev else v.copy() for v in vals]
            outs = [torch.zeros(d, dtype=torch.float32, device="cuda") if out_dev else np.zeros(d, np.float32) for _ in vals]
            rc, sc = clip_call(R.lib(), None if (in_dev or out_dev) else 1, sb, ins, d, T, nb, fb, ff, outs)      # (a device pointer always takes the kernels)
            assert rc == 0 and sc == scales and [host(o).tobytes() for o in outs] == want, (seeded, in_dev, out_dev)
            assert [host(i).tobytes() for i in ins] == [v.tobytes() for v in vals], "an input was written"
    # n_vec = 3 mixed within one call: device -> host, host -> device, host -> host
    ins = [dev(vals[0]), vals[1].copy(), vals[2].copy()]
    outs = [np.zeros(d, np.float32), torch.zeros(d, dtype=torch.float32, device="cuda"), np.zeros(d, np.float32)]
    rc, sc = clip_call(R.lib(), None, sb, ins, d, T, nb, fb, ff, outs)
    assert rc == 0 and sc == scales and [host(o).tobytes() for o in outs] == want
    # in place: a device vector and a host vector in one call
    t, h = dev(vals[1]), vals[2].copy()
    rc, sc = clip_call(R.lib(), None, sb[32:] if seeded else None, [t, h], d, T[1:], nb, fb, ff, [t, h])
    assert rc == 0 and sc == scales[1:] and [host(t).tobytes(), h.tobytes()] == want[1:]
    # the Python wrappers
    l2 = R.l2_range_proof_vec
    got, m = l2.clip_l2(dev(vals[1]), nb, T[1], seed=seeds[1] if seeded else None, fp=(fb, ff), with_scale=True)
    assert got.tobytes() == want[1] and m == scales[1]
    t = dev(vals[2])
    assert l2.clip_l2_vecs([t], nb, [T[2]], seeds=[seeds[2]] if seeded else None, fp=(fb, ff), out=[t])[0] is t and host(t).tobytes() == want[2]
print("L2_CLIP_DEVICE PASS")
