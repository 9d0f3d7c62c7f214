"""Worker of tests/test_gpu_devices_dispatch.py (a process of its own per call, so that logical device 1 holds no generator tables before
the call under test).

  gpu_devices_dispatch_worker.py batch_create | batch_verify | single_create | batch_of_one

rofl_set_option("devices", 0b10) with the calling thread on device 0 (logical device 1 is mapped onto the same GPU): the call runs on
device 1 -- that device has the generator tables of the shape afterwards and had none before --, returns what the devices = 0 call
returns, and the calling thread is on device 0 when it comes back.  d = 70, 8-bit range, two chunks of 64 values, fp 32/7.
Prints 'one device ok: <call>' and exits 0."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    call = sys.argv[1]
    import orc
    import rofl_project_code_amd as R
    from rofl_project_code_amd import api
    api.map_device(1, 0)
    R.set_device(0)
    fp = (32, 7); d, nb, P = 70, 8, 2
    m = 128 // P                      # values per chunk: the generator tables of the shape are those of (nb, m)
    ins = []
    for i in range(2):
        rng = np.random.default_rng(8200 + i)
        ins.append(((rng.integers(-100, 100, size=d) / 128.0).astype(np.float32), orc.rand_scalars(rng, d)))
    xs, bls = [v for v, _ in ins], [b for _, b in ins]
    nonces = lambda: [R.Nonce.seeded(bytes([0x61 + i]) * 32) for i in range(2)]      # noqa: E731
    same = lambda a, b: all((x[0] == y[0]).all() and (x[1] == y[1]).all() for x, y in zip(a, b))      # noqa: E731
    runs = {
        "batch_create": lambda: R.range_proof_vec.create_rangeproof_batch(xs, bls, nb, P, nonces=nonces(), fp=fp),
        "batch_of_one": lambda: R.range_proof_vec.create_rangeproof_batch(xs[:1], bls[:1], nb, P, nonces=nonces()[:1], fp=fp),
        "single_create": lambda: [R.range_proof_vec.create_rangeproof(xs[0], bls[0], nb, P, nonce=nonces()[0], fp=fp)],
    }
    if call == "batch_verify":        # two clients' proofs, one of them tampered: the verdicts of the devices = 0 call
        made = runs["batch_create"]()
        proofs = [p.copy() for p, _ in made]; commits = [c for _, c in made]
        proofs[1][1, 70] ^= 1
        run = lambda: R.range_proof_vec.verify_rangeproof_batch(proofs, commits, nb, verifier_seed=b"\x05" * 32, fp=fp)      # noqa: E731
        same = lambda a, b: a == b == [True, False]      # noqa: E731
    else:
        run = runs[call]
    want = run()                      # devices = 0: on device 0
    R.set_device(1); before = api.bp_gens_table_bytes(nb, m)
    R.set_device(0); here = api.bp_gens_table_bytes(nb, m)
    assert before == 0 and here > 0, (before, here)
    R.set_option("devices", 0b10)
    try:
        got = run()
        assert api.get_device() == 0, "the binding leaked"
    finally:
        R.set_option("devices", 0)
    assert same(got, want), "devices = 0b10 differs from devices = 0"
    R.set_device(1); after = api.bp_gens_table_bytes(nb, m)
    R.set_device(0)
    assert after > 0, "the call did not run on the listed device"
    print("one device ok: %s (tables on device 1: %d bytes)" % (call, after))


if __name__ == "__main__":
    main()
