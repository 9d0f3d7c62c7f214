"""The device accumulator (rofl_acc_*, DeviceAccumulator): a round's running sum of ElGamal pairs kept on the GPU, against the host-side
EncModelParamsAccumulator (one rofl_add_points_vec per client) and the independent oracle (tests/orc.py), bit for bit.

Updates are ElGamal pairs (L, R) = (m B + r B~, r B) made with commit_vec, the blindings of a round cancelling (generate_cancelling_scalar_vec),
so no proofs are needed: aggregation never looks at them."""
import ctypes
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

import orc

pytestmark = pytest.mark.gpu
FP = (32, 7)
BASEPOINT = bytes.fromhex("e2f2ae0a6abc4e71a884a961c500515f58e30b6aa582dd8db6a65945e08d2d76")


@pytest.fixture(scope="module")
def R():
    import rofl_project_code_amd as R
    from rofl_project_code_amd import build
    build.build()
    R.set_device(0)
    return R


def _round(R, n, d, seed, lo=-300, hi=300):
    """n clients' updates of d pairs: values k / 128 (k in [lo, hi)), blindings that sum to zero over the n clients"""
    rng = np.random.default_rng(seed)
    xs = [(rng.integers(lo, hi, size=d) / 128.0).astype(np.float32) for _ in range(n)]
    bls = []
    for _ in range(n - 1):
        b = rng.integers(0, 256, size=(d, 32), dtype=np.uint8); b[:, 31] &= 0x0F      # < 2^252: canonical
        bls.append(b)
    bls.append(R.pedersen_ops.add_scalar_vec(np.zeros((d, 32), np.uint8), R.pedersen_ops.add_scalar_vec_vec(bls), subtract=True))
    pairs = []
    for x, b in zip(xs, bls):
        m = R.conversion32.f32_to_scalar_vec(x, fp=FP)
        pairs.append(np.ascontiguousarray(np.concatenate([R.pedersen_ops.commit_vec(m, b), R.pedersen_ops.commit_no_blinding_vec(b)], axis=1)))
    return xs, pairs


def _range_msg(R, pairs):
    """an EncParamsRange holding the pairs (its proofs are not looked at by aggregation)"""
    return R.EncParamsRange(pairs, np.zeros((pairs.shape[0], 128), np.uint8), np.zeros((1, 608), np.uint8), 32, 1.0)


def _l2_msg(R, pairs):
    """serialised EncParamsL2 (SquareRandProofCommitments: the pair c, then c_sq), deserialised without a copy"""
    csq = np.tile(np.frombuffer(BASEPOINT, np.uint8), (pairs.shape[0], 1))
    ev = np.ascontiguousarray(np.concatenate([pairs, csq], axis=1))
    m = R.EncParamsL2(ev, np.zeros((pairs.shape[0], 192), np.uint8), np.zeros((1, 672), np.uint8), np.zeros(608, np.uint8), 32, 32)
    buf = m.serialize(as_array=True)
    got = R.EncParamsL2.deserialize(buf, copy=False)
    assert np.shares_memory(got.enc_values, buf) and (got.enc_values == ev).all()
    return got, buf


def _sum_f32(xs):
    return np.sum(np.stack(xs).astype(np.float64), axis=0).astype(np.float32)


def test_matches_the_host_accumulator_after_every_add_and_at_full_size(R):
    R.api.set_fp(*FP)
    xs, pairs = _round(R, 12, 20, 1)
    host, dev = R.EncModelParamsAccumulator.unity(20), R.DeviceAccumulator.unity(20)
    for c, p in enumerate(pairs):
        assert host.accumulate_other(_range_msg(R, p)) and dev.accumulate_other(_range_msg(R, p))
        assert (dev.export() == host.acc).all(), c
        if c < len(pairs) - 1:
            assert host.extract() is None and dev.extract() is None      # the blindings have not cancelled yet
    a, b = host.extract(), dev.extract()
    assert a is not None and a.tobytes() == b.tobytes() and a.tobytes() == _sum_f32(xs).tobytes()
    dev.close()
    d = 55000
    xs, pairs = _round(R, 12, d, 2)
    host = R.EncModelParamsAccumulator.unity(d)
    with R.DeviceAccumulator.unity(d) as dev:
        for p in pairs:
            host.accumulate_other(_range_msg(R, p))
            dev.accumulate_other(_range_msg(R, p))
        assert (dev.export() == host.acc).all()
        a, b = host.extract(), dev.extract()
        assert a.tobytes() == b.tobytes() == _sum_f32(xs).tobytes()
        for ts, bits in ((1 << 12, 16), (1 << 9, 16)):      # explicit tables: the same values as discrete_log_vec + scalar_to_f32_vec
            assert host.extract(ts, bits).tobytes() == dev.extract(ts, bits).tobytes()


def test_export_equals_a_fold_of_the_oracle(R):
    xs, pairs = _round(R, 5, 16, 3)
    with R.DeviceAccumulator.unity(16) as dev:
        dev.accumulate_batch([_range_msg(R, p) for p in pairs])
        acc = np.zeros((32, 32), np.uint8)
        for p in pairs:
            rc, acc = orc.add_points_vec(acc, p.reshape(-1, 32))
            assert rc == 0
        assert (dev.export().reshape(-1, 32) == acc).all()


def test_batched_single_and_concurrent_adds_agree(R):
    d = 300
    xs, pairs = _round(R, 12, d, 4)
    msgs = [_range_msg(R, p) for p in pairs]
    with R.DeviceAccumulator.unity(d) as a:
        a.accumulate_batch(msgs)
        ref, ref_x = a.export(), a.extract()
    assert ref_x.tobytes() == _sum_f32(xs).tobytes()
    for order in (list(range(12)), list(range(11, -1, -1)), list(np.random.default_rng(5).permutation(12))):
        with R.DeviceAccumulator.unity(d) as b:
            for i in order:
                b.accumulate_other(msgs[i])
            assert (b.export() == ref).all()
    # four threads on ONE accumulator (serialised by its lock), and four accumulators side by side on the lanes
    shared = R.DeviceAccumulator.unity(d)
    own = [R.DeviceAccumulator.unity(d) for _ in range(4)]
    errs = []

    def work(k):
        try:
            for i in range(k, 12, 4):
                shared.accumulate_other(msgs[i])
            own[k].accumulate_batch(msgs)
        except Exception as e:      # noqa: BLE001
            errs.append(e)
    ts = [threading.Thread(target=work, args=(k,)) for k in range(4)]
    [t.start() for t in ts]
    [t.join() for t in ts]
    assert not errs, errs
    assert (shared.export() == ref).all() and shared.extract().tobytes() == ref_x.tobytes()
    for o in own:
        assert (o.export() == ref).all()
        o.close()
    shared.close()


def test_l2_records_are_read_in_place(R):
    R.api.set_fp(*FP)
    d = 1000
    xs, pairs = _round(R, 6, d, 6)
    l2 = [_l2_msg(R, p) for p in pairs]
    host = R.EncModelParamsAccumulator.unity(d)
    for m, _ in l2:
        host.accumulate_other(m)
    with R.DeviceAccumulator.unity(d) as dev:
        dev.accumulate_batch([m for m, _ in l2])
        assert (dev.export() == host.acc).all()
        assert dev.extract().tobytes() == host.extract().tobytes() == _sum_f32(xs).tobytes()
    with R.DeviceAccumulator.unity(d) as dev:      # mixed containers in one batch: 64- and 96-byte records
        dev.accumulate_batch([l2[0][0], _range_msg(R, pairs[1])] + [m for m, _ in l2[2:]])
        assert (dev.export() == host.acc).all()


def test_zip_truncation(R):
    d = 40
    xs, pairs = _round(R, 4, 60, 7)
    lens = [60, 25, 40, 0]
    host = R.EncModelParamsAccumulator.unity(d)
    with R.DeviceAccumulator.unity(d) as dev:
        for p, n in zip(pairs, lens):
            host.accumulate_other(_range_msg(R, p[:n]))
        dev.accumulate_batch([_range_msg(R, p[:n]) for p, n in zip(pairs, lens)])
        assert (dev.export() == host.acc).all()
    # the C ABI's d_each: the same clients from their full arrays
    with R.DeviceAccumulator.unity(d) as dev:
        R.api.accumulator.add(dev._h, [p.ctypes.data for p in pairs], lens, 64)
        assert (dev.export() == host.acc).all()


def test_reference_unity(R):
    R.api.set_fp(*FP)
    d, n = 24, 5
    xs, pairs = _round(R, n, d, 8)
    B = np.frombuffer(BASEPOINT, np.uint8)
    with R.DeviceAccumulator.unity(d, reference_unity=True) as dev:
        dev.accumulate_batch([_range_msg(R, p) for p in pairs])
        got = dev.extract()
        ex = dev.export()
    # the oracle: sums that start from (B, B), unity check R == B, BSGS over the default table
    acc = np.tile(np.concatenate([B, B]), (d, 1))
    for p in pairs:
        rc, s = orc.add_points_vec(acc.reshape(-1, 32), p.reshape(-1, 32))
        assert rc == 0
        acc = s.reshape(d, 64)
    assert (ex == acc).all() and (acc[:, 32:] == B).all()
    rc, sc = orc.bsgs_solve(np.ascontiguousarray(acc[:, :32]), 1 << 15, 16)
    assert rc == 0
    want = np.array([orc.scalar_to_f32(sc[i], *FP) for i in range(d)], np.float32)
    assert got.tobytes() == want.tobytes()
    assert got.tobytes() == (_sum_f32(xs) + np.float32(1 / 128)).tobytes()
    with R.DeviceAccumulator.unity(d, reference_unity=True) as dev:      # R != B: the reference's None
        dev.accumulate_batch([_range_msg(R, p) for p in pairs[:-1]])
        assert dev.extract() is None
    with R.DeviceAccumulator.unity(d) as dev:      # (B, B) records into an init-0 accumulator: R == B is not the identity
        dev.accumulate_pairs(np.tile(np.concatenate([B, B]), (d, 1)))
        assert dev.extract() is None


def test_an_undecodable_record_leaves_the_sum_unchanged(R):
    d = 500
    xs, pairs = _round(R, 12, d, 9)
    msgs = [_range_msg(R, p) for p in pairs]
    with R.DeviceAccumulator.unity(d) as dev:
        dev.accumulate_batch(msgs[:3])
        before = dev.export()
        bad = pairs[5].copy(); bad[77, 32:] = 0xFF      # not a canonical field element
        with pytest.raises(R.RoflError) as e:
            dev.accumulate_batch(msgs[3:5] + [_range_msg(R, bad)] + msgs[6:])
        assert e.value.code == 5
        assert (dev.export() == before).all()
        bad2 = pairs[5].copy(); bad2[3, 0] |= 1      # a negative s: an invalid encoding
        with pytest.raises(R.RoflError) as e:
            dev.accumulate_other(_range_msg(R, bad2))
        assert e.value.code == 5 and (dev.export() == before).all()
        dev.accumulate_batch(msgs[3:])
        assert dev.extract().tobytes() == _sum_f32(xs).tobytes()


def test_device_tensor_records(R):
    """records handed over as a GPU torch tensor (torch in a child process, as the other device-pointer tests do)"""
    code = r"""
import os, sys
import numpy as np
import torch
torch.cuda.init()
sys.path.insert(0, %r); sys.path.insert(0, %r)
import rofl_project_code_amd as R
import test_gpu_accumulator as T
R.set_device(0); R.api.set_fp(32, 7)
xs, pairs = T._round(R, 6, 700, 10)
with R.DeviceAccumulator.unity(700) as a, R.DeviceAccumulator.unity(700) as b, R.DeviceAccumulator.unity(700) as c:
    for p in pairs:
        a.accumulate_pairs(p)
        b.accumulate_pairs(torch.from_numpy(p).cuda())
        ev = torch.from_numpy(np.ascontiguousarray(np.concatenate([p, p[:, :32]], axis=1))).cuda()
        c.accumulate_pairs(ev, stride=96)
    assert (a.export() == b.export()).all() and (a.export() == c.export()).all()
    assert a.extract().tobytes() == b.extract().tobytes() == T._sum_f32(xs).tobytes()
print("DEVICE_TENSOR PASS")
""" % (os.path.dirname(os.path.dirname(os.path.abspath(__file__))), os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "DEVICE_TENSOR PASS" in r.stdout, r.stdout + r.stderr[-3000:]


def test_partials_of_two_devices_merge(R):
    from rofl_project_code_amd import api
    api.map_device(1, 0)      # the box has one GPU: logical device 1 is a second full context on it
    d = 2000
    xs, pairs = _round(R, 12, d, 11)
    msgs = [_range_msg(R, p) for p in pairs]
    with R.DeviceAccumulator.unity(d) as whole:
        whole.accumulate_batch(msgs)
        try:
            R.set_device(1)
            part1 = R.DeviceAccumulator.unity(d)
        finally:
            R.set_device(0)
        part0 = R.DeviceAccumulator.unity(d)
        part0.accumulate_batch(msgs[:7])
        part1.accumulate_batch(msgs[7:])      # runs on logical device 1, whatever this thread is bound to
        with R.DeviceAccumulator.unity(d) as merged:
            merged.accumulate_pairs(part0.export())
            merged.accumulate_pairs(part1.export())
            assert (merged.export() == whole.export()).all()
            assert merged.extract().tobytes() == whole.extract().tobytes() == _sum_f32(xs).tobytes()
        part0.close(); part1.close()


def test_handles_after_destroy_and_no_leak(R):
    from rofl_project_code_amd import api
    L = api.lib()
    a = R.DeviceAccumulator.unity(64)
    h = a._h
    a.close()
    a.close()      # (the Python object frees once)
    assert L.rofl_acc_destroy(ctypes.c_uint64(h)) == 11
    assert L.rofl_acc_reset(ctypes.c_uint64(h)) == 11
    out = np.zeros((64, 64), np.uint8)
    assert L.rofl_acc_export(ctypes.c_uint64(h), out.ctypes.data_as(ctypes.c_void_p)) == 11
    with pytest.raises(R.RoflError) as e:
        a.export()
    assert e.value.code == 11
    with pytest.raises(R.RoflError) as e:
        a.accumulate_pairs(np.zeros((4, 64), np.uint8))
    assert e.value.code == 11
    with R.DeviceAccumulator.unity(64) as b:       # checks that need a live handle: stride, size overflow
        recs = (ctypes.c_void_p * 1)(out.ctypes.data)
        assert L.rofl_acc_add(ctypes.c_uint64(b._h), ctypes.c_size_t(1), recs, None, ctypes.c_size_t(32)) == 11
        assert L.rofl_acc_add(ctypes.c_uint64(b._h), ctypes.c_size_t(1 << 60), recs, None, ctypes.c_size_t(96)) == 11
    hip_path = next(ln.split()[-1] for ln in open("/proc/self/maps") if "libamdhip64" in ln)      # the HIP runtime the library runs on
    hip = ctypes.CDLL(hip_path)
    free, total = ctypes.c_size_t(), ctypes.c_size_t()

    def free_now():
        assert hip.hipMemGetInfo(ctypes.byref(free), ctypes.byref(total)) == 0
        return free.value
    for _ in range(3):      # warm: the lanes' workspaces
        R.DeviceAccumulator.unity(55000).close()
    f0 = free_now()
    for _ in range(200):
        R.DeviceAccumulator.unity(55000).close()
    assert abs(free_now() - f0) <= (1 << 20)


def test_multi_pass_add_across_point_tiles(R):
    """d past one point tile (131 072): every add takes the multi-pass path (work copy, tiles with j0 > 0, commit fold).  Checked after
    every add against the host-held class, with zip truncation across the tile boundary and a bad record in the second tile."""
    R.api.set_fp(*FP)
    d = 140000
    xs, pairs = _round(R, 3, d, 12)
    host = R.EncModelParamsAccumulator.unity(d)
    with R.DeviceAccumulator.unity(d) as dev:
        for c, p in enumerate(pairs):
            host.accumulate_other(_range_msg(R, p)); dev.accumulate_other(_range_msg(R, p))
            assert (dev.export() == host.acc).all(), c
        assert dev.extract().tobytes() == host.extract().tobytes() == _sum_f32(xs).tobytes()
        before = dev.export()
        bad = pairs[1].copy(); bad[135000, 32:] = 0xFF      # not a canonical field element, in the second tile
        with pytest.raises(R.RoflError) as e:
            dev.accumulate_batch([_range_msg(R, pairs[0]), _range_msg(R, bad), _range_msg(R, pairs[2])])
        assert e.value.code == 5 and (dev.export() == before).all()
        # clients that end inside the first tile, exactly at it, and in the second
        lens = [100000, 131072, 139999]
        for p, n in zip(pairs, lens):
            host.accumulate_other(_range_msg(R, p[:n]))
        dev.accumulate_batch([_range_msg(R, p[:n]) for p, n in zip(pairs, lens)])
        assert (dev.export() == host.acc).all()


def test_multi_pass_add_in_several_client_groups(R):
    """One add of more records than a group holds (33 x 131 072 = 4.3 M > 1.5 M: three groups, the staging buffers reused): equal to the
    merge of single-pass batches and to the sum of the known values; a bad record in the last group leaves the sum unchanged."""
    R.api.set_fp(*FP)
    d, n = 131072, 33
    xs, pairs = _round(R, n, d, 13, lo=-100, hi=100)
    msgs = [_range_msg(R, p) for p in pairs]
    with R.DeviceAccumulator.unity(d) as whole, R.DeviceAccumulator.unity(d) as merged:
        whole.accumulate_batch(msgs)
        for k in range(0, n, 11):      # 11 x 131 072 = 1.44 M records: single-pass batches
            with R.DeviceAccumulator.unity(d) as part:
                part.accumulate_batch(msgs[k:k + 11])
                merged.accumulate_pairs(part.export())
        ex = whole.export()
        assert (ex == merged.export()).all()
        assert whole.extract().tobytes() == _sum_f32(xs).tobytes()
        bad = pairs[31].copy(); bad[5, 0] |= 1      # a negative s: an invalid encoding
        with pytest.raises(R.RoflError) as e:
            whole.accumulate_batch(msgs[:31] + [_range_msg(R, bad), msgs[32]])
        assert e.value.code == 5 and (whole.export() == ex).all()
