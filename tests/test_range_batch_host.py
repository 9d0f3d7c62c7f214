"""CPU-only checks of the server's L-inf round (rofl_verify_compressed_randproof_batch, EncParamsRange.verify_batch,
EncParamsRangeCompressed.verify_batch): the entry point is exported and declared in the header and in the Rust overlay, every bad
parameter answers 11 before a device is touched, the eight-lane transcript of the compressed randomness proof equals the scalar one, and
verify_batch's merge of its two legs -- run against canned leg results -- maps every verdict back to its client, sends off-shape members
and "split it" batches through verify(), and raises infrastructure errors instead of turning them into verdicts.  The GPU behaviour is in
test_gpu_range_batch.py."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FN = "rofl_verify_compressed_randproof_batch"
HOOK = "rofl_dbg_host_merlin8_lbl3_selftest"


def test_symbol_is_exported_and_declared(hiplib):
    hdr = open(os.path.join(ROOT, "include", "rofl_zk.h")).read()
    dbg = open(os.path.join(ROOT, "include", "rofl_zk_debug.h")).read()
    ffi = open(os.path.join(ROOT, "integration", "rofl_crypto_overlay", "src", "ffi.rs")).read()
    assert hasattr(hiplib, FN) and FN + "(" in hdr and "fn " + FN + "(" in ffi
    assert hasattr(hiplib, HOOK) and HOOK + "(" in dbg and HOOK + "(" not in hdr
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "check_ffi.py")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr


def test_parameter_checks_need_no_device(hiplib):
    """Each bad parameter is 11 (ROFL_BAD_PARAM), checked before the device is touched: run in a child process that sees no GPU.  An empty
    round is 0 without a device."""
    code = r"""
import ctypes
L = ctypes.CDLL(%r)
sz, p = ctypes.c_size_t, ctypes.c_void_p
proof = ctypes.create_string_buffer(128); pairs = ctypes.create_string_buffer(64 * 4)
P = (p * 2)(ctypes.addressof(proof), ctypes.addressof(proof)); C = (p * 2)(ctypes.addressof(pairs), ctypes.addressof(pairs))
P0 = (p * 2)(ctypes.addressof(proof), None); C0 = (p * 2)(ctypes.addressof(pairs), None)
ok = (ctypes.c_int * 4)(7, 7, 7, 7)
F = L.rofl_verify_compressed_randproof_batch
rcs = {
    "d = 900 000": F(sz(2), P, C, sz(900000), ok),
    "d = 2^40": F(sz(2), P, C, sz(1 << 40), ok),
    "null proofs": F(sz(2), None, C, sz(4), ok),
    "null pairs": F(sz(2), P, None, sz(4), ok),
    "null ok_out": F(sz(2), P, C, sz(4), None),
    "a null proof": F(sz(2), P0, C, sz(4), ok),
    "a null pair vector": F(sz(2), P, C0, sz(4), ok),
    "32 768 clients: 65 536 problems": F(sz(32768), P, C, sz(4), ok),
    "2^62 clients": F(sz(1 << 62), P, C, sz(4), ok),
}
bad = {k: v for k, v in rcs.items() if v != 11}
assert not bad, bad
assert F(sz(0), None, None, sz(4), ok) == 0 and F(sz(0), P, C, sz(0), ok) == 0
print("compressed batch params ok", len(rcs))
""" % hiplib._name
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")      # whatever the host has: no device is reachable
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "compressed batch params ok 9" in r.stdout, r.stdout + r.stderr[-2000:]


def test_x8_triplet_label_transcripts_match_the_scalar_ones(hiplib):
    """keccak_x8.hpp append_lbl3_run_x8 (eight CompressedRandProof transcripts per AVX-512 stream) against Merlin::append_lbl one pair at a
    time: every lane count, records crossing the rate block at every offset, d = 1, 37 and 40 000; state bytes, positions and the challenge
    drawn after C' compared.  Skipped on a CPU without AVX-512, where the library keeps the scalar sponge."""
    f = getattr(hiplib, HOOK)
    if f(8, 1, 0, None, None) == -1:
        pytest.skip("no AVX-512 on this CPU")
    for d in (1, 37):
        for lanes in range(1, 9):
            assert [s for s in range(0, 170) if f(lanes, d, s, None, None)] == [], (lanes, d)
    for lanes in range(1, 9):
        assert f(lanes, 40000, 3 * lanes, None, None) == 0, lanes
    assert f(0, 8, 0, None, None) == 11 and f(9, 8, 0, None, None) == 11


# ---- verify_batch's merge of its two legs, against canned leg results
class _Legs:
    """Stand-ins for the api legs.  A member's identity is the byte its arrays are filled with; bad_rand / bad_range say which members each
    leg rejects.  Batched and single calls are recorded; the batched randomness leg raises `fail` when it is set."""

    def __init__(self, bad_rand=(), bad_range=(), fail=None):
        self.bad_rand, self.bad_range, self.fail = set(bad_rand), set(bad_range), fail
        self.batches, self.singles = [], []

    def _rand_batch(self, pairs_list):
        ids = [int(c[0, 0]) for c in pairs_list]
        self.batches.append(("rand", ids))
        if self.fail is not None:
            raise self.fail
        return [i not in self.bad_rand for i in ids]

    def _rand_one(self, pairs):
        i = int(np.asarray(pairs).reshape(-1)[0])
        self.singles.append(("rand", i))
        return i not in self.bad_rand

    # rand_proof_vec / compressed_rand_proof
    def verify_randproof_vec_batch(self, proofs_list, pairs_list):
        assert all(p.shape[0] == c.shape[0] for p, c in zip(proofs_list, pairs_list))
        return self._rand_batch(pairs_list)

    def helper_verify_batch(self, proofs, pairs_list):
        assert all(np.asarray(p).size == 128 for p in proofs)
        return self._rand_batch(pairs_list)

    def verify_randproof_vec(self, proofs, pairs):
        from rofl_project_code_amd.api import RoflError
        if np.asarray(proofs).reshape(-1, 128).shape[0] != np.asarray(pairs).reshape(-1, 64).shape[0]:
            raise RoflError(1, "WrongNumberOfElGamalPairs")
        return self._rand_one(pairs)

    def helper_verify(self, proof, pairs):
        return self._rand_one(pairs)

    # range_proof_vec
    def verify_rangeproof_batch(self, proofs_list, commits_list, prove_range, verifier_seed=None, fp=None, commit_stride=32):
        assert commit_stride == 64 and all(c.ndim == 2 and c.shape[1] == 64 for c in commits_list)
        ids = [int(p[0, 0]) for p in proofs_list]
        self.batches.append(("range", ids, [c.shape[0] for c in commits_list]))
        return [i not in self.bad_range for i in ids]

    def verify_rangeproof(self, proofs, commits, prove_range, verifier_seed=None, fp=None):
        i = int(proofs[0, 0])
        self.singles.append(("range", i))
        return i not in self.bad_range


def _update(compressed, i, d=40, check=1.0, rand_rows=None, P=2):
    from rofl_project_code_amd import params
    ev = np.full((d, 64), i, np.uint8)
    rp = np.full((P, 608), i, np.uint8)
    if compressed:
        return params.EncParamsRangeCompressed(ev, np.full(128, i, np.uint8), rp, 8, check)
    return params.EncParamsRange(ev, np.full((d if rand_rows is None else rand_rows, 128), i, np.uint8), rp, 8, check)


@pytest.fixture
def legs(monkeypatch):
    from rofl_project_code_amd import params
    monkeypatch.setattr(params, "_concurrently", lambda *thunks: [t() for t in thunks])

    def install(fake):
        for name in ("rand_proof_vec", "compressed_rand_proof", "range_proof_vec"):
            monkeypatch.setattr(params, name, fake)
        return fake
    return install


def _cls(compressed):
    from rofl_project_code_amd import params
    return params.EncParamsRangeCompressed if compressed else params.EncParamsRange


@pytest.mark.parametrize("compressed", [False, True], ids=["Range", "RangeCompressed"])
def test_verdict_is_the_and_of_both_legs_per_client(legs, compressed):
    cls = _cls(compressed)
    fake = legs(_Legs(bad_rand={11, 14}, bad_range={12, 14}))
    ups = [_update(compressed, i, check=0.25) for i in (10, 11, 12, 13, 14, 15)]
    got = cls.verify_batch(ups, verifier_seed=b"\x01" * 32, fp=(16, 7))
    assert got == [True, False, False, True, False, True]
    # one call per leg for the whole round, in the clients' order, nothing client by client; the range leg gets the first k = 10 of 40 pairs
    assert fake.batches == [("rand", [10, 11, 12, 13, 14, 15]), ("range", [10, 11, 12, 13, 14, 15], [10] * 6)] and fake.singles == []
    assert got == [u.verify(verifier_seed=b"\x01" * 32, fp=(16, 7)) for u in ups]
    fake.batches.clear(); fake.singles.clear()
    assert cls.verify_batch(ups[::-1], fp=(16, 7)) == got[::-1] and fake.singles == []
    assert cls.verify_batch([], fp=(16, 7)) == []


def test_range_leg_reads_the_pairs_in_place(legs, monkeypatch):
    from rofl_project_code_amd import params
    seen = []
    fake = legs(_Legs())
    real = fake.verify_rangeproof_batch

    def spy(proofs_list, commits_list, *a, **kw):
        seen.extend(commits_list)
        return real(proofs_list, commits_list, *a, **kw)
    monkeypatch.setattr(fake, "verify_rangeproof_batch", spy)
    ups = [_update(True, i, check=0.5) for i in range(3)]
    assert params.EncParamsRangeCompressed.verify_batch(ups, fp=(16, 7)) == [True] * 3
    assert [c.shape for c in seen] == [(20, 64)] * 3 and all(np.shares_memory(c, u.enc_values) for c, u in zip(seen, ups))


@pytest.mark.parametrize("compressed", [False, True], ids=["Range", "RangeCompressed"])
def test_off_shape_members_go_through_verify(legs, compressed, monkeypatch):
    cls = _cls(compressed)
    fake = legs(_Legs(bad_range={3}))
    ups = [_update(compressed, i) for i in range(5)]
    ups.append(_update(compressed, 40, d=41))                 # another d
    ups.append(_update(compressed, 41, P=3))                  # another range-proof shape
    ups.append(_update(compressed, 42, check=0.5))            # another k
    ups.append(_update(compressed, 43, check=float("nan")))   # a check_percentage _num_checked rejects: verify() says False
    if compressed:
        odd = _update(True, 44)
        odd.rand_proof = np.full(96, 44, np.uint8)            # a proof of the wrong size
        ups.append(odd)
    else:
        ups.append(_update(False, 44, rand_rows=39))          # one rand proof short
    called = []
    real = cls.verify

    def spy(self, verifier_seed=None, fp=None):
        called.append(int(self.enc_values[0, 0]))
        return real(self, verifier_seed=verifier_seed, fp=fp)
    monkeypatch.setattr(cls, "verify", spy)
    got = cls.verify_batch(ups, fp=(16, 7))
    assert got == [True, True, True, False, True, True, True, True, False, False]
    assert sorted(called) == [40, 41, 42, 43, 44]
    assert [b[1] for b in fake.batches] == [[0, 1, 2, 3, 4]] * 2


@pytest.mark.parametrize("compressed", [False, True], ids=["Range", "RangeCompressed"])
def test_split_it_falls_back_to_per_client_verification(legs, compressed):
    from rofl_project_code_amd.api import RoflError
    fake = legs(_Legs(bad_rand={2}, bad_range={4}, fail=RoflError(11, "batch too large (split it)")))
    ups = [_update(compressed, i) for i in range(6)]
    assert _cls(compressed).verify_batch(ups, fp=(16, 7)) == [True, True, False, True, False, True]
    assert sorted({i for _, i in fake.singles}) == [0, 1, 2, 3, 4, 5]


@pytest.mark.parametrize("compressed", [False, True], ids=["Range", "RangeCompressed"])
def test_infrastructure_errors_are_raised_not_verdicts(legs, compressed):
    from rofl_project_code_amd.api import RoflError
    legs(_Legs(fail=RoflError(99, "HIP error 1 (invalid argument) in kernel launch")))
    with pytest.raises(RoflError) as e:
        _cls(compressed).verify_batch([_update(compressed, i) for i in range(4)], fp=(16, 7))
    assert e.value.code == 99


def test_helper_verify_batch_rejects_malformed_members_without_the_library(monkeypatch):
    """Members whose arrays have the wrong shape are False before any call; the others are grouped by d, one call per group."""
    from rofl_project_code_amd import api
    calls = []

    class FakeLib:
        def rofl_verify_compressed_randproof_batch(self, n, pp, cp, d, ok):
            calls.append((n.value, d.value))
            for k in range(n.value):
                ok[k] = 1
            return 0
    monkeypatch.setattr(api, "lib", lambda: FakeLib())
    pf = np.zeros(128, np.uint8)
    got = api.compressed_rand_proof.helper_verify_batch(
        [pf, pf, np.zeros(127, np.uint8), pf, pf, pf],
        [np.zeros((5, 64), np.uint8), np.zeros((7, 64), np.uint8), np.zeros((5, 64), np.uint8), np.zeros(320, np.uint8),
         np.zeros((5, 64), np.uint8), np.zeros((0, 64), np.uint8)])
    assert got == [True, True, False, False, True, True]
    assert sorted(calls) == [(1, 0), (1, 7), (2, 5)]
    assert api.compressed_rand_proof.helper_verify_batch([], []) == []
    with pytest.raises(ValueError):
        api.compressed_rand_proof.helper_verify_batch([pf], [])
