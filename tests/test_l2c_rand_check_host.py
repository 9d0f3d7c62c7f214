"""CPU-only checks of the opt-in CompressedRandProof check of EncL2Compressed updates (rofl_verify_compressed_randproof_batch_strided,
rofl_round_create_rand, api.compressed_rand_proof.helper_verify_batch_strided, api.device_round.create_rand, EncParamsL2CompressedStrict):
the symbols are exported and declared, every parameter check answers 11 before a device is touched, the Python layer has the documented
signatures, and the eight-lane transcript over 96-byte records equals the scalar one over the packed pairs.  The GPU behaviour is in
test_gpu_l2c_rand_check.py."""
import inspect
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_FUNCS = ("rofl_verify_compressed_randproof_batch_strided", "rofl_round_create_rand")
HOOK = "rofl_dbg_host_merlin8_lbl3_strided_selftest"


def test_symbols_are_exported_and_declared(hiplib):
    hdr = open(os.path.join(ROOT, "include", "rofl_zk.h")).read()
    dbg = open(os.path.join(ROOT, "include", "rofl_zk_debug.h")).read()
    ffi = open(os.path.join(ROOT, "integration", "rofl_crypto_overlay", "src", "ffi.rs")).read()
    for n in NEW_FUNCS:
        assert hasattr(hiplib, n), n
        assert n + "(" in hdr and "fn " + n + "(" in ffi, n
    assert hasattr(hiplib, HOOK) and HOOK + "(" in dbg and HOOK + "(" not in hdr
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "check_ffi.py")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and " 0 differences" in r.stdout, r.stdout + r.stderr


def test_parameter_checks_need_no_device(hiplib):
    """Each bad parameter of both new functions is 11 (ROFL_BAD_PARAM), answered before the device is touched: run in a child process that
    sees no GPU.  An empty call is 0 without a device; rofl_round_create_ex still refuses 96-byte records with the flag."""
    code = r"""
import ctypes
L = ctypes.CDLL(%r)
sz, u64, p, un = ctypes.c_size_t, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint
proof = ctypes.create_string_buffer(128); recs = ctypes.create_string_buffer(128 * 4)
P = (p * 2)(ctypes.addressof(proof), ctypes.addressof(proof)); C = (p * 2)(ctypes.addressof(recs), ctypes.addressof(recs))
P0 = (p * 2)(ctypes.addressof(proof), None); C0 = (p * 2)(ctypes.addressof(recs), None)
ok = (ctypes.c_int * 4)(7, 7, 7, 7)
h = ctypes.c_uint64(0)
cnt = ctypes.c_uint64(123)
F, G = L.rofl_verify_compressed_randproof_batch_strided, L.rofl_round_create_rand
rcs = {
    "stride 32": F(sz(2), P, C, sz(32), sz(4), ok),
    "stride 128": F(sz(2), P, C, sz(128), sz(4), ok),
    "stride 0": F(sz(2), P, C, sz(0), sz(4), ok),
    "stride 32, no clients": F(sz(0), None, None, sz(32), sz(4), ok),
    "d = 900 000, stride 96": F(sz(2), P, C, sz(96), sz(900000), ok),
    "d = 900 000, stride 64": F(sz(2), P, C, sz(64), sz(900000), ok),
    "d = 2^40": F(sz(2), P, C, sz(96), sz(1 << 40), ok),
    "null proofs": F(sz(2), None, C, sz(96), sz(4), ok),
    "null records": F(sz(2), P, None, sz(96), sz(4), ok),
    "null ok_out": F(sz(2), P, C, sz(96), sz(4), None),
    "a null proof": F(sz(2), P0, C, sz(96), sz(4), ok),
    "a null record vector": F(sz(2), P, C0, sz(96), sz(4), ok),
    "32 768 clients": F(sz(32768), P, C, sz(96), sz(4), ok),
    "2^62 clients": F(sz(1 << 62), P, C, sz(64), sz(4), ok),
    "create_rand record_len 32": G(sz(8), sz(32), sz(4), ctypes.byref(h)),
    "create_rand record_len 128": G(sz(8), sz(128), sz(4), ctypes.byref(h)),
    "create_rand d = 0": G(sz(0), sz(96), sz(4), ctypes.byref(h)),
    "create_rand d = 900000, 96": G(sz(900000), sz(96), sz(4), ctypes.byref(h)),
    "create_rand d = 900000, 64": G(sz(900000), sz(64), sz(4), ctypes.byref(h)),
    "create_rand max_clients 0": G(sz(8), sz(96), sz(0), ctypes.byref(h)),
    "create_rand too many clients": G(sz(8), sz(96), sz(1 << 20), ctypes.byref(h)),
    "create_rand null out, 96": G(sz(8), sz(96), sz(4), None),
    "create_rand null out, 64": G(sz(8), sz(64), sz(4), None),
    "create_ex flag 1, record_len 96 (unchanged)": L.rofl_round_create_ex(sz(8), sz(96), sz(4), un(1), ctypes.byref(h)),
}
bad = {k: v for k, v in rcs.items() if v != 11}
assert not bad, bad
assert F(sz(0), None, None, sz(96), sz(4), ok) == 0 and F(sz(0), P, C, sz(64), sz(0), ok) == 0
assert h.value == 0 and list(ok) == [7, 7, 7, 7]
assert L.rofl_dbg_point_decodes(ctypes.byref(cnt)) == 0 and cnt.value == 0      # nothing was handed to a device
print("l2c rand check params ok", len(rcs))
""" % hiplib._name
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")      # whatever the host has: no device is reachable
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "l2c rand check params ok 24" in r.stdout, r.stdout + r.stderr[-2000:]


def test_python_layer_has_the_documented_signatures():
    import rofl_project_code_amd as R
    from rofl_project_code_amd import api, params
    assert list(inspect.signature(api.compressed_rand_proof.helper_verify_batch_strided).parameters) == ["proofs_list", "records_list", "stride"]
    assert list(inspect.signature(api.compressed_rand_proof.helper_verify_batch).parameters) == ["proofs", "pairs_list"]      # the dense one is as it was
    assert list(inspect.signature(api.device_round.create_rand).parameters) == ["d", "record_len", "max_clients"]
    S, B = R.EncParamsL2CompressedStrict, R.EncParamsL2Compressed
    assert S is params.EncParamsL2CompressedStrict and issubclass(S, B) and S is not B
    assert S.kind == B.kind == params.WIRE_ENC_NORM_COMPRESSED
    for name in ("__init__", "encrypt", "encrypt_batch", "serialize", "deserialize", "verify", "verify_batch"):
        assert list(inspect.signature(getattr(S, name)).parameters) == list(inspect.signature(getattr(B, name)).parameters), name
    p = inspect.signature(S.verify_batch).parameters
    assert list(p) == ["updates", "verifier_seed", "fp", "_legs"] and p["verifier_seed"].default is None and p["fp"].default is None
    # the same constructor, the same bytes: only the class differs
    z = S(np.zeros((2, 96), np.uint8), np.zeros((2, 160), np.uint8), np.zeros(128, np.uint8), np.zeros((1, 8), np.uint8), np.zeros(8, np.uint8), 8, 32)
    assert type(z) is S and z.enc_values.shape == (2, 96) and z.rand_proof.shape == (128,)
    assert S._checks_rand and not B._checks_rand and not params.EncParamsL2._checks_rand
    doc = " ".join(B.verify.__doc__.split())
    assert "EncParamsL2CompressedStrict" in doc and "not re-checked" not in doc
    assert "EncParamsL2CompressedStrict" in " ".join(R.DeviceRound.__doc__.split())


def test_helper_verify_batch_strided_rejects_malformed_members_without_the_library(monkeypatch):
    """Members whose arrays have the wrong shape are False before any call; the others are grouped by d, one call per group, with the
    stride handed on."""
    from rofl_project_code_amd import api
    calls = []

    class FakeLib:
        def rofl_verify_compressed_randproof_batch_strided(self, n, pp, cp, stride, d, ok):
            calls.append((n.value, stride.value, d.value))
            for k in range(n.value):
                ok[k] = 1
            return 0
    monkeypatch.setattr(api, "lib", lambda: FakeLib())
    pf = np.zeros(128, np.uint8)
    got = api.compressed_rand_proof.helper_verify_batch_strided(
        [pf, pf, np.zeros(127, np.uint8), pf, pf, pf, pf],
        [np.zeros((5, 96), np.uint8), np.zeros((7, 96), np.uint8), np.zeros((5, 96), np.uint8), np.zeros(480, np.uint8),
         np.zeros((5, 96), np.uint8), np.zeros((0, 96), np.uint8), np.zeros((5, 64), np.uint8)], 96)
    assert got == [True, True, False, False, True, True, False]
    assert sorted(calls) == [(1, 96, 0), (1, 96, 7), (2, 96, 5)]
    assert api.compressed_rand_proof.helper_verify_batch_strided([], [], 96) == []
    with pytest.raises(ValueError):
        api.compressed_rand_proof.helper_verify_batch_strided([pf], [], 96)
    for stride in (32, 128):
        with pytest.raises(api.RoflError) as e:
            api.compressed_rand_proof.helper_verify_batch_strided([pf], [np.zeros((5, stride), np.uint8)], stride)
        assert e.value.code == 11


def test_strided_x8_transcripts_match_the_scalar_ones_over_the_packed_pairs(hiplib):
    """keccak_x8.hpp append_lbl3_run_x8 over 96-byte records (the last 32 bytes of every record filled with bytes that differ per lane)
    against Merlin::append_lbl over the first 64 bytes of each record: lanes 5 to 8 (the counts at which compressed_prefixes takes the
    x8 path), counts 0 to 9 and 1000, records crossing the rate block at every offset; state bytes, positions and the challenge drawn after
    C' compared.  Stride 64 is the dense hook's case.  Skipped on a CPU without AVX-512, where the library keeps the scalar sponge."""
    f = getattr(hiplib, HOOK)
    if f(8, 1, 0, 96, None, None) == -1:
        pytest.skip("no AVX-512 on this CPU")
    for lanes in range(5, 9):
        for count in list(range(0, 10)) + [1000]:
            skews = range(0, 170) if count < 10 else (0, 3 * lanes, 167)
            assert [s for s in skews if f(lanes, count, s, 96, None, None)] == [], (lanes, count)
        assert f(lanes, 9, 5, 64, None, None) == 0 and f(lanes, 9, 5, 80, None, None) == 0
    assert f(0, 8, 0, 96, None, None) == 11 and f(9, 8, 0, 96, None, None) == 11
    assert f(8, 8, 0, 63, None, None) == 11 and f(8, 8, 0, 257, None, None) == 11 and f(8, 8, 401, 96, None, None) == 11


# ---- the Python layer against canned legs: which legs run for which class, and how their verdicts merge
class _FakeLegs:
    """Stand-in for the `_legs` of verify_batch.  A member's identity is the byte its enc_values are filled with; bad_* say which
    members each leg rejects; the randomness leg raises `fail` when it is set."""

    def __init__(self, bad_rand=(), bad_sq=(), bad_range=(), fail=None):
        self.bad_rand, self.bad_sq, self.bad_range, self.fail = set(bad_rand), set(bad_sq), set(bad_range), fail
        self.calls = []

    @staticmethod
    def _ids(us):
        return [int(u.enc_values[0, 0]) for u in us]

    def rand(self, cls, us, idx):
        self.calls.append(("rand", self._ids(us)))
        if self.fail is not None:
            raise self.fail
        return [i not in self.bad_rand for i in self._ids(us)]

    def square(self, cls, us, idx):
        self.calls.append(("square", self._ids(us)))
        return [i not in self.bad_sq for i in self._ids(us)], np.zeros((len(us), 32), np.uint8)

    def range(self, us, idx, k, prove_range, seed, fp, stride):
        assert stride == 96 and k == us[0].enc_values.shape[0]
        self.calls.append(("range", self._ids(us)))
        return [i not in self.bad_range for i in self._ids(us)]


def _l2c(cls, i, d=12, rand_len=128):
    return cls(np.full((d, 96), i, np.uint8), np.full((d, 160), i, np.uint8), np.full(rand_len, i, np.uint8), np.full((2, 608), i, np.uint8),
               np.full(608, i, np.uint8), 8, 32)


@pytest.fixture
def canned(monkeypatch):
    from rofl_project_code_amd import params
    monkeypatch.setattr(params, "_concurrently", lambda *thunks: [t() for t in thunks])

    class _Sum:
        @staticmethod
        def verify_rangeproof_l2_batch(proofs, sums, prove_range, verifier_seed=None, fp=None):
            return [True] * len(proofs)
    monkeypatch.setattr(params, "l2_range_proof_vec", _Sum)
    return params


def test_verify_batch_runs_the_randomness_leg_for_the_strict_class_only(canned):
    S, B = canned.EncParamsL2CompressedStrict, canned.EncParamsL2Compressed
    for cls in (S, B):
        legs = _FakeLegs(bad_rand={11, 14}, bad_sq={12}, bad_range={14, 15})
        ups = [_l2c(cls, i) for i in (10, 11, 12, 13, 14, 15)]
        got = cls.verify_batch(ups, fp=(32, 7), _legs=legs)
        kinds = sorted(c[0] for c in legs.calls)
        if cls is S:
            assert got == [True, False, False, True, False, False]
            assert kinds == ["rand", "range", "square"] and all(c[1] == [10, 11, 12, 13, 14, 15] for c in legs.calls)
        else:      # the reference's arm: no randomness leg, the verdicts it always gave
            assert got == [True, True, False, True, False, False]
            assert kinds == ["range", "square"]
        assert cls.verify_batch([], fp=(32, 7), _legs=legs) == []


def test_a_member_with_a_proof_of_another_size_is_verified_on_its_own(canned, monkeypatch):
    S, B = canned.EncParamsL2CompressedStrict, canned.EncParamsL2Compressed
    called = []
    monkeypatch.setattr(B, "verify", lambda self, verifier_seed=None, fp=None: called.append(int(self.enc_values[0, 0])) or False)
    legs = _FakeLegs()
    ups = [_l2c(S, i) for i in range(4)] + [_l2c(S, 40, rand_len=127), _l2c(S, 41, d=13)]
    assert S.verify_batch(ups, fp=(32, 7), _legs=legs) == [True] * 4 + [False, False]
    assert sorted(called) == [40, 41] and all(c[1] == [0, 1, 2, 3] for c in legs.calls)
    # a round of nothing but 127-byte proofs has no majority shape: every member on its own
    called.clear(); legs.calls.clear()
    assert S.verify_batch([_l2c(S, i, rand_len=127) for i in range(3)], fp=(32, 7), _legs=legs) == [False] * 3
    assert sorted(called) == [0, 1, 2] and legs.calls == []
    # the reference-faithful class never looked at the proof's size: the member stays in the batch
    called.clear(); legs.calls.clear()
    assert B.verify_batch([_l2c(B, i) for i in range(4)] + [_l2c(B, 40, rand_len=127)], fp=(32, 7), _legs=legs) == [True] * 5
    assert called == []


def test_the_randomness_leg_keeps_the_error_policy(canned, monkeypatch):
    from rofl_project_code_amd.api import RoflError
    S = canned.EncParamsL2CompressedStrict
    ups = [_l2c(S, i) for i in range(4)]
    with pytest.raises(RoflError) as e:      # a HIP error is raised, never a verdict
        S.verify_batch(ups, fp=(32, 7), _legs=_FakeLegs(fail=RoflError(99, "HIP error 1 (invalid argument) in kernel launch")))
    assert e.value.code == 99
    called = []
    monkeypatch.setattr(S, "verify", lambda self, verifier_seed=None, fp=None: called.append(int(self.enc_values[0, 0])) or True)
    assert S.verify_batch(ups, fp=(32, 7), _legs=_FakeLegs(fail=RoflError(11, "batch too large (split it)"))) == [True] * 4
    assert sorted(called) == [0, 1, 2, 3]      # a parameter of the batched call: client by client


def test_strict_verify_is_the_and_of_four_legs(canned, monkeypatch):
    """verify() of the strict class: the three legs of EncParamsL2Compressed and the strided call over enc_values in place (stride 96)"""
    from rofl_project_code_amd.api import RoflError
    S, B = canned.EncParamsL2CompressedStrict, canned.EncParamsL2Compressed
    seen = []

    class _Sq:
        @staticmethod
        def verify_l2rangeproof_vec(proofs, commits):
            return True

    class _Rg:
        @staticmethod
        def verify_rangeproof(proofs, commits, prove_range, verifier_seed=None, fp=None):
            return True

    class _L2:
        @staticmethod
        def verify_rangeproof_l2(proof, commit, prove_range, verifier_seed=None, fp=None):
            return True

    class _Comp:
        verdict = True

        @classmethod
        def helper_verify_batch_strided(cls, proofs_list, records_list, stride):
            seen.append((len(proofs_list), records_list[0], stride))
            if isinstance(cls.verdict, Exception):
                raise cls.verdict
            return [cls.verdict]
    for name, fake in (("square_proof_vec", _Sq), ("range_proof_vec", _Rg), ("l2_range_proof_vec", _L2), ("compressed_rand_proof", _Comp)):
        monkeypatch.setattr(canned, name, fake)
    monkeypatch.setattr(B, "_sum_c_sq", lambda self: np.zeros(32, np.uint8))
    u, v = _l2c(S, 7), _l2c(B, 7)
    assert u.verify(fp=(32, 7)) is True and v.verify(fp=(32, 7)) is True
    assert len(seen) == 1 and seen[0][0] == 1 and seen[0][1] is u.enc_values and seen[0][2] == 96      # in place, and only for the strict class
    _Comp.verdict = False
    assert u.verify(fp=(32, 7)) is False and v.verify(fp=(32, 7)) is True
    _Comp.verdict = RoflError(11, "bad parameter")      # what d >= 900 000 gets: the message's fault
    assert u.verify(fp=(32, 7)) is False
    _Comp.verdict = RoflError(99, "HIP error")
    with pytest.raises(RoflError):
        u.verify(fp=(32, 7))


def test_device_round_creates_the_round_its_class_needs(monkeypatch):
    """DeviceRound of the strict class keeps the transcripts (rofl_round_create_rand, 96-byte records) and runs its randomness leg over
    the cache; past d = 900 000 it keeps the host call; DeviceRound of EncParamsL2Compressed is created as before."""
    from rofl_project_code_amd import api, params
    made = []
    monkeypatch.setattr(api.device_round, "create", staticmethod(lambda d, record_len, max_clients, flags=0: made.append(("create", d, record_len, max_clients, flags)) or 1))
    monkeypatch.setattr(api.device_round, "create_rand", staticmethod(lambda d, record_len, max_clients: made.append(("create_rand", d, record_len, max_clients)) or 2))
    monkeypatch.setattr(api.device_round, "destroy", staticmethod(lambda h: None))
    S, B = params.EncParamsL2CompressedStrict, params.EncParamsL2Compressed
    D = params.DeviceRound
    with D(S, 12, 4) as a, D(B, 12, 4) as b, D(S, 900000, 2) as c, D(params.EncParamsRangeCompressed, 12, 4) as e:
        assert made == [("create_rand", 12, 96, 4), ("create", 12, 96, 4, 0), ("create", 900000, 96, 2, 0), ("create", 12, 64, 4, 1)]
        assert a._compressed and not b._compressed and not c._compressed and e._compressed
        ups = [_l2c(S, i) for i in range(3)]
        monkeypatch.setattr(api.device_round, "ingest", staticmethod(lambda h, records: 0))
        a.ingest(ups)
        asked = []
        monkeypatch.setattr(api.device_round, "verify_compressed", staticmethod(lambda h, proofs: asked.append((h, list(proofs))) or [True, False, True]))
        assert a.rand(S, [ups[2], ups[0]], [2, 0]) == [True, True]
        assert asked == [(2, [ups[0].rand_proof.ctypes.data, None, ups[2].rand_proof.ctypes.data])]
        # members outside the cache: the host-bytes strided call
        host = []
        monkeypatch.setattr(S, "_rand_batch", staticmethod(lambda us: host.append(len(us)) or [True] * len(us)))
        a._slot[1] = None
        assert a.rand(S, ups, [0, 1, 2]) == [True] * 3 and host == [3] and len(asked) == 1
    with pytest.raises(ValueError):
        D(object, 12, 4)
