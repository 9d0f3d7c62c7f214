"""CPU-only checks of the standard signatures (rofl_ed25519_*): the Python model tests/ed25519_model.py pinned to RFC 8032 and, where one
loads, to libsodium; then the host twins rofl_dbg_host_ed25519_* against the model, bytes and verdicts, no tolerance: every padding case of
SHA-512 at packed (unaligned) starts, the key-refusal corpus, every verdict class, the torsion corpus (keys and R with a small-order part,
where the exact cofactorless rule differs from its neighbours), the parameter checks and the cap on the bytes hashed.  No call here reaches a GPU."""
import ctypes
import os
import sys

import numpy as np
import pytest

import ed25519_model as E

sz, vp = ctypes.c_size_t, ctypes.c_void_p


def call(L, name, *args):
    fn = getattr(L, name)
    fn.argtypes = [sz if isinstance(a, int) else vp for a in args]
    return fn(*[a if isinstance(a, int) or a is None else a.ctypes.data for a in args])


def pack(msgs):
    off = np.zeros(len(msgs) + 1, np.uint64)
    off[1:] = np.cumsum([len(m) for m in msgs])
    return (np.frombuffer(b"".join(msgs), np.uint8).copy() if off[-1] else None), off


def rows(items, width=32):
    return np.frombuffer(b"".join(bytes(i) for i in items), np.uint8).reshape(-1, width).copy()


def host_sign(L, seeds, msgs, refs=None):
    data, off = pack(msgs)
    r = None if refs is None else np.asarray(refs, np.uint32).reshape(-1, 2).copy()
    n = len(seeds) if r is None else len(r)
    sig, pk = np.full((n, 64), 0xaa, np.uint8), np.full((len(seeds), 32), 0xaa, np.uint8)
    assert call(L, "rofl_dbg_host_ed25519_sign", len(seeds), rows(seeds), pk, len(msgs), data, off, n, r, sig) == 0
    return sig, pk


def host_verify(L, pks, msgs, sigs, refs=None, name="rofl_dbg_host_ed25519_verify"):
    data, off = pack(msgs)
    r = None if refs is None else np.asarray(refs, np.uint32).reshape(-1, 2).copy()
    out = np.full(len(sigs), 0xaa, np.uint8)
    rc = call(L, name, len(pks), rows(pks), len(msgs), data, off, len(sigs), r, rows(sigs, 64), out)
    return out if rc == 0 else rc


def test_the_model_is_rfc_8032():
    assert E.encode(E.B) == b"\x58" + b"\x66" * 31
    seed = bytes.fromhex("9d61b19deffd5a60ba844af492ec2cc44449c5697b326919703bac031cae7f60")
    pk = bytes.fromhex("d75a980182b10ab7d54bfed3c964073a0ee172f3daa62325af021a68f707511a")
    sig = bytes.fromhex("e5564300c360ac729086e2cc806e828a84877f1eb8e5d974d873e065224901555fb8821590a33bacc61e39701cf9b46bd25bf5f0595bbe24655141438e7a100b")
    assert E.public_key(seed) == pk and E.sign(seed, b"") == sig and E.verify(pk, b"", sig) == 0 and E.verify(pk, b"x", sig) == 1


def test_the_model_is_libsodium():
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    import sodium_bp
    so = sodium_bp.load_sodium()
    if so is None:
        pytest.skip("no libsodium on this box")
    rng = np.random.default_rng(20261126)
    for n in (0, 1, 111, 300):
        seed, m = rng.bytes(32), rng.bytes(n)
        pk, sk, sig = ctypes.create_string_buffer(32), ctypes.create_string_buffer(64), ctypes.create_string_buffer(64)
        assert so.crypto_sign_seed_keypair(pk, sk, seed) == 0 and so.crypto_sign_detached(sig, None, m, ctypes.c_ulonglong(n), sk) == 0
        assert E.public_key(seed) == pk.raw and E.sign(seed, m) == sig.raw


@pytest.fixture(scope="module")
def padding_batch():
    """one seed and one message per length of E.LENS, packed back to back behind a one-byte message, with the model's keys and signatures"""
    rng = np.random.default_rng(20261127)
    msgs = [rng.bytes(1)] + [rng.bytes(n) for n in E.LENS]
    seeds = [rng.bytes(32) for _ in msgs]
    return seeds, msgs, rows(E.public_key(s) for s in seeds), rows((E.sign(s, m) for s, m in zip(seeds, msgs)), 64)


def test_every_padding_case_at_unaligned_starts(hiplib, padding_batch):
    seeds, msgs, pks, sigs = padding_batch
    assert {int(o) % 8 for o in pack(msgs)[1]} == set(range(8))
    got, pk = host_sign(hiplib, seeds, msgs)
    assert pk.tobytes() == pks.tobytes() and got.tobytes() == sigs.tobytes()
    out = np.zeros_like(pks)
    assert call(hiplib, "rofl_dbg_host_ed25519_public_keys", len(seeds), rows(seeds), out) == 0 and out.tobytes() == pks.tobytes()
    assert not host_verify(hiplib, pks, msgs, sigs).any()
    changed = [(m[:-1] + bytes([m[-1] ^ 1])) if m else b"\0" for m in msgs]
    assert (host_verify(hiplib, pks, changed, sigs) == 1).all()


def test_every_verdict_class_and_the_neighbours_of_a_refused_key(hiplib, padding_batch):
    seeds, msgs, pks, sigs = padding_batch
    cases = E.verdict_cases(pks[5].tobytes(), msgs[5], sigs[5].tobytes())
    want = [c[3] for c in cases]
    assert [E.verify(*c[:3]) for c in cases] == want and want.count(2) == 16 and want.count(1) == 4
    # every case between two good signatures of another key: they stay good
    keys, ms, sg = [pks[7]], [msgs[7]], [sigs[7]]
    for k, m, s, _ in cases:
        keys += [k, pks[7]]; ms += [m, msgs[7]]; sg += [s, sigs[7]]
    got = host_verify(hiplib, keys, ms, sg)
    assert got[0::2].tolist() == [0] * (len(cases) + 1) and got[1::2].tolist() == want


@pytest.fixture(scope="module")
def torsion():
    """ed25519_model.torsion_cases of one fixed seed: computed once, never changed"""
    return tuple(E.torsion_cases(bytes(range(32))))


def interleaved(cases, good):
    """keys, messages, signatures: `good` first, then every case followed by `good` again, so the cases sit at the odd places"""
    keys, ms, sg = [good[0]], [good[1]], [good[2]]
    for c in cases:
        keys += [c[0], good[0]]; ms += [c[1], good[1]]; sg += [c[2], good[2]]
    return keys, ms, sg


def test_the_torsion_corpus_is_what_its_algebra_says(torsion):
    family = lambda f: [c for c in torsion if c[4][0] == f]      # noqa: E731
    assert {f: len(family(f)) for f in E.TORSION_SIZES} == E.TORSION_SIZES and len(torsion) == sum(E.TORSION_SIZES.values())
    assert [c[4] for c in family("a")] == ["a%d" % i for i in range(1, 8) for _ in range(4)]
    # (a): a key per T_i, none of small order; the verdict is a function of the order of T_i and k mod 8 alone, and both verdicts show for every i
    for i, order in zip(range(1, 8), (8, 4, 8, 2, 8, 4, 8)):
        mine = [c for c in torsion if c[4] == "a%d" % i]
        assert len({c[0] for c in mine}) == 1 and not E.is_identity(E.mul(8, E.decode(mine[0][0])))
        k8 = [E.challenge(c[2][:32], c[0], c[1]) % 8 for c in mine]
        assert k8[:3] == [0, 4, 2] and k8[3] % 2 == 1
        accepted = {8: [0, 1, 1, 1], 4: [0, 0, 1, 1], 2: [0, 0, 0, 1]}[order]      # only at 0 mod 8; also at 4 mod 8; also at 2 mod 8; never at an odd k
        assert [c[3] for c in mine] == accepted
    assert len({c[0] for c in family("a")}) == 7
    assert [c[3] for c in family("b")] == [1] * 7 and len({c[2][:32] for c in family("b")}) == 7
    c0, c1 = family("c")
    assert (c0[3], c1[3]) == (0, 1) and c0[2][:32] == E.encode(E.IDENTITY) and c1[2][:32] == (E.P + 1).to_bytes(32, "little")
    small = [E.encode(t) for t in E.small_order_points()]
    assert all(c[3] == 0 and c[2][:32] in small for c in family("d")) and len({c[2][:32] for c in family("d")}) == 3
    assert [(int.from_bytes(c[2][32:], "little"), c[3]) for c in family("e")] == [(0, 1), (1, 1), (E.L - 1, 1)]
    ys = [int.from_bytes(c[0], "little") for c in family("f")]
    assert sorted(ys) == sorted(y | s << 255 for y in range(E.P, 2**255) for s in (0, 1)) and all(c[3] == 2 for c in family("f"))
    # 23 of the 38 are points once y is reduced: only the canonical check stands between them and a verdict of 0 or 1
    assert sum(E.decode((y % 2**255 % E.P | y >> 255 << 255).to_bytes(32, "little")) is not None for y in ys) == 23


def test_the_host_twin_on_the_torsion_corpus(hiplib, padding_batch, torsion):
    seeds, msgs, pks, sigs = padding_batch
    keys, ms, sg = interleaved(torsion, (pks[7].tobytes(), msgs[7], sigs[7].tobytes()))
    got = host_verify(hiplib, keys, ms, sg)
    assert got[0::2].tolist() == [0] * (len(torsion) + 1)
    assert got[1::2].tolist() == [c[3] for c in torsion], [c[4] for c, g in zip(torsion, got[1::2]) if c[3] != g]


def test_the_torsion_corpus_under_libsodium(torsion):
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    import sodium_bp
    so = sodium_bp.load_sodium()
    if so is None:
        pytest.skip("no libsodium on this box")
    # libsodium checks the cofactorless equation on R's bytes too, but refuses a small-order R by policy, which this project does not:
    # (c) and (d) are left out; (f) is the key refusal that test_every_verdict_class... holds
    mine = [c for c in torsion if c[4][0] in "abe"]
    assert len(mine) == 38
    for key, m, sig, verdict, tag in mine:
        assert (so.crypto_sign_verify_detached(sig, m, ctypes.c_ulonglong(len(m)), key) == 0) == (verdict == 0), tag


def test_checks_and_the_cap_come_before_any_work(hiplib, padding_batch):
    seeds, msgs, pks, sigs = padding_batch
    assert call(hiplib, "rofl_dbg_host_ed25519_sign", 0, None, None, 0, None, None, 0, None, None) == 0
    assert host_sign(hiplib, [bytes(32)], [b"every seed is a key"])[0].tobytes() == E.sign(bytes(32), b"every seed is a key")
    assert host_verify(hiplib, pks[:2], msgs[:3], sigs[:2]) == 11 and host_verify(hiplib, pks, msgs, sigs[:1], [(0, 99)]) == 11
    # 2^30 + 1 bytes hashed: one 2^20 + 1 byte message (named by its offsets, never allocated or read) under 1024 refs
    off, refs = np.array([0, 2**20 + 1], np.uint64), np.zeros((1024, 2), np.uint32)
    dummy, out = np.zeros(8, np.uint8), np.zeros((1024, 64), np.uint8)
    for name, args in (("sign", (1, pks[:1], None, 1, dummy, off, 1024, refs, out)), ("verify", (1, pks[:1], 1, dummy, off, 1024, refs, out, out))):
        for prefix in ("rofl_dbg_host_ed25519_", "rofl_ed25519_"):
            assert call(hiplib, prefix + name, *args) == 11
    err = ctypes.create_string_buffer(512)
    hiplib.rofl_last_error(err, sz(512))
    assert b"2^30" in err.value
