"""The corpus of tests/ristretto_corpus.py against every decoder that runs without a GPU: classify() names an entry valid exactly when
pyref.ristretto_decode accepts it, the oracle refuses and accepts the same entries (and adds B to the accepted ones as pyref does), and the two
host builds of the product's codec -- fe32.hpp's (rofl_dbg_host_decode_encode) and fe26.hpp's register-radix one that the kernels run
(rofl_dbg_host_fd_codec) -- return 5 or round-trip the bytes.  This pins the corpus and its labels for tests/test_gpu_decode_sites.py and puts
the classes that are refused only after the square-root chain (nonsquare, nonsquare_v0, tneg, y0) into the CPU suite."""
import ctypes

import numpy as np
import pytest

import orc
import ristretto_corpus as RC

pyref = RC.pyref
CORPUS = RC.corpus()
IDS = ["%s-%s" % (c, n) for n, _, c in CORPUS]
B_ENC = pyref.ristretto_encode(pyref.BASE)


def test_corpus_shape():
    names = [n for n, _, _ in CORPUS]
    assert len(set(names)) == len(names) == 33 + RC.N_RANDOM
    count = {c: sum(1 for e in CORPUS if e[2] == c) for c in RC.CLASSES}
    assert count["noncanon"] == 6 and count["bit255"] == 2 and count["negative"] == 4 and count["y0"] == 1 and count["nonsquare_v0"] == 1
    rnd = {c: sum(1 for n, _, k in CORPUS if k == c and n.startswith("random")) for c in ("nonsquare", "tneg", "valid")}
    assert sum(rnd.values()) == RC.N_RANDOM and min(rnd.values()) >= RC.CLASS_FLOOR, rnd
    assert count["valid"] == rnd["valid"] + 19
    assert tuple(e[2] for e in RC.representatives()) == RC.INVALID_CLASSES
    assert [n for n, _, _ in RC.valid_edges()] == ["0", "p-3", "smallest"] + ["%dB" % k for k in range(1, 17)]
    assert RC.corpus() is CORPUS      # (deterministic and computed once)


def test_edges_are_what_their_names_say():
    by = {n: b for n, b, _ in CORPUS}
    P = RC.P
    val = {n: int.from_bytes(b, "little") for n, b in by.items()}
    assert val["p"] == P and val["p+1"] == P + 1 and val["p+2"] == P + 2 and val["p+3"] == P + 3 and val["p+17"] == 2 ** 255 - 2 and val["2^255-1"] == 2 ** 255 - 1
    assert val["p-1"] == P - 1 and val["p-3"] == P - 3 and val["0"] == 0 and val["1"] == 1
    r = val["sqrt(-1)"]
    assert r % 2 == 0 and r * r % P == P - 1
    # nothing even and non-zero below the smallest valid s decodes
    assert all(pyref.ristretto_decode(RC.enc(s)) is None for s in range(2, val["smallest"], 2)) and val["smallest"] > 0
    for n in ("B|bit255", "2B|bit255"):
        b = bytearray(by[n]); assert b[31] & 0x80
        b[31] &= 0x7F
        assert pyref.ristretto_decode(bytes(b)) is not None
    for n, k in (("p-s(B)", 1), ("p-s(2B)", 2)):
        assert RC.enc(P - val[n]) == by["%dB" % k]
    # p - 1 and sqrt(-1) pass the two checks that read the bytes: only the arithmetic refuses them
    for n in ("p-1", "sqrt(-1)"):
        assert val[n] < P and val[n] % 2 == 0


@pytest.mark.parametrize("name,b,cls", CORPUS, ids=IDS)
def test_every_decoder_agrees(hiplib, name, b, cls):
    pt = pyref.ristretto_decode(b)
    assert RC.classify(b) == cls and (cls == "valid") == (pt is not None)
    rc, out = orc.add_points_vec(np.frombuffer(b, np.uint8), np.frombuffer(B_ENC, np.uint8))
    for fn in (hiplib.rofl_dbg_host_decode_encode, hiplib.rofl_dbg_host_fd_codec):
        back = ctypes.create_string_buffer(b"\xa5" * 32, 32)
        got = fn(b, back)
        if cls == "valid":
            assert got == 0 and back.raw == b, (fn.__name__, name)
        else:
            assert got == 5, (fn.__name__, name, cls)
    if cls == "valid":
        assert rc == 0 and out.tobytes() == pyref.ristretto_encode(pyref.pt_add(pt, pyref.BASE)), name
    else:
        assert rc == 5, (name, cls)


def test_corpus_in_one_oracle_call():
    # the oracle's vector entry refuses a call that holds any invalid entry and adds the valid ones element-wise
    valid = [e for e in CORPUS if e[2] == "valid"]
    a = RC.as_array(valid)
    rc, out = orc.add_points_vec(a, np.tile(np.frombuffer(B_ENC, np.uint8), (len(valid), 1)))
    assert rc == 0
    for (n, b, _), o in zip(valid, out):
        assert o.tobytes() == RC.pyref_add(b, B_ENC), n
    for rep in RC.representatives():
        bad = a.copy(); bad[len(valid) // 2] = RC.row(rep)
        assert orc.add_points_vec(bad, a)[0] == 5 and orc.add_points_vec(a, bad)[0] == 5, rep[0]
