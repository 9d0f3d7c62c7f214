"""CPU-only checks of the Merkle trees (rofl_merkle_build / rofl_merkle_verify): the Python model of the definition (tests/mt_model.py)
against tests/golden/merkle.json, against the recursion of RFC 6962 and against the tiled order of reduction the device kernel uses; the host
route rofl_dbg_host_merkle_* against the model (tree sizes around the powers of two, every padding case of the leaf digest at misaligned
starts, digests as input, every verdict class); every parameter check of the four C entry points (they come before the device is touched);
the view helpers of secret_sharing against the model's byte layouts; and the Rust declarations.  No call here reaches a GPU."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import mt_model as M
import sig_model as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sz, vp = ctypes.c_size_t, ctypes.c_void_p
BUILD_ARGS = [sz, vp, vp, vp, vp, sz, vp, vp]
VERIFY_ARGS = [sz, vp, vp, sz, vp, vp, vp, vp, sz, vp]
KNOWN = {"empty": "6dcc6ff77429365f05cb798fc9a51211c9f7095bec289adf17e27069bb7194d4",
         "two": "c6b03251aa5b2561eb3f3bb1cfce6a2e9987e8bc929b29c50ac00913c749f23d",
         "three": "9ed40eb76da9cd9aaf8dedcdb9e64fe712b1708ca010d9e915ab7df0e4668670",
         "five": "dde86a52c775ed690632658d6eac2e3e7a571b53da9400c26f8187a856517802"}
SIZES = (1, 2, 3, 5, 63, 64, 65, 513)


def _p(x):
    return None if x is None else x.ctypes.data


def _build(L, name, n, data, off, root, leaves, n_paths, idx, paths):
    fn = getattr(L, name)
    fn.argtypes = BUILD_ARGS
    return fn(n, _p(data), _p(off), _p(root), _p(leaves), n_paths, _p(idx), _p(paths))


def _verify(L, name, n_roots, roots, counts, n_paths, refs, data, off, paths, stride, out):
    fn = getattr(L, name)
    fn.argtypes = VERIFY_ARGS
    return fn(n_roots, _p(roots), _p(counts), n_paths, _p(refs), _p(data), _p(off), _p(paths), stride, _p(out))


def _last_error(L):
    err = ctypes.create_string_buffer(512)
    L.rofl_last_error(err, sz(512))
    return err.value.decode()


def host_build(L, msgs=None, digests=None, paths_for=(), name="rofl_dbg_host_merkle_build"):
    """-> (root bytes, leaves uint8[n, 32], paths uint8[k, depth, 32])"""
    if digests is None:
        data, off = S.pack(msgs)
        n = len(msgs)
    else:
        data, off = M.rows32(digests), None
        n = data.shape[0]
    idx = np.asarray(list(paths_for), np.uint32)
    root, leaves = np.full(32, 0xaa, np.uint8), np.full((n, 32), 0xaa, np.uint8)
    paths = np.full((len(idx), M.depth(n), 32), 0xaa, np.uint8)
    assert _build(L, name, n, data if data.size else None, off, root, leaves, len(idx), idx if len(idx) else None, paths if paths.size else None) == 0
    return root.tobytes(), leaves, paths


def host_verify(L, roots, counts, paths, msgs=None, digests=None, refs=None, name="rofl_dbg_host_merkle_verify"):
    roots = M.rows32(roots)
    counts = np.asarray(counts, np.uint32)
    paths = np.ascontiguousarray(np.asarray(paths, np.uint8))
    if digests is None:
        data, off = S.pack(msgs)
        n = len(msgs)
    else:
        data, off = M.rows32(digests), None
        n = data.shape[0]
    r = None if refs is None else np.ascontiguousarray(np.asarray(refs, np.uint32).reshape(-1, 2))
    out = np.full(n, 0xaa, np.uint8)
    assert _verify(L, name, len(roots), roots, counts, n, r, data if data.size else None, off, paths if paths.size else None, paths.shape[1], out) == 0
    return out


def mixed_messages(rng, n):
    """n messages of 0 .. 299 bytes: most of one Keccak block, one of several blocks among them"""
    lens = rng.integers(0, 100, n)
    lens[rng.integers(0, n)] = 299
    if n > 3:
        lens[1], lens[2] = 0, 112
    return [rng.bytes(int(k)) for k in lens]


def verdict_cases(n=13, seed=20261201):
    """Every verdict class on one tree of n = 13 leaves (depth 4; leaf 12 has two empty slots), good paths beside bad ones, rows of
    stride 6 -> (root, n, refs, messages, digests, paths uint8[k, 6, 32], expected verdicts).  The expectations are written down here, not
    computed: the callers hold the model to them as well."""
    rng = np.random.default_rng(seed)
    msgs = [rng.bytes(20 + i) for i in range(n)]
    root, leaves, paths = M.build(msgs, paths_for=range(n))
    stride = 6
    rows = np.zeros((n, stride, 32), np.uint8)
    rows[:, :M.depth(n)] = paths
    assert not rows[12, :2].any() and rows[12, 2:4].any(axis=1).all() and rows[5, :4].any(axis=1).all()
    cases = []

    def add(j, msg, row, want):
        cases.append((j, bytes(msg), np.asarray(row, np.uint8).copy(), want))
    add(5, msgs[5], rows[5], 0)
    r = rows[5].copy(); r[2, 7] ^= 0x10; add(5, msgs[5], r, 1)                      # a bit of a sibling
    m = bytearray(msgs[5]); m[3] ^= 0x01; add(5, m, rows[5], 1)                     # a bit of the leaf message
    add(4, msgs[5], rows[5], 1)                                                     # a wrong index with the right path (the order of a pair)
    add(7, msgs[5], rows[5], 1)                                                     # ... and another
    add(12, msgs[12], rows[12], 0)                                                  # the right edge: two empty slots  
    add(13, msgs[12], rows[12], 2)                                                  # index = n
    add(2 ** 32 - 1, msgs[0], rows[0], 2)                                           # index far above n
    r = rows[12].copy(); r[1, 31] = 1; add(12, msgs[12], r, 2)                      # a nonzero byte in a slot the shape leaves empty
    r = rows[5].copy(); r[4, 0] = 0x80; add(5, msgs[5], r, 2)                       # ... in the first slot beyond the depth
    r = rows[0].copy(); r[5, 17] = 1; add(0, msgs[0], r, 2)                         # ... in the last slot of the row
    r = rows[12].copy(); r[0, 0] = 1; r[3, 0] ^= 1; add(12, msgs[12], r, 2)         # malformed wins over a failing climb
    add(0, msgs[0], rows[0], 0)
    add(11, msgs[11], rows[11], 0)
    # a leaf digest used as a node: the pair (leaf 10, leaf 11) offered as ONE leaf whose "message" is the two digests, one level up
    fake = leaves[10].tobytes() + leaves[11].tobytes()
    r = np.zeros((stride, 32), np.uint8); r[:3] = rows[10][1:4]
    add(5, fake, r, 1)
    refs = [(0, c[0]) for c in cases]
    out_msgs = [c[1] for c in cases]
    digs = np.frombuffer(b"".join(M.leaf(m) for m in out_msgs), np.uint8).reshape(-1, 32).copy()
    return root, n, refs, out_msgs, digs, np.stack([c[2] for c in cases]), np.array([c[3] for c in cases], np.uint8)


# ---------------------------------------------------------------- the model
def test_model_reproduces_the_golden_file_and_the_known_answers():
    g = json.load(open(os.path.join(ROOT, "tests", "golden", "merkle.json")))
    assert g == M.golden()
    by_name = {c["name"]: c for c in g["cases"]}
    for name, want in KNOWN.items():
        assert by_name[name]["root"] == want
    five = by_name["five"]
    assert [bytes.fromhex(m) for m in five["messages"]] == [bytes([i]) * i for i in range(5)]
    p4 = five["paths"][4]
    assert p4[0] == p4[1] == "00" * 32 and p4[2].startswith("3cafe949678e8dbb")
    for c in g["cases"]:      # every recorded path climbs to the recorded root
        n = len(c["messages"])
        for j in range(n):
            assert M.climb(bytes.fromhex(c["root"]), n, j, bytes.fromhex(c["leaves"][j]), [bytes.fromhex(s) for s in c["paths"][j]]) == 0


@pytest.mark.parametrize("n", list(range(1, 70)) + [127, 128, 129, 511, 512, 513, 1023, 1025])
def test_model_levels_are_rfc6962_and_every_tile_size_gives_them(n):
    dg = [M.leaf(b"%d/%d" % (i, n)) for i in range(n)]
    lv = M.levels(dg)
    assert [len(x) for x in lv][-1] == 1 and len(lv) == M.depth(n) + 1
    assert lv[-1][0] == M.rfc6962_top(dg)
    for T in (2, 4, 8, 512):
        assert M.tiled_top(dg, T) == lv[-1][0]
    rt = M.root(dg)
    for j in {0, n - 1, n // 2}:
        p = M.path(lv, j)
        assert M.climb(rt, n, j, dg[j], p) == 0
        assert all(s == M.EMPTY for l, s in enumerate(p) if ((j >> l) ^ 1) >= len(lv[l]))
    if n > 1:
        assert M.climb(rt, n + 1, 0, dg[0], M.path(lv, 0) + [M.EMPTY]) != 0      # the leaf count is bound into the root


def test_model_verdict_cases_are_the_written_expectations():
    root, n, refs, msgs, digs, paths, want = verdict_cases()
    assert set(want.tolist()) == {0, 1, 2}
    assert (M.verify([root], [n], paths, messages=msgs, refs=refs) == want).all()
    assert (M.verify([root], [n], paths, digests=digs, refs=refs) == want).all()


# ---------------------------------------------------------------- the host route against the model
def test_host_route_gives_the_known_answers(hiplib):
    for name, msgs in M.golden_cases()[:4]:
        assert host_build(hiplib, msgs)[0].hex() == KNOWN[name]


@pytest.mark.parametrize("n", SIZES)
def test_host_build_is_the_model(hiplib, n):
    rng = np.random.default_rng(20261210 + n)
    msgs = mixed_messages(rng, n)
    want = sorted({0, n - 1, n // 2, max(n - 2, 0)})
    want = want + want[:1]      # a repeat, out of order
    root, leaves, paths = host_build(hiplib, msgs, paths_for=want)
    mroot, mleaves, mpaths = M.build(msgs, paths_for=want)
    assert root == mroot and (leaves == mleaves).all() and (paths == mpaths).all()
    # the digest-input form is the message form
    root2, leaves2, paths2 = host_build(hiplib, digests=mleaves, paths_for=want)
    assert root2 == root and (leaves2 == leaves).all() and (paths2 == paths).all()
    # every path verifies, in both forms, with a stride above the depth
    rows = np.zeros((len(want), M.depth(n) + 2, 32), np.uint8)
    rows[:, :M.depth(n)] = paths
    refs = [(0, j) for j in want]
    assert not host_verify(hiplib, [root], [n], rows, msgs=[msgs[j] for j in want], refs=refs).any()
    assert not host_verify(hiplib, [root], [n], rows, digests=leaves[want], refs=refs).any()


def test_host_leaf_digest_at_every_padding_case_and_misaligned_starts(hiplib):
    rng = np.random.default_rng(20261211)
    msgs, where = S.misaligned_messages(rng)
    assert sorted(len(msgs[w]) for w in where) == sorted(S.LENS)
    root, leaves, paths = host_build(hiplib, msgs, paths_for=where)
    mroot, mleaves, mpaths = M.build(msgs, paths_for=where)
    assert (leaves == mleaves).all() and root == mroot and (paths == mpaths).all()
    assert not host_verify(hiplib, [root], [len(msgs)], paths, msgs=[msgs[w] for w in where], refs=[(0, w) for w in where]).any()


def test_host_verdict_classes(hiplib):
    root, n, refs, msgs, digs, paths, want = verdict_cases()
    assert (host_verify(hiplib, [root], [n], paths, msgs=msgs, refs=refs) == want).all()
    assert (host_verify(hiplib, [root], [n], paths, digests=digs, refs=refs) == want).all()
    # a flipped bit in the root fails every good path and leaves the malformed ones malformed
    bad = bytearray(root); bad[9] ^= 0x04
    got = host_verify(hiplib, [bytes(bad)], [n], paths, msgs=msgs, refs=refs)
    assert (got == np.where(want == 2, 2, 1)).all()
    # the root of the same leaves under another leaf count is another root
    assert (host_verify(hiplib, [root], [n + 1], paths, msgs=msgs, refs=refs)[want == 0] != 0).all()


def test_host_two_roots_in_one_call_and_no_ref_list(hiplib):
    rng = np.random.default_rng(20261212)
    a, b = [rng.bytes(9) for _ in range(5)], [rng.bytes(30) for _ in range(70)]
    ra, _, pa = host_build(hiplib, a, paths_for=range(5))
    rb, _, pb = host_build(hiplib, b, paths_for=range(70))
    stride = 9
    rows = np.zeros((75, stride, 32), np.uint8)
    rows[:5, :3], rows[5:, :7] = pa, pb
    refs = [(0, j) for j in range(5)] + [(1, j) for j in range(70)]
    assert not host_verify(hiplib, [ra, rb], [5, 70], rows, msgs=a + b, refs=refs).any()
    swapped = [(1 - r, j) for r, j in refs]
    got = host_verify(hiplib, [ra, rb], [5, 70], rows, msgs=a + b, refs=swapped)
    assert (got == M.verify([ra, rb], [5, 70], rows, messages=a + b, refs=swapped)).all() and got.all()
    # refs == NULL: every path under root 0, index i; a sixth path is index 5 >= n, verdict 2
    six = np.zeros((6, 3, 32), np.uint8); six[:5] = pa
    assert host_verify(hiplib, [ra], [5], six, msgs=a + [a[0]]).tolist() == [0, 0, 0, 0, 0, 2]


# ---------------------------------------------------------------- parameter checks: before the device is touched
@pytest.mark.parametrize("name", ["rofl_merkle_build", "rofl_dbg_host_merkle_build"])
def test_build_parameter_checks(hiplib, name):
    L = hiplib
    data, off = S.pack([b"ab", b"c", b""])
    root, leaves, idx, paths = np.zeros(32, np.uint8), np.zeros((3, 32), np.uint8), np.array([0, 2], np.uint32), np.zeros((2, 2, 32), np.uint8)

    def bad(text, *a):
        assert _build(L, name, *a) == 11
        assert text in _last_error(L), (_last_error(L), text)
    assert _build(L, name, 0, None, None, None, None, 0, None, None) == 0      # the empty call
    bad("paths of a tree without leaves", 0, None, None, root, None, 1, idx, paths)
    bad("bad parameter", 3, data, off, None, None, 0, None, None)
    bad("bad parameter", 3, None, None, root, None, 0, None, None)
    bad("bad parameter", 3, None, off, root, None, 0, None, None)
    bad("bad parameter", 3, data, off, root, None, 2, None, paths)
    bad("bad parameter", 3, data, off, root, None, 2, idx, None)
    bad("more than 2^20 leaves", (1 << 20) + 1, data, None, root, None, 0, None, None)
    o = off.copy(); o[0] = 1
    bad("the first message offset is 0", 3, data, o, root, None, 0, None, None)
    o = off.copy(); o[2] = 1
    bad("message offset 2 is below the one before it", 3, data, o, root, None, 0, None, None)
    o = off.copy(); o[3] = (1 << 30) + 1
    bad("more than 2^30 message bytes", 3, data, o, root, None, 0, None, None)
    bad("more than 2^24 paths", 3, data, off, root, None, (1 << 24) + 1, idx, paths)
    bad("more than 2^30 path bytes", 5, np.zeros((5, 32), np.uint8), None, root, None, 1 << 24, idx, paths)      # depth 3: 2^24 x 96 bytes
    bad("path 1 names a leaf that is not in the tree", 3, data, off, root, None, 2, np.array([2, 3], np.uint32), paths)


@pytest.mark.parametrize("name", ["rofl_merkle_verify", "rofl_dbg_host_merkle_verify"])
def test_verify_parameter_checks(hiplib, name):
    L = hiplib
    data, off = S.pack([b"ab", b"c"])
    roots, counts, out = np.zeros((2, 32), np.uint8), np.array([3, 70], np.uint32), np.zeros(2, np.uint8)
    refs, paths = np.array([[0, 1], [1, 69]], np.uint32), np.zeros((2, 7, 32), np.uint8)

    def bad(text, *a):
        assert _verify(L, name, *a) == 11
        assert text in _last_error(L), (_last_error(L), text)
    assert _verify(L, name, 0, None, None, 0, None, None, None, None, 0, None) == 0      # the empty call
    for k in (1, 2, 9):
        a = [2, roots, counts, 2, refs, data, off, paths, 7, out]; a[k] = None
        bad("bad parameter", *a)
    bad("bad parameter", 2, roots, counts, 2, refs, None, None, paths, 7, out)
    bad("bad parameter", 2, roots, counts, 2, refs, None, off, paths, 7, out)
    bad("bad parameter", 2, roots, counts, 2, refs, data, off, None, 7, out)
    bad("paths without roots", 0, roots, counts, 2, refs, data, off, paths, 7, out)
    bad("more than 2^20 roots", (1 << 20) + 1, roots, counts, 2, refs, data, off, paths, 7, out)
    bad("more than 2^24 paths", 2, roots, counts, (1 << 24) + 1, refs, data, off, paths, 7, out)
    bad("a stride above 20", 2, roots, counts, 2, refs, data, off, paths, 21, out)
    bad("more than 2^30 path bytes", 2, roots, counts, 1 << 24, refs, data, off, paths, 7, out)
    bad("the leaf count of root 1 is not in [1, 2^20]", 2, roots, np.array([3, 0], np.uint32), 2, refs, data, off, paths, 7, out)
    bad("the leaf count of root 0 is not in [1, 2^20]", 2, roots, np.array([(1 << 20) + 1, 3], np.uint32), 2, refs, data, off, paths, 7, out)
    bad("without a ref list there is one root", 2, roots, counts, 2, None, data, off, paths, 7, out)
    bad("ref 1 names a root that is not in the call", 2, roots, counts, 2, np.array([[0, 1], [2, 0]], np.uint32), data, off, paths, 7, out)
    bad("the stride is below the depth of root 1", 2, roots, counts, 2, refs, data, off, paths, 6, out)
    bad("the stride is below the depth of root 0", 1, roots, counts, 2, None, data, off, paths, 1, out)
    o = off.copy(); o[0] = 1
    bad("the first message offset is 0", 2, roots, counts, 2, refs, data, o, paths, 7, out)
    o = off.copy(); o[2] = 1
    bad("message offset 2 is below the one before it", 2, roots, counts, 2, refs, data, o, paths, 7, out)
    # an index >= its root's leaf count is per-path data: verdict 2, not an error (the host entry only: the other would touch the device)
    if "host" in name:
        assert _verify(L, name, 2, roots, counts, 2, np.array([[0, 3], [1, 70]], np.uint32), data, off, paths, 7, out) == 0 and out.tolist() == [2, 2]
    # a root that no ref names may be deeper than the stride
    assert "host" not in name or _verify(L, name, 2, roots, counts, 2, np.array([[0, 1], [0, 2]], np.uint32), data, off, paths, 2, out) == 0


# ---------------------------------------------------------------- the Python wrappers and the view helpers
def test_python_wrappers_on_the_host_route(hiplib):
    from rofl_project_code_amd import api
    rng = np.random.default_rng(20261213)
    msgs = mixed_messages(rng, 11)
    hb, hv = hiplib.rofl_dbg_host_merkle_build, hiplib.rofl_dbg_host_merkle_verify
    hb.argtypes = hv.argtypes = None
    assert [api.merkle.depth(n) for n in (1, 2, 3, 4, 5, 1 << 20)] == [0, 1, 2, 2, 3, 20]
    mroot, mleaves, mpaths = M.build(msgs, paths_for=[10, 0, 10])
    root = api.merkle._build(hb, msgs, None, None, False)
    assert root.tobytes() == mroot
    root, paths, leaves = api.merkle._build(hb, msgs, None, [10, 0, 10], True)
    assert root.tobytes() == mroot and (paths == mpaths).all() and (leaves == mleaves).all()
    root2, leaves2 = api.merkle._build(hb, None, mleaves, None, True)
    assert root2.tobytes() == mroot and (leaves2 == mleaves).all()
    assert api.merkle._verify(hv, [root], [11], paths, [msgs[10], msgs[0], msgs[9]], None, [(0, 10), (0, 0), (0, 10)]).tolist() == [0, 0, 1]
    assert api.merkle._verify(hv, root, [11], paths[1:2], None, mleaves[:1], None).tolist() == [0]
    one = api.merkle._build(hb, [b""], None, [0], False)
    assert one[0].tobytes().hex() == KNOWN["empty"] and one[1].shape == (1, 0, 32)
    assert api.merkle._verify(hv, one[0], [1], one[1], [b""], None, None).tolist() == [0]
    with pytest.raises(ValueError):
        api.merkle.build(msgs, digests=mleaves)
    with pytest.raises(ValueError):
        api.merkle.build(msgs, paths_for=[11])
    with pytest.raises(ValueError):
        api.merkle.build([])
    with pytest.raises(ValueError):
        api.merkle.verify([root], [11, 12], paths, messages=msgs[:3])
    with pytest.raises(ValueError):
        api.merkle.verify([root], [11], paths[:, :, :31], messages=msgs[:3])


def test_view_helpers_have_the_models_byte_layouts(hiplib, monkeypatch):
    import rofl_project_code_amd as R
    from rofl_project_code_amd import api
    assert R.merkle is api.merkle
    ss = api.secret_sharing
    rng = np.random.default_rng(20261214)
    sigs = {int(d): rng.integers(0, 256, (2, 64), dtype=np.uint8) for d in (7, 2, 40, 3, 11, 5)}
    leaf = ss.view_leaf(9, 7, sigs[7])
    assert leaf == M.view_leaf(9, 7, sigs[7]) and len(leaf) == 156 and leaf[:16] == b"rofl-zk/view/v2\0"
    rt = bytes(range(32))
    msg = ss.view_root_message(9, 6, np.frombuffer(rt, np.uint8))
    assert msg == ss.view_root_message(9, 6, rt) == M.view_root_message(9, 6, rt) and len(msg) == 60 and msg[:16] == b"rofl-zk/view/v2r"
    with pytest.raises(ValueError):
        ss.view_leaf(9, 7, sigs[7][:1])
    with pytest.raises(ValueError):
        ss.view_root_message(9, 6, rt[:31])
    # view_tree is ONE merkle.build call over the leaves in ascending dealer order; here on the host route
    hb, hv = hiplib.rofl_dbg_host_merkle_build, hiplib.rofl_dbg_host_merkle_verify
    hb.argtypes = hv.argtypes = None
    calls = []

    def build(messages=None, digests=None, paths_for=None, with_leaves=False):
        calls.append(len(messages))
        return api.merkle._build(hb, messages, digests, paths_for, with_leaves)
    monkeypatch.setattr(api.merkle, "build", staticmethod(build))
    monkeypatch.setattr(api.merkle, "verify", staticmethod(lambda roots, counts, paths, messages=None, digests=None, refs=None:
                                                           api.merkle._verify(hv, roots, counts, paths, messages, digests, refs)))
    order = sorted(sigs)
    mroot, _, mpaths = M.build([M.view_leaf(9, d, sigs[d]) for d in order], paths_for=[order.index(40), order.index(2)])
    root, dealers = ss.view_tree(9, sigs)
    assert root.tobytes() == mroot and dealers == order
    root, dealers, paths = ss.view_tree(9, sigs, paths_for=[40, 2])
    assert root.tobytes() == mroot and (paths == mpaths).all() and calls == [6, 6]
    with pytest.raises(ValueError):
        ss.view_tree(9, sigs, paths_for=[4])
    got = ss.verify_view_entries(9, root, 6, [order.index(40), order.index(2), order.index(2)], [(40, sigs[40]), (2, sigs[2]), (3, sigs[2])], paths[[0, 1, 1]])
    assert got.tolist() == [0, 0, 1]
    other = dict(sigs); other[3] = sigs[3] ^ 1; del other[11]; other[12] = sigs[11]
    assert ss.differing_view_entries(9, sigs, other) == [3, 11, 12] and ss.differing_view_entries(9, sigs, dict(sigs)) == []


def test_rust_declarations_match_the_header():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "check_ffi.py")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "rofl_merkle_build" in open(os.path.join(ROOT, "integration", "rofl_crypto_overlay", "src", "ffi.rs")).read()
