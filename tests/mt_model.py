"""Python model of the Merkle trees of rofl_merkle_build / rofl_merkle_verify (include/rofl_zk.h), independent of the library; shared by
test_merkle_host.py and test_gpu_merkle.py.  Every label is 16 bytes:
  leaf(m)    = SHAKE256("rofl-zk/mtr/v1/l" || u64le(len m) || m)[0 .. 32);
  node(a, b) = SHAKE256("rofl-zk/mtr/v1/n" || a || b)[0 .. 32);
  level 0 is the n leaf digests; node i of level l + 1 is node(level_l[2i], level_l[2i + 1]); the last node of a level of odd width moves
  up unchanged; top is the one node of the last level, depth(n) = bit_length(n - 1);
  root       = SHAKE256("rofl-zk/mtr/v1/r" || u64le(n) || top)[0 .. 32);
  path of leaf j: depth(n) slots, slot l = level_l[(j >> l) ^ 1] if that node exists, 32 zero bytes otherwise;
  verdict 2: j >= n or a nonzero byte in a slot the shape leaves empty (the slots beyond the depth included); 0: the climb gives the root;
  1: anything else.
The tree is the one of RFC 6962 (split at the largest power of two below n) with other hashes: rfc6962_top() is that recursion, and
tiled_top() reduces aligned tiles of T nodes and then the tile roots, the order the device kernel works in."""
import hashlib

import numpy as np

DOM_L, DOM_N, DOM_R = b"rofl-zk/mtr/v1/l", b"rofl-zk/mtr/v1/n", b"rofl-zk/mtr/v1/r"
assert len(DOM_L) == len(DOM_N) == len(DOM_R) == 16
EMPTY = bytes(32)
MAX_STRIDE = 20


def rows32(x):
    """uint8[k, 32] of an array, one 32-byte string or a list of 32-byte strings / rows"""
    if isinstance(x, (bytes, bytearray)):
        x = [x]
    if isinstance(x, (list, tuple)):
        x = [np.frombuffer(bytes(r), np.uint8) if isinstance(r, (bytes, bytearray)) else np.asarray(r, np.uint8).reshape(-1) for r in x]
        x = np.stack(x) if x else np.zeros((0, 32), np.uint8)
    return np.ascontiguousarray(np.asarray(x, np.uint8).reshape(-1, 32))


def leaf(m):
    m = bytes(m)
    return hashlib.shake_256(DOM_L + len(m).to_bytes(8, "little") + m).digest(32)


def node(a, b):
    assert len(a) == 32 and len(b) == 32
    return hashlib.shake_256(DOM_N + bytes(a) + bytes(b)).digest(32)


def root_of(n, top):
    assert len(top) == 32
    return hashlib.shake_256(DOM_R + int(n).to_bytes(8, "little") + bytes(top)).digest(32)


def depth(n):
    assert n >= 1
    return (n - 1).bit_length()


def reduce_once(level):
    up = [node(level[2 * i], level[2 * i + 1]) for i in range(len(level) // 2)]
    if len(level) & 1:
        up.append(level[-1])
    return up


def levels(digests):
    """[level 0 .. level depth(n)], each a list of 32-byte strings"""
    lv = [[bytes(d) for d in digests]]
    assert lv[0]
    while len(lv[-1]) > 1:
        lv.append(reduce_once(lv[-1]))
    assert len(lv) == depth(len(digests)) + 1
    return lv


def root(digests):
    return root_of(len(digests), levels(digests)[-1][0])


def path(lv, j):
    """the depth(n) slots of leaf j, from levels()"""
    assert 0 <= j < len(lv[0])
    out = []
    for l in range(len(lv) - 1):
        s = (j >> l) ^ 1
        out.append(lv[l][s] if s < len(lv[l]) else EMPTY)
    return out


def climb(rt, n, j, digest, slots):
    """the verdict of one path: `slots` is the whole row (stride slots), `digest` the leaf digest"""
    slots = [bytes(s) for s in slots]
    if j >= n:
        return 2
    d, w, cur = depth(n), n, bytes(digest)
    assert len(slots) >= d
    empty = [l >= d for l in range(len(slots))]
    for l in range(d):
        empty[l] = ((j >> l) ^ 1) >= w
        w = (w + 1) // 2
    if any(e and s != EMPTY for e, s in zip(empty, slots)):
        return 2
    for l in range(d):
        if not empty[l]:
            cur = node(slots[l], cur) if (j >> l) & 1 else node(cur, slots[l])
    return 0 if root_of(n, cur) == bytes(rt) else 1


def rfc6962_top(digests):
    """the tree of RFC 6962 section 2.1 over the leaf digests: split at the largest power of two below n"""
    n = len(digests)
    if n == 1:
        return bytes(digests[0])
    k = 1 << ((n - 1).bit_length() - 1)
    return node(rfc6962_top(digests[:k]), rfc6962_top(digests[k:]))


def tiled_top(digests, T):
    """aligned tiles of T nodes reduced log2(T) levels each, then the tile roots the same way, until one node is left"""
    assert T >= 2 and T & (T - 1) == 0
    cur = [bytes(d) for d in digests]
    while len(cur) > 1:
        nxt = []
        for t in range(0, len(cur), T):
            tile = cur[t:t + T]
            while len(tile) > 1:
                tile = reduce_once(tile)
            nxt.append(tile[0])
        cur = nxt
    return cur[0]


def build(messages=None, digests=None, paths_for=()):
    """what merkle.build returns: (root bytes, leaves uint8[n, 32], paths uint8[k, depth, 32])"""
    dg = [leaf(m) for m in messages] if digests is None else [bytes(d) for d in rows32(digests)]
    lv = levels(dg)
    d = depth(len(dg))
    paths = np.zeros((len(paths_for), d, 32), np.uint8)
    for k, j in enumerate(paths_for):
        for l, s in enumerate(path(lv, int(j))):
            paths[k, l] = np.frombuffer(s, np.uint8)
    return root_of(len(dg), lv[-1][0]), np.frombuffer(b"".join(dg), np.uint8).reshape(-1, 32).copy(), paths


def verify(roots, counts, paths, messages=None, digests=None, refs=None):
    """what merkle.verify returns: uint8[n_paths]; paths uint8[n_paths, stride, 32]"""
    roots = rows32(roots)
    paths = np.asarray(paths, np.uint8)
    dg = [leaf(m) for m in messages] if digests is None else [bytes(d) for d in rows32(digests)]
    if refs is None:
        refs = [(0, i) for i in range(len(dg))]
    out = np.zeros(len(dg), np.uint8)
    for i, (r, j) in enumerate(refs):
        out[i] = climb(roots[r].tobytes(), int(counts[r]), int(j), dg[i], [paths[i, l].tobytes() for l in range(paths.shape[1])])
    return out


def view_leaf(round_no, dealer, sigs2x64):
    s = np.asarray(sigs2x64, np.uint8)
    assert s.shape == (2, 64)
    return b"rofl-zk/view/v2\0" + int(round_no).to_bytes(8, "little") + int(dealer).to_bytes(4, "little") + s[0].tobytes() + s[1].tobytes()


def view_root_message(round_no, count, rt):
    assert len(bytes(rt)) == 32
    return b"rofl-zk/view/v2r" + int(round_no).to_bytes(8, "little") + int(count).to_bytes(4, "little") + bytes(rt)


def golden_cases():
    """(name, messages) of tests/golden/merkle.json: the four known answers of the definition and a handful of further n"""
    cases = [("empty", [b""]), ("two", [b"", b"a"]), ("three", [b"", b"a", b"ab"]), ("five", [bytes([i]) * i for i in range(5)])]
    for n in (6, 7, 8, 9, 33, 65):
        cases.append(("n%d" % n, [b"leaf %d of %d" % (i, n) + bytes([i & 0xff]) * (i % 5) for i in range(n)]))
    return cases


def golden():
    """the content of tests/golden/merkle.json, from this model"""
    out = []
    for name, msgs in golden_cases():
        rt, lv, paths = build(msgs, paths_for=range(len(msgs)))
        out.append({"name": name, "messages": [m.hex() for m in msgs], "root": rt.hex(), "leaves": [bytes(x).hex() for x in lv],
                    "paths": [[bytes(s).hex() for s in p] for p in paths]})
    return {"definition": "rofl-zk/mtr/v1", "cases": out}
