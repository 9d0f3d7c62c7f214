"""Python model of the verifiable sharing of rofl_feldman_commit / rofl_feldman_verify (include/rofl_zk.h), independent of the library; shared by
test_feldman_host.py and test_gpu_feldman.py:
  polynomial of a secret = [s mod l, a_1, ..., a_{t-1}] with the coefficients of shamir_model.coefficients;
  commitments = encode(c_k * B) for its coefficients c_k, the identity encoding (32 zero bytes) for a zero coefficient;
  verdict of a share y at the point x = 0 if y mod l == f(x) else 1 -- from integers alone, also for a polynomial whose coefficients were
  tampered with, so the verify expectations need no point arithmetic.
The point arithmetic is tests/golden/pyref.py as dh_model.py uses it; fast=True takes the product from the oracle's MSM of one term instead
(same bytes, ~100x faster)."""
import numpy as np

import dh_model as D
import shamir_model as M

L = M.L


def polynomial(secret, seed, t):
    """[s mod l, a_1, ..., a_{t-1}]"""
    return [int.from_bytes(bytes(secret), "little") % L] + M.coefficients(seed, t)


def polynomials(secrets, seeds, t):
    return [polynomial(s, c, t) for s, c in zip(secrets, seeds)]


def commit_ints(coeffs, fast=True):
    """the commitments of one polynomial given as integers -> uint8[t, 32]"""
    enc = [bytes(32) if c % L == 0 else D._product(c % L, D.BASE_ENC, fast) for c in coeffs]
    return np.frombuffer(b"".join(enc), np.uint8).reshape(len(coeffs), 32).copy()


def commit(secrets, seeds, t, fast=True):
    """-> uint8[n_secrets, t, 32]"""
    rows = [commit_ints(p, fast) for p in polynomials(secrets, seeds, t)]
    return np.stack(rows) if rows else np.zeros((0, t, 32), np.uint8)


def evaluate(coeffs, x):
    return sum(c * pow(int(x), k, L) for k, c in enumerate(coeffs)) % L


def verdicts(polys, xs, shares):
    """polys: one list of integer coefficients per secret (what the commitments commit to); shares uint8[n_secrets, len(xs), 32]
    -> uint8[n_secrets, len(xs)] of 0 / 1"""
    xs = [int(x) for x in xs]
    shares = np.asarray(shares, np.uint8).reshape(len(polys), len(xs), 32)
    out = np.zeros((len(polys), len(xs)), np.uint8)
    for r, p in enumerate(polys):
        for c, x in enumerate(xs):
            out[r, c] = 0 if int.from_bytes(shares[r, c].tobytes(), "little") % L == evaluate(p, x) else 1
    return out
