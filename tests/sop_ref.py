"""Shared by the sum-of-products sumcheck tests (CPU and GPU): the prover of
    S = sum_x sum_t alpha_t prod_j pool[idx(t, j)](x)
restated in numpy / Python ints on top of sumcheck_product_ref.py: a round's polynomial is the alpha-weighted sum of the terms'
product round polynomials (round_coefficients there), lower-degree terms contributing zeros to the high coefficients; the bind, the
transcript (a fresh one per instance that absorbs c_0..c_D in order and then draws) and the verifier's claim chain are the product
reference's.  terms: [(alpha, (idx, ...)), ...].  Everything is exact."""
import numpy as np

import oracle_lib as O
import sumcheck_product_ref as R

P = O.P_BB
_P = np.uint64(P)


def degree(terms):
    return max(len(idx) for _, idx in terms)


def round_coefficients(pool, terms):
    """[c_0..c_D] of the round over the current pool"""
    c = [0] * (degree(terms) + 1)
    for alpha, idx in terms:
        for j, x in enumerate(R.round_coefficients([pool[i] for i in idx])):
            c[j] = (c[j] + int(alpha) * x) % P
    return c


def combine(terms, evals):
    """sum_t alpha_t prod_j evals[idx(t, j)]"""
    s = 0
    for alpha, idx in terms:
        pr = int(alpha) % P
        for i in idx:
            pr = pr * int(evals[i]) % P
        s = (s + pr) % P
    return s


def prove(pool, terms, challenges=None):
    """(claimed_sum, rounds, point, table_evals, final_eval) of the instance; challenges: the interactive form (no transcript)"""
    fs = [np.ascontiguousarray(t, dtype=np.uint64).copy() for t in pool]
    v = len(fs[0]).bit_length() - 1
    tr = O.Transcript()
    rounds, point, claimed = [], [], None
    for j in range(v):
        c = round_coefficients(fs, terms)
        if j == 0:
            claimed = (2 * c[0] + sum(c[1:])) % P
        rounds += c
        if challenges is None:
            for x in c:
                tr.append_field(x)
            ch = tr.challenge()
        else:
            ch = int(challenges[j])
        point.append(ch)
        half = len(fs[0]) // 2
        fs = [(f[:half] + (np.uint64(ch) * ((f[half:] + _P - f[:half]) % _P)) % _P) % _P for f in fs]
    evals = [int(f[0]) for f in fs]
    return claimed, np.array(rounds, dtype=np.uint64), np.array(point, dtype=np.uint64), np.array(evals, dtype=np.uint64), combine(terms, evals)


def claimed_sum(pool, terms):
    """S term by term over the hypercube"""
    s = 0
    for alpha, idx in terms:
        pr = np.ones(len(pool[0]), dtype=np.uint64)
        for i in idx:
            pr = (pr * np.asarray(pool[i], dtype=np.uint64)) % _P
        s = (s + int(alpha) * (int(np.sum(pr, dtype=np.uint64)) % P)) % P
    return s


def check_proof(pool, terms, proof, fiat_shamir=True, mle_eval=R.exact_mle_eval):
    """asserts what a verifier with oracle access to the pool checks of an honest proof"""
    claimed, rounds, point, evals, fe = proof
    d, v = degree(terms), len(point)
    pt = [int(x) for x in point]
    assert len(rounds) == (d + 1) * v and len(evals) == len(pool)
    if fiat_shamir:
        ok, expected, drawn = R.claim_chain(claimed, rounds, v, d)
        assert ok and drawn == pt
    else:
        expected = int(claimed)
        for j in range(v):
            c = [int(x) for x in rounds[(d + 1) * j: (d + 1) * (j + 1)]]
            assert (R.eval_univariate(c, 0) + R.eval_univariate(c, 1)) % P == expected
            expected = R.eval_univariate(c, pt[j])
    assert expected == int(fe)
    for f, e in zip(pool, evals):
        assert int(e) == mle_eval(f, pt[::-1])  # MSB-first binds: the table's extension at the reversed point
    assert combine(terms, evals) == int(fe)


same = R.same


# ---------------------------------------------------------------- term structures the tests share
def structure(M, T, seed):
    """T terms over a pool of M tables, seeded: mixed degrees 1..3 (each at most M distinct + repeats allowed), a repeated index
    where a term has room for one, table M - 1 left unnamed when M > 1 and T < 8, alphas cycling through random, 0, 1, p - 1"""
    rng = np.random.default_rng(seed)
    named = M if (M == 1 or T == 8) else M - 1
    special = [None, 0, 1, P - 1]
    terms = []
    for t in range(T):
        d = 1 + (t + seed) % 3
        idx = [int(rng.integers(0, named)) for _ in range(d)]
        if d >= 2 and t % 2 == 1:
            idx[1] = idx[0]  # f * f
        a = special[t % 4] if T > 1 else None
        terms.append((int(rng.integers(0, P)) if a is None else a, tuple(idx)))
    if T >= 3:  # all three degrees present
        assert {len(i) for _, i in terms} == {1, 2, 3}
    return terms
