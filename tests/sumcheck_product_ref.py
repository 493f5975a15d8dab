"""Shared by the product-sumcheck tests (CPU and GPU): the prover of sum_x prod_j f_j(x) restated in numpy on top of the oracle's
transcript and field -- SumcheckProver.prove (sumcheck_prover.zig:26-91) with the round polynomial
g(t) = sum_i prod_j (a_j + t (b_j - a_j)), a_j = f_j[i], b_j = f_j[i + m/2], in coefficient form c_0..c_d, partialEval's MSB-first
bind (multilinear.zig:166-173), a fresh transcript that absorbs c_0..c_d and then draws the challenge
(sumcheck_protocol.zig:176-184) -- and the verifier's claim chain for d + 1 coefficients per round (sumcheck_verifier.zig:172-205).
u64 arithmetic, reduced after every multiply (operands below p < 2^31: a product is below 2^62), so everything is exact."""
import numpy as np

import oracle_lib as O

P = O.P_BB
_P = np.uint64(P)


def round_coefficients(fs):
    """[c_0..c_d] of the round over the tables fs (d arrays of m canonical u64 values)"""
    half = len(fs[0]) // 2
    g = [np.ones(half, dtype=np.uint64)]
    for f in fs:
        a = f[:half]
        e = (f[half:] + _P - a) % _P
        nxt = [(g[0] * a) % _P]
        for x in range(1, len(g)):
            nxt.append(((g[x] * a) % _P + (g[x - 1] * e) % _P) % _P)
        nxt.append((g[-1] * e) % _P)
        g = nxt
    return [int(np.sum(c, dtype=np.uint64)) % P for c in g]  # fewer than 2^32 terms below 2^31


def prove(tables, challenges=None):
    """(claimed_sum, rounds, point, factor_evals, final_eval) of the instance whose factors are `tables`; challenges: the
    interactive form (no transcript)"""
    fs = [np.ascontiguousarray(t, dtype=np.uint64).copy() for t in tables]
    d, n = len(fs), len(fs[0])
    v = n.bit_length() - 1
    tr = O.Transcript()
    rounds, point, claimed = [], [], None
    for j in range(v):
        c = round_coefficients(fs)
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
    fe = 1
    for x in evals:
        fe = fe * x % P
    return claimed, np.array(rounds, dtype=np.uint64), np.array(point, dtype=np.uint64), np.array(evals, dtype=np.uint64), fe


def eval_univariate(coeffs, x):
    c = np.ascontiguousarray(coeffs, dtype=np.uint64)
    return O.lib.orc_eval_univariate(P, c.ctypes.data_as(O.u64p), len(c), int(x))


def claim_chain(claimed, rounds, v, d):
    """(rounds_ok, expected_eval) -- sumcheck_verify_ref.claim_chain with d + 1 coefficients per round: g(0) + g(1) must equal the
    claim, the coefficients are absorbed in order, the claim becomes g(challenge); also returns the challenges drawn"""
    tr = O.Transcript()
    claim = int(claimed)
    point = []
    for j in range(v):
        c = [int(x) for x in rounds[(d + 1) * j: (d + 1) * (j + 1)]]
        if (eval_univariate(c, 0) + eval_univariate(c, 1)) % P != claim:
            return False, claim, point
        for x in c:
            tr.append_field(x)
        ch = tr.challenge()
        point.append(ch)
        claim = eval_univariate(c, ch)
    return True, claim, point


def check_proof(tables, proof, fiat_shamir=True):
    """asserts what a verifier with oracle access to the factors checks of an honest proof"""
    claimed, rounds, point, evals, fe = proof
    d, v = len(tables), len(point)
    pt = [int(x) for x in point]
    if fiat_shamir:
        ok, expected, drawn = claim_chain(claimed, rounds, v, d)
        assert ok and drawn == pt
    else:
        expected = int(claimed)
        for j in range(v):
            c = [int(x) for x in rounds[(d + 1) * j: (d + 1) * (j + 1)]]
            assert (eval_univariate(c, 0) + eval_univariate(c, 1)) % P == expected
            expected = eval_univariate(c, pt[j])
    assert expected == int(fe)  # g_v(r_v) == final_eval
    prod = 1
    for f, e in zip(tables, evals):
        assert int(e) == O.mle_eval(P, f, pt[::-1])  # the prover binds MSB-first: the factor's extension at the reversed point
        prod = prod * int(e) % P
    assert prod == int(fe)


def same(a, b):
    """two proofs are equal word for word"""
    return (int(a[0]) == int(b[0]) and np.array_equal(np.asarray(a[1], dtype=np.uint64), np.asarray(b[1], dtype=np.uint64))
            and np.array_equal(np.asarray(a[2], dtype=np.uint64), np.asarray(b[2], dtype=np.uint64))
            and np.array_equal(np.asarray(a[3], dtype=np.uint64), np.asarray(b[3], dtype=np.uint64)) and int(a[4]) == int(b[4]))
