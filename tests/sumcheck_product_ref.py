"""Shared by the product-sumcheck tests (CPU and GPU): the prover of sum_x prod_j f_j(x) restated in numpy on top of the oracle's
transcript and field -- SumcheckProver.prove (sumcheck_prover.zig:26-91) with the round polynomial
g(t) = sum_i prod_j (a_j + t (b_j - a_j)), a_j = f_j[i], b_j = f_j[i + m/2], in coefficient form c_0..c_d, partialEval's MSB-first
bind (multilinear.zig:166-173), a fresh transcript that absorbs c_0..c_d and then draws the challenge
(sumcheck_protocol.zig:176-184) -- and the verifier's claim chain for d + 1 coefficients per round (sumcheck_verifier.zig:172-205).
u64 arithmetic, reduced after every multiply (operands below p < 2^31: a product is below 2^62), so everything is exact."""
import numpy as np

import exact_ref
import oracle_lib as O

P = O.P_BB
_P = np.uint64(P)

# ---------------------------------------------------------------- inputs where the fused bind pass can go wrong
# exact_ref.PATTERNS plus two steps (exact_ref's tuple is iterated by the radix tests, so the new names live here)
STEPS = ("step_up", "step_down")
# constructed: no product of the other inputs reaches monty_reduce's equality (high word == subtracted word) except as 0 == 0.
# Here every 16-byte vector of index pairs holds a0 a1 = 1, p - 1, 1, p - 1: a lane's deferred low-word sum is a non-zero multiple
# of p (found by reasoning, not by search: 1 + (p - 1) = p), which monty_reduce must take to 0, not to p.
REDUCE_EDGE = ("one_pm1", "all_one")
PATTERN_SETS = (("all_pm1",) * 3, ("last_pm1",) * 3, ("step_down",) * 3, ("step_up",) * 3, ("alternating", "ramp", "random"),
                ("last_pm1", "all_pm1", "ramp"), ("step_down", "random", "step_up"))
EDGE_CHALLENGES = exact_ref.CHALLENGES + ("zero_pm1",)


def pattern(name, nv, seed=0):
    """exact_ref.pattern, and step_up (low half 0, high half p - 1) / step_down (low half p - 1, high half 0) / REDUCE_EDGE's two"""
    if name == "all_one":
        return np.ones(1 << nv, dtype=np.uint64)
    if name == "one_pm1":  # 1, p - 1, 1, p - 1, ...
        a = np.ones(1 << nv, dtype=np.uint64)
        a[1::2] = P - 1
        return a
    if name not in STEPS:
        return exact_ref.pattern(name, nv, seed)
    a = np.zeros(1 << nv, dtype=np.uint64)
    if name == "step_up":
        a[len(a) // 2:] = P - 1
    else:
        a[:len(a) // 2] = P - 1
    return a


def edge_challenges(name, nv):
    """exact_ref.challenges, and zero_pm1: 0, p - 1, 0, ... (None for Fiat-Shamir)"""
    if name != "zero_pm1":
        return exact_ref.challenges(name, nv)
    c = np.zeros(nv, dtype=np.uint64)
    c[1::2] = P - 1
    return c


def edge_cases(nv):
    """every (pattern names, challenge name) of the edge matrix at 2^nv: PATTERN_SETS x d = 1..3 (the first d patterns of the
    set) x EDGE_CHALLENGES -- 126 cases over 8 distinct tables (at d = 1 two sets' first patterns repeat: 114 are distinct)"""
    return [(ps[:d], c) for ps in PATTERN_SETS for d in (1, 2, 3) for c in EDGE_CHALLENGES]


def edge_pattern_names():
    return sorted({n for ps in PATTERN_SETS for n in ps} | set(REDUCE_EDGE))


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


exact_mle_eval = exact_ref.eval  # as check_proof's mle_eval: vectorised, for tables beyond the C oracle's O(v 2^v) eval


def check_proof(tables, proof, fiat_shamir=True, mle_eval=None):
    """asserts what a verifier with oracle access to the factors checks of an honest proof; mle_eval(table, point) evaluates a
    factor's multilinear extension (the C oracle's by default)"""
    if mle_eval is None:
        def mle_eval(f, pt):
            return O.mle_eval(P, f, pt)
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
        assert int(e) == mle_eval(f, pt[::-1])  # the prover binds MSB-first: the factor's extension at the reversed point
        prod = prod * int(e) % P
    assert prod == int(fe)


def same(a, b):
    """two proofs are equal word for word"""
    return (int(a[0]) == int(b[0]) and np.array_equal(np.asarray(a[1], dtype=np.uint64), np.asarray(b[1], dtype=np.uint64))
            and np.array_equal(np.asarray(a[2], dtype=np.uint64), np.asarray(b[2], dtype=np.uint64))
            and np.array_equal(np.asarray(a[3], dtype=np.uint64), np.asarray(b[3], dtype=np.uint64)) and int(a[4]) == int(b[4]))
