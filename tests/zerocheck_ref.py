"""Shared by the eq-table and product-verification tests (CPU and GPU): eq(tau, .) built straight from its definition, its
extension at a point in closed form, the verdict of SumcheckVerifier.verify (sumcheck_verifier.zig:48-108, 172-205) over a
product of factors on top of sumcheck_product_ref.claim_chain, and the tampered copies of a proof the tests reject.

A factor is a table (np.uint64 array) or Eq(tau): the table eq(tau, .) that a verifier never builds.  u64 arithmetic, reduced
after every multiply (operands below p < 2^31), so everything is exact."""
import numpy as np

import exact_ref
import oracle_lib as O
import sumcheck_product_ref as R

P = O.P_BB
_P = np.uint64(P)


class Eq:
    """the factor eq(tau, .), given by its tau alone"""

    def __init__(self, tau):
        self.tau = [int(t) for t in tau]


def eq_table(tau):
    """E[x] = prod_j (bit j of x ? tau_j : 1 - tau_j): tau[0] goes with the LSB of x (Multilinear.eval's convention)"""
    e = np.ones(1, dtype=np.uint64)
    for t in tau:  # variable j doubles the table: the new (high) index bit 0 -> 1 - tau_j, 1 -> tau_j
        t = int(t)
        e = np.concatenate([(e * np.uint64((1 - t) % P)) % _P, (e * np.uint64(t)) % _P])
    return e


def eq_at(tau, q):
    """the multilinear extension of eq(tau, .) at q: prod_j (tau_j q_j + (1 - tau_j)(1 - q_j))"""
    w = 1
    for t, x in zip(tau, q):
        t, x = int(t), int(x)
        w = w * ((t * x + (1 - t) * (1 - x)) % P) % P
    return w


def dot(a, b):
    """sum_x a[x] b[x] mod p (terms below p after the reduction: the u64 sum of fewer than 2^32 of them is exact)"""
    return int(np.sum((np.asarray(a, dtype=np.uint64) * np.asarray(b, dtype=np.uint64)) % _P, dtype=np.uint64)) % P


def materialise(factors):
    return [eq_table(f.tau) if isinstance(f, Eq) else np.asarray(f, dtype=np.uint64) for f in factors]


def verdict(factors, proof, reversed_point=False, check_factor_evals=True, mle_eval=exact_ref.eval):
    """(accept, expected_eval, oracle_evals): the rounds by R.claim_chain; every factor's extension at the proof's point (as
    given, or reversed), a table's by mle_eval, an Eq's in closed form; accept iff the rounds held, the oracles' product equals
    the last claim and final_eval, and (check_factor_evals) every oracle equals its factor eval"""
    claimed, rounds, point, evals, fe = proof
    d, pt = len(factors), [int(x) for x in point]
    ok, expected, _ = R.claim_chain(claimed, rounds, len(pt), d)
    q = pt[::-1] if reversed_point else pt
    orc = [eq_at(f.tau, q) if isinstance(f, Eq) else int(mle_eval(f, q)) for f in factors]
    prod = 1
    for x in orc:
        prod = prod * x % P
    good = ok and prod == expected and prod == int(fe)
    if check_factor_evals:
        good = good and orc == [int(x) for x in evals]
    return bool(good), int(expected), orc


TAMPERS = ("round_first", "round_middle", "round_last", "claimed_sum", "final_eval", "factor_eval", "point", "tau", "tables_swapped",
           "eq_as_other_table")


def tampered(factors, proof, other_table, other_tau):
    """{name: (factors, proof)} for every name of TAMPERS: an honest instance whose FIRST factor is an Eq with ONE thing changed.
    A word changes by + 1 mod p; tables_swapped replaces the last two factors (the tables) by other_table; eq_as_other_table passes the
    Eq factor as the materialised table of other_tau."""
    assert isinstance(factors[0], Eq) and len(factors) == 3
    claimed, rounds, point, evals, fe = proof
    d, v = len(factors), len(point)
    rounds, point, evals = (np.asarray(a, dtype=np.uint64) for a in (rounds, point, evals))

    def bump(a, i):
        b = a.copy()
        b[i] = (int(b[i]) + 1) % P
        return b

    out = {}
    for name, w in (("round_first", 0), ("round_middle", (d + 1) * (v // 2) + 1), ("round_last", (d + 1) * (v - 1) + d)):
        out[name] = (factors, (claimed, bump(rounds, w), point, evals, fe))
    out["claimed_sum"] = (factors, ((int(claimed) + 1) % P, rounds, point, evals, fe))
    out["final_eval"] = (factors, (claimed, rounds, point, evals, (int(fe) + 1) % P))
    out["factor_eval"] = (factors, (claimed, rounds, point, bump(evals, d - 1), fe))
    out["point"] = (factors, (claimed, rounds, bump(point, v // 2), evals, fe))
    tau = list(factors[0].tau)
    tau[v // 2] = (tau[v // 2] + 1) % P
    out["tau"] = ([Eq(tau)] + list(factors[1:]), proof)
    out["tables_swapped"] = ([factors[0], other_table, other_table], proof)
    out["eq_as_other_table"] = ([eq_table(other_tau)] + list(factors[1:]), proof)
    assert tuple(out) == TAMPERS
    return out


def zero_check(v, seed):
    """(factors, proof): the zero-check of g (g - 1) = 0 for a seeded 0/1 table g of 2^v entries under a seeded tau --
    factors [Eq(tau), g, g - 1], proof R.prove over the materialised eq table"""
    n = 1 << v
    tau = [int(x) for x in O.splitmix64_field(seed, v)]
    g = O.splitmix64_field(seed + 1, n) & np.uint64(1)
    gm1 = (g + np.uint64(P - 1)) % _P
    return [Eq(tau), g, gm1], R.prove([eq_table(tau), g, gm1])


_PINNED = {}


def pinned_zero_check(v):
    """(factors, proof, other_table, other_tau) for the tamper tests at 2^v, computed once: the first seed at which the
    reference rejects EVERY tamper (one that it happens to accept -- probability about v / p -- moves on to the next seed, so
    none is ever dropped)"""
    if v not in _PINNED:
        for seed in range(9000 + 100 * v, 9000 + 100 * v + 30, 10):
            factors, proof = zero_check(v, seed)
            other = O.splitmix64_field(seed + 2, 1 << v)
            other_tau = [int(x) for x in O.splitmix64_field(seed + 3, v)]
            if all(not verdict(fs, pr, reversed_point=True)[0] for fs, pr in tampered(factors, proof, other, other_tau).values()):
                _PINNED[v] = (factors, proof, other, other_tau)
                break
        else:
            raise AssertionError("no seed at which the reference rejects every tamper")
    return _PINNED[v]
