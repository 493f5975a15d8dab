"""Shared by the closed-form zero-check tests (CPU and GPU): the reference proof of an instance (pool, terms, tau) is the
sum-of-products reference's proof with the MATERIALISED eq table appended to the pool and named by every term (sop_ref.prove;
field arithmetic is exact, so the closed-form prover must write the same words), its table evals split into the pool's and eq's;
the verdict restates the verifier on sumcheck_product_ref.claim_chain with eq in closed form (zerocheck_ref.eq_at).

A proof is (claimed_sum, rounds [(D + 2) words per round, D = deg C], point, table_evals [M], eq_eval, final_eval)."""
import numpy as np

import exact_ref
import oracle_lib as O
import sop_ref as S
import sumcheck_product_ref as R
import zerocheck_ref as Z

P = O.P_BB


def table_route(pool, terms, tau_or_table):
    """the instance as the table route states it: (pool + [eq], terms with eq's index appended to every term)"""
    M = len(pool)
    return list(pool) + [tau_or_table], [(alpha, tuple(idx) + (M,)) for alpha, idx in terms]


def prove(pool, terms, tau, challenges=None):
    full, tt = table_route(pool, terms, Z.eq_table(tau))
    claimed, rounds, point, evals, fe = S.prove(full, tt, challenges)
    return claimed, rounds, point, evals[:len(pool)], int(evals[len(pool)]), fe


def same(a, b):
    return (int(a[0]) == int(b[0]) and np.array_equal(np.asarray(a[1], dtype=np.uint64), np.asarray(b[1], dtype=np.uint64))
            and np.array_equal(np.asarray(a[2], dtype=np.uint64), np.asarray(b[2], dtype=np.uint64))
            and np.array_equal(np.asarray(a[3], dtype=np.uint64), np.asarray(b[3], dtype=np.uint64))
            and int(a[4]) == int(b[4]) and int(a[5]) == int(b[5]))


def from_sop(proof, M):
    """the table route's proof (pool of M + 1, eq last) in this module's shape"""
    claimed, rounds, point, evals, fe = proof
    return claimed, rounds, point, evals[:M], int(evals[M]), fe


def verdict(pool, terms, tau, proof, reversed_point=True, check_table_evals=True, check_eq_eval=True, mle_eval=exact_ref.eval):
    """(accept, expected_eval, oracle_evals [M]): the rounds by claim_chain at D + 1; every table's extension at the proof's point
    (as given, or reversed), eq's in closed form; accept iff the rounds held, eq * C(oracles) equals the last claim and
    final_eval, and every checked eval equals its oracle"""
    claimed, rounds, point, evals, eq_eval, fe = proof
    pt = [int(x) for x in point]
    ok, expected, _ = R.claim_chain(claimed, rounds, len(pt), S.degree(terms) + 1)
    q = pt[::-1] if reversed_point else pt
    orc = [int(mle_eval(f, q)) for f in pool]
    e = Z.eq_at(tau, q)
    o = e * S.combine(terms, orc) % P
    good = ok and o == expected and o == int(fe)
    if check_table_evals:
        good = good and orc == [int(x) for x in evals]
    if check_eq_eval:
        good = good and e == int(eq_eval)
    return bool(good), int(expected), orc


TAMPERS = ("claimed_sum", "round", "point", "table_eval", "eq_eval", "final_eval", "tau", "table_swapped")


def tampered(pool, terms, tau, proof, other_table):
    """{name: (pool, terms, tau, proof)} for every name of TAMPERS: the honest instance with ONE thing changed.  A word changes
    by + 1 mod p; table_swapped replaces the first pool table by other_table."""
    claimed, rounds, point, evals, eq_eval, fe = proof
    rounds, point, evals = (np.asarray(a, dtype=np.uint64) for a in (rounds, point, evals))
    v = len(point)

    def bump(a, i):
        b = a.copy()
        b[i] = (int(b[i]) + 1) % P
        return b

    out = {
        "claimed_sum": (pool, terms, tau, ((int(claimed) + 1) % P, rounds, point, evals, eq_eval, fe)),
        "round": (pool, terms, tau, (claimed, bump(rounds, (S.degree(terms) + 2) * (v // 2) + 1), point, evals, eq_eval, fe)),
        "point": (pool, terms, tau, (claimed, rounds, bump(point, v // 2), evals, eq_eval, fe)),
        "table_eval": (pool, terms, tau, (claimed, rounds, point, bump(evals, len(evals) - 1), eq_eval, fe)),
        "eq_eval": (pool, terms, tau, (claimed, rounds, point, evals, (int(eq_eval) + 1) % P, fe)),
        "final_eval": (pool, terms, tau, (claimed, rounds, point, evals, eq_eval, (int(fe) + 1) % P)),
    }
    t2 = list(tau)
    t2[v // 2] = (int(t2[v // 2]) + 1) % P
    out["tau"] = (pool, terms, t2, proof)
    out["table_swapped"] = ([other_table] + list(pool[1:]), terms, tau, proof)
    assert tuple(out) == TAMPERS
    return out


def instance(v, seed, M=3, terms=None):
    """a seeded instance at 2^v: M random tables, a random tau, terms (default a*b - c)"""
    n = 1 << v
    pool = [O.splitmix64_field(seed + 1 + j, n) for j in range(M)]
    tau = [int(x) for x in O.splitmix64_field(seed, v)]
    return pool, terms or [(1, (0, 1)), (P - 1, (2,))], tau


_PINNED = {}


def pinned(v):
    """(pool, terms, tau, proof, other_table) for the tamper tests at 2^v, computed once: the first seed at which the reference
    rejects EVERY tamper, chosen as zerocheck_ref.pinned_zero_check chooses its seed, so that no tamper is ever dropped"""
    if v not in _PINNED:
        for seed in range(9500 + 100 * v, 9500 + 100 * v + 30, 10):
            pool, terms, tau = instance(v, seed)
            proof = prove(pool, terms, tau)
            other = O.splitmix64_field(seed + 7, 1 << v)
            if all(not verdict(*t)[0] for t in tampered(pool, terms, tau, proof, other).values()):
                _PINNED[v] = (pool, terms, tau, proof, other)
                break
        else:
            raise AssertionError("no seed at which the reference rejects every tamper")
    return _PINNED[v]
