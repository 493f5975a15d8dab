"""Shared by the sumcheck-verification tests (CPU and GPU): tampered copies of a proof, and the verifier restated on top of the
oracle's transcript and eval -- the claim chain of SumcheckVerifier.verify (sumcheck_verifier.zig:58-93) with
VerificationResult.expected_eval, and the final check (:96-100) at the point as given or reversed."""
import numpy as np

import oracle_lib as O

P = O.P_BB


def claim_chain(claimed, rounds, v):
    """(rounds_ok, expected_eval): expected_eval is the claim at the failing round, or the final claim"""
    tr = O.Transcript()
    claim = int(claimed)
    for j in range(v):
        c0, c1 = int(rounds[2 * j]), int(rounds[2 * j + 1])
        if (2 * c0 + c1) % P != claim:
            return False, claim
        tr.append_field(c0)
        tr.append_field(c1)
        claim = (c0 + c1 * tr.challenge()) % P
    return True, claim


def verdict(table, claimed, rounds, point, fe, reversed_point=False):
    pt = [int(x) for x in point]
    ok, expected = claim_chain(claimed, rounds, len(pt))
    ev = O.mle_eval(P, table, pt[::-1] if reversed_point else pt)
    return bool(ok and ev == expected and ev == int(fe)), expected, ev


def tampered(claimed, rounds, point, fe):
    """[(kind, claimed, rounds, point, final_eval)]: the proof itself, then copies with ONE word changed (+1 mod p) -- a coefficient
    of the first, a middle and the last round, a point coordinate, final_eval, claimed_sum"""
    v = len(point)
    rounds = np.asarray(rounds, dtype=np.uint64)
    point = np.asarray(point, dtype=np.uint64)
    out = [("honest", int(claimed), rounds.copy(), point.copy(), int(fe))]

    def bump(a, i):
        b = a.copy()
        b[i] = (int(b[i]) + 1) % P
        return b

    for name, w in (("first", 0), ("middle", 2 * (v // 2) + 1), ("last", 2 * v - 2)):
        out.append(("round_" + name, int(claimed), bump(rounds, w), point.copy(), int(fe)))
    out.append(("point", int(claimed), rounds.copy(), bump(point, v // 2), int(fe)))
    out.append(("final_eval", int(claimed), rounds.copy(), point.copy(), (int(fe) + 1) % P))
    out.append(("claimed_sum", (int(claimed) + 1) % P, rounds.copy(), point.copy(), int(fe)))
    return out
