"""Exact, vectorised host reference of the multilinear operations (numpy uint64), for tables far beyond what the C oracle's
O(v * 2^v) eval and scalar loops can check in a test: a 2^27-element sumcheck takes about two seconds and a few GB.

Every value stays canonical (< p < 2^31) between steps, and every intermediate fits a u64 -- the bound is written next to
each line.  Semantics are those of src/poly/multilinear.zig and the sumcheck prover (oracle/zigz_oracle.c): bind
(partialEval) fixes the MOST significant index bit, eval's point[0] is the LEAST significant one.  tests/test_exact_ref_cpu.py
pins every function to the C oracle."""
import numpy as np

import oracle_lib as O

P = O.P_BB
_P = np.uint64(P)
assert P < 1 << 31


def canon(ev):
    """a copy of the table as canonical u64 (every entry < p)"""
    a = np.array(ev, dtype=np.uint64).reshape(-1)
    assert a.size and a.size & (a.size - 1) == 0, "the length must be a power of two"
    assert a.size <= 1 << 32  # half sums below: 2^31 terms < 2^31 each < 2^62
    assert not a.size or int(a.max()) < P, "not canonical"
    return a


def _fold(a0, a1, r):
    """a0 + r * (a1 - a0) mod p, entrywise, for canonical a0, a1 and r < p (a new array; the inputs are not written)"""
    d = a1 + _P                  # < 2^31 + 2^31 = 2^32
    d -= a0                      # in (0, 2^32): a1 + p - a0 > 0
    d *= np.uint64(r)            # < 2^31 * 2^32 = 2^63
    d += a0                      # < 2^63 + 2^31 < 2^64
    d %= _P
    return d


def bind(ev, r):
    """partialEval(r): out[i] = (1 - r) * ev[i] + r * ev[i + n/2]"""
    return _bind(canon(ev), r)


def _bind(a, r):
    assert a.size >= 2 and 0 <= int(r) < P
    h = a.size // 2
    return _fold(a[:h], a[h:], int(r))


def half_sums(ev):
    """exact u64 sums of the two halves (index MSB 0 / 1): each < 2^31 * 2^31 = 2^62"""
    return _half_sums(canon(ev))


def _half_sums(a):
    h = a.size // 2
    return int(a[:h].sum(dtype=np.uint64)), int(a[h:].sum(dtype=np.uint64))


def round_poly(ev):
    """roundPolynomial: [q(0), q(1) - q(0)] mod p"""
    return _round_poly(canon(ev))


def _round_poly(a):
    s0, s1 = _half_sums(a)
    c0, s1 = s0 % P, s1 % P
    return [c0, (s1 - c0) % P]  # Python ints


def total(ev):
    """sumOverHypercube mod p (u64 sum < 2^32 * 2^31 = 2^63)"""
    return int(canon(ev).sum(dtype=np.uint64)) % P


def eval(ev, point):  # noqa: A001 (the operation's name in multilinear.zig)
    """eval(point): point[0] is bound to the least significant index bit, point[v-1] to the most significant one"""
    a = canon(ev)
    nv = a.size.bit_length() - 1
    assert len(point) == nv
    for r in point:
        assert 0 <= int(r) < P
        pairs = a.reshape(-1, 2)  # pairs[j] = (a[2j], a[2j + 1]): the LSB is 0 / 1
        a = _fold(pairs[:, 0], pairs[:, 1], int(r))
    return int(a[0])


def sumcheck_prove(ev, challenges=None):
    """SumcheckProver.prove (Fiat-Shamir through the oracle's transcript) or proveInteractive(challenges).
    Returns (rounds[2v], point[v], final_eval) as u64 arrays and an int, like oracle_lib.sumcheck_prove."""
    a = canon(ev)
    nv = a.size.bit_length() - 1
    assert nv >= 1
    if challenges is not None:
        assert len(challenges) == nv
    rounds = np.zeros(2 * nv, dtype=np.uint64)
    point = np.zeros(nv, dtype=np.uint64)
    tr = O.Transcript() if challenges is None else None
    for k in range(nv):
        c0, c1 = _round_poly(a)
        rounds[2 * k], rounds[2 * k + 1] = c0, c1
        if tr is None:
            ch = int(challenges[k])
        else:
            tr.append_field(c0)
            tr.append_field(c1)
            ch = tr.challenge(P)
        point[k] = ch
        a = _bind(a, ch)
    return rounds, point, int(a[0])


# ---------------------------------------------------------------- inputs where kernels go wrong
PATTERNS = ("random", "all_pm1", "last_pm1", "block_pm1", "alternating", "ramp")
CHALLENGES = ("fs", "zero", "one", "pm1", "random")


def first_stage_k(nv):
    """the k of the first radix stage of a 2^nv sumcheck (api_mle.cpp radix_run): the block sums of 2^k blocks"""
    return min(nv - 8, 10) if nv > 10 else max(nv - 1, 0)


def pattern(name, nv, seed=0):
    """a 2^nv table of one of PATTERNS (u64, canonical)"""
    n = 1 << nv
    if name == "random":
        return O.splitmix64_field(0x5EED + 97 * nv + seed, n)
    if name == "all_pm1":
        return np.full(n, P - 1, dtype=np.uint64)
    a = np.zeros(n, dtype=np.uint64)
    if name == "last_pm1":
        a[-1] = P - 1
    elif name == "block_pm1":  # p - 1 throughout block 2^k - 1 of the first stage, 0 elsewhere
        k = first_stage_k(nv)
        b = n >> k
        a[((1 << k) - 1) * b: (1 << k) * b] = P - 1
    elif name == "alternating":
        a[1::2] = P - 1
    elif name == "ramp":
        a = np.arange(n, dtype=np.uint64) % _P
    else:
        raise ValueError(name)
    return a


def challenges(name, nv, seed=0):
    """a fixed challenge vector of CHALLENGES, or None for Fiat-Shamir ("fs")"""
    if name == "fs":
        return None
    if name == "zero":
        return np.zeros(nv, dtype=np.uint64)
    if name == "one":
        return np.ones(nv, dtype=np.uint64)
    if name == "pm1":
        return np.full(nv, P - 1, dtype=np.uint64)
    if name == "random":
        return O.splitmix64_field(0xC4A1 + 31 * nv + seed, nv)
    raise ValueError(name)
