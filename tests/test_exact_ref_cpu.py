"""tests/exact_ref.py against the C oracle (CPU only): every operation at nv 0..14, for every value pattern and random tables,
with random, fixed and edge challenges -- entry for entry and, for the sumcheck, byte for byte."""
import numpy as np
import pytest

import exact_ref as E
import oracle_lib as O

P = O.P_BB
NVS = list(range(15))


def _tables(nv):
    yield from ((name, E.pattern(name, nv)) for name in E.PATTERNS)
    yield "random2", O.splitmix64_field(0xA11 + nv, 1 << nv)


def _scalars(nv):
    return (0, 1, P - 1, 2, int(O.splitmix64_field(0xB0 + nv, 1)[0]))


@pytest.mark.parametrize("nv", NVS)
def test_bind_sums_round_poly(nv):
    for name, ev in _tables(nv):
        assert E.total(ev) == O.mle_sum(P, ev), name
        if nv == 0:
            continue
        assert E.round_poly(ev) == O.mle_round_poly(P, ev), name
        s0, s1 = E.half_sums(ev)
        h = len(ev) // 2
        assert s0 == sum(int(x) for x in ev[:h]) and s1 == sum(int(x) for x in ev[h:]), name  # exact, not reduced
        for r in _scalars(nv):
            assert np.array_equal(E.bind(ev, r), O.mle_partial_eval(P, ev, r)), (name, r)


@pytest.mark.parametrize("nv", NVS)
def test_eval(nv):
    points = [[0] * nv, [1] * nv, [P - 1] * nv, ([1] + [0] * (nv - 1)) if nv else [],
              list(O.splitmix64_field(0xE0 + nv, nv)), list(O.splitmix64_field(0xE1 + nv, nv))]
    for name, ev in _tables(nv):
        for pt in points:
            assert E.eval(ev, pt) == O.mle_eval(P, ev, pt), (name, pt)
        if nv:
            assert E.eval(ev, [1] + [0] * (nv - 1)) == int(ev[1])  # point[0] is the LSB
            assert E.eval(ev, [0] * (nv - 1) + [1]) == int(ev[len(ev) // 2])


@pytest.mark.parametrize("nv", NVS[1:])
def test_sumcheck(nv):
    for name, ev in _tables(nv):
        for cname in E.CHALLENGES:
            chs = E.challenges(cname, nv)
            r, pt, fe = E.sumcheck_prove(ev, chs)
            r0, pt0, fe0 = O.sumcheck_prove(P, ev, chs)
            assert np.array_equal(r, r0) and np.array_equal(pt, pt0) and fe == fe0, (name, cname)
            assert O.sumcheck_to_bytes(r, pt, fe) == O.sumcheck_to_bytes(r0, pt0, fe0), (name, cname)
            if chs is not None:
                assert np.array_equal(pt, chs)


def test_patterns_are_what_they_say():
    nv = 20
    k = E.first_stage_k(nv)
    assert k == 10 and E.first_stage_k(13) == 5 and E.first_stage_k(27) == 10
    b = E.pattern("block_pm1", nv)
    blk = (1 << nv) >> k
    assert np.all(b[-blk:] == P - 1) and not b[:-blk].any()
    last = E.pattern("last_pm1", nv)
    assert last[-1] == P - 1 and not last[:-1].any()
    alt = E.pattern("alternating", nv)
    assert not alt[0::2].any() and np.all(alt[1::2] == P - 1)
    assert np.array_equal(E.pattern("ramp", 4), np.arange(16, dtype=np.uint64))
    assert np.all(E.pattern("all_pm1", 3) == P - 1)
    rnd = E.pattern("random", nv)
    assert int(rnd.max()) < P and len(set(rnd[:64].tolist())) == 64


def test_large_table_limits():
    """the worst case of every bound at a large size: all p - 1 with the challenge p - 1 (and a single hot entry)"""
    nv = 22
    ev = E.pattern("all_pm1", nv)
    assert E.half_sums(ev) == ((P - 1) << (nv - 1), (P - 1) << (nv - 1))
    assert E.total(ev) == ((P - 1) << nv) % P
    assert np.all(E.bind(ev, P - 1) == P - 1)  # a constant table binds to itself
    assert E.eval(ev, [P - 1] * nv) == P - 1
    r, pt, fe = E.sumcheck_prove(ev, E.challenges("pm1", nv))
    assert fe == P - 1
    hot = E.pattern("last_pm1", nv)
    # eval at point x of e_{n-1} * (p - 1) = (p - 1) * prod x_i; sumcheck binds MSB-first with the same product
    x = [int(v) for v in O.splitmix64_field(0x7, nv)]
    prod = 1
    for v in x:
        prod = prod * v % P
    assert E.eval(hot, x) == (P - 1) * prod % P
    assert E.sumcheck_prove(hot, x)[2] == (P - 1) * prod % P
