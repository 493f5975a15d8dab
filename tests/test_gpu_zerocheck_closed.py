"""The zero-check sumcheck with the eq factor in closed form on the GPU (zigz_[dev_]sumcheck_prove_zerocheck_batch,
zigz_[dev_]sumcheck_verify_zerocheck_batch): every comparison is exact, word for word -- against the existing route (the eq table
materialised by zigz_dev_eq_table_batch, appended to the pool and named by every term of zigz_dev_sumcheck_prove_sop_batch) where
deg C <= 2, against zerocheck_closed_ref.py everywhere else."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as O
import sop_ref as S
import zerocheck_closed_ref as ZC
import zerocheck_ref as Z

pytestmark = pytest.mark.gpu

P = O.P_BB
_P = np.uint64(P)
E = None
REV = 1  # ZIGZ_SUMCHECK_VERIFY_POINT_REVERSED
HALF = (P + 1) // 2
SPECIAL_TAU = [0, 1, HALF, P - 1]


@pytest.fixture(scope="module")
def ctx():
    import zigz_amd
    global E
    from zigz_amd import errors
    E = errors
    c = zigz_amd.Context(0)
    yield c


class Dev:
    """host tables uploaded one behind the other into one device buffer, each 16-byte aligned; room for eq tables behind them"""

    def __init__(self, ctx, tables, extra_words=0):
        self.ctx = ctx
        offs, o = [], 0
        for t in tables:
            offs.append(o)
            o += (len(t) + 3) // 4 * 4
        self.base = ctx.dev_alloc((o + extra_words + 4) * 4)
        if o:
            packed = np.zeros(o, dtype=np.uint64)
            for t, a in zip(tables, offs):
                packed[a: a + len(t)] = t
            ctx.upload(packed, self.base)
        self.ptrs = [self.base + 4 * a for a in offs]
        self.extra = self.base + 4 * o

    def free(self):
        self.ctx.dev_free(self.base)


def rnd(seed, n):
    return O.splitmix64_field(seed, n)


def mixed_tau(seed, v):
    """random words with 0, 1, (p + 1) / 2 and p - 1 mixed in"""
    tau = [int(x) for x in rnd(seed, v)]
    for j in range(v):
        if (j + seed) % 4 == 0:
            tau[j] = SPECIAL_TAU[(j + seed) // 4 % 4]
    return tau


def prove_dev(ctx, instances, challenges=None):
    """instances: [(host tables, terms, tau)]; uploads the pools and calls the device form.  Also checks that the caller's tables
    are unchanged afterwards."""
    tabs = [t for pool, _, _ in instances for t in pool]
    d = Dev(ctx, tabs)
    try:
        it = iter(d.ptrs)
        inst = [([next(it) for _ in pool], terms, tau) for pool, terms, tau in instances]
        out = ctx.dev_sumcheck_prove_zerocheck_batch(inst, [len(pool[0]) for pool, _, _ in instances], challenges)
        for t, p in zip(tabs, d.ptrs):
            assert np.array_equal(ctx.download(p, len(t)), t)
        return out
    finally:
        d.free()


def low_degree_terms(M, T, seed):
    """T terms of degree 1..2 over a pool of M tables (the table route has room for eq as a third factor): (1, 1) is f * f,
    (3, 2) is a * b - c, otherwise degrees alternate, an index repeats in every other quadratic term and the alphas cycle through
    random, 0, 1, p - 1"""
    if (M, T) == (1, 1):
        return [(int(rnd(seed, 1)[0]), (0, 0))]
    if (M, T) == (3, 2):
        return [(1, (0, 1)), (P - 1, (2,))]
    rng = np.random.default_rng(seed)
    special = [None, 0, 1, P - 1]
    terms = []
    for t in range(T):
        idx = [int(rng.integers(0, M)) for _ in range(1 + t % 2)]
        if len(idx) == 2 and t % 4 == 3:
            idx[1] = idx[0]
        a = special[t % 4]
        terms.append((int(rng.integers(0, P)) if a is None else a, tuple(idx)))
    return terms


def both_routes(ctx, pool, terms, tau, challenges=None):
    """(the closed-form entry's proof, the table route's proof in the same shape) of one instance, both on the device"""
    n, M = len(pool[0]), len(pool)
    dv = Dev(ctx, pool, extra_words=n)
    try:
        ctx.dev_eq_table_batch([dv.extra], [n], [tau])
        full, tt = ZC.table_route(dv.ptrs, terms, dv.extra)
        want, = ctx.dev_sumcheck_prove_sop_batch([(full, tt)], [n], challenges)
        got, = ctx.dev_sumcheck_prove_zerocheck_batch([(dv.ptrs, terms, tau)], [n], challenges)
        for t, p in zip(pool, dv.ptrs):
            assert np.array_equal(ctx.download(p, n), t)
        return got, ZC.from_sop(want, M)
    finally:
        dv.free()


# ---------------------------------------------------------------- 1: word for word against the existing entry, deg C <= 2
# 11: round 0 only is live and a workgroup's block is larger than the pair count; 12: the first bind, 1024 next-round pairs; 13:
# exactly one full round-0 block; 14: two blocks, hi is non-trivial in round 0; 17: many workgroups, hi shrinks over six rounds
@pytest.mark.parametrize("M,T", [(1, 1), (3, 2), (7, 8)])
@pytest.mark.parametrize("v", [11, 12, 13, 14, 17])
def test_equals_the_table_route_word_for_word(ctx, v, M, T):
    pool = [rnd(21000 + 31 * v + 3 * M + j, 1 << v) for j in range(M)]
    terms = low_degree_terms(M, T, seed=v + M)
    got, want = both_routes(ctx, pool, terms, mixed_tau(21050 + v + M, v))
    assert ZC.same(got, want)
    assert len(got[1]) == (S.degree(terms) + 2) * v and len(got[3]) == M


def test_equals_the_table_route_at_2_to_the_20(ctx):
    v, n = 20, 1 << 20
    pool = [rnd(21100 + j, n) for j in range(3)]
    terms = low_degree_terms(3, 2, 0)
    tau = mixed_tau(21110, v)
    got, want = both_routes(ctx, pool, terms, tau)
    assert ZC.same(got, want), "Fiat-Shamir"
    ch = [rnd(21120, v)]
    got, want = both_routes(ctx, pool, terms, tau, ch)
    assert ZC.same(got, want) and np.array_equal(got[2], ch[0]), "fixed challenges"


# ---------------------------------------------------------------- 2: against the Python reference, deg C = 3 included
def test_tails_equal_the_reference(ctx):
    """v = 1..10 in one call: host rounds only, mixed degrees up to 3 (rounds of up to 5 coefficients)"""
    inst = []
    for v in range(1, 11):
        M, T = [(1, 1), (4, 3), (8, 8)][v % 3]
        inst.append(([rnd(21200 + 13 * v + j, 1 << v) for j in range(M)], S.structure(M, T, seed=v), mixed_tau(21250 + v, v)))
    assert {S.degree(t) for _, t, _ in inst} >= {3}
    for g, (pool, terms, tau) in zip(prove_dev(ctx, inst), inst):
        assert ZC.same(g, ZC.prove(pool, terms, tau))


@pytest.mark.parametrize("M,T", [(1, 1), (4, 3), (8, 8)])
@pytest.mark.parametrize("v", [11, 12, 13, 14])
def test_equals_the_reference(ctx, v, M, T):
    pool = [rnd(21300 + 31 * v + 3 * M + j, 1 << v) for j in range(M)]
    terms = S.structure(M, T, seed=v + M)
    tau = mixed_tau(21350 + v, v)
    ch = rnd(21360 + M, v)
    assert ZC.same(prove_dev(ctx, [(pool, terms, tau)])[0], ZC.prove(pool, terms, tau)), "Fiat-Shamir"
    assert ZC.same(prove_dev(ctx, [(pool, terms, tau)], [ch])[0], ZC.prove(pool, terms, tau, ch)), "fixed challenges"


@pytest.fixture(scope="module")
def mixed():
    """different lengths, M, T and degrees in one call: the live set shrinks in stages.  (instances, reference proofs)"""
    shapes = [(1, 1, 1), (5, 2, 3), (10, 8, 8), (11, 3, 3), (12, 8, 5), (14, 4, 8), (16, 2, 2)]
    inst = []
    for i, (v, M, T) in enumerate(shapes):
        pool = [rnd(21400 + 13 * i + j, 1 << v) for j in range(M)]
        inst.append((pool, S.structure(M, T, seed=i), mixed_tau(21450 + i, v)))
    inst[0] = (inst[0][0], [(5, (0,))], inst[0][2])  # D = 1
    inst[6] = (inst[6][0], [(P - 1, (0, 1)), (3, (1,))], inst[6][2])  # D = 2
    assert {S.degree(t) for _, t, _ in inst} == {1, 2, 3}
    return inst, [ZC.prove(*x) for x in inst]


def test_mixed_batch_then_reversed_then_again(ctx, mixed):
    """no stale partial, weight or workspace word survives from one call into the next"""
    inst, ref = mixed
    for order in (1, -1, 1):
        got = prove_dev(ctx, inst[::order])
        for g, r in zip(got, ref[::order]):
            assert ZC.same(g, r)


# ---------------------------------------------------------------- 3: saturation
@pytest.mark.parametrize("v", [13, 14])
def test_saturated_inputs(ctx, v):
    """all tables p - 1, alphas p - 1, 8 terms of degree 3 all naming one table: every raw product is maximal; tau all p - 1, all
    0 and all 1 (indicator weights: every W but one is zero), and (p + 1) / 2 at the round-0 coordinate (2 tau - 1 = 0)"""
    n = 1 << v
    pool = [np.full(n, P - 1, dtype=np.uint64)]
    terms = [(P - 1, (0, 0, 0))] * 8
    half_first = [int(x) for x in rnd(21500 + v, v)]
    half_first[v - 1] = HALF  # round 0 binds the top index bit, which is tau[v - 1]'s
    taus = ([P - 1] * v, [0] * v, [1] * v, half_first)
    # ... and the same taus over random tables with terms of every degree, where the differences b - a do not vanish
    rpool = [rnd(21510 + v + j, n) for j in range(3)]
    rterms = [(P - 1, (0, 1, 2)), (HALF, (1, 1)), (1, (2,))]
    inst = [(pool, terms, tau) for tau in taus] + [(rpool, rterms, tau) for tau in taus]
    got = prove_dev(ctx, inst)
    for g, (pl, tm, tau) in zip(got, inst):
        assert ZC.same(g, ZC.prove(pl, tm, tau)), tau[:2]
    assert int(got[7][1][4]) == 0  # the linear factor of round 0 is the constant 1/2: no X^4 term


# ---------------------------------------------------------------- 4: guards
def _raw_prove(ctx, fn, ptr_t, ptrs, pool_sizes, all_terms, taus, ns, fill=0xABCDEF, no_taus=False):
    """the raw entry over prefilled output buffers with room behind them: (status, bad_index, the six buffers)"""
    from zigz_amd._ffi import u64p
    k = len(ns)
    nt, dg, (ix, ixp), (co, cop) = ctx._sop_terms(all_terms)
    tq, tp = ctx._cat_u64(taus)
    outs = [np.full(4096, fill, dtype=np.uint64) for _ in range(6)]
    bad = C.c_size_t(2 ** 64 - 1)
    rc = fn(ctx.h, k, (C.c_uint * max(k, 1))(*pool_sizes), (ptr_t * max(len(ptrs), 1))(*ptrs), (C.c_size_t * max(k, 1))(*ns), nt, dg, ixp,
            cop, None if no_taus else tp, None, *[o.ctypes.data_as(u64p) for o in outs], C.byref(bad))
    return rc, bad.value, outs


def test_words_behind_the_outputs_are_untouched(ctx):
    from zigz_amd._ffi import lib, vp
    ns = [1 << 12, 1 << 5]
    pools = [[rnd(21600 + j, ns[0]) for j in range(3)], [rnd(21610 + j, ns[1]) for j in range(2)]]
    terms = [[(7, (0, 1, 2)), (9, (2,))], [(3, (0, 1))]]
    taus = [mixed_tau(21620, 12), mixed_tau(21621, 5)]
    dv = Dev(ctx, pools[0] + pools[1])
    try:
        rc, bad, outs = _raw_prove(ctx, lib.zigz_dev_sumcheck_prove_zerocheck_batch, vp, dv.ptrs, [3, 2], terms, taus, ns)
        assert rc == 0 and bad == 2 ** 64 - 1
        used = [2, 5 * 12 + 4 * 5, 12 + 5, 3 + 2, 2, 2]  # claimed, rounds, points, table evals, eq evals, final evals
        ref = [ZC.prove(p, t, tau) for p, t, tau in zip(pools, terms, taus)]
        for o, u in zip(outs, used):
            assert np.all(o[u:] == 0xABCDEF) and np.all(o[:u] != 0xABCDEF)
        assert [int(x) for x in outs[0][:2]] == [r[0] for r in ref]
        assert np.array_equal(outs[1][:used[1]], np.concatenate([r[1] for r in ref]))
        assert np.array_equal(outs[3][:used[3]], np.concatenate([r[3] for r in ref]))
        assert [int(x) for x in outs[4][:2]] == [r[4] for r in ref] and [int(x) for x in outs[5][:2]] == [r[5] for r in ref]
    finally:
        dv.free()


def test_host_form_equals_the_device_form(ctx, mixed):
    inst, ref = mixed
    sub = [inst[i] for i in (0, 2, 3, 5)]
    got = ctx.sumcheck_prove_zerocheck_batch(sub)
    for g, i in zip(got, (0, 2, 3, 5)):
        assert ZC.same(g, ref[i])
    bad = [(list(pool), terms, tau) for pool, terms, tau in sub]
    t = bad[2][0][1].copy()
    t[77] = P
    bad[2][0][1] = t
    with pytest.raises(E.ZigzError) as e:
        ctx.sumcheck_prove_zerocheck_batch(bad)
    assert e.value.code == E.NOT_CANONICAL and e.value.bad_index == 2
    # ... and the host verifier decides like the device one
    verd = ctx.sumcheck_verify_zerocheck_batch(sub, got, REV)
    assert verd[0].tolist() == [1] * 4 and verd[3] == 0


def test_prover_errors_name_the_first_failing_instance_and_touch_nothing(ctx):
    from zigz_amd._ffi import lib, vp
    n, v = 1 << 11, 11
    dv = Dev(ctx, [rnd(21700 + j, n) for j in range(3)])
    try:
        p = dv.ptrs
        ok, one = [(1, (0, 1))], [(1, (0,))]
        tau = [5] * v
        fn = lib.zigz_dev_sumcheck_prove_zerocheck_batch
        for ptrs, sizes, terms, taus, ns, code, idx in [
                (p, [2, 1], [ok, one], [tau, []], [n, 1], E.NO_VARIABLES, 1),
                (p, [2, 1], [ok, one], [tau, [5] * 3], [n, 12], E.LENGTH_NOT_POWER_OF_TWO, 1),
                (p, [2, 1], [ok, one], [tau, [5] * 31], [n, 1 << 31], E.INVALID_ARGUMENT, 1),
                (p, [2, 1], [ok, [(1, (1,))]], [tau, tau], [n, n], E.INVALID_ARGUMENT, 1),          # pool index >= M
                (p, [2, 1], [ok, [(P, (0,))]], [tau, tau], [n, n], E.NOT_CANONICAL, 1),             # coefficient >= p
                (p, [2, 1], [[(1, (0, 1, 1, 0))], one], [tau, tau], [n, n], E.INVALID_ARGUMENT, 0),  # deg C = 4
                (p, [0, 1], [ok, one], [tau, tau], [n, n], E.INVALID_ARGUMENT, 0),
                (p + [p[0]] * 7, [1, 9], [one, one], [tau, tau], [n, n], E.INVALID_ARGUMENT, 1),
                ([p[0], p[1] + 4, p[2]], [1, 2], [one, ok], [tau, tau], [n, n], E.INVALID_ARGUMENT, 1),
                ([p[0], None, p[2]], [1, 2], [one, ok], [tau, tau], [n, n], E.INVALID_ARGUMENT, 1),
                (p, [2, 1], [ok, one], [tau, [5] * 10 + [P]], [n, n], E.NOT_CANONICAL, 1),           # a tau word >= p
                (p, [2, 1], [ok, one], [[P] + [5] * 10, tau], [n, 12], E.NOT_CANONICAL, 0),          # ... in front of a bad shape
                (p, [2, 1], [ok, one], [tau, [P] * 3], [n, 12], E.LENGTH_NOT_POWER_OF_TWO, 1)]:      # the shape before the tau
            rc, bad, outs = _raw_prove(ctx, fn, vp, ptrs, sizes, terms, taus, ns)
            assert (rc, bad) == (code, idx) and all(np.all(o == 0xABCDEF) for o in outs), (sizes, terms, ns)
        rc, bad, outs = _raw_prove(ctx, fn, vp, p, [2, 1], [ok, one], [tau, tau], [n, n], no_taus=True)
        assert rc == E.INVALID_ARGUMENT and all(np.all(o == 0xABCDEF) for o in outs)
        rc, bad, outs = _raw_prove(ctx, fn, vp, [p[0]] * 4097, [1] * 4097, [one] * 4097, [[5]] * 4097, [2] * 4097)
        assert rc == E.INVALID_ARGUMENT and all(np.all(o == 0xABCDEF) for o in outs)
        rc, bad, outs = _raw_prove(ctx, fn, vp, [], [], [], [], [])
        assert rc == 0 and bad == 2 ** 64 - 1 and all(np.all(o == 0xABCDEF) for o in outs)
        with pytest.raises(E.ZigzError) as e:
            ctx.dev_sumcheck_prove_zerocheck_batch([(p[:2], ok, tau), (p[2:], one, tau)], [n, n],
                                                   [np.zeros(11, np.uint64), np.full(11, P, np.uint64)])
        assert e.value.code == E.NOT_CANONICAL and e.value.bad_index == 1
    finally:
        dv.free()


# ---------------------------------------------------------------- 5: end to end
def test_zero_check_of_a_constraint_system(ctx):
    """C = alpha_1 (a b - c) + alpha_2 (d d - d) over the pool {a, b, c, d}.  SOUNDNESS NOTE: the verifier checks that the proof
    proves its claimed sum; that a zero-check's claimed sum IS zero is the caller's comparison."""
    n, v = 1 << 14, 14
    tau = [int(x) for x in rnd(21800, v)]
    a, b, d = rnd(21801, n), rnd(21802, n), rnd(21803, n) & np.uint64(1)
    a1, a2 = (int(x) for x in rnd(21804, 2))
    terms = [(a1, (0, 1)), (P - a1, (2,)), (a2, (3, 3)), (P - a2, (3,))]
    for spoiled in (False, True):
        c = (a * b) % _P
        if spoiled:
            c[n // 3] = (c[n // 3] + np.uint64(1)) % _P
        dv = Dev(ctx, [a, b, c, d], extra_words=n)
        try:
            proof, = ctx.dev_sumcheck_prove_zerocheck_batch([(dv.ptrs, terms, tau)], [n])
            assert ZC.same(proof, ZC.prove([a, b, c, d], terms, tau))
            assert (proof[0] != 0) == spoiled
            if spoiled:  # - alpha_1 eq(tau, x) at the spoiled row
                assert proof[0] == (P - a1) * int(Z.eq_table(tau)[n // 3]) % P
            got = ctx.dev_sumcheck_verify_zerocheck_batch([(dv.ptrs, terms, tau)], [n], [proof], REV)
            assert got[0].tolist() == [1] and got[3] == 0 and got[1] == [proof[5]] and got[2] == [[int(x) for x in proof[3]]]
            # the EXISTING verifier takes the same proof with eq as a ZIGZ_FACTOR_EQ pool entry behind the tables
            full, tt = ZC.table_route(dv.ptrs, terms, None)
            sop_proof = (proof[0], proof[1], proof[2], np.concatenate([proof[3], np.array([proof[4]], dtype=np.uint64)]), proof[5])
            old = ctx.dev_sumcheck_verify_sop_batch([(full, tt)], [n], [sop_proof], REV, taus=[tau])
            assert old[0].tolist() == [1] and old[3] == 0 and old[1] == got[1] and old[2] == [got[2][0] + [proof[4]]]
        finally:
            dv.free()


def test_degree_four_instance_verifies(ctx):
    """C = a b c - e with e = a b c: rounds of 5 coefficients, which nothing else in the library can prove or verify"""
    n, v = 1 << 12, 12
    a, b, c = (rnd(21900 + j, n) for j in range(3))
    e = a * b % _P * c % _P
    tau = mixed_tau(21910, v)
    terms = [(1, (0, 1, 2)), (P - 1, (3,))]
    dv = Dev(ctx, [a, b, c, e])
    try:
        proof, = ctx.dev_sumcheck_prove_zerocheck_batch([(dv.ptrs, terms, tau)], [n])
        assert proof[0] == 0 and len(proof[1]) == 5 * v
        assert ZC.same(proof, ZC.prove([a, b, c, e], terms, tau))
        got = ctx.dev_sumcheck_verify_zerocheck_batch([(dv.ptrs, terms, tau)], [n], [proof], REV)
        assert got[0].tolist() == [1] and got[3] == 0
        assert (bool(got[0][0]), got[1][0], got[2][0]) == ZC.verdict([a, b, c, e], terms, tau, proof)
    finally:
        dv.free()


# ---------------------------------------------------------------- 6: the verifier
def _verify_dev(ctx, items, flags, **kw):
    """items: [(pool, terms, tau, proof)] with host tables"""
    tabs = [f for pool, _, _, _ in items for f in pool]
    dv = Dev(ctx, tabs)
    try:
        it = iter(dv.ptrs)
        inst = [([next(it) for _ in pool], terms, tau) for pool, terms, tau, _ in items]
        return ctx.dev_sumcheck_verify_zerocheck_batch(inst, [1 << len(pr[2]) for _, _, _, pr in items], [pr for _, _, _, pr in items],
                                                       flags, **kw)
    finally:
        dv.free()


def test_tampered_proofs_are_rejected(ctx):
    """the honest proof and one proof per tamper in one call at 2^12, at the first seed at which the reference rejects every
    tamper; oracle_evals is written for the rejected proofs too"""
    pool, terms, tau, honest, other = ZC.pinned(12)
    assert ZC.same(prove_dev(ctx, [(pool, terms, tau)])[0], honest)
    items = [(pool, terms, tau, honest)] + list(ZC.tampered(pool, terms, tau, honest, other).values())
    assert len(items) == 1 + len(ZC.TAMPERS)
    verd, exp, orc, rej = _verify_dev(ctx, items, REV)
    want = [ZC.verdict(*it) for it in items]
    assert [w[0] for w in want] == [True] + [False] * len(ZC.TAMPERS)  # the reference rejects every tamper
    assert [(bool(x), e, o) for x, e, o in zip(verd, exp, orc)] == want and rej == len(ZC.TAMPERS)
    # flags == 0, the point as given: honest proofs of two or more variables are rejected in general, and the outputs are the reference's
    verd, exp, orc, rej = _verify_dev(ctx, items[:2], 0)
    assert [(bool(x), e, o) for x, e, o in zip(verd, exp, orc)] == [ZC.verdict(*it, reversed_point=False) for it in items[:2]]
    assert verd.tolist() == [0, 0]
    # without table_evals / eq_evals the changed eval passes
    by_name = dict(zip(ZC.TAMPERS, items[1:]))
    verd, _, _, rej = _verify_dev(ctx, [items[0], by_name["table_eval"]], REV, check_table_evals=False)
    assert verd.tolist() == [1, 1] and rej == 0
    verd, _, _, rej = _verify_dev(ctx, [by_name["eq_eval"], by_name["table_eval"]], REV, check_eq_evals=False)
    assert verd.tolist() == [1, 0] and rej == 1


def test_verifier_statuses(ctx):
    n, v = 1 << 6, 6
    pool = [rnd(22000 + j, n) for j in range(2)]
    terms = [(7, (0, 1)), (1, (1,))]
    tau = mixed_tau(22010, v)
    proof = ZC.prove(pool, terms, tau)
    dv = Dev(ctx, pool)
    try:
        p = dv.ptrs

        def call(inst=None, ns=None, proofs=None, flags=REV):
            return ctx.dev_sumcheck_verify_zerocheck_batch(inst or [(p, terms, tau)] * 2, ns or [n, n], proofs or [proof, proof], flags)

        assert call()[0].tolist() == [1, 1]
        over = (proof[0], proof[1].copy(), proof[2], proof[3], proof[4], proof[5])
        over[1][4 * v - 1] = P  # the last word of the (D + 2) v round words
        for kw, code, idx in [
                (dict(flags=2), E.INVALID_ARGUMENT, None),
                (dict(inst=[(p, terms, tau), (p + [p[0]] * 7, terms, tau)]), E.INVALID_ARGUMENT, 1),        # M = 9
                (dict(inst=[(p, terms, tau), (p, terms * 5, tau)]), E.INVALID_ARGUMENT, 1),               # T = 10
                (dict(inst=[(p, terms, tau), (p, [(1, (0, 1, 1, 1))], tau)]), E.INVALID_ARGUMENT, 1),     # deg C = 4
                (dict(inst=[(p, terms, tau), (p, [(1, (0, 2))], tau)]), E.INVALID_ARGUMENT, 1),           # pool index >= M
                (dict(inst=[(p, terms, tau), ([p[0], None], terms, tau)]), E.INVALID_ARGUMENT, 1),        # a NULL table
                (dict(inst=[(p, terms, tau), ([p[0], p[1] + 4], terms, tau)]), E.INVALID_ARGUMENT, 1),    # misaligned
                (dict(ns=[n, 1]), E.NO_VARIABLES, 1),
                (dict(ns=[n, 48]), E.LENGTH_NOT_POWER_OF_TWO, 1),
                (dict(proofs=[proof, over]), E.NOT_CANONICAL, 1),
                (dict(inst=[(p, terms, tau), (p, [(P, (0, 1)), (1, (1,))], tau)]), E.NOT_CANONICAL, 1),   # coefficient >= p
                (dict(inst=[(p, terms, [P] * v), (p, terms, tau)]), E.NOT_CANONICAL, 0)]:                 # tau >= p
            with pytest.raises(E.ZigzError) as e:
                call(**kw)
            assert e.value.code == code and (idx is None or e.value.bad_index == idx), kw
        # k == 0: ZIGZ_OK, *n_rejected = 0
        assert ctx.dev_sumcheck_verify_zerocheck_batch([], [], [], REV)[3] == 0
    finally:
        dv.free()
