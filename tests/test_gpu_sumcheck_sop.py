"""The batched sum-of-products sumcheck on the GPU (zigz_[dev_]sumcheck_prove_sop_batch, zigz_[dev_]sumcheck_verify_sop_batch):
every comparison is exact, word for word -- against the product entry where the statement is one it can prove (one term; a linear
combination; a difference of two products under fixed challenges), against sop_ref.py everywhere else."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as O
import sop_ref as S
import zerocheck_ref as Z

pytestmark = pytest.mark.gpu

P = O.P_BB
_P = np.uint64(P)
E = None
REV = 1  # ZIGZ_SUMCHECK_VERIFY_POINT_REVERSED


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
        self.lens = [len(t) for t in tables]
        self.extra = self.base + 4 * o

    def free(self):
        self.ctx.dev_free(self.base)


def rnd(seed, n):
    return O.splitmix64_field(seed, n)


def prove_dev(ctx, instances, challenges=None):
    """instances: [(host tables, terms)]; uploads the pools and calls the device form.  Also checks that the caller's tables are
    unchanged afterwards."""
    tabs = [t for pool, _ in instances for t in pool]
    d = Dev(ctx, tabs)
    try:
        it = iter(d.ptrs)
        inst = [([next(it) for _ in pool], terms) for pool, terms in instances]
        out = ctx.dev_sumcheck_prove_sop_batch(inst, [len(pool[0]) for pool, _ in instances], challenges)
        for t, p in zip(tabs, d.ptrs):
            assert np.array_equal(ctx.download(p, len(t)), t)
        return out
    finally:
        d.free()


# ---------------------------------------------------------------- 1-3: against the existing product entry
@pytest.mark.parametrize("n", [1 << 12, 1 << 16])
@pytest.mark.parametrize("d", [1, 2, 3])
def test_one_term_is_the_product_entry(ctx, d, n):
    fs = [rnd(11000 + 7 * d + j + n.bit_length(), n) for j in range(d)]
    dv = Dev(ctx, fs)
    try:
        for ch in (None, [rnd(11050 + d, n.bit_length() - 1)]):
            want, = ctx.dev_sumcheck_prove_product_batch([dv.ptrs], [n], ch)
            got, = ctx.dev_sumcheck_prove_sop_batch([(dv.ptrs, [(1, tuple(range(d)))])], [n], ch)
            assert S.same(got, want)
    finally:
        dv.free()


def test_linear_terms_are_the_product_entry_on_the_combined_table(ctx):
    n = 1 << 14
    fs = [rnd(11100 + j, n) for j in range(4)]
    alphas = [int(x) for x in rnd(11110, 4)]
    comb = np.zeros(n, dtype=np.uint64)
    for a, f in zip(alphas, fs):
        comb = (comb + (np.uint64(a) * f) % _P) % _P
    dv = Dev(ctx, fs + [comb])
    try:
        want, = ctx.dev_sumcheck_prove_product_batch([[dv.ptrs[4]]], [n])
        got, = ctx.dev_sumcheck_prove_sop_batch([(dv.ptrs[:4], [(a, (j,)) for j, a in enumerate(alphas)])], [n])
        assert got[0] == want[0] and np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2]) and got[4] == want[4]
    finally:
        dv.free()


def test_large_zero_check_rounds_are_the_difference_of_two_product_proofs(ctx):
    """pool {eq, a, b, c}, terms (1; eq a b) and (p - 1; eq c) at 2^20 and 2^22 under fixed challenges: every round word is R_1 - R_2
    of the product entry's proofs of {eq, a, b} and {eq, c} (R_2 padded with a zero cubic coefficient).  2^22 has 512 workgroups: the
    finish launch's loop over the partials makes a second trip."""
    ns = [1 << 20, 1 << 22]
    pools = [[rnd(11200 + 10 * i + j, n) for j in range(4)] for i, n in enumerate(ns)]
    ch = [rnd(11250 + i, n.bit_length() - 1) for i, n in enumerate(ns)]
    dv = Dev(ctx, [t for pool in pools for t in pool])
    try:
        ptr = [dv.ptrs[4 * i: 4 * i + 4] for i in range(2)]
        terms = [(1, (0, 1, 2)), (P - 1, (0, 3))]
        got = ctx.dev_sumcheck_prove_sop_batch([(ptr[0], terms), (ptr[1], terms)], ns, ch)
        prod = ctx.dev_sumcheck_prove_product_batch([ptr[0][:3], [ptr[0][0], ptr[0][3]], ptr[1][:3], [ptr[1][0], ptr[1][3]]],
                                                    [ns[0], ns[0], ns[1], ns[1]], [ch[0], ch[0], ch[1], ch[1]])
        for i, n in enumerate(ns):
            v = n.bit_length() - 1
            r1 = prod[2 * i][1].reshape(v, 4)
            r2 = np.concatenate([prod[2 * i + 1][1].reshape(v, 3), np.zeros((v, 1), dtype=np.uint64)], axis=1)
            assert np.array_equal(got[i][1].reshape(v, 4), (r1 + _P - r2) % _P), n
            assert got[i][0] == (prod[2 * i][0] + P - prod[2 * i + 1][0]) % P
            assert np.array_equal(got[i][2], ch[i])
            assert np.array_equal(got[i][3], np.concatenate([prod[2 * i][3], prod[2 * i + 1][3][1:]]))
            assert got[i][4] == S.combine(terms, got[i][3])
    finally:
        dv.free()


# ---------------------------------------------------------------- 4: against the reference
SIZES = [2, 1024, 2048, 8192, 16384, 1 << 17]  # 1024: tail only; 2048: first live length, one partial workgroup; 8192: one chunk


@pytest.mark.parametrize("M,T", [(1, 1), (4, 2), (8, 8)])
@pytest.mark.parametrize("n", SIZES)
def test_equals_the_reference(ctx, n, M, T):
    pool = [rnd(11300 + 31 * n.bit_length() + 3 * M + j, n) for j in range(M)]
    terms = S.structure(M, T, seed=n.bit_length() + M)
    ch = rnd(11350 + M, n.bit_length() - 1)
    fs, fixed = prove_dev(ctx, [(pool, terms)])[0], prove_dev(ctx, [(pool, terms)], [ch])[0]
    assert S.same(fs, S.prove(pool, terms)), "Fiat-Shamir"
    assert S.same(fixed, S.prove(pool, terms, ch)), "fixed challenges"


@pytest.fixture(scope="module")
def mixed():
    """different M, T, D and lengths 2^1 .. 2^14 plus one 2^20: the live set shrinks in stages.  (instances, reference proofs)"""
    shapes = [(1, 1, 1), (2, 3, 2), (14, 8, 8), (5, 1, 1), (20, 4, 2), (11, 3, 3), (12, 8, 5), (10, 2, 2), (13, 4, 8), (3, 2, 1)]
    inst = []
    for i, (v, M, T) in enumerate(shapes):
        pool = [rnd(11400 + 13 * i + j, 1 << v) for j in range(M)]
        inst.append((pool, S.structure(M, T, seed=i)))
    inst[3] = (inst[3][0], [(5, (0,))])  # D = 1
    inst[7] = (inst[7][0], [(P - 1, (0, 1)), (3, (1,))])  # D = 2
    assert {S.degree(t) for _, t in inst} == {1, 2, 3}
    return inst, [S.prove(pool, terms) for pool, terms in inst]


def test_mixed_batch_then_reversed_then_again(ctx, mixed):
    """no stale partial or workspace word survives from one call into the next"""
    inst, ref = mixed
    for order in (1, -1, 1):
        got = prove_dev(ctx, inst[::order])
        for g, r in zip(got, ref[::order]):
            assert S.same(g, r)


# ---------------------------------------------------------------- 5: saturation
@pytest.mark.parametrize("n", [1 << 13, 1 << 20])
def test_saturated_cubic_terms(ctx, n):
    """all words p - 1, 8 terms of degree 3, alphas p - 1: every raw product is maximal"""
    pool = [np.full(n, P - 1, dtype=np.uint64)] * 3
    terms = [(P - 1, (t % 3, (t + 1) % 3, (t + 2) % 3)) for t in range(8)]
    assert S.same(prove_dev(ctx, [(pool, terms)])[0], S.prove(pool, terms))


def test_saturated_steps_of_degree_two(ctx):
    """low half 0, high half p - 1 at 2^20: a = 0 and e = p - 1 at every pair of round 0"""
    n = 1 << 20
    step = np.concatenate([np.zeros(n // 2, dtype=np.uint64), np.full(n // 2, P - 1, dtype=np.uint64)])
    pool = [step, step]
    terms = [(P - 1, (0, 1))] * 4 + [(P - 1, (1, 1))] * 4
    assert S.same(prove_dev(ctx, [(pool, terms)])[0], S.prove(pool, terms))


@pytest.mark.parametrize("n", [1 << 11, 1 << 13])
def test_edge_alphas_and_challenges(ctx, n):
    v = n.bit_length() - 1
    pool = [rnd(11500 + j + v, n) for j in range(3)]
    inst, chs = [], []
    for alpha in (0, 1, P - 1):
        for c in (0, 1, P - 1):
            inst.append((pool, [(alpha, (0, 1, 2)), (alpha, (1, 2)), (alpha, (2,))]))
            chs.append(np.full(v, c, dtype=np.uint64))
    got = prove_dev(ctx, inst, chs)
    for (pl, terms), ch, g in zip(inst, chs, got):
        assert S.same(g, S.prove(pl, terms, ch))


# ---------------------------------------------------------------- 6: nothing behind the outputs is written
def _raw_prove(ctx, fn, ptr_t, ptrs, pool_sizes, all_terms, ns, fill=0xABCDEF):
    """the raw entry over prefilled output buffers with room behind them: (status, bad_index, the five buffers)"""
    from zigz_amd._ffi import u64p, u8p
    k = len(ns)
    nt, dg, (ix, ixp), (co, cop) = ctx._sop_terms(all_terms)
    outs = [np.full(4096, fill, dtype=np.uint64) for _ in range(5)]
    bad = C.c_size_t(2 ** 64 - 1)
    rc = fn(ctx.h, k, (C.c_uint * max(k, 1))(*pool_sizes), (ptr_t * max(len(ptrs), 1))(*ptrs), (C.c_size_t * max(k, 1))(*ns), nt, dg, ixp,
            cop, None, *[o.ctypes.data_as(u64p) for o in outs], C.byref(bad))
    return rc, bad.value, outs


def test_words_behind_the_outputs_are_untouched(ctx):
    from zigz_amd._ffi import lib, vp
    ns = [1 << 12, 1 << 5]
    pools = [[rnd(11600 + j, ns[0]) for j in range(3)], [rnd(11610 + j, ns[1]) for j in range(2)]]
    terms = [[(7, (0, 1, 2)), (9, (2,))], [(3, (0, 1))]]
    dv = Dev(ctx, pools[0] + pools[1])
    try:
        rc, bad, outs = _raw_prove(ctx, lib.zigz_dev_sumcheck_prove_sop_batch, vp, dv.ptrs, [3, 2], terms, ns)
        assert rc == 0 and bad == 2 ** 64 - 1
        used = [2, 4 * 12 + 3 * 5, 12 + 5, 3 + 2, 2]
        ref = [S.prove(p, t) for p, t in zip(pools, terms)]
        for o, u in zip(outs, used):
            assert np.all(o[u:] == 0xABCDEF) and np.all(o[:u] != 0xABCDEF)
        assert [int(x) for x in outs[0][:2]] == [r[0] for r in ref] and [int(x) for x in outs[4][:2]] == [r[4] for r in ref]
        assert np.array_equal(outs[1][:used[1]], np.concatenate([r[1] for r in ref]))
        assert np.array_equal(outs[3][:used[3]], np.concatenate([r[3] for r in ref]))
    finally:
        dv.free()


# ---------------------------------------------------------------- 7: host form
def test_host_form_equals_the_device_form(ctx, mixed):
    inst, ref = mixed
    sub = [inst[i] for i in (0, 2, 5, 7)]
    got = ctx.sumcheck_prove_sop_batch(sub)
    for g, i in zip(got, (0, 2, 5, 7)):
        assert S.same(g, ref[i])
    bad = [(list(pool), terms) for pool, terms in sub]
    t = bad[2][0][1].copy()
    t[77] = P
    bad[2][0][1] = t
    with pytest.raises(E.ZigzError) as e:
        ctx.sumcheck_prove_sop_batch(bad)
    assert e.value.code == E.NOT_CANONICAL and e.value.bad_index == 2


def test_prover_errors_name_the_first_failing_instance_and_touch_nothing(ctx):
    from zigz_amd._ffi import lib, vp
    n = 1 << 11
    dv = Dev(ctx, [rnd(11700 + j, n) for j in range(3)])
    try:
        p = dv.ptrs
        ok = [(1, (0, 1))]
        fn = lib.zigz_dev_sumcheck_prove_sop_batch
        for ptrs, sizes, terms, ns, code, idx in [
                (p, [2, 1], [ok, [(1, (0,))]], [n, 1], E.NO_VARIABLES, 1),
                (p, [2, 1], [ok, [(1, (0,))]], [n, 12], E.LENGTH_NOT_POWER_OF_TWO, 1),
                (p, [2, 1], [ok, [(1, (0,))]], [n, 1 << 31], E.INVALID_ARGUMENT, 1),
                (p, [2, 1], [ok, [(1, (1,))]], [n, n], E.INVALID_ARGUMENT, 1),         # pool index >= M
                (p, [2, 1], [ok, [(P, (0,))]], [n, n], E.NOT_CANONICAL, 1),            # coefficient >= p
                (p, [2, 1], [[(1, (0, 1, 1, 0))], [(1, (0,))]], [n, n], E.INVALID_ARGUMENT, 0),  # degree 4
                (p, [0, 1], [ok, [(1, (0,))]], [n, n], E.INVALID_ARGUMENT, 0),
                (p + [p[0]] * 7, [1, 9], [[(1, (0,))], [(1, (0,))]], [n, n], E.INVALID_ARGUMENT, 1),
                (p, [2, 1], [ok, [(1, (0,))] * 9], [n, n], E.INVALID_ARGUMENT, 1),
                ([p[0], p[1] + 4, p[2]], [1, 2], [[(1, (0,))], ok], [n, n], E.INVALID_ARGUMENT, 1),
                ([p[0], None, p[2]], [1, 2], [[(1, (0,))], ok], [n, n], E.INVALID_ARGUMENT, 1)]:
            rc, bad, outs = _raw_prove(ctx, fn, vp, ptrs, sizes, terms, ns)
            assert (rc, bad) == (code, idx) and all(np.all(o == 0xABCDEF) for o in outs), (sizes, terms, ns)
        rc, bad, outs = _raw_prove(ctx, fn, vp, [p[0]] * 4097, [1] * 4097, [[(1, (0,))]] * 4097, [n] * 4097)
        assert rc == E.INVALID_ARGUMENT and all(np.all(o == 0xABCDEF) for o in outs)
        rc, bad, outs = _raw_prove(ctx, fn, vp, [], [], [], [])
        assert rc == 0 and bad == 2 ** 64 - 1 and all(np.all(o == 0xABCDEF) for o in outs)
        with pytest.raises(E.ZigzError) as e:
            ctx.dev_sumcheck_prove_sop_batch([(p[:2], ok), (p[2:], [(1, (0,))])], [n, n], [np.zeros(11, np.uint64), np.full(11, P, np.uint64)])
        assert e.value.code == E.NOT_CANONICAL and e.value.bad_index == 1
    finally:
        dv.free()


# ---------------------------------------------------------------- 8: the zero-check of a constraint system, end to end
def test_zero_check_of_a_constraint_system(ctx):
    """C = alpha_1 (a b - c) + alpha_2 (d d - d) over the pool {eq, a, b, c, d}: four terms, one proof, one point.  SOUNDNESS NOTE:
    the verifier checks that the proof proves its claimed sum; that a zero-check's claimed sum IS zero is the caller's comparison."""
    n, v = 1 << 14, 14
    tau = [int(x) for x in rnd(11800, v)]
    a, b, d = rnd(11801, n), rnd(11802, n), rnd(11803, n) & np.uint64(1)
    a1, a2 = (int(x) for x in rnd(11804, 2))
    terms = [(a1, (0, 1, 2)), (P - a1, (0, 3)), (a2, (0, 4, 4)), (P - a2, (0, 4))]
    for spoiled in (False, True):
        c = (a * b) % _P
        if spoiled:
            c[n // 3] = (c[n // 3] + np.uint64(1)) % _P
        dv = Dev(ctx, [a, b, c, d], extra_words=n)
        try:
            ctx.dev_eq_table_batch([dv.extra], [n], [tau])
            pool = [dv.extra] + dv.ptrs
            proof, = ctx.dev_sumcheck_prove_sop_batch([(pool, terms)], [n])
            e = Z.eq_table(tau)
            assert S.same(proof, S.prove([e, a, b, c, d], terms))
            assert (proof[0] != 0) == spoiled
            if spoiled:  # - alpha_1 eq(tau, x) at the spoiled row
                assert proof[0] == (P - a1) * int(e[n // 3]) % P
            got = ctx.dev_sumcheck_verify_sop_batch([([None] + dv.ptrs, terms)], [n], [proof], REV, taus=[tau])
            assert got[0].tolist() == [1] and got[3] == 0 and got[1] == [proof[4]] and got[2] == [[int(x) for x in proof[3]]]
            mat = ctx.dev_sumcheck_verify_sop_batch([(pool, terms)], [n], [proof], REV)
            assert mat[0].tolist() == [1] and mat[1:] == got[1:]
        finally:
            dv.free()


# ---------------------------------------------------------------- 9: the verifier
def _oracles(pool, point, rev):
    q = [int(x) for x in point]
    q = q[::-1] if rev else q
    return [Z.eq_at(f.tau, q) if isinstance(f, Z.Eq) else O.mle_eval(P, f, q) for f in pool]


def _verdict(pool, terms, proof, rev, check_table_evals=True):
    """(accept, expected_eval, oracle_evals) restated on sumcheck_product_ref.claim_chain and the oracle's mle_eval"""
    import sumcheck_product_ref as R
    claimed, rounds, point, evals, fe = proof
    ok, expected, _ = R.claim_chain(claimed, rounds, len(point), S.degree(terms))
    orc = _oracles(pool, point, rev)
    o = S.combine(terms, orc)
    acc = ok and o == expected and o == int(fe) and (not check_table_evals or orc == [int(x) for x in evals])
    return bool(acc), expected, orc


def _verify_dev(ctx, items, flags, **kw):
    """items: [(pool, terms, proof)], a pool entry a host table or a Z.Eq"""
    tabs = [f for pool, _, _ in items for f in pool if not isinstance(f, Z.Eq)]
    dv = Dev(ctx, tabs)
    try:
        it = iter(dv.ptrs)
        inst = [([None if isinstance(f, Z.Eq) else next(it) for f in pool], terms) for pool, terms, _ in items]
        taus = [f.tau for pool, _, _ in items for f in pool if isinstance(f, Z.Eq)]
        return ctx.dev_sumcheck_verify_sop_batch(inst, [1 << len(pr[2]) for _, _, pr in items], [pr for _, _, pr in items], flags,
                                                 taus=taus or None, **kw)
    finally:
        dv.free()


def test_tampered_proofs_are_rejected(ctx):
    """one proof per tamper in one call at 2^6; oracle_evals is written for the rejected proofs too"""
    v, n = 6, 64
    tau = [int(x) for x in rnd(11900, v)]
    pool = [Z.Eq(tau), rnd(11901, n), rnd(11902, n), rnd(11903, n)]
    terms = [(int(rnd(11904, 1)[0]), (0, 1, 2)), (P - 1, (0, 3)), (5, (3,))]
    honest = S.prove([Z.eq_table(tau)] + pool[1:], terms)

    def bump(proof, field, at=0):
        p = [proof[0], proof[1].copy(), proof[2].copy(), proof[3].copy(), proof[4]]
        if field in (0, 4):
            p[field] = (p[field] + 1) % P
        else:
            p[field][at] = (int(p[field][at]) + 1) % P
        return tuple(p)

    items = [(pool, terms, honest), (pool, terms, bump(honest, 1, 4 * 3 + 1)), (pool, terms, bump(honest, 2, 2)),
             (pool, terms, bump(honest, 3, 1)), (pool, terms, bump(honest, 4)), (pool, terms, bump(honest, 0)),
             (pool, [(terms[0][0], terms[0][1]), ((terms[1][0] + 1) % P, terms[1][1]), terms[2]], honest)]
    verd, exp, orc, rej = _verify_dev(ctx, items, REV)
    want = [_verdict(pl, t, pr, True) for pl, t, pr in items]
    assert [w[0] for w in want] == [True] + [False] * 6  # the reference rejects every tamper
    assert [(bool(x), e, o) for x, e, o in zip(verd, exp, orc)] == want and rej == 6
    # the point as given: honest proofs of two or more variables are rejected in general, and the outputs are the reference's
    verd, exp, orc, rej = _verify_dev(ctx, items[:2], 0)
    assert [(bool(x), e, o) for x, e, o in zip(verd, exp, orc)] == [_verdict(pl, t, pr, False) for pl, t, pr in items[:2]]
    # without table_evals the changed table eval passes
    verd, _, _, rej = _verify_dev(ctx, [items[0], items[3]], REV, check_table_evals=False)
    assert verd.tolist() == [1, 1] and rej == 0


@pytest.mark.parametrize("flags", [0, REV])
def test_one_term_verifies_like_the_product_verifier(ctx, flags):
    items = []
    for n in (2, 1 << 5, 1 << 11, 1 << 14):
        for d in (1, 2, 3):
            items.append([rnd(12000 + 7 * d + j + n.bit_length() * 31, n) for j in range(d)])
    dv = Dev(ctx, [t for fs in items for t in fs])
    try:
        it = iter(dv.ptrs)
        inst = [[next(it) for _ in fs] for fs in items]
        ns = [len(fs[0]) for fs in items]
        proofs = ctx.dev_sumcheck_prove_product_batch(inst, ns)
        want = ctx.dev_sumcheck_verify_product_batch(inst, ns, proofs, flags)
        got = ctx.dev_sumcheck_verify_sop_batch([(p, [(1, tuple(range(len(p))))]) for p in inst], ns, proofs, flags)
        assert got[0].tolist() == want[0].tolist() and got[1:] == want[1:]
        if flags == REV:
            assert got[3] == 0
    finally:
        dv.free()


def test_a_call_with_only_eq_entries_launches_nothing_and_decides(ctx):
    v = 5
    t1, t2 = ([int(x) for x in rnd(12100 + j, v)] for j in range(2))
    terms = [(3, (0, 1)), (P - 2, (1,))]
    proof = S.prove([Z.eq_table(t1), Z.eq_table(t2)], terms)
    bad = (proof[0], proof[1], proof[2], proof[3], (proof[4] + 1) % P)
    got = ctx.dev_sumcheck_verify_sop_batch([([None, None], terms)] * 2, [1 << v] * 2, [proof, bad], REV, taus=[t1, t2, t1, t2])
    assert got[0].tolist() == [1, 0] and got[3] == 1
    assert got[2][0] == [Z.eq_at(t, [int(x) for x in proof[2]][::-1]) for t in (t1, t2)] == [int(x) for x in proof[3]]
    # the host form takes the same call (no table to narrow)
    assert ctx.sumcheck_verify_sop_batch([([None, None], terms)] * 2, [proof, bad], REV, taus=[t1, t2, t1, t2])[0].tolist() == [1, 0]


def test_verifier_statuses(ctx):
    n, v = 1 << 6, 6
    pool = [rnd(12200 + j, n) for j in range(2)]
    terms = [(7, (0, 1)), (1, (1,))]
    proof = S.prove(pool, terms)
    dv = Dev(ctx, pool)
    try:
        p = dv.ptrs

        def call(inst=None, ns=None, proofs=None, flags=REV, taus=None):
            return ctx.dev_sumcheck_verify_sop_batch(inst or [(p, terms)] * 2, ns or [n, n], proofs or [proof, proof], flags, taus=taus)

        assert call()[0].tolist() == [1, 1]
        over = (proof[0], proof[1].copy(), proof[2], proof[3], proof[4])
        over[1][5] = P
        for kw, code, idx in [
                (dict(flags=2), E.INVALID_ARGUMENT, None),
                (dict(inst=[(p, terms), (p + [p[0]] * 7, terms)]), E.INVALID_ARGUMENT, 1),        # M = 9
                (dict(inst=[(p, terms), (p, terms * 5)]), E.INVALID_ARGUMENT, 1),               # T = 10
                (dict(inst=[(p, terms), (p, [(1, (0, 1, 1, 1))])]), E.INVALID_ARGUMENT, 1),     # degree 4
                (dict(inst=[(p, terms), (p, [(1, (0, 2))])]), E.INVALID_ARGUMENT, 1),           # pool index >= M
                (dict(inst=[(p, terms), ([p[0], None], terms)]), E.INVALID_ARGUMENT, 1),        # an eq entry without eq_points
                (dict(inst=[(p, terms), ([p[0], p[1] + 4], terms)]), E.INVALID_ARGUMENT, 1),    # misaligned
                (dict(ns=[n, 1]), E.NO_VARIABLES, 1),
                (dict(ns=[n, 48]), E.LENGTH_NOT_POWER_OF_TWO, 1),
                (dict(proofs=[proof, over]), E.NOT_CANONICAL, 1),
                (dict(inst=[(p, terms), (p, [(P, (0, 1)), (1, (1,))])]), E.NOT_CANONICAL, 1),   # coefficient >= p
                (dict(inst=[([None, p[1]], terms), (p, terms)], taus=[[P] * v]), E.NOT_CANONICAL, 0)]:
            with pytest.raises(E.ZigzError) as e:
                call(**kw)
            assert e.value.code == code and (idx is None or e.value.bad_index == idx), kw
        # k == 0: ZIGZ_OK, *n_rejected = 0
        assert ctx.dev_sumcheck_verify_sop_batch([], [], [], REV)[3] == 0
    finally:
        dv.free()
