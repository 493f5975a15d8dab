"""Batched product-proof verification on the GPU (zigz_dev_sumcheck_verify_product_batch, zigz_sumcheck_verify_product_batch) and
the zero-check end to end: verdicts, expected evals, oracle evals and the reject count equal SumcheckVerifier.verify as
zerocheck_ref restates it, for honest proofs of the GPU prover and for every tamper of the pinned set, under both point orders;
an eq factor given by its tau verifies like the materialised table; d = 1 is the linear verifier; argument errors write nothing."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as O
import zerocheck_ref as Z

pytestmark = pytest.mark.gpu

P = O.P_BB
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
        self.extra = self.base + 4 * o

    def free(self):
        self.ctx.dev_free(self.base)


def verify(ctx, items, flags, **kw):
    """items: [(factors, proof)] with host tables; uploads them and calls the device form"""
    tabs = [f for fs, _ in items for f in fs if not isinstance(f, Z.Eq)]
    d = Dev(ctx, tabs)
    try:
        it = iter(d.ptrs)
        inst = [[None if isinstance(f, Z.Eq) else next(it) for f in fs] for fs, _ in items]
        taus = [f.tau for fs, _ in items for f in fs if isinstance(f, Z.Eq)]
        ns = [1 << len(pr[2]) for _, pr in items]
        return ctx.dev_sumcheck_verify_product_batch(inst, ns, [pr for _, pr in items], flags, taus=taus or None, **kw)
    finally:
        d.free()


def check(got, items, rev, **kw):
    verd, exp, orc, rej = got
    want = [Z.verdict(fs, pr, reversed_point=rev, **kw) for fs, pr in items]
    assert [(bool(v), e, o) for v, e, o in zip(verd, exp, orc)] == want
    assert rej == sum(1 for w in want if not w[0])
    return want


@pytest.mark.parametrize("n", [2, 1 << 10, 1 << 11, 1 << 14, 1 << 20])
def test_zero_check_end_to_end(ctx, n):
    """eq table on the device -> product prover over [E_tau, g, g - 1] -> verifier with the eq factor given by tau alone.
    SOUNDNESS NOTE: the verifier checks that the proof proves its claimed sum; that a zero-check's claimed sum IS zero is the
    caller's comparison.  With one entry of g set to 2 the claimed sum is non-zero and the proof still verifies."""
    v = n.bit_length() - 1
    tau = [int(x) for x in O.splitmix64_field(9700 + v, v)]
    g = O.splitmix64_field(9710 + v, n) & np.uint64(1)
    for broken in (False, True):
        if broken:
            g = g.copy()
            g[n // 3] = 2
        gm1 = (g + np.uint64(P - 1)) % np.uint64(P)
        d = Dev(ctx, [g, gm1], extra_words=n)
        try:
            ctx.dev_eq_table_batch([d.extra], [n], [tau])
            proof, = ctx.dev_sumcheck_prove_product_batch([[d.extra, d.ptrs[0], d.ptrs[1]]], [n])
            e = Z.eq_table(tau)
            want_sum = Z.dot((e * g) % np.uint64(P), gm1)
            assert proof[0] == want_sum and (want_sum != 0) == broken
            a = ctx.dev_sumcheck_verify_product_batch([[None, d.ptrs[0], d.ptrs[1]]], [n], [proof], REV, taus=[tau])
            b = ctx.dev_sumcheck_verify_product_batch([[d.extra, d.ptrs[0], d.ptrs[1]]], [n], [proof], REV)
            assert a[0].tolist() == [1] and a[3] == 0 and a[1] == [proof[4]] and a[2] == [[int(x) for x in proof[3]]]
            assert b[0].tolist() == a[0].tolist() and b[1:] == a[1:]
            assert np.array_equal(ctx.download(d.extra, n), e)
        finally:
            d.free()


@pytest.fixture(scope="module")
def honest(ctx):
    """proofs of the GPU prover at d = 1, 2, 3 and n = 2 .. 2^20 over seeded tables, one batch"""
    items = []
    for n in (2, 1 << 5, 1 << 11, 1 << 14, 1 << 20):
        for d in (1, 2, 3):
            items.append([O.splitmix64_field(9800 + 7 * d + j + n.bit_length() * 31, n) for j in range(d)])
    dv = Dev(ctx, [t for fs in items for t in fs])
    it = iter(dv.ptrs)
    inst = [[next(it) for _ in fs] for fs in items]
    ns = [len(fs[0]) for fs in items]
    proofs = ctx.dev_sumcheck_prove_product_batch(inst, ns)
    yield items, inst, ns, proofs, dv
    dv.free()


@pytest.mark.parametrize("flags", [0, REV])
def test_honest_proofs_of_the_gpu_prover(ctx, honest, flags):
    items, inst, ns, proofs, dv = honest
    got = ctx.dev_sumcheck_verify_product_batch(inst, ns, proofs, flags)
    want = check(got, list(zip(items, proofs)), bool(flags))
    if flags:
        assert all(w[0] for w in want)
    else:  # the reference's point order: one variable accepts, seeded proofs of two or more do not
        assert [w[0] for w in want] == [n == 2 for n in ns]


def test_degree_one_is_the_linear_verifier(ctx, honest):
    items, inst, ns, proofs, dv = honest
    sel = [i for i, fs in enumerate(items) if len(fs) == 1]
    bumped = [(proofs[i][0], proofs[i][1], proofs[i][2], proofs[i][3], (proofs[i][4] + (j % 2)) % P) for j, i in enumerate(sel)]
    for flags in (0, REV):
        a = ctx.dev_sumcheck_verify_product_batch([inst[i] for i in sel], [ns[i] for i in sel], bumped, flags, check_factor_evals=False)
        b = ctx.dev_sumcheck_verify_batch([inst[i][0] for i in sel], [ns[i] for i in sel], [p[0] for p in bumped],
                                          [(p[1], p[2], p[4]) for p in bumped], flags)
        assert a[0].tolist() == b[0].tolist() and a[1] == b[1] and [o[0] for o in a[2]] == b[2] and a[3] == b[3]


@pytest.mark.parametrize("v", [11, 14])
def test_every_tamper(ctx, v):
    factors, proof, other, other_tau = Z.pinned_zero_check(v)
    cases = Z.tampered(factors, proof, other, other_tau)
    items = [(factors, proof)] + list(cases.values())
    want = check(verify(ctx, items, REV), items, True)
    assert [w[0] for w in want] == [True] + [False] * len(cases)
    check(verify(ctx, items, 0), items, False)


def test_4096_proofs_every_seventh_tampered(ctx):
    k, n, v = 4096, 1 << 10, 10
    tabs = [O.splitmix64_field(9900 + j, n) for j in range(6)]
    taus = [[int(x) for x in O.splitmix64_field(9910 + j, v)] for j in range(2)]
    protos = []
    for fs in ([tabs[0]], [tabs[1], tabs[2]], [Z.Eq(taus[0]), tabs[3], tabs[4]], [Z.Eq(taus[1]), tabs[5]]):
        protos.append((fs, Z.R.prove(Z.materialise(fs))))
    ref = {}
    items = []
    for i in range(k):
        fs, (c, r, q, ev, fe) = protos[i % len(protos)]
        bad = i % 7 == 0
        if bad:
            r = r.copy()
            r[(i // 7) % len(r)] = (int(r[(i // 7) % len(r)]) + 1) % P
        items.append((fs, (c, r, q, ev, fe), (i % len(protos), (i // 7) % len(r) if bad else -1)))
    d = Dev(ctx, tabs)
    try:
        ptr = {id(t): p for t, p in zip(tabs, d.ptrs)}
        inst = [[None if isinstance(f, Z.Eq) else ptr[id(f)] for f in fs] for fs, _, _ in items]
        tl = [f.tau for fs, _, _ in items for f in fs if isinstance(f, Z.Eq)]
        verd, exp, orc, rej = ctx.dev_sumcheck_verify_product_batch(inst, [n] * k, [pr for _, pr, _ in items], REV, taus=tl)
    finally:
        d.free()
    for (fs, pr, key), vd, e, o in zip(items, verd, exp, orc):
        if key not in ref:  # (every 7th proof has its own changed word; the honest ones repeat four prototypes)
            ref[key] = Z.verdict(fs, pr, reversed_point=True)
        assert (bool(vd), e, o) == ref[key], key
    assert rej == k - int(verd.sum()) and rej >= k // 7


def test_host_form_and_null_factor_evals(ctx):
    factors, proof, other, other_tau = Z.pinned_zero_check(11)
    items = [(factors, proof)] + list(Z.tampered(factors, proof, other, other_tau).values())
    got = ctx.sumcheck_verify_product_batch([[None if isinstance(f, Z.Eq) else f for f in fs] for fs, _ in items], [pr for _, pr in items],
                                            REV, taus=[f.tau for fs, _ in items for f in fs if isinstance(f, Z.Eq)])
    dev = verify(ctx, items, REV)
    assert got[0].tolist() == dev[0].tolist() and got[1:] == dev[1:]
    check(got, items, True)
    # factor_evals = NULL: factor evals 2 x and y / 2 have the right product and are not looked at
    c, r, q, ev, fe = proof
    inv2 = (P + 1) // 2
    wrong = np.array([ev[0], 2 * int(ev[1]) % P, int(ev[2]) * inv2 % P], dtype=np.uint64)
    item = [(factors, (c, r, q, wrong, fe))]
    assert check(verify(ctx, item, REV, check_factor_evals=False), item, True, check_factor_evals=False)[0][0] is True
    assert check(verify(ctx, item, REV), item, True)[0][0] is False
    # a call without a table factor launches nothing and still verifies
    tau2 = [int(x) for x in O.splitmix64_field(9950, 5)]
    only_eq = [([Z.Eq(tau2)], Z.R.prove([Z.eq_table(tau2)]))]
    assert check(verify(ctx, only_eq, REV), only_eq, True)[0][0] is True and only_eq[0][1][0] == 1


def test_argument_errors_write_nothing(ctx):
    from zigz_amd._ffi import lib, u8p, u64p, vp
    ns = [4, 8, 2, 16]
    degrees = [1, 3, 2, 3]
    kinds = [0, 1, 0, 0, 0, 0, 1, 0, 0]
    host = [O.splitmix64_field(9960 + j, ns[i]) for i, d in enumerate(degrees) for j in range(d)]
    dv = Dev(ctx, host)
    k, nf = len(ns), sum(degrees)
    cat = lambda n, seed: np.ascontiguousarray(O.splitmix64_field(seed, n))
    rounds, points, fev, taus, cs, fe = cat(2 * 2 + 4 * 3 + 3 * 1 + 4 * 4, 1), cat(10, 2), cat(nf, 3), cat(3 + 4, 4), cat(k, 5), cat(k, 6)

    def raw(dev, nn=ns, dg=degrees, kd=kinds, flags=0, edit=None, null=None, shift=None, with_taus=True, rejected=True, kk=k):
        arrs = dict(rounds=rounds.copy(), points=points.copy(), fev=fev.copy(), taus=taus.copy(), cs=cs.copy(), fe=fe.copy())
        if edit:
            arrs[edit[0]][edit[1]] = P
        verd = np.full(k, 7, dtype=np.uint8)
        out = np.full(k + nf, 0xABCDEF, dtype=np.uint64)
        n_rej, bad = C.c_size_t(999), C.c_size_t(12345)
        if dev:
            ptrs = (vp * nf)(*[None if kd[f] == 1 or null == f else dv.ptrs[f] + (4 if shift == f else 0) for f in range(nf)])
            fn = lib.zigz_dev_sumcheck_verify_product_batch
        else:
            ptrs = (u64p * nf)(*[None if kd[f] == 1 or null == f else host[f].ctypes.data_as(u64p) for f in range(nf)])
            fn = lib.zigz_sumcheck_verify_product_batch
        p = lambda a: a.ctypes.data_as(u64p)
        rc = fn(ctx.h, kk, (C.c_uint * k)(*dg), ptrs, np.array(kd, dtype=np.uint8).ctypes.data_as(u8p), p(arrs["taus"]) if with_taus else None,
                (C.c_size_t * k)(*nn), p(arrs["cs"]), p(arrs["rounds"]), p(arrs["points"]), p(arrs["fev"]), p(arrs["fe"]), flags,
                verd.ctypes.data_as(u8p), p(out), p(out[k:]), C.byref(n_rej) if rejected else None, C.byref(bad))
        return rc, bad.value, n_rej.value, bool(np.all(verd == 7) and np.all(out == 0xABCDEF))

    try:
        for dev in (True, False):
            rc, bad, n_rej, untouched = raw(dev)
            assert (rc, bad, untouched) == (0, 12345, False) and n_rej == k  # random words prove nothing: all rejected, no error
            assert raw(dev, kk=0) == (0, 12345, 0, True)
            assert raw(dev, kk=4097) == (E.INVALID_ARGUMENT, 12345, 999, True)
            assert raw(dev, flags=2) == (E.INVALID_ARGUMENT, 12345, 999, True)
            assert raw(dev, rejected=False) == (E.INVALID_ARGUMENT, 12345, 999, True)
            assert raw(dev, with_taus=False) == (E.INVALID_ARGUMENT, 1, 999, True)
            assert raw(dev, dg=[1, 3, 4, 3]) == (E.INVALID_ARGUMENT, 2, 999, True)
            assert raw(dev, kd=[0, 1, 0, 0, 0, 2, 1, 0, 0]) == (E.INVALID_ARGUMENT, 2, 999, True)
            assert raw(dev, null=8) == (E.INVALID_ARGUMENT, 3, 999, True)
            assert raw(dev, nn=[4, 8, 1, 16]) == (E.NO_VARIABLES, 2, 999, True)
            assert raw(dev, nn=[4, 6, 2, 16]) == (E.LENGTH_NOT_POWER_OF_TWO, 1, 999, True)
            assert raw(dev, nn=[4, 8, 2, 1 << 33]) == (E.INVALID_ARGUMENT, 3, 999, True)
            for name, idx, proof in (("rounds", 4 + 12 + 1, 2), ("points", 9, 3), ("fev", 1, 1), ("taus", 3, 3), ("cs", 0, 0), ("fe", 3, 3)):
                assert raw(dev, edit=(name, idx)) == (E.NOT_CANONICAL, proof, 999, True), name
            # a word >= p in proof 1 in front of proof 3's bad length
            assert raw(dev, nn=[4, 8, 2, 12], edit=("rounds", 5)) == (E.NOT_CANONICAL, 1, 999, True)
        assert raw(True, shift=4) == (E.INVALID_ARGUMENT, 2, 999, True)
        # host tables: a value >= p is the proof's error, also in front of a later shape error
        host[2][1] = P
        assert raw(False) == (E.NOT_CANONICAL, 1, 999, True)
        assert raw(False, nn=[4, 8, 2, 12]) == (E.NOT_CANONICAL, 1, 999, True)
        host[2][1] = 5
    finally:
        dv.free()


def test_table_factors_of_2_pow_24_chunks_are_refused(ctx):
    """11 proofs of three 2^32-word table factors make 33 * 2^19 chunks, more than one launch's grid: ZIGZ_ERR_INVALID_ARGUMENT
    before anything is read, launched or written (no table of that size exists: the pointers are never followed)"""
    from zigz_amd._ffi import lib, u8p, u64p, vp
    k, d, v = 11, 3, 32
    small = np.zeros(4, dtype=np.uint64)
    base = ctx.dev_alloc(64)
    words = np.zeros(k * (d + 1) * v, dtype=np.uint64)
    p = lambda a: a.ctypes.data_as(u64p)
    try:
        for dev in (True, False):
            verd = np.full(k, 7, dtype=np.uint8)
            out = np.full(k + k * d, 0xABCDEF, dtype=np.uint64)
            n_rej, bad = C.c_size_t(999), C.c_size_t(12345)
            ptrs = (vp * (k * d))(*[base] * (k * d)) if dev else (u64p * (k * d))(*[p(small)] * (k * d))
            fn = lib.zigz_dev_sumcheck_verify_product_batch if dev else lib.zigz_sumcheck_verify_product_batch
            rc = fn(ctx.h, k, (C.c_uint * k)(*[d] * k), ptrs, None, None, (C.c_size_t * k)(*[1 << v] * k), p(words), p(words), p(words),
                    p(words), p(words), 0, verd.ctypes.data_as(u8p), p(out), p(out[k:]), C.byref(n_rej), C.byref(bad))
            assert (rc, bad.value, n_rej.value) == (E.INVALID_ARGUMENT, 12345, 999)
            assert np.all(verd == 7) and np.all(out == 0xABCDEF)
    finally:
        ctx.dev_free(base)
