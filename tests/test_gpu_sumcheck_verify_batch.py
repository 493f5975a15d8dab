"""Batched sumcheck verification on the GPU (zigz_dev_sumcheck_verify_batch, zigz_sumcheck_verify_batch): verdicts, expected
evals and oracle evals of honest and tampered proofs equal SumcheckVerifier.verify as the oracle restates it -- under the
reference's point order (flags = 0: honest proofs of two or more variables are rejected in general) and with
POINT_REVERSED (honest proofs accept) -- and nothing else on the context is disturbed."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as O
import sumcheck_verify_ref as R

pytestmark = pytest.mark.gpu

P = O.P_BB
E = None
REV = 1  # ZIGZ_SUMCHECK_VERIFY_POINT_REVERSED


@pytest.fixture(scope="module")
def ctx():
    import zigz_amd
    global E
    from zigz_amd import errors, hip
    E = errors
    assert hip.SUMCHECK_VERIFY_POINT_REVERSED == REV
    c = zigz_amd.Context(0)
    yield c


class DevTables:
    """seeded tables uploaded into one device buffer, each 16-byte aligned (offsets in u32 words: multiples of 4)"""

    def __init__(self, ctx, tables, extra_offset=0):
        self.ctx = ctx
        self.off, o = [], extra_offset
        for t in tables:
            self.off.append(o)
            o += (len(t) + 3) // 4 * 4
        packed = np.zeros(max(o, 4), dtype=np.uint64)
        for t, a in zip(tables, self.off):
            packed[a:a + len(t)] = t
        self.base = ctx.dev_alloc(len(packed) * 4)
        ctx.upload(packed, self.base)
        self.ptrs = [self.base + 4 * a for a in self.off]

    def free(self):
        self.ctx.dev_free(self.base)


@pytest.fixture(scope="module")
def batch(ctx):
    """proofs of a mixed batch (n = 2 .. 2^17, one constant table) from the batched prover, honest and tampered, with the
    reference verdicts under both point orders (computed once)"""
    ns = [2, 2, 4, 8, 64, 1 << 10, 1 << 13, 1 << 15, 1 << 17, 256]
    tables = [O.splitmix64_field(51000 + i, n) for i, n in enumerate(ns)]
    tables[-1] = np.full(256, 424242, dtype=np.uint64)
    d = DevTables(ctx, tables)
    proved = ctx.dev_sumcheck_prove_batch(d.ptrs, ns)
    items = []  # (table index, kind, claimed, rounds, point, final_eval)
    for i, (rounds, point, fe) in enumerate(proved):
        assert O.sumcheck_to_bytes(rounds, point, fe) == O.sumcheck_to_bytes(*O.sumcheck_prove(P, tables[i]))
        for kind, c, r, q, f in R.tampered(O.mle_sum(P, tables[i]), rounds, point, fe):
            items.append((i, kind, c, r, q, f))
    ref = {rev: [R.verdict(tables[i], c, r, q, f, reversed_point=rev) for i, _, c, r, q, f in items] for rev in (False, True)}
    yield ns, tables, d, items, ref
    d.free()


def _call(ctx, d, ns, items, flags):
    return ctx.dev_sumcheck_verify_batch([d.ptrs[i] for i, *_ in items], [ns[i] for i, *_ in items], [c for _, _, c, *_ in items],
                                         [(r, q, f) for *_, r, q, f in items], flags)


def test_reference_point_order(ctx, batch):
    ns, tables, d, items, ref = batch
    verd, exp, orc, rej = _call(ctx, d, ns, items, 0)
    for j, (i, kind, c, r, q, f) in enumerate(items):
        ok, expected, ev = ref[False][j]
        assert (bool(verd[j]), exp[j], orc[j]) == (ok, expected, ev), (ns[i], kind)
        assert ok == O.sumcheck_verify(P, tables[i], c, r, q, f), (ns[i], kind)
    assert rej == len(items) - int(verd.sum())
    # one variable and the constant table accept; honest seeded proofs of two or more variables do not
    honest = [bool(verd[j]) for j, it in enumerate(items) if it[1] == "honest"]
    assert True in honest and False in honest


def test_point_reversed(ctx, batch):
    ns, tables, d, items, ref = batch
    verd, exp, orc, rej = _call(ctx, d, ns, items, REV)
    for j, (i, kind, c, r, q, f) in enumerate(items):
        ok, expected, ev = ref[True][j]
        assert (bool(verd[j]), exp[j], orc[j]) == (ok, expected, ev), (ns[i], kind)
        if kind == "honest":
            assert verd[j] == 1, ns[i]
        elif not (i == len(ns) - 1 and kind == "point"):  # (a constant's extension is that constant at every point)
            assert verd[j] == 0, (ns[i], kind)
        if kind == "claimed_sum":  # rejected at round 0: the expected eval is the tampered sum itself
            assert exp[j] == c and verd[j] == 0
    assert rej == len(items) - int(verd.sum())


def test_host_form_and_null_outputs(ctx, batch):
    ns, tables, d, items, ref = batch
    sel = [it for it in items if ns[it[0]] <= 1 << 13]
    want = [ref[True][j] for j, it in enumerate(items) if ns[it[0]] <= 1 << 13]
    verd, exp, orc, rej = ctx.sumcheck_verify_batch([tables[i] for i, *_ in sel], [c for _, _, c, *_ in sel],
                                                    [(r, q, f) for *_, r, q, f in sel], REV)
    assert [(bool(v), e, o) for v, e, o in zip(verd, exp, orc)] == want
    assert rej == sum(1 for w in want if not w[0])
    # verdicts, expected_evals and oracle_evals may be NULL: the count alone
    from zigz_amd._ffi import lib, u64p, vp
    k = len(items)
    cat = lambda xs: np.ascontiguousarray(np.concatenate([np.asarray(x, dtype=np.uint64).reshape(-1) for x in xs]))
    cs, rr, qq, ff = cat([[c] for _, _, c, *_ in items]), cat([r for *_, r, _, _ in items]), cat([q for *_, q, _ in items]), \
        cat([[f] for *_, f in items])
    n_rej = C.c_size_t(999)
    rc = lib.zigz_dev_sumcheck_verify_batch(ctx.h, (vp * k)(*[d.ptrs[i] for i, *_ in items]), (C.c_size_t * k)(*[ns[i] for i, *_ in items]),
                                            k, cs.ctypes.data_as(u64p), rr.ctypes.data_as(u64p), qq.ctypes.data_as(u64p),
                                            ff.ctypes.data_as(u64p), REV, None, None, None, C.byref(n_rej), None)
    assert rc == 0 and n_rej.value == sum(1 for w in ref[True] if not w[0])


def test_large_table(ctx):
    n = 1 << 20
    t = O.splitmix64_field(52000, n)
    d = DevTables(ctx, [t])
    try:
        (rounds, point, fe), = ctx.dev_sumcheck_prove_batch(d.ptrs, [n])
        s = O.mle_sum(P, t)
        verd, exp, orc, rej = ctx.dev_sumcheck_verify_batch(d.ptrs * 2, [n, n], [s, s], [(rounds, point, fe), (rounds, point, (fe + 1) % P)], REV)
        assert verd.tolist() == [1, 0] and rej == 1
        assert exp == [fe, fe] and orc == [fe, fe]
        assert orc[0] == ctx.dev_mle_eval(d.ptrs[0], n, [int(x) for x in point][::-1])
    finally:
        d.free()


def test_inside_a_commit_job(ctx, batch):
    """the batch verified between zigz_commit_begin_dev and zigz_commit_roots: the job's roots are those of a job run alone,
    and the statistics and options are as they were"""
    import zigz_amd
    ns, tables, d, items, ref = batch
    nv, ncols = 10, 4
    cols = O.splitmix64_field(53000, ncols << nv)
    dc = DevTables(ctx, [cols])
    opts = ("run_aware_mask", "cons_group_mask", "small_domain_mask", "per_round_sumcheck", "fold_eval")
    try:
        job = zigz_amd.CommitJob(ctx, d_cols=dc.ptrs[0], ncols=ncols, nv=nv)
        alone = job.roots().copy()
        job.end()
        job = zigz_amd.CommitJob(ctx, d_cols=dc.ptrs[0], ncols=ncols, nv=nv)
        stats, options = ctx.stats(), [ctx.get_option(o) for o in opts]
        verd, exp, orc, rej = _call(ctx, d, ns, items, REV)
        assert ctx.stats() == stats and [ctx.get_option(o) for o in opts] == options
        roots = job.roots()
        job.end()
        assert np.array_equal(roots, alone)
        assert [(bool(v), e, o) for v, e, o in zip(verd, exp, orc)] == ref[True]
    finally:
        dc.free()


def test_empty_and_error_cases(ctx, batch):
    ns, tables, d, items, ref = batch
    verd, exp, orc, rej = ctx.dev_sumcheck_verify_batch([], [], [], [], 0)
    assert len(verd) == 0 and exp == [] and orc == [] and rej == 0
    from zigz_amd._ffi import lib, u8p, u64p, vp
    sel = items[:4]
    k = len(sel)
    cat = lambda xs: np.ascontiguousarray(np.concatenate([np.asarray(x, dtype=np.uint64).reshape(-1) for x in xs]))
    cs, rr, qq, ff = cat([[c] for _, _, c, *_ in sel]), cat([r for *_, r, _, _ in sel]), cat([q for *_, q, _ in sel]), \
        cat([[f] for *_, f in sel])

    def raw(nn, flags=0):
        verd = np.full(k, 7, dtype=np.uint8)
        out = np.full(2 * k, 0xABCDEF, dtype=np.uint64)
        n_rej, bad = C.c_size_t(999), C.c_size_t(12345)
        rc = lib.zigz_dev_sumcheck_verify_batch(ctx.h, (vp * k)(*[d.ptrs[i] for i, *_ in sel]), (C.c_size_t * k)(*nn), k,
                                                cs.ctypes.data_as(u64p), rr.ctypes.data_as(u64p), qq.ctypes.data_as(u64p),
                                                ff.ctypes.data_as(u64p), flags, verd.ctypes.data_as(u8p), out.ctypes.data_as(u64p),
                                                out[k:].ctypes.data_as(u64p), C.byref(n_rej), C.byref(bad))
        return rc, bad.value, n_rej.value, bool(np.all(verd == 7) and np.all(out == 0xABCDEF))

    good = [ns[i] for i, *_ in sel]
    rc, bad, n_rej, untouched = raw(good)
    assert rc == 0 and bad == 12345 and not untouched and n_rej == sum(1 for w in ref[False][:4] if not w[0])
    for nn, code, idx in [([good[0], good[1], 1, good[3]], E.NO_VARIABLES, 2), ([good[0], 3, good[2], good[3]], E.LENGTH_NOT_POWER_OF_TWO, 1)]:
        assert raw(nn) == (code, idx, 999, True)
    assert raw(good, flags=2) == (E.INVALID_ARGUMENT, 12345, 999, True)
    rr[3] = P  # a round coefficient >= p: proof 1 (the first proof has one variable, two words)
    assert raw(good) == (E.NOT_CANONICAL, 1, 999, True)
